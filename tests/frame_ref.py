"""Float64 restatement of the frame transform (dav_frame_transform_u8, include/dav_kernels.h) the frame front-end tests compare
against: numpy only, device-free.

Per axis, n_in source pixels -> n_out outputs: scale = n_in / n_out, support = max(scale, 1); output o has centre
c = (o + 0.5) scale, taps k in [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)), weights
max(0, 1 - |k - c + 0.5| / max(scale, 1)) divided by their sum — the antialiased bilinear (triangle) filter of PIL's
Image.resize(BILINEAR) and of F.interpolate(mode='bilinear', antialias=True, align_corners=False)
(tests/test_frame_frontend_host.py holds it to both)."""
import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def axis_weights(n_in, n_out):
    """[n_out, n_in] float64 resampling matrix of one axis."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    M = np.zeros((n_out, n_in), np.float64)
    for o in range(n_out):
        c = (o + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        k = np.arange(lo, hi)
        w = np.maximum(0.0, 1.0 - np.abs(k - c + 0.5) / max(scale, 1.0))
        M[o, lo:hi] = w / w.sum()
    return M


def resample(frame, box, out_hw):
    """frame [H, W, C] (any real dtype), box (i, j, h, w) -> float64 [RH, RW, C] in the frame's units: crop FIRST, then resize
    (pixels outside the box never contribute), no rounding anywhere."""
    i, j, h, w = box
    x = np.asarray(frame[i:i + h, j:j + w], np.float64)
    My, Mx = axis_weights(h, out_hw[0]), axis_weights(w, out_hw[1])
    return np.einsum('oy,yxc->oxc', My, np.einsum('px,yxc->ypc', Mx, x))


def transform(frame, row, size, mean=MEAN, std=STD):
    """One sample: uint8 [H, W, 3] and its parameter row [i, j, h, w, RH, RW, top, left, flip] -> float64 [3, size, size]."""
    i, j, h, w, RH, RW, top, left, flip = (int(v) for v in row)
    v = resample(frame, (i, j, h, w), (RH, RW))[top:top + size, left:left + size]
    if flip:
        v = v[:, ::-1]
    v = (v / 255.0 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def transform_batch(frames, rows, size, mean=MEAN, std=STD):
    return np.stack([transform(f, r, size, mean, std) for f, r in zip(np.asarray(frames), np.asarray(rows))])


def smooth_frame(H, W, seed):
    """A smooth uint8 test picture (sums of low-frequency waves), next to plain noise the other kind of source in the tests."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = g.uniform(0.5, 4) / H, g.uniform(0.5, 4) / W, g.uniform(0, 2 * np.pi)
            out[..., c] += np.sin(2 * np.pi * (fy * y + fx * x) + ph)
    return np.clip(np.rint(127.5 + 127.5 * out / 4 * 1.6), 0, 255).astype(np.uint8)


def noise_frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
