"""Float64 restatement of torchaudio's default resampler (torchaudio.functional.resample: Hann-windowed sinc, polyphase,
lowpass_filter_width 6, rolloff 0.99) and of the reference's Pad (util/audio_transforms.py:19-27), for the tests of
csrc/data/resample.hip.  Written from the published algorithm with loops over the definition, not from the package's table code:

    g = gcd(orig, new); o = orig / g; n = new / g; base = min(o, n) rolloff; width = ceil(lpw o / base)
    idx[k] = (k - width) / o,  k = 0 .. 2 width + o - 1
    t[p, k] = clamp((-p / n + idx[k]) base, -lpw, lpw)
    taps[p, k] = sinc(t) cos^2(t pi / lpw / 2) base / o
    y[f n + p] = sum_k taps[p, k] xpad[f o + k],  xpad = width zeros, x, width + o zeros;  the first ceil(n L / o) samples kept."""
import math

import numpy as np


def geometry(orig, new, lpw=6, rolloff=0.99):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    width = int(math.ceil(lpw * o / (min(o, n) * rolloff)))
    return o, n, width, 2 * width + o


def taps64(orig, new, lpw=6, rolloff=0.99):
    o, n, width, K = geometry(orig, new, lpw, rolloff)
    base = min(o, n) * rolloff
    out = np.empty((n, K), np.float64)
    for p in range(n):
        for k in range(K):
            t = min(max((-p / n + (k - width) / o) * base, -lpw), lpw)
            window = math.cos(t * math.pi / lpw / 2) ** 2
            t *= math.pi
            out[p, k] = (1.0 if t == 0 else math.sin(t) / t) * window * (base / o)
    return out


def frames_of(x, o, width, K):
    """[.., L] -> the windows xpad[f o : f o + K] of every frame f, [.., F, K] (float64), F = L // o + 1 as the strided
    convolution over the padded signal gives"""
    x = np.asarray(x, np.float64)
    L = x.shape[-1]
    xpad = np.concatenate([np.zeros(x.shape[:-1] + (width,)), x, np.zeros(x.shape[:-1] + (width + o,))], -1)
    F = (L + 2 * width + o - K) // o + 1
    idx = np.arange(F)[:, None] * o + np.arange(K)[None, :]
    return xpad[..., idx]


def resample(x, taps, o, n, width, return_abs=False):
    """x [.., L] -> y [.., ceil(n L / o)] in float64 with the given table [n, K] (the float64 one above, or a kernel's fp32 table
    widened); with ``return_abs`` also sum_k |taps x| per output, the scale of the rounding bound."""
    taps = np.asarray(taps, np.float64)
    K = taps.shape[1]
    assert taps.shape == (n, K) and K == 2 * width + o
    fr = frames_of(x, o, width, K)                                # [.., F, K]
    L = np.asarray(x).shape[-1]
    R = -(-n * L // o)
    y = np.einsum('...fk,pk->...fp', fr, taps).reshape(fr.shape[:-2] + (-1,))[..., :R]
    if not return_abs:
        return y
    a = np.einsum('...fk,pk->...fp', np.abs(fr), np.abs(taps)).reshape(fr.shape[:-2] + (-1,))[..., :R]
    return y, a


def resample_rates(x, orig, new):
    if int(orig) == int(new):
        return np.asarray(x, np.float64)
    o, n, width, _ = geometry(orig, new)
    return resample(x, taps64(orig, new), o, n, width)


def pad_loop(x, samples):
    """the reference's Pad, literally: append the flipped signal until long enough, then cut"""
    x = np.asarray(x)
    while x.shape[-1] < samples:
        x = np.concatenate([x, x[..., ::-1]], -1)
    return x[..., :samples]


def mirror_map(R, out_len):
    """m(j) of include/dav_kernels.h: the source index of output j under Pad"""
    j = np.arange(out_len) % (2 * R)
    return np.where(j < R, j, 2 * R - 1 - j)
