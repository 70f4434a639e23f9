"""Writes tests/golden/frame_transform.npz: small uint8 sources, parameter rows of the frame transform and what PIL makes of them.

    python tests/golden/gen_frame_golden.py

Needs PIL (the tests that read the fixture do not).  Train form: Image.crop(box).resize((S, S), BILINEAR) [+ FLIP_LEFT_RIGHT];
eval form: Image.resize((RW, RH), BILINEAR).crop(window).  Every case is checked here against the float64 restatement
(tests/frame_ref.py) at 1 + 5e-3 grey levels before it is written: PIL rounds to uint8 after the horizontal and after the
vertical pass (<= 0.5 each, the vertical weights sum to 1) and keeps its coefficients in 22-bit fixed point (a few 1e-4 levels
per pass).  Keys: src<k> uint8 [H, W, 3]; rows int32 [n, 9] (i, j, h, w, RH, RW, top, left, flip); src_of int32 [n];
size int32 [n]; pil<n> uint8 [S, S, 3]."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frame_ref as R  # noqa: E402

BOUND = 1.0 + 5e-3

SOURCES = [('noise', 96, 128, 11), ('smooth', 96, 128, 12), ('noise', 80, 56, 13), ('smooth', 64, 96, 14)]
# (source, i, j, h, w, RH, RW, top, left, flip, S)
CASES = [
    (0, 10, 20, 70, 90, 32, 32, 0, 0, 0, 32),        # downscale, both axes
    (0, 0, 0, 96, 128, 48, 48, 0, 0, 1, 48),         # the whole frame, flipped
    (0, 30, 40, 20, 24, 64, 64, 0, 0, 0, 64),        # upscale
    (0, 5, 7, 90, 1, 16, 16, 0, 0, 0, 16),           # a 1-pixel-wide box
    (1, 3, 50, 81, 61, 64, 64, 0, 0, 1, 64),
    (1, 0, 0, 96, 128, 73, 97, 4, 8, 0, 64),         # eval form: resize the whole frame, cut a window
    (2, 0, 0, 80, 56, 52, 36, 10, 2, 0, 32),         # eval form, portrait
    (2, 11, 3, 33, 50, 48, 48, 0, 0, 0, 48),         # down in x, up in y
    (3, 0, 0, 64, 96, 18, 27, 1, 5, 0, 16),          # eval form, strong downscale (support 3.6)
    (3, 7, 9, 50, 80, 16, 16, 0, 0, 1, 16),
]


def pil_case(src, row, S):
    i, j, h, w, RH, RW, top, left, flip = row
    im = Image.fromarray(src).crop((j, i, j + w, i + h)).resize((RW, RH), Image.BILINEAR)
    im = im.crop((left, top, left + S, top + S))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def main():
    out = {}
    srcs = []
    for k, (kind, H, W, seed) in enumerate(SOURCES):
        srcs.append(R.noise_frame(H, W, seed) if kind == 'noise' else R.smooth_frame(H, W, seed))
        out[f'src{k}'] = srcs[-1]
    rows, src_of, size = [], [], []
    for n, c in enumerate(CASES):
        k, row, S = c[0], list(c[1:10]), c[10]
        pil = pil_case(srcs[k], row, S)
        assert pil.shape == (S, S, 3) and pil.dtype == np.uint8
        i, j, h, w, RH, RW, top, left, flip = row
        ref = R.resample(srcs[k], (i, j, h, w), (RH, RW))[top:top + S, left:left + S]
        ref = ref[:, ::-1] if flip else ref
        worst = float(np.abs(ref - pil).max())
        print(f'case {n}: worst |rule - PIL| = {worst:.4f} grey levels')
        assert worst <= BOUND, (n, worst)
        out[f'pil{n}'] = pil
        rows.append(row)
        src_of.append(k)
        size.append(S)
    out.update(rows=np.asarray(rows, np.int32), src_of=np.asarray(src_of, np.int32), size=np.asarray(size, np.int32))
    path = os.path.join(HERE, 'frame_transform.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
