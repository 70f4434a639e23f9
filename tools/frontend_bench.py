#!/usr/bin/env python3
"""Times the device-side input stage: TrainFrameTransform (csrc/data/frames.hip) against the stock PyTorch-ROCm restatement on the
same device and frames — per sample (the boxes differ) crop, F.interpolate(mode='bilinear', antialias=True), flip, normalise —
alternating in one process, and the audio front-end (Pad -> RandomVol -> LogMelSpectrogram) beside it.

    python tools/frontend_bench.py [--reps 30] [--rounds 5] [--bench-ms MS_PER_STEP] [--out profiles/frontend_bench.json]

Device-event medians after warm-up.  The parameter rows are drawn once and uploaded outside the timed region for the kernel figure
(`kernel_ms`); `module_ms` is the whole module call (host draws + upload + launch).  Bytes = frames read + fp32 written (the
algorithmic minimum: every source byte once); the achievable HBM rate on an MI355X is about 6.3 TB/s.  --bench-ms takes
ms_per_step of a plain `python bench.py` on the same box and reports the front-ends' share of it."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_TBS = 6.3


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def torch_restatement(frames, rows, size, mean, std):
    out = torch.empty(frames.shape[0], 3, size, size, device=frames.device)
    for b, (i, j, h, w, RH, RW, top, left, flip) in enumerate(rows):
        x = frames[b, i:i + h, j:j + w].permute(2, 0, 1)[None].float()
        y = F.interpolate(x, size=(RH, RW), mode='bilinear', antialias=True, align_corners=False)[0, :, top:top + size, left:left + size]
        if flip:
            y = y.flip(-1)
        out[b] = (y / 255.0 - mean) / std
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--hw', type=int, nargs=2, default=(256, 340))
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--bench-ms', type=float, default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from deepavfusion_amd import ops
    from deepavfusion_amd.util import audio_transforms as aT
    from deepavfusion_amd.util.frame_transforms import IMAGENET_MEAN, IMAGENET_STD, TrainFrameTransform
    dev = torch.device('cuda')
    B, (H, W), S = a.batch, a.hw, a.size
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    tf = TrainFrameTransform(S, scale=(0.5, 1.0), seed=0)
    got = tf(frames)
    rows = tf.last_rows.tolist()
    params = tf.last_rows.to(dev)
    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).view(3, 1, 1)
    ref = torch_restatement(frames, rows, S, mean, std)
    max_diff = float((got - ref).abs().max())
    out = torch.empty(B, 3, S, S, device=dev)
    kernel = lambda: ops.frame_transform(frames, params, S, IMAGENET_MEAN, IMAGENET_STD, out=out)
    module = lambda: tf(frames)
    torch_fn = lambda: torch_restatement(frames, rows, S, mean, std)
    wave = (torch.randn(B, 160000, generator=g) * 0.1).clamp(-1, 1).to(dev)
    audio = aT.Compose([aT.Pad(10.0, 16000), aT.RandomVol(per_sample=True), aT.LogMelSpectrogram(16000, 128).to(dev)])
    audio_fn = lambda: audio(wave)
    fns = {'kernel_ms': kernel, 'module_ms': module, 'torch_ms': torch_fn, 'audio_ms': audio_fn}
    for fn in fns.values():                                     # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in fns}
    for _ in range(a.rounds):                                   # alternate the legs: other work shares the box
        for k, fn in fns.items():
            per_round[k].append(_median_ms(fn, a.reps if k != 'torch_ms' else max(5, a.reps // 3)))
    med = {k: sorted(v)[len(v) // 2] for k, v in per_round.items()}
    nbytes = frames.numel() + out.numel() * 4
    p = torch.cuda.get_device_properties(0)
    row = {'what': 'frontend', 'B': B, 'frame_hw': [H, W], 'size': S, 'scale': [0.5, 1.0], 'reps': a.reps, 'rounds': a.rounds,
           **{k: round(v, 4) for k, v in med.items()},
           'rounds_ms': {k: [round(x, 4) for x in v] for k, v in per_round.items()},
           'torch_over_kernel': round(med['torch_ms'] / med['kernel_ms'], 1),
           'torch_over_module': round(med['torch_ms'] / med['module_ms'], 1),
           'bytes': nbytes, 'kernel_gbs': round(nbytes / med['kernel_ms'] / 1e6, 1), 'hbm_achievable_gbs': HBM_ACHIEVABLE_TBS * 1e3,
           'max_abs_diff_vs_torch': max_diff, 'frontends_ms': round(med['module_ms'] + med['audio_ms'], 4),
           'device': p.name, 'date': time.strftime('%Y-%m-%d')}
    if a.bench_ms:
        row['bench_ms_per_step'] = a.bench_ms
        row['frontends_share_of_step'] = round(row['frontends_ms'] / a.bench_ms, 4)
    print(json.dumps(row))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'rows': [row], 'measured_on': f'{p.name} {getattr(p, "gcnArchName", "")}'.strip(),
                       'command': 'python tools/frontend_bench.py ' + ' '.join(sys.argv[1:])}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
