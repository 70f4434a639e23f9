#!/usr/bin/env python3
"""Times the device-side audio resampler: PrepareWaveform (csrc/data/resample.hip: Resample -> Pad -> RandomVol in one launch)
against the stock PyTorch-ROCm restatement on the same device and waveforms — F.pad + F.conv1d(stride=o) with the same taps, the
cut to ceil(n L / o), then the torch Pad / RandomVol modules — alternating in one process.

    python tools/resample_bench.py [--reps 30] [--rounds 5] [--batch 64] [--seconds 10] [--out profiles/resample_bench.json]

Device-event medians after warm-up, for 44100 -> 16000 and 48000 -> 16000 with fp32 and int16 input (the restatement gets the
int16 input too and scales it first, as the loader would have).  The gains are drawn once and uploaded outside the timed region
for the kernel figure (`kernel_ms`); `module_ms` is the whole module call (host draws + upload + launch).  The kernel's bound
is the larger of 2 taps outputs FLOP over the fp32 vector peak (157.3 TFLOP/s) and (input + output) bytes over the achievable
HBM rate (about 6.3 TB/s on an MI355X); the row says which one binds and the kernel's share of it."""
import argparse
import json
import os
import random
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_TBS = 6.3
FP32_VECTOR_TFLOPS = 157.3


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


def torch_restatement(wave, taps, o, width, out_r, pad, vol):
    """torchaudio's _apply_sinc_resample_kernel with stock ops, then the package's torch Pad and RandomVol"""
    x = wave.float() / 32768.0 if wave.dtype == torch.int16 else wave
    y = F.conv1d(F.pad(x[:, None], (width, width + o)), taps[:, None], stride=o)          # [B, n, frames]
    y = y.transpose(1, 2).reshape(x.shape[0], -1)[:, :out_r]
    return vol(pad(y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from deepavfusion_amd import ops
    from deepavfusion_amd.util import audio_transforms as aT
    dev = torch.device('cuda')
    B, new = a.batch, 16000
    g = torch.Generator().manual_seed(0)
    rows = []
    for orig in (44100, 48000):
        L = int(a.seconds * orig)
        mod = aT.PrepareWaveform(orig, new, a.seconds).to(dev)
        pad, vol = aT.Pad(a.seconds, new), aT.RandomVol(per_sample=True)
        f32 = (torch.randn(B, L, generator=g) * 0.1).clamp(-1, 1)
        waves = {'fp32': f32.to(dev), 'int16': (f32 * 32767).to(torch.int16).to(dev)}
        gain = torch.pow(10.0, torch.empty(B).uniform_(-6, 6, generator=g).to(dev) / 20.0)
        out = torch.empty(B, mod.samples, device=dev)
        out_r = mod.out_samples(L)
        fns, diffs = {}, {}
        for name, w in waves.items():
            fns[f'kernel_{name}_ms'] = lambda w=w: ops.wave_resample(w, mod.taps_kn, mod.o, mod.n, mod.width, out_len=mod.samples,
                                                                      gain=gain, clamp=True, out=out)
            fns[f'module_{name}_ms'] = lambda w=w: mod(w)
            fns[f'torch_{name}_ms'] = lambda w=w: torch_restatement(w, mod.taps, mod.o, mod.width, out_r, pad, vol)
            random.seed(0)
            got = mod(w)
            random.seed(0)
            diffs[name] = float((got - torch_restatement(w, mod.taps, mod.o, mod.width, out_r, pad, vol)).abs().max())
        for fn in fns.values():                                     # warm-up: code objects, allocator, the convolution's solver
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        per_round = {k: [] for k in fns}
        for _ in range(a.rounds):                                   # alternate the legs: other work shares the box
            for k, fn in fns.items():
                per_round[k].append(_median_ms(fn, a.reps if not k.startswith('torch') else max(5, a.reps // 3)))
        med = {k: sorted(v)[len(v) // 2] for k, v in per_round.items()}
        outputs = B * min(out_r, mod.samples)                       # resampled values actually computed
        flop = 2.0 * mod.ntaps * outputs
        flop_ms = flop / (FP32_VECTOR_TFLOPS * 1e9)
        row = {'what': 'resample', 'orig_freq': orig, 'new_freq': new, 'o': mod.o, 'n': mod.n, 'taps': mod.ntaps,
               'frames_per_workgroup': aT.resample_tile(orig, new), 'B': B, 'seconds': a.seconds, 'in_samples': L,
               'out_samples': mod.samples, 'reps': a.reps, 'rounds': a.rounds, **{k: round(v, 4) for k, v in med.items()},
               'rounds_ms': {k: [round(x, 4) for x in v] for k, v in per_round.items()}, 'flop': flop,
               'max_abs_diff_vs_torch': diffs}
        for name, w in waves.items():
            nbytes = w.numel() * w.element_size() + out.numel() * 4
            bytes_ms = nbytes / (HBM_ACHIEVABLE_TBS * 1e9)
            bound_ms = max(flop_ms, bytes_ms)
            k_ms, t_ms = med[f'kernel_{name}_ms'], med[f'torch_{name}_ms']
            row[name] = {'bytes': nbytes, 'flop_bound_ms': round(flop_ms, 5), 'bytes_bound_ms': round(bytes_ms, 5),
                         'binds': 'fp32 vector peak' if flop_ms >= bytes_ms else 'HBM bandwidth',
                         'kernel_share_of_bound': round(bound_ms / k_ms, 4), 'kernel_tflops': round(flop / k_ms / 1e9, 2),
                         'torch_over_kernel': round(t_ms / k_ms, 2), 'torch_over_module': round(t_ms / med[f'module_{name}_ms'], 2),
                         'kernel_not_slower_than_torch': bool(k_ms <= t_ms)}
        rows.append(row)
        print(json.dumps(row))
    p = torch.cuda.get_device_properties(0)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'rows': rows, 'fp32_vector_peak_tflops': FP32_VECTOR_TFLOPS, 'hbm_achievable_gbs': HBM_ACHIEVABLE_TBS * 1e3,
                       'measured_on': f'{p.name} {getattr(p, "gcnArchName", "")}'.strip(), 'date': time.strftime('%Y-%m-%d'),
                       'command': 'python tools/resample_bench.py ' + ' '.join(sys.argv[1:])}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
