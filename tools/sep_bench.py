#!/usr/bin/env python3
"""Times the fused source-separation audio call — SpectrogramMasking on dav_sep_mask_istft (csrc/sep/stft.hip: STFT -> sigmoid ->
mel mask -> product -> inverse STFT in one launch) — against two baselines on the same waveforms and masks, alternating in one
process:

  torch_device   a stock PyTorch-ROCm restatement on the device: torch.stft -> sigmoid / cat / einsum -> torch.istft, batched
                 over B and K (what one would write without the kernel);
  host_reference the reference's path (eval_avsrcsep.py:245-254, :272-277): per sample and per source, the mask copied to the
                 host, sigmoid / cat / einsum and torch.stft / torch.istft on the CPU (waveforms already on the host, as the
                 reference's loader leaves them).

    python tools/sep_bench.py [--reps 20] [--rounds 5] [--batch 32] [--masks 2] [--seconds 3] [--out profiles/sep_bench.json]

Shape: B = 32 mixtures, K = 2 masks, 48000 samples at 16 kHz (the reference's 3 s evaluation clip).  Device legs: device-event
medians per round after warm-up, the median over the rounds and their spread (min .. max); the host leg: a host clock around the
loop, which ends in host tensors.  The kernel's work is counted from the shapes: a direct real DFT with the bin-pair symmetry
takes 4 fmaf per (thread, two samples or bins): 8 (n_fft / 2) (n_fft / 4 + 1) FLOP per transformed frame, (1 + K) transforms per
frame, 12 frames held per 9 hops of output; the share of the fp32 vector peak is of the packed-FMA figure (157.3 TFLOP/s)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def torch_device(wave, logits, fb, window, n_fft, hop):
    """wave [B, S], logits [B, K, n_mels, T] on the device -> [B, K, L] with stock ops"""
    B, K = logits.shape[:2]
    X = torch.stft(wave, n_fft, hop_length=hop, window=window, center=True, pad_mode='reflect', normalized=False, onesided=True,
                   return_complex=True)
    m = torch.cat((torch.sigmoid(logits), torch.zeros(B, K, logits.shape[2], 1, device=logits.device)), dim=3)
    m = torch.einsum('bkmt,fm->bkft', m, fb)
    Y = (m * X[:, None]).reshape(B * K, *X.shape[1:])
    return torch.istft(Y, n_fft, hop_length=hop, window=window, center=True, normalized=False, onesided=True).view(B, K, -1)


def host_reference(wave_cpu, logits, fb_cpu, window_cpu, n_fft, hop):
    """the reference's loop: per sample, per source; the mask comes off the device inside the call"""
    outs = []
    for i in range(wave_cpu.shape[0]):
        for k in range(logits.shape[1]):
            stft_mix = torch.stft(wave_cpu[i:i + 1], n_fft, hop_length=hop, window=window_cpu, center=True, pad_mode='reflect',
                                  normalized=False, onesided=True, return_complex=True)
            pm = logits[i:i + 1, k]
            pm = torch.cat((torch.sigmoid(pm).detach().cpu(), torch.zeros(*pm.shape[:2], 1)), dim=2)
            pm = torch.einsum('bmt,fm->bft', pm, fb_cpu)
            outs.append(torch.istft(pm * stft_mix, n_fft, hop_length=hop, window=window_cpu, center=True, normalized=False, onesided=True))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--masks', type=int, default=2)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--rate', type=int, default=16000)
    ap.add_argument('--mels', type=int, default=128)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sep_bench measures on an MI355X; no device found')
    from deepavfusion_amd import ops
    from deepavfusion_amd.util.separation import SpectrogramMasking
    dev = torch.device('cuda')
    B, K, S = a.batch, a.masks, int(a.seconds * a.rate)
    sm = SpectrogramMasking(a.rate, a.mels).to(dev)
    n_fft, hop, T = sm.n_fft, sm.hop, S // sm.hop
    g = torch.Generator().manual_seed(0)
    wave_cpu = (torch.randn(B, S, generator=g) * 0.1).clamp(-1, 1)
    wave = wave_cpu.to(dev)
    logits = (3.0 * torch.randn(B, K, a.mels, T, generator=g)).to(dev)
    mel = sm.mel_spec
    window_cpu, fb_cpu = mel.window.cpu(), mel.fbank.cpu()
    fns = {'fused_ms': lambda: sm(wave, logits),
           'torch_device_ms': lambda: torch_device(wave, logits, mel.fbank, mel.window, n_fft, hop)}
    got, ref = fns['fused_ms'](), fns['torch_device_ms']()
    host = torch.stack([y[0] for y in host_reference(wave_cpu, logits, fb_cpu, window_cpu, n_fft, hop)]).view(B, K, -1)
    diffs = {'fused_vs_torch_device': float((got - ref).abs().max()), 'fused_vs_host_reference': float((got.cpu() - host).abs().max()),
             'output_abs_max': float(ref.abs().max())}
    for fn in fns.values():                                         # warm-up: code objects, allocator, the FFT plans
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in fns}
    per_round['host_reference_ms'] = []
    for _ in range(a.rounds):                                       # alternate the legs: other work shares the box
        for k, fn in fns.items():
            per_round[k].append(_median_ms(fn, a.reps))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_reference(wave_cpu, logits, fb_cpu, window_cpu, n_fft, hop)
        per_round['host_reference_ms'].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in per_round.items()}
    frames, n_freqs = T + 1, n_fft // 2 + 1
    tile_hops = ops.istft_tile(n_fft, hop) // hop
    held = -(-T // tile_hops) * ops.ISTFT_FRAMES                    # frames a row's workgroups transform, halo included
    per_frame = 2.0 * 4 * (n_fft // 2) * (n_fft // 4 + 1)           # threads n_fft / 4 + 1, n_fft / 2 trips of 4 fmaf each
    flop_needed = B * frames * (1 + K) * per_frame
    flop_done = B * held * (1 + K) * per_frame
    row = {'what': 'sep_mask_istft', 'B': B, 'K': K, 'samples': S, 'rate': a.rate, 'n_fft': n_fft, 'hop': hop, 'n_mels': a.mels,
           'frames': frames, 'reps': a.reps, 'rounds': a.rounds, **{k: round(v, 4) for k, v in med.items()},
           'spread_ms': {k: [round(min(v), 4), round(max(v), 4)] for k, v in per_round.items()},
           'rounds_ms': {k: [round(x, 4) for x in v] for k, v in per_round.items()},
           'torch_device_over_fused': round(med['torch_device_ms'] / med['fused_ms'], 2),
           'host_reference_over_fused': round(med['host_reference_ms'] / med['fused_ms'], 1),
           'fused_not_slower_than_torch_device': bool(med['fused_ms'] <= med['torch_device_ms']),
           'direct_dft_flop_needed': flop_needed, 'direct_dft_flop_with_halo': flop_done,
           'fused_tflops_with_halo': round(flop_done / med['fused_ms'] / 1e9, 2),
           'fused_share_of_fp32_vector_peak': round(flop_done / med['fused_ms'] / 1e9 / FP32_VECTOR_TFLOPS, 4),
           'max_abs_diff': diffs}
    print(json.dumps(row))
    if a.out:
        p = torch.cuda.get_device_properties(0)
        with open(a.out, 'w') as f:
            json.dump({'rows': [row], 'fp32_vector_peak_tflops': FP32_VECTOR_TFLOPS,
                       'measured_on': f'{p.name} {getattr(p, "gcnArchName", "")}'.strip(), 'date': time.strftime('%Y-%m-%d'),
                       'command': 'python tools/sep_bench.py ' + ' '.join(sys.argv[1:])}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
