#!/usr/bin/env python3
"""Times the weighted k-NN probe at its shape — 15,440 queries against a 183 k-row train bank, D = 768, three modalities + the sum
view, k = 20 — three ways on the same operands and device:

  fused   dav_knn_topk_wide_f32 + dav_knn_vote_f32 (csrc/probe/knn_wide.hip);
  narrow  dav_knn_topk_f32 at k = 8: what the lists in the workspace cost over lists in registers (no vote: reported, not gated);
  torch   a stock-PyTorch restatement: chunks of queries, three einsums, one add, four topk(k), a one-hot vote.

The three alternate over ``--rounds`` rounds; medians and the peak memory of each (growth of max_memory_allocated over the operands)
go to ``--out``.  The one gate: fused is no slower than torch.

    python tools/knn_wide_bench.py [--rounds 3] [--chunk 512] [--out profiles/knn_wide_bench.json]

FLOP = 2 Nq N D M; the fp32 MFMA peak is 157.3 TF (MI355X, 2.4 GHz, 256 CUs x 4 SIMDs x 64 FLOP/clk)."""
import argparse
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_TF = 157.3
T = 0.07


def torch_restatement(Q, X, labels, C, k, chunk):
    inv_t = [1 / T, 1 / T, 1 / T, 1 / (3 * T)]
    scores, preds = [], []
    for i in range(0, Q[0].shape[0], chunk):
        s = [torch.einsum('qd,nd->qn', q[i:i + chunk], x) for q, x in zip(Q, X)]
        s.append((s[0] + s[1]) + s[2])
        val, idx = zip(*(torch.topk(t, k=k, dim=1, sorted=True) for t in s))
        del s
        w = torch.exp(torch.stack(val) * torch.tensor(inv_t, device=val[0].device)[:, None, None])       # [V, q, k]
        hot = torch.nn.functional.one_hot(labels[torch.stack(idx)], C)                                     # [V, q, k, C]
        sc = (hot * w[..., None]).sum(2)
        scores.append(sc)
        preds.append(sc.argmax(-1))
    return torch.cat(scores, 1), torch.cat(preds, 1)


def _timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return e0.elapsed_time(e1), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--queries', type=int, default=15440)
    ap.add_argument('--bank', type=int, default=183000)
    ap.add_argument('--dim', type=int, default=768)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--classes', type=int, default=309)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=512, help='queries per chunk of the torch restatement (the reference uses 128)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from deepavfusion_amd import ops
    Nq, N, D, k, C = args.queries, args.bank, args.dim, args.k, args.classes
    g = torch.Generator(device='cuda').manual_seed(0)
    Q = [torch.nn.functional.normalize(torch.randn(Nq, D, device='cuda', generator=g), dim=1) for _ in range(3)]
    X = [torch.nn.functional.normalize(torch.randn(N, D, device='cuda', generator=g), dim=1) for _ in range(3)]
    labels = torch.randint(0, C, (N,), device='cuda', generator=g)
    labels32 = labels.int()
    inv_t = [1 / T] * 3 + [1 / (3 * T)]
    S = ops.knn_splits(Nq, N)

    def fused():
        val, idx = ops.knn_topk(Q, X, k, sum_view=True, splits=S)
        return ops.knn_vote(val, idx, labels32, C, k, inv_t)

    runs = {'fused': fused,
            'narrow_k8': lambda: ops.knn_topk(Q, X, 8, sum_view=True, splits=S),
            'torch': lambda: torch_restatement(Q, X, labels, C, k, args.chunk)}
    # the fused pair against the restatement, once: the same votes wherever the restatement's own fp32 scores leave no doubt
    fs, fp = fused()
    ts, tp = torch_restatement(Q, X, labels, C, k, args.chunk)
    agree = float((fp == tp).double().mean())
    rel = float(((fs - ts).abs().amax(-1) / ts.amax(-1)).max())
    del fs, fp, ts, tp
    for fn in runs.values():
        _timed(fn)                                            # warm-up: first launches, library heuristics, the allocator's pools
    ms, peak = {n: [] for n in runs}, {n: 0 for n in runs}
    for _ in range(args.rounds):
        for n, fn in runs.items():
            t, p = _timed(fn)
            ms[n].append(t)
            peak[n] = max(peak[n], p)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    flop = 2.0 * Nq * N * D * 3
    dev = torch.cuda.get_device_properties(0)
    row = {'what': 'knn_wide', 'Nq': Nq, 'N': N, 'D': D, 'M': 3, 'sum_view': 1, 'k': k, 'classes': C, 'splits': S,
           'torch_chunk': args.chunk, 'rounds': args.rounds,
           'ms': {n: round(v, 2) for n, v in med.items()}, 'ms_all': {n: [round(t, 2) for t in v] for n, v in ms.items()},
           'peak_mb': {n: round(p / 2**20, 1) for n, p in peak.items()},
           'workspace_mb': round(ops.knn_workspace_bytes(Nq, 4, k, S) / 2**20, 1),
           'fused_vs_torch': round(med['torch'] / med['fused'], 2), 'fused_vs_narrow_k8': round(med['fused'] / med['narrow_k8'], 3),
           'fused_no_slower_than_torch': bool(med['fused'] <= med['torch']),
           'fused_tflops': round(flop / med['fused'] / 1e9, 1), 'frac_fp32_peak': round(flop / med['fused'] / 1e9 / PEAK_F32_TF, 3),
           'pred_agreement_with_torch': round(agree, 5), 'max_rel_score_diff': float(f'{rel:.3g}'), 'device': dev.name}
    print(json.dumps(row))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'rows': [row], 'date': datetime.date.today().isoformat(),
                       'measured_on': f'{dev.name} ({getattr(dev, "gcnArchName", "")}), 1 GPU',
                       'command': 'python tools/knn_wide_bench.py ' + ' '.join(sys.argv[1:])}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
