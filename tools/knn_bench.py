#!/usr/bin/env python3
"""Times dav_knn_topk_f32 (the nearest-neighbour probe's fused similarity + top-k, csrc/probe/knn.hip) against a torch restatement
of the reference's loop (util/knn_probe.py:113-131: chunks of 128 queries, three einsums, one add, four topk(2)) on the same device
and data, and the probe's evaluate() end to end at ViT-B on the synthetic labelled set.

    python tools/knn_bench.py [--reps 10] [--out profiles/knn_bench.json] [--eval-samples 1024]

One JSON line per measurement; FLOP = 2 Nq N D M; the fp32 MFMA peak is 157.3 TF (MI355X, 2.4 GHz, 256 CUs x 4 SIMDs x 64 FLOP/clk)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_TF = 157.3


def _time_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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


def torch_reference(v, a, mm, labels):
    out = []
    for i in range(0, labels.shape[0], 128):
        sa = torch.einsum('qd,nd->qn', a[i:i + 128], a)
        sv = torch.einsum('qd,nd->qn', v[i:i + 128], v)
        smm = torch.einsum('qd,nd->qn', mm[i:i + 128], mm)
        for s in (sa, sv, smm, sv + sa + smm):
            sc, nn_idx = torch.topk(s, k=2, dim=1, sorted=True)
            out.append((labels[nn_idx[:, 1]], sc[:, 1]))
    return out


def bench_kernel(n, D, reps):
    from deepavfusion_amd import ops
    g = torch.Generator(device='cuda').manual_seed(0)
    F = [torch.nn.functional.normalize(torch.randn(n, D, device='cuda', generator=g), dim=1) for _ in range(3)]
    labels = torch.randint(0, 309, (n,), device='cuda', generator=g)
    S = ops.knn_splits(n, n)
    ws = torch.empty(ops.knn_workspace_bytes(n, 4, 2, S), dtype=torch.uint8, device='cuda')
    out = (torch.empty(4, n, 2, device='cuda'), torch.empty(4, n, 2, dtype=torch.int32, device='cuda'))
    k_ms = _time_ms(lambda: ops.knn_topk(F, F, 2, sum_view=True, splits=S, out=out, workspace=ws), reps)
    t_ms = _time_ms(lambda: torch_reference(F[0], F[1], F[2], labels), max(3, reps // 3))
    flop = 2.0 * n * n * D * 3
    return {'what': 'knn_topk', 'N': n, 'Nq': n, 'D': D, 'M': 3, 'sum_view': 1, 'k': 2, 'splits': S,
            'kernel_ms': round(k_ms, 3), 'torch_ms': round(t_ms, 3), 'speedup': round(t_ms / k_ms, 2),
            'kernel_tflops': round(flop / k_ms / 1e9, 1), 'frac_fp32_peak': round(flop / k_ms / 1e9 / PEAK_F32_TF, 3)}


def bench_evaluate(samples, batch):
    import train
    from deepavfusion_amd.build_model import build_avmae
    from deepavfusion_amd.configs import CONFIGS
    from deepavfusion_amd.util import knn_probe as K
    cfg = CONFIGS['base']
    model = build_avmae(cfg).cuda()
    ds = K.SyntheticLabelledAV(samples, 16, cfg.image_size, cfg.audio_size, seed=0)
    probe = K.EvalAVNNProbe(train._wrap({'dataset': None, 'batch_size': batch * 4}), train._wrap({'eval_freq': 1, 'print_freq': 10}),
                            train._wrap({'seed': 0, 'workers': 4}), dataset=ds)
    probe.evaluate(model)                                   # warm-up (first launches, loader workers)
    torch.cuda.synchronize()
    t0 = time.time()
    metrics = probe.evaluate(model)
    torch.cuda.synchronize()
    total = (time.time() - t0) * 1e3
    v, a, mm, labels = probe.extract(model)
    knn = _time_ms(lambda: K.knn_predictions(v, a, mm, labels), 5)
    return {'what': 'evaluate', 'model': 'base', 'samples': samples, 'batch': batch, 'evaluate_ms': round(total, 1),
            'knn_ms': round(knn, 3), 'knn_share': round(knn / total, 4), 'metrics': metrics}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--eval-samples', type=int, default=1024)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = [bench_kernel(15440, 768, args.reps), bench_kernel(2048, 768, args.reps)]
    if args.eval_samples:
        rows.append(bench_evaluate(args.eval_samples, 16))
    dev = torch.cuda.get_device_properties(0)
    for r in rows:
        r['device'] = dev.name
        print(json.dumps(r))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'rows': rows, 'measured_on': f'{dev.name} {getattr(dev, "gcnArchName", "")}'.strip(),
                       'command': 'python tools/knn_bench.py ' + ' '.join(sys.argv[1:])}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
