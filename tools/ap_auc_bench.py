#!/usr/bin/env python3
"""Times the multi-label metrics of the probe (per-class AP and ROC AUC, four views) three ways on the same data, for each of the
two forms the probe has (the dense vote scores; the reference protocol's neighbour label x neighbour score):

  host    what nn_probe.metrics=host does: the predictions / vote scores copied to the host, then util/knn_probe.py's numpy
          restatement of sklearn (probe_metrics / vote_metrics); a host clock around it, copies included;
  torch   a stock-PyTorch restatement on the device: torch.sort along the rows, fp64 cumsum, ties grouped — all four views in one
          batched call; device events, and the peak of torch's allocator above the resident inputs;
  kernel  ops.ap_auc (dav_ap_auc_f64, csrc/probe/ap_auc.hip), outputs and workspace allocated once; device events.

    python tools/ap_auc_bench.py [--n 20000] [--classes 527] [--reps 20] [--host-reps 2] [--out profiles/ap_auc_bench.json]

One JSON line per form.  The three results are compared with each other on the way (max |difference| of the per-class values
between torch and kernel, of the eight means between host and kernel)."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_ap_auc(y, s):
    """y bool [n, C], s fp32 [V, n, C] -> (ap, auc) fp64 [V, C]: sklearn's curves with ties grouped, in stock torch ops."""
    V, n, C = s.shape
    ss, order = torch.sort(s, dim=1, descending=True)
    tps = torch.gather(y.expand(V, n, C), 1, order).double().cumsum(1)
    last = torch.ones(V, n, C, dtype=torch.bool, device=s.device)               # the last row of every tie group
    last[:, :-1] = ss[:, 1:] != ss[:, :-1]
    rank = torch.arange(1, n + 1, device=s.device, dtype=torch.float64)[None, :, None]
    fps = rank - tps
    zero = torch.zeros((), dtype=torch.float64, device=s.device)

    def before(x):                                                              # x at the end of the previous group (0 for the first)
        m = torch.cummax(torch.where(last, x, zero), 1).values
        return torch.cat([torch.zeros_like(m[:, :1]), m[:, :-1]], 1)
    tp0, fp0 = before(tps), before(fps)
    P = tps[:, -1]
    Nn = n - P
    ap = torch.where(last, (tps - tp0) * (tps / rank), zero).sum(1) / P
    auc = torch.where(last, (fps - fp0) * (tps + tp0) / 2, zero).sum(1) / (P * Nn)
    return ap, auc


def _event_ms(fn, reps, warmup=3):
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
    return ts[len(ts) // 2], ts[0], ts[-1]


def _host_ms(fn, reps):
    fn()                                                                        # warm-up: first copies, numpy's caches
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], out


def _peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


def bench(form, n, C, N, reps, host_reps):
    from deepavfusion_amd import ops
    from deepavfusion_amd.util import knn_probe as K
    V, k = 4, 20
    g = torch.Generator(device='cuda').manual_seed(0)
    labels = (torch.rand(n, C, device='cuda', generator=g) < 0.02).long()       # as extract() gathers them: int64 multi-hot
    labels[torch.randint(0, n, (C,), device='cuda', generator=g), torch.arange(C, device='cuda')] = 1      # every class occurs
    truth = labels.to(torch.uint8)
    out = (torch.empty(V, C, dtype=torch.float64, device='cuda'), torch.empty(V, C, dtype=torch.float64, device='cuda'),
           torch.empty(C, dtype=torch.int32, device='cuda'))
    ws = torch.empty(ops.ap_auc_workspace_bytes(V, n, C), dtype=torch.uint8, device='cuda')
    if form == 'dense':
        # vote scores as dav_knn_vote_f32 leaves them: k weights exp(sim / T) spread over the classes of k neighbours, zero elsewhere
        scores = torch.zeros(V, n, C, device='cuda')
        bank = (torch.rand(N, C, device='cuda', generator=g) < 0.02).float()
        for v in range(V):
            for _ in range(k):
                w = torch.exp(torch.rand(n, 1, device='cuda', generator=g) / 0.07 * 0.5)
                scores[v] += bank[torch.randint(0, N, (n,), device='cuda', generator=g)] * w
        del bank

        def host():
            return K.vote_metrics(OrderedDict((m, scores[K._VIEW[m]].cpu().numpy()) for m in K.MODALITIES), None,
                                  labels.cpu().numpy(), True, k)

        def stock():
            return torch_ap_auc(truth.bool(), scores)

        def kernel():
            return ops.ap_auc(truth, scores, out=out, workspace=ws)
        tag = f'knn{k}'
    else:
        idx = torch.randint(0, n, (V, n), device='cuda', generator=g)
        val = torch.rand(V, n, device='cuda', generator=g) * 2 - 1
        idx32 = idx.to(torch.int32)

        def host():
            return K.probe_metrics(OrderedDict((m, (labels[idx[K._VIEW[m]]].cpu().numpy(), val[K._VIEW[m]].cpu().numpy()))
                                               for m in K.MODALITIES), labels.cpu().numpy(), True)

        def stock():
            return torch_ap_auc(truth.bool(), truth[idx].float() * val[:, :, None])

        def kernel():
            return ops.ap_auc(truth, nbr=idx32, nbr_val=val, nbr_labels=truth, out=out, workspace=ws)
        tag = 'nn'
    host_ms, host_out = _host_ms(host, host_reps)
    torch_peak, (t_ap, t_auc) = _peak_mb(stock)
    kernel_peak, _ = _peak_mb(kernel)
    ap, auc, pos = (t.clone() for t in kernel())
    assert torch.equal(pos.long(), labels.sum(0)) and not torch.isnan(auc).any()
    dev_out = K.device_metrics(ap.cpu().numpy(), auc.cpu().numpy(), pos.cpu().numpy(), tag)
    assert list(dev_out) == list(host_out)
    # the two device paths alternate, so that a change of clocks or of the neighbours on the machine meets both
    t_ms, k_ms = [], []
    for _ in range(3):
        t_ms.append(_event_ms(stock, max(3, reps // 4)))
        k_ms.append(_event_ms(kernel, reps))
    t_med, k_med = sorted(t[0] for t in t_ms)[1], sorted(t[0] for t in k_ms)[1]
    return {'what': 'ap_auc', 'form': form, 'n': n, 'C': C, 'V': V, 'bank_rows': N if form == 'dense' else n,
            'host_ms': round(host_ms, 1), 'torch_ms': round(t_med, 3), 'kernel_ms': round(k_med, 3),
            'torch_ms_min_max': [round(min(t[1] for t in t_ms), 3), round(max(t[2] for t in t_ms), 3)],
            'kernel_ms_min_max': [round(min(t[1] for t in k_ms), 3), round(max(t[2] for t in k_ms), 3)],
            'host_over_kernel': round(host_ms / k_med, 1), 'torch_over_kernel': round(t_med / k_med, 2),
            'torch_peak_mb': round(torch_peak, 1), 'kernel_peak_mb': round(kernel_peak, 3),
            'kernel_workspace_mb': round(ws.numel() / 2 ** 20, 3),
            'max_diff_torch_kernel': float(max((t_ap - ap).abs().max(), (t_auc - auc).abs().max())),
            'max_diff_host_kernel_means': float(max(abs(host_out[key] - dev_out[key]) for key in host_out)),
            'bound_per_class': 4 * n * 2.0 ** -53}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=20000)
    p.add_argument('--classes', type=int, default=527)
    p.add_argument('--bank', type=int, default=183000)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--host-reps', type=int, default=2)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/ap_auc_bench.py measures on an MI355X; there is no CPU fallback')
    dev = torch.cuda.get_device_properties(0)
    rows = []
    for form in ('dense', 'neighbour'):
        r = bench(form, args.n, args.classes, args.bank, args.reps, args.host_reps)
        r['device'] = dev.name
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'rows': rows, 'measured_on': f'{dev.name} {getattr(dev, "gcnArchName", "")}'.strip(),
                       'command': f'python tools/ap_auc_bench.py --n {args.n} --classes {args.classes} --bank {args.bank} '
                                  f'--reps {args.reps} --host-reps {args.host_reps}'}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
