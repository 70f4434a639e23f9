"""The nearest-neighbour probe on the device: dav_mean_l2n_f32 and dav_knn_topk_f32 elementwise against float64, ties and
determinism, the probe end to end against a torch restatement of the reference's evaluate, and train.py's probe cadence."""
import ast
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kcheck import INT_POISON, U32, Guarded, exact, poisoned, sum_bound, within  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _unit_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().to(DEV)


def test_mean_l2n_elementwise_strided_and_zero_row():
    from deepavfusion_amd import ops
    B, L, D, pad = 5, 37, 768, 8
    g = torch.Generator().manual_seed(3)
    base = torch.randn(B, L + 1, D + pad, generator=g).to(DEV)
    base[2] = 0.0                                                   # zero row: the eps clamp gives zeros
    x = base[:, 1:, :D]                                             # row stride D + pad, batch stride (L + 1)(D + pad)
    out = Guarded(B, D, torch.float32, device=DEV, fill='poison')
    ops.mean_l2n(x, out=out.t)
    x64 = x.double()
    v = x64.mean(1)
    n = v.norm(dim=1, keepdim=True)
    ref = v / n.clamp_min(1e-12)
    e = sum_bound(x64.abs().sum(1), L, v) / L                       # the mean: an L-term sum, one division
    en = e.norm(dim=1, keepdim=True)
    bound = (e + v.abs() * (en / n.clamp_min(1e-300) + (D + 4) * U32)) / n.clamp_min(1e-300) + 4 * U32 * ref.abs()
    rows = [0, 1, 3, 4]
    ok, worst, msg = within(out.t[rows], ref[rows], bound[rows], 'mean_l2n')
    assert ok, msg
    nz, msg = exact(out.t[2], torch.zeros(D, device=DEV), 'mean_l2n zero row')
    assert nz == 0, msg
    n_stray, where = out.stray()
    assert n_stray == 0, where
    print(f'mean_l2n worst err/bound {worst:.3f}')


def _knn_ref(Qs, Xs, sum_view):
    """float64 scores per view and their elementwise bound (an fp32 D-term FMA chain per modality; the sum view adds the three
    bounds and two roundings)."""
    D = Qs[0].shape[1]
    S, Bd = [], []
    for q, x in zip(Qs, Xs):
        S.append(q.double() @ x.double().t())
        Bd.append(D * U32 * (q.double().abs() @ x.double().abs().t()) + U32 * S[-1].abs())
    if sum_view:
        s = (S[0] + S[1]) + S[2] if len(S) == 3 else (S[0] + S[1] if len(S) == 2 else S[0].clone())
        S.append(s)
        Bd.append(sum(Bd) + 2 * U32 * sum(t.abs() for t in S[:-1]))
    return S, Bd


def _check_topk(val, idx, S, Bd, k, tag):
    """values within the row's bound of the true j-th largest; each value consistent with its index; indices exact where the
    float64 gaps on both sides exceed twice the bound.  -> number of positions too close to judge."""
    close = 0
    assert torch.isfinite(val).all(), f'{tag}: unwritten (NaN) values'
    N = S[0].shape[1]
    assert ((idx >= 0) & (idx < N)).all(), f'{tag}: index out of range'
    for v, (s, b) in enumerate(zip(S, Bd)):
        rb = b.max(dim=1).values[:, None]
        kk = min(k + 1, N)
        top, ti = torch.topk(s, kk, dim=1)
        ok, _, msg = within(val[v], top[:, :k], rb.expand(-1, k), f'{tag} view {v} values')
        assert ok, msg
        ok, _, msg = within(val[v], torch.gather(s, 1, idx[v].long()), torch.gather(b, 1, idx[v].long()), f'{tag} view {v} val/idx')
        assert ok, msg
        assert (val[v][:, 1:] <= val[v][:, :-1]).all(), f'{tag}: not sorted'
        gap_hi = torch.cat([torch.full_like(top[:, :1], float('inf')), top[:, :-1] - top[:, 1:]], 1)[:, :k]
        gap_lo = (top[:, :-1] - top[:, 1:])[:, :k] if kk > k else torch.full_like(top[:, :k], float('inf'))
        judge = (gap_hi > 2 * rb) & (gap_lo > 2 * rb)
        close += int((~judge).sum())
        bad = judge & (idx[v].long() != ti[:, :k])
        assert not bad.any(), f'{tag} view {v}: {int(bad.sum())} indices wrong where the gap is clear'
    return close


CASES = [(Nq, N, D, k) for Nq in (1, 37, 1000) for N in ('k', 129, 4097) for D in (64, 768) for k in (1, 2, 8)]


def test_knn_topk_values_and_indices():
    from deepavfusion_amd import ops
    close_total, n_pos = 0, 0
    for c, (Nq, N, D, k) in enumerate(CASES):
        N = k if N == 'k' else N
        M, sv = ((1, 0), (1, 1), (3, 0), (3, 1))[c % 4]
        Qs = [_unit_rows(Nq, D, 10 * c + m) for m in range(M)]
        Xs = [_unit_rows(N, D, 10 * c + 5 + m) for m in range(M)]
        V = M + sv
        val, idx = poisoned((V, Nq, k), torch.float32, DEV), poisoned((V, Nq, k), torch.int32, DEV)
        ops.knn_topk(Qs, Xs, k, sum_view=bool(sv), out=(val, idx))
        assert (idx != INT_POISON).all()
        S, Bd = _knn_ref(Qs, Xs, sv)
        close_total += _check_topk(val, idx, S, Bd, k, f'Nq={Nq} N={N} D={D} k={k} M={M} sum={sv}')
        n_pos += V * Nq * k
    # the probe's shape: N = Nq = 15,440, D = 768, M = 3 + sum, queries aliasing the bank
    n, D, k = 15440, 768, 2
    F = [_unit_rows(n, D, 900 + m) for m in range(3)]
    val, idx = poisoned((4, n, k), torch.float32, DEV), poisoned((4, n, k), torch.int32, DEV)
    ops.knn_topk(F, F, k, sum_view=True, out=(val, idx))
    S, Bd = _knn_ref(F, F, 1)
    close_total += _check_topk(val, idx, S, Bd, k, 'probe shape')
    n_pos += 4 * n * k
    del S, Bd
    print(f'knn_topk: {close_total} of {n_pos} positions too close to judge')


def test_knn_topk_ties_and_determinism():
    from deepavfusion_amd import ops
    N, D = 1000, 64
    X = _unit_rows(N, D, 77)
    X[200] = X[17]
    X[650] = X[17]
    X[900] = X[400]
    Xs = [X, _unit_rows(N, D, 78), _unit_rows(N, D, 79)]
    ref = None
    for splits in (1, 3, 8, None):
        out = ops.knn_topk(Xs, Xs, 8, sum_view=True, splits=splits)
        if ref is None:
            ref = out
            val, idx = out
            assert idx[0, 17, :3].tolist() == [17, 200, 650] and idx[0, 200, :3].tolist() == [17, 200, 650]
            assert idx[0, 400, :2].tolist() == [400, 900] and idx[0, 900, :2].tolist() == [400, 900]
            eq = val[:, :, 1:] == val[:, :, :-1]
            assert (idx[:, :, 1:][eq] > idx[:, :, :-1][eq]).all()         # every tie, lower index first
        else:
            assert exact(out[0], ref[0])[0] == 0 and torch.equal(out[1], ref[1]), f'splits={splits}'
    # query chunking: 128 at a time (views into the same bank tensors) equals all at once
    vals, idxs = [], []
    for i in range(0, N, 128):
        v, ix = ops.knn_topk([x[i:i + 128] for x in Xs], Xs, 8, sum_view=True, splits=2)
        vals.append(v)
        idxs.append(ix)
    assert exact(torch.cat(vals, 1), ref[0])[0] == 0 and torch.equal(torch.cat(idxs, 1), ref[1])


def _cfg(d):
    import train
    return train._wrap(d)


def _reference_preds(v, a, mm, labels):
    """util/knn_probe.py:113-131 of the reference in torch: chunks of 128 queries, einsum + topk(2), read at position 1."""
    preds = {m: [] for m in ('audio', 'image', 'fusion', 'all')}
    gaps = {m: [] for m in preds}
    for i in range(0, labels.shape[0], 128):
        sa = torch.einsum('qd,nd->qn', a[i:i + 128], a)
        sv = torch.einsum('qd,nd->qn', v[i:i + 128], v)
        smm = torch.einsum('qd,nd->qn', mm[i:i + 128], mm)
        for mod, s in (('audio', sa), ('image', sv), ('fusion', smm), ('all', sv + sa + smm)):
            _, nn_idx = torch.topk(s, k=2, dim=1, sorted=True)
            preds[mod].append(labels[nn_idx[:, 1]])
    s64 = {'audio': a.double() @ a.double().t(), 'image': v.double() @ v.double().t(), 'fusion': mm.double() @ mm.double().t()}
    s64['all'] = (s64['image'] + s64['audio']) + s64['fusion']
    for mod, s in s64.items():
        top = torch.topk(s, 3, dim=1).values
        D = v.shape[1]
        b = (3 if mod == 'all' else 1) * (D + 4) * U32 * 2
        gaps[mod] = ((top[:, 0] - top[:, 1]) <= 2 * b) | ((top[:, 1] - top[:, 2]) <= 2 * b)
    return {m: torch.cat(p) for m, p in preds.items()}, gaps


def test_probe_end_to_end_matches_reference_restatement():
    metrics = pytest.importorskip('sklearn.metrics')
    from deepavfusion_amd.build_model import build_avmae
    from deepavfusion_amd.configs import CONFIGS
    from deepavfusion_amd.util.knn_probe import EvalAVNNProbe, SyntheticLabelledAV, knn_predictions, probe_metrics
    cfg = CONFIGS['micro']
    torch.manual_seed(0)
    model = build_avmae(cfg).to(DEV)
    ncls = 8
    ds = SyntheticLabelledAV(256, ncls, cfg.image_size, cfg.audio_size, seed=1, noise=1.5)     # harder than the default 0.5
    probe = EvalAVNNProbe(_cfg({'dataset': None, 'batch_size': 64}), _cfg({'eval_freq': 1, 'print_freq': 10}),
                          _cfg({'seed': 0, 'workers': 0}), dataset=ds)
    out = probe.evaluate(model)
    assert list(out) == ['audio_nn_acc', 'image_nn_acc', 'fusion_nn_acc', 'all_nn_acc']
    v, a, mm, labels = probe.extract(model)
    assert v.shape == (256, cfg.embed_dim) and torch.allclose(v.norm(dim=1), torch.ones(256, device=DEV), atol=1e-5)
    preds = knn_predictions(v, a, mm, labels)
    again = probe_metrics({m: (p.cpu().numpy(), s.cpu().numpy()) for m, (p, s) in preds.items()}, labels.cpu().numpy(), False)
    assert again == out                                             # evaluate() is repeatable bit for bit
    ref, close = _reference_preds(v, a, mm, labels)
    n_close = 0
    for mod in ref:
        clear = ~close[mod]
        n_close += int(close[mod].sum())
        assert torch.equal(preds[mod][0][clear], ref[mod][clear]), mod
        acc_ref = float((ref[mod] == labels).double().mean() * 100)
        assert abs(out[f'{mod}_nn_acc'] - acc_ref) <= 100.0 * int(close[mod].sum()) / 256 + 1e-9, (mod, out, acc_ref)
    print(f'probe micro accuracies {out} (chance {100 / ncls:.1f} %), {n_close} queries too close to judge')
    assert min(out.values()) > 2 * 100 / ncls
    # the multi-label path on the device's predictions: multi-hot labels (own class + the next one for every third clip)
    lab = labels.cpu().numpy()
    mh = np.zeros((256, ncls + 2), np.int64)
    mh[np.arange(256), lab] = 1
    mh[np.arange(0, 256, 3), (lab[::3] + 1) % ncls] = 1
    mh_dev = torch.from_numpy(mh).to(DEV)
    from deepavfusion_amd import ops
    _, idx = ops.knn_topk((v, a, mm), (v, a, mm), 2, sum_view=True)
    view = {'image': 0, 'audio': 1, 'fusion': 2, 'all': 3}
    mpreds = {}
    for m, (p, s) in preds.items():
        rows = idx[view[m], :, 1]
        assert torch.equal(labels[rows], p)
        mpreds[m] = (mh_dev[rows], s)
    ml = probe_metrics({m: (p.cpu().numpy(), s.cpu().numpy()) for m, (p, s) in mpreds.items()}, mh, True)
    seen = mh.sum(0) > 0
    assert not seen.all()                                           # two classes never occur: removed as the reference does
    for m, (p, s) in mpreds.items():
        sc = p.cpu().numpy() * s.cpu().numpy()[:, None]
        assert abs(ml[f'{m}_nn_ap'] - metrics.average_precision_score(mh[:, seen], sc[:, seen], average=None).mean()) <= 1e-12
        assert abs(ml[f'{m}_nn_auc'] - metrics.roc_auc_score(mh[:, seen], sc[:, seen], average=None).mean()) <= 1e-12


def test_train_py_probe_cadence_and_checkpoint_equality(tmp_path):
    import train
    over = ['model.image.backbone=vit_tiny', 'model.audio.backbone=vit_tiny', 'model.fusion.num_heads=3', 'data.image_size=64',
            'data.audio_dur=2.', 'opt.batch_size=4', 'opt.epochs=3', 'opt.warmup_epochs=1', 'data.steps_per_epoch=2',
            'log.print_freq=1', 'log.eval_freq=2', f'output_dir={tmp_path}', 'job_name=t', 'env.workers=0',
            'nn_probe.dataset=synthetic', 'nn_probe.batch_size=32', 'nn_probe.num_samples=96', 'nn_probe.num_classes=4']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')] + over, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = re.findall(r'\[NN-probe\]\[Ep-(\d+)/3\] (\{.*\})$', r.stdout, re.M)       # after the log's timestamp
    assert [int(e) for e, _ in lines] == [0, 2], r.stdout[-3000:]
    last = ast.literal_eval(lines[-1][1])
    assert list(last) == ['audio_nn_acc', 'image_nn_acc', 'fusion_nn_acc', 'all_nn_acc']
    # a fresh model loaded from the checkpoint written right after epoch 2's probe gives the same metrics, bit for bit
    from deepavfusion_amd.models.avmae import AVMAE
    from deepavfusion_amd.models.deepavfusion import DeepAVFusion
    from deepavfusion_amd.util.knn_probe import EvalAVNNProbe
    cfg = train.load_config('deepavfusion', over)
    m = cfg.model
    enc = DeepAVFusion(image_arch='vit_tiny', image_pretrained='', image_size=(64, 64), audio_arch='vit_tiny', audio_pretrained='',
                       audio_size=(128, 128), fusion_arch=m.fusion.arch, fusion_layers=m.fusion.layers,
                       num_fusion_tkns=(m.fusion.num_fusion_tkns, m.fusion.num_aggr_image_tkns, m.fusion.num_aggr_audio_tkns),
                       fusion_mlp_ratio=m.fusion.mlp_ratio, fusion_attn_ratio=m.fusion.attn_ratio, fusion_num_heads=m.fusion.num_heads)
    model = AVMAE(enc, enc.embed_dim, image_decoder_arch=m.image.decoder_arch, image_decoder_depth=m.image.decoder_depth,
                  image_mask_ratio=m.image.mask_ratio, image_norm_loss=m.image.norm_loss, audio_decoder_arch=m.audio.decoder_arch,
                  audio_decoder_depth=m.audio.decoder_depth, audio_mask_ratio=m.audio.mask_ratio, audio_norm_loss=m.audio.norm_loss)
    ck = torch.load(os.path.join(str(tmp_path), 't', 'checkpoints', 'checkpoint_latest.pth'), map_location='cpu')
    assert ck['epoch'] == 3
    model.load_state_dict(ck['state_dict'], strict=True)
    model.to(DEV)
    got = EvalAVNNProbe(cfg.nn_probe, cfg.log, cfg.env).evaluate(model)
    assert got == last, (got, last)
