"""The weighted k-NN probe on the device: dav_knn_topk_wide_f32 elementwise against float64 (values, indices, order, poison), bit
for bit against dav_knn_topk_f32, ties / splits / chunking / an adversely ordered bank; dav_knn_vote_f32 against integer counts and
a float64 restatement; the memory both need; and the probe end to end with ``nn_probe.k`` set."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kcheck import INT_POISON, U32, Guarded, exact, within  # noqa: E402
from test_knn_probe_gpu import _knn_ref, _unit_rows  # noqa: E402  (the narrow kernel's seeding and score bound)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _topk(Qs, Xs, k, sum_view, splits=None, name='dav_knn_topk_wide_f32', guarded=False):
    """One call of a top-k entry point by name (ops.knn_topk would pick the narrow one for k <= 8), outputs poisoned, the workspace
    filled with 0xFF bytes.  -> (val [V, Nq, k], idx int32 [V, Nq, k]) and, with ``guarded``, their Guarded buffers."""
    from deepavfusion_amd import _lib, ops
    M, (Nq, D), N = len(Qs), Qs[0].shape, Xs[0].shape[0]
    V = M + int(sum_view)
    S = ops.knn_splits(Nq, N) if splits is None else splits
    gv, gi = Guarded(V * Nq, k, torch.float32, device=DEV), Guarded(V * Nq, k, torch.int32, device=DEV)
    ws = torch.full((ops.knn_workspace_bytes(Nq, V, k, S),), 0xFF, dtype=torch.uint8, device=DEV)
    qp = [q.data_ptr() for q in Qs] + [None] * (3 - M)
    xp = [x.data_ptr() for x in Xs] + [None] * (3 - M)
    rc = getattr(_lib.load(), name)(qp[0], xp[0], qp[1], xp[1], qp[2], xp[2], M, Nq, N, D, Qs[0].stride(0), Xs[0].stride(0),
                                    int(sum_view), k, S, gv.ptr(), gi.ptr(), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f'{name} returned {rc}'
    out = gv.t.view(V, Nq, k), gi.t.view(V, Nq, k)
    return out + (gv, gi) if guarded else out


def _check_wide(val, idx, S, Bd, k, tag, exact_idx):
    """No poison; indices in range and distinct; rows sorted; every value within the row's bound of the float64 j-th largest and
    within its element's bound of the float64 score of its own index.  ``exact_idx``: indices exact where the float64 gaps on both
    sides exceed twice the bound.  -> (positions left out of the exact-index check, positions)."""
    assert torch.isfinite(val).all(), f'{tag}: unwritten (NaN) values'
    assert (idx != INT_POISON).all(), f'{tag}: unwritten indices'
    N = S[0].shape[1]
    assert ((idx >= 0) & (idx < N)).all(), f'{tag}: index out of range'
    srt = idx.sort(dim=2).values
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all(), f'{tag}: a bank row twice in one list'
    assert (val[:, :, 1:] <= val[:, :, :-1]).all(), f'{tag}: not sorted'
    close = 0
    for v, (s, b) in enumerate(zip(S, Bd)):
        rb = b.max(dim=1).values[:, None]
        kk = min(k + 1, N)
        top, ti = torch.topk(s, kk, dim=1)
        ok, _, msg = within(val[v], top[:, :k], rb.expand(-1, k), f'{tag} view {v} values')
        assert ok, msg
        ok, _, msg = within(val[v], torch.gather(s, 1, idx[v].long()), torch.gather(b, 1, idx[v].long()), f'{tag} view {v} val/idx')
        assert ok, msg
        if exact_idx:
            gap = top[:, :-1] - top[:, 1:]
            inf = torch.full_like(top[:, :1], float('inf'))
            gap_hi = torch.cat([inf, gap], 1)[:, :k]
            gap_lo = torch.cat([gap, inf], 1)[:, :k]             # N == k: nothing below the last entry
            judge = (gap_hi > 2 * rb) & (gap_lo > 2 * rb)
            close += int((~judge).sum())
            bad = judge & (idx[v].long() != ti[:, :k])
            assert not bad.any(), f'{tag} view {v}: {int(bad.sum())} indices wrong where the gap is clear'
    return close, val.numel()


SHAPES = [(37, 129, 64, 9), (37, 129, 64, 64), (1, 64, 64, 64), (37, 65, 64, 64), (37, 4097, 64, 20), (37, 4097, 64, 64),
          (130, 4097, 768, 20), (130, 1000, 768, 33), (130, 4097, 768, 64)]


@pytest.mark.parametrize('c', range(len(SHAPES)), ids=['-'.join(map(str, s)) for s in SHAPES])
def test_wide_topk_values_and_indices(c):
    """Float64 reference alone, measured on the CPU with these seeds: the exact-index check leaves out at most 0.81 % of the
    positions of any D = 64 shape (allowed here: 2 %); at D = 768 it would leave out 9-37 %, so those shapes are not judged by
    index — their values, value/index consistency, distinctness and order are."""
    Nq, N, D, k = SHAPES[c]
    for M, sv in ((1, 0), (3, 1)):
        Qs = [_unit_rows(Nq, D, 10 * c + m) for m in range(M)]
        Xs = [_unit_rows(N, D, 10 * c + 5 + m) for m in range(M)]
        val, idx, gv, gi = _topk(Qs, Xs, k, sv, guarded=True)
        S, Bd = _knn_ref(Qs, Xs, sv)
        tag = f'Nq={Nq} N={N} D={D} k={k} M={M} sum={sv}'
        close, n = _check_wide(val, idx, S, Bd, k, tag, exact_idx=D == 64)
        for g in (gv, gi):
            n_stray, where = g.stray()
            assert n_stray == 0, f'{tag}: {where}'
        if D == 64:
            print(f'{tag}: {close} of {n} positions ({100.0 * close / n:.2f} %) too close to judge by index')
            assert close <= 0.02 * n, f'{tag}: the exact-index check leaves out {close} of {n} positions'


def test_ops_routes_long_lists_to_the_wide_kernel():
    from deepavfusion_amd import ops
    Qs = [_unit_rows(37, 64, 400 + m) for m in range(3)]
    Xs = [_unit_rows(300, 64, 405 + m) for m in range(3)]
    for k in (9, 64):
        val, idx = ops.knn_topk(Qs, Xs, k, sum_view=True)
        rv, ri = _topk(Qs, Xs, k, 1)
        assert idx.dtype == torch.int64 and exact(val, rv.contiguous())[0] == 0 and torch.equal(idx, ri.long())
    with pytest.raises(RuntimeError, match='bad shape'):
        ops.knn_topk(Qs, Xs, 65, sum_view=True)


def test_wide_agrees_with_the_narrow_kernel_bit_for_bit():
    Qs = [_unit_rows(130, 768, 500 + m) for m in range(3)]
    Xs = [_unit_rows(4097, 768, 505 + m) for m in range(3)]
    nv, ni = _topk(Qs, Xs, 8, 1, name='dav_knn_topk_f32')
    wv, wi = _topk(Qs, Xs, 8, 1)
    n, msg = exact(wv.contiguous(), nv.contiguous(), 'wide k=8 vs narrow k=8')
    assert n == 0 and torch.equal(wi, ni), msg
    wv, wi = _topk(Qs, Xs, 64, 1)
    n, msg = exact(wv[:, :, :8].contiguous(), nv.contiguous(), 'first 8 of wide k=64 vs narrow k=8')
    assert n == 0 and torch.equal(wi[:, :, :8], ni), msg


TWELVE = [5, 100, 127, 128, 200, 255, 300, 400, 511, 640, 777, 999]      # tiles 0, 1, 2, 3, 5, 6, 7
THREE = [50, 450, 900]


def test_wide_ties_and_determinism():
    N, D, k = 1000, 64, 16
    X = _unit_rows(N, D, 77)
    X[TWELVE] = X[TWELVE[0]].clone()
    X[THREE] = X[THREE[0]].clone()
    Xs = [X, _unit_rows(N, D, 78), _unit_rows(N, D, 79)]
    ref = None
    for splits in (1, 3, 8, None):
        val, idx = _topk(Xs, Xs, k, 1, splits=splits)
        if ref is None:
            ref = (val.clone(), idx.clone())
            for q in TWELVE:
                assert idx[0, q, :12].tolist() == TWELVE, (q, idx[0, q].tolist())
            for q in THREE:
                assert idx[0, q, :3].tolist() == THREE, (q, idx[0, q].tolist())
            eq = val[:, :, 1:] == val[:, :, :-1]
            assert int(eq.sum()) >= 12 * 11 + 3 * 2
            assert (idx[:, :, 1:][eq] > idx[:, :, :-1][eq]).all()         # every tie, lower index first
        else:
            assert exact(val.contiguous(), ref[0])[0] == 0 and torch.equal(idx, ref[1]), f'splits={splits}'
    vals, idxs = [], []
    for i in range(0, N, 128):                                            # views into the same bank tensors
        v, ix = _topk([x[i:i + 128] for x in Xs], Xs, k, 1, splits=2)
        vals.append(v)
        idxs.append(ix)
    assert exact(torch.cat(vals, 1), ref[0])[0] == 0 and torch.equal(torch.cat(idxs, 1), ref[1])


def _canonical(val, idx):
    """rows re-sorted by (value descending, index ascending)"""
    o = idx.sort(dim=-1, stable=True).indices
    val, idx = torch.gather(val, -1, o), torch.gather(idx, -1, o)
    o = val.sort(dim=-1, descending=True, stable=True).indices
    return torch.gather(val, -1, o), torch.gather(idx, -1, o)


def test_wide_adverse_order():
    """The bank sorted by ascending similarity to query 0: every bank row displaces one of that query's list."""
    Nq, N, D, k = 37, 2000, 64, 64
    Q, X = [_unit_rows(Nq, D, 600)], _unit_rows(N, D, 605)
    order = torch.argsort(X.double() @ Q[0][0].double())                 # sorted row j is shuffled row order[j]
    rv, ri = _topk(Q, [X], k, 0)
    sv, si = _topk(Q, [X[order].contiguous()], k, 0)
    assert (si[0, 0] >= N - k - 16).all()                                 # query 0: the last rows of the sorted bank
    mv, mi = _canonical(sv, order[si.long()].int())
    n, msg = exact(mv.contiguous(), rv.contiguous(), 'sorted bank vs shuffled bank')
    assert n == 0 and torch.equal(mi, ri), msg


# ---- vote -------------------------------------------------------------------------------------------------------------------

T = 0.07


def _vote_ref(val, idx, labels, C, k, inv_t, self_offset):
    """float64 restatement on the same (val, idx): -> scores [V, Nq, C], their elementwise bound, the neighbours used [V, Nq, kk].
    With x_j = val_j inv_t and w_j = exp(x_j):  the fp32 product x_j carries a relative u, which the exponent turns into a
    relative |x_j| u of w_j; expf is accurate to 1 ulp = 2 u; a class's k terms are added one after the other, (k - 1) u of their
    sum.  Bound of a class: u sum over its neighbours of w_j (|x_j| + 2 + k)."""
    V, Nq, kk = val.shape
    q = torch.arange(Nq, device=val.device)[None, :, None]
    keep = (idx != q + self_offset) if self_offset >= 0 else torch.ones_like(idx, dtype=torch.bool)
    used = keep & (keep.cumsum(2) <= k)
    assert (used.sum(2) == k).all()
    x = val.double() * torch.tensor(inv_t, dtype=torch.float64, device=val.device)[:, None, None]
    w = torch.exp(x) * used
    wb = U32 * w * (x.abs() + 2 + k)
    if labels.dim() == 1:
        hot = torch.nn.functional.one_hot(labels.long()[idx.long()], C).double()
    else:
        hot = labels[idx.long()].double()
    return torch.einsum('vqj,vqjc->vqc', w, hot), torch.einsum('vqj,vqjc->vqc', wb, hot), used


def _argmax_low(s):
    C = s.shape[-1]
    cls = torch.arange(C, device=s.device).expand_as(s)
    return torch.where(s == s.max(-1, keepdim=True).values, cls, C).min(-1).values


@pytest.fixture(scope='module')
def lists():
    """top-k outputs (V = 4, Nq = 130, kk = 21) over a bank of 1000 whose first 130 rows are the queries"""
    Xs = [_unit_rows(1000, 64, 700 + m) for m in range(3)]
    val, idx = _topk([x[:130] for x in Xs], Xs, 21, 1)
    assert (idx[:, :, 0] == torch.arange(130, device=DEV)).all()        # a bank row equal to the query comes first
    return val.contiguous(), idx.contiguous()


@pytest.mark.parametrize('C', [3, 10, 309])
@pytest.mark.parametrize('self_offset', [-1, 0])
def test_vote_counts_and_weights(lists, C, self_offset):
    """inv_t = 0: exact integer counts.  inv_t = 1 / T (a third of it for the sum view): scores within u sum_j w_j (|x_j| + 2 + k)
    of the float64 restatement (derivation: _vote_ref), pred exact where the two best classes are further apart than twice the
    bound of either."""
    from deepavfusion_amd import ops
    val, idx = lists
    k, N = 20, 1000
    g = torch.Generator().manual_seed(C)
    ids = torch.randint(0, C, (N,), generator=g, dtype=torch.int32).to(DEV)
    multi = (torch.rand(N, C, generator=g) < 0.3).to(torch.uint8).to(DEV)
    weights = [float(np.float32(1 / T))] * 3 + [float(np.float32(1 / (3 * T)))]
    for inv_t in ([0.0] * 4, weights):
        for labels in (ids, multi):
            scores = torch.full((4, 130, C), float('nan'), device=DEV)
            pred = torch.full((4, 130), INT_POISON, dtype=torch.int32, device=DEV)
            ops.knn_vote(val, idx, labels, C, k, inv_t, self_offset=self_offset, out=(scores, None if labels is multi else pred))
            ref, bound, used = _vote_ref(val, idx, labels, C, k, inv_t, self_offset)
            # the query's own row: first in every list, skipped with self_offset = 0 and used with -1
            assert bool(used[:, :, 0].any()) == (self_offset < 0) and bool(used[:, :, 20].any()) == (self_offset >= 0)
            tag = f'C={C} self_offset={self_offset} inv_t={inv_t[0]:.3g} {"multi-hot" if labels is multi else "class ids"}'
            if inv_t[0] == 0.0:
                n, msg = exact(scores, ref.float(), tag)
                assert n == 0, msg
                assert float(scores.sum()) == (4 * 130 * k if labels is ids else float(multi[idx.long()].double().mul(used[..., None]).sum()))
            else:
                ok, worst, msg = within(scores, ref, bound, tag)
                assert ok, msg
                print(f'{tag}: worst err/bound {worst:.3f}')
            if labels is ids:
                assert (pred != INT_POISON).all()
                again = torch.full_like(pred, INT_POISON)
                s2 = torch.full_like(scores, float('nan'))
                ops.knn_vote(val, idx, labels, C, k, inv_t, self_offset=self_offset, out=(s2, again))
                assert exact(s2, scores)[0] == 0 and torch.equal(again, pred)                 # repeatable bit for bit
                assert torch.equal(pred.long(), _argmax_low(scores)), f'{tag}: pred is not the argmax of scores, ties to the lower class'
                if inv_t[0] == 0.0:
                    ties = (scores == scores.max(-1, keepdim=True).values).sum(-1) > 1
                    assert ties.any(), f'{tag}: no tie between classes in this case'
                    print(f'{tag}: {int(ties.sum())} of {ties.numel()} queries with tied classes')
                else:
                    top2 = torch.topk(ref, 2, dim=-1)
                    b2 = torch.gather(bound, 2, top2.indices).sum(-1)
                    clear = (top2.values[..., 0] - top2.values[..., 1]) > 2 * b2
                    assert (~clear).sum() <= 0.01 * clear.numel(), f'{tag}: {int((~clear).sum())} queries too close to judge'
                    assert torch.equal(pred.long()[clear], top2.indices[..., 0][clear]), tag


def test_vote_refuses_too_few_entries(lists):
    from deepavfusion_amd import ops
    val, idx = lists
    ids = torch.zeros(1000, dtype=torch.int32, device=DEV)
    ops.knn_vote(val, idx, ids, 3, 21, [0.0] * 4, self_offset=-1)
    with pytest.raises(ValueError):
        ops.knn_vote(val, idx, ids, 3, 21, [0.0] * 4, self_offset=0)          # 20 entries remain after the exclusion
    with pytest.raises(ValueError):
        ops.knn_vote(val, idx, ids, 3, 22, [0.0] * 4)


def test_topk_and_vote_memory():
    """Peak growth <= what is returned + the documented workspace + 1 MB; the four score matrices alone would be 512 MB."""
    from deepavfusion_amd import ops
    Nq, N, D, k, C = 2048, 16384, 64, 20, 10
    Qs = [_unit_rows(Nq, D, 800 + m) for m in range(3)]
    Xs = [_unit_rows(N, D, 805 + m) for m in range(3)]
    labels = torch.randint(0, C, (N,), dtype=torch.int32).to(DEV)
    out = (torch.empty(4, Nq, k, device=DEV), torch.empty(4, Nq, k, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    val, idx64 = ops.knn_topk(Qs, Xs, k, sum_view=True, out=out)
    scores, pred = ops.knn_vote(val, out[1], labels, C, k, [1 / T] * 3 + [1 / (3 * T)])
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    returned = sum(t.numel() * t.element_size() for t in (idx64, scores, pred)) + 4 * Nq * 4          # + the int32 pred
    ws = ops.knn_workspace_bytes(Nq, 4, k, ops.knn_splits(Nq, N))
    print(f'top-k + vote: peak growth {grown / 2**20:.1f} MB, returned {returned / 2**20:.1f} MB, workspace {ws / 2**20:.1f} MB')
    assert grown <= returned + ws + 2**20
    assert 4 * Nq * N * 4 == 512 * 2**20 and grown < 512 * 2**20 / 4


# ---- probe end to end -----------------------------------------------------------------------------------------------------------

def _cfg(d):
    import train
    return train._wrap(d)


NCLS = 8


@pytest.fixture(scope='module')
def micro():
    from deepavfusion_amd.build_model import build_avmae
    from deepavfusion_amd.configs import CONFIGS
    from deepavfusion_amd.util.knn_probe import SyntheticLabelledAV
    cfg = CONFIGS['micro']
    torch.manual_seed(0)
    model = build_avmae(cfg).to(DEV)
    ds = SyntheticLabelledAV(256, NCLS, cfg.image_size, cfg.audio_size, seed=1, noise=1.5)
    return cfg, model, ds


def _probe(ds, **over):
    from deepavfusion_amd.util.knn_probe import EvalAVNNProbe
    bank = over.pop('bank_dataset', None)
    return EvalAVNNProbe(_cfg({'dataset': None, 'batch_size': 64, **over}), _cfg({'eval_freq': 1, 'print_freq': 10}),
                         _cfg({'seed': 0, 'workers': 0}), dataset=ds, bank_dataset=bank)


def test_probe_weighted_vote_end_to_end(micro):
    cfg, model, ds = micro
    k = 20
    probe = _probe(ds, k=k, bank_samples=512)
    out = probe.evaluate(model)
    mods = ('audio', 'image', 'fusion', 'all')
    assert list(out) == [f'{m}_nn_acc' for m in mods] + [f'{m}_knn20_acc' for m in mods]
    assert probe.evaluate(model) == out                                  # repeatable bit for bit
    plain = _probe(ds).evaluate(model)
    assert list(plain) == [f'{m}_nn_acc' for m in mods] and all(out[key] == plain[key] for key in plain)     # k: null -> today's dict
    v, a, mm, labels = probe.extract(model)
    bv, ba, bmm, bank_labels = probe.extract_bank(model)
    assert bv.shape == (512, cfg.embed_dim) and labels.shape == (256,)
    assert torch.equal(bank_labels.cpu(), (torch.arange(512) + 256) % NCLS)          # the next 512 clips, in order
    # float64 restatement on the probe's own features
    S, Bd = _knn_ref((v, a, mm), (bv, ba, bmm), 1)
    share = {}
    for mod, view, m_v in (('image', 0, 1), ('audio', 1, 1), ('fusion', 2, 1), ('all', 3, 3)):
        s, b = S[view], Bd[view].max()
        top = torch.topk(s, k + 1, dim=1)
        x = top.values[:, :k] / (T * m_v)
        w = torch.exp(x)
        hot = torch.nn.functional.one_hot(bank_labels[top.indices[:, :k]], NCLS).double()
        votes = torch.einsum('qj,qjc->qc', w, hot)
        # a weight is off by the score's error through the exponent, b / (T m_v), and by the kernel's own arithmetic (_vote_ref)
        vb = torch.einsum('qj,qjc->qc', w * (b / (T * m_v) + U32 * (x.abs() + 2 + k)), hot)
        best = torch.topk(votes, 2, dim=1)
        unclear = ((top.values[:, k - 1] - top.values[:, k]) <= 2 * b) | \
            ((best.values[:, 0] - best.values[:, 1]) <= 2 * torch.gather(vb, 1, best.indices).sum(1))
        share[mod] = float(unclear.double().mean())
        acc = float((_argmax_low(votes) == labels).double().mean() * 100)
        assert abs(out[f'{mod}_knn20_acc'] - acc) <= 100.0 * share[mod] + 1e-9, (mod, out, acc, share)
    print(f'probe micro {out} (chance {100 / NCLS:.1f} %); share of queries inside the bound {share}')
    assert min(out[f'{m}_knn20_acc'] for m in mods) > 2 * 100 / NCLS
    # without a bank: the eval set against itself, own clip excluded
    own = _probe(ds, k=k).evaluate(model)
    assert list(own) == list(out) and min(own[f'{m}_knn20_acc'] for m in mods) > 2 * 100 / NCLS


class _MultiHot(torch.utils.data.Dataset):
    """own class + the next one for every third clip, two classes never set"""

    def __init__(self, base):
        self.base = base

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        image, spec, anno = self.base[i]
        c = anno['class']
        lab = torch.zeros(NCLS + 2, dtype=torch.int64)
        lab[c] = 1
        if i % 3 == 0:
            lab[(c + 1) % NCLS] = 1
        return image, spec, {'class': lab}


def test_probe_weighted_vote_multi_label(micro):
    metrics = pytest.importorskip('sklearn.metrics')
    from deepavfusion_amd.util.knn_probe import SyntheticLabelledAV, knn_vote_predictions
    cfg, model, ds = micro
    bank = SyntheticLabelledAV(512, NCLS, cfg.image_size, cfg.audio_size, seed=1, noise=1.5, offset=256)
    probe = _probe(_MultiHot(ds), k=20, bank_dataset=_MultiHot(bank))
    out = probe.evaluate(model)
    mods = ('audio', 'image', 'fusion', 'all')
    assert list(out) == [f'{m}_nn_{x}' for m in mods for x in ('ap', 'auc')] + [f'{m}_knn20_{x}' for m in mods for x in ('ap', 'auc')]
    *feats, labels = probe.extract(model)
    *bfeats, bank_labels = probe.extract_bank(model)
    votes = knn_vote_predictions(tuple(feats), tuple(bfeats), bank_labels, NCLS + 2, 20, T, exclude_self=False)
    y = labels.cpu().numpy()
    seen = y.sum(0) > 0
    assert seen.sum() == NCLS
    for m in mods:
        sc = votes[m][0].cpu().numpy()
        assert votes[m][1] is None and sc.shape == y.shape
        assert abs(out[f'{m}_knn20_ap'] - metrics.average_precision_score(y[:, seen], sc[:, seen], average=None).mean()) <= 1e-12
        assert abs(out[f'{m}_knn20_auc'] - metrics.roc_auc_score(y[:, seen], sc[:, seen], average=None).mean()) <= 1e-12
        assert out[f'{m}_knn20_auc'] > 0.6
