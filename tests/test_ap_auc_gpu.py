"""dav_ap_auc_f64 on the device (csrc/probe/ap_auc.hip) through ops.ap_auc: every element of ap / auc / pos against the numpy
restatement of sklearn in util/knn_probe.py (average_precision / roc_auc, themselves held to sklearn within 1e-12 by
test_knn_probe_host.py), outputs poisoned, outputs and workspace in guarded buffers; the neighbour form against the dense form on
the materialised product bit for bit; repeatability; and the probe end to end with nn_probe.metrics=device against metrics=host.

Tolerance of a column: 4 n 2^-53 absolute.  Each side sums at most n non-negative terms whose total is <= 1, every term carries a
few roundings and every addition one: <= (n + 3) 2^-53 per side, and the two sides add in different orders.

The design's internal boundaries, all among the row counts: a wave (64), the workgroup (1024: rows per trip of the load loop, pairs
per trip of the sort), a word of the truth mask (32), and powers of two of the two sorted runs — the positives and the negatives of
a column, whose lengths are built to 63 / 64 / 65 in six columns of the 130-class cases."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kcheck import Guarded, exact, within  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'

FAMILIES = ('continuous', 'eighths', 'equal', 'zeros', 'negative', 'subnormal')


def _truth(rng, n, C):
    """uint8 [n, C] and the set of columns BUILT with one class only.  Every other column gets at least one positive and one
    negative by construction.  130 classes: column 0 no positive, 1 all positive, 2 exactly one positive, 3 exactly one negative,
    4-6 with 63 / 64 / 65 positives, 7-9 with 63 / 64 / 65 negatives (n >= 130)."""
    y = (rng.random((n, C)) < 0.3).astype(np.uint8)
    built = np.zeros(C, bool)
    if n == 1:
        built[:] = True
        return y, built
    for c in range(C):
        r = rng.choice(n, 2, replace=False)
        y[r[0], c], y[r[1], c] = 1, 0
    if C == 130:
        y[:, 0], y[:, 1] = 0, 1
        built[:2] = True
        y[:, 2] = 0
        y[rng.integers(n), 2] = 1
        y[:, 3] = 1
        y[rng.integers(n), 3] = 0
        if n >= 130:
            for c, m in zip(range(4, 10), (63, 64, 65, 63, 64, 65)):
                col = np.zeros(n, np.uint8)
                col[rng.choice(n, m, replace=False)] = 1
                y[:, c] = col if c < 7 else 1 - col
    pos = y.sum(0)
    assert np.array_equal((pos == 0) | (pos == n), built)           # the yardstick has no other degenerate column
    return y, built


def _scores(rng, family, V, n, C):
    s = rng.standard_normal((V, n, C)).astype(np.float32)
    if family == 'eighths':                                        # most thresholds tied
        s = (np.round(s * 8) / 8).astype(np.float32)
    elif family == 'equal':
        s[:] = np.float32(0.25)
    elif family == 'zeros':                                        # more than half zeros of both signs
        z = rng.random(s.shape)
        s[z < 0.35] = np.float32(0.0)
        s[z > 0.70] = np.float32(-0.0)
    elif family == 'negative':
        s = -np.abs(s) - np.float32(1.0)
    elif family == 'subnormal':                                    # 0, +-1, +-2, +-3 units of 2^-149, both zeros
        bits = rng.integers(0, 4, s.shape).astype(np.uint32) | (rng.integers(0, 2, s.shape).astype(np.uint32) << np.uint32(31))
        s = bits.view(np.float32)
        if s.size >= 500:                                          # both zeros occur, and nothing was flushed on the way
            assert np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all() and len(np.unique(s)) == 7
    return np.ascontiguousarray(s)


def _yardstick(y, scores):
    """ap / auc [V, C] from knn_probe.average_precision / roc_auc (NaN where roc_auc raises: one class only) and pos [C]."""
    from deepavfusion_amd.util.knn_probe import average_precision, roc_auc
    V, n, C = scores.shape
    pos = y.sum(0).astype(np.int32)
    two = (pos > 0) & (pos < n)
    ap, auc = np.empty((V, C)), np.full((V, C), np.nan)
    for v in range(V):
        ap[v] = average_precision(y, scores[v])
        if two.any():
            auc[v, two] = roc_auc(y[:, two], scores[v][:, two])
    return ap, auc, pos


class _Out:
    """ap / auc / pos poisoned in guarded buffers, and a guarded workspace of exactly the documented size."""

    def __init__(self, V, n, C):
        from deepavfusion_amd import ops
        self.ap = Guarded(V, C, torch.float64, device=DEV)
        self.auc = Guarded(V, C, torch.float64, device=DEV)
        self.pos = Guarded(1, C, torch.int32, device=DEV)
        self.ws = Guarded(1, ops.ap_auc_workspace_bytes(V, n, C), torch.uint8, device=DEV, fill=0x5A)

    def kw(self):
        return dict(out=(self.ap.t, self.auc.t, self.pos.t[0]), workspace=self.ws.t[0])

    def no_stray(self, tag):
        for name in ('ap', 'auc', 'pos', 'ws'):
            n_stray, where = getattr(self, name).stray()
            assert n_stray == 0, f'{tag} {name}: {where}'


def _check(tag, got, y, scores, built):
    """every element of (ap, auc, pos) on the device against the yardstick of (y, scores) on the host"""
    ap, auc, pos = (t.cpu() for t in got)
    rap, rauc, rpos = _yardstick(y, scores)
    n = y.shape[0]
    bound = 4 * n * 2.0 ** -53
    assert torch.equal(pos, torch.from_numpy(rpos)), f'{tag} pos'
    ok, worst_ap, msg = within(ap, torch.from_numpy(rap), bound, f'{tag} ap')
    assert ok, msg
    nan = torch.isnan(auc)
    expect = torch.from_numpy(np.broadcast_to(built, auc.shape).copy())
    assert torch.equal(nan, expect), f'{tag}: NaN AUC in columns {nan.nonzero().tolist()}, built {expect.nonzero().tolist()}'
    assert np.array_equal(np.isnan(rauc), expect.numpy())
    fin = ~nan
    ok, worst_auc, msg = within(auc[fin], torch.from_numpy(rauc)[fin], bound, f'{tag} auc')
    assert ok, msg
    return max(worst_ap, worst_auc)


def _dev_view(a, pad):
    """the array on the device as a view whose rows are ``pad`` elements wider than its last dimension"""
    t = torch.from_numpy(a)
    if not pad:
        return t.to(DEV)
    wide = torch.full(tuple(a.shape[:-1]) + (a.shape[-1] + pad,), 7, dtype=t.dtype, device=DEV)
    wide[..., :a.shape[-1]] = t.to(DEV)
    return wide[..., :a.shape[-1]]


def _run_dense(n, C, V, seed):
    from deepavfusion_amd import ops
    rng = np.random.default_rng(seed)
    y, built = _truth(rng, n, C)
    pad = 5 if V == 4 else 0                                        # the four-view cases read views of wider rows
    yd = _dev_view(y, pad)
    worst = 0.0
    for fam in FAMILIES:
        s = _scores(rng, fam, V, n, C)
        o = _Out(V, n, C)
        got = ops.ap_auc(yd, _dev_view(s, pad), **o.kw())
        tag = f'n={n} C={C} V={V} {fam}'
        worst = max(worst, _check(tag, got, y, s, built))
        o.no_stray(tag)
    return worst


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 1000, 1023, 1024, 1025, 2047, 2048, 2049])
def test_dense_form_every_element(n):
    worst = 0.0
    for C in (1, 3, 130):
        for V in (1, 4):
            worst = max(worst, _run_dense(n, C, V, seed=1000 * n + 10 * C + V))
    print(f'ap_auc dense n={n}: worst err / bound {worst:.3g}')


def test_dense_form_at_the_capacity():
    from deepavfusion_amd import ops
    worst = _run_dense(ops.AP_AUC_MAX_ROWS, 3, 1, seed=7)
    print(f'ap_auc dense n={ops.AP_AUC_MAX_ROWS}: worst err / bound {worst:.3g}')


@pytest.mark.parametrize('n,C,V', [(1, 3, 1), (65, 1, 4), (1000, 130, 4), (1025, 3, 1), (2049, 130, 1)])
def test_neighbour_form_equals_the_dense_form_on_the_product(n, C, V):
    """nbr_labels[nbr] * nbr_val is formed in the kernel: the same bits as the dense form on the materialised fp32 product (which
    holds -0.0 wherever a negative value meets a zero label), and both within the bound of the yardstick.  An index outside the
    bank has no label: a zero score."""
    from deepavfusion_amd import ops
    rng = np.random.default_rng(31 * n + C + V)
    y, built = _truth(rng, n, C)
    N = 300
    bank = (rng.random((N, C)) < 0.4).astype(np.uint8)
    nbr = rng.integers(0, N, (V, n))
    if n > 2:
        nbr[0, 0], nbr[V - 1, n - 1] = -1, N                        # outside the bank on either side
    val = rng.standard_normal((V, n)).astype(np.float32)           # cosine similarities of either sign
    inside = (nbr >= 0) & (nbr < N)
    lab = bank[np.clip(nbr, 0, N - 1)] * inside[..., None]
    prod = (lab.astype(np.float32) * val[..., None]).astype(np.float32)
    assert n < 3 or (np.signbit(prod) & (prod == 0)).any()          # -0.0 does arise
    yd = torch.from_numpy(y).to(DEV)
    tag = f'n={n} C={C} V={V}'
    od, on, on32 = _Out(V, n, C), _Out(V, n, C), _Out(V, n, C)
    dense = ops.ap_auc(yd, torch.from_numpy(prod).to(DEV), **od.kw())
    args = dict(nbr_val=torch.from_numpy(val).to(DEV), nbr_labels=torch.from_numpy(bank).to(DEV))
    neigh = ops.ap_auc(yd, nbr=torch.from_numpy(nbr).to(DEV), **args, **on.kw())                       # int64 indices: converted
    neigh32 = ops.ap_auc(yd, nbr=torch.from_numpy(nbr.astype(np.int32)).to(DEV), **args, **on32.kw())
    worst = _check(tag + ' neighbour', neigh, y, prod, built)
    for name, a, b, c in zip(('ap', 'auc', 'pos'), dense, neigh, neigh32):
        for other in (b, c):
            nd, msg = exact(other, a, f'{tag} {name}: neighbour form against dense form')
            assert nd == 0, msg
    for o in (od, on, on32):
        o.no_stray(tag)
    print(f'ap_auc neighbour {tag}: worst err / bound {worst:.3g}')


def test_two_calls_agree_bit_for_bit():
    from deepavfusion_amd import ops
    rng = np.random.default_rng(11)
    n, C, V = 3000, 130, 4
    y, _ = _truth(rng, n, C)
    yd = torch.from_numpy(y).to(DEV)
    for fam in ('continuous', 'eighths'):
        sd = torch.from_numpy(_scores(rng, fam, V, n, C)).to(DEV)
        first = [t.clone() for t in ops.ap_auc(yd, sd)]
        torch.cuda.synchronize()
        again = ops.ap_auc(yd, sd)
        for name, a, b in zip(('ap', 'auc', 'pos'), first, again):
            nd, msg = exact(b, a, f'{fam} {name}: second call against the first')
            assert nd == 0, msg


# ---- the probe end to end -----------------------------------------------------------------------------------------------------

NCLS = 8


def _cfg(d):
    import train
    return train._wrap(d)


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


def _probe(ds, **over):
    from deepavfusion_amd.util.knn_probe import EvalAVNNProbe
    bank = over.pop('bank_dataset', None)
    return EvalAVNNProbe(_cfg({'dataset': None, 'batch_size': 64, **over}), _cfg({'eval_freq': 1, 'print_freq': 10}),
                         _cfg({'seed': 0, 'workers': 0}), dataset=ds, bank_dataset=bank)


def test_probe_metrics_device_equals_host(monkeypatch):
    from deepavfusion_amd import ops
    from deepavfusion_amd.build_model import build_avmae
    from deepavfusion_amd.configs import CONFIGS
    from deepavfusion_amd.util.knn_probe import SyntheticLabelledAV
    cfg = CONFIGS['micro']
    torch.manual_seed(0)
    model = build_avmae(cfg).to(DEV)
    ds = SyntheticLabelledAV(256, NCLS, cfg.image_size, cfg.audio_size, seed=1, noise=1.5)
    bank = SyntheticLabelledAV(512, NCLS, cfg.image_size, cfg.audio_size, seed=1, noise=1.5, offset=256)
    calls = []
    real = ops.ap_auc
    monkeypatch.setattr(ops, 'ap_auc', lambda *a, **kw: (calls.append(sorted(kw)), real(*a, **kw))[1])
    mods = ('audio', 'image', 'fusion', 'all')
    for bank_ds in (_MultiHot(bank), None):                         # a bank of its own; the eval set against itself
        host = _probe(_MultiHot(ds), k=20, bank_dataset=bank_ds, metrics='host').evaluate(model)
        assert not calls
        dev = _probe(_MultiHot(ds), k=20, bank_dataset=bank_ds, metrics='device').evaluate(model)
        assert calls == [['nbr', 'nbr_labels', 'nbr_val'], []]      # one call per protocol: the neighbour form, then the dense form
        calls.clear()
        assert list(dev) == list(host) == [f'{m}_nn_{x}' for m in mods for x in ('ap', 'auc')] + \
            [f'{m}_knn20_{x}' for m in mods for x in ('ap', 'auc')]
        for key in host:
            assert abs(dev[key] - host[key]) <= 1e-12, (key, dev[key], host[key])
        assert all(0.0 < v <= 1.0 for v in dev.values())
    # a set with more clips than a column holds: the host functions, and one warning however often the probe runs
    cap = ops.AP_AUC_MAX_ROWS
    monkeypatch.setattr(ops, 'AP_AUC_MAX_ROWS', 255)
    probe = _probe(_MultiHot(ds), k=20, metrics='device')
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        first, second = probe.evaluate(model), probe.evaluate(model)
    assert sum('nn_probe.metrics=device' in str(w.message) for w in seen) == 1
    assert first == second == host and not calls                    # ``host``: the eval set against itself, from the loop above
    monkeypatch.setattr(ops, 'AP_AUC_MAX_ROWS', cap)
    # a single-label set ignores the key
    host = _probe(ds, k=20, bank_samples=512, metrics='host').evaluate(model)
    dev = _probe(ds, k=20, bank_samples=512, metrics='device').evaluate(model)
    assert dev == host and list(dev) == [f'{m}_nn_acc' for m in mods] + [f'{m}_knn20_acc' for m in mods] and not calls
