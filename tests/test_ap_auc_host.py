"""Host side of the multi-label probe metrics on the device (csrc/probe/ap_auc.hip, deepavfusion_amd/util/knn_probe.py): the header
and the C-ABI error contract of dav_ap_auc_f64, the workspace formula, the wrapper's argument checks, the nn_probe.metrics key and
the host half of the device path against probe_metrics / vote_metrics.  No GPU needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENTRY = 'dav_ap_auc_f64'


def _header():
    return open(os.path.join(ROOT, 'include', 'dav_kernels.h')).read()


def _doc():
    hdr = _header()
    return hdr[:hdr.index(f'int {ENTRY}(')].rsplit('/*', 2)[1]        # the comment in front of the enum and the declaration


def test_header_declares_the_entry_point_and_its_capacity():
    from deepavfusion_amd import _lib, ops
    hdr = _header()
    assert f'int {ENTRY}(' in hdr and ENTRY in _lib.SIGNATURES
    m = re.search(r'enum \{ dav_ap_auc_max_rows = (\d+) \};', hdr)
    assert m and int(m.group(1)) == ops.AP_AUC_MAX_ROWS >= 32768
    assert '#define DAV_ABI_VERSION 9 ' in hdr and _lib.ABI_VERSION == 9
    doc = _doc()
    assert '-1:' in doc and '-3:' in doc and '-5:' in doc
    assert not any('ap_auc' in n and 'workspace' in n for n in _lib.SIGNATURES)      # priced in Python, from the header's formula


def _call(**over):
    from deepavfusion_amd import _lib
    args = [None if t is C.c_void_p else t(0) for t in _lib.SIGNATURES[ENTRY]]
    for k, v in over.items():
        args[int(k[1:])] = v
    return getattr(_lib.load(), ENTRY)(*args)


def test_cabi_error_contract():
    p, i, l, sz = C.c_void_p, C.c_int, C.c_long, C.c_size_t
    from deepavfusion_amd import ops
    # dav_ap_auc_f64(y @0, ldy @1, n @2, C @3, V @4, scores @5, score_rs @6, score_vs @7, nbr @8, nbr_val @9, nbr_labels @10, N @11,
    #                ap @12, auc @13, pos @14, workspace @15, workspace_bytes @16, stream); no pointer is ever dereferenced here
    n, Cc, V = 1000, 130, 4
    need = Cc * ((n + 31) // 32) * 4
    base = dict(a0=p(4096), a1=l(Cc), a2=i(n), a3=i(Cc), a4=i(V), a12=p(8192), a13=p(12288), a14=p(16384), a15=p(20480), a16=sz(need))
    dense = dict(base, a5=p(24576), a6=l(Cc), a7=l(n * Cc))
    neigh = dict(base, a8=p(28672), a9=p(32768), a10=p(36864), a11=i(500))
    assert _call() == -1                                                           # empty
    both = dict(dense, a8=p(28672), a9=p(32768), a10=p(36864), a11=i(500))
    for ok in (dense, neigh):
        for bad in (dict(a2=i(0)), dict(a3=i(0)), dict(a4=i(0)), dict(a2=i(-1)), dict(a4=i(5)), dict(a1=l(Cc - 1)),
                    dict(a2=i(ops.AP_AUC_MAX_ROWS + 1), a16=sz(1 << 30)), dict(a0=p(0)), dict(a12=p(0)), dict(a13=p(0)), dict(a14=p(0))):
            assert _call(**{**ok, **bad}) == -1, bad
        assert _call(**{**ok, 'a16': sz(need - 1)}) == -3                          # short workspace
        assert _call(**{**ok, 'a15': p(0)}) == -3                                  # no workspace
        for bad in (dict(a12=p(8192 + 4)), dict(a13=p(12288 + 4)), dict(a14=p(16384 + 2)), dict(a15=p(20480 + 2))):
            assert _call(**{**ok, **bad}) == -5, bad
    assert _call(**base) == -1                                                     # neither form
    assert _call(**both) == -1                                                     # both forms
    assert _call(**dict(dense, a10=p(36864))) == -1                                # dense scores and a part of the other form
    assert _call(**dict(dense, a6=l(Cc - 1))) == -1                                # score rows narrower than C
    for bad in (dict(a10=p(0)), dict(a8=p(0)), dict(a9=p(0)), dict(a11=i(0))):     # the neighbour form without one of its parts
        assert _call(**{**neigh, **bad}) == -1, bad
    assert _call(**dict(dense, a5=p(24576 + 2))) == -5
    assert _call(**dict(neigh, a8=p(28672 + 2))) == -5
    assert _call(**dict(neigh, a9=p(32768 + 1))) == -5
    # the capacity itself is in range: with everything else valid the next check (the workspace) answers
    assert _call(**dict(dense, a2=i(ops.AP_AUC_MAX_ROWS), a16=sz(need))) == -3


def test_workspace_helper_equals_the_header_formula():
    from deepavfusion_amd import ops
    m = re.search(r'workspace_bytes >= (C \* \(\(n \+ 31\) / 32\) \* 4)', _doc())
    assert m, 'the header documents the workspace of dav_ap_auc_f64 as a closed formula'
    formula = m.group(1).replace('/', '//')
    for V, n, Cc in ((4, 20000, 527), (1, 33, 3), (2, 1, 1)):
        assert ops.ap_auc_workspace_bytes(V, n, Cc) == eval(formula, {'C': Cc, 'n': n, 'V': V})
    assert ops.ap_auc_workspace_bytes(4, 20000, 527) == 527 * 625 * 4


def test_wrapper_refuses_bad_arguments_before_any_launch():
    from deepavfusion_amd import ops
    n, Cc, N = 12, 5, 30
    y = torch.zeros(n, Cc, dtype=torch.uint8)
    sc = torch.zeros(4, n, Cc)
    nbr, val, lab = torch.zeros(4, n, dtype=torch.int64), torch.zeros(4, n), torch.zeros(N, Cc, dtype=torch.uint8)
    bad = [
        dict(y=y),                                                                  # neither form
        dict(y=y, scores=sc, nbr=nbr, nbr_val=val, nbr_labels=lab),                 # both
        dict(y=y, scores=sc, nbr_labels=lab),                                       # dense and a part of the other
        dict(y=y, nbr=nbr, nbr_val=val),                                            # no bank labels
        dict(y=y, nbr=nbr, nbr_labels=lab),
        dict(y=y.long(), scores=sc),                                                # truth must be uint8
        dict(y=y.t(), scores=sc.transpose(1, 2)),                                   # unit column stride
        dict(y=y, scores=sc.double()),
        dict(y=y, scores=sc[:, :-1]),                                               # another row count
        dict(y=y, scores=torch.zeros(5, n, Cc)),                                    # five views
        dict(y=y, scores=torch.zeros(4, n, 2 * Cc)[:, :, ::2]),                     # strided columns
        dict(y=y, nbr=nbr.float(), nbr_val=val, nbr_labels=lab),
        dict(y=y, nbr=nbr, nbr_val=val[:3], nbr_labels=lab),
        dict(y=y, nbr=nbr, nbr_val=val, nbr_labels=lab.long()),
        dict(y=y, nbr=nbr, nbr_val=val, nbr_labels=lab[:, :-1]),
        dict(y=torch.zeros(ops.AP_AUC_MAX_ROWS + 1, 1, dtype=torch.uint8), scores=torch.zeros(1, ops.AP_AUC_MAX_ROWS + 1, 1)),
        dict(y=torch.zeros(0, Cc, dtype=torch.uint8), scores=torch.zeros(1, 0, Cc)),
        dict(y=y, scores=sc, out=(torch.zeros(4, Cc), torch.zeros(4, Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.int32))),
        dict(y=y, scores=sc, workspace=torch.zeros(ops.ap_auc_workspace_bytes(4, n, Cc) - 1, dtype=torch.uint8)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.ap_auc(kw.pop('y'), kw.pop('scores', None), **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                      # valid arguments reach the launch
        ops.ap_auc(y, sc)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ap_auc(y, torch.zeros(4, n, Cc + 3)[:, :, :Cc])                         # a view of wider rows is accepted
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ap_auc(y, nbr=nbr, nbr_val=val, nbr_labels=lab)


def test_config_composes_metrics_host_by_default():
    import train
    from deepavfusion_amd.util.knn_probe import metrics_mode
    assert train.load_config('deepavfusion', []).nn_probe.metrics == 'host'
    assert train.load_config('deepavfusion', ['nn_probe.metrics=device']).nn_probe.metrics == 'device'
    assert metrics_mode('host') == metrics_mode(None) == 'host' and metrics_mode('device') == 'device'
    for bad in ('gpu', 'Device', '', 0, True):
        with pytest.raises(ValueError, match='nn_probe.metrics'):
            metrics_mode(bad)


def test_where_the_metrics_run():
    from deepavfusion_amd import ops
    from deepavfusion_amd.util.knn_probe import metrics_on_device
    assert metrics_on_device('device', True, 18000) and metrics_on_device('device', True, ops.AP_AUC_MAX_ROWS)
    assert not metrics_on_device('device', True, ops.AP_AUC_MAX_ROWS + 1)           # too many clips for a column: the host path
    assert not metrics_on_device('device', False, 100)                             # single-label sets ignore the key
    assert not metrics_on_device('host', True, 100) and not metrics_on_device(None, True, 100)
    with pytest.raises(ValueError):
        metrics_on_device('both', True, 100)


def _columns(y, scores):
    """ap / auc [V, C] and pos [C] as the kernel defines them, from the yardstick: NaN where roc_auc raises, columns without a
    positive included (AP 0.0 there)."""
    from deepavfusion_amd.util.knn_probe import average_precision, roc_auc
    V, n, Cc = scores.shape
    ap, auc = np.empty((V, Cc)), np.full((V, Cc), np.nan)
    for v in range(V):
        ap[v] = average_precision(y, scores[v])
        for c in range(Cc):
            if 0 < y[:, c].sum() < n:
                auc[v, c] = roc_auc(y[:, c:c + 1], scores[v][:, c:c + 1])[0]
    return ap, auc, y.sum(0).astype(np.int32)


def test_host_half_of_the_device_path_equals_the_host_metrics():
    from deepavfusion_amd.util.knn_probe import _VIEW, MODALITIES, device_metrics, probe_metrics, vote_metrics
    rng = np.random.default_rng(5)
    n, Cc = 40, 7
    y = (rng.random((n, Cc)) < 0.3).astype(np.int64)
    y[:, 2] = 0                                                                     # never occurs: dropped by the seen mask
    y[:, 5] = 0
    assert (y.sum(0) > 0).sum() == Cc - 2 and (y.sum(0) < n).all()
    # the vote scores, one dense [n, C] per view
    dense = rng.random((4, n, Cc)).astype(np.float32)
    ref = vote_metrics({m: dense[_VIEW[m]] for m in MODALITIES}, None, y, True, 20)
    got = device_metrics(*_columns(y, dense), 'knn20')
    assert list(got) == list(ref) == [f'{m}_knn20_{x}' for m in MODALITIES for x in ('ap', 'auc')]
    assert got == ref
    # the reference protocol: the labels of one neighbour times its score
    nbr = rng.integers(0, n, (4, n))
    val = rng.standard_normal((4, n)).astype(np.float32)
    ref = probe_metrics({m: (y[nbr[_VIEW[m]]], val[_VIEW[m]]) for m in MODALITIES}, y, True)
    prod = np.stack([y[nbr[v]] * val[v][:, None] for v in range(4)])
    got = device_metrics(*_columns(y, prod), 'nn')
    assert list(got) == list(ref) == [f'{m}_nn_{x}' for m in MODALITIES for x in ('ap', 'auc')]
    assert got == ref
    # a class that every clip has: the kernel's NaN becomes the restatement's error; the same NaN on an unseen class is ignored
    y2 = y.copy()
    y2[:, 1] = 1
    with pytest.raises(ValueError, match='Only one class present'):
        vote_metrics({m: dense[_VIEW[m]] for m in MODALITIES}, None, y2, True, 20)
    ap, auc, pos = _columns(y2, dense)
    assert np.isnan(auc[:, [1, 2, 5]]).all() and np.isnan(auc).sum() == 12
    with pytest.raises(ValueError, match='Only one class present'):
        device_metrics(ap, auc, pos, 'knn20')
