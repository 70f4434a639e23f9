"""Host side of the weighted k-NN probe (csrc/probe/knn_wide.hip, deepavfusion_amd/util/knn_probe.py): the new nn_probe keys, the
C-ABI error contract of dav_knn_topk_wide_f32 / dav_knn_vote_f32, the workspace formula, the shifted synthetic set and the metric
keys of the vote.  No GPU needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_config_composes_the_vote_keys_off_by_default():
    import train
    p = train.load_config('deepavfusion', []).nn_probe
    assert p.k is None and p.bank_partition is None and p.bank_samples is None
    assert p.temperature == 0.07 and isinstance(p.temperature, float)
    p = train.load_config('deepavfusion', ['nn_probe.dataset=shards', 'nn_probe.k=20', 'nn_probe.temperature=0.1',
                                           'nn_probe.bank_partition=train']).nn_probe
    assert (p.k, p.temperature, p.bank_partition, p.bank_samples) == (20, 0.1, 'train', None) and isinstance(p.k, int)
    p = train.load_config('deepavfusion', ['nn_probe.dataset=synthetic', 'nn_probe.k=10', 'nn_probe.bank_samples=2048']).nn_probe
    assert (p.k, p.bank_samples, p.bank_partition) == (10, 2048, None) and isinstance(p.bank_samples, int)


def _call(name, **over):
    from deepavfusion_amd import _lib
    args = [None if t is C.c_void_p else t(0) for t in _lib.SIGNATURES[name]]
    for k, v in over.items():
        args[int(k[1:])] = v
    return getattr(_lib.load(), name)(*args)


def test_cabi_error_contract_of_the_wide_topk():
    p, i, l, sz = C.c_void_p, C.c_int, C.c_long, C.c_size_t
    # dav_knn_topk_wide_f32(q0, x0, q1, x1, q2, x2, M @6, Nq, N, D, ldq @10, ldx, sum_view @12, k @13, splits @14, top_val @15,
    #                       top_idx, workspace @17, workspace_bytes @18, stream)
    name = 'dav_knn_topk_wide_f32'
    Nq, N, D, M, V, k, S = 37, 129, 64, 3, 4, 20, 2
    need = S * V * Nq * k * 8
    kn = dict(a0=p(4096), a1=p(8192), a2=p(12288), a3=p(16384), a4=p(20480), a5=p(24576), a6=i(M), a7=i(Nq), a8=i(N), a9=i(D),
              a10=l(D), a11=l(D), a12=i(1), a13=i(k), a14=i(S), a15=p(28672), a16=p(32768), a17=p(36864), a18=sz(need))
    assert _call(name) == -1                                                       # empty
    for bad in (dict(a7=i(0)), dict(a8=i(0)), dict(a9=i(0)), dict(a6=i(0)), dict(a6=i(4)), dict(a13=i(0)), dict(a13=i(65)),
                dict(a8=i(19)), dict(a14=i(0)), dict(a14=i(65536)), dict(a12=i(2)), dict(a9=i(62), a10=l(64), a11=l(64)),
                dict(a10=l(32)), dict(a4=p(0)), dict(a15=p(0)), dict(a16=p(0))):
        assert _call(name, **{**kn, **bad}) == -1, bad
    for bad in (dict(a0=p(4096 + 4)), dict(a5=p(24576 + 8)), dict(a10=l(66)), dict(a11=l(70)), dict(a17=p(36864 + 4)),
                dict(a15=p(28672 + 2))):
        assert _call(name, **{**kn, **bad}) == -5, bad
    assert _call(name, **{**kn, 'a18': sz(need - 1)}) == -3                        # short workspace
    assert _call(name, **{**kn, 'a13': i(64), 'a18': sz(need)}) == -3              # k = 64 is in range; its workspace is larger
    assert _call(name, **{**kn, 'a12': i(0), 'a18': sz(S * M * Nq * k * 8 - 8)}) == -3
    assert _call(name, **{**kn, 'a17': p(0)}) == -3
    # the narrow entry point still refuses what the wide one takes
    assert _call('dav_knn_topk_f32', **{**kn, 'a13': i(9)}) == -1


def test_cabi_error_contract_of_the_vote():
    p, i = C.c_void_p, C.c_int
    # dav_knn_vote_f32(top_val, top_idx, V @2, Nq, kk @4, k @5, labels @6, multihot @7, N @8, C @9, inv_t @10, self_offset @11,
    #                  scores @12, pred @13, stream)
    name = 'dav_knn_vote_f32'
    inv_t = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    host = C.cast(inv_t, C.c_void_p)
    ok = dict(a0=p(4096), a1=p(8192), a2=i(4), a3=i(130), a4=i(21), a5=i(20), a6=p(12288), a8=i(1000), a9=i(10), a10=host,
              a11=i(-1), a12=p(16384), a13=p(20480))
    assert _call(name) == -1                                                       # empty
    for bad in (dict(a2=i(0)), dict(a2=i(5)), dict(a3=i(0)), dict(a4=i(0)), dict(a5=i(0)), dict(a5=i(22)), dict(a4=i(70), a5=i(65)),
                dict(a8=i(0)), dict(a9=i(0)), dict(a6=p(0)), dict(a7=p(24576)), dict(a0=p(0)), dict(a1=p(0)), dict(a10=p(0)),
                dict(a12=p(0)), dict(a13=p(0)), dict(a11=i(-2)), dict(a5=i(21), a11=i(0))):
        assert _call(name, **{**ok, **bad}) == -1, bad
    for bad in (dict(a0=p(4096 + 2)), dict(a1=p(8192 + 1)), dict(a6=p(12288 + 2)), dict(a12=p(16384 + 2)), dict(a13=p(20480 + 2))):
        assert _call(name, **{**ok, **bad}) == -5, bad
    # the header states each case
    hdr = open(os.path.join(ROOT, 'include', 'dav_kernels.h')).read()
    for entry in ('dav_knn_topk_wide_f32', 'dav_knn_vote_f32'):
        doc = hdr[:hdr.index(f'int {entry}(')].rsplit('/*', 1)[1]
        assert '-1:' in doc and '-5:' in doc and ('-3:' in doc or entry.endswith('vote_f32')), entry


def test_workspace_helper_equals_the_header_formula():
    from deepavfusion_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'dav_kernels.h')).read()
    doc = hdr[:hdr.index('int dav_knn_topk_wide_f32(')].rsplit('/*', 1)[1]
    m = re.search(r'workspace_bytes >= (splits \* V \* Nq \* k \* 8)', doc)
    assert m, 'the header documents the workspace of dav_knn_topk_wide_f32 as a closed formula'
    for Nq, V, k, splits in ((37, 4, 20, 2), (15440, 4, 21, 5), (1, 1, 64, 1), (2048, 3, 9, 32)):
        assert ops.knn_workspace_bytes(Nq, V, k, splits) == eval(m.group(1))
    assert 'dav_knn_wide_workspace_bytes' not in _lib.SIGNATURES and not any('knn' in n and 'workspace' in n for n in _lib.SIGNATURES)
    assert ops.KNN_MAX_K == 64 and ops.KNN_NARROW_K == 8


def test_knn_vote_wrapper_refuses_bad_arguments_before_any_launch():
    from deepavfusion_amd import ops
    val, idx = torch.zeros(4, 5, 21), torch.zeros(4, 5, 21, dtype=torch.int32)
    ids = torch.zeros(100, dtype=torch.int32)
    for kw in (dict(k=21, self_offset=0), dict(k=22), dict(k=0), dict(k=20, inv_t=[1.0] * 3)):
        args = dict(k=20, inv_t=[1.0] * 4, self_offset=-1)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.knn_vote(val, idx, ids, 10, args['k'], args['inv_t'], self_offset=args['self_offset'])
    with pytest.raises(ValueError):
        ops.knn_vote(val, idx, torch.zeros(100, 10), 10, 20, [1.0] * 4)             # multi-hot must be uint8
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.knn_vote(val, idx, ids, 10, 20, [1.0] * 4)


def test_synthetic_set_offset():
    from deepavfusion_amd.util.knn_probe import SyntheticLabelledAV
    base = SyntheticLabelledAV(12, 5, (16, 16), (8, 16), seed=3)
    same = SyntheticLabelledAV(12, 5, (16, 16), (8, 16), seed=3, offset=0)
    shifted = SyntheticLabelledAV(4, 5, (16, 16), (8, 16), seed=3, offset=7)
    assert len(shifted) == 4
    for i in range(12):
        for x, y in zip(base[i], same[i]):
            assert x == y if isinstance(x, dict) else torch.equal(x, y)
    for i in range(4):
        image, spec, anno = shifted[i]
        ref = base[7 + i]
        assert torch.equal(image, ref[0]) and torch.equal(spec, ref[1]) and anno == ref[2] == {'class': (7 + i) % 5}
    assert not torch.equal(shifted[0][0], base[0][0])


def test_vote_metric_keys():
    from deepavfusion_amd.util.knn_probe import MODALITIES, average_precision, roc_auc, vote_metrics
    labels = np.array([0, 1, 2, 1])
    scores = {m: np.eye(3)[[0, 1, 2, 1]] for m in MODALITIES}
    preds = {m: np.array(p) for m, p in zip(MODALITIES, ([0, 1, 2, 1], [0, 0, 2, 1], [2, 2, 0, 0], [0, 1, 1, 1]))}
    out = vote_metrics(scores, preds, labels, False, 20)
    assert list(out) == ['audio_knn20_acc', 'image_knn20_acc', 'fusion_knn20_acc', 'all_knn20_acc']
    assert [out[k] for k in out] == [100.0, 75.0, 0.0, 75.0]
    ml = np.array([[1, 0, 0, 0], [0, 1, 1, 0], [1, 1, 0, 0], [0, 0, 1, 0]])        # class 3 never occurs among the queries
    rng = np.random.default_rng(0)
    sc = {m: rng.random((4, 4)) for m in MODALITIES}
    out = vote_metrics(sc, None, ml, True, 5)
    assert list(out) == [f'{m}_knn5_{x}' for m in MODALITIES for x in ('ap', 'auc')]
    for m in MODALITIES:
        assert out[f'{m}_knn5_ap'] == float(average_precision(ml[:, :3], sc[m][:, :3]).mean())
        assert out[f'{m}_knn5_auc'] == float(roc_auc(ml[:, :3], sc[m][:, :3]).mean())
