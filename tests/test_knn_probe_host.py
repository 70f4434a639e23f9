"""Host side of the nearest-neighbour probe (deepavfusion_amd/util/knn_probe.py, csrc/probe/knn.hip): the AP / AUC restatement,
the nn_probe config group, the C-ABI error contract of dav_mean_l2n_f32 / dav_knn_topk_f32 and the metric dict.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _tied_multilabel(seed, n=300, ncls=12):
    """multi-hot labels with a few classes never seen, and scores as the probe makes them: label of a neighbour x its similarity,
    so most entries are exactly 0 and the rest come in ties"""
    rng = np.random.default_rng(seed)
    labels = (rng.random((n, ncls)) < 0.15).astype(np.int64)
    labels[:, [3, 7]] = 0                                               # unseen classes (removed as the reference does)
    labels[0, :] = 1
    labels[0, [3, 7]] = 0
    labels[1, :] = 0                                                    # every seen class has a negative too
    nb = rng.integers(0, n, n)
    sim = np.round(rng.random(n), 1).astype(np.float32)                 # 11 distinct values: ties everywhere
    scores = labels[nb] * sim[:, None]
    return labels, scores


def test_ap_auc_restatement_matches_sklearn():
    metrics = pytest.importorskip('sklearn.metrics')
    from deepavfusion_amd.util.knn_probe import average_precision, roc_auc
    for seed in range(4):
        labels, scores = _tied_multilabel(seed)
        seen = labels.sum(0) > 0
        assert seen.sum() == labels.shape[1] - 2
        y, s = labels[:, seen], scores[:, seen]
        assert (s == 0).mean() > 0.5
        np.testing.assert_allclose(average_precision(y, s), metrics.average_precision_score(y, s, average=None), rtol=0, atol=1e-12)
        np.testing.assert_allclose(roc_auc(y, s), metrics.roc_auc_score(y, s, average=None), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        roc_auc(np.ones((4, 1), np.int64), np.arange(4.0)[:, None])


def test_config_composes_nn_probe_group_off_by_default():
    import train
    cfg = train.load_config('deepavfusion', [])
    p = cfg.nn_probe
    assert p.dataset is None                                            # probe off
    assert p.batch_size == cfg.opt.batch_size == 64 and isinstance(p.batch_size, int)
    assert (p.audio_rate, p.audio_dur, p.audio_mels, p.image_size, p.crop_min, p.data_path) == \
        (cfg.data.audio_rate, cfg.data.audio_dur, cfg.data.audio_mels, cfg.data.image_size, cfg.data.crop_min, None)
    assert {'num_classes', 'num_samples'} <= set(p) and cfg.log.eval_freq == 10
    cfg = train.load_config('deepavfusion', ['nn_probe.dataset=synthetic', 'opt.batch_size=8', 'data.image_size=64'])
    assert cfg.nn_probe.dataset == 'synthetic' and cfg.nn_probe.batch_size == 8 and cfg.nn_probe.image_size == 64
    assert cfg.job_name == 'deepavfusion_synthetic_ep300_bs8x1x1_blr0.00015'       # interpolations inside text stay text
    assert cfg.opt.pt_warmup_epochs == '300/2'


def _call(name, **over):
    from deepavfusion_amd import _lib
    args = [None if t is C.c_void_p else t(0) for t in _lib.SIGNATURES[name]]
    for k, v in over.items():
        args[int(k[1:])] = v
    return getattr(_lib.load(), name)(*args)


def test_cabi_error_contract_of_the_probe_kernels():
    p, i, l, sz = C.c_void_p, C.c_int, C.c_long, C.c_size_t
    # dav_mean_l2n_f32(x, B, L, D, ld_row, ld_batch, out, stream)
    ok = dict(a0=p(4096), a1=i(2), a2=i(3), a3=i(64), a4=l(64), a5=l(192), a6=p(8192))
    assert _call('dav_mean_l2n_f32') == -1
    assert _call('dav_mean_l2n_f32', **{**ok, 'a2': i(0)}) == -1
    assert _call('dav_mean_l2n_f32', **{**ok, 'a4': l(32)}) == -1                 # row stride below D
    assert _call('dav_mean_l2n_f32', **{**ok, 'a0': p(4098)}) == -5
    # dav_knn_topk_f32(q0, x0, q1, x1, q2, x2, M @6, Nq, N, D, ldq @10, ldx, sum_view @12, k @13, splits @14, top_val @15, top_idx,
    #                  workspace @17, workspace_bytes @18, stream)
    Nq, N, D, M, V, k, S = 37, 129, 64, 3, 4, 2, 2
    need = S * V * Nq * k * 8
    kn = dict(a0=p(4096), a1=p(8192), a2=p(12288), a3=p(16384), a4=p(20480), a5=p(24576), a6=i(M), a7=i(Nq), a8=i(N), a9=i(D),
              a10=l(D), a11=l(D), a12=i(1), a13=i(k), a14=i(S), a15=p(28672), a16=p(32768), a17=p(36864), a18=sz(need))
    assert _call('dav_knn_topk_f32') == -1                                        # empty
    for bad in (dict(a7=i(0)), dict(a8=i(0)), dict(a9=i(0)), dict(a6=i(0)), dict(a6=i(4)), dict(a13=i(0)), dict(a13=i(9)),
                dict(a8=i(1), a13=i(2)), dict(a14=i(0)), dict(a12=i(2)), dict(a9=i(62), a10=l(64), a11=l(64)), dict(a10=l(32)),
                dict(a4=p(0))):
        assert _call('dav_knn_topk_f32', **{**kn, **bad}) == -1, bad
    for bad in (dict(a0=p(4096 + 4)), dict(a5=p(24576 + 8)), dict(a10=l(66)), dict(a11=l(70)), dict(a17=p(36864 + 4))):
        assert _call('dav_knn_topk_f32', **{**kn, **bad}) == -5, bad
    assert _call('dav_knn_topk_f32', **{**kn, 'a18': sz(need - 1)}) == -3          # short workspace
    assert _call('dav_knn_topk_f32', **{**kn, 'a12': i(0), 'a18': sz(S * M * Nq * k * 8 - 8)}) == -3
    assert _call('dav_knn_topk_f32', **{**kn, 'a17': p(0)}) == -3
    from deepavfusion_amd import ops
    assert ops.knn_workspace_bytes(Nq, V, k, S) == need
    assert ops.knn_splits(15440, 15440) * -(-15440 // 128) >= 512 and ops.knn_splits(1, 4) == 1 and ops.knn_splits(37, 4097) == 33


def test_metric_dict_keys_and_order():
    from deepavfusion_amd.util.knn_probe import MODALITIES, probe_metrics
    labels = np.array([0, 1, 2, 1])
    preds = {m: (np.array(p), np.array([0.9, 0.8, 0.7, 0.6], np.float32))
             for m, p in zip(MODALITIES, ([0, 1, 2, 1], [0, 0, 2, 1], [2, 2, 0, 0], [0, 1, 1, 1]))}
    out = probe_metrics(preds, labels, multi_label=False)
    assert list(out) == ['audio_nn_acc', 'image_nn_acc', 'fusion_nn_acc', 'all_nn_acc']
    assert [out[k] for k in out] == [100.0, 75.0, 0.0, 75.0]
    ml = np.array([[1, 0, 0], [0, 1, 1], [1, 1, 0], [0, 0, 1]])
    mp = {m: (ml[[1, 0, 3, 2]], np.array([0.5, 0.4, 0.4, 0.1])) for m in MODALITIES}
    out = probe_metrics(mp, ml, multi_label=True)
    assert list(out) == [f'{m}_nn_{x}' for m in MODALITIES for x in ('ap', 'auc')]
    assert all(0.0 <= v <= 1.0 for v in out.values())
