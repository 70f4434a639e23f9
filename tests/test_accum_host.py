"""CPU: the host side of gradient accumulation in the captured step — the micro-step plan of util.misc.GraphedStep and the error
contract of the gated weight-gradient entry points (dav_gemm_tn_grouped_bf16_gated, dav_gemm_tn_gang_bf16_gated)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATED = ('dav_gemm_tn_grouped_bf16_gated', 'dav_gemm_tn_gang_bf16_gated')


@pytest.mark.parametrize('dist_active', [False, True])
@pytest.mark.parametrize('accum_iter', [1, 2, 4])
def test_micro_step_plan(accum_iter, dist_active):
    """Write-first only on the window's first micro-step, bucket schedule and optimizer pass only on its last."""
    from deepavfusion_amd.util.misc import micro_step_plan
    for accums in range(accum_iter):
        write_first, reduce, optimize = micro_step_plan(accums, accum_iter, dist_active)
        assert write_first == (accums == 0)
        assert reduce == (accums == accum_iter - 1)
        assert optimize == (accums == accum_iter - 1)
    if accum_iter == 1:
        assert tuple(micro_step_plan(0, 1, dist_active)) == (True, True, True)
    for bad in (-1, accum_iter):
        with pytest.raises(ValueError):
            micro_step_plan(bad, accum_iter, dist_active)


def test_gated_entry_points_are_declared_listed_and_exported():
    from deepavfusion_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'dav_kernels.h')).read()
    declared = set(re.findall(r'\b(dav_[a-z0-9_]+)\s*\(', hdr))
    lib = _lib.load()
    for name in GATED:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # the gate is one more pointer in front of the stream
    assert _lib.SIGNATURES[GATED[0]] == _lib.SIGNATURES['dav_gemm_tn_grouped_bf16'][:-1] + [C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES[GATED[1]] == _lib.SIGNATURES['dav_gemm_tn_gang_bf16'][:-1] + [C.c_void_p, C.c_void_p]
    assert lib.dav_abi_version() == _lib.ABI_VERSION == 9
    assert C.sizeof(_lib.DavTnProblem) == 88          # 4 pointers, 6 + 6 + 1 ints, padded to 8: the layout of ABI 9


def _problems(_lib):
    pr = (_lib.DavTnProblem * 2)()
    for q, (N, K) in zip(pr, ((768, 3072), (192, 264))):
        q.A, q.B, q.C = 4096, 8192, 12288
        q.Mc, q.N, q.K, q.lda, q.ldb, q.ldc = 3136, N, K, N, K, K
        q.flags = 1
    return pr


def test_gated_entry_points_error_codes():
    """Validation comes before any HIP call: the dummy pointers are never dereferenced, so this runs without a GPU."""
    from deepavfusion_amd import _lib
    lib = _lib.load()
    p = lambda v: C.c_void_p(v)
    gate, ws = p(16384), p(1 << 20)
    # all-zero arguments: a bad shape
    assert lib.dav_gemm_tn_grouped_bf16_gated(None, 0, None, None) == -1
    assert lib.dav_gemm_tn_gang_bf16_gated(None, 0, None, C.c_size_t(0), None, None) == -1
    pr = _problems(_lib)
    need = lib.dav_gemm_tn_gang_workspace_bytes(pr, 2)
    assert need == 128 + 2 * 96 + 8 * (3 * 12 + 1 * 2)           # shared with the ungated entry point, unchanged
    # a NULL gate with otherwise valid arguments
    assert lib.dav_gemm_tn_grouped_bf16_gated(pr, 2, None, None) == -1
    assert lib.dav_gemm_tn_gang_bf16_gated(pr, 2, ws, C.c_size_t(need), None, None) == -1
    # workspace codes as for dav_gemm_tn_gang_bf16
    assert lib.dav_gemm_tn_gang_bf16_gated(pr, 2, p((1 << 20) + 4), C.c_size_t(need), gate, None) == -5
    assert lib.dav_gemm_tn_gang_bf16_gated(pr, 2, ws, C.c_size_t(need - 1), gate, None) == -3
    # problem validation as for the ungated entry points: unknown flag bits, a misaligned C, a ragged contraction (grouped only)
    pr[1].flags = 3
    assert lib.dav_gemm_tn_gang_bf16_gated(pr, 2, ws, C.c_size_t(need), gate, None) == -1
    assert lib.dav_gemm_tn_grouped_bf16_gated(pr, 2, gate, None) == -1
    pr[1].flags, pr[1].C = 1, 12288 + 4
    assert lib.dav_gemm_tn_gang_bf16_gated(pr, 2, ws, C.c_size_t(need), gate, None) == -5
    assert lib.dav_gemm_tn_grouped_bf16_gated(pr, 2, gate, None) == -5
    pr[1].C, pr[1].Mc = 12288, 100
    assert lib.dav_gemm_tn_grouped_bf16_gated(pr, 2, gate, None) == -1
    assert lib.dav_gemm_tn_grouped_bf16_gated(pr, 41, gate, None) == -1          # more than 40 problems per grouped launch


def test_ops_and_engine_take_a_gate():
    """The Python plumbing: an optional gate on both ops and on engine.wgrad_overwrite_begin; no gate = the ungated calls."""
    import inspect
    from deepavfusion_amd import engine, ops
    assert inspect.signature(ops.gemm_tn_grouped).parameters['gate'].default is None
    assert inspect.signature(ops.gemm_tn_gang).parameters['gate'].default is None
    assert inspect.signature(engine.wgrad_overwrite_begin).parameters['gate'].default is None
    engine.wgrad_overwrite_begin()
    try:
        assert engine._OVERWRITE['gate'] is None
    finally:
        assert engine.wgrad_overwrite_end() == []
    assert engine._OVERWRITE is None
