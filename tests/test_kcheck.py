"""CPU: the elementwise kernel checks of tests/kcheck.py catch the localized errors that the relative-L2 checks of
tests/gpu_selfcheck.py / tests/gpu_fuzz.py let through.  Every case builds a correct float64 "kernel output", mutates it the way
a kernel could go wrong, and asserts: the old rel() check passes, the new check fails (and the unmutated output passes both)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_fuzz  # noqa: E402
import gpu_selfcheck  # noqa: E402
import kcheck as K  # noqa: E402

BF16 = torch.bfloat16


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def test_one_wrong_dq_row_in_the_fuzz_shape():
    """gpu_fuzz.fuzz_attn checks dq at rel 2.5e-2: with B*H*Nq = 7200 one negated query row passes it."""
    B, H, Nq, Nk, d = 3, 4, 600, 64, 64
    q, k, v, dO = _bf(B, H, Nq, d, seed=1), _bf(B, H, Nk, d, seed=2), _bf(B, H, Nk, d, seed=3), _bf(B, H, Nq, d, seed=4)
    scale = d ** -0.5
    O = K.attn_bounds(q, k, v, None, None, scale)['O'].to(BF16)
    r = K.attn_bounds(q, k, v, dO, O, scale)
    dq = r['dq'].to(BF16)                                   # a correct kernel result: the reference rounded to the output type
    assert gpu_fuzz.rel(dq.float(), r['dq']) <= 2.5e-2
    assert K.within(dq, r['dq'], r['bdq'], 'dq')[0]
    bad = dq.clone()
    bad[1, 2, 345] = -bad[1, 2, 345]
    assert gpu_fuzz.rel(bad.float(), r['dq']) <= 2.5e-2     # old check: passes
    ok, ratio, msg = K.within(bad, r['dq'], r['bdq'], 'dq')
    assert not ok and ratio > 1.0 and '[1, 2, 345, ' in msg


def test_one_tile_ten_percent_off_in_a_bf16_gemm_output():
    """gpu_selfcheck.gemm_nt checks bf16 outputs at rel 6e-3: one 128 x 128 tile 10 % off at 5184 x 2304 passes it."""
    M, N, Kd = 5184, 2304, 64
    A, W = _bf(M, Kd, seed=5), _bf(N, Kd, scale=0.05, seed=6)
    ref = A.double() @ W.double().t()
    C = ref.to(BF16)
    bound = K.gemm_bound(A, W, ref, BF16)
    assert gpu_selfcheck.rel(C, ref) <= 6e-3 and K.within(C, ref, bound)[0]
    bad = C.clone()
    bad[3 * 128:4 * 128, 7 * 128:8 * 128] *= 1.1
    assert gpu_selfcheck.rel(bad, ref) <= 6e-3
    ok, _, msg = K.within(bad, ref, bound, 'C')
    assert not ok and 'tile128 (3, 7)' in msg and 'tile256 (1, 3)' in msg


def test_a_tile_never_written():
    """A tile the kernel skips: in a buffer the caching allocator hands back it holds an earlier launch's (correct) answer and
    the old check passes; in a poisoned buffer it stays NaN.  A stale tile from a different problem fails the bound as well."""
    M, N, Kd = 300, 200, 128
    A, W = _bf(M, Kd, seed=7), _bf(N, Kd, scale=0.05, seed=8)
    ref = A.double() @ W.double().t()
    bound = K.gemm_bound(A, W, ref, torch.float32)
    result = ref.float()
    skip = (slice(256, 300), slice(128, 200))               # the ragged corner tile
    old = torch.empty(M, N)
    old.copy_(result)                                       # the block still holds the previous configuration's answer
    new = K.poisoned((M, N), torch.float32)
    for out in (old, new):
        keep = out[skip].clone()
        out.copy_(result)
        out[skip] = keep                                    # ... the kernel under test skipped the tile
    assert gpu_selfcheck.rel(old, ref) <= 1e-4 and K.within(old, ref, bound)[0]
    ok, ratio, msg = K.within(new, ref, bound, 'C')
    assert not ok and ratio == float('inf') and 'tile128 (2, 1)' in msg
    stale = result.clone()
    stale[skip] = (ref[skip] * 1.0003).float()              # what another problem of similar values left there
    assert gpu_selfcheck.rel(stale, ref) <= 1e-4
    assert not K.within(stale, ref, bound)[0]


def test_one_byte_changed_in_a_guard_band():
    """A store one element past the output (or into the row padding) leaves the result itself correct: only the guard shows it."""
    M, N, Kd, ld = 37, 100, 136, 104
    A, W = _bf(M, Kd, seed=9), _bf(N, Kd, scale=0.05, seed=10)
    ref = A.double() @ W.double().t()
    for where in ('trailing', 'leading', 'padding'):
        g = K.Guarded(M, N, torch.float32, ld=ld)
        assert bool(g.t.isnan().all()) and g.t.stride() == (ld, 1) and g.ptr() % 16 == 0
        g.t.copy_(ref.float())
        assert g.stray() == (0, '')
        raw = g.flat.view(torch.uint8)
        off = {'trailing': raw.numel() - K.GUARD_BYTES, 'leading': K.GUARD_BYTES - 1,
               'padding': K.GUARD_BYTES + (5 * ld + N) * 4 + 2}[where]
        raw[off] ^= 0x01
        assert gpu_selfcheck.rel(g.t, ref) <= 1e-4 and K.within(g.t, ref, K.gemm_bound(A, W, ref, torch.float32))[0]
        n, msg = g.stray()
        assert n == 1 and where in msg, msg
    # bf16 views keep the 16-byte alignment too, and the guard compares bits (a NaN payload is not "equal" by value)
    g = K.Guarded(3, 8, BF16, ld=16)
    assert g.ptr() % 16 == 0 and g.stray()[0] == 0


def test_a_row_the_row_map_skips_is_written():
    """gpu_selfcheck's row-map check starts from zeros: a kernel that zero-fills the rows outside c_rowmap passes it.  Rows the map
    skips must keep their bits (here: the poison)."""
    Bsz, rpb, tot, N, Kd = 5, 70, 90, 512, 256
    A, W = _bf(Bsz * rpb, Kd, seed=11), _bf(N, Kd, scale=0.1, seed=12)
    ref = torch.zeros(Bsz, tot, N, dtype=torch.float64)
    ref[:, 1:1 + rpb] = (A.double() @ W.double().t()).view(Bsz, rpb, N)
    ref = ref.view(-1, N)
    mapped = torch.zeros(Bsz, tot, dtype=torch.bool)
    mapped[:, 1:1 + rpb] = True
    mapped = mapped.view(-1)
    old = torch.zeros(Bsz * tot, N, dtype=BF16)
    new = K.poisoned((Bsz * tot, N), BF16)
    before = new.clone()
    for out in (old, new):
        out[mapped] = ref[mapped].to(BF16)
        out[3 * tot + 80] = 0.0                             # the kernel under test also wrote one skipped row
    assert gpu_selfcheck.rel(old, ref) <= 6e-3
    bound = K.gemm_bound(A, W, ref[mapped], BF16)
    assert K.within(new[mapped], ref[mapped], bound)[0]
    n, i = K.changed(new, before, ~mapped)
    assert n == N and i == (3 * tot + 80) * N
    assert K.changed(before.clone(), before, ~mapped) == (0, -1)


def test_within_rejects_non_finite_and_reports_the_worst_element():
    ref = torch.zeros(4, 300, dtype=torch.float64)
    got = ref.clone()
    assert K.within(got, ref, 0.0) == (True, 0.0, '')
    got[2, 299] = float('inf')
    ok, ratio, msg = K.within(got, ref, 1e30, 'x')
    assert not ok and ratio == float('inf') and '[2, 299] tile128 (0, 2) tile256 (0, 1)' in msg
    got[2, 299] = 0.5
    got[0, 0] = 0.25
    ok, ratio, msg = K.within(got, ref, 0.1, 'x')
    assert not ok and abs(ratio - 5.0) < 1e-12 and '2 of 1200' in msg and '[2, 299]' in msg
    # an integer output: poison is the sentinel
    assert bool((K.poisoned((3,), torch.int32) == K.INT_POISON).all())


def test_prefilled_accumulators_must_add_to_the_prefill():
    """An accumulating output checked against prefill + result: a kernel that WROTE instead of adding is off by the prefill."""
    N, Kd, Mc = 72, 40, 128
    A, Bm = _bf(Mc, N, seed=13), _bf(Mc, Kd, seed=14)
    pre = K.prefilled((N, Kd), seed=15)
    prod = A.double().t() @ Bm.double()
    ref = pre.double() + prod
    bound = K.gemm_bound(A.t(), Bm.t(), ref, torch.float32)
    assert K.within((pre.double() + prod).float(), ref, bound)[0]
    assert not K.within(prod.float(), ref, bound)[0]
