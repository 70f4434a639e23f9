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


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_unshuffle_bwd_reduce_that_overwrites_instead_of_accumulating():
    """dpos / dmask_token are accumulated (+=).  The old check passed zeros: a kernel that WROTE its sums passes it; into a random
    prefill it is off by the prefill."""
    B, L, nk, D = 3, 24, 5, 64
    gx = torch.randn(B, L, D, generator=_gen(20)).double()
    restore = torch.stack([torch.randperm(L, generator=_gen(21 + b)) for b in range(B)])
    msk = (restore >= nk).double().unsqueeze(-1)
    sums = {'dpos': (gx.sum(0), gx.abs().sum(0), B), 'dmask_token': ((gx * msk).sum((0, 1)), (gx * msk).abs().sum((0, 1)), B * L)}
    for name, (s, a, n) in sums.items():
        right = lambda pre: (pre + s).float()                   # noqa: E731  the contract
        wrong = lambda pre: s.float()                           # noqa: E731  a kernel that overwrites
        zero = torch.zeros(s.shape, dtype=torch.float64)
        assert gpu_selfcheck.rel(right(zero), s) <= 1e-5 and gpu_selfcheck.rel(wrong(zero), s) <= 1e-5    # old check: both pass
        pre = K.prefilled(tuple(s.shape), seed=22).double()
        ref = pre + s
        bound = K.sum_bound(pre.abs() + a, n + 1, ref)
        assert K.within(right(pre), ref, bound)[0]
        assert not K.within(wrong(pre), ref, bound)[0], name


def test_two_loss_patch_entries_swapped():
    """patch_mse_fwd: only the scalar loss was compared.  Swapping two masked rows' loss_patch leaves it unchanged."""
    B, C, H, W = 3, 3, 64, 96
    L, P = (H // 16) * (W // 16), 256 * C
    img, pred = torch.randn(B, C, H, W, generator=_gen(23)), torch.randn(B, L, P, generator=_gen(24))
    mask = (torch.rand(B, L, generator=_gen(25)) > 0.3).float()
    M = K.mse_bounds(img, pred, mask, True)
    lp = M['loss_patch'].float()
    loss = float((lp.double() * mask.double()).sum() / mask.double().sum())
    assert abs(loss - float(M['loss'])) / float(M['loss']) <= 1e-5 and K.within(lp, M['loss_patch'], M['bloss_patch'])[0]
    i, j = [int(x) for x in mask.flatten().nonzero()[:2, 0]]
    bad = lp.clone().flatten()
    bad[i], bad[j] = lp.flatten()[j], lp.flatten()[i]
    bad = bad.view(B, L)
    loss_bad = float((bad.double() * mask.double()).sum() / mask.double().sum())
    assert abs(loss_bad - float(M['loss'])) / float(M['loss']) <= 1e-5        # old check: the scalar is unchanged
    ok, _, msg = K.within(bad, M['loss_patch'], M['bloss_patch'], 'loss_patch')
    assert not ok and '2 of' in msg


def test_mse_bounds_edges():
    """a constant patch (variance 0: rstd = 1 / sqrt(1e-6)), norm off (mean 0 and rstd 1 exactly), masked-out rows of the
    gradient exactly 0"""
    img, pred = torch.randn(2, 1, 32, 32, generator=_gen(26)), torch.randn(2, 4, 256, generator=_gen(27))
    img[0, :, :16, :16] = 0.3
    mask = torch.tensor([[1., 0., 1., 1.], [1., 1., 1., 1.]])
    M = K.mse_bounds(img, pred, mask, True)
    assert abs(float(M['trstd'][0, 0]) - 1e3) < 1e-6 and float(M['btrstd'][0, 0]) < 1e-2 * 1e3
    M0 = K.mse_bounds(img, pred, mask, False)
    assert float(M0['btmean'].abs().max()) == 0.0 and bool((M0['trstd'] == 1).all())
    ref, bnd = K.mse_grad(img, pred, mask, M['tmean'].float(), M['trstd'].float(), mask.sum(), 0.7, BF16)
    assert float(ref[0, 1].abs().max()) == 0.0 and float(bnd[0, 1].max()) == 0.0
    assert K.within(ref.to(BF16), ref, bnd)[0]
    bad = ref.to(BF16).clone()
    bad[0, 1, 17] = 1e-30                                           # a masked-out row must be exactly 0
    assert not K.within(bad, ref, bnd)[0]


def test_one_wrong_pixel_in_patch_gather_at_the_bench_shape():
    """patch_gather at the bench image shape (B 64, 224 x 224, 49 kept) was checked at rel 4e-3: one pixel swapped with its
    neighbour passes it; the bit-exact check names it."""
    B, C, H, W, nk = 64, 3, 224, 224, 49
    L = (H // 16) * (W // 16)
    img = torch.randn(B, C, H, W, generator=_gen(28))
    ids = torch.stack([torch.randperm(L, generator=_gen(29 + b))[:nk] for b in range(B)])
    cols = img.reshape(B, C, H // 16, 16, W // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, L, C * 256)
    ref = cols.gather(1, ids.unsqueeze(-1).expand(-1, -1, C * 256)).reshape(B * nk, -1)
    good = ref.to(BF16)
    assert gpu_selfcheck.rel(good, ref) <= 4e-3 and K.exact(good, ref.to(BF16)) == (0, '')
    bad = good.clone()
    bad[1000, 300], bad[1000, 301] = good[1000, 301], good[1000, 300]
    assert gpu_selfcheck.rel(bad, ref) <= 4e-3                                  # old check: passes
    n, msg = K.exact(bad, ref.to(BF16), 'A')
    assert n == 2 and '[1000, 300]' in msg


def _window_case(B=2, nW=4, H=2, A=16, nF=9, d=32, seed=30):
    N = A + nF
    g = _gen(seed)
    q, k, v, dO = (torch.randn(B * nW, H, N, d, generator=g).to(BF16) for _ in range(4))
    bias = torch.zeros(B * nW, H, N, N)
    bias[:, :, :A, :A] = torch.randn(B * nW, H, A, A, generator=g) * 0.7
    return q, k, v, dO, bias, d ** -0.5


def test_one_wrong_ds_entry_in_window_attention():
    """attn_bias_bwd's dS was compared at rel 2e-2: one entry off by twice its bound passes it; attn_bounds' bdS does not."""
    q, k, v, dO, bias, scale = _window_case()
    O = K.attn_bounds(q, k, v, None, None, scale, bias=bias)['O'].to(BF16)
    r = K.attn_bounds(q, k, v, dO, O, scale, bias=bias)
    dS = r['dS'].float()
    assert gpu_selfcheck.rel(dS, r['dS']) <= 2e-2 and K.within(dS, r['dS'], r['bdS'])[0]
    i = int(r['dS'].abs().flatten().argsort()[r['dS'].numel() // 2])          # an entry of median magnitude
    bad = dS.clone().flatten()
    bad[i] += 2 * float(r['bdS'].flatten()[i])
    bad = bad.view(dS.shape)
    assert gpu_selfcheck.rel(bad, r['dS']) <= 2e-2                              # old check: passes
    ok, ratio, _ = K.within(bad, r['dS'], r['bdS'], 'dS')
    assert not ok and 1.5 < ratio < 2.5


def test_window_fold_fusion_row_summed_over_one_window_less():
    """window_fold's fusion rows are res + (1 / nW) sum over the nW windows, checked at rel 1e-6 over the whole output: a sum that
    skips one window where that window's term is small (here 1e-4) passes it; the nW-term sum bound does not."""
    B, nW, A, nF, C = 2, 4, 16, 9, 96
    N, L = A + nF, nW * A
    t = torch.randn(B, nW, N, C, generator=_gen(31))
    res = torch.randn(B, nF + L, C, generator=_gen(32))
    t[1, 2, A + 5, 40] = 1e-4
    fs = 1.0 / nW
    f64 = res[:, :nF].double() + fs * t[:, :, A:].double().sum(1)
    bound = K.sum_bound(res[:, :nF].double().abs() + fs * t[:, :, A:].double().abs().sum(1), nW + 2, f64)
    tok = t[:, :, :A].reshape(B, L, C).double() + res[:, nF:].double()
    right = f64.float()
    bad = right.clone()
    bad[1, 5, 40] = float(f64[1, 5, 40] - fs * 1e-4)                           # window 2 skipped in this element
    full = lambda f: torch.cat([f.double(), tok], 1)                            # noqa: E731
    want = torch.cat([f64, tok], 1)
    assert gpu_selfcheck.rel(full(right), want) <= 1e-6 and K.within(right, f64, bound)[0]
    assert gpu_selfcheck.rel(full(bad), want) <= 1e-6                           # old check: passes
    ok, ratio, msg = K.within(bad, f64, bound, 'fusion rows')
    assert not ok and ratio > 1.0 and '[1, 5, 40]' in msg


def test_unshuffle_fwd_writing_into_the_leading_rows():
    """unshuffle_fwd writes rows nF.. of each batch element; the old check read only those rows of a zero-filled buffer, so a
    kernel that also zero-fills (or writes) the nF leading rows passes it.  In a poisoned buffer the leading rows must keep their bits."""
    B, L, nk, D, nF = 3, 24, 5, 64, 3
    emb, mt, pos = torch.randn(B * nk, D, generator=_gen(33)), torch.randn(D, generator=_gen(34)), torch.randn(L, D, generator=_gen(35))
    restore = torch.stack([torch.randperm(L, generator=_gen(36 + b)) for b in range(B)])
    full = torch.cat([emb.view(B, nk, D), mt.view(1, 1, D).expand(B, L - nk, D)], 1)
    want = full.gather(1, restore.unsqueeze(-1).expand(-1, -1, D)) + pos
    lead = torch.zeros(B, nF + L, dtype=torch.bool)
    lead[:, :nF] = True
    old, new = torch.zeros(B, nF + L, D), K.poisoned((B, nF + L, D), torch.float32)
    before = new.clone()
    for out in (old, new):
        out[:, nF:] = want
        out[2, 1] = 0.0                                                         # ... and one leading row
    assert gpu_selfcheck.rel(old[:, nF:], want) <= 1e-6 and K.exact(new[:, nF:], want) == (0, '')
    assert K.changed(new, before, lead) == (D, (2 * (nF + L) + 1) * D)
    good = before.clone()
    good[:, nF:] = want
    assert K.changed(good, before, lead) == (0, -1)


def test_f32_attention_bound_is_tight():
    """the fp32 twins' allowance (kcheck.f32_attn_up) stays well below bf16's one rounding: an O off by three times its fp32 bound —
    which the bf16 bound would pass — fails it"""
    q, k, v, dO, bias, scale = _window_case(seed=37)
    q, k, v = q.float(), k.float(), v.float()
    up = K.f32_attn_up(q, k, scale, bias)
    assert up < K.U16 / 20
    r = K.attn_bounds(q, k, v, None, None, scale, up=up, r_out=K.out_round(torch.float32), bias=bias)
    O = r['O'].float()
    assert K.within(O, r['O'], r['bO'])[0]
    bad = (r['O'] + 3 * r['bO']).float()
    assert K.within(bad, r['O'], K.attn_bounds(q, k, v, None, None, scale, bias=bias)['bO'])[0]
    assert not K.within(bad, r['O'], r['bO'])[0]


# ---- the optimizer pass (kcheck.adamw_ref): an fp32 transcription of dav_adamw_flat's formula passes, six ways it could go wrong
# do not

_ADAMW_SIZES = [192, 36864, 576, 1000] + [64] * 6 + [2304, 192, 192, 768, 40]      # 1000 and 40: padded to 1024 and 64
_ADAMW_DECAYED = [sz in (36864, 2304, 768) for sz in _ADAMW_SIZES]
_B1, _B2, _EPS, _GS = 0.9, 0.95, 1e-8, 0.37


def _adamw_case():
    """A flat state of the kind util/flat.py lays out (|p| ~ 0.02, lr wd >= 1e-5 on the decayed segments, padding all zero), in the
    middle of training (m, v non-zero), and one gradient"""
    ends, hyper, real = K.seg_table(_ADAMW_SIZES, _ADAMW_DECAYED)
    n = ends[-1]
    assert n % 4096 and n > 4096 * 10                              # the last 4096-chunk is a partial one
    g = _gen(40)
    p, g0, g1 = (torch.where(real, torch.randn(n, generator=g) * s, torch.zeros(())) for s in (0.02, 1.0, 1.0))     # padding: +0
    sc = 10.0 ** torch.randint(-4, 1, (len(ends),), generator=g).float()       # gradient magnitude per parameter
    seg = torch.tensor(ends)
    g0, g1 = g0 * K.seg_expand(seg, sc, n), g1 * K.seg_expand(seg, sc, n)
    m, v = 0.1 * g0, 0.05 * g0 * g0
    bc = torch.tensor([1 - _B1 ** 2, (1 - _B2 ** 2) ** 0.5])
    return dict(p=p, g=g1, m=m, v=v, seg=seg, hyper=torch.tensor(hyper), bc=bc, ends=ends, n=n, real=real)


def _adamw_f32(c, lr=None, wd=None, gs_v=_GS):
    """dav_adamw_flat's statement order in fp32 torch ops, one rounding per operation (every scalar an fp32 tensor).  lr / wd:
    per-element tables (default: the case's own); gs_v: the gradient scale used for v (a mutant passes 1)."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)          # noqa: E731
    hy = c['hyper'].view(-1, 2)
    lr = K.seg_expand(c['seg'], hy[:, 0], c['n']) if lr is None else lr
    wd = K.seg_expand(c['seg'], hy[:, 1], c['n']) if wd is None else wd
    b1, b2, eps, bc1, bc2 = f(_B1), f(_B2), f(_EPS), c['bc'][0], c['bc'][1]
    gx, gv = c['g'] * f(_GS), c['g'] * f(gs_v)
    m = b1 * c['m'] + (1 - b1) * gx
    v = b2 * c['v'] + (1 - b2) * gv * gv
    p = c['p'] * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / bc2 + eps)
    assert p.dtype == m.dtype == v.dtype == torch.float32
    return p, m, v


def _adamw_judge(c, p, m, v):
    """(ok, message) of p, m, v against kcheck.adamw_ref of the case's input state"""
    r = K.adamw_ref(c['p'], c['g'], c['m'], c['v'], c['seg'], c['hyper'], _B1, _B2, _EPS, c['bc'], _GS)
    return {k: K.within(got, r[k], r['b' + k], k)[::2] for k, got in (('p', p), ('m', m), ('v', v))}


def _nbad(msg):
    """(number of elements outside the bound, flat index of the worst one) from a ``within`` message"""
    return int(msg.split(': ')[1].split(' of')[0]), int(msg.split('worst at [')[1].split(']')[0])


def test_adamw_fp32_transcription_is_inside_the_bounds():
    c = _adamw_case()
    j = _adamw_judge(c, *_adamw_f32(c))
    assert all(ok for ok, _ in j.values()), j
    # the padding stays exactly +0 through the formula (what gpu_selfcheck.optimizer asks of the kernel)
    for t in _adamw_f32(c):
        assert K.exact(t[~c['real']], torch.zeros(int((~c['real']).sum()))) == (0, '')


def test_adamw_first_float4_behind_a_boundary_with_the_neighbours_hyper():
    """(a) a lane whose segment walk stops one short: 4 elements updated with the previous segment's lr / wd"""
    c = _adamw_case()
    hy = c['hyper'].view(-1, 2)
    lr, wd = K.seg_expand(c['seg'], hy[:, 0], c['n']), K.seg_expand(c['seg'], hy[:, 1], c['n'])
    e = c['ends'][5]                                               # between two of the 64-element segments
    lr[e:e + 4], wd[e:e + 4] = lr[e - 1], wd[e - 1]
    j = _adamw_judge(c, *_adamw_f32(c, lr, wd))
    assert not j['p'][0] and _nbad(j['p'][1])[0] == 4 and e <= _nbad(j['p'][1])[1] < e + 4, j['p']
    assert j['m'][0] and j['v'][0]                                 # the moments do not depend on the table


def test_adamw_weight_decay_on_a_segment_without():
    """(b) wd = 0.05 applied to a 1-D parameter"""
    c = _adamw_case()
    hy = c['hyper'].view(-1, 2)
    wd = K.seg_expand(c['seg'], hy[:, 1], c['n'])
    lo, hi = c['ends'][1], c['ends'][2]                            # the 576-element segment: wd 0
    assert float(wd[lo:hi].max()) == 0.0
    wd[lo:hi] = 0.05
    j = _adamw_judge(c, *_adamw_f32(c, wd=wd))
    assert not j['p'][0] and _nbad(j['p'][1])[0] > 0.9 * (hi - lo) and lo <= _nbad(j['p'][1])[1] < hi, j['p']
    assert j['m'][0] and j['v'][0]


def test_adamw_one_float4_of_the_last_partial_chunk_not_updated():
    """(c) a float4 group in the ragged last 4096-chunk keeps its old p / m / v"""
    c = _adamw_case()
    p, m, v = _adamw_f32(c)
    i = c['n'] // 4096 * 4096 + 1028
    assert i + 4 <= c['n'] and bool(c['real'][i:i + 4].all())
    for new, old in ((p, c['p']), (m, c['m']), (v, c['v'])):
        new[i:i + 4] = old[i:i + 4]
    j = _adamw_judge(c, p, m, v)
    for k in 'pmv':
        assert not j[k][0] and _nbad(j[k][1])[0] == 4 and i <= _nbad(j[k][1])[1] < i + 4, j[k]


def test_adamw_mirror_taken_from_the_old_parameters():
    """(d) the bf16 mirror must be ONE rounding of the p just stored: bit-exact, where the old rel <= 4e-3 passes the stale one"""
    c = _adamw_case()
    p = _adamw_f32(c)[0]
    assert K.exact(p.to(BF16), p.to(BF16)) == (0, '')
    stale = c['p'].to(BF16)
    assert gpu_selfcheck.rel(stale[:c['ends'][0]], p[:c['ends'][0]]) > 0          # (not the same numbers)
    n, msg = K.exact(stale, p.to(BF16), 'mirror')
    assert n > 0.5 * int(c['real'].sum()) and 'mirror' in msg


def test_adamw_a_kept_gradient_segment_zero_filled():
    """(e) zero_grad with keep_grad = 1 on a segment: its gradient must come back bit-identical"""
    c = _adamw_case()
    lo, hi = c['ends'][6], c['ends'][7]
    keep = torch.zeros(c['n'], dtype=torch.bool)
    keep[lo:hi] = True
    right = torch.where(keep, c['g'], torch.zeros(()))
    assert K.changed(right, c['g'], keep) == (0, -1) and K.exact(right[~keep], torch.zeros(c['n'] - (hi - lo))) == (0, '')
    wrong = torch.zeros(c['n'])
    n, i = K.changed(wrong, c['g'], keep)
    assert n == hi - lo and i == lo


def test_adamw_second_moment_from_the_unscaled_gradient():
    """(f) v updated with g instead of g * grad_scale"""
    c = _adamw_case()
    j = _adamw_judge(c, *_adamw_f32(c, gs_v=1.0))
    assert j['m'][0] and not j['v'][0] and not j['p'][0], j
    assert _nbad(j['v'][1])[0] > 0.9 * int(c['real'].sum())


def test_exact_sees_a_negative_zero():
    """the DropPath backward's dropped rows are checked with ``exact``: -0 where +0 is due is a difference"""
    z = torch.zeros(4, dtype=BF16)
    assert K.exact(-z, z)[0] == 4 and K.exact(z, z) == (0, '')


def test_depth_bounds_are_not_vacuous():
    """sum_bound with n = the element count allows a relative 6e-2 at 10^6 elements; the depth bounds stay near 1e-6 (l2norm) and
    track the workgroup count (the fused sum(g^2): one atomic add each)"""
    assert K.adamw_grid(4) == (1, 1) and K.adamw_grid(4100) == (2, 1) and K.adamw_grid(16384 * 4096) == (16384, 1)
    assert K.adamw_grid(16384 * 4096 + 4) == (16384, 2)
    assert K.adamw_sumsq_bound(900000, 1.0) == (16 + 10 + 220) * K.U32
    assert K.l2norm_bound(1234567, 2.0) == ((8 + 11) / 2 + 2) * K.U32 * 2.0
    assert K.l2norm_bound(3, 1.0) == (11 / 2 + 2) * K.U32                          # tail only: no float4 trip
