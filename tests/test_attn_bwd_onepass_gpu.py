"""GPU: the one-pass attention backward (csrc/attention.hip attn_bwd_one_body) forced on with dav_tune knob 5 = 2, held to what
tests/gpu_selfcheck.py attention() holds the dQ + dK/dV kernel pair to: the per-element bounds of tests/kcheck.py against a float64
reference on the same bf16 operands, outputs poisoned with NaN before the call, guard bands and padding columns around them.
Also: Delta against rowsum(dO o O), the context rows of a fused qkv gradient, repeatability, grouped == single launches, and the
fall-back to the kernel pair just above the fit rule (seen through the number of recorded launches)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

# (B, H, Nq, Nk, dqk, dv, layout): 'fused' = q / k / v inside one [B, Nk, 3, H, d] buffer, the queries its last Nq rows (the tower
# blocks: the rows in front are the fusion-token context rows); 'cross' = q [B, Nq, H d], k | v in one [B, Nk, 2 H d] buffer (the
# aggregation cross-attentions); 'sep' = three buffers (the pair attention)
PATH_SHAPES = [
    (2, 12, 63, 95, 64, 64, 'fused'), (2, 12, 49, 81, 64, 64, 'fused'),          # tower self-attention, ViT-B
    (3, 12, 8, 63, 64, 64, 'cross'), (3, 12, 8, 49, 64, 64, 'cross'),            # aggregations
    (2, 12, 16, 64, 16, 64, 'sep'),                                              # pair attention
    (2, 12, 80, 112, 64, 64, 'fused'), (2, 12, 8, 80, 64, 64, 'cross'),          # base_m75: 80 audio tokens
    (2, 16, 63, 95, 64, 64, 'fused'), (2, 16, 49, 81, 64, 64, 'fused'),          # ViT-L head counts
    (2, 16, 8, 63, 64, 64, 'cross'), (2, 16, 8, 49, 64, 64, 'cross'), (2, 16, 16, 64, 16, 64, 'sep'),
]
EDGE_SHAPES = [(2, 2, nq, nk, dqk, 64, 'sep') for dqk in (64, 16) for nq in (1, 8, 15, 16, 17, 63, 64) for nk in (1, 31, 32, 33, 95, 96)]


@pytest.fixture
def onepass():
    """knob 5 = 2 (one pass whenever the problem fits) for the test, the rule again afterwards"""
    from deepavfusion_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dav_tune(5, 2), 'dav_tune')
    try:
        yield lib
    finally:
        lib.dav_tune(5, 0)


class Case:
    """Operands, float64 reference + bounds (kcheck.attn_bounds) and guarded gradient buffers of one problem."""

    def __init__(self, B, H, Nq, Nk, dqk, dv, layout, seed=0):
        import torch

        import kcheck as kc
        from deepavfusion_amd import ops
        dev, bf = torch.device('cuda'), torch.bfloat16
        self.shape, self.layout = (B, H, Nq, Nk, dqk, dv), layout
        self.scale = 0.125 if dqk == 16 else dqk ** -0.5
        g = torch.Generator(device='cpu').manual_seed(1000 + seed)
        rnd = lambda *s: torch.randn(*s, generator=g).to(device=dev, dtype=bf)
        self.off = Nk - Nq if layout == 'fused' else 0
        # [rows per batch element, columns, first row, first column] of q, k, v inside their buffers
        if layout == 'fused':
            assert dqk == dv and Nq <= Nk
            buf = rnd(B * Nk, 3 * H * dqk)
            self.bufs = [buf, buf, buf]
            self.geo = [(Nk, 3 * H * dqk, self.off, 0), (Nk, 3 * H * dqk, 0, H * dqk), (Nk, 3 * H * dqk, 0, 2 * H * dqk)]
        elif layout == 'cross':
            assert dqk == dv
            qb, kvb = rnd(B * Nq, H * dqk), rnd(B * Nk, 2 * H * dqk)
            self.bufs = [qb, kvb, kvb]
            self.geo = [(Nq, H * dqk, 0, 0), (Nk, 2 * H * dqk, 0, 0), (Nk, 2 * H * dqk, 0, H * dqk)]
        else:
            self.bufs = [rnd(B * Nq, H * dqk), rnd(B * Nk, H * dqk), rnd(B * Nk, H * dv)]
            self.geo = [(Nq, H * dqk, 0, 0), (Nk, H * dqk, 0, 0), (Nk, H * dv, 0, 0)]
        self.n = (Nq, Nk, Nk)
        self.d = (dqk, dqk, dv)
        self.q, self.k, self.v = (self.heads(t, i).float() for i, t in enumerate(self.bufs))
        self.O = kc.poisoned((B * Nq, H * dv), bf, dev)
        self.LSE = kc.poisoned((B, H, Nq), torch.float32, dev)
        st = [x for (rows, cols, _, _) in self.geo for x in (rows * cols, cols)]
        ops.attn_fwd(*self.ptrs(self.bufs, [cols for (_, cols, _, _) in self.geo]), self.O, self.LSE, B, H, Nq, Nk, dqk, dv, *st,
                     Nq * H * dv, H * dv, self.scale)
        self.dO = rnd(B * Nq, H * dv)
        self.in_strides = st
        self.Ok = self.O.view(B, Nq, H, dv).permute(0, 2, 1, 3)
        self.dOk = self.dO.view(B, Nq, H, dv).permute(0, 2, 1, 3)
        self.r64 = kc.attn_bounds(self.q, self.k, self.v, self.dOk, self.Ok, self.scale)

    def heads(self, t2d, i):
        """[B, H, n, d] view of operand i (0 q, 1 k, 2 v) inside a [B * rows, cols] buffer (or a guarded view of one)"""
        B, H = self.shape[0], self.shape[1]
        rows, cols, r0, c0 = self.geo[i]
        return t2d.reshape(B, rows, cols)[:, r0:r0 + self.n[i], c0:c0 + H * self.d[i]].reshape(B, self.n[i], H, self.d[i]).permute(0, 2, 1, 3)

    def ptrs(self, bufs, lds):
        return [t.data_ptr() + 2 * (self.geo[i][2] * lds[i] + self.geo[i][3]) for i, t in enumerate(bufs)]

    def grads(self, fill='poison', pad=8):
        """guarded gradient buffers with the geometry of the operand buffers and ``pad`` padding columns per row"""
        import kcheck as kc
        import torch
        B = self.shape[0]
        made = {}
        out = []
        for t, (rows, cols, _, _) in zip(self.bufs, self.geo):
            if id(t) not in made:
                made[id(t)] = kc.Guarded(B * rows, cols, torch.bfloat16, ld=cols + pad, device=t.device, fill=fill)
            out.append(made[id(t)])
        return out

    def backward(self, gr, dq_ctx_rows=0, part=3):
        import torch

        from deepavfusion_amd import ops
        B, H, Nq, Nk, dqk, dv = self.shape
        Delta = torch.full_like(self.LSE, float('nan'))
        gst = [x for g_, (rows, _, _, _) in zip(gr, self.geo) for x in (rows * g_.ld, g_.ld)]
        base = [g_.ptr() + 2 * (r0 * g_.ld + c0) for g_, (_, _, r0, c0) in zip(gr, self.geo)]
        ops.attn_bwd(*self.ptrs(self.bufs, [cols for (_, cols, _, _) in self.geo]), self.O, self.dO, self.LSE, Delta, *base,
                     B, H, Nq, Nk, dqk, dv, *self.in_strides, Nq * H * dv, H * dv, Nq * H * dv, H * dv, *gst, self.scale,
                     part=part, dq_ctx_rows=dq_ctx_rows)
        return Delta

    def check(self, gr, Delta, tag):
        """elementwise bounds of dq / dk / dv and Delta, guard bands; returns the list of failures"""
        import kcheck as kc
        import torch
        bad = []
        for i, nm in enumerate(('dq', 'dk', 'dv')):
            got = self.heads(gr[i].t, i)
            ok, ratio, msg = kc.within(got, self.r64[nm], self.r64['b' + nm], f'{tag} {nm}')
            print(f'{tag} {nm}: worst err/bound {ratio:.3e}')
            if not ok:
                bad.append(msg)
        d64, O64 = self.dOk.double(), self.Ok.double()
        ref = (d64 * O64).sum(-1)
        ok, ratio, msg = kc.within(Delta, ref, kc.sum_bound((d64 * O64).abs().sum(-1), self.shape[5], ref), f'{tag} Delta')
        print(f'{tag} Delta: worst err/bound {ratio:.3e}')
        if not ok:
            bad.append(msg)
        seen = set()
        for g_ in gr:
            if id(g_) not in seen:
                seen.add(id(g_))
                n, where = g_.stray()
                if n:
                    bad.append(f'{tag}: {n} stray elements, first in the {where}')
        torch.cuda.synchronize()
        return bad


def _tag(shape, layout):
    B, H, Nq, Nk, dqk, dv = shape
    return f'onepass B{B} H{H} {Nq}x{Nk} d{dqk}/{dv} {layout}'


def _run(shapes, seed0=0):
    from deepavfusion_amd import ops
    bad = []
    for i, (B, H, Nq, Nk, dqk, dv, layout) in enumerate(shapes):
        assert ops.attn_bwd_onepass_fits(Nq, Nk, dqk, dv), (Nq, Nk, dqk, dv)
        c = Case(B, H, Nq, Nk, dqk, dv, layout, seed=seed0 + i)
        gr = c.grads()
        Delta = c.backward(gr)
        bad += c.check(gr, Delta, _tag(c.shape, layout))
    return bad


def test_path_shapes_within_elementwise_bounds(onepass):
    bad = _run(PATH_SHAPES)
    assert not bad, bad[:10]


def test_edge_shapes_within_elementwise_bounds(onepass):
    bad = _run(EDGE_SHAPES, seed0=100)
    assert not bad, bad[:10]


@pytest.mark.parametrize('shape', [s for s in PATH_SHAPES if s[6] == 'fused'] + [(2, 2, 5, 13, 64, 64, 'fused'), (2, 3, 17, 33, 64, 64, 'fused')])
def test_fused_qkv_gradient_context_rows(onepass, shape):
    """q / k / v strided inside a fused qkv buffer.  Plain call: the q slots of the context rows (rows in front of the queries) keep
    their poison, nothing outside the three head blocks is written (padding columns, guard bands).  dq_ctx_rows > 0: they read as
    zero and everything else is bit-identical to the plain call."""
    import kcheck as kc
    import torch
    B, H, Nq, Nk, dqk, dv, layout = shape
    c = Case(B, H, Nq, Nk, dqk, dv, layout, seed=200)
    tag = _tag(c.shape, layout)
    off = c.off
    assert off > 0
    g0 = c.grads()
    d0 = c.backward(g0)
    bad = c.check(g0, d0, tag)
    buf = g0[0]
    ctx = torch.zeros(B, Nk, 3, dtype=torch.bool, device=buf.t.device)
    ctx[:, :off, 0] = True
    t0 = buf.t.reshape(B, Nk, 3, H * dqk)
    n, _ = kc.changed(t0, kc.poisoned(t0.shape, torch.bfloat16, t0.device), ctx)
    assert n == 0, f'{tag}: {n} context-row q slots written by the plain backward'
    g1 = c.grads(fill=float('nan'))
    d1 = c.backward(g1, dq_ctx_rows=off)
    bad += c.check(g1, d1, tag + ' ctx')
    t1 = g1[0].t.reshape(B, Nk, 3, H * dqk)
    want = t0.clone()
    want[:, :off, 0] = 0.0
    assert float(t1[:, :off, 0].abs().max()) == 0.0, f'{tag}: context rows do not read as zero'
    assert kc.changed(t1, want)[0] == 0, f'{tag}: dq_ctx_rows changed the gradient outside the context rows'
    assert torch.equal(d0, d1)
    assert not bad, bad[:10]


def _bits(g_):
    import torch
    return g_.flat.view(torch.int16)


def test_repeatable(onepass):
    """the same problem twice: bit-identical gradients and Delta (fixed summation order, no atomics)"""
    import torch
    for (B, H, Nq, Nk, dqk, dv, layout) in [(8, 12, 63, 95, 64, 64, 'fused'), (8, 12, 8, 63, 64, 64, 'cross'), (8, 12, 16, 64, 16, 64, 'sep'),
                                             (4, 12, 80, 112, 64, 64, 'fused')]:
        c = Case(B, H, Nq, Nk, dqk, dv, layout, seed=300)
        runs = []
        for _ in range(2):
            gr = c.grads(fill='zero')
            Delta = c.backward(gr, dq_ctx_rows=c.off)
            torch.cuda.synchronize()
            runs.append((gr, Delta))
        for a, b in zip(runs[0][0], runs[1][0]):
            assert torch.equal(_bits(a), _bits(b)), _tag(c.shape, layout)
        assert torch.equal(runs[0][1], runs[1][1])


def test_grouped_launch_equals_single_launches(onepass):
    """three problems of one head-width family recorded in an all-independent launch batch (what a region is) go out as ONE grid
    (attn_grouped_kernel<.., 3>) and give bit-identical results to three single launches"""
    import torch

    from deepavfusion_amd import engine as E
    cases = [Case(2, 12, 49, 81, 64, 64, 'fused', seed=400), Case(2, 12, 63, 95, 64, 64, 'fused', seed=401), Case(3, 12, 8, 63, 64, 64, 'cross', seed=402)]
    single = []
    for c in cases:
        gr = c.grads(fill='zero')
        single.append((gr, c.backward(gr, dq_ctx_rows=c.off)))
    torch.cuda.synchronize()
    grouped = [c.grads(fill='zero') for c in cases]
    deltas = []
    E.BATCH_STATS[:] = [0, 0]
    with E.batch(auto_lanes=True):
        for c, gr in zip(cases, grouped):
            deltas.append(c.backward(gr, dq_ctx_rows=c.off))
    torch.cuda.synchronize()
    assert E.BATCH_STATS == [3, 1], E.BATCH_STATS
    for c, (gs, ds), gg, dg in zip(cases, single, grouped, deltas):
        for a, b in zip(gs, gg):
            assert torch.equal(_bits(a), _bits(b)), _tag(c.shape, c.layout)
        assert torch.equal(ds, dg)
        assert not c.check(gg, dg, _tag(c.shape, c.layout) + ' grouped')


def _recorded_launches(c, part=3, lanes=False):
    """launches one backward records in an all-independent batch (``lanes``: in a lane of a lockstep batch)"""
    import torch

    from deepavfusion_amd import engine as E
    gr = c.grads()
    E.BATCH_STATS[:] = [0, 0]
    with E.batch(auto_lanes=not lanes):
        Delta = c.backward(gr, part=part)
    torch.cuda.synchronize()
    return E.BATCH_STATS[0], gr, Delta


def test_falls_back_to_two_kernels_above_the_fit_rule(onepass):
    """96 x 128 rows (64-wide heads) is the largest padded problem the rule takes, 97 x 128 pads to 128 x 128 and must go out as the dQ +
    dK/dV pair; so must everything under knob value 1, a single part, and head width 32 — all still inside the bounds"""
    from deepavfusion_amd import _lib, ops
    assert ops.attn_bwd_onepass_fits(96, 128, 64, 64) and not ops.attn_bwd_onepass_fits(97, 128, 64, 64)
    fit, above = Case(2, 3, 96, 128, 64, 64, 'sep', seed=500), Case(2, 3, 97, 128, 64, 64, 'sep', seed=501)
    n, gr, Delta = _recorded_launches(fit)
    assert n == 1, n
    assert not fit.check(gr, Delta, _tag(fit.shape, 'sep'))
    n, gr, Delta = _recorded_launches(above)
    assert n == 2, n
    assert not above.check(gr, Delta, _tag(above.shape, 'sep') + ' (two kernels)')
    narrow = Case(2, 4, 49, 49, 32, 32, 'sep', seed=502)
    assert _recorded_launches(narrow)[0] == 2
    assert _recorded_launches(fit, part=1)[0] == 1          # a single part is the kernel of that part
    _lib.check(onepass.dav_tune(5, 1), 'dav_tune')
    n, gr, Delta = _recorded_launches(fit)
    assert n == 2, n
    assert not fit.check(gr, Delta, _tag(fit.shape, 'sep') + ' (knob 1)')


def test_rule_takes_the_path_shapes():
    """default knob: the short path shapes go out as one launch, the decoders' as two"""
    from deepavfusion_amd import _lib
    _lib.check(_lib.load().dav_tune(5, 0), 'dav_tune')
    assert _recorded_launches(Case(2, 12, 63, 95, 64, 64, 'fused', seed=600))[0] == 1
    assert _recorded_launches(Case(2, 12, 16, 64, 16, 64, 'sep', seed=601))[0] == 1
    assert _recorded_launches(Case(2, 16, 228, 228, 32, 32, 'sep', seed=602))[0] == 2


def test_same_bits_as_the_kernel_pair(onepass):
    """the one-pass kernel forms every product and every sum in the order the dQ and dK/dV kernels do: gradients and Delta are
    bit-identical to the pair's (knob value 1), on path shapes, edge shapes and with context rows"""
    import torch
    from deepavfusion_amd import _lib
    shapes = PATH_SHAPES + [(2, 2, 17, 33, 64, 64, 'fused'), (2, 2, 1, 1, 64, 64, 'sep'), (2, 2, 64, 96, 16, 64, 'sep'), (2, 3, 96, 128, 64, 64, 'sep'),
                            (2, 2, 15, 31, 16, 64, 'sep')]
    for i, (B, H, Nq, Nk, dqk, dv, layout) in enumerate(shapes):
        c = Case(B, H, Nq, Nk, dqk, dv, layout, seed=700 + i)
        runs = []
        for knob in (2, 1):
            _lib.check(onepass.dav_tune(5, knob), 'dav_tune')
            gr = c.grads(fill='zero')
            Delta = c.backward(gr, dq_ctx_rows=c.off)
            torch.cuda.synchronize()
            runs.append((gr, Delta))
        for a, b in zip(runs[0][0], runs[1][0]):
            assert torch.equal(_bits(a), _bits(b)), _tag(c.shape, layout)
        assert torch.equal(runs[0][1], runs[1][1]), _tag(c.shape, layout)


def test_a_lane_of_a_lockstep_batch_keeps_two_ranks(onepass):
    """recorded into a lane of a launch batch the backward stays dQ, then dK/dV (the lanes' line-up counts two ranks), with the
    same bits as the single one-pass launch"""
    import torch
    c = Case(2, 12, 63, 95, 64, 64, 'fused', seed=800)
    n, gr, Delta = _recorded_launches(c, lanes=True)
    assert n == 2, n
    assert not c.check(gr, Delta, _tag(c.shape, c.layout) + ' (lane)')
    n1, gr1, Delta1 = _recorded_launches(c)
    assert n1 == 1, n1
    torch.cuda.synchronize()
    for a, b in zip(gr, gr1):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(Delta, Delta1)
