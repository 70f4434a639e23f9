"""GPU: engine.attention_fwd / attention_bwd called with operand views against ops.attn_fwd / ops.attn_bwd called directly with
hand-written addresses and strides on the same operands: O, LSE, dq, dk, dv and Delta equal bit for bit, at the smallest shapes at
which a wrong offset or stride shows (queries that start some rows into a packed buffer, v at a column offset, row counts that are
no multiple of 32).  The gradient buffers carry 32 padding columns per row and start as NaN: what no kernel writes stays NaN."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

PAD = 32


def _bits(t):
    import torch
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _compare(views, gviews, direct, B, H, Nq, Nk, hd, ctx):
    """``direct`` = (q, k, v addresses, their 6 strides, dq, dk, dv addresses, their 6 strides) written out by hand."""
    import torch

    from deepavfusion_amd import engine as E
    from deepavfusion_amd import ops
    dev, scale = views[0].t.device, hd ** -0.5
    ptrs, st, gptrs, gst = direct
    nan = lambda *s, dtype=torch.float32: torch.full(s, float('nan'), dtype=dtype, device=dev)
    O1, LSE1 = E.attention_fwd(*views, B, H, Nq, Nk, hd, hd, scale)
    O2, LSE2 = nan(B * Nq, H * hd, dtype=torch.bfloat16), nan(B, H, Nq)
    ops.attn_fwd(*ptrs, O2, LSE2, B, H, Nq, Nk, hd, hd, *st, Nq * H * hd, H * hd, scale)
    assert torch.equal(_bits(O1), _bits(O2)) and torch.equal(_bits(LSE1), _bits(LSE2))
    assert bool(torch.isfinite(O1.float()).all()) and bool(torch.isfinite(LSE1).all())
    dO = torch.randn(B * Nq, H * hd, generator=torch.Generator().manual_seed(7)).to(device=dev, dtype=torch.bfloat16)
    bufs = list({id(g.t): g.t for g in gviews}.values())
    got = []
    for how in ('views', 'direct'):
        for t in bufs:
            t.fill_(float('nan'))
        Delta = nan(B, H, Nq)
        if how == 'views':
            E.attention_bwd(*views, O1, dO, LSE1, *gviews, B, H, Nq, Nk, hd, hd, scale, Delta=Delta, dq_ctx_rows=ctx)
        else:
            ops.attn_bwd(*ptrs, O1, dO, LSE1, Delta, *gptrs, B, H, Nq, Nk, hd, hd, *st, Nq * H * hd, H * hd, Nq * H * hd, H * hd, *gst,
                         scale, part=3, dq_ctx_rows=ctx)
        torch.cuda.synchronize()
        got.append([t.clone() for t in bufs] + [Delta])
    for a, b in zip(*got):
        assert torch.equal(_bits(a), _bits(b))
    assert bool(torch.isfinite(got[0][-1]).all())
    return got[0][:-1]


def test_packed_tower_layout_with_context_rows():
    """qkv [B * R, 3D], the queries the last n of the R = nF + n rows; the gradient buffer [B * R, 3D + PAD]"""
    import torch

    from deepavfusion_amd import engine as E
    B, H, hd, nF, n = 2, 2, 64, 8, 17
    D, R = H * hd, nF + n                       # 128, 25
    dev = torch.device('cuda')
    qkv = torch.randn(B * R, 3 * D, generator=torch.Generator().manual_seed(1)).to(device=dev, dtype=torch.bfloat16)
    dqkv = torch.empty(B * R, 3 * D + PAD, dtype=torch.bfloat16, device=dev)
    assert (qkv.shape, dqkv.shape) == ((50, 384), (50, 416))
    views = E.qkv_cols(qkv, R, D, nF)
    gviews = (E.cols(dqkv, R, 0, nF), E.cols(dqkv, R, D), E.cols(dqkv, R, 2 * D))
    p, g = qkv.data_ptr(), dqkv.data_ptr()
    direct = ((p + 2 * 8 * 384, p + 2 * 128, p + 2 * 256), (9600, 384) * 3,
              (g + 2 * 8 * 416, g + 2 * 128, g + 2 * 256), (10400, 416) * 3)
    for ctx in (nF, 0):
        (d,) = _compare(views, gviews, direct, B, H, n, R, hd, ctx)
        d = d.view(B, R, 3 * D + PAD)
        assert bool(torch.isnan(d[:, :, 3 * D:]).all()), 'padding columns written'
        assert bool(torch.isfinite(d[:, :, D:3 * D].float()).all()) and bool(torch.isfinite(d[:, nF:, :D].float()).all())
        slots = d[:, :nF, :D]                   # the context rows' dq slots: zero-filled by the dQ kernel, else untouched
        assert bool((slots == 0).all()) if ctx else bool(torch.isnan(slots).all())


def test_cross_layout_with_v_at_a_column_offset():
    """q [B * Nq, D], k | v in one [B * Nk, 2D] buffer; gradient buffers with PAD more columns"""
    import torch

    from deepavfusion_amd import engine as E
    B, H, Nq, Nk, hd = 3, 2, 8, 17, 64
    D = H * hd
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(2)
    q = torch.randn(B * Nq, D, generator=gen).to(device=dev, dtype=torch.bfloat16)
    kv = torch.randn(B * Nk, 2 * D, generator=gen).to(device=dev, dtype=torch.bfloat16)
    dq = torch.empty(B * Nq, D + PAD, dtype=torch.bfloat16, device=dev)
    dkv = torch.empty(B * Nk, 2 * D + PAD, dtype=torch.bfloat16, device=dev)
    assert (q.shape, kv.shape, dq.shape, dkv.shape) == ((24, 128), (51, 256), (24, 160), (51, 288))
    views = (E.cols(q, Nq), E.cols(kv, Nk), E.cols(kv, Nk, D))
    gviews = (E.cols(dq, Nq), E.cols(dkv, Nk), E.cols(dkv, Nk, D))
    direct = ((q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * 128), (1024, 128, 4352, 256, 4352, 256),
              (dq.data_ptr(), dkv.data_ptr(), dkv.data_ptr() + 2 * 128), (1280, 160, 4896, 288, 4896, 288))
    d_q, d_kv = _compare(views, gviews, direct, B, H, Nq, Nk, hd, 0)
    assert bool(torch.isnan(d_q[:, D:]).all()) and bool(torch.isnan(d_kv[:, 2 * D:]).all()), 'padding columns written'
    assert bool(torch.isfinite(d_q[:, :D].float()).all()) and bool(torch.isfinite(d_kv[:, :2 * D].float()).all())
