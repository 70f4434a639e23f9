"""CPU: the attention operand views of the engine (engine.AttnView / cols / qkv_cols) and the checks attention_fwd / attention_bwd
make before any library call.  The layouts of every call site are held to literal (offset, batch stride, row stride) triples; the
library entry points are replaced by stubs, so nothing here needs the HIP library or a GPU (only shapes and addresses matter)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepavfusion_amd import engine as E  # noqa: E402
from deepavfusion_amd import ops  # noqa: E402

B, D, H, nF, n = 2, 128, 2, 8, 17
R = nF + n                      # 25 rows per batch element of the packed tower projection
nq, nk = 8, 17
nmm, nv, na, P, Da = 4, 2, 2, 4, 32
nS = 25
nW, N = 4, 24
FWD = ('attn_fwd', 'attn_drop_fwd', 'attn_bias_fwd')
BWD = ('attn_bwd', 'attn_drop_bwd', 'attn_bias_bwd')


def buf(rows, ld):
    return torch.empty((rows, ld), dtype=torch.bfloat16)


def sites():
    """name -> (views (q, k, v), literal (off, bs, rs) of each, problem (batch, H, Nq, Nk, dqk, dv), dq_ctx_rows)"""
    qkv = buf(B * R, 3 * D)
    q, kv = buf(B * nq, D), buf(B * nk, 2 * D)
    q2, Kp, Vp = buf(B * nmm, Da), buf(B * P, Da), buf(B * P, D)
    qt, kvt = buf(B * nF, Da), buf(B * nS, 2 * Da)
    qd, KV = buf(B * nF, Da), buf(B * P, 2 * Da)
    wqkv = buf(B * nW * N, 3 * D)
    return {
        'tower': (E.qkv_cols(qkv, R, D, nF), [(3072, 9600, 384), (128, 9600, 384), (256, 9600, 384)], (B, H, n, R, 64, 64), nF),
        'aggregation': ((E.cols(q, nq), E.cols(kv, nk), E.cols(kv, nk, D)), [(0, 1024, 128), (0, 4352, 256), (128, 4352, 256)],
                        (B, H, nq, nk, 64, 64), 0),
        'pair': ((E.cols(q2, nmm), E.cols(Kp, P), E.cols(Vp, P)), [(0, 128, 32), (0, 128, 32), (0, 512, 128)], (B, H, nmm, P, 16, 64), 0),
        'token': ((E.cols(qt, nF), E.cols(kvt, nS), E.cols(kvt, nS, Da)), [(0, 256, 32), (0, 1600, 64), (32, 1600, 64)],
                  (B, H, nF, nS, 16, 16), 0),
        'dense': ((E.cols(qd, nF), E.cols(KV, P), E.cols(KV, P, Da)), [(0, 256, 32), (0, 256, 64), (32, 256, 64)], (B, H, nF, P, 16, 16), 0),
        'swin': (E.qkv_cols(wqkv, N, D), [(0, 9216, 384), (128, 9216, 384), (256, 9216, 384)], (B * nW, H, N, N, 64, 64), 0),
    }


SITES = sorted(sites())


@pytest.fixture
def unreachable(monkeypatch):
    def stub(*a, **kw):
        pytest.fail('a library entry point was reached with an operand that must be refused')
    for name in FWD + BWD:
        monkeypatch.setattr(ops, name, stub)


@pytest.fixture
def recorded(monkeypatch):
    calls = []
    for name in FWD + BWD:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)))
    return calls


@pytest.mark.parametrize('site', SITES)
def test_constructor_reproduces_the_parent_layouts(site):
    views, want, _, _ = sites()[site]
    assert [tuple(v[1:]) for v in views] == want
    assert all(isinstance(v, E.AttnView) and v.t.dim() == 2 for v in views)


def like(v, t=None, **kw):
    """the view with its buffer or a stride replaced"""
    return v._replace(**kw) if t is None else E.AttnView(t, *v[1:])._replace(**kw)


def bad_operands(v, width, rows_used):
    """the violations of one good view ``v`` (``width`` = H * d columns, ``rows_used`` = N rows from its first row)"""
    rows, ld = v.bs // v.rs, v.rs
    r0, c0 = divmod(v.off, ld)
    wide = torch.empty((v.t.shape[0], 2 * ld), dtype=v.t.dtype)[:, :ld]
    return {
        'non-contiguous': like(v, wide),
        '3-D': like(v, v.t.view(B, -1, ld)),
        'columns one past ld': E.cols(v.t, rows, ld - width + 1, r0),
        'rows one past the batch element': E.cols(v.t, rows, c0, rows - rows_used + 1),
        'B * rows is not the row count': like(v, torch.empty((v.t.shape[0] + 1, ld), dtype=v.t.dtype)),
        'row stride is not ld': like(v, rs=ld - 1),
        'batch stride no multiple of the row stride': like(v, bs=v.bs + 1),
    }


@pytest.mark.parametrize('which', range(3))
@pytest.mark.parametrize('site', ['tower', 'aggregation'])
def test_forward_refuses_bad_operands(unreachable, site, which):
    views, _, (b, h, Nq, Nk, dqk, dv), _ = sites()[site]
    width, rows_used = h * (dv if which == 2 else dqk), (Nq if which == 0 else Nk)
    assert 'non-contiguous' in bad_operands(views[which], width, rows_used)
    for what, v in bad_operands(views[which], width, rows_used).items():
        ops_ = list(views)
        ops_[which] = v
        with pytest.raises(ValueError, match=f"operand {'qkv'[which]}:"):
            E.attention_fwd(*ops_, b, h, Nq, Nk, dqk, dv, 0.125)
        with pytest.raises(ValueError):
            E.attention_fwd(*ops_, b, h, Nq, Nk, dqk, dv, 0.125, keep=(None, 32, 1.0))


@pytest.mark.parametrize('which', range(6))
@pytest.mark.parametrize('site', ['tower', 'aggregation'])
def test_backward_refuses_bad_operands(unreachable, site, which):
    views, _, (b, h, Nq, Nk, dqk, dv), ctx = sites()[site]
    grads = tuple(like(v, torch.empty_like(v.t)) for v in views)
    O, LSE = torch.empty((b * Nq, h * dv), dtype=torch.bfloat16), torch.empty((b, h, Nq))
    width, rows_used = h * (dv if which % 3 == 2 else dqk), (Nq if which % 3 == 0 else Nk)
    for what, v in bad_operands((views + grads)[which], width, rows_used).items():
        ops_ = list(views + grads)
        ops_[which] = v
        with pytest.raises(ValueError, match=f"operand {('q', 'k', 'v', 'dq', 'dk', 'dv')[which]}:"):
            E.attention_bwd(*ops_[:3], O, O, LSE, *ops_[3:], b, h, Nq, Nk, dqk, dv, 0.125, dq_ctx_rows=ctx)


def test_backward_refuses_context_rows_that_are_not_dq_first_row(unreachable):
    views, _, (b, h, Nq, Nk, dqk, dv), ctx = sites()['tower']
    grads = tuple(like(v, torch.empty_like(v.t)) for v in views)
    O, LSE = torch.empty((b * Nq, h * dv), dtype=torch.bfloat16), torch.empty((b, h, Nq))
    for rows in (ctx - 1, ctx + 1):
        with pytest.raises(ValueError, match='operand dq:'):
            E.attention_bwd(*views, O, O, LSE, *grads, b, h, Nq, Nk, dqk, dv, 0.125, dq_ctx_rows=rows)
    # the aggregation's dq starts at row 0: any context-row count is wrong there
    views, _, (b, h, Nq, Nk, dqk, dv), _ = sites()['aggregation']
    grads = tuple(like(v, torch.empty_like(v.t)) for v in views)
    O, LSE = torch.empty((b * Nq, h * dv), dtype=torch.bfloat16), torch.empty((b, h, Nq))
    with pytest.raises(ValueError, match='operand dq:'):
        E.attention_bwd(*views, O, O, LSE, *grads, b, h, Nq, Nk, dqk, dv, 0.125, dq_ctx_rows=1)


@pytest.mark.parametrize('site', SITES)
def test_table_rows_pass_and_reach_the_library_with_the_literal_layout(recorded, site):
    views, want, (b, h, Nq, Nk, dqk, dv), ctx = sites()[site]
    grads = tuple(like(v, torch.empty_like(v.t)) for v in views)
    extra, entry = {}, ('attn_fwd', 'attn_bwd')
    if site == 'swin':
        ld = 32
        bias = torch.empty((nW, h, Nq, ld))
        extra, entry = dict(bias=(bias, nW, ld)), ('attn_bias_fwd', 'attn_bias_bwd')
    O, LSE = E.attention_fwd(*views, b, h, Nq, Nk, dqk, dv, 0.125, **extra)
    assert O.shape == (b * Nq, h * dv) and LSE.shape == (b, h, Nq) and LSE.dtype == torch.float32
    if site == 'swin':
        extra['dS'] = torch.empty((b, h, Nq, ld))
    E.attention_bwd(*views, O, O, LSE, *grads, b, h, Nq, Nk, dqk, dv, 0.125, dq_ctx_rows=ctx, **extra)
    (fn, fa, fk), (bn, ba, bk) = recorded
    assert (fn, bn) == entry
    es = 2                                                                   # bf16 operands
    strides = [x for (_, bs, rs) in want for x in (bs, rs)]
    o_strides = [Nq * h * dv, h * dv]
    # forward: q, k, v addresses, O, LSE, the problem, the operand strides, O's strides, scale [, bias, nb, ld]
    assert [p - v.t.data_ptr() for p, v in zip(fa[:3], views)] == [es * off for (off, _, _) in want]
    assert fa[3] is O and fa[4] is LSE
    assert list(fa[5:11]) == [b, h, Nq, Nk, dqk, dv]
    assert list(fa[11:20]) == strides + o_strides + [0.125]
    # backward: the same in front, Delta, the gradient addresses and — behind O's and dO's strides — the gradient strides
    assert [p - v.t.data_ptr() for p, v in zip(ba[:3], views)] == [es * off for (off, _, _) in want]
    assert ba[3] is O and ba[4] is O and ba[5] is LSE and ba[6].shape == LSE.shape
    assert [p - v.t.data_ptr() for p, v in zip(ba[7:10], grads)] == [es * off for (off, _, _) in want]
    assert list(ba[10:16]) == [b, h, Nq, Nk, dqk, dv]
    assert list(ba[16:33]) == strides + o_strides + o_strides + strides + [0.125]
    if site == 'swin':
        assert fa[20] is bias and list(fa[21:]) == [nW, ld] and not fk
        assert ba[33] is bias and list(ba[34:36]) == [nW, ld] and ba[36] is extra['dS'] and bk == dict(part=3)
    else:
        assert len(fa) == 20 and not fk
        assert len(ba) == 33 and bk == dict(part=3, dq_ctx_rows=ctx)
