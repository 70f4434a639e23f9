"""Thin torch-tensor wrappers over the C ABI (include/dav_kernels.h).

PyTorch is used here only for device memory and streams: every wrapper passes raw
device pointers plus torch's *current* HIP stream to the HIP library, so the calls
are ordered with surrounding torch work and can be captured in a hipGraph.
There is no fallback path: a missing library or a non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib

BF16 = torch.bfloat16
F32 = torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


# While a launch batch is being recorded (engine.batch / dav_batch_begin) kernels run LATER than the Python code that
# "launches" them, so every tensor handed to the library is kept alive until the batch has been issued: torch's caching
# allocator would otherwise hand a temporary's block to a later allocation of the same recording, and with lanes issued
# in lockstep that later kernel may run BEFORE the temporary's last reader.
import threading

_TLS = threading.local()          # .hold: list while THIS thread records a batch (the library's batch state is per thread too:
                                  # autograd runs the backward — and its batches — on its own thread)


def hold(*tensors):
    h = getattr(_TLS, 'hold', None)
    if h is not None:
        h.extend(t for t in tensors if t is not None)


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('deepavfusion_amd kernels need tensors on an MI355X (cuda) device; there is no CPU fallback')
    h = getattr(_TLS, 'hold', None)
    if h is not None:
        h.append(t)
    return t.data_ptr()


def batch_begin(auto_lanes=False):
    _lib.check(_lib.load().dav_batch_begin(int(auto_lanes)), 'dav_batch_begin')
    _TLS.hold = []


def batch_lane():
    _lib.check(_lib.load().dav_batch_lane(), 'dav_batch_lane')


def batch_skip(steps):
    _lib.check(_lib.load().dav_batch_skip(int(steps)), 'dav_batch_skip')


def batch_region(begin):
    _lib.check(_lib.load().dav_batch_region(int(begin)), 'dav_batch_region')


class unbatched:
    """Launches inside go out at once even while a batch is being recorded (weight-cache refreshes: nothing recorded
    so far depends on them, the launches recorded next read their result)."""

    def __enter__(self):
        self.on = getattr(_TLS, 'hold', None) is not None
        if self.on:
            _lib.load().dav_batch_suspend(1)

    def __exit__(self, *exc):
        if self.on:
            _lib.load().dav_batch_suspend(0)
        return False


def batch_end(abort=False):
    """Issue (or drop) the recorded launches; returns (recorded, issued) launch counts."""
    lib = _lib.load()
    try:
        if abort:
            lib.dav_batch_abort()
            return 0, 0
        _lib.check(lib.dav_batch_end(), 'dav_batch_end')
        a, b = C.c_int(0), C.c_int(0)
        lib.dav_batch_stats(C.byref(a), C.byref(b))
        return a.value, b.value
    finally:
        _TLS.hold = None


def _rm(m: Optional[Sequence[int]]):
    return (C.c_int * 3)(*m) if m is not None else None


def gemm_nt(A, B, M, N, K, *, lda=None, ldb=None, a_rowmap=None, bias=None, act=0, aux=None, ldaux=0, res=None, ldres=0,
            res_rowmap=None, res_rows=None, C_out=None, ldc=None, c_bf16=False, c_rowmap=None, C2=None, ldc2=0, c2_mode=0,
            beta=0, alpha=1.0, variant=0):
    """C[M,N] = epi(A[M,K] . B[N,K]^T); see dav_gemm_nt_bf16 (fp32 operands: dav_gemm_nt_f32, csrc/f32_path.hip)."""
    lib = _lib.load()
    if A.dtype == F32:                  # (c_bf16 is meaningless here: every output of the fp32 path is fp32)
        _lib.check(lib.dav_gemm_nt_f32(_ptr(A), _ptr(B), M, N, K, lda if lda is not None else K, ldb if ldb is not None else K,
                                       _rm(a_rowmap), _ptr(bias), act, _ptr(aux), ldaux, _ptr(res), ldres, _rm(res_rowmap),
                                       _ptr(res_rows), _ptr(C_out), ldc if ldc is not None else N, _rm(c_rowmap), _ptr(C2), ldc2,
                                       c2_mode, beta, float(alpha), (variant >> 12) & 1, _stream()), 'dav_gemm_nt_f32')
        return
    _lib.check(lib.dav_gemm_nt_bf16(_ptr(A), _ptr(B), M, N, K, lda if lda is not None else K, ldb if ldb is not None else K,
                                    _rm(a_rowmap), _ptr(bias), act, _ptr(aux), ldaux, _ptr(res), ldres, _rm(res_rowmap),
                                    _ptr(res_rows), _ptr(C_out), ldc if ldc is not None else N, int(c_bf16), _rm(c_rowmap),
                                    _ptr(C2), ldc2, c2_mode, beta, float(alpha), variant, _stream()), 'dav_gemm_nt_bf16')


def gemm_nt_ln(A, B, M, N, K, *, ln=None, prod=None, lda=None, ldb=None, a_rowmap=None, bias=None, act=0, aux=None, ldaux=0, res=None,
               ldres=0, res_rowmap=None, res_rows=None, C_out=None, ldc=None, c_bf16=False, c_rowmap=None, C2=None, ldc2=0,
               c2_mode=0, beta=0, variant=0):
    """dav_gemm_nt_ln_bf16 (bf16 path only).  ``ln`` = dict(stats, ln_c, eps[, A2, stats2, a_r0, a_r1]): A holds RAW twin rows, B the
    gamma-folded weight, ``bias`` the folded bias (consumer side).  ``prod`` = dict(stats_out=..., twin_out=..., ld_twin=...):
    row-statistics partials + bf16 twin of the fp32 result (producer side)."""
    lib = _lib.load()
    q = _lib.DavNtLn()
    if ln is not None:
        q.stats, q.ln_c, q.eps = _ptr(ln['stats']), _ptr(ln['ln_c']), float(ln['eps'])
        q.stats2, q.A2 = _ptr(ln.get('stats2')), _ptr(ln.get('A2'))
        q.a_r0, q.a_r1 = int(ln.get('a_r0', 0)), int(ln.get('a_r1', 0))
    if prod is not None:
        q.stats_out, q.twin_out, q.ld_twin = _ptr(prod.get('stats_out')), _ptr(prod.get('twin_out')), int(prod.get('ld_twin', N))
    _lib.check(lib.dav_gemm_nt_ln_bf16(_ptr(A), _ptr(B), M, N, K, lda if lda is not None else K, ldb if ldb is not None else K,
                                       _rm(a_rowmap), _ptr(bias), act, _ptr(aux), ldaux, _ptr(res), ldres, _rm(res_rowmap),
                                       _ptr(res_rows), _ptr(C_out), ldc if ldc is not None else N, int(c_bf16), _rm(c_rowmap),
                                       _ptr(C2), ldc2, c2_mode, beta, 1.0, variant, C.byref(q), _stream()), 'dav_gemm_nt_ln_bf16')


LN_FOLD_MAX = 48          # dav_ln_fold_grouped: pairs per launch


def ln_fold_grouped(items):
    """items: [(w fp32 [N, K], gamma, beta, bias or None, w_ln_bf16, ln_c, ln_d), ...] (dav_ln_fold_grouped)."""
    lib = _lib.load()
    for i in range(0, len(items), LN_FOLD_MAX):
        chunk = items[i:i + LN_FOLD_MAX]
        arr = (_lib.DavLnFold * len(chunk))()
        for q, (w, g, b, bias, wl, c, d) in zip(arr, chunk):
            q.w, q.gamma, q.beta, q.bias, q.w_ln_bf16, q.ln_c, q.ln_d = _ptr(w), _ptr(g), _ptr(b), _ptr(bias), _ptr(wl), _ptr(c), _ptr(d)
            q.N, q.K = int(w.shape[0]), int(w.shape[1])
        _lib.check(lib.dav_ln_fold_grouped(arr, len(chunk), _stream()), 'dav_ln_fold_grouped')


def rowstats_cast(x, x_bs, B, rows, D, twin, stats):
    """bf16 twin + per-row {sum, sum of squares} partials over 64-column slots of fp32 rows (dav_rowstats_cast)."""
    _lib.check(_lib.load().dav_rowstats_cast(_ptr(x), x_bs, B, rows, D, _ptr(twin), _ptr(stats), _stream()), 'dav_rowstats_cast')


def layernorm_bwd_twin(xb0, xb0_bs, st0, r0, xb1, xb1_bs, st1, r1, B, D, eps, dy_bf16, dy_f32, gamma, beta,
                       dx0=None, dx0_bs=0, acc0=0, res0=None, res0_bs=0, dx0_bf16=None, dx0_bf_bs=0,
                       dx1=None, dx1_bs=0, acc1=0, res1=None, res1_bs=0, dx1_bf16=None, dx1_bf_bs=0, h_out=None, dgamma=None, dbeta=None,
                       defer=None):
    """dav_layernorm_bwd_twin; xb* / st* / dx* may be (tensor, element offset) pairs.  ``defer`` as layernorm_bwd."""
    lib = _lib.load()

    def po(t):
        if t is None:
            return None
        if isinstance(t, tuple):
            return _ptr(t[0]) + t[0].element_size() * t[1]
        return _ptr(t)
    ws = None
    if dgamma is not None:
        ws = torch.empty(lib.dav_layernorm_bwd_workspace_bytes(B * (r0 + r1), D) // 4, dtype=F32, device=dgamma.device)
        if defer is not None:
            defer.append((ws, dgamma, dbeta, B * (r0 + r1), D))
            dgamma = dbeta = None
    _lib.check(lib.dav_layernorm_bwd_twin(po(xb0), xb0_bs, po(st0), r0, po(xb1), xb1_bs, po(st1), r1, B, D, float(eps),
                                          _ptr(dy_bf16), _ptr(dy_f32), _ptr(gamma), _ptr(beta),
                                          po(dx0), dx0_bs, acc0, po(res0), res0_bs, po(dx0_bf16), dx0_bf_bs,
                                          po(dx1), dx1_bs, acc1, po(res1), res1_bs, po(dx1_bf16), dx1_bf_bs,
                                          _ptr(h_out), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel() * 4 if ws is not None else 0,
                                          _stream()), 'dav_layernorm_bwd_twin')


def nt_issue_log(enable=None, with_flags=False):
    """enable True / False: start (clearing) / stop logging the NT launches the library issues; None: fetch the log as a
    list of (cfg, b_kn, [(M, N, K), ...]) — one entry per launch (grouped launches have several problems); with_flags adds a
    fourth element, the problems' epilogue flags (act | c_bf16 << 2 | has_res << 3 | c2_mode << 4 | beta << 8)."""
    lib = _lib.load()
    if enable is not None:
        lib.dav_nt_issue_log(int(enable), None, 0)
        return None
    n = -lib.dav_nt_issue_log(0, (C.c_int * 1)(), 0)
    if n <= 0:
        return []
    buf = (C.c_int * n)()
    lib.dav_nt_issue_log(0, buf, n)
    out, i = [], 0
    while i < n:
        cfg, bt, cnt = buf[i], buf[i + 1], buf[i + 2]
        probs = [(buf[i + 3 + 4 * j], buf[i + 4 + 4 * j], buf[i + 5 + 4 * j]) for j in range(cnt)]
        flags = [buf[i + 6 + 4 * j] for j in range(cnt)]
        out.append((cfg, bt, probs, flags) if with_flags else (cfg, bt, probs))
        i += 3 + 4 * cnt
    return out


def gemm_tn(A, B, Mc, N, K, C_out, *, lda=None, ldb=None, ldc=None, a_rowmap=None, b_rowmap=None, beta=1, bias_grad=None,
            variant=0):
    """C[N,K] (+)= A[Mc,N]^T . B[Mc,K]; see dav_gemm_tn_bf16 (fp32 operands: dav_gemm_tn_f32)."""
    lib = _lib.load()
    if A.dtype == F32:
        _lib.check(lib.dav_gemm_tn_f32(_ptr(A), _ptr(B), Mc, N, K, lda if lda is not None else N, ldb if ldb is not None else K,
                                       _rm(a_rowmap), _rm(b_rowmap), _ptr(C_out), ldc if ldc is not None else K, beta,
                                       _ptr(bias_grad), _stream()), 'dav_gemm_tn_f32')
        return
    _lib.check(lib.dav_gemm_tn_bf16(_ptr(A), _ptr(B), Mc, N, K, lda if lda is not None else N, ldb if ldb is not None else K,
                                    _rm(a_rowmap), _rm(b_rowmap), _ptr(C_out), ldc if ldc is not None else K, beta,
                                    _ptr(bias_grad), variant, _stream()), 'dav_gemm_tn_bf16')


TN_GROUP_MAX = 40          # dav_gemm_tn_grouped_bf16: problems per launch


def _gate_ptr(gate):
    if gate.dtype != torch.int32 or gate.numel() != 1 or not gate.is_cuda:
        raise ValueError('write gate: one int32 element in device memory')
    return _ptr(gate)


def gemm_tn_grouped(problems, gate=None):
    """problems: list of dicts(A, B, Mc, N, K, C, lda, ldb, ldc, a_rowmap, b_rowmap, bias_grad[, overwrite]); see
    dav_gemm_tn_grouped_bf16 (overwrite: C is written instead of accumulated, DavTnProblem.flags bit 0).  ``gate`` (int32 [1] on the
    device): the ``overwrite`` problems are written only while gate[0] != 0 when the launch RUNS, else accumulated
    (dav_gemm_tn_grouped_bf16_gated; bf16 operands only)."""
    lib = _lib.load()
    if problems and problems[0]['A'].dtype == F32:      # fp32 path: one launch per problem
        if gate is not None and any(d.get('overwrite') for d in problems):
            raise RuntimeError('gemm_tn_grouped: the fp32 path has no gated form; queue its problems without overwrite')
        for d in problems:
            gemm_tn(d['A'], d['B'], d['Mc'], d['N'], d['K'], d['C'], lda=d['lda'], ldb=d['ldb'], ldc=d['ldc'],
                    a_rowmap=d.get('a_rowmap'), b_rowmap=d.get('b_rowmap'), beta=0 if d.get('overwrite') else 1,
                    bias_grad=d.get('bias_grad'))
        return
    # more than one launch (40 problems each at most): deal the list out in turns, so that every launch gets its share of the long
    # and of the short contractions — cut consecutively, 68 problems became 32 long + 32 medium + 4 small ones whose ~100 tiles
    # had the 512 workgroup slots to themselves for a whole contraction
    n_launch = (len(problems) + TN_GROUP_MAX - 1) // TN_GROUP_MAX
    for i in range(n_launch):
        chunk = problems[i::n_launch]
        if gate is not None:
            _lib.check(lib.dav_gemm_tn_grouped_bf16_gated(_tn_problem_array(chunk), len(chunk), _gate_ptr(gate), _stream()),
                       'dav_gemm_tn_grouped_bf16_gated')
            continue
        _lib.check(lib.dav_gemm_tn_grouped_bf16(_tn_problem_array(chunk), len(chunk), _stream()), 'dav_gemm_tn_grouped_bf16')


def _tn_problem_array(problems):
    arr = (_lib.DavTnProblem * len(problems))()
    for q, d in zip(arr, problems):
        q.A, q.B, q.C, q.bias_grad = _ptr(d['A']), _ptr(d['B']), _ptr(d['C']), _ptr(d.get('bias_grad'))
        q.Mc, q.N, q.K, q.lda, q.ldb, q.ldc = d['Mc'], d['N'], d['K'], d['lda'], d['ldb'], d['ldc']
        q.a_rowmap[:] = d.get('a_rowmap') or (0, 0, 0)
        q.b_rowmap[:] = d.get('b_rowmap') or (0, 0, 0)
        q.flags = 1 if d.get('overwrite') else 0
    return arr


def gemm_tn_gang(problems, workspace_fill=None, gate=None):
    """The queued weight-gradient problems of several layers (dicts as for gemm_tn_grouped, no two with the same C) as ONE
    gang-scheduled launch of 256 x 256 tiles (dav_gemm_tn_gang_bf16).  The workspace is allocated here on the current stream
    (``workspace_fill``: a byte value to fill it with first — tests check that the kernel initialises its own state).
    ``gate``: as for gemm_tn_grouped (dav_gemm_tn_gang_bf16_gated)."""
    if not problems:
        return
    if problems[0]['A'].dtype == F32:
        return gemm_tn_grouped(problems) if gate is None else gemm_tn_grouped(problems, gate)
    lib = _lib.load()
    arr = _tn_problem_array(problems)
    nbytes = int(lib.dav_gemm_tn_gang_workspace_bytes(arr, len(problems)))
    if nbytes == 0:
        raise RuntimeError('dav_gemm_tn_gang_workspace_bytes: invalid weight-gradient problem (shape / alignment)')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=problems[0]['A'].device)
    if workspace_fill is not None:
        ws.fill_(workspace_fill)
    hold(ws)
    if gate is not None:
        _lib.check(lib.dav_gemm_tn_gang_bf16_gated(arr, len(problems), _ptr(ws), nbytes, _gate_ptr(gate), _stream()), 'dav_gemm_tn_gang_bf16_gated')
        return
    _lib.check(lib.dav_gemm_tn_gang_bf16(arr, len(problems), _ptr(ws), nbytes, _stream()), 'dav_gemm_tn_gang_bf16')


def _attn_fwd_call(variant, q_ptr, k_ptr, v_ptr, O, LSE, dims, scale, tail=()):
    """The argument block all forward attention entry points share.  ``variant`` ('' / '_bias' / '_drop') and the dtype of ``O`` pick
    the entry point, ``dims`` = (B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs), ``tail`` = the variant's own
    arguments, which follow ``scale`` in the C signature (_lib.SIGNATURES)."""
    name = 'dav_attn' + variant + '_fwd' + ('_f32' if O.dtype == F32 else '')
    _lib.check(getattr(_lib.load(), name)(q_ptr, k_ptr, v_ptr, _ptr(O), _ptr(LSE), *dims, float(scale), *tail, _stream()), name)


def _attn_bwd_call(variant, q_ptr, k_ptr, v_ptr, O, dO, LSE, Delta, dq_ptr, dk_ptr, dv_ptr, dims, scale, part, tail=(), dq_ctx_rows=0):
    """The backward counterpart: ``dims`` = (B, H, Nq, Nk, dqk, dv) + the (batch, row) strides of q, k, v, O, dO, dq, dk, dv.  C order
    behind ``scale``: the variant's ``tail``, the context-row count (dav_attn_bwd_ctx and dav_attn_drop_bwd only), ``part``.  The
    callers refuse ``dq_ctx_rows`` on the fp32 path, which has no such entry."""
    f32 = O.dtype == F32
    if variant == '':
        entry = 'dav_attn_bwd_f32' if f32 else ('dav_attn_bwd_ctx' if dq_ctx_rows else 'dav_attn_bwd_part')
    else:
        entry = 'dav_attn' + variant + '_bwd' + ('_f32' if f32 else '')
    ctx = (int(dq_ctx_rows),) if entry in ('dav_attn_bwd_ctx', 'dav_attn_drop_bwd') else ()
    _lib.check(getattr(_lib.load(), entry)(q_ptr, k_ptr, v_ptr, _ptr(O), _ptr(dO), _ptr(LSE), _ptr(Delta), dq_ptr, dk_ptr, dv_ptr, *dims,
                                           float(scale), *tail, *ctx, part, _stream()),
               'dav_attn_bwd' if entry == 'dav_attn_bwd_part' else entry)


def attn_fwd(q_ptr, k_ptr, v_ptr, O, LSE, B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs, scale):
    """q / k / v are raw addresses (views into fused projection buffers) of the dtype of ``O``."""
    _attn_fwd_call('', q_ptr, k_ptr, v_ptr, O, LSE, (B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs), scale)


def attn_bias_fwd(q_ptr, k_ptr, v_ptr, O, LSE, B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs, scale,
                  bias, bias_nb, bias_ld):
    """attn_fwd with an additive logit bias [bias_nb, H, Nq, bias_ld] (bf16 path: log2 units; fp32 path: natural units)."""
    _attn_fwd_call('_bias', q_ptr, k_ptr, v_ptr, O, LSE, (B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs), scale,
                   (_ptr(bias), bias_nb, bias_ld))


def attn_bias_bwd(q_ptr, k_ptr, v_ptr, O, dO, LSE, Delta, dq_ptr, dk_ptr, dv_ptr, B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs,
                  v_bs, v_rs, o_bs, o_rs, do_bs, do_rs, dq_bs, dq_rs, dk_bs, dk_rs, dv_bs, dv_rs, scale, bias, bias_nb, bias_ld,
                  dS, part=3):
    """attn_bwd with the bias of the forward; dS [B, H, Nq, bias_ld] fp32 receives the gradient of the biased logits."""
    _attn_bwd_call('_bias', q_ptr, k_ptr, v_ptr, O, dO, LSE, Delta, dq_ptr, dk_ptr, dv_ptr,
                   (B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs, do_bs, do_rs, dq_bs, dq_rs, dk_bs, dk_rs,
                    dv_bs, dv_rs), scale, part, (_ptr(bias), bias_nb, bias_ld, _ptr(dS)))


def window_unfold(src, rows32, B, nW, A, nF, L, Cc, fusion_scale, out):
    """[B, nF + L, C] rows -> [B * nW, A + nF, C] window sequences (see dav_window_unfold)."""
    _lib.check(_lib.load().dav_window_unfold(_ptr(src), int(src.dtype == BF16), _ptr(rows32), B, nW, A, nF, L, Cc, float(fusion_scale),
                                             _ptr(out), int(out.dtype == BF16), _stream()), 'dav_window_unfold')


def window_fold(t, inv32, res, B, nW, A, nF, L, Cc, fusion_scale, out):
    """[B * nW, A + nF, C] fp32 sequences (+ res) -> [B, nF + L, C] fp32 rows (see dav_window_fold)."""
    _lib.check(_lib.load().dav_window_fold(_ptr(t), _ptr(inv32), _ptr(res), B, nW, A, nF, L, Cc, float(fusion_scale), _ptr(out),
                                           _stream()), 'dav_window_fold')


def relpos_bias_build(table, index32, mask, nb, H, A, N, ld, mul, out):
    _lib.check(_lib.load().dav_relpos_bias_build(_ptr(table), _ptr(index32), _ptr(mask), nb, H, A, N, ld, float(mul), _ptr(out),
                                                 _stream()), 'dav_relpos_bias_build')


def relpos_bias_bwd(dS, index32, Bw, H, A, N, ld, T, dtable):
    _lib.check(_lib.load().dav_relpos_bias_bwd(_ptr(dS), _ptr(index32), Bw, H, A, N, ld, T, _ptr(dtable), _stream()),
               'dav_relpos_bias_bwd')


def attn_bwd(q_ptr, k_ptr, v_ptr, O, dO, LSE, Delta, dq_ptr, dk_ptr, dv_ptr, B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs,
             v_bs, v_rs, o_bs, o_rs, do_bs, do_rs, dq_bs, dq_rs, dk_bs, dk_rs, dv_bs, dv_rs, scale, part=3, dq_ctx_rows=0):
    """part 1: dQ (+ Delta) kernel only, 2: dK/dV kernel only (after part 1), 3: both.  dq_ctx_rows (bf16 path): rows in front of
    the first query row of every batch element of the dQ buffer whose dqk columns the dQ kernel zero-fills (dav_attn_bwd_ctx)."""
    if O.dtype == F32 and dq_ctx_rows:
        raise RuntimeError('dq_ctx_rows: bf16 path only')
    _attn_bwd_call('', q_ptr, k_ptr, v_ptr, O, dO, LSE, Delta, dq_ptr, dk_ptr, dv_ptr,
                   (B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs, do_bs, do_rs, dq_bs, dq_rs, dk_bs, dk_rs,
                    dv_bs, dv_rs), scale, part, dq_ctx_rows=dq_ctx_rows)


ATTN_RESIDENT_MAX = 80 * 1024      # csrc/attention.hip: LDS of a resident attention workgroup (two per CU)


def attn_bwd_onepass_lds(Nq, Nk, dqk, dv):
    """Dynamic LDS bytes of the one-pass attention backward (csrc/attention.hip attn_lds<.., 3>): Q, dO and K tiles with rows padded to
    32 and head widths to at least 32 columns, the bf16 dS^T patch, LSE + Delta."""
    nqp, nkp = (Nq + 31) & ~31, (Nk + 31) & ~31
    return nqp * (2 * max(dqk, 32) + 2 * max(dv, 32)) + nkp * 2 * max(dqk, 32) + nqp * nkp * 2 + nqp * 8


def attn_bwd_onepass_fits(Nq, Nk, dqk, dv):
    """Mirror of onepass_fits (csrc/attention.hip) at the default knob setting: does ``attn_bwd(part=3)`` without bias / dropout go
    out as ONE launch?  (Not when it is recorded into a lane of a launch batch: there a backward keeps its two ranks.)  The engine
    chooses one region or two for the aggregations' backward with it; the library decides on its own."""
    return (dqk, dv) in ((64, 64), (16, 64)) and attn_bwd_onepass_lds(Nq, Nk, dqk, dv) <= ATTN_RESIDENT_MAX


def layernorm_fwd(x0, x0_bs, r0, x1, x1_bs, r1, B, D, gamma, beta, eps, y_bf16, y_f32, mean, rstd):
    lib = _lib.load()
    if y_bf16 is not None and y_bf16.dtype == F32:      # fp32 path: the "operand copy" of the output is fp32 too
        if y_f32 is not None and y_f32.data_ptr() != y_bf16.data_ptr():
            raise RuntimeError('fp32 LayerNorm: pass one output buffer')
        y_bf16, y_f32 = None, y_bf16
    _lib.check(lib.dav_layernorm_fwd(_ptr(x0), x0_bs, r0, _ptr(x1), x1_bs, r1, B, D, _ptr(gamma), _ptr(beta), float(eps),
                                     _ptr(y_bf16), _ptr(y_f32), _ptr(mean), _ptr(rstd), _stream()), 'dav_layernorm_fwd')


def layernorm_bwd(x0, x0_bs, r0, x1, x1_bs, r1, B, D, dy_bf16, dy_f32, gamma, mean, rstd,
                  dx0=None, dx0_bs=0, acc0=0, res0=None, res0_bs=0, dx0_bf16=None, dx0_bf_bs=0,
                  dx1=None, dx1_bs=0, acc1=0, res1=None, res1_bs=0, dx1_bf16=None, dx1_bf_bs=0, dgamma=None, dbeta=None,
                  defer=None):
    """``defer``: a list; when given, only the partial dgamma/dbeta rows are produced and
    (workspace, dgamma, dbeta, rows, D) is appended for a later ``layernorm_bwd_reduce_grouped``."""
    lib = _lib.load()
    twins = []
    if dy_bf16 is not None and dy_bf16.dtype == F32:    # fp32 path: both gradient inputs are fp32 -> one (summed) fp32 input
        if dy_f32 is not None:
            tmp = torch.empty_like(dy_bf16)
            _lib.check(lib.dav_add_f32(_ptr(dy_bf16), _ptr(dy_f32), _ptr(tmp), tmp.numel(), _stream()), 'dav_add_f32')
            dy_f32 = tmp
        else:
            dy_f32 = dy_bf16
        dy_bf16 = None
    if dx0_bf16 is not None and dx0_bf16.dtype == F32:  # ... and the "bf16 twins" of the outputs are fp32 row copies
        twins.append((dx0, dx0_bs, r0, dx0_bf16, dx0_bf_bs))
        dx0_bf16 = None
    if dx1_bf16 is not None and dx1_bf16.dtype == F32:
        twins.append((dx1, dx1_bs, r1, dx1_bf16, dx1_bf_bs))
        dx1_bf16 = None
    ws = None
    if dgamma is not None:
        ws = torch.empty(lib.dav_layernorm_bwd_workspace_bytes(B * (r0 + r1), D) // 4, dtype=F32, device=dgamma.device)
        if defer is not None:
            defer.append((ws, dgamma, dbeta, B * (r0 + r1), D))
            dgamma = dbeta = None
    _lib.check(lib.dav_layernorm_bwd(_ptr(x0), x0_bs, r0, _ptr(x1), x1_bs, r1, B, D, _ptr(dy_bf16), _ptr(dy_f32),
                                     _ptr(gamma), _ptr(mean), _ptr(rstd),
                                     _ptr(dx0), dx0_bs, acc0, _ptr(res0), res0_bs, _ptr(dx0_bf16), dx0_bf_bs,
                                     _ptr(dx1), dx1_bs, acc1, _ptr(res1), res1_bs, _ptr(dx1_bf16), dx1_bf_bs,
                                     _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel() * 4 if ws is not None else 0, _stream()),
               'dav_layernorm_bwd')
    for (dx, bs, rows, twin, twin_bs) in twins:
        _lib.check(lib.dav_rows_gather_f32(_ptr(dx), bs, 0, None, B, rows, D, _ptr(twin), twin_bs, _stream()), 'dav_rows_gather_f32')


def layernorm_bwd_reduce_grouped(items):
    lib = _lib.load()
    for i in range(0, len(items), 64):
        chunk = items[i:i + 64]
        arr = (_lib.DavLnReduce * len(chunk))()
        for q, (ws, dg, db, rows, D) in zip(arr, chunk):
            q.workspace, q.dgamma, q.dbeta, q.rows, q.D = _ptr(ws), _ptr(dg), _ptr(db), rows, D
        _lib.check(lib.dav_layernorm_bwd_reduce_grouped(arr, len(chunk), _stream()), 'dav_layernorm_bwd_reduce_grouped')


def mask_build(noise: torch.Tensor, len_keep: int):
    """AVMAE.random_masking for given noise -> (ids_keep i64, mask f32, ids_restore i64, ids_keep i32, ids_restore i32)."""
    lib = _lib.load()
    N, L = noise.shape
    dev = noise.device
    ids_keep = torch.empty(N, len_keep, dtype=torch.int64, device=dev)
    ids_restore = torch.empty(N, L, dtype=torch.int64, device=dev)
    mask = torch.empty(N, L, dtype=F32, device=dev)
    ids_keep32 = torch.empty(N, len_keep, dtype=torch.int32, device=dev)
    ids_restore32 = torch.empty(N, L, dtype=torch.int32, device=dev)
    _lib.check(lib.dav_mask_build(_ptr(noise.contiguous()), N, L, len_keep, _ptr(ids_keep), _ptr(ids_restore), _ptr(mask),
                                  _ptr(ids_keep32), _ptr(ids_restore32), _stream()), 'dav_mask_build')
    return ids_keep, mask, ids_restore, ids_keep32, ids_restore32


def patch_gather(img, ids_keep32, nk, out, pt=1):
    """img [B,C,H,W] with 16x16 patches, or a clip [B,C,T,H,W] with (pt,16,16) tubelets."""
    lib = _lib.load()
    if out.dtype == F32:
        if img.dim() == 5:
            B, Cc, T, H, W = img.shape
        else:
            (B, Cc, H, W), T = img.shape, 1
        _lib.check(lib.dav_patch_gather_f32(_ptr(img), B, Cc, T, H, W, pt, _ptr(ids_keep32), nk, _ptr(out), _stream()), 'dav_patch_gather_f32')
        return
    if img.dim() == 5:
        B, Cc, T, H, W = img.shape
        _lib.check(lib.dav_patch_gather3d(_ptr(img), B, Cc, T, H, W, pt, _ptr(ids_keep32), nk, _ptr(out), _stream()),
                   'dav_patch_gather3d')
        return
    B, Cc, H, W = img.shape
    _lib.check(lib.dav_patch_gather(_ptr(img), B, Cc, H, W, _ptr(ids_keep32), nk, _ptr(out), _stream()), 'dav_patch_gather')


def unshuffle_fwd(emb, mask_token, pos, ids_restore32, B, L, nk, D, out, out_bs, out_row_off):
    lib = _lib.load()
    _lib.check(lib.dav_unshuffle_fwd(_ptr(emb), _ptr(mask_token), _ptr(pos), _ptr(ids_restore32), B, L, nk, D, _ptr(out),
                                     out_bs, out_row_off, _stream()), 'dav_unshuffle_fwd')


def rows_gather_cast(x, x_bs, row_off, ids32, B, n, D, out):
    lib = _lib.load()
    if out.dtype == F32:
        _lib.check(lib.dav_rows_gather_f32(_ptr(x), x_bs, row_off, _ptr(ids32), B, n, D, _ptr(out), 0, _stream()), 'dav_rows_gather_f32')
        return
    _lib.check(lib.dav_rows_gather_cast(_ptr(x), x_bs, row_off, _ptr(ids32), B, n, D, _ptr(out), _stream()), 'dav_rows_gather_cast')


def unshuffle_bwd_reduce(dx, dx_bs, row_off, ids_restore32, B, L, nk, D, dpos, dmask_token):
    lib = _lib.load()
    _lib.check(lib.dav_unshuffle_bwd_reduce(_ptr(dx), dx_bs, row_off, _ptr(ids_restore32), B, L, nk, D, _ptr(dpos),
                                            _ptr(dmask_token), _stream()), 'dav_unshuffle_bwd_reduce')


def patch_mse_fwd(img, pred, mask, norm_pix, loss_patch, tmean, trstd, loss, mask_sum):
    lib = _lib.load()
    B, Cc, H, W = img.shape
    _lib.check(lib.dav_patch_mse_fwd(_ptr(img), _ptr(pred), _ptr(mask), B, Cc, H, W, int(norm_pix), _ptr(loss_patch),
                                     _ptr(tmean), _ptr(trstd), _ptr(loss), _ptr(mask_sum), _stream()), 'dav_patch_mse_fwd')


def patch_mse_bwd(img, pred, mask, tmean, trstd, mask_sum, gout, dpred_bf16):
    lib = _lib.load()
    B, Cc, H, W = img.shape
    if dpred_bf16.dtype == F32:
        _lib.check(lib.dav_patch_mse_bwd_f32(_ptr(img), _ptr(pred), _ptr(mask), _ptr(tmean), _ptr(trstd), _ptr(mask_sum), _ptr(gout),
                                             B, Cc, H, W, _ptr(dpred_bf16), _stream()), 'dav_patch_mse_bwd_f32')
        return
    _lib.check(lib.dav_patch_mse_bwd(_ptr(img), _ptr(pred), _ptr(mask), _ptr(tmean), _ptr(trstd), _ptr(mask_sum), _ptr(gout),
                                     B, Cc, H, W, _ptr(dpred_bf16), _stream()), 'dav_patch_mse_bwd')


def pair_expand(Pv, Pa, B, nv, na, Wd, out):
    lib = _lib.load()
    if out.dtype == F32:
        _lib.check(lib.dav_pair_expand_f32(_ptr(Pv), _ptr(Pa), B, nv, na, Wd, _ptr(out), _stream()), 'dav_pair_expand_f32')
        return
    _lib.check(lib.dav_pair_expand(_ptr(Pv), _ptr(Pa), B, nv, na, Wd, _ptr(out), _stream()), 'dav_pair_expand')


def pair_reduce(d, B, nv, na, Wd, dPv, dPa):
    lib = _lib.load()
    if d.dtype == F32:
        _lib.check(lib.dav_pair_reduce_f32(_ptr(d), B, nv, na, Wd, _ptr(dPv), _ptr(dPa), _stream()), 'dav_pair_reduce_f32')
        return
    _lib.check(lib.dav_pair_reduce(_ptr(d), B, nv, na, Wd, _ptr(dPv), _ptr(dPa), _stream()), 'dav_pair_reduce')


def cast_bf16(x, y):
    lib = _lib.load()
    _lib.check(lib.dav_cast_bf16(_ptr(x), _ptr(y), x.numel(), _stream()), 'dav_cast_bf16')


def cast_transpose_bf16(x2d, y):
    lib = _lib.load()
    R, Cc = x2d.shape
    _lib.check(lib.dav_cast_transpose_bf16(_ptr(x2d), _ptr(y), R, Cc, _stream()), 'dav_cast_transpose_bf16')


def l2norm(x_flat, out, workspace, scale=1.0):
    lib = _lib.load()
    _lib.check(lib.dav_l2norm(_ptr(x_flat), x_flat.numel(), float(scale), _ptr(out), _ptr(workspace),
                              workspace.numel() * workspace.element_size(), _stream()), 'dav_l2norm')


def adamw_flat(p, g, m, v, p_bf16, seg_end, hyper, nseg, beta1, beta2, eps, bias_corr, grad_scale=1.0, sumsq_out=None,
               zero_grad=False, keep_grad=None, gscale_dev=None):
    """keep_grad: uint8 [nseg] or None — segments whose gradient is NOT zero-filled by zero_grad (see dav_adamw_flat).
    gscale_dev: float32 [1] device scalar from ``step_guard`` (clip factor; 0 = skip the update) or None."""
    lib = _lib.load()
    _lib.check(lib.dav_adamw_flat(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), p.numel(), _ptr(seg_end), _ptr(hyper), nseg,
                                  float(beta1), float(beta2), float(eps), _ptr(bias_corr), float(grad_scale), _ptr(sumsq_out),
                                  int(zero_grad), _ptr(keep_grad), _ptr(gscale_dev), _stream()), 'dav_adamw_flat')


def add_cast(a, b):
    """(a + b as fp32, the same as bf16) in one pass (dav_add_cast); a, b: contiguous fp32 of the same shape, numel % 4 == 0."""
    lib = _lib.load()
    out = torch.empty_like(a)
    out_b = torch.empty(a.shape, dtype=BF16, device=a.device)
    _lib.check(lib.dav_add_cast(_ptr(a), _ptr(b), _ptr(out), _ptr(out_b), a.numel(), _stream()), 'dav_add_cast')
    return out, out_b


def step_guard(loss_a, loss_b, gnorm, clip, grad_scale, out_scale, bad_count):
    """Device-side replacement of train.py:166-167 / util/misc.py:118-120 for a captured step (dav_step_guard)."""
    lib = _lib.load()
    _lib.check(lib.dav_step_guard(_ptr(loss_a), _ptr(loss_b), _ptr(gnorm), float(clip if clip else 0.0), float(grad_scale),
                                  _ptr(out_scale), _ptr(bad_count), _stream()), 'dav_step_guard')


def rows_axpy(res, y, scale, B, rows, D, out):
    """out[b, r] = res[b, r] + scale[b] * y[b, r]  (fp32 rows of D; DropPath forward)."""
    lib = _lib.load()
    _lib.check(lib.dav_rows_axpy(_ptr(res), _ptr(y), _ptr(scale), B, rows, D, _ptr(out), _stream()), 'dav_rows_axpy')


def rows_scale_cast(g, scale, B, rows, D, out_bf16):
    """out_bf16[b, r] = bf16(scale[b] * g[b, r])  (DropPath backward, branch side)."""
    lib = _lib.load()
    _lib.check(lib.dav_rows_scale_cast(_ptr(g), _ptr(scale), B, rows, D, _ptr(out_bf16), _stream()), 'dav_rows_scale_cast')


def attn_drop_fwd(q_ptr, k_ptr, v_ptr, O, LSE, B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs, scale,
                  keep, keep_ld, keep_scale):
    """Attention with dropout on the softmax probabilities (dav_attn_drop_fwd / _f32): keep = bytes 0 / 1 [B, H, Nq, keep_ld]."""
    _attn_fwd_call('_drop', q_ptr, k_ptr, v_ptr, O, LSE, (B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs), scale,
                   (_ptr(keep), keep_ld, float(keep_scale)))


def attn_drop_bwd(q_ptr, k_ptr, v_ptr, O, dO, LSE, Delta, dq_ptr, dk_ptr, dv_ptr, B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs,
                  v_bs, v_rs, o_bs, o_rs, do_bs, do_rs, dq_bs, dq_rs, dk_bs, dk_rs, dv_bs, dv_rs, scale, keep, keep_ld, keep_scale,
                  part=3, dq_ctx_rows=0):
    if O.dtype == F32 and dq_ctx_rows:
        raise ValueError('the fp32 attention kernels have no context-row entry')
    _attn_bwd_call('_drop', q_ptr, k_ptr, v_ptr, O, dO, LSE, Delta, dq_ptr, dk_ptr, dv_ptr,
                   (B, H, Nq, Nk, dqk, dv, q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs, do_bs, do_rs, dq_bs, dq_rs, dk_bs, dk_rs,
                    dv_bs, dv_rs), scale, part, (_ptr(keep), keep_ld, float(keep_scale)), dq_ctx_rows)


def dropout_rows(x, keep, keep_scale, B, rows, D, out, res=None, rowscale=None):
    """out[b, r] = (res[b, r] if res else 0) + (rowscale[b] if rowscale else 1) * keep[b, r] * keep_scale * x[b, r]
    (dav_dropout_rows; x / out bf16 or fp32, keep bytes [B * rows, D] or None; out may alias x or res)."""
    lib = _lib.load()
    _lib.check(lib.dav_dropout_rows(_ptr(x), int(x.dtype == F32), _ptr(res), _ptr(keep), float(keep_scale), _ptr(rowscale), B, rows, D,
                                    _ptr(out), int(out.dtype == F32), _stream()), 'dav_dropout_rows')


def cast_transpose_grouped(pairs):
    """pairs: [(x fp32 [R, C], y bf16 [C, R]), ...] -> every y = bf16(x^T) in one launch (dav_cast_transpose_grouped)."""
    if not pairs:
        return
    arr = (_lib.DavTranspose * len(pairs))()
    for q, (x, y) in zip(arr, pairs):
        q.x, q.y_bf16, q.R, q.C = _ptr(x), _ptr(y), int(x.shape[0]), int(x.shape[1])
    _lib.check(_lib.load().dav_cast_transpose_grouped(arr, len(pairs), _stream()), 'dav_cast_transpose_grouped')


# ---- nearest-neighbour probe (csrc/probe/knn.hip) ------------------------------------------------------------------------

KNN_TILE = 128          # queries per workgroup and bank rows per tile of dav_knn_topk_f32 / dav_knn_topk_wide_f32
KNN_NARROW_K = 8        # longest list of dav_knn_topk_f32 (lists in registers); longer ones go to dav_knn_topk_wide_f32
KNN_MAX_K = 64          # longest list of dav_knn_topk_wide_f32 (lists in the workspace), and the most neighbours of a vote


def knn_splits(Nq, N):
    """Bank splits of dav_knn_topk_f32 that give the grid at least 2 x 256 workgroups (the header's suggested count)."""
    qt, nt = -(-Nq // KNN_TILE), -(-N // KNN_TILE)
    return max(1, min(nt, -(-512 // qt)))


def knn_workspace_bytes(Nq, V, k, splits):
    """splits * V * Nq * k * 8: one (score, index) list per split, view and query — the formula of both top-k entry points,
    dav_knn_topk_f32 (k <= 8) and dav_knn_topk_wide_f32 (k <= 64) (include/dav_kernels.h)."""
    return splits * V * Nq * k * 8


def mean_l2n(x, out=None):
    """F.normalize(x.mean(1), p=2, dim=1) of a fp32 [B, L, D] view with unit column stride (dav_mean_l2n_f32)."""
    B, L, D = x.shape
    if x.dtype != F32 or x.stride(2) != 1:
        raise ValueError('mean_l2n needs fp32 [B, L, D] with unit column stride')
    out = torch.empty(B, D, dtype=F32, device=x.device) if out is None else out
    _lib.check(_lib.load().dav_mean_l2n_f32(_ptr(x), B, L, D, x.stride(1), x.stride(0), _ptr(out), _stream()), 'dav_mean_l2n_f32')
    return out


def knn_topk(queries, banks, k, sum_view=True, splits=None, out=None, workspace=None):
    """Top-k bank rows of every query, per modality and (sum_view) for the sum of the modality scores: dav_knn_topk_f32 for
    k <= 8, dav_knn_topk_wide_f32 for 8 < k <= 64 (the same scores and the same order: a longer list starts with the shorter one).
    queries / banks: 1-3 fp32 [Nq, D] / [N, D] tensors with unit column stride (a query tensor may be its bank); the sum view
    is (s_0 + s_1) + s_2.  -> (values [V, Nq, k] fp32, indices [V, Nq, k] int64), V = len(queries) + sum_view."""
    M = len(queries)
    if M != len(banks) or not 1 <= M <= 3:
        raise ValueError('knn_topk takes 1 to 3 (query, bank) pairs')
    Nq, D = queries[0].shape
    N = banks[0].shape[0]
    for t in list(queries) + list(banks):
        if t.dtype != F32 or t.dim() != 2 or t.shape[1] != D or t.stride(1) != 1:
            raise ValueError('knn_topk needs fp32 [rows, D] operands with unit column stride')
    if any(q.shape[0] != Nq or q.stride(0) != queries[0].stride(0) for q in queries) or \
            any(x.shape[0] != N or x.stride(0) != banks[0].stride(0) for x in banks):
        raise ValueError('all query (bank) tensors need the same rows and row stride')
    V = M + int(bool(sum_view))
    S = knn_splits(Nq, N) if splits is None else int(splits)
    dev = queries[0].device
    if out is None:
        out = (torch.empty(V, Nq, k, dtype=F32, device=dev), torch.empty(V, Nq, k, dtype=torch.int32, device=dev))
    nbytes = knn_workspace_bytes(Nq, V, k, S)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    qp = [_ptr(q) for q in queries] + [None] * (3 - M)
    xp = [_ptr(x) for x in banks] + [None] * (3 - M)
    name = 'dav_knn_topk_f32' if k <= KNN_NARROW_K else 'dav_knn_topk_wide_f32'
    _lib.check(getattr(_lib.load(), name)(qp[0], xp[0], qp[1], xp[1], qp[2], xp[2], M, Nq, N, D, queries[0].stride(0),
                                          banks[0].stride(0), int(bool(sum_view)), int(k), S, _ptr(out[0]), _ptr(out[1]),
                                          _ptr(workspace), workspace.numel() * workspace.element_size(), _stream()), name)
    return out[0], out[1].long()


def knn_vote(top_val, top_idx, labels, num_classes, k, inv_t, self_offset=-1, out=None):
    """Weighted vote over top-k lists (dav_knn_vote_f32).  top_val fp32 / top_idx int32 (or int64: converted) [V, Nq, kk] as
    knn_topk returns them; labels: class ids [N] (any integer dtype: converted to int32) or a multi-hot uint8 [N, C]; inv_t: V
    floats, w = exp(score * inv_t[v]) (0 -> plain counts); self_offset >= 0 skips the entry whose index is q + self_offset (0: the
    bank is the query set).  The first k entries that remain vote, so kk >= k, and kk >= k + 1 with an exclusion.
    -> (scores fp32 [V, Nq, C], pred int64 [V, Nq] = argmax with ties to the lower class, or None for multi-hot labels);
    ``out`` = (scores, pred int32 or None) to write into."""
    if top_val.dim() != 3 or top_val.shape != top_idx.shape or top_val.dtype != F32 or not top_val.is_contiguous():
        raise ValueError('knn_vote needs dense fp32 top_val and top_idx of one shape [V, Nq, kk]')
    V, Nq, kk = top_val.shape
    k, C_, self_offset = int(k), int(num_classes), int(self_offset)
    inv_t = [float(x) for x in inv_t]
    if len(inv_t) != V:
        raise ValueError(f'knn_vote needs one inv_t per view: {len(inv_t)} for {V} views')
    if not 1 <= k <= min(KNN_MAX_K, kk - (self_offset >= 0)):
        raise ValueError(f'knn_vote: k = {k} neighbours of kk = {kk} entries' + (' less the excluded one' if self_offset >= 0 else '')
                         + f' (k <= {KNN_MAX_K})')
    if top_idx.dtype != torch.int32 or not top_idx.is_contiguous():
        top_idx = top_idx.to(torch.int32).contiguous()
    multi = labels.dim() == 2
    if multi:
        if labels.dtype != torch.uint8 or labels.shape[1] != C_ or not labels.is_contiguous():
            raise ValueError('knn_vote needs multi-hot labels as dense uint8 [N, num_classes]')
    elif labels.dim() != 1 or labels.dtype.is_floating_point:
        raise ValueError('knn_vote needs class ids [N] or multi-hot uint8 [N, num_classes]')
    elif labels.dtype != torch.int32 or not labels.is_contiguous():
        labels = labels.to(torch.int32).contiguous()
    dev = top_val.device
    if out is None:
        out = (torch.empty(V, Nq, C_, dtype=F32, device=dev), None if multi else torch.empty(V, Nq, dtype=torch.int32, device=dev))
    scores, pred = out
    arr = (C.c_float * V)(*inv_t)
    _lib.check(_lib.load().dav_knn_vote_f32(_ptr(top_val), _ptr(top_idx), V, Nq, kk, k, None if multi else _ptr(labels),
                                            _ptr(labels) if multi else None, int(labels.shape[0]), C_, arr, self_offset,
                                            _ptr(scores), None if multi else _ptr(pred), _stream()), 'dav_knn_vote_f32')
    return scores, (None if multi else pred.long())


# ---- multi-label probe metrics (csrc/probe/ap_auc.hip) -------------------------------------------------------------------

AP_AUC_MAX_ROWS = 32768   # dav_ap_auc_max_rows of include/dav_kernels.h: one workgroup holds a whole column in LDS
AP_AUC_MAX_VIEWS = 4


def ap_auc_workspace_bytes(V, n, C):
    """C * ((n + 31) / 32) * 4: the truth as one bit mask per class — the formula of dav_ap_auc_f64 (include/dav_kernels.h); the
    views share it."""
    return C * ((n + 31) // 32) * 4


def ap_auc(y, scores=None, *, nbr=None, nbr_val=None, nbr_labels=None, out=None, workspace=None):
    """Per-class average precision and ROC AUC of V score views against multi-hot truth, sklearn's definitions with ties grouped
    (dav_ap_auc_f64).  y uint8 [n, C] with unit column stride.  Exactly one form of scores:
      dense      ``scores`` fp32 [V, n, C] (or [n, C]) with unit column stride; rows may be wider than C (a view);
      neighbour  ``nbr`` int32 (or int64: converted) [V, n] (or [n]), ``nbr_val`` fp32 of the same shape, ``nbr_labels`` multi-hot
                 uint8 [N, C]: the score of (row i, class c) is nbr_labels[nbr[v, i], c] * nbr_val[v, i].
    -> (ap fp64 [V, C], auc fp64 [V, C] with NaN where a column has one class only, pos int32 [C]); ``out`` = (ap, auc, pos) dense
    tensors to write into."""
    if y.dim() != 2 or y.dtype != torch.uint8 or y.stride(1) != 1 or (y.shape[0] > 1 and y.stride(0) < y.shape[1]):
        raise ValueError('ap_auc needs the truth as uint8 [n, C] with unit column stride and rows that do not overlap')
    n, C_ = y.shape
    dense = scores is not None
    if dense == (nbr is not None or nbr_val is not None or nbr_labels is not None):
        raise ValueError('ap_auc takes either dense scores or the neighbour form (nbr, nbr_val, nbr_labels), not both or neither')
    if not 1 <= n <= AP_AUC_MAX_ROWS or C_ < 1:
        raise ValueError(f'ap_auc: {n} rows x {C_} classes (1 <= rows <= {AP_AUC_MAX_ROWS}, classes >= 1)')
    dev = y.device
    if dense:
        if scores.dim() == 2:
            scores = scores.unsqueeze(0)
        if scores.dim() != 3 or scores.dtype != F32 or tuple(scores.shape[1:]) != (n, C_) or scores.stride(2) != 1:
            raise ValueError(f'ap_auc needs dense-form scores as fp32 [V, {n}, {C_}] with unit column stride')
        V = scores.shape[0]
        rs = scores.stride(1) if n > 1 else C_
        vs = scores.stride(0) if V > 1 else 0
        if rs < C_ or vs < 0:
            raise ValueError('ap_auc: the rows of a score view must not overlap')
        operands = (scores,)
    else:
        if nbr is None or nbr_val is None or nbr_labels is None:
            raise ValueError('ap_auc: the neighbour form needs nbr, nbr_val and nbr_labels')
        if nbr.dim() == 1:
            nbr, nbr_val = nbr.unsqueeze(0), nbr_val.unsqueeze(0)
        if nbr.dim() != 2 or nbr.shape[1] != n or nbr.dtype.is_floating_point or nbr.dtype == torch.bool:
            raise ValueError(f'ap_auc needs nbr as integer indices [V, {n}]')
        if nbr_val.dtype != F32 or nbr_val.shape != nbr.shape:
            raise ValueError(f'ap_auc needs nbr_val as fp32 {list(nbr.shape)}')
        if nbr_labels.dim() != 2 or nbr_labels.dtype != torch.uint8 or nbr_labels.shape[1] != C_ or nbr_labels.shape[0] < 1:
            raise ValueError(f'ap_auc needs nbr_labels as multi-hot uint8 [N, {C_}]')
        V = nbr.shape[0]
        if nbr.dtype != torch.int32 or not nbr.is_contiguous():
            nbr = nbr.to(torch.int32).contiguous()
        nbr_val, nbr_labels = nbr_val.contiguous(), nbr_labels.contiguous()
        rs = vs = 0
        operands = (nbr, nbr_val, nbr_labels)
    if not 1 <= V <= AP_AUC_MAX_VIEWS:
        raise ValueError(f'ap_auc takes 1 to {AP_AUC_MAX_VIEWS} views, not {V}')
    if any(t.device != dev for t in operands):
        raise ValueError('the truth and the scores live on different devices')
    if out is None:
        out = (torch.empty(V, C_, dtype=torch.float64, device=dev), torch.empty(V, C_, dtype=torch.float64, device=dev),
               torch.empty(C_, dtype=torch.int32, device=dev))
    ap, auc, pos = out
    for t, dt, shape in ((ap, torch.float64, (V, C_)), (auc, torch.float64, (V, C_)), (pos, torch.int32, (C_,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'ap_auc writes dense ap / auc fp64 [{V}, {C_}] and pos int32 [{C_}]')
    nbytes = ap_auc_workspace_bytes(V, n, C_)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError(f'ap_auc needs a workspace of {nbytes} bytes')
    _lib.check(_lib.load().dav_ap_auc_f64(_ptr(y), y.stride(0) if n > 1 else C_, n, C_, V, _ptr(scores) if dense else None, rs, vs,
                                          None if dense else _ptr(nbr), None if dense else _ptr(nbr_val),
                                          None if dense else _ptr(nbr_labels), 0 if dense else int(nbr_labels.shape[0]),
                                          _ptr(ap), _ptr(auc), _ptr(pos), _ptr(workspace),
                                          workspace.numel() * workspace.element_size(), _stream()), 'dav_ap_auc_f64')
    return ap, auc, pos


# ---- frame transform of the input stage (csrc/data/frames.hip) -----------------------------------------------------------

FRAME_PARAM_COLS = 9    # i, j, h, w, RH, RW, top, left, flip (include/dav_kernels.h)


def frame_transform(frames, params, size, mean, std, out=None):
    """Crop + antialiased bilinear resample + flip + /255 + (x - mean) / std of a batch of frames in one launch
    (dav_frame_transform_u8).  frames uint8 [B, H, W, 3] dense on the device, params int32 [B, 9] on the device (rows as in
    include/dav_kernels.h; the kernel clamps them, callers validate them on the host before upload: util/frame_transforms.py),
    mean / std three floats each -> fp32 [B, 3, size, size]."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError('frame_transform needs dense uint8 frames [B, H, W, 3]')
    B, H, W, _ = frames.shape
    if params.dtype != torch.int32 or tuple(params.shape) != (B, FRAME_PARAM_COLS) or not params.is_contiguous():
        raise ValueError(f'frame_transform needs dense int32 params [{B}, {FRAME_PARAM_COLS}]')
    if params.device != frames.device:
        raise ValueError('frames and params live on different devices')
    size = int(size)
    if out is None:
        out = torch.empty(B, 3, size, size, dtype=F32, device=frames.device)
    elif out.dtype != F32 or tuple(out.shape) != (B, 3, size, size) or not out.is_contiguous():
        raise ValueError(f'frame_transform writes dense fp32 [{B}, 3, {size}, {size}]')
    m, s = [float(v) for v in mean], [float(v) for v in std]
    _lib.check(_lib.load().dav_frame_transform_u8(_ptr(frames), B, H, W, _ptr(params), size, m[0], m[1], m[2], s[0], s[1], s[2],
                                                  _ptr(out), _stream()), 'dav_frame_transform_u8')
    return out


RESAMPLE_MAX_RATIO = 1024   # dav_resample_max_ratio of include/dav_kernels.h: the reduced rates o, n of dav_wave_resample


def wave_resample_tile(o, n, width):
    """Frames (of ``o`` input samples) one workgroup of dav_wave_resample owns at this geometry: where its tiles meet."""
    t = _lib.load().dav_wave_resample_tile(int(o), int(n), int(width))
    _lib.check(min(t, 0), 'dav_wave_resample_tile')
    return t


def wave_resample(wave, taps_kn, o, n, width, out_len=None, gain=None, clamp=False, out=None):
    """Windowed-sinc polyphase resampling of a batch of waveforms with Pad's mirror, a per-row gain and the clamp to [-1, 1] in
    the epilogue, one launch (dav_wave_resample).  wave fp32 or int16 [B, L] on the device, unit stride along L (rows may be
    strided); taps_kn fp32 [2 width + o, n] dense, the table k-major; gain fp32 [B] or None -> fp32 [B, out_len]
    (default out_len: R = ceil(n L / o)); ``out``: an fp32 [B, out_len] view with unit stride along its rows."""
    if wave.dtype not in (F32, torch.int16) or wave.dim() != 2 or wave.stride(1) != 1:
        raise ValueError('wave_resample needs fp32 or int16 waveforms [B, L] with unit stride along L')
    B, L = wave.shape
    o, n, width = int(o), int(n), int(width)
    if taps_kn.dtype != F32 or tuple(taps_kn.shape) != (2 * width + o, n) or not taps_kn.is_contiguous():
        raise ValueError(f'wave_resample needs a dense fp32 tap table [{2 * width + o}, {n}] (k-major)')
    if taps_kn.device != wave.device or (gain is not None and gain.device != wave.device):
        raise ValueError('waveforms, taps and gains live on different devices')
    if gain is not None and (gain.dtype != F32 or tuple(gain.shape) != (B,) or not gain.is_contiguous()):
        raise ValueError(f'wave_resample needs dense fp32 gains [{B}]')
    out_len = -(-n * L // o) if out_len is None else int(out_len)
    if out is None:
        out = torch.empty(B, out_len, dtype=F32, device=wave.device)
    elif out.dtype != F32 or tuple(out.shape) != (B, out_len) or out.stride(1) != 1:
        raise ValueError(f'wave_resample writes fp32 [{B}, {out_len}] with unit stride along its rows')
    _lib.check(_lib.load().dav_wave_resample(_ptr(wave), int(wave.dtype == torch.int16), B, L, wave.stride(0) if B > 1 else L,
                                             _ptr(taps_kn), o, n, width, _ptr(gain), int(bool(clamp)), _ptr(out), out_len,
                                             out.stride(0) if B > 1 else out_len, _stream()), 'dav_wave_resample')
    return out


# ---- source-separation audio (csrc/sep/stft.hip) ----------------------------------------------------------------------------

STFT_FRAMES = 8      # dav_stft_frames of include/dav_kernels.h: frames one workgroup of dav_stft_c32 owns
ISTFT_FRAMES = 12    # dav_istft_frames: frames one workgroup of dav_istft_c32 / dav_sep_mask_istft holds, halo included


def istft_tile(n_fft, hop):
    """Output samples one workgroup of the inverse owns: hop * (ISTFT_FRAMES - 2 h - 1), h = (n_fft / 2 - 1) / hop frames of
    halo on each side (the formula of include/dav_kernels.h): outputs j and j + 1 with (j + 1) % tile == 0 come from different
    workgroups.  0 for a geometry the kernels refuse."""
    n_fft, hop = int(n_fft), int(hop)
    if n_fft < 2 or n_fft % 2 or hop < 1:
        return 0
    return hop * max(ISTFT_FRAMES - 2 * ((n_fft // 2 - 1) // hop) - 1, 0)


def _sep_tables(n_fft, dev, *tables):
    for t in tables:
        if t.dtype != F32 or tuple(t.shape) != (n_fft,) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'the window and the cos / sin tables are dense fp32 [{n_fft}] on the operands\' device')


def _sep_waves(wave, what):
    if not wave.is_cuda:
        raise RuntimeError(f'{what} runs on an MI355X (cuda) device; there is no CPU fallback')
    if wave.dtype != F32 or wave.dim() != 2 or wave.stride(1) != 1:
        raise ValueError(f'{what} needs fp32 waveforms [B, S] with unit stride along S')
    return wave.shape


def stft(wave, window, cos_tab, sin_tab, n_fft, hop, out=None):
    """torch.stft(center=True, pad_mode='reflect', onesided=True, normalized=False, return_complex=True) with the caller's window
    of n_fft samples (dav_stft_c32).  wave fp32 [B, S] on the device, unit stride along S (rows may be strided) -> complex64
    [B, n_fft / 2 + 1, S / hop + 1].  ``out``: the fp32 view [B * n_freqs, 2 * frames] of such a result (re / im interleaved) with
    unit column stride and an even row stride; it is returned in place of the complex tensor."""
    B, S = _sep_waves(wave, 'stft')
    n_fft, hop = int(n_fft), int(hop)
    _sep_tables(n_fft, wave.device, window, cos_tab, sin_tab)
    n_freqs, frames = n_fft // 2 + 1, S // max(hop, 1) + 1
    if out is None:
        ret = torch.empty(B, n_freqs, frames, dtype=torch.complex64, device=wave.device)
        fl = torch.view_as_real(ret).view(B * n_freqs, 2 * frames)
    else:
        ret = fl = out
        if fl.dtype != F32 or tuple(fl.shape) != (B * n_freqs, 2 * frames) or fl.stride(1) != 1 or fl.stride(0) % 2 or fl.device != wave.device:
            raise ValueError(f'stft writes the fp32 view [{B * n_freqs}, {2 * frames}] of a complex64 result, rows an even stride apart')
    _lib.check(_lib.load().dav_stft_c32(_ptr(wave), B, S, wave.stride(0) if B > 1 else S, n_fft, hop, _ptr(window), _ptr(cos_tab),
                                        _ptr(sin_tab), _ptr(fl), fl.stride(0) // 2, _stream()), 'dav_stft_c32')
    return ret


def istft(spec, window, cos_tab, sin_tab, n_fft, hop, out=None):
    """torch.istft(center=True, normalized=False, onesided=True, length=None) with the caller's window (dav_istft_c32).  spec
    complex64 [B, n_fft / 2 + 1, frames] on the device with unit stride along the frames (bin rows may be strided, batch elements
    lie n_freqs rows apart) -> fp32 [B, hop * (frames - 1)]; ``out``: such a view with unit stride along its rows."""
    if not spec.is_cuda:
        raise RuntimeError('istft runs on an MI355X (cuda) device; there is no CPU fallback')
    n_fft, hop = int(n_fft), int(hop)
    n_freqs = n_fft // 2 + 1
    if spec.dtype != torch.complex64 or spec.dim() != 3 or spec.shape[1] != n_freqs:
        raise ValueError(f'istft needs a complex64 spectrum [B, {n_freqs}, frames]')
    B, _, frames = spec.shape
    rs = spec.stride(1) if n_freqs > 1 else frames
    if spec.stride(2) != 1 or rs < frames or (B > 1 and spec.stride(0) != n_freqs * rs):
        raise ValueError('istft needs unit stride along the frames and batch elements n_freqs bin rows apart')
    _sep_tables(n_fft, spec.device, window, cos_tab, sin_tab)
    L = hop * (frames - 1)
    if out is None:
        out = torch.empty(B, max(L, 0), dtype=F32, device=spec.device)
    elif out.dtype != F32 or tuple(out.shape) != (B, L) or out.stride(1) != 1 or out.device != spec.device:
        raise ValueError(f'istft writes fp32 [{B}, {L}] with unit stride along its rows')
    _lib.check(_lib.load().dav_istft_c32(_ptr(torch.view_as_real(spec)), rs, B, frames, n_fft, hop, _ptr(window), _ptr(cos_tab),
                                         _ptr(sin_tab), _ptr(out), out.stride(0) if B > 1 else L, _stream()), 'dav_istft_c32')
    return out


def sep_mask_istft(wave, logits, window, cos_tab, sin_tab, fbank, band_lo, band_hi, n_fft, hop, out=None):
    """The reference's SpectrogramMasking (eval_avsrcsep.py:272-277) for K masks per mixture in one launch (dav_sep_mask_istft):
    istft(einsum('bmt,fm->bft', cat(sigmoid(logits), 0), fbank) * stft(wave)).  wave fp32 [B, S] with unit stride along S, logits
    fp32 [B, K, n_mels, T] dense with T + 1 == S / hop + 1, fbank fp32 [n_freqs, n_mels] dense with band_lo / band_hi int32
    [n_mels] (MelSpectrogram's buffers) -> fp32 [B, K, hop * T]; ``out``: an fp32 view [B * K, hop * T] with unit stride along its
    rows (returned as it is)."""
    B, S = _sep_waves(wave, 'sep_mask_istft')
    n_fft, hop = int(n_fft), int(hop)
    n_freqs = n_fft // 2 + 1
    dev = wave.device
    if logits.dtype != F32 or logits.dim() != 4 or logits.shape[0] != B or not logits.is_contiguous() or logits.device != dev:
        raise ValueError(f'sep_mask_istft needs dense fp32 mask logits [{B}, K, n_mels, T] on the waveforms\' device')
    _, K, n_mels, T = logits.shape
    if T + 1 != S // max(hop, 1) + 1:
        raise ValueError(f'sep_mask_istft: {T} mask frames for {S // max(hop, 1) + 1} STFT frames (the last frame\'s mask is the appended zero column: T + 1 == frames)')
    _sep_tables(n_fft, dev, window, cos_tab, sin_tab)
    if fbank.dtype != F32 or tuple(fbank.shape) != (n_freqs, n_mels) or not fbank.is_contiguous() or fbank.device != dev:
        raise ValueError(f'sep_mask_istft needs the dense fp32 filterbank [{n_freqs}, {n_mels}]')
    for t in (band_lo, band_hi):
        if t.dtype != torch.int32 or tuple(t.shape) != (n_mels,) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'sep_mask_istft needs dense int32 band_lo / band_hi [{n_mels}]')
    L = hop * T
    if out is None:
        ret = torch.empty(B, K, L, dtype=F32, device=dev)
        rows = ret.view(B * K, L)
    else:
        ret = rows = out
        if rows.dtype != F32 or tuple(rows.shape) != (B * K, L) or rows.stride(1) != 1 or rows.device != dev:
            raise ValueError(f'sep_mask_istft writes fp32 [{B * K}, {L}] with unit stride along its rows')
    _lib.check(_lib.load().dav_sep_mask_istft(_ptr(wave), B, S, wave.stride(0) if B > 1 else S, _ptr(logits), K, n_mels, T, n_fft, hop,
                                              _ptr(window), _ptr(cos_tab), _ptr(sin_tab), _ptr(fbank), _ptr(band_lo), _ptr(band_hi),
                                              _ptr(rows), rows.stride(0) if B * K > 1 else L, _stream()), 'dav_sep_mask_istft')
    return ret
