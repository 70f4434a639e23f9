"""Elementwise checks of kernel outputs (used by tests/gpu_selfcheck.py and tests/gpu_fuzz.py; device-agnostic, its own tests
run on the CPU: tests/test_kcheck.py).

A relative-L2 figure over a whole tensor hides a localized error: one wrong row among thousands, one tile off by 10 %, one
tile never written whose memory still holds an earlier correct answer.  So every output is judged three ways:

* it starts POISONED (NaN / an integer sentinel) when the contract says the kernel writes it, or PREFILLED with random values
  when the contract says it accumulates — an element the kernel skips cannot pass;
* every element must satisfy |got - ref| <= bound, the bound propagated from the magnitudes of the operands in float64 through
  the same formula (``within`` and the ``*_bound`` helpers below) — no fixed per-shape tolerance;
* the output sits in a GUARDED buffer: guard bands in front and behind and the padding of its row stride hold a fixed byte
  pattern that must come back bit-identical (``Guarded``) — a store past N, past the last row or into a neighbour shows.
"""
import math

import torch

GUARD_BYTES = 256                 # each guard band (a multiple of 16: the view keeps the 16-byte alignment of the allocation)
GUARD_BYTE = 0xA5                 # fill pattern of every byte outside the view (fp32 0xA5A5A5A5 / bf16 0xA5A5: finite, never a result)
INT_POISON = -0x5A5A5A5B          # sentinel of int outputs
U32 = 2.0 ** -24                  # unit roundoff of fp32
FLT_MIN = 2.0 ** -126             # smallest normal fp32: the kernels flush what falls below it to 0
U16 = 2.0 ** -8                   # unit roundoff of bf16 (8 significant bits): EXACTLY the worst case of one rounding, no slack —
                                  # the bf16-output bounds hold because the accumulation term adds to it; never lower this

# one constant per family, fixed here (never per shape); see the *_bound helpers for what each multiplies
C_GEMM = 1.0                      # fp32 accumulation over K: the classical K * u * |A||B|^T
C_ATTN = 4.0                      # P (and dS) rounded to bf16 before their products, plus the exp / max-shift of the softmax
GELU_ABS = 5e-7                   # erf approximation of the GELU epilogue (|err| <= 1.5e-7, gpu_selfcheck.gemm_nt) + its fp32 evaluation

RATIOS = {}                       # family -> worst err / bound seen (printed per family on the device)


def poisoned(shape, dtype, device='cpu'):
    """An output the kernel is contracted to WRITE: NaN (floating) or INT_POISON everywhere."""
    if dtype.is_floating_point:
        return torch.full(shape, float('nan'), dtype=dtype, device=device)
    return torch.full(shape, INT_POISON, dtype=dtype, device=device)


def prefilled(shape, dtype=torch.float32, device='cpu', seed=0):
    """An output the kernel is contracted to ACCUMULATE into: random values (the check is then out == prefill + result)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g).to(device=device, dtype=dtype)


class Guarded:
    """A [rows, cols] output as a view with row stride ``ld`` inside a larger buffer: GUARD_BYTES of pattern in front, the padding
    columns of every row and GUARD_BYTES behind.  ``fill``: 'poison' (written outputs), 'zero', a number, or a tensor to copy in
    (accumulated outputs)."""

    def __init__(self, rows, cols, dtype, ld=None, device='cpu', fill='poison'):
        ld = cols if ld is None else ld
        assert ld >= cols
        es = torch.tensor([], dtype=dtype).element_size()
        assert GUARD_BYTES % es == 0
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.lead = GUARD_BYTES // es
        n = self.lead + rows * ld + self.lead
        self.flat = torch.empty(n, dtype=dtype, device=device)
        self.flat.view(torch.uint8).fill_(GUARD_BYTE)
        self.t = self.flat[self.lead:self.lead + rows * ld].view(rows, ld)[:, :cols]
        self.set(fill)
        inside = torch.zeros(n, dtype=torch.bool, device=device)
        inside[self.lead:self.lead + rows * ld].view(rows, ld)[:, :cols] = True
        self._outside = ~inside

    def set(self, fill):
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.reshape(self.rows, self.cols))
        elif fill == 'poison':
            self.t.copy_(poisoned((self.rows, self.cols), self.dtype, self.t.device))
        elif fill == 'zero':
            self.t.zero_()
        else:
            self.t.fill_(fill)
        return self

    def ptr(self):
        return self.t.data_ptr()

    def stray(self):
        """(number of elements outside the view whose bytes changed, description of the first one or '')"""
        b = self.flat.view(torch.uint8).view(self.flat.numel(), -1)
        changed = (b != GUARD_BYTE).any(1) & self._outside
        n = int(changed.sum())
        if not n:
            return 0, ''
        i = int(changed.nonzero()[0, 0])
        if i < self.lead:
            where = f'leading guard, {self.lead - i} elements in front of the view'
        elif i >= self.lead + self.rows * self.ld:
            where = f'trailing guard, element {i - self.lead - self.rows * self.ld} behind the view'
        else:
            r, c = divmod(i - self.lead, self.ld)
            where = f'row {r} padding column {c} (cols {self.cols}, ld {self.ld})'
        return n, where


def changed(t, before, mask=None):
    """Elements of ``t`` whose BITS differ from the snapshot ``before`` (only where ``mask``: a bool over the leading dims, e.g.
    the rows a row map skips, the context rows of a fused buffer).  Returns (count, flat index of the first one or -1)."""
    es = t.element_size()
    a = t.contiguous().view(torch.uint8).view(-1, es)
    b = before.contiguous().view(torch.uint8).view(-1, es)
    diff = (a != b).any(1).view(t.shape)
    if mask is not None:
        diff = diff & mask.view(tuple(mask.shape) + (1,) * (t.dim() - mask.dim())).expand_as(diff)
    n = int(diff.sum())
    return n, (int(diff.flatten().nonzero()[0, 0]) if n else -1)


def tile_of(idx, shape):
    """'[r, c] tile128 (r//128, c//128) tile256 (...)' of a flat index into ``shape`` (the last two dims are the matrix)."""
    pos = []
    for s in reversed(shape):
        pos.append(idx % s)
        idx //= s
    pos = pos[::-1]
    if len(pos) >= 2:
        r, c = pos[-2], pos[-1]
        return f'{pos} tile128 ({r // 128}, {c // 128}) tile256 ({r // 256}, {c // 256})'
    return f'{pos}'


def within(got, ref, bound, tag=''):
    """Elementwise |got - ref| <= bound in float64; a non-finite ``got`` always fails.  Returns (ok, worst err / bound, message);
    the message names the worst element and its 128- and 256-tile."""
    g = got.detach().double()
    r = ref.detach().double().expand_as(g)
    b = torch.as_tensor(bound, dtype=torch.float64, device=g.device).expand_as(g)
    err = (g - r).abs()
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float('inf')))
    if ratio.numel() == 0:
        return True, 0.0, ''
    worst = float(ratio.max())
    ok = worst <= 1.0
    if ok:
        return True, worst, ''
    i = int(ratio.flatten().argmax())
    nbad = int((ratio > 1.0).sum())
    msg = (f'{tag}: {nbad} of {g.numel()} elements outside the bound; worst at {tile_of(i, tuple(g.shape))}: '
           f'got {float(g.flatten()[i]):.6g} ref {float(r.flatten()[i]):.6g} bound {float(b.flatten()[i]):.3g}')
    return False, worst, msg


def exact(got, ref, tag=''):
    """Bit-for-bit equality of ``got`` with ``ref`` (same dtype and shape: a copy, a single rounding of the same fp32 value, +0
    where +0 is due — a NaN poison or a -0 counts as a difference).  Returns (number of elements that differ, message naming the
    first one and its 128- and 256-tile, '' when none)."""
    n, i = changed(got, ref)
    if not n:
        return 0, ''
    return n, (f'{tag}: {n} of {got.numel()} elements differ; first at {tile_of(i, tuple(got.shape))}: '
               f'got {float(got.flatten()[i]):.6g} ref {float(ref.flatten()[i]):.6g}')


def note(family, ratio):
    if math.isfinite(ratio):
        RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)


# ---- bounds ---------------------------------------------------------------------------------------------------------------

def out_round(dtype):
    """relative rounding allowance of the stored value: bf16 2^-8, fp32 2^-22 (a few roundings of the epilogue's adds)"""
    return U16 if dtype == torch.bfloat16 else 4 * U32


def gemm_scale(A, B):
    """|A| |B|^T in float64 for A [M, K], B [N, K]"""
    return A.detach().double().abs() @ B.detach().double().abs().t()


def gemm_bound(A, B, ref, out_dtype, alpha=1.0, c=C_GEMM):
    """C = alpha * A . B^T (+ epilogue terms that enter through |ref|): c * 2^-24 * K * |alpha| |A||B|^T + r_out |ref|"""
    K = A.shape[-1]
    return c * U32 * K * abs(alpha) * gemm_scale(A, B) + out_round(out_dtype) * ref.detach().double().abs()


def gelu_bound(pre_bound, ref, out_dtype):
    """GELU epilogue: |gelu'| <= 1.13 carries the pre-activation bound; + 1e-6 |ref| + the erf approximation"""
    return 1.13 * pre_bound + (1e-6 + out_round(out_dtype)) * ref.detach().double().abs() + GELU_ABS


def dgelu_bound(pre_bound, ref, out_dtype):
    """GELU' twin: |gelu''| <= 0.8 carries the pre-activation bound"""
    return 0.8 * pre_bound + (1e-6 + out_round(out_dtype)) * ref.detach().double().abs() + GELU_ABS


def softmax64(q, k, scale, bias=None):
    """float64 P = softmax(scale q k^T (+ bias)) of [.., N, d] operands, and the float64 logits"""
    s = (q.detach().double() @ k.detach().double().transpose(-2, -1)) * scale
    if bias is not None:
        s = s + bias.double()
    return s.softmax(-1), s


def attn_bounds(q, k, v, dO, O, scale, keep=None, up=U16, r_out=U16, c=C_ATTN, bias=None):
    """Float64 references and elementwise bounds of attention forward and backward ([B, H, N, d] operands, keep: the keep mask
    already divided by the keep probability, or None).  P is rounded to bf16 (relative ``up``) before P.V, dS before dS.K / dS^T.Q:
      O   : c up (P~|V|) + r_out |O|                      (P~ = P * keep)
      dV  : c up (P~^T |dO|) + r_out |dV|
      dQ  : scale c up (P o (keep |dO||V|^T + Dabs)) |K| + r_out |dQ|,  dK likewise with |Q|
    where Dabs = sum |dO| |O| bounds the row term Delta = sum dO O (the kernel forms it from its own rounded O).
      dS  : c up S + 4 u |dS| + 2^-126 (|dO||V|^T + Dabs) — a P below the smallest normal fp32 (a logit masked by -100) may be
            flushed to 0, an absolute error of at most 2^-126 in P times |dP - Delta|."""
    P, s = softmax64(q, k, scale, bias)
    q64, k64, v64 = (t.detach().double() for t in (q, k, v))
    Pk = P if keep is None else P * keep.double()
    O64 = Pk @ v64
    lse = torch.logsumexp(s, -1)
    b_O = c * up * (Pk @ v64.abs()) + r_out * O64.abs()
    b_lse = 1e-5 * (1.0 + lse.abs() + s.abs().amax(-1))
    out = dict(P=P, O=O64, lse=lse, bO=b_O, blse=b_lse)
    if dO is None:
        return out
    d64 = dO.detach().double()
    dP = d64 @ v64.transpose(-2, -1)
    if keep is not None:
        dP = dP * keep.double()
    Delta = (d64 * O64).sum(-1, keepdim=True)
    dS = P * (dP - Delta)
    dq = scale * dS @ k64
    dk = scale * dS.transpose(-2, -1) @ q64
    dv = Pk.transpose(-2, -1) @ d64
    Dabs = (d64.abs() * O.detach().double().abs()).sum(-1, keepdim=True) + (d64.abs() * O64.abs()).sum(-1, keepdim=True)
    mag = d64.abs() @ v64.abs().transpose(-2, -1)
    if keep is not None:
        mag = mag * keep.double()
    S = P * (mag + Dabs)
    out.update(dq=dq, dk=dk, dv=dv,
               bdq=scale * c * up * (S @ k64.abs()) + r_out * dq.abs(),
               bdk=scale * c * up * (S.transpose(-2, -1) @ q64.abs()) + r_out * dk.abs(),
               bdv=c * up * (Pk.transpose(-2, -1) @ d64.abs()) + r_out * dv.abs(),
               dS=dS, bdS=c * up * S + 4 * U32 * dS.abs() + FLT_MIN * (mag + Dabs))
    return out


def sum_bound(abs_sum, n, ref, out_dtype=torch.float32):
    """An fp32 sum of n terms in ANY order (sequential, per-lane partials + shuffles, atomics): |fl(sum) - sum| <= (n - 1) u sum|t_i|
    + O(u^2), taken as n u sum|t_i|; plus the rounding of the stored value, r_out |ref|.  A prefill the kernel adds to, and a
    scale applied to the sum, count as one term each.  ``abs_sum`` = sum|t_i| (float64), n a number or a tensor per element."""
    return n * U32 * torch.as_tensor(abs_sum).double() + out_round(out_dtype) * ref.detach().double().abs()


def f32_attn_up(q, k, scale, bias=None, dv=None):
    """Relative error allowance of P (and of what rides on it) in the fp32 attention kernels (up of ``attn_bounds``; r_out
    out_round(fp32)).  A logit s = scale q.k (+ bias) is a d-term fp32 dot product: |ds| <= d u scale (|q||k|^T) + u |s|; P = exp(s -
    lse) takes |ds| + |dlse| <= 2 max|ds| as a relative error, the exp a few u; the sums over the Nk keys (l, P.V, dP) and over the dv
    value columns (dP, Delta) add Nk u and dv u.  So up = u (2 d scale max(|q||k|^T) + 2 max|s| + Nk + dv + 8) — max over all rows."""
    q64, k64 = q.detach().double(), k.detach().double()
    d, Nk = q64.shape[-1], k64.shape[-2]
    s = (q64 @ k64.transpose(-2, -1)) * scale
    if bias is not None:
        s = s + bias.double()
    mag = float((q64.abs() @ k64.abs().transpose(-2, -1)).max())
    return U32 * (2 * d * scale * mag + 2 * float(s.abs().max()) + Nk + (d if dv is None else dv) + 8)


def patchify64(img):
    """[B, C, H, W] -> float64 [B, L, 256 C] 16 x 16 patches, channel fastest (the loss kernels' and the oracle's order)"""
    B, C, H, W = img.shape
    x = img.detach().double().reshape(B, C, H // 16, 16, W // 16, 16)
    return x.permute(0, 2, 4, 3, 5, 1).reshape(B, (H // 16) * (W // 16), 256 * C)


def mse_bounds(img, pred, mask, norm):
    """Float64 AVMAE.patchify + forward_loss (per-patch mean, unbiased variance, eps 1e-6 inside the sqrt) and elementwise bounds
    of what dav_patch_mse_fwd writes, from the magnitudes of one patch's P = 256 C target values t and predictions:
      tmean  : e_m = u (P mean|t| + |m|)                                          (P-term sum, one division)
      var    : Σ(t - m~)^2 = Σ(t - m)^2 + P (m - m~)^2 exactly, so e_q = (P + 3) u (q + P e_m^2) + P e_m^2   (q = Σ(t - m)^2)
      trstd  : r = (q / (P - 1) + 1e-6)^-1/2, dr/dq = -r^3 / (2 (P - 1)): e_r = r^3 e_q / (2 (P - 1)) + 4 u r
      x = pred - (t - m) r: e_x = |t - m| e_r + r e_m + 3 u (|pred| + |t - m| r)
      loss_patch = mean x^2: (2 Σ|x| e_x + Σ e_x^2) / P + (P + 2) u mean x^2
      loss = Σ(loss_patch mask) / Σ mask: (Σ e_lp mask + (n + 2) u Σ|loss_patch mask|) / Σ mask   (n = B L);  mask_sum exact.
    Without norm m = 0 and r = 1 exactly.  pred [B, L, P], mask [B, L]."""
    t = patchify64(img)
    p64, m64 = pred.detach().double().reshape(t.shape), mask.detach().double().reshape(t.shape[:2])
    P = t.shape[-1]
    if norm:
        m = t.mean(-1, keepdim=True)
        q = ((t - m) ** 2).sum(-1, keepdim=True)
        r = (q / (P - 1) + 1e-6).rsqrt()
        e_m = U32 * (P * t.abs().mean(-1, keepdim=True) + m.abs())
        e_q = (P + 3) * U32 * (q + P * e_m ** 2) + P * e_m ** 2
        e_r = r ** 3 * e_q / (2 * (P - 1)) + 4 * U32 * r
    else:
        m, r = torch.zeros_like(t[..., :1]), torch.ones_like(t[..., :1])
        e_m, e_r = torch.zeros_like(m), torch.zeros_like(r)
    c = t - m
    x = p64 - c * r
    e_x = c.abs() * e_r + r * e_m + 3 * U32 * (p64.abs() + c.abs() * r)
    lp = (x ** 2).mean(-1)
    b_lp = (2 * (x.abs() * e_x).sum(-1) + (e_x ** 2).sum(-1)) / P + (P + 2) * U32 * lp
    ms = m64.sum()
    loss = (lp * m64).sum() / ms
    b_loss = ((b_lp * m64).sum() + (lp.numel() + 2) * U32 * (lp * m64).abs().sum()) / ms
    return dict(loss_patch=lp, tmean=m.squeeze(-1), trstd=r.squeeze(-1), bloss_patch=b_lp, btmean=e_m.squeeze(-1),
                btrstd=e_r.squeeze(-1), loss=loss, bloss=b_loss, mask_sum=ms)


def mse_grad(img, pred, mask, tmean, trstd, mask_sum, gout, out_dtype):
    """Float64 reference and bound of dav_patch_mse_bwd(_f32) from the kernel's own statistics (tmean / trstd / mask_sum of the
    forward): d pred = mask gout 2 / (P mask_sum) (pred - (t - tmean) trstd).  Eight fp32 roundings along the way (three for the
    coefficient, t - m, x r, pred - .., two products), relative to |pred| + |t - m| r:  8 u |coef mask| (|pred| + |t - m| r) +
    r_out |ref|.  Rows with mask 0 must come out exactly 0 (their bound is 0)."""
    t = patchify64(img)
    p64 = pred.detach().double().reshape(t.shape)
    m64 = mask.detach().double().reshape(t.shape[:2] + (1,))
    tm, tr = tmean.detach().double().reshape(m64.shape), trstd.detach().double().reshape(m64.shape)
    coef = m64 * float(gout) * 2 / (t.shape[-1] * float(mask_sum))
    c = (t - tm).abs() * tr
    ref = coef * (p64 - (t - tm) * tr)
    return ref, 8 * U32 * coef.abs() * (p64.abs() + c) + out_round(out_dtype) * ref.abs()


def gang(probs):
    """dav_gemm_tn_gang_bf16 (through ops.gemm_tn_gang) with its workspace filled with 0xFF bytes: the header only says caller-owned,
    so the kernel must initialise its tickets itself on every call"""
    from deepavfusion_amd import ops
    ops.gemm_tn_gang(probs, workspace_fill=0xFF)
    torch.cuda.synchronize()


C_LN = 64.0                       # LayerNorm: fp32 mean / variance / rstd over D <= a few thousand columns, then per-element products


def ln_bounds(x, gamma, beta, eps, dy=None):
    """Float64 LayerNorm over the last dim (rows [.., D]) and elementwise bounds from the magnitudes:
      y      : C_LN u (|gamma| (|xhat| + rstd mean|x|) + |beta|)                       (xhat = (x - mean) rstd)
      dx     : C_LN u rstd (|g| + mean|g| + |xhat| mean|g xhat|) (1 + |xhat|)           (g = dy gamma)
      dgamma : u (rows sum|dy xhat| + C_LN sum |dy| (1 + |xhat|) (1 + rstd mean|x|)),  dbeta: u rows sum|dy|"""
    x64 = x.detach().double()
    D = x64.shape[-1]
    mean = x64.mean(-1, keepdim=True)
    rstd = (((x64 - mean) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (x64 - mean) * rstd
    g64, b64 = gamma.detach().double(), beta.detach().double()
    stat = 1 + rstd * x64.abs().mean(-1, keepdim=True)
    out = dict(y=xh * g64 + b64, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1),
               by=C_LN * U32 * (g64.abs() * (xh.abs() + stat) + b64.abs()))
    if dy is None:
        return out
    d64 = dy.detach().double()
    gd = d64 * g64
    dx = rstd * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    mag = rstd * (gd.abs() + gd.abs().mean(-1, keepdim=True) + xh.abs() * (gd * xh).abs().mean(-1, keepdim=True))
    d2, x2 = d64.reshape(-1, D), xh.reshape(-1, D)
    rows = d2.shape[0]
    out.update(dx=dx, bdx=C_LN * U32 * mag * (1 + xh.abs()) * stat,
               dgamma=(d2 * x2).sum(0), dbeta=d2.sum(0),
               bdgamma=U32 * (rows * (d2 * x2).abs().sum(0) + C_LN * (d2.abs() * (1 + x2.abs()) * stat.reshape(-1, 1)).sum(0)),
               bdbeta=U32 * rows * d2.abs().sum(0))
    return out


# ---- flat-buffer optimizer pass (dav_adamw_flat, dav_l2norm) and the DropPath row kernels -----------------------------------------
# Worst err / bound seen on an MI355X (tests/gpu_selfcheck.py optimizer / misc_kernels; the constants below come from the counts
# in the docstrings, none was fitted to these figures):
#   adamw_ref p 0.35, m 0.49, v 0.39 (0.9 M elements, 70 segments) and p 0.36, m 0.48, v 0.54 (67 M elements, 309 segments, two trips)
#   adamw_sumsq_bound 0.03 .. 0.045 (219 workgroups; the atomic adds land in a different order every run) and 0.0012 (16384 workgroups)
#   l2norm_bound 0.097   rows_axpy_bound 0.48   step_guard (4 u) 0.12

ADAMW_CHUNK = 4096                # elements one workgroup of dav_adamw_flat handles per trip: 256 lanes x 4 float4 of 4
ADAMW_GRID_CAP = 16384            # its grid is capped here; longer buffers take further trips of the grid-stride loop
L2NORM_GRID_CAP = 1024            # dav_l2norm: partial sums of at most this many workgroups of 256 lanes, one float4 per lane and trip


def f32(x):
    """the value a C ``float`` argument takes: x rounded to fp32, as a Python float (so float64 arithmetic widens it exactly)"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def seg_table(sizes, decayed, base_lr=1e-2, wd=0.05, align=64):
    """The flat layout util/flat.py gives a list of parameters: each of ``sizes`` rounded up to ``align`` elements, laid out back to
    back, one segment per parameter.  Segment i gets lr = base_lr * 0.75^(i mod 7) (a layer-wise scale: neighbours always differ)
    and weight decay ``wd`` where ``decayed[i]`` else 0 (the 1-D parameters).  Returns (seg_end list, hyper list [lr0, wd0, lr1, ..],
    real bool mask over the n elements as a CPU tensor: False on the padding behind a size that is no multiple of ``align``)."""
    ends, hyper, off = [], [], 0
    for i, (sz, dec) in enumerate(zip(sizes, decayed)):
        assert sz > 0
        off += (sz + align - 1) // align * align
        ends.append(off)
        hyper += [base_lr * 0.75 ** (i % 7), wd if dec else 0.0]
    real = torch.zeros(off, dtype=torch.bool)
    start = 0
    for sz, e in zip(sizes, ends):
        real[start:start + sz] = True
        start = e
    return ends, hyper, real


def seg_expand(seg_end, per_seg, n, start=0):
    """per-element value of a per-segment table for the elements start .. start + n - 1: element i belongs to the first segment
    whose seg_end is > i (searchsorted; NOT the kernel's own binary search + walk)"""
    i = torch.arange(start, start + n, device=seg_end.device, dtype=torch.int64)
    s = torch.searchsorted(seg_end.to(torch.int64).contiguous(), i, right=True).clamp_max(seg_end.numel() - 1)
    return per_seg[s]


def adamw_ref(p, g, m, v, seg_end, hyper, beta1, beta2, eps, bias_corr, grad_scale, start=0):
    """ONE float64 AdamW step of dav_adamw_flat from the fp32 state given (``start``: index of p[0] in the flat buffer, for a slice
    of a long one).  Every scalar the kernel receives as a float enters as its fp32 value widened to float64.
      g' = g grad_scale;  m' = beta1 m + (1 - beta1) g';  v' = beta2 v + (1 - beta2) g'^2
      p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / bc2 + eps)          (bias_corr = [bc1, bc2]: 1 - beta1^t, sqrt(1 - beta2^t))
    Bounds, counting the kernel's fp32 roundings (u = 2^-24; 1 - beta is exact in fp32 for beta >= 1/2):
      m' : t1 = beta1 m is rounded once, t2 = (1 - beta1) g' twice (g', the product), the sum once more — at most 2 u |t1| + 3 u |t2|,
           taken as 4 u (|t1| + |t2|)
      v' : g' once (it enters squared: 2 u), two products, beta2 v once, the sum once; every term is >= 0, so the errors are
           relative to v' itself: 6 u v'
      p' : decay = fl(1 - fl(lr wd)) is off by at most 2 u, p decay is rounded once and so is the difference: u (4 |p| + |p'|);
           U = step m' / den with step = lr / bc1 and den = sqrt(v') / bc2 + eps carries the error of m' (step bound(m') / den), that of
           v' through the square root (3 u), and one rounding each of the sqrt, the division by bc2, the addition of eps, step, the
           product and the last division (6 u): 9 u |U|, taken as 10 u |U|.
    An fp32 transcription of the kernel's formula against this reference (2^20 elements, 4 steps, gradient scales 1e-6 .. 10,
    grad_scale 1 / 0.37 / 0.013, zeros in p and g) reached 0.48 of the p bound and 0.64 of the m and v bounds.
    Returns dict(p, m, v, bp, bm, bv) in float64."""
    n = p.numel()
    p64, g64, m64, v64 = (t.detach().double() for t in (p, g, m, v))
    hy = hyper.detach().float().double().view(-1, 2)
    lr, wd = seg_expand(seg_end, hy[:, 0], n, start), seg_expand(seg_end, hy[:, 1], n, start)
    b1, b2, e, gs = f32(beta1), f32(beta2), f32(eps), f32(grad_scale)
    bc1, bc2 = (float(x) for x in bias_corr.detach().float().double().cpu())
    gp = g64 * gs
    t1, t2 = b1 * m64, (1.0 - b1) * gp
    mn = t1 + t2
    vn = b2 * v64 + (1.0 - b2) * gp * gp
    den = vn.sqrt() / bc2 + e
    step = lr / bc1
    U = step * mn / den
    pn = p64 * (1.0 - lr * wd) - U
    bm = 4 * U32 * (t1.abs() + t2.abs())
    bv = 6 * U32 * vn
    bp = U32 * (4 * p64.abs() + pn.abs()) + step * bm / den + 10 * U32 * U.abs()
    return dict(p=pn, m=mn, v=vn, bp=bp, bm=bm, bv=bv)


def adamw_grid(n):
    """(workgroups, trips of the grid-stride loop) of dav_adamw_flat at n elements"""
    grid = min(-(-n // ADAMW_CHUNK), ADAMW_GRID_CAP)
    return grid, -(-n // (grid * ADAMW_CHUNK))


def adamw_sumsq_bound(n, sumsq):
    """dav_adamw_flat's fused sum(g^2), an fp32 sum whose depth is the kernel's: a lane adds 4 squares per float4 and visits 4
    float4 per trip, then 6 shuffle levels, 4 wave partials, and one atomic add per workgroup into one fp32 word:
    (16 trips + 6 + 4 + workgroups) u sum(g^2)   (every term >= 0; the rounding of each square rides on its term's count)"""
    grid, trips = adamw_grid(n)
    return (16 * trips + 6 + 4 + grid) * U32 * float(sumsq)


def l2norm_bound(n, ref):
    """dav_l2norm: out = scale sqrt(sum x^2).  A lane of the partial kernel adds 4 squares per float4 over its trips (+ 1 tail element
    in workgroup 0), then 6 shuffle levels and 4 wave partials in fp32: d = 4 trips + 1 + 6 + 4 roundings relative to sum x^2 (all
    terms >= 0).  The partials are combined in double, so the last stage adds only the square root (which halves the relative
    error: d / 2), the scale in double and the one rounding of the stored float: (d / 2 + 2) u |ref|."""
    n4 = n >> 2
    grid = max(1, min(-(-n4 // 256), L2NORM_GRID_CAP))
    trips = -(-n4 // (grid * 256))
    return ((4 * trips + 1 + 6 + 4) / 2 + 2) * U32 * abs(float(ref))


def rows_axpy_bound(res, y, s_rows, ref):
    """out = res + s y per row (dav_rows_axpy): the product and the sum are one rounding each, or one in all where the compiler
    contracts them to an fma — never bit-exact against either, so: u (|res| + 2 |s y| + |out|).  s_rows: [rows, 1] scale per row."""
    return U32 * (res.detach().double().abs() + 2 * (s_rows.detach().double() * y.detach().double()).abs() + ref.detach().double().abs())
