#!/usr/bin/env python3
"""Run every HIP kernel against a torch fp32 reference on the GPU box and print the errors.
Diagnostic companion of tests/ (never aborts on the first failure).  Usage: python tests/gpu_selfcheck.py [filter]"""
import math
import os
import sys
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepavfusion_amd import ops  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import kcheck as kc  # noqa: E402

dev = torch.device('cuda')
BF16, F32 = torch.bfloat16, torch.float32
RESULTS = []


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def report(name, err, tol):
    ok = err <= tol and math.isfinite(err)
    RESULTS.append((name, err, tol, ok))
    print(f'{"PASS" if ok else "FAIL"} {name}: err={err:.3e} tol={tol:.1e}', flush=True)


def elem(name, family, got, ref, bound):
    """elementwise |got - ref| <= bound (tests/kcheck.py); the worst err / bound of each family is kept in kcheck.RATIOS"""
    ok, ratio, msg = kc.within(got, ref, bound, name)
    kc.note(family, ratio)
    RESULTS.append((name + ' elementwise', ratio, 1.0, ok))
    print(f'{"PASS" if ok else "FAIL"} {name} elementwise: worst err/bound={ratio:.3e}' + (f' — {msg}' if msg else ''), flush=True)


def guard(name, g):
    """every byte around a kcheck.Guarded output (guard bands, row padding) still holds its pattern"""
    n, where = g.stray()
    RESULTS.append((name + ' guard', float(n), 0.0, n == 0))
    print(f'{"PASS" if n == 0 else "FAIL"} {name} guard: {n} stray elements' + (f' — first in the {where}' if n else ''), flush=True)


def kept(name, t, before, mask=None):
    """memory the kernel must not touch (rows a row map skips, context rows, padding) is bit-identical to its snapshot"""
    n, i = kc.changed(t, before, mask)
    RESULTS.append((name + ' untouched', float(n), 0.0, n == 0))
    print(f'{"PASS" if n == 0 else "FAIL"} {name} untouched: {n} elements changed' + (f' — first at {kc.tile_of(i, tuple(t.shape))}' if n else ''), flush=True)


def same(name, got, ref):
    """bit-exact: every element of ``got`` equals ``ref`` bit for bit (tests/kcheck.py exact)"""
    n, msg = kc.exact(got, ref, name)
    RESULTS.append((name + ' bit-exact', float(n), 0.0, n == 0))
    print(f'{"PASS" if n == 0 else "FAIL"} {name} bit-exact: {n} elements differ' + (f' — {msg}' if msg else ''), flush=True)


def rejected(name, fn):
    """a call outside the header's contract must fail with an error (RuntimeError from the C ABI), not run"""
    try:
        fn()
        torch.cuda.synchronize()
        ok = False
    except RuntimeError:
        ok = True
    RESULTS.append((name + ' rejected', 0.0 if ok else 1.0, 0.0, ok))
    print(f'{"PASS" if ok else "FAIL"} {name} rejected by the C ABI' + ('' if ok else ' — it ran'), flush=True)


def check(fn):
    def run():
        try:
            fn()
            torch.cuda.synchronize()
        except Exception:
            traceback.print_exc()
            RESULTS.append((fn.__name__, float('nan'), 0, False))
            print(f'FAIL {fn.__name__}: exception', flush=True)
    run.__name__ = fn.__name__
    return run


def rnd(*shape, dtype=F32, scale=1.0, seed=None):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed if seed is not None else (hash(shape) & 0xffff))
    return (torch.randn(*shape, generator=g) * scale).to(device=dev, dtype=dtype)


@check
def gemm_nt():
    gelu64 = lambda x: 0.5 * x * (1 + torch.erf(x * 0.5 ** 0.5))
    dgelu64 = lambda x: 0.5 * (1 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * math.pi) ** 0.5
    for (M, N, K) in [(162, 192, 64), (5184, 2304, 768), (130, 768, 3072), (64, 48, 192), (512, 512, 48), (4032, 768, 256), (37, 100, 136)]:
        A, Bm = rnd(M, K, dtype=BF16, seed=1), rnd(N, K, dtype=BF16, scale=0.05, seed=2)
        prod64 = A.double() @ Bm.double().t()
        acc64 = kc.C_GEMM * kc.U32 * K * kc.gemm_scale(A, Bm)
        for variant in (0, 1, 2, 3):
            A, Bm = rnd(M, K, dtype=BF16, seed=1), rnd(N, K, dtype=BF16, scale=0.05, seed=2)
            bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
            ref = A.float() @ Bm.float().t() + bias
            pre64 = prod64 + bias.double()
            tag = f'gemm_nt {M}x{N}x{K} v{variant}'
            C = kc.poisoned((M, N), F32, dev)
            ops.gemm_nt(A, Bm, M, N, K, bias=bias, C_out=C, variant=variant)
            report(f'gemm_nt {M}x{N}x{K} v{variant} bias', rel(C, ref), 1e-4)
            elem(tag + ' bias', 'gemm_nt', C, pre64, acc64 + kc.out_round(F32) * pre64.abs())
            # gelu + preact twin, bf16 out
            U = kc.poisoned((M, N), BF16, dev)
            Z = kc.poisoned((M, N), BF16, dev)
            ops.gemm_nt(A, Bm, M, N, K, bias=bias, act=1, C_out=U, c_bf16=True, C2=Z, ldc2=N, c2_mode=1, variant=variant)
            report(f'gemm_nt {M}x{N}x{K} v{variant} gelu', rel(U, torch.nn.functional.gelu(ref)), 6e-3)
            report(f'gemm_nt {M}x{N}x{K} v{variant} preact', rel(Z, ref), 6e-3)
            elem(tag + ' gelu', 'gemm_nt', U, gelu64(pre64), kc.gelu_bound(acc64, gelu64(pre64), BF16))
            elem(tag + ' preact', 'gemm_nt', Z, pre64, acc64 + kc.U16 * pre64.abs())
            # gelu fp32 out (the erf approximation itself: |err| <= 1.5e-7) + GELU' twin; then the multiply-only backward form
            U32 = kc.poisoned((M, N), F32, dev)
            D = kc.poisoned((M, N), BF16, dev)
            ops.gemm_nt(A, Bm, M, N, K, bias=bias, act=1, C_out=U32, C2=D, ldc2=N, c2_mode=4, variant=variant)
            xg = ref.clone().requires_grad_(True)
            torch.nn.functional.gelu(xg).sum().backward()
            report(f'gemm_nt {M}x{N}x{K} v{variant} gelu32', float((U32 - torch.nn.functional.gelu(ref)).abs().max()), 2e-5)
            report(f"gemm_nt {M}x{N}x{K} v{variant} gelu'twin", float((D.float() - xg.grad).abs().max()), 5e-3)
            elem(tag + ' gelu32', 'gemm_nt', U32, gelu64(pre64), kc.gelu_bound(acc64, gelu64(pre64), F32))
            elem(tag + " gelu'twin", 'gemm_nt', D, dgelu64(pre64), kc.dgelu_bound(acc64, dgelu64(pre64), BF16))
            G = kc.poisoned((M, N), F32, dev)
            ops.gemm_nt(A, Bm, M, N, K, act=3, aux=D, ldaux=N, C_out=G, variant=variant)
            report(f'gemm_nt {M}x{N}x{K} v{variant} act3', rel(G, (ref - bias) * D.float()), 1e-4)
            g64 = prod64 * D.double()
            elem(tag + ' act3', 'gemm_nt', G, g64, acc64 * D.double().abs() + kc.out_round(F32) * g64.abs())
            # residual + beta accumulate (into a random prefill) + bf16 twin of the final value
            C0 = kc.prefilled((M, N), F32, dev, seed=M + N + variant)
            C = C0.clone()
            T = kc.poisoned((M, N), BF16, dev)
            ops.gemm_nt(A, Bm, M, N, K, res=res, ldres=N, C_out=C, beta=1, C2=T, ldc2=N, c2_mode=3, variant=variant)
            report(f'gemm_nt {M}x{N}x{K} v{variant} res+beta', rel(C, ref - bias + res + C0), 1e-4)
            report(f'gemm_nt {M}x{N}x{K} v{variant} twin', rel(T, ref - bias + res + C0), 6e-3)
            fin64 = prod64 + res.double() + C0.double()
            elem(tag + ' res+beta', 'gemm_nt', C, fin64, acc64 + kc.out_round(F32) * fin64.abs())
            elem(tag + ' twin', 'gemm_nt', T, fin64, acc64 + kc.U16 * fin64.abs())
    # every second-generation tile configuration (explicit cfg in variant bits 4-11)
    for (M, N, K) in [(5184, 2304, 768), (300, 200, 128), (4032, 768, 3072)]:
        A, Bm = rnd(M, K, dtype=BF16, seed=1), rnd(N, K, dtype=BF16, scale=0.05, seed=2)
        bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
        ref = A.float() @ Bm.float().t() + bias + res
        ref64 = A.double() @ Bm.double().t() + bias.double() + res.double()
        bnd = kc.gemm_bound(A, Bm, ref64, F32)
        experimental = (1, 13, 15, 16, 17, 18, 19, 20, 21, 22) if ops._lib.load().dav_build_flags() & 1 else ()      # make EXPERIMENTAL=1
        for cfg in (3, 5, 7, 8, 60) + experimental:
            g = kc.Guarded(M, N, F32, ld=N + 8 * (cfg % 3), device=dev)            # poisoned, inside guard bands, row stride > N for most
            C = g.t
            ops.gemm_nt(A, Bm, M, N, K, bias=bias, res=res, ldres=N, C_out=C, ldc=g.ld, variant=cfg << 4)
            report(f'gemm_nt {M}x{N}x{K} cfg{cfg}', rel(C, ref), 1e-4)
            elem(f'gemm_nt {M}x{N}x{K} cfg{cfg}', 'gemm_nt', C, ref64, bnd)
            guard(f'gemm_nt {M}x{N}x{K} cfg{cfg} ldc{g.ld}', g)
    # the big-tile / deep-ring configurations of round 2 (43 / 45 = 256x128, 44 / 46 = 128x256 on 32-deep rings, 7 = 64x64 on
    # four stages) with every epilogue kind the step gives them: staged bf16 output, the SPLIT staged epilogue with a GELU' twin,
    # multiply by aux, fp32 + residual; forward form and b_kn (32-deep stages in b_kn mode are new)
    for (M, N, K) in [(2100, 1024, 512), (1000, 768, 192), (300, 512, 64)]:
        A = rnd(M, K, dtype=BF16, seed=31)
        W_nk, W_kn = rnd(N, K, dtype=BF16, scale=0.05, seed=32), rnd(K, N, dtype=BF16, scale=0.05, seed=33)
        bias, res, aux = rnd(N, seed=34), rnd(M, N, seed=35), rnd(M, N, dtype=BF16, seed=36)
        for cfg in (43, 44, 45, 46, 7, 8, 3):
            for bt in (0, 1):
                Wm, kw = (W_kn, dict(ldb=N)) if bt else (W_nk, {})
                base = A.float() @ (W_kn.float() if bt else W_nk.float().t())
                var = (cfg << 4) | (bt << 12)
                tag = f'gemm_nt {M}x{N}x{K} cfg{cfg} b_kn{bt}'
                W64 = W_kn.double().t() if bt else W_nk.double()
                prod64 = A.double() @ W64.t()
                acc64 = kc.C_GEMM * kc.U32 * K * (A.double().abs() @ W64.abs().t())
                pre64 = prod64 + bias.double()
                gU = kc.Guarded(M, N, BF16, ld=N + 8 * bt, device=dev)
                U, D = gU.t, kc.poisoned((M, N), BF16, dev)
                ops.gemm_nt(A, Wm, M, N, K, bias=bias, act=1, C_out=U, ldc=gU.ld, c_bf16=True, C2=D, ldc2=N, c2_mode=4, variant=var, **kw)
                xg = (base + bias).clone().requires_grad_(True)
                torch.nn.functional.gelu(xg).sum().backward()
                report(tag + ' gelu (staged)', rel(U, torch.nn.functional.gelu(base + bias)), 6e-3)
                report(tag + " gelu' twin (staged)", float((D.float() - xg.grad).abs().max()), 5e-3)
                elem(tag + ' gelu (staged)', 'gemm_nt', U, gelu64(pre64), kc.gelu_bound(acc64, gelu64(pre64), BF16))
                elem(tag + " gelu' twin (staged)", 'gemm_nt', D, dgelu64(pre64), kc.dgelu_bound(acc64, dgelu64(pre64), BF16))
                guard(tag + ' gelu (staged)', gU)
                G = kc.poisoned((M, N), BF16, dev)
                ops.gemm_nt(A, Wm, M, N, K, act=3, aux=aux, ldaux=N, C_out=G, c_bf16=True, variant=var, **kw)
                report(tag + ' act3 bf16', rel(G, base * aux.float()), 6e-3)
                g64 = prod64 * aux.double()
                elem(tag + ' act3 bf16', 'gemm_nt', G, g64, acc64 * aux.double().abs() + kc.U16 * g64.abs())
                gC = kc.Guarded(M, N, F32, ld=N + 40 * (1 - bt), device=dev)
                C = gC.t
                ops.gemm_nt(A, Wm, M, N, K, bias=bias, res=res, ldres=N, C_out=C, ldc=gC.ld, variant=var, **kw)
                report(tag + ' fp32 + res', rel(C, base + bias + res), 1e-4)
                f64 = pre64 + res.double()
                elem(tag + ' fp32 + res', 'gemm_nt', C, f64, acc64 + kc.out_round(F32) * f64.abs())
                guard(tag + ' fp32 + res', gC)
    # 256 x 256 tiles (configuration 60, csrc/gemm_nt256.h; K % 128 == 0): every epilogue kind in both operand modes, ragged M / N
    # edges (tiles of 256 on 2100 / 1000 / 300 rows, 200 .. 2304 columns), a K of a single pair of K-tiles, row maps, grouped form
    for (M, N, K) in [(2100, 1024, 512), (1000, 768, 256), (300, 512, 128), (5184, 2304, 768), (517, 200, 384)]:
        A = rnd(M, K, dtype=BF16, seed=41)
        W_nk, W_kn = rnd(N, K, dtype=BF16, scale=0.05, seed=42), rnd(K, N, dtype=BF16, scale=0.05, seed=43)
        bias, res, aux = rnd(N, seed=44), rnd(M, N, seed=45), rnd(M, N, dtype=BF16, seed=46)
        for bt in (0, 1):
            Wm, kw = (W_kn, dict(ldb=N)) if bt else (W_nk, {})
            base = A.float() @ (W_kn.float() if bt else W_nk.float().t())
            var = (60 << 4) | (bt << 12)
            tag = f'gemm_nt {M}x{N}x{K} cfg60 b_kn{bt}'
            W64 = W_kn.double().t() if bt else W_nk.double()
            prod64 = A.double() @ W64.t()
            acc64 = kc.C_GEMM * kc.U32 * K * (A.double().abs() @ W64.abs().t())
            pre64 = prod64 + bias.double()
            U, D = kc.poisoned((M, N), BF16, dev), kc.poisoned((M, N), BF16, dev)
            ops.gemm_nt(A, Wm, M, N, K, bias=bias, act=1, C_out=U, c_bf16=True, C2=D, ldc2=N, c2_mode=4, variant=var, **kw)
            xg = (base + bias).clone().requires_grad_(True)
            torch.nn.functional.gelu(xg).sum().backward()
            report(tag + ' gelu', rel(U, torch.nn.functional.gelu(base + bias)), 6e-3)
            report(tag + " gelu' twin", float((D.float() - xg.grad).abs().max()), 5e-3)
            elem(tag + ' gelu', 'gemm_nt', U, gelu64(pre64), kc.gelu_bound(acc64, gelu64(pre64), BF16))
            elem(tag + " gelu' twin", 'gemm_nt', D, dgelu64(pre64), kc.dgelu_bound(acc64, dgelu64(pre64), BF16))
            gZ = kc.Guarded(M, N, BF16, ld=N + 8 * (1 + 4 * bt), device=dev)
            Z = gZ.t
            ops.gemm_nt(A, Wm, M, N, K, bias=bias, act=1, C_out=U, c_bf16=True, C2=Z, ldc2=gZ.ld, c2_mode=1, variant=var, **kw)
            report(tag + ' preact twin', rel(Z, base + bias), 6e-3)
            elem(tag + ' preact twin', 'gemm_nt', Z, pre64, acc64 + kc.U16 * pre64.abs())
            guard(tag + f' preact twin ldc2 {gZ.ld}', gZ)
            G = kc.poisoned((M, N), BF16, dev)
            ops.gemm_nt(A, Wm, M, N, K, act=3, aux=aux, ldaux=N, C_out=G, c_bf16=True, variant=var, **kw)
            report(tag + ' act3 bf16', rel(G, base * aux.float()), 6e-3)
            g64 = prod64 * aux.double()
            elem(tag + ' act3 bf16', 'gemm_nt', G, g64, acc64 * aux.double().abs() + kc.U16 * g64.abs())
            xa = aux.float().requires_grad_(True)
            torch.nn.functional.gelu(xa).sum().backward()
            G = kc.poisoned((M, N), BF16, dev)
            ops.gemm_nt(A, Wm, M, N, K, act=2, aux=aux, ldaux=N, C_out=G, c_bf16=True, alpha=0.5, variant=var, **kw)
            report(tag + ' act2 bf16 alpha', rel(G, 0.5 * base * xa.grad), 6e-3)
            dg64 = dgelu64(aux.double())
            a64 = 0.5 * prod64 * dg64
            elem(tag + ' act2 bf16 alpha', 'gemm_nt', G, a64, 0.5 * acc64 * dg64.abs() + kc.dgelu_bound(0.0, dg64, F32) * 0.5 * prod64.abs() + kc.U16 * a64.abs())
            C0 = kc.prefilled((M, N), F32, dev, seed=M + bt)
            C = C0.clone()
            T = kc.poisoned((M, N), BF16, dev)
            ops.gemm_nt(A, Wm, M, N, K, bias=bias, res=res, ldres=N, C_out=C, beta=1, C2=T, ldc2=N, c2_mode=3, variant=var, **kw)
            report(tag + ' fp32 + res + beta', rel(C, base + bias + res + C0), 1e-4)
            report(tag + ' final twin', rel(T, base + bias + res + C0), 6e-3)
            f64 = pre64 + res.double() + C0.double()
            elem(tag + ' fp32 + res + beta', 'gemm_nt', C, f64, acc64 + kc.out_round(F32) * f64.abs())
            elem(tag + ' final twin', 'gemm_nt', T, f64, acc64 + kc.U16 * f64.abs())
            gP = kc.Guarded(M, N, BF16, ld=N + 8 * (M % 2), device=dev, fill=7.0)
            P = gP.t
            ops.gemm_nt(A, Wm, M, N, K, C_out=P, ldc=gP.ld, c_bf16=True, variant=var, **kw)
            report(tag + ' plain bf16', rel(P, base), 6e-3)
            elem(tag + ' plain bf16', 'gemm_nt', P, prod64, acc64 + kc.U16 * prod64.abs())
            guard(tag + f' plain bf16 ldc {gP.ld}', gP)
    # (row maps: A rows 4.. of every batch, C rows 1..)
    Bsz, rpb, tot, N, K = 5, 70, 90, 512, 256
    M = Bsz * rpb
    Afull, Bm = rnd(Bsz * tot, K, dtype=BF16, seed=47), rnd(N, K, dtype=BF16, scale=0.1, seed=48)
    Asub = Afull.view(Bsz, tot, K)[:, 4:4 + rpb, :].reshape(M, K)
    Cfull = torch.zeros(Bsz * tot, N, device=dev, dtype=BF16)
    ops.gemm_nt(Afull, Bm, M, N, K, a_rowmap=(rpb, tot, 4), C_out=Cfull, c_bf16=True, c_rowmap=(rpb, tot, 1), variant=60 << 4)
    ref_full = torch.zeros(Bsz, tot, N, device=dev)
    ref_full[:, 1:1 + rpb] = (Asub.float() @ Bm.float().t()).view(Bsz, rpb, N)
    report('gemm_nt cfg60 rowmaps', rel(Cfull, ref_full.view(-1, N)), 6e-3)
    # the same launch into poison: mapped rows within their bound, the rows the map skips bit-identical
    mapped = torch.zeros(Bsz, tot, dtype=torch.bool, device=dev)
    mapped[:, 1:1 + rpb] = True
    mapped = mapped.view(-1)
    Cp = kc.poisoned((Bsz * tot, N), BF16, dev)
    before = Cp.clone()
    ops.gemm_nt(Afull, Bm, M, N, K, a_rowmap=(rpb, tot, 4), C_out=Cp, c_bf16=True, c_rowmap=(rpb, tot, 1), variant=60 << 4)
    ref64 = Asub.double() @ Bm.double().t()
    elem('gemm_nt cfg60 rowmaps', 'gemm_nt', Cp[mapped], ref64, kc.gemm_bound(Asub, Bm, ref64, BF16))
    kept('gemm_nt cfg60 rowmaps: rows outside c_rowmap', Cp, before, ~mapped)
    # act 2 (multiply by gelu'(aux)) and row maps
    M, N, K = 3 * 7, 128, 64
    Bsz, rpb, tot = 3, 7, 11
    Afull = rnd(Bsz * tot, K, dtype=BF16, seed=5)
    Bm = rnd(N, K, dtype=BF16, scale=0.1, seed=6)
    aux = rnd(M, N, dtype=BF16, seed=7)
    Asub = Afull.view(Bsz, tot, K)[:, 4:, :].reshape(M, K)
    x = aux.float().requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    ref = (Asub.float() @ Bm.float().t()) * x.grad
    Cfull = torch.zeros(Bsz * tot, N, device=dev)
    resfull = rnd(Bsz * tot, N, seed=8)
    ops.gemm_nt(Afull, Bm, M, N, K, a_rowmap=(rpb, tot, 4), act=2, aux=aux, ldaux=N, res=resfull, ldres=N, res_rowmap=(rpb, tot, 2),
                C_out=Cfull, c_rowmap=(rpb, tot, 1))
    ref_full = torch.zeros_like(Cfull).view(Bsz, tot, N)
    ref_full[:, 1:8] = ref.view(Bsz, rpb, N) + resfull.view(Bsz, tot, N)[:, 2:9]
    report('gemm_nt rowmaps+act2', rel(Cfull, ref_full.view(-1, N)), 1e-4)
    # again into poison: mapped rows elementwise, skipped rows bit-identical
    mapped = torch.zeros(Bsz, tot, dtype=torch.bool, device=dev)
    mapped[:, 1:8] = True
    mapped = mapped.view(-1)
    Cp = kc.poisoned((Bsz * tot, N), F32, dev)
    before = Cp.clone()
    ops.gemm_nt(Afull, Bm, M, N, K, a_rowmap=(rpb, tot, 4), act=2, aux=aux, ldaux=N, res=resfull, ldres=N, res_rowmap=(rpb, tot, 2),
                C_out=Cp, c_rowmap=(rpb, tot, 1))
    dg64 = dgelu64(aux.double())
    p64 = Asub.double() @ Bm.double().t()
    r64 = p64 * dg64 + resfull.view(Bsz, tot, N)[:, 2:9].reshape(M, N).double()
    elem('gemm_nt rowmaps+act2', 'gemm_nt', Cp[mapped], r64,
         kc.C_GEMM * kc.U32 * K * kc.gemm_scale(Asub, Bm) * dg64.abs() + kc.dgelu_bound(0.0, dg64, F32) * p64.abs() + kc.out_round(F32) * r64.abs())
    kept('gemm_nt rowmaps+act2: rows outside c_rowmap', Cp, before, ~mapped)
    rows = torch.randint(0, 5, (M,), device=dev, dtype=torch.int32)
    pos = rnd(5, N, seed=9)
    C = kc.poisoned((M, N), F32, dev)
    ops.gemm_nt(Asub.contiguous(), Bm, M, N, K, res=pos, ldres=N, res_rows=rows, C_out=C)
    report('gemm_nt res_rows', rel(C, Asub.float() @ Bm.float().t() + pos[rows.long()]), 1e-4)
    r64 = Asub.double() @ Bm.double().t() + pos.double()[rows.long()]
    elem('gemm_nt res_rows', 'gemm_nt', C, r64, kc.gemm_bound(Asub, Bm, r64, F32))
    # B given as [K, N] (dgrad reading W itself), incl. column offset / ldb and all tile configs
    for (M2, N2, K2) in [(300, 768, 192), (5184, 768, 2304), (2048, 136, 64), (4032, 3072, 768)]:
        A2 = rnd(M2, K2, dtype=BF16, seed=15)
        Wkn = rnd(K2, 2 * N2, dtype=BF16, scale=0.05, seed=16)
        W64 = Wkn[:, N2:].t()
        r64 = A2.double() @ W64.double().t()
        bnd = kc.gemm_bound(A2, W64, r64, F32)
        for cfg in (0, 3, 8, 5):
            g = kc.Guarded(M2, N2, F32, ld=N2 + 8 * (cfg % 2), device=dev)
            C = g.t
            ops.gemm_nt(A2, Wkn.view(-1)[N2:], M2, N2, K2, ldb=2 * N2, C_out=C, ldc=g.ld, variant=(1 << 12) | (cfg << 4))
            report(f'gemm_nt b_kn {M2}x{N2}x{K2} cfg{cfg}', rel(C, A2.float() @ Wkn[:, N2:].float()), 1e-4)
            elem(f'gemm_nt b_kn {M2}x{N2}x{K2} cfg{cfg}', 'gemm_nt', C, r64, bnd)
            guard(f'gemm_nt b_kn {M2}x{N2}x{K2} cfg{cfg} ldc {g.ld}', g)
    # B sub-matrix (column offset, ldb)
    Bw = rnd(N, 2 * K, dtype=BF16, scale=0.1, seed=10)
    C = kc.poisoned((M, N), F32, dev)
    ops.gemm_nt(Asub.contiguous(), Bw.view(-1)[K:], M, N, K, ldb=2 * K, C_out=C)
    report('gemm_nt ldb/offset', rel(C, Asub.float() @ Bw[:, K:].float().t()), 1e-4)
    r64 = Asub.double() @ Bw[:, K:].double().t()
    elem('gemm_nt ldb/offset', 'gemm_nt', C, r64, kc.gemm_bound(Asub, Bw[:, K:], r64, F32))


@check
def gemm_tn():
    for (Mc, N, K) in [(162, 192, 64), (5184, 768, 768), (100, 48, 192), (4032, 256, 768), (77, 136, 200), (6080, 3072, 768), (3136, 192, 768), (128, 72, 40)]:
        for variant in (0, 1, 2, 16, 32):
            A, Bm = rnd(Mc, N, dtype=BF16, seed=11), rnd(Mc, K, dtype=BF16, seed=12)
            ref = A.float().t() @ Bm.float()
            P0, pb0 = kc.prefilled((N, K), F32, dev, seed=Mc + variant), kc.prefilled((N,), F32, dev, seed=N + variant)
            C = P0.clone()
            bg = pb0.clone()
            ops.gemm_tn(A, Bm, Mc, N, K, C, beta=1, bias_grad=bg, variant=variant)
            report(f'gemm_tn {Mc}x{N}x{K} v{variant} acc', rel(C, P0 + ref), 2e-4)
            report(f'gemm_tn {Mc}x{N}x{K} v{variant} bias_grad', rel(bg, pb0 + A.float().sum(0)), 2e-4)
            r64 = A.double().t() @ Bm.double()
            bnd = kc.gemm_bound(A.t(), Bm.t(), r64, F32)
            elem(f'gemm_tn {Mc}x{N}x{K} v{variant} acc', 'gemm_tn', C, P0.double() + r64, bnd + kc.out_round(F32) * P0.double().abs())
            b64 = pb0.double() + A.double().sum(0)
            elem(f'gemm_tn {Mc}x{N}x{K} v{variant} bias_grad', 'gemm_tn', bg, b64, kc.C_GEMM * kc.U32 * Mc * A.double().abs().sum(0) + kc.out_round(F32) * b64.abs())
            gS = kc.Guarded(N, K, F32, ld=K + 8 * (variant % 3), device=dev, fill=7.0)
            C = gS.t
            ops.gemm_tn(A, Bm, Mc, N, K, C, ldc=gS.ld, beta=0, variant=variant)
            report(f'gemm_tn {Mc}x{N}x{K} v{variant} store', rel(C, ref), 2e-4)
            elem(f'gemm_tn {Mc}x{N}x{K} v{variant} store', 'gemm_tn', C, r64, bnd)
            guard(f'gemm_tn {Mc}x{N}x{K} v{variant} store ldc {gS.ld}', gS)
    # grouped launch of several problems (deferred wgrads of a layer), incl. bias grads and the split-K path; every gradient starts
    # from a random prefill inside its own guard bands (a stray write into a neighbour's gradient shows there)
    probs, refs, pres = [], [], []
    for i, (Mc, N, K) in enumerate([(3136, 768, 768), (3136, 2304, 768), (4032, 768, 3072), (512, 192, 768), (2048, 72, 136), (6080, 3072, 768)]):
        A, Bm = rnd(Mc, N, dtype=BF16, seed=60 + i), rnd(Mc, K, dtype=BF16, seed=70 + i)
        P0, pb0 = kc.prefilled((N, K), F32, dev, seed=80 + i), kc.prefilled((N,), F32, dev, seed=90 + i)
        gC = kc.Guarded(N, K, F32, ld=K + 8 * (i % 3), device=dev, fill=P0)
        C = gC.t
        bg = pb0.clone() if i % 2 == 0 else None
        probs.append(dict(A=A, B=Bm, Mc=Mc, N=N, K=K, C=C, lda=N, ldb=K, ldc=gC.ld, bias_grad=bg, guard=gC))
        refs.append((C, P0 + A.float().t() @ Bm.float(), bg, None if bg is None else pb0 + A.float().sum(0)))
        pres.append((P0, pb0))

    def tn_elem(tag, i, times=1, written=False):
        """gradient == (0 if written else prefill) + times * A^T B, bias == prefill + times * colsum(A), each element within its bound"""
        pr, (P0, pb0) = probs[i], pres[i]
        r64 = (0.0 if written else P0.double()) + times * (pr['A'].double().t() @ pr['B'].double())
        elem(tag + ' C', 'gemm_tn', pr['C'], r64, times * kc.gemm_bound(pr['A'].t(), pr['B'].t(), r64, F32))
        if pr['bias_grad'] is not None:
            b64 = pb0.double() + times * pr['A'].double().sum(0)
            elem(tag + ' bias', 'gemm_tn', pr['bias_grad'], b64,
                 times * kc.C_GEMM * kc.U32 * pr['Mc'] * pr['A'].double().abs().sum(0) + kc.out_round(F32) * b64.abs())
        guard(tag + f' ldc {pr["ldc"]}', pr['guard'])
    ops.gemm_tn_grouped(probs)
    for i, (C, rc, bg, rb) in enumerate(refs):
        report(f'gemm_tn grouped #{i} C', rel(C, rc), 2e-4)
        if bg is not None:
            report(f'gemm_tn grouped #{i} bias', rel(bg, rb), 2e-4)
        tn_elem(f'gemm_tn grouped #{i}', i)
    ops.gemm_tn_grouped(probs[:2])        # small group -> split-K atomics path
    report('gemm_tn grouped split acc', rel(refs[0][0], 2 * refs[0][1] - pres[0][0]), 2e-4)
    for i in range(2):
        tn_elem(f'gemm_tn grouped split #{i}', i, times=2)
    # written (not accumulated) tiles: DavTnProblem.flags bit 0 — old contents (NaN here) are ignored, the bias gradient still
    # accumulates, never split over the contraction (a small group would otherwise take the atomics path); mixed with an accumulating problem
    for group in (probs[:2], probs):
        for i, pr in enumerate(group):
            pr['overwrite'] = i != 1
            if pr['overwrite']:
                pr['C'].fill_(float('nan'))
            else:
                pr['C'].copy_(pres[i][0])
            if pr['bias_grad'] is not None:
                pr['bias_grad'].copy_(pres[i][1])
        ops.gemm_tn_grouped(group)
        for i, (C, rc, bg, rb) in enumerate(refs[:len(group)]):
            report(f'gemm_tn grouped[{len(group)}] #{i} {"written" if i != 1 else "accumulated"}', rel(C, rc - (pres[i][0] if i != 1 else 0.0)), 2e-4)
            if bg is not None:
                report(f'gemm_tn grouped[{len(group)}] #{i} bias', rel(bg, rb), 2e-4)
            tn_elem(f'gemm_tn grouped[{len(group)}] #{i} {"written" if i != 1 else "accumulated"}', i, written=i != 1)
    for pr in probs:
        pr.pop('overwrite')
        pr.pop('guard')
    # row maps + ldc sub-block
    Bsz, rpb, tot, N, K = 3, 5, 9, 64, 128
    Af, Bf = rnd(Bsz * tot, N, dtype=BF16, seed=13), rnd(Bsz * tot, K, dtype=BF16, seed=14)
    As = Af.view(Bsz, tot, N)[:, 2:7].reshape(-1, N)
    Bs = Bf.view(Bsz, tot, K)[:, 4:9].reshape(-1, K)
    Cw = torch.zeros(N, 2 * K, device=dev)
    ops.gemm_tn(Af, Bf, Bsz * rpb, N, K, Cw.view(-1)[K:], ldc=2 * K, a_rowmap=(rpb, tot, 2), b_rowmap=(rpb, tot, 4), beta=1)
    ref = torch.zeros_like(Cw)
    ref[:, K:] = As.float().t() @ Bs.float()
    report('gemm_tn rowmaps+ldc', rel(Cw, ref), 2e-4)
    gW = kc.Guarded(N, K, F32, ld=2 * K, device=dev, fill=kc.prefilled((N, K), F32, dev, seed=99))
    P0 = gW.t.clone()
    ops.gemm_tn(Af, Bf, Bsz * rpb, N, K, gW.t, ldc=gW.ld, a_rowmap=(rpb, tot, 2), b_rowmap=(rpb, tot, 4), beta=1)
    r64 = P0.double() + As.double().t() @ Bs.double()
    elem('gemm_tn rowmaps+ldc (prefilled)', 'gemm_tn', gW.t, r64, kc.gemm_bound(As.t(), Bs.t(), r64, F32))
    guard('gemm_tn rowmaps+ldc (prefilled) ldc 2K', gW)


@check
def gemm_tn_gang():
    """dav_gemm_tn_gang_bf16: the queued weight gradients of several layers as one persistent launch of 256 x 256 tiles."""
    # odd K-tile counts (Mc = 64 * odd), N / K below, across and beyond one tile, ragged last tiles, a long contraction
    shapes = [(512, 768, 768), (3136, 192, 768), (4032, 2304, 768), (3136, 768, 3072), (640, 8, 264), (14592, 512, 1536), (2048, 520, 776),
              (64, 256, 256), (192, 1032, 40), (5184, 2304, 768), (6080, 3072, 1024),
              (2592, 1024, 1024), (3040, 1024, 3072), (1568, 4096, 1024), (40, 264, 520), (200, 8, 8), (63 * 8, 768, 192)]      # ragged: Mc % 64 != 0
    for mode in ('accumulate', 'written', 'mixed'):
        probs, refs, guards = [], [], []
        for i, (Mc, N, K) in enumerate(shapes):
            A, Bm = rnd(Mc, N, dtype=BF16, seed=160 + i), rnd(Mc, K, dtype=BF16, seed=170 + i)
            ow = mode == 'written' or (mode == 'mixed' and i % 2 == 0)
            gC = kc.Guarded(N, K, F32, ld=K + 8 * (0, 0, 1, 5)[i % 4], device=dev, fill=float('nan') if ow else 0.25)
            C = gC.t
            bg = torch.full((N,), 0.5, device=dev) if i % 3 != 1 else None
            probs.append(dict(A=A, B=Bm, Mc=Mc, N=N, K=K, C=C, lda=N, ldb=K, ldc=gC.ld, bias_grad=bg, overwrite=ow))
            refs.append((C, (0.0 if ow else 0.25) + A.float().t() @ Bm.float(), bg, None if bg is None else 0.5 + A.float().sum(0)))
            guards.append(gC)
        kc.gang(probs)
        for i, (C, rc, bg, rb) in enumerate(refs):
            report(f'gemm_tn_gang {mode} #{i} {shapes[i]} C', rel(C, rc), 2e-4)
            if bg is not None:
                report(f'gemm_tn_gang {mode} #{i} bias', rel(bg, rb), 2e-4)
            pr = probs[i]
            r64 = (0.0 if pr['overwrite'] else 0.25) + pr['A'].double().t() @ pr['B'].double()
            elem(f'gemm_tn_gang {mode} #{i} {shapes[i]} C', 'gemm_tn_gang', C, r64, kc.gemm_bound(pr['A'].t(), pr['B'].t(), r64, F32))
            guard(f'gemm_tn_gang {mode} #{i} {shapes[i]} ldc {pr["ldc"]}', guards[i])
    # bit-repeatable whoever draws which ticket: the same launch twice, written tiles
    Cs = []
    for _ in range(2):
        for pr in probs:
            pr['overwrite'] = True
            pr['C'], pr['ldc'] = kc.poisoned((pr['N'], pr['K']), F32, dev), pr['K']
        kc.gang(probs)
        torch.cuda.synchronize()
        Cs.append([pr['C'].clone() for pr in probs])
    report('gemm_tn_gang bit-repeatable', float(max((a != b).sum() for a, b in zip(*Cs))), 0.0)
    # row maps on both operands + a column block of a wider gradient (ldc), rows-per-batch below and above 64
    for (Bsz, rpb, tot, offa, offb, N, K) in [(16, 12, 20, 3, 8, 320, 136), (8, 81, 95, 14, 0, 768, 512), (64, 8, 40, 32, 0, 264, 768)]:
        Af, Bf = rnd(Bsz * tot, N, dtype=BF16, seed=113), rnd(Bsz * tot, K, dtype=BF16, seed=114)
        Mc = Bsz * rpb                    # (8 x 81 = 648 rows: a ragged contraction THROUGH a row map — ViT-L's towers at small batch)
        As = Af.view(Bsz, tot, N)[:, offa:offa + rpb].reshape(-1, N)
        Bs = Bf.view(Bsz, tot, K)[:, offb:offb + rpb].reshape(-1, K)
        Cw = torch.zeros(N, 2 * K, device=dev)
        ops.gemm_tn_gang([dict(A=Af, B=Bf, Mc=Mc, N=N, K=K, C=Cw.view(-1)[K:], lda=N, ldb=K, ldc=2 * K, a_rowmap=(rpb, tot, offa),
                               b_rowmap=(rpb, tot, offb), bias_grad=None)])
        ref = torch.zeros_like(Cw)
        ref[:, K:] = As.float().t() @ Bs.float()
        report(f'gemm_tn_gang rowmaps+ldc rpb={rpb}', rel(Cw, ref), 2e-4)
        # written into poison with a row stride of K + 24, inside guards (0xFF workspace)
        gC = kc.Guarded(N, K, F32, ld=K + 24, device=dev)
        kc.gang([dict(A=Af, B=Bf, Mc=Mc, N=N, K=K, C=gC.t, lda=N, ldb=K, ldc=gC.ld, a_rowmap=(rpb, tot, offa), b_rowmap=(rpb, tot, offb),
                   bias_grad=None, overwrite=True)])
        r64 = As.double().t() @ Bs.double()
        elem(f'gemm_tn_gang rowmaps written rpb={rpb}', 'gemm_tn_gang', gC.t, r64, kc.gemm_bound(As.t(), Bs.t(), r64, F32))
        guard(f'gemm_tn_gang rowmaps written rpb={rpb} ldc {gC.ld}', gC)
    # a few hundred problems in one launch (several table-writer launches)
    many, refs = [], []
    for i in range(150):
        Mc, N, K = 64 * (1 + i % 5), 8 * (1 + (7 * i) % 60), 8 * (1 + (11 * i) % 70)
        A, Bm = rnd(Mc, N, dtype=BF16, seed=300 + i), rnd(Mc, K, dtype=BF16, seed=500 + i)
        C = torch.zeros(N, K, device=dev)
        many.append(dict(A=A, B=Bm, Mc=Mc, N=N, K=K, C=C, lda=N, ldb=K, ldc=K, bias_grad=None, overwrite=bool(i & 1)))
        refs.append(A.float().t() @ Bm.float())
    ops.gemm_tn_gang(many)
    report('gemm_tn_gang 150 problems', max(rel(pr['C'], r) for pr, r in zip(many, refs)), 2e-4)
    # one very wide weight: 50 x 50 tiles = 104 gangs, more than one table-writer launch carries (its tickets span two), beside a small one
    A, Bm = rnd(64, 12800, dtype=BF16, seed=700), rnd(64, 12800, dtype=BF16, seed=701)
    A2, B2 = rnd(100, 264, dtype=BF16, seed=702), rnd(100, 40, dtype=BF16, seed=703)
    Cbig, C2 = kc.poisoned((12800, 12800), F32, dev), torch.zeros(264, 40, device=dev)
    ops.gemm_tn_gang([dict(A=A, B=Bm, Mc=64, N=12800, K=12800, C=Cbig, lda=12800, ldb=12800, ldc=12800, bias_grad=None, overwrite=True),
                      dict(A=A2, B=B2, Mc=100, N=264, K=40, C=C2, lda=264, ldb=40, ldc=40, bias_grad=None)])
    report('gemm_tn_gang 12800 x 12800 weight (104 gangs)', rel(Cbig, A.float().t() @ Bm.float()), 2e-4)
    report('gemm_tn_gang ... and the problem after it', rel(C2, A2.float().t() @ B2.float()), 2e-4)
    del Cbig


def ref_attn(q, k, v, scale):
    s = (q @ k.transpose(-2, -1)) * scale
    return s.softmax(-1) @ v


@check
def patch_gather3d():
    for (B, C, T, H, W, pt) in [(2, 3, 4, 48, 32, 2), (1, 3, 8, 64, 64, 2), (2, 1, 3, 32, 48, 1)]:
        x = rnd(B, C, T, H, W, seed=91)
        gt, gh, gw = T // pt, H // 16, W // 16
        L = gt * gh * gw
        cols = x.view(B, C, gt, pt, gh, 16, gw, 16).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, L, C * pt * 256)
        A = kc.poisoned((B * L, C * pt * 256), BF16, dev)
        ops.patch_gather(x, None, L, A, pt)
        report(f'patch_gather3d all {B}x{C}x{T}x{H}x{W}', rel(A.view(B, L, -1), cols.to(BF16)), 1e-6)
        nk = max(1, L // 3)
        ids = torch.stack([torch.randperm(L, device=dev)[:nk] for _ in range(B)]).to(torch.int32)
        A2 = kc.poisoned((B * nk, C * pt * 256), BF16, dev)
        ops.patch_gather(x, ids, nk, A2, pt)
        ref = torch.gather(cols, 1, ids.long().unsqueeze(-1).expand(-1, -1, cols.shape[-1]))
        report(f'patch_gather3d kept {B}x{C}x{T}x{H}x{W}', rel(A2.view(B, nk, -1), ref.to(BF16)), 1e-6)
        # bit-exact (a copy + one round-to-nearest-even), guarded, and the fp32 twin dav_patch_gather_f32 (an exact copy)
        for sel, n, want in ((None, L, cols), (ids, nk, ref)):
            for dt in (BF16, F32):
                nm = f'patch_gather3d {"kept" if sel is not None else "all"} {B}x{C}x{T}x{H}x{W}' + (' fp32' if dt == F32 else '')
                g = kc.Guarded(B * n, C * pt * 256, dt, device=dev)
                ops.patch_gather(x, sel, n, g.t, pt)
                same(nm, g.t.view(B, n, -1), want.to(dt))
                guard(nm, g)


@check
def attention():
    for (B, H, Nq, Nk, dqk, dv, off) in [(2, 3, 49, 81, 64, 64, 32), (3, 2, 8, 49, 64, 64, 0), (2, 16, 228, 228, 32, 32, 0),
                                        (2, 2, 352, 352, 32, 32, 0), (2, 12, 16, 64, 16, 64, 0), (3, 2, 4, 6, 16, 64, 0),
                                        (2, 2, 5, 13, 64, 64, 8), (1, 1, 1, 1, 32, 32, 0), (2, 12, 63, 95, 64, 64, 32),
                                        # long sequences: keys / queries stream through LDS in chunks
                                        (2, 3, 784, 816, 64, 64, 32), (2, 2, 352, 352, 64, 64, 0), (1, 2, 100, 1000, 64, 64, 0),
                                        (1, 2, 1000, 40, 64, 64, 0), (2, 2, 1300, 1300, 32, 32, 0), (1, 3, 17, 530, 16, 64, 0),
                                        (1, 2, 257, 257, 64, 64, 0),
                                        # q/k/v head width 16 (token / dense_mmi fusion archs at attn_ratio 0.25)
                                        (2, 12, 32, 112, 16, 16, 0), (1, 3, 32, 3087, 16, 16, 0), (2, 2, 9, 20, 16, 16, 0)]:
        scale = 0.125 if dqk == 16 else dqk ** -0.5
        # fused layout when dqk == dv: buffer [B, Nk, 3, H, d]; queries are rows off.. of the same buffer
        fused = dqk == dv and Nq <= Nk
        if fused:
            buf = rnd(B, Nk, 3, H, dqk, dtype=BF16, seed=21)
            assert Nq + off == Nk or off == 0
            qo = off if Nq + off == Nk else 0
            qt = (buf, qo * 3 * H * dqk); kt = (buf, H * dqk); vt = (buf, 2 * H * dqk)
            strides = (Nk * 3 * H * dqk, 3 * H * dqk) * 3
            q = buf[:, qo:qo + Nq, 0].permute(0, 2, 1, 3).float()
            k = buf[:, :, 1].permute(0, 2, 1, 3).float()
            v = buf[:, :, 2].permute(0, 2, 1, 3).float()
        else:
            qb, kb, vb = rnd(B, Nq, H, dqk, dtype=BF16, seed=22), rnd(B, Nk, H, dqk, dtype=BF16, seed=23), rnd(B, Nk, H, dv, dtype=BF16, seed=24)
            qt, kt, vt = (qb, 0), (kb, 0), (vb, 0)
            strides = (Nq * H * dqk, H * dqk, Nk * H * dqk, H * dqk, Nk * H * dv, H * dv)
            q, k, v = qb.permute(0, 2, 1, 3).float(), kb.permute(0, 2, 1, 3).float(), vb.permute(0, 2, 1, 3).float()
        q.requires_grad_(True); k.requires_grad_(True); v.requires_grad_(True)
        ref = ref_attn(q, k, v, scale)
        O = kc.poisoned((B * Nq, H * dv), BF16, dev)
        LSE = kc.poisoned((B, H, Nq), F32, dev)
        p = lambda t: t[0].data_ptr() + 2 * t[1]
        ops.attn_fwd(p(qt), p(kt), p(vt), O, LSE, B, H, Nq, Nk, dqk, dv, *strides, Nq * H * dv, H * dv, scale)
        tag = f'attn B{B} H{H} {Nq}x{Nk} d{dqk}/{dv}'
        report(tag + ' fwd', rel(O.view(B, Nq, H, dv).permute(0, 2, 1, 3), ref), 1e-2)
        lse_ref = torch.logsumexp((q @ k.transpose(-2, -1)) * scale, -1)
        report(tag + ' lse', rel(LSE, lse_ref), 1e-4)
        dO = rnd(B * Nq, H * dv, dtype=BF16, seed=25)
        ref.backward(dO.view(B, Nq, H, dv).permute(0, 2, 1, 3).float())
        Ok = O.view(B, Nq, H, dv).permute(0, 2, 1, 3)
        r64 = kc.attn_bounds(q, k, v, dO.view(B, Nq, H, dv).permute(0, 2, 1, 3), Ok, scale)
        elem(tag + ' fwd', 'attention', Ok, r64['O'], r64['bO'])
        elem(tag + ' lse', 'attention', LSE, r64['lse'], r64['blse'])
        if fused:
            dbuf = kc.poisoned(buf.shape, BF16, dev)                 # the q slots of the qo context rows stay poisoned (checked below)
            dqt = (dbuf, qt[1]); dkt = (dbuf, kt[1]); dvt = (dbuf, vt[1])
        else:
            dqb, dkb, dvb = (kc.poisoned(t.shape, BF16, dev) for t in (qb, kb, vb))
            dqt, dkt, dvt = (dqb, 0), (dkb, 0), (dvb, 0)
        Delta = torch.empty_like(LSE)
        ops.attn_bwd(p(qt), p(kt), p(vt), O, dO, LSE, Delta, p(dqt), p(dkt), p(dvt), B, H, Nq, Nk, dqk, dv, *strides,
                     Nq * H * dv, H * dv, Nq * H * dv, H * dv, *strides, scale)
        if fused:
            gq = dbuf[:, qo:qo + Nq, 0].permute(0, 2, 1, 3); gk = dbuf[:, :, 1].permute(0, 2, 1, 3); gv = dbuf[:, :, 2].permute(0, 2, 1, 3)
        else:
            gq, gk, gv = dqb.permute(0, 2, 1, 3), dkb.permute(0, 2, 1, 3), dvb.permute(0, 2, 1, 3)
        report(tag + ' dq', rel(gq, q.grad), 2e-2)
        report(tag + ' dk', rel(gk, k.grad), 2e-2)
        report(tag + ' dv', rel(gv, v.grad), 2e-2)
        elem(tag + ' dq', 'attention', gq, r64['dq'], r64['bdq'])
        elem(tag + ' dk', 'attention', gk, r64['dk'], r64['bdk'])
        elem(tag + ' dv', 'attention', gv, r64['dv'], r64['bdv'])
        if fused and qo > 0:
            # dav_attn_bwd_ctx: the dQ kernel zero-fills the q slots of the qo context-only rows in front of the queries — into a
            # buffer full of NaNs the whole fused gradient must come out equal to the one written into zeros above
            ctx = torch.zeros(B, Nk, 3, dtype=torch.bool, device=dev)
            ctx[:, :qo, 0] = True
            kept(tag + f' q slots of the {qo} context rows (plain backward)', dbuf, kc.poisoned(buf.shape, BF16, dev), ctx)
            dbuf2 = torch.full_like(buf, float('nan'))
            ops.attn_bwd(p(qt), p(kt), p(vt), O, dO, LSE, Delta, dbuf2.data_ptr() + 2 * qt[1], dbuf2.data_ptr() + 2 * kt[1],
                         dbuf2.data_ptr() + 2 * vt[1], B, H, Nq, Nk, dqk, dv, *strides, Nq * H * dv, H * dv, Nq * H * dv, H * dv,
                         *strides, scale, dq_ctx_rows=qo)
            want = dbuf.clone()
            want[:, :qo, 0] = 0.0
            same = torch.equal(dbuf2, want) and float(dbuf2[:, :qo, 0].abs().max()) == 0.0
            report(tag + f' ctx rows {qo}', 0.0 if same else 1.0, 1e-9)


@check
def dropout():
    """Attention dropout (dav_attn_drop_fwd / _bwd, bf16 and fp32 kernels) and dropout on activations (dav_dropout_rows) against
    torch with the SAME keep masks: the kernels are deterministic in the mask, the draw is the caller's."""
    for (B, H, Nq, Nk, dqk, dv, off, pdrop) in [(2, 3, 49, 81, 64, 64, 32, 0.1), (3, 2, 8, 49, 64, 64, 0, 0.5), (2, 16, 228, 228, 32, 32, 0, 0.1),
                                               (2, 12, 16, 64, 16, 64, 0, 0.2), (3, 2, 4, 6, 16, 64, 0, 0.3), (1, 1, 1, 1, 32, 32, 0, 0.5),
                                               (2, 12, 63, 95, 64, 64, 32, 0.1), (2, 2, 204, 204, 64, 64, 0, 0.1),
                                               (2, 12, 32, 112, 16, 16, 0, 0.2), (1, 3, 32, 3087, 16, 16, 0, 0.1), (2, 2, 9, 20, 16, 16, 0, 0.3),
                                               # chunked variants (keys / queries stream through LDS)
                                               (2, 3, 784, 816, 64, 64, 32, 0.1), (1, 2, 100, 1000, 64, 64, 0, 0.2), (1, 2, 1000, 40, 64, 64, 0, 0.1),
                                               (2, 2, 1300, 1300, 32, 32, 0, 0.1), (1, 3, 17, 530, 16, 64, 0, 0.25)]:
        scale = 0.125 if dqk == 16 else dqk ** -0.5
        keep_p = 1.0 - pdrop
        ld = (Nk + 31) // 32 * 32
        g = torch.Generator(device='cpu'); g.manual_seed(1000 + Nq * 7 + Nk)
        keep = (torch.rand(B, H, Nq, ld, generator=g) < keep_p).to(torch.uint8).to(dev)
        km = keep[..., :Nk].float() / keep_p
        for f32 in (False, True):
            dt = F32 if f32 else BF16
            es = 4 if f32 else 2
            fused = dqk == dv and Nq <= Nk
            if fused:
                buf = rnd(B, Nk, 3, H, dqk, dtype=dt, seed=21)
                qo = off if Nq + off == Nk else 0
                qt = (buf, qo * 3 * H * dqk); kt = (buf, H * dqk); vt = (buf, 2 * H * dqk)
                strides = (Nk * 3 * H * dqk, 3 * H * dqk) * 3
                q = buf[:, qo:qo + Nq, 0].permute(0, 2, 1, 3).float()
                k = buf[:, :, 1].permute(0, 2, 1, 3).float()
                v = buf[:, :, 2].permute(0, 2, 1, 3).float()
            else:
                qo = 0
                qb, kb, vb = rnd(B, Nq, H, dqk, dtype=dt, seed=22), rnd(B, Nk, H, dqk, dtype=dt, seed=23), rnd(B, Nk, H, dv, dtype=dt, seed=24)
                qt, kt, vt = (qb, 0), (kb, 0), (vb, 0)
                strides = (Nq * H * dqk, H * dqk, Nk * H * dqk, H * dqk, Nk * H * dv, H * dv)
                q, k, v = qb.permute(0, 2, 1, 3).float(), kb.permute(0, 2, 1, 3).float(), vb.permute(0, 2, 1, 3).float()
            q.requires_grad_(True); k.requires_grad_(True); v.requires_grad_(True)
            ref = (((q @ k.transpose(-2, -1)) * scale).softmax(-1) * km) @ v
            O = kc.poisoned((B * Nq, H * dv), dt, dev)
            LSE = kc.poisoned((B, H, Nq), F32, dev)
            p = lambda t: t[0].data_ptr() + es * t[1]
            ops.attn_drop_fwd(p(qt), p(kt), p(vt), O, LSE, B, H, Nq, Nk, dqk, dv, *strides, Nq * H * dv, H * dv, scale, keep, ld, 1.0 / keep_p)
            tag = f'attn_drop {"f32" if f32 else "bf16"} B{B} H{H} {Nq}x{Nk} d{dqk}/{dv} p{pdrop}'
            tf, tb = (2e-5, 5e-5) if f32 else (1e-2, 2e-2)
            report(tag + ' fwd', rel(O.view(B, Nq, H, dv).permute(0, 2, 1, 3), ref), tf)
            report(tag + ' lse', rel(LSE, torch.logsumexp((q @ k.transpose(-2, -1)) * scale, -1)), 1e-4)
            dO = rnd(B * Nq, H * dv, dtype=dt, seed=25)
            ref.backward(dO.view(B, Nq, H, dv).permute(0, 2, 1, 3).float())
            Ok = O.view(B, Nq, H, dv).permute(0, 2, 1, 3)
            up, ro = (2.0 ** -18, 4 * kc.U32) if f32 else (kc.U16, kc.U16)
            r64 = kc.attn_bounds(q, k, v, dO.view(B, Nq, H, dv).permute(0, 2, 1, 3), Ok, scale, keep=km, up=up, r_out=ro)
            elem(tag + ' fwd', 'dropout', Ok, r64['O'], r64['bO'])
            elem(tag + ' lse', 'dropout', LSE, r64['lse'], r64['blse'])
            fill = float('nan')             # written outputs (bf16 with context rows: the dQ kernel zero-fills their q slots)
            if fused:
                dbuf = torch.full_like(buf, fill)
                dqt = (dbuf, qt[1]); dkt = (dbuf, kt[1]); dvt = (dbuf, vt[1])
            else:
                dqb, dkb, dvb = (kc.poisoned(t.shape, dt, dev) for t in (qb, kb, vb))
                dqt, dkt, dvt = (dqb, 0), (dkb, 0), (dvb, 0)
            Delta = torch.empty_like(LSE)
            ops.attn_drop_bwd(p(qt), p(kt), p(vt), O, dO, LSE, Delta, p(dqt), p(dkt), p(dvt), B, H, Nq, Nk, dqk, dv, *strides,
                              Nq * H * dv, H * dv, Nq * H * dv, H * dv, *strides, scale, keep, ld, 1.0 / keep_p,
                              dq_ctx_rows=qo if not f32 else 0)
            if fused:
                gq = dbuf[:, qo:qo + Nq, 0].permute(0, 2, 1, 3); gk = dbuf[:, :, 1].permute(0, 2, 1, 3); gv = dbuf[:, :, 2].permute(0, 2, 1, 3)
                if qo > 0 and not f32:
                    report(tag + f' ctx rows {qo}', float(dbuf[:, :qo, 0].abs().max().nan_to_num(nan=1.0)), 1e-9)
                elif qo > 0:
                    ctx = torch.zeros(B, Nk, 3, dtype=torch.bool, device=dev)
                    ctx[:, :qo, 0] = True
                    kept(tag + f' q slots of the {qo} context rows', dbuf, torch.full_like(buf, fill), ctx)
            else:
                gq, gk, gv = dqb.permute(0, 2, 1, 3), dkb.permute(0, 2, 1, 3), dvb.permute(0, 2, 1, 3)
            report(tag + ' dq', rel(gq, q.grad), tb)
            report(tag + ' dk', rel(gk, k.grad), tb)
            report(tag + ' dv', rel(gv, v.grad), tb)
            elem(tag + ' dq', 'dropout', gq, r64['dq'], r64['bdq'])
            elem(tag + ' dk', 'dropout', gk, r64['dk'], r64['bdk'])
            elem(tag + ' dv', 'dropout', gv, r64['dv'], r64['bdv'])
    # dropout on activations, DropPath folded in
    for (B, rows, D) in [(4, 49, 768), (3, 7, 128), (2, 204, 3072), (1, 1, 4)]:
        g = torch.Generator(device='cpu'); g.manual_seed(7 + rows)
        keep = (torch.rand(B * rows, D, generator=g) < 0.8).to(torch.uint8).to(dev)
        rs = (torch.rand(B, generator=g) < 0.7).float().to(dev) / 0.7
        res = rnd(B * rows, D, seed=3)
        for din in (F32, BF16):
            for dout in (F32, BF16):
                x = rnd(B * rows, D, dtype=din, seed=5)
                for (kp, rsc, rr) in [(keep, None, None), (keep, rs, res), (None, rs, None), (keep, None, res)]:
                    ref = x.float()
                    if kp is not None:
                        ref = ref * kp.float() / 0.8
                    if rsc is not None:
                        ref = (ref.view(B, rows, D) * rsc.view(B, 1, 1)).reshape(B * rows, D)
                    if rr is not None:
                        ref = ref + rr
                    out = kc.poisoned((B * rows, D), dout, dev)
                    ops.dropout_rows(x, kp, 1.0 / 0.8, B, rows, D, out, res=rr, rowscale=rsc)
                    r64 = x.double() * (1.0 if kp is None else kp.double() * float(torch.tensor(1.0 / 0.8)))
                    if rsc is not None:
                        r64 = (r64.view(B, rows, D) * rsc.double().view(B, 1, 1)).reshape(B * rows, D)
                    mag = r64.abs() + (0.0 if rr is None else rr.double().abs())
                    if rr is not None:
                        r64 = r64 + rr.double()
                    elem(f'dropout_rows {B}x{rows}x{D} {str(din)[6:]}->{str(dout)[6:]} keep{kp is not None} rs{rsc is not None} res{rr is not None}',
                         'dropout', out, r64, 4 * kc.U32 * mag + (kc.U16 * r64.abs() if dout == BF16 else 0.0))
                    report(f'dropout_rows {B}x{rows}x{D} {str(din)[6:]}->{str(dout)[6:]} keep{kp is not None} rs{rsc is not None} res{rr is not None}',
                           rel(out, ref.to(dout)), 1e-6 if dout == F32 else 4e-3)
                if din == dout:         # in place
                    y = x.clone()
                    ops.dropout_rows(y, keep, 1.25, B, rows, D, y)
                    report(f'dropout_rows in place {B}x{rows}x{D} {str(din)[6:]}', rel(y, (x.float() * keep.float() * 1.25).to(din)), 1e-6 if din == F32 else 4e-3)


@check
def window_attention():
    """Swin decoder kernels (models/swin.py): attention with the relative-position bias + shift mask on the A x A corner of
    [A window tokens | nF fusion tokens] sequences (bias table per window, b % nb), its dS output and the table gradient
    reduced from it, and the unfold / fold row movers — against plain torch, then elementwise (tests/kcheck.py): every output
    starts poisoned (accumulated ones prefilled), the bf16 kernels and their fp32 twins are held to float64 bounds, the bias
    build and the row copies are bit-exact."""
    LOG2E = 1.4426950408889634
    for (B, nW, H, A, nF, d, masked, pad) in [(2, 4, 2, 16, 9, 32, True, 0), (3, 6, 2, 16, 9, 32, False, 0), (2, 20, 16, 16, 32, 32, True, 0),
                                               (1, 1, 2, 16, 3, 32, False, 0), (2, 4, 2, 16, 16, 64, True, 0),
                                               # 7 x 7 windows (SwinTransformerBlock's default: N = 69 crosses a 64-key tile) and one
                                               # 3 x 3 window (models/swin.py:60-62: a grid no larger than the window), bias_ld > Nk rounded up
                                               (2, 4, 2, 49, 20, 32, True, 32), (3, 1, 2, 9, 5, 32, False, 32),
                                               # the base_swin decoders (image 16 windows, audio 20) at the bench batch
                                               (64, 16, 16, 16, 32, 32, True, 0), (64, 20, 16, 16, 32, 32, False, 0)]:
        N, D = A + nF, H * d
        Nkp = (N + 31) // 32 * 32
        ld = Nkp + pad
        win = int(round(A ** 0.5))
        T = (2 * win - 1) ** 2
        table = rnd(T, H, seed=71, scale=0.7)
        coords = torch.stack(torch.meshgrid(torch.arange(win), torch.arange(win), indexing='ij')).flatten(1)
        relc = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (win - 1)
        index = (relc[..., 0] * (2 * win - 1) + relc[..., 1]).to(dev)
        index32 = index.reshape(-1).to(torch.int32)
        mask = None
        if masked:
            mask = torch.where(rnd(nW, A, A, seed=72) > 0.3, torch.full((nW, A, A), -100.0, device=dev), torch.zeros(nW, A, A, device=dev))
            mask[:, torch.arange(A), torch.arange(A)] = 0.0            # a row never masks itself
        nb = nW if masked else 1
        bias2 = kc.poisoned((nb, H, N, ld), F32, dev)
        ops.relpos_bias_build(table, index32, mask, nb, H, A, N, ld, LOG2E, bias2)
        full = torch.zeros(nb, H, N, N, device=dev)
        corner = table[index.reshape(-1)].view(A, A, H).permute(2, 0, 1)[None] + (mask[:, None] if masked else 0.0)
        full[:, :, :A, :A] = corner
        report(f'relpos_bias_build nW{nW} H{H} N{N}', rel(bias2[..., :N] / LOG2E, full) + (float(bias2[..., N:].abs().max()) if ld > N else 0.0), 1e-6)
        # (table[index] + mask) * mul in fp32 on the corner, +0 everywhere else (padding columns included)
        bias_n = kc.poisoned((nb, H, N, ld), F32, dev)                  # natural units: the fp32 twins' bias
        ops.relpos_bias_build(table, index32, mask, nb, H, A, N, ld, 1.0, bias_n)
        for mul, got in ((LOG2E, bias2), (1.0, bias_n)):
            want = torch.zeros(nb, H, N, ld, device=dev)
            want[:, :, :A, :A] = corner * mul
            same(f'relpos_bias_build nW{nW} H{H} A{A} N{N} ld{ld} mul{mul:.3f}', got, want)
        buf = rnd(B * nW, N, 3, H, d, dtype=BF16, seed=73)
        q = buf[:, :, 0].permute(0, 2, 1, 3).float().requires_grad_(True)
        k = buf[:, :, 1].permute(0, 2, 1, 3).float().requires_grad_(True)
        v = buf[:, :, 2].permute(0, 2, 1, 3).float().requires_grad_(True)
        scale = d ** -0.5
        fullrep = full.repeat(B * nW // nb, 1, 1, 1)
        logits = (q @ k.transpose(-2, -1)) * scale + fullrep
        logits.retain_grad()
        ref = logits.softmax(-1) @ v
        O = kc.poisoned((B * nW * N, D), BF16, dev)
        LSE = kc.poisoned((B * nW, H, N), F32, dev)
        st = (N * 3 * D, 3 * D) * 3
        p0 = buf.data_ptr()
        ops.attn_bias_fwd(p0, p0 + 2 * D, p0 + 4 * D, O, LSE, B * nW, H, N, N, d, d, *st, N * D, D, scale, bias2, nb, ld)
        tag = f'window attn B{B} nW{nW} H{H} A{A} N{N} d{d} mask{int(masked)}'
        report(tag + ' fwd', rel(O.view(B * nW, N, H, d).permute(0, 2, 1, 3), ref), 1e-2)
        report(tag + ' lse', rel(LSE, torch.logsumexp(logits, -1)), 1e-4)
        dO = rnd(B * nW * N, D, dtype=BF16, seed=74)
        dOv = dO.view(B * nW, N, H, d).permute(0, 2, 1, 3)
        ref.backward(dOv.float())
        Ok = O.view(B * nW, N, H, d).permute(0, 2, 1, 3)
        r64 = kc.attn_bounds(q, k, v, dOv, Ok, scale, bias=fullrep)
        elem(tag + ' fwd', 'window_attention', Ok, r64['O'], r64['bO'])
        elem(tag + ' lse', 'window_attention', LSE, r64['lse'], r64['blse'])
        dbuf = kc.poisoned(buf.shape, BF16, dev)
        dS = kc.poisoned((B * nW, H, N, ld), F32, dev)
        Delta = kc.poisoned(LSE.shape, F32, dev)
        d0 = dbuf.data_ptr()
        ops.attn_bias_bwd(p0, p0 + 2 * D, p0 + 4 * D, O, dO, LSE, Delta, d0, d0 + 2 * D, d0 + 4 * D, B * nW, H, N, N, d, d,
                          *st, N * D, D, N * D, D, *st, scale, bias2, nb, ld, dS)
        report(tag + ' dq', rel(dbuf[:, :, 0].permute(0, 2, 1, 3), q.grad), 2e-2)
        report(tag + ' dk', rel(dbuf[:, :, 1].permute(0, 2, 1, 3), k.grad), 2e-2)
        report(tag + ' dv', rel(dbuf[:, :, 2].permute(0, 2, 1, 3), v.grad), 2e-2)
        report(tag + ' dS', rel(dS[..., :N], logits.grad), 2e-2)
        for i, g in enumerate(('dq', 'dk', 'dv')):
            elem(f'{tag} {g}', 'window_attention', dbuf[:, :, i].permute(0, 2, 1, 3), r64[g], r64['b' + g])
        elem(tag + ' dS', 'window_attention', dS[..., :N], r64['dS'], r64['bdS'])
        dO64, Ok64 = dOv.double(), Ok.double()
        delta64 = (dO64 * Ok64).sum(-1)                                  # Delta = dO . O (the kernel's bf16 O): a d-term fp32 sum
        elem(tag + ' Delta', 'window_attention', Delta, delta64, kc.sum_bound((dO64 * Ok64).abs().sum(-1), d, delta64))
        # header contract: dS columns [Nk, Nk rounded up to 32) receive finite values, the columns beyond keep their bits
        nfin = int((~torch.isfinite(dS[..., N:Nkp])).sum())
        report(tag + f' dS columns {N}..{Nkp} finite', float(nfin), 0.0)
        kept(tag + f' dS columns {Nkp}..{ld}', dS[..., Nkp:], kc.poisoned(dS[..., Nkp:].shape, F32, dev))
        want = torch.zeros(T, H, device=dev)
        want.index_add_(0, index.reshape(-1), dS[:, :, :A, :A].sum(0).permute(1, 2, 0).reshape(A * A, H))
        if A * A <= 1024:
            gz = kc.Guarded(T, H, F32, device=dev, fill='zero')
            ops.relpos_bias_bwd(dS, index32, B * nW, H, A, N, ld, T, gz.t)
            report(tag + ' dtable (from the kernel dS)', rel(gz.t, want), 1e-5)
            guard(tag + ' dtable', gz)
            # dtable += ...: into a random prefill; entry e sums B * nW * (pairs of e) terms + the prefill
            pre = kc.prefilled((T, H), F32, dev, seed=78)
            dtab = pre.clone()
            ops.relpos_bias_bwd(dS, index32, B * nW, H, A, N, ld, T, dtab)
            cS = dS[:, :, :A, :A].double()
            want64 = pre.double().index_add(0, index.reshape(-1), cS.sum(0).permute(1, 2, 0).reshape(A * A, H))
            absum = pre.double().abs().index_add(0, index.reshape(-1), cS.abs().sum(0).permute(1, 2, 0).reshape(A * A, H))
            npairs = torch.bincount(index.reshape(-1), minlength=T).double()[:, None]
            elem(tag + ' dtable += (prefilled)', 'relpos_bias_bwd', dtab, want64, kc.sum_bound(absum, B * nW * npairs + 1, want64))
        else:                   # header: A * A <= 1024
            rejected(f'relpos_bias_bwd A{A}', lambda: ops.relpos_bias_bwd(dS, index32, B * nW, H, A, N, ld, T, kc.prefilled((T, H), F32, dev)))
        # ---- the fp32 twins (dav_attn_bias_fwd_f32 / _bwd_f32): fp32 operands of the same values, natural-units bias
        b32 = buf.float()
        p1 = b32.data_ptr()
        O32, LSE32 = kc.poisoned((B * nW * N, D), F32, dev), kc.poisoned((B * nW, H, N), F32, dev)
        ops.attn_bias_fwd(p1, p1 + 4 * D, p1 + 8 * D, O32, LSE32, B * nW, H, N, N, d, d, *st, N * D, D, scale, bias_n, nb, ld)
        O32v = O32.view(B * nW, N, H, d).permute(0, 2, 1, 3)
        dO32 = dO.float()
        up = kc.f32_attn_up(q, k, scale, fullrep)
        r32 = kc.attn_bounds(q, k, v, dOv, O32v, scale, up=up, r_out=kc.out_round(F32), bias=fullrep)
        tag32 = tag + ' fp32'
        elem(tag32 + ' fwd', 'window_attention_f32', O32v, r32['O'], r32['bO'])
        elem(tag32 + ' lse', 'window_attention_f32', LSE32, r32['lse'], r32['blse'])
        dbuf32 = kc.poisoned(b32.shape, F32, dev)
        dS32 = kc.poisoned((B * nW, H, N, ld), F32, dev)
        d1 = dbuf32.data_ptr()
        ops.attn_bias_bwd(p1, p1 + 4 * D, p1 + 8 * D, O32, dO32, LSE32, kc.poisoned(LSE.shape, F32, dev), d1, d1 + 4 * D, d1 + 8 * D,
                          B * nW, H, N, N, d, d, *st, N * D, D, N * D, D, *st, scale, bias_n, nb, ld, dS32)
        for i, g in enumerate(('dq', 'dk', 'dv')):
            elem(f'{tag32} {g}', 'window_attention_f32', dbuf32[:, :, i].permute(0, 2, 1, 3), r32[g], r32['b' + g])
        elem(tag32 + ' dS', 'window_attention_f32', dS32[..., :N], r32['dS'], r32['bdS'])
        kept(tag32 + f' dS columns {N}..{ld}', dS32[..., N:], kc.poisoned(dS32[..., N:].shape, F32, dev))
        del r64, r32, fullrep, logits, ref
        # ---- row movers: [B, nF + L, C] <-> [B * nW, A + nF, C] through a random token permutation
        L, C = nW * A, 96
        rows = torch.randperm(L, generator=torch.Generator().manual_seed(5)).to(dev)
        inv = torch.empty_like(rows); inv[rows] = torch.arange(L, device=dev)
        rows32, inv32 = rows.to(torch.int32), inv.to(torch.int32)
        x = rnd(B, nF + L, C, seed=75)
        seq = kc.poisoned((B * nW * N, C), BF16, dev)
        ops.window_unfold(x, rows32, B, nW, A, nF, L, C, 0.5, seq)
        want = torch.cat([x[:, nF:][:, rows].reshape(B * nW, A, C), (0.5 * x[:, None, :nF]).expand(B, nW, nF, C).reshape(B * nW, nF, C)], 1)
        report(f'window_unfold nW{nW} nF{nF}', rel(seq.view(B * nW, N, C), want), 4e-3)
        fs = 1.0 / nW
        for sdt, odt in ((F32, BF16), (BF16, BF16), (F32, F32), (BF16, F32)):
            src = x.to(sdt)
            name = f'window_unfold nW{nW} A{A} nF{nF} {str(sdt)[6:]}->{str(odt)[6:]}'
            g = kc.Guarded(B * nW * N, C, odt, device=dev)
            if sdt == BF16 and odt == F32:           # header: bf16 -> fp32 is not provided
                rejected(name, lambda: ops.window_unfold(src, rows32, B, nW, A, nF, L, C, fs, g.t))
                continue
            ops.window_unfold(src, rows32, B, nW, A, nF, L, C, fs, g.t)
            o4 = g.t.view(B, nW, N, C)
            same(name + ' token rows', o4[:, :, :A], src[:, nF:][:, rows].reshape(B, nW, A, C).to(odt))
            same(name + ' fusion rows', o4[:, :, A:], (fs * src[:, None, :nF].float()).expand(B, nW, nF, C).to(odt))
            guard(name, g)
        t = rnd(B * nW * N, C, seed=76)
        res = rnd(B, nF + L, C, seed=77)
        out = kc.poisoned((B, nF + L, C), F32, dev)
        ops.window_fold(t, inv32, res, B, nW, A, nF, L, C, 1.0 / nW, out)
        tv = t.view(B, nW, N, C)
        tok = tv[:, :, :A].reshape(B, L, C)[:, inv]
        want = res + torch.cat([tv[:, :, A:].mean(1), tok], 1)
        report(f'window_fold nW{nW} nF{nF}', rel(out, want), 1e-6)
        # token rows: one fp32 add (none without res); fusion rows: res + fs * (sum over the nW windows)
        for with_res in (True, False):
            name = f'window_fold nW{nW} A{A} nF{nF} res{int(with_res)}'
            g = kc.Guarded(B * (nF + L), C, F32, device=dev)
            ops.window_fold(t, inv32, res if with_res else None, B, nW, A, nF, L, C, fs, g.t)
            o3 = g.t.view(B, nF + L, C)
            same(name + ' token rows', o3[:, nF:], res[:, nF:] + tok if with_res else tok)
            r0 = res[:, :nF].double() if with_res else torch.zeros(B, nF, C, dtype=torch.float64, device=dev)
            f64 = r0 + fs * tv[:, :, A:].double().sum(1)
            absum = r0.abs() + fs * tv[:, :, A:].double().abs().sum(1)
            elem(name + ' fusion rows', 'window_fold', o3[:, :nF], f64, kc.sum_bound(absum, nW + 2, f64))
            guard(name, g)


@check
def layernorm():
    for (B, r0, r1, D) in [(3, 4, 9, 128), (2, 0, 81, 768), (64, 32, 49, 768), (2, 0, 228, 512), (3, 5, 0, 192), (2, 3, 3, 1024)]:
        x0 = rnd(B, max(r0, 1), D, seed=31)[:, :r0].contiguous() if r0 else None
        x1 = rnd(B, max(r1, 1), D, seed=32)[:, :r1].contiguous() if r1 else None
        g, bt = rnd(D, seed=33) * 0.1 + 1, rnd(D, seed=34) * 0.1
        xs = [t for t in (x0, x1) if t is not None]
        xc = torch.cat(xs, 1).clone().requires_grad_(True)
        gp, bp = g.clone().requires_grad_(True), bt.clone().requires_grad_(True)
        ref = torch.nn.functional.layer_norm(xc, (D,), gp, bp, 1e-6)
        R = r0 + r1
        y, y32 = kc.poisoned((B * R, D), BF16, dev), kc.poisoned((B * R, D), F32, dev)
        mean, rstd = kc.poisoned((B * R,), F32, dev), kc.poisoned((B * R,), F32, dev)
        a0, a1 = (x0, x1) if x0 is not None else (x1, None)
        n0, n1 = (r0, r1) if x0 is not None else (r1, 0)
        ops.layernorm_fwd(a0, n0 * D, n0, a1, n1 * D, n1, B, D, g, bt, 1e-6, y, y32, mean, rstd)
        tag = f'ln B{B} {r0}+{r1} D{D}'
        report(tag + ' fwd32', rel(y32, ref.view(-1, D)), 1e-5)
        report(tag + ' fwd16', rel(y, ref.view(-1, D)), 5e-3)
        dy = rnd(B * R, D, dtype=BF16, seed=35)
        dy32 = rnd(B * R, D, seed=36)
        ref.backward((dy.float() + dy32).view(B, R, D))
        L = kc.ln_bounds(xc.view(-1, D), g, bt, 1e-6, dy.double() + dy32.double())
        elem(tag + ' fwd32', 'layernorm', y32, L['y'], L['by'] + kc.out_round(F32) * L['y'].abs())
        elem(tag + ' fwd16', 'layernorm', y, L['y'], L['by'] + kc.U16 * L['y'].abs())
        elem(tag + ' mean', 'layernorm', mean, L['mean'], kc.C_LN * kc.U32 * xc.view(-1, D).double().abs().mean(-1))
        elem(tag + ' rstd', 'layernorm', rstd, L['rstd'], kc.C_LN * kc.U32 * L['rstd'])
        P0 = kc.prefilled((B, n0, D), F32, dev, seed=38)
        dx0 = P0.clone()
        res0 = rnd(B, n0, D, seed=37)
        tw0 = kc.poisoned((B, n0, D), BF16, dev)
        dx1 = kc.poisoned((B, n1, D), F32, dev) if n1 else None
        pg, pb = kc.prefilled((D,), F32, dev, seed=39), kc.prefilled((D,), F32, dev, seed=40)
        dg, db = pg.clone(), pb.clone()
        ops.layernorm_bwd(a0, n0 * D, n0, a1, n1 * D, n1, B, D, dy, dy32, g, mean, rstd,
                          dx0, n0 * D, 1, res0, n0 * D, tw0, n0 * D, dx1, n1 * D, 0, None, 0, None, 0, dg, db)
        report(tag + ' dx0(acc+res)', rel(dx0, xc.grad[:, :n0] + P0 + res0), 1e-4)
        report(tag + ' dx0 twin', rel(tw0, xc.grad[:, :n0] + P0 + res0), 5e-3)
        if n1:
            report(tag + ' dx1', rel(dx1, xc.grad[:, n0:]), 1e-4)
        report(tag + ' dgamma', rel(dg, pg + gp.grad), 1e-4)
        report(tag + ' dbeta', rel(db, pb + bp.grad), 1e-4)
        dx64, bdx = L['dx'].view(B, R, D), L['bdx'].view(B, R, D)
        acc64 = dx64[:, :n0] + P0.double() + res0.double()
        bacc = bdx[:, :n0] + kc.out_round(F32) * (dx64[:, :n0].abs() + P0.double().abs() + res0.double().abs())
        elem(tag + ' dx0(acc+res)', 'layernorm', dx0, acc64, bacc)
        elem(tag + ' dx0 twin', 'layernorm', tw0, acc64, bacc + kc.U16 * acc64.abs())
        if n1:
            elem(tag + ' dx1', 'layernorm', dx1, dx64[:, n0:], bdx[:, n0:] + kc.out_round(F32) * dx64[:, n0:].abs())
        elem(tag + ' dgamma', 'layernorm', dg, pg.double() + L['dgamma'], L['bdgamma'] + kc.out_round(F32) * (pg.double().abs() + L['dgamma'].abs()))
        elem(tag + ' dbeta', 'layernorm', db, pb.double() + L['dbeta'], L['bdbeta'] + kc.out_round(F32) * (pb.double().abs() + L['dbeta'].abs()))
        # the same backward with the statistics deferred (dav_layernorm_bwd_reduce_grouped): into other random prefills
        pg2, pb2 = kc.prefilled((D,), F32, dev, seed=41), kc.prefilled((D,), F32, dev, seed=42)
        dg2, db2 = pg2.clone(), pb2.clone()
        defer = []
        ops.layernorm_bwd(a0, n0 * D, n0, a1, n1 * D, n1, B, D, dy, dy32, g, mean, rstd,
                          dx0=kc.poisoned((B, n0, D), F32, dev), dx0_bs=n0 * D, dgamma=dg2, dbeta=db2, defer=defer)
        ops.layernorm_bwd_reduce_grouped(defer)
        elem(tag + ' deferred dgamma', 'layernorm', dg2, pg2.double() + L['dgamma'], L['bdgamma'] + kc.out_round(F32) * (pg2.double().abs() + L['dgamma'].abs()))
        elem(tag + ' deferred dbeta', 'layernorm', db2, pb2.double() + L['dbeta'], L['bdbeta'] + kc.out_round(F32) * (pb2.double().abs() + L['dbeta'].abs()))


def _slot_stats(x):
    """[rows, D] fp32 -> [rows, D/64, 2] {sum, sum of squares} per 64-column slot (float64 reference)"""
    r, D = x.shape
    v = x.double().view(r, D // 64, 64)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1)


@check
def ln_fused():
    """LayerNorm folded into the GEMMs either side of it (dav_gemm_nt_ln_bf16, dav_ln_fold_grouped, dav_rowstats_cast,
    dav_layernorm_bwd_twin) against torch fp32 / fp64 on the same operands."""
    ln = torch.nn.functional.layer_norm
    # 1. stand-alone row statistics + twin (incl. a broadcast source: batch stride 0)
    for (B, rows, D, bs) in [(3, 7, 128, None), (2, 81, 768, None), (4, 16, 512, 0), (2, 5, 1024, None), (64, 49, 768, None)]:
        x = rnd(B if bs is None else 1, rows, D, seed=41) + 0.3
        tw = kc.poisoned((B * rows, D), BF16, dev)
        st = kc.poisoned((B * rows, D // 64, 2), F32, dev)
        ops.rowstats_cast(x, rows * D if bs is None else 0, B, rows, D, tw, st)
        xe = x.expand(B, rows, D).reshape(B * rows, D)
        report(f'rowstats B{B} r{rows} D{D} twin', float((tw.float() - xe.to(BF16).float()).abs().max()), 0.0)
        report(f'rowstats B{B} r{rows} D{D} sums', rel(st, _slot_stats(xe)), 2e-6)
    # 2. weight fold
    items, refs = [], []
    for (N, K, has_b) in [(2304, 768, True), (1536, 512, True), (96, 64, False), (3072, 1024, True), (40, 192, True)]:
        w = rnd(N, K, scale=0.05, seed=42)
        g, bt = rnd(K, seed=43) * 0.2 + 1, rnd(K, seed=44) * 0.2
        bias = rnd(N, seed=45) if has_b else None
        wl, c, d = kc.poisoned((N, K), BF16, dev), kc.poisoned((N,), F32, dev), kc.poisoned((N,), F32, dev)
        items.append((w, g, bt, bias, wl, c, d))
        wl_ref = (w * g).to(BF16)
        refs.append((wl_ref, wl_ref.double().sum(1), (w.double() * bt.double()).sum(1) + (bias.double() if has_b else 0)))
    ops.ln_fold_grouped(items)
    for (w, g, bt, bias, wl, c, d), (wl_ref, c_ref, d_ref) in zip(items, refs):
        tag = f'ln_fold {w.shape[0]}x{w.shape[1]}'
        report(tag + ' w_ln', float((wl.float() - wl_ref.float()).abs().max()), 0.0)
        report(tag + ' c', rel(c, c_ref), 2e-6)
        report(tag + ' d', rel(d, d_ref), 2e-6)
    # 3. producer side: statistics partials + twin of the fp32 result, through row maps, in every tile configuration that has them
    for (M, N, K, cfg, cmap) in [(3136, 768, 768, 0, None), (3136, 768, 768, 3, None), (1024, 768, 3072, 8, None), (130, 512, 512, 7, None),
                                 (260, 512, 2048, 5, None), (22528, 512, 2048, 0, None), (64 * 8, 768, 768, 0, (8, 16, 4)), (200, 192, 192, 0, None),
                                 (4096, 1024, 1024, 3, None)]:
        A, Bm = rnd(M, K, dtype=BF16, seed=46), rnd(N, K, dtype=BF16, scale=0.05, seed=47)
        bias = rnd(N, seed=48)
        rows_out = M if cmap is None else (M // cmap[0]) * cmap[1]
        res = rnd(rows_out, N, seed=49)
        C = torch.zeros(rows_out, N, device=dev)
        tw = torch.zeros(rows_out, N, device=dev, dtype=BF16)
        st = torch.zeros(rows_out, N // 64, 2, device=dev)
        ops.gemm_nt_ln(A, Bm, M, N, K, prod=dict(stats_out=st, twin_out=tw, ld_twin=N), bias=bias, res=res, ldres=N, res_rowmap=cmap,
                       C_out=C, c_rowmap=cmap, variant=cfg << 4)
        ref = A.float() @ Bm.float().t() + bias
        if cmap is None:
            want = ref + res
            got, gtw, gst = C, tw, st
        else:
            rpb, bs_, off = cmap
            idx = (torch.arange(M, device=dev) // rpb) * bs_ + off + torch.arange(M, device=dev) % rpb
            want = ref + res[idx]
            got, gtw, gst = C[idx], tw[idx], st[idx]
        tag = f'nt_ln producer {M}x{N}x{K} cfg{cfg}{" rowmap" if cmap else ""}'
        report(tag + ' C', rel(got, want), 1e-4)
        report(tag + ' twin', float((gtw.float() - got.to(BF16).float()).abs().max()), 0.0)
        report(tag + ' sums', rel(gst, _slot_stats(got)), 5e-6)
    # 4. consumer side: raw twin + partials + folded weight == LayerNorm -> Linear
    for (B, r0, r1, D, N, cfg, act, c_bf16) in [(64, 16, 49, 768, 2304, 0, 0, True), (64, 0, 49, 768, 3072, 0, 1, True), (8, 0, 352, 512, 1536, 44, 0, True),
                                                (8, 0, 352, 512, 2048, 44, 1, True), (4, 0, 320, 512, 256, 0, 0, False), (2, 5, 12, 192, 576, 0, 0, True),
                                                (64, 0, 49, 768, 1536, 45, 0, True), (3, 0, 50, 1024, 3072, 3, 0, True), (16, 16, 64, 768, 2304, 8, 0, True),
                                                (2, 0, 33, 128, 64, 7, 0, False)]:
        R = r0 + r1
        M = B * R
        eps = 1e-6 if D != 512 else 1e-5
        x0 = (rnd(B, max(r0, 1), D, seed=51) * 1.3 + 0.2)[:, :r0].contiguous() if r0 else None
        x1 = (rnd(B, r1, D, seed=52) * 0.7 - 0.1)
        w32 = rnd(N, D, scale=0.05, seed=53)            # fp32 master; the un-fused path contracts with its bf16 mirror
        w = w32.to(BF16)
        g, bt, bias = rnd(D, seed=54) * 0.2 + 1, rnd(D, seed=55) * 0.2, rnd(N, seed=56)
        wl, c, d = torch.empty_like(w), kc.poisoned((N,), F32, dev), kc.poisoned((N,), F32, dev)
        ops.ln_fold_grouped([(w32, g, bt, bias, wl, c, d)])
        segs = []
        for xs, r in ((x0, r0), (x1, r1)):
            if xs is None:
                continue
            tw = kc.poisoned((B * r, D), BF16, dev)
            st = kc.poisoned((B * r, D // 64, 2), F32, dev)
            ops.rowstats_cast(xs, r * D, B, r, D, tw, st)
            segs.append((tw, st, r))
        xc = torch.cat([t for t in (x0, x1) if t is not None], 1)
        h = ln(xc, (D,), g, bt, eps).view(M, D)
        ref = h @ w32.t() + bias
        pre = ref
        if act == 1:
            ref = torch.nn.functional.gelu(ref)
        out = kc.poisoned((M, N), BF16 if c_bf16 else F32, dev)
        Z = kc.poisoned((M, N), BF16, dev) if act == 1 else None
        lnd = dict(stats=segs[0][1], ln_c=c, eps=eps)
        if len(segs) == 2:
            lnd.update(A2=segs[1][0], stats2=segs[1][1], a_r0=r0, a_r1=r1)
        ops.gemm_nt_ln(segs[0][0], wl, M, N, D, ln=lnd, bias=d, act=act, C_out=out, c_bf16=c_bf16, C2=Z, ldc2=N, c2_mode=4 if act == 1 else 0,
                       variant=cfg << 4)
        tag = f'nt_ln consumer B{B} {r0}+{r1} D{D} N{N} cfg{cfg} act{act}'
        report(tag, rel(out, ref), 6e-3)
        if Z is not None:
            xg = pre.clone().requires_grad_(True)
            torch.nn.functional.gelu(xg).sum().backward()
            report(tag + " gelu'twin", float((Z.float() - xg.grad).abs().max()), 2e-2)
        # against the un-fused product path on the same operands (LayerNorm kernel -> bf16 -> GEMM): both are bf16-operand results
        y = kc.poisoned((M, D), BF16, dev)
        mean, rstd = kc.poisoned((M,), F32, dev), kc.poisoned((M,), F32, dev)
        a0, a1 = (x0, x1) if x0 is not None else (x1, None)
        n0, n1 = (r0, r1) if x0 is not None else (r1, 0)
        ops.layernorm_fwd(a0, n0 * D, n0, a1, n1 * D if a1 is not None else 0, n1, B, D, g, bt, eps, y, None, mean, rstd)
        out2 = kc.poisoned((M, N), F32, dev)
        ops.gemm_nt(y, w, M, N, D, bias=bias, act=act, C_out=out2)
        report(tag + ' vs unfused (fp32 ref distance ratio)', rel(out, ref) / max(rel(out2, ref), 1e-9), 2.0)
    # 4b. consumer through a row map (the decoder head reads x[:, nF:])
    B, nF, L, D, N = 4, 8, 96, 512, 256
    x = rnd(B, nF + L, D, seed=57)
    tw, st = kc.poisoned((B * (nF + L), D), BF16, dev), kc.poisoned((B * (nF + L), D // 64, 2), F32, dev)
    ops.rowstats_cast(x, (nF + L) * D, B, nF + L, D, tw, st)
    w = rnd(N, D, scale=0.05, seed=58)
    g, bt, bias = rnd(D, seed=59) * 0.2 + 1, rnd(D, seed=60) * 0.2, rnd(N, seed=61)
    wl, c, d = kc.poisoned((N, D), BF16, dev), kc.poisoned((N,), F32, dev), kc.poisoned((N,), F32, dev)
    ops.ln_fold_grouped([(w, g, bt, bias, wl, c, d)])
    out = kc.poisoned((B * L, N), F32, dev)
    ops.gemm_nt_ln(tw, wl, B * L, N, D, ln=dict(stats=st, ln_c=c, eps=1e-5), a_rowmap=(L, nF + L, nF), bias=d, C_out=out)
    ref = ln(x[:, nF:], (D,), g, bt, 1e-5).reshape(B * L, D) @ w.t() + bias
    report('nt_ln consumer rowmap', rel(out, ref), 6e-3)
    # 5. backward from the twin: exact against autograd ON THE TWIN'S VALUES, h_out = the LayerNorm output
    for (B, r0, r1, D) in [(3, 4, 9, 128), (2, 0, 81, 768), (64, 16, 49, 768), (2, 0, 228, 512), (2, 3, 3, 1024)]:
        R = r0 + r1
        eps = 1e-6
        xs = [(rnd(B, r, D, seed=62 + i) * (1 + i) + 0.1 * i) for i, r in enumerate((r0, r1)) if r]
        twins = []
        for xx in xs:
            r = xx.shape[1]
            tw, st = kc.poisoned((B * r, D), BF16, dev), kc.poisoned((B * r, D // 64, 2), F32, dev)
            ops.rowstats_cast(xx, r * D, B, r, D, tw, st)
            twins.append((tw, st, r))
        g, bt = rnd(D, seed=33) * 0.1 + 1, rnd(D, seed=34) * 0.1
        xc = torch.cat([tw.float().view(B, r, D) for (tw, st, r) in twins], 1).clone().requires_grad_(True)
        gp, bp = g.clone().requires_grad_(True), bt.clone().requires_grad_(True)
        ref = ln(xc, (D,), gp, bp, eps)
        dy, dy32 = rnd(B * R, D, dtype=BF16, seed=35), rnd(B * R, D, seed=36)
        ref.backward((dy.float() + dy32).view(B, R, D))
        (t0, s0, n0) = twins[0]
        (t1, s1, n1) = twins[1] if len(twins) == 2 else (None, None, 0)
        dx0 = torch.full((B, n0, D), 1.0, device=dev)
        res0 = rnd(B, n0, D, seed=37)
        tw0 = kc.poisoned((B, n0, D), BF16, dev)
        dx1 = kc.poisoned((B, max(n1, 1), D), F32, dev)[:, :n1].contiguous() if n1 else None
        dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        h = kc.poisoned((B * R, D), BF16, dev)
        ops.layernorm_bwd_twin(t0, n0 * D, s0, n0, t1, n1 * D, s1, n1, B, D, eps, dy, dy32, g, bt,
                               dx0, n0 * D, 1, res0, n0 * D, tw0, n0 * D, dx1, n1 * D, 0, None, 0, None, 0, h_out=h, dgamma=dg, dbeta=db)
        tag = f'ln_bwd_twin B{B} {r0}+{r1} D{D}'
        # (the statistics are those of the fp32 rows, x itself their bf16 rounding: mean / rstd differ from the twin's own by ~1e-3 relative)
        report(tag + ' dx0(acc+res)', rel(dx0, xc.grad[:, :n0] + 1.0 + res0), 3e-3)
        report(tag + ' dx0 twin', rel(tw0, xc.grad[:, :n0] + 1.0 + res0), 6e-3)
        if n1:
            report(tag + ' dx1', rel(dx1, xc.grad[:, n0:]), 3e-3)
        report(tag + ' dgamma', rel(dg, gp.grad), 3e-3)
        report(tag + ' dbeta', rel(db, bp.grad), 1e-4)
        report(tag + ' h_out', rel(h, ref.detach().view(-1, D)), 6e-3)


@check
def masking():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'masking.npz'))
    for t in sorted({k.split('.')[0] for k in g.files}):
        noise = torch.from_numpy(g[f'{t}.noise']).to(dev)
        lk = g[f'{t}.ids_keep'].shape[1]
        ik, mask, ir, ik32, ir32 = ops.mask_build(noise, lk)
        ok = (np.array_equal(ik.cpu().numpy(), g[f'{t}.ids_keep']) and np.array_equal(ir.cpu().numpy(), g[f'{t}.ids_restore'])
              and np.array_equal(mask.cpu().numpy(), g[f'{t}.mask']) and np.array_equal(ik32.cpu().numpy(), g[f'{t}.ids_keep'])
              and np.array_equal(ir32.cpu().numpy(), g[f'{t}.ids_restore']))
        report(f'mask_build {t} bit-exact', 0.0 if ok else 1.0, 0.0)
    noise = torch.rand(64, 320, device=dev)
    ik, mask, ir, _, _ = ops.mask_build(noise, 63)
    sh = torch.argsort(noise, dim=1)
    ok = torch.equal(ik, sh[:, :63]) and torch.equal(ir, torch.argsort(sh, dim=1))
    report('mask_build vs torch.argsort 64x320', 0.0 if ok else 1.0, 0.0)


def base_shapes():
    """The bench workload's shapes (config 'base' at bench.py's batch of 64 pairs): per modality (C, H, W, patches, kept), the
    decoder width, the fusion rows and the factorised (v, a) pairs (nv, na, pair widths: key Da and value D)."""
    from deepavfusion_amd.configs import CONFIGS
    c = CONFIGS['base']
    mods = []
    for C, (H, W), ratio in ((3, c.image_size, c.image_mask_ratio), (1, c.audio_size, c.audio_mask_ratio)):
        L = (H // c.patch) * (W // c.patch)
        mods.append((C, H, W, L, int(L * (1 - ratio))))          # len_keep of models/avmae.py:132
    return dict(B=64, mods=mods, D=c.decoder_dim, nF=sum(c.fusion_tkns), nv=c.fusion_tkns[1], na=c.fusion_tkns[2],
                widths=(int(c.embed_dim * c.fusion_attn_ratio), c.embed_dim))


def _row_movers(B, C, H, W, nk, D, nF, tag, seed):
    """patch_gather (+ its fp32 twin), unshuffle_fwd, rows_gather_cast (+ fp32 twin), unshuffle_bwd_reduce at one shape: copies and
    single roundings bit-exact, every output guarded, the accumulated ones prefilled"""
    L = (H // 16) * (W // 16)
    gen = torch.Generator().manual_seed(seed)
    img = rnd(B, C, H, W, seed=seed)
    ids = torch.stack([torch.randperm(L, generator=gen)[:nk] for _ in range(B)]).to(dev).to(torch.int32)
    cols = img.reshape(B, C, H // 16, 16, W // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, L, C * 256)
    kept_cols = cols.gather(1, ids.long().unsqueeze(-1).expand(-1, -1, C * 256)).reshape(B * nk, -1)
    for sel, n, want in ((ids, nk, kept_cols), (None, L, cols.reshape(B * L, -1))):
        name = f'patch_gather {"kept" if sel is not None else "all"} {tag}'
        for dt in (BF16, F32):
            g = kc.Guarded(B * n, C * 256, dt, device=dev)
            ops.patch_gather(img, sel, n, g.t)
            nm = name + (' fp32' if dt == F32 else '')
            if dt == BF16:
                report(nm, rel(g.t, want), 4e-3)
            same(nm, g.t, want.to(dt))
            guard(nm, g)
    # un-shuffle: out[b, nF + r] = (kept ? emb : mask_token) + pos[r] — one fp32 add; the nF leading rows are not the kernel's
    emb, mt, pos = rnd(B * nk, D, seed=seed + 1), rnd(D, seed=seed + 2), rnd(L, D, seed=seed + 3)
    restore = torch.stack([torch.randperm(L, generator=gen) for _ in range(B)]).to(dev)
    r32 = restore.to(torch.int32)
    g = kc.Guarded(B * (nF + L), D, F32, device=dev)
    before = g.t.clone()
    out = g.t.view(B, nF + L, D)
    ops.unshuffle_fwd(emb, mt, pos, r32, B, L, nk, D, out, (nF + L) * D, nF)
    full = torch.cat([emb.view(B, nk, D), mt.view(1, 1, D).expand(B, L - nk, D)], 1)
    want = full.gather(1, restore.unsqueeze(-1).expand(-1, -1, D)) + pos
    report(f'unshuffle_fwd {tag}', rel(out[:, nF:], want), 1e-6)
    same(f'unshuffle_fwd {tag}', out[:, nF:], want)
    lead = torch.zeros(B, nF + L, dtype=torch.bool, device=dev)
    lead[:, :nF] = True
    kept(f'unshuffle_fwd {tag} the {nF} leading rows', g.t, before, lead.view(-1))
    guard(f'unshuffle_fwd {tag}', g)
    gx = rnd(B, nF + L, D, seed=seed + 4)
    keep = torch.argsort(restore, dim=1)[:, :nk].to(torch.int32)
    for sel, n, want in ((keep, nk, gx[:, nF:].gather(1, keep.long().unsqueeze(-1).expand(-1, -1, D))), (None, L, gx[:, nF:])):
        name = f'rows_gather_cast {"ids" if sel is not None else "row_off"} {tag}'
        for dt in (BF16, F32):
            g = kc.Guarded(B * n, D, dt, device=dev)
            ops.rows_gather_cast(gx, (nF + L) * D, nF, sel, B, n, D, g.t)
            nm = name + (' fp32' if dt == F32 else '')
            if dt == BF16:
                report(nm, rel(g.t.view(B, n, D), want), 4e-3)
            same(nm, g.t.view(B, n, D), want.to(dt))
            guard(nm, g)
    # dpos += sum over b (B terms), dmask_token += sum over the masked (b, r) (B L terms, atomics) — into zeros, then random prefills
    gp, gm = kc.Guarded(L, D, F32, device=dev, fill='zero'), kc.Guarded(1, D, F32, device=dev, fill='zero')
    ops.unshuffle_bwd_reduce(gx, (nF + L) * D, nF, r32, B, L, nk, D, gp.t, gm.t)
    msk = (restore >= nk).float().unsqueeze(-1)
    report(f'unshuffle dpos {tag}', rel(gp.t, gx[:, nF:].sum(0)), 1e-5)
    report(f'unshuffle dmask_token {tag}', rel(gm.t[0], (gx[:, nF:] * msk).sum((0, 1))), 1e-5)
    pp, pm = kc.prefilled((L, D), F32, dev, seed=seed + 5), kc.prefilled((1, D), F32, dev, seed=seed + 6)
    gp.set(pp)
    gm.set(pm)
    ops.unshuffle_bwd_reduce(gx, (nF + L) * D, nF, r32, B, L, nk, D, gp.t, gm.t)
    g64, m64 = gx[:, nF:].double(), msk.double()
    wp = pp.double() + g64.sum(0)
    elem(f'unshuffle dpos += (prefilled) {tag}', 'unshuffle_bwd', gp.t, wp, kc.sum_bound(pp.double().abs() + g64.abs().sum(0), B + 1, wp))
    wm = pm.double() + (g64 * m64).sum((0, 1))
    elem(f'unshuffle dmask_token += (prefilled) {tag}', 'unshuffle_bwd', gm.t, wm,
         kc.sum_bound(pm.double().abs() + (g64 * m64).abs().sum((0, 1)), B * L + 1, wm))
    guard(f'unshuffle dpos {tag}', gp)
    guard(f'unshuffle dmask_token {tag}', gm)


def _patch_loss(B, C, H, W, tag, seed, edges=False):
    """dav_patch_mse_fwd / _bwd / _bwd_f32 against the oracle (rel, as before) and elementwise against kcheck.mse_bounds.
    edges: a constant patch (variance 0: rstd = 1 / sqrt(1e-6)), a row with mask 0 and a batch element with every patch masked."""
    from oracle import avmae_oracle as O
    L, P = (H // 16) * (W // 16), 256 * C
    im = rnd(B, C, H, W, seed=seed)
    pred = rnd(B, L, P, seed=seed + 1)
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(seed)) > 0.3).float().to(dev)
    if edges:
        im[0, :, :16, :16] = 0.3
        mask[0, 0], mask[0, 1], mask[B - 1] = 1.0, 0.0, 1.0
    gsc = torch.tensor(0.7, device=dev)
    for norm in (True, False):
        t = f'{tag} norm{int(norm)}'
        pr = pred.clone().requires_grad_(True)
        ref = O.forward_loss(O.patchify(im, (16, 16)), pr, mask, norm)
        (ref * gsc).backward()
        lp, tm, tr = (kc.poisoned((B * L,), F32, dev) for _ in range(3))
        loss, ms = kc.poisoned((1,), F32, dev), kc.poisoned((1,), F32, dev)
        ops.patch_mse_fwd(im, pred, mask, norm, lp, tm, tr, loss, ms)
        report(f'patch_mse fwd {t}', abs(float(loss) - float(ref)) / abs(float(ref)), 1e-5)
        M = kc.mse_bounds(im, pred, mask, norm)
        for nm, got in (('loss_patch', lp), ('tmean', tm), ('trstd', tr)):
            elem(f'patch_mse {nm} {t}', 'patch_mse', got.view(B, L), M[nm], M['b' + nm])
        elem(f'patch_mse loss {t}', 'patch_mse', loss[0], M['loss'], M['bloss'])
        same(f'patch_mse mask_sum {t}', ms, mask.sum().view(1))
        for dt in (BF16, F32):
            nm = f'patch_mse bwd {t}' + (' fp32' if dt == F32 else '')
            g = kc.Guarded(B * L, P, dt, device=dev)
            ops.patch_mse_bwd(im, pred, mask, tm, tr, ms, gsc, g.t)
            if dt == BF16:
                report(nm, rel(g.t.view(B, L, P), pr.grad), 5e-3)
            want, bnd = kc.mse_grad(im, pred, mask, tm, tr, ms, gsc, dt)
            elem(nm, 'patch_mse', g.t.view(B, L, P), want, bnd)          # masked-out rows: bound 0, exactly 0
            guard(nm, g)


def _pairs(B, nv, na, Wd, tag, seed):
    """pair_expand (one fp32 add + a rounding: bit-exact) and pair_reduce (na- / nv-term sums), bf16 kernels and fp32 twins"""
    Pv, Pa = rnd(B * nv, Wd, seed=seed), rnd(B * na, Wd, seed=seed + 1)
    ref = (Pv.view(B, nv, 1, Wd) + Pa.view(B, 1, na, Wd)).reshape(-1, Wd)
    for dt in (BF16, F32):
        nm = f'pair_expand {tag}' + (' fp32' if dt == F32 else '')
        g = kc.Guarded(B * nv * na, Wd, dt, device=dev)
        ops.pair_expand(Pv, Pa, B, nv, na, Wd, g.t)
        if dt == BF16:
            report(nm, rel(g.t, ref), 4e-3)
        same(nm, g.t, ref.to(dt))
        guard(nm, g)
    d = rnd(B * nv * na, Wd, dtype=BF16, seed=seed + 2)
    d4 = d.double().view(B, nv, na, Wd)
    wv, wa = d4.sum(2).reshape(-1, Wd), d4.sum(1).reshape(-1, Wd)
    for dt in (BF16, F32):
        nm = f'pair_reduce {tag}' + (' fp32' if dt == F32 else '')
        gv, ga = kc.Guarded(B * nv, Wd, dt, device=dev), kc.Guarded(B * na, Wd, dt, device=dev)
        ops.pair_reduce(d.to(dt), B, nv, na, Wd, gv.t, ga.t)
        if dt == BF16:
            report(nm + ' v', rel(gv.t, wv), 4e-3)
            report(nm + ' a', rel(ga.t, wa), 4e-3)
        elem(nm + ' v', 'pair_reduce', gv.t, wv, kc.sum_bound(d4.abs().sum(2).reshape(-1, Wd), na, wv, dt))
        elem(nm + ' a', 'pair_reduce', ga.t, wa, kc.sum_bound(d4.abs().sum(1).reshape(-1, Wd), nv, wa, dt))
        guard(nm + ' v', gv)
        guard(nm + ' a', ga)


def drnd(n, seed, scale=1.0):
    """n fp32 normals drawn ON the device (the long buffers of the grid-cap cases)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, device=dev, generator=g) * scale


def _drop_path_rows(Bq, rq, Dq, seed):
    """dav_rows_axpy (per element against float64: the multiply-add may be contracted, so it is not bit-exact; out of place and in
    place over y) and dav_rows_scale_cast (one product, one rounding: bit-exact, guarded) with zeros among the per-sample scales"""
    tag = f'B{Bq} rows{rq} D{Dq}'
    R = Bq * rq
    res, yb = rnd(R, Dq, seed=seed), rnd(R, Dq, seed=seed + 1)
    sc = torch.tensor([0.0 if b % 3 == 0 else 1.25 for b in range(Bq)], device=dev)
    srow = sc.repeat_interleave(rq)[:, None]
    res0, y0, sc0 = res.clone(), yb.clone(), sc.clone()
    ref = res.double() + srow.double() * yb.double()
    bound = kc.rows_axpy_bound(res, yb, srow, ref)
    g = kc.Guarded(R, Dq, F32, device=dev)
    ops.rows_axpy(res, yb, sc, Bq, rq, Dq, g.t)
    report(f'rows_axpy {tag}', rel(g.t, res + yb * srow), 1e-6)
    elem(f'rows_axpy {tag}', 'rows_axpy', g.t, ref, bound)
    guard(f'rows_axpy {tag}', g)
    kept(f'rows_axpy {tag} res, y, scale', torch.cat([res.flatten(), yb.flatten(), sc]), torch.cat([res0.flatten(), y0.flatten(), sc0]))
    gy = kc.Guarded(R, Dq, F32, device=dev, fill=yb)
    ops.rows_axpy(res, gy.t, sc, Bq, rq, Dq, gy.t)                   # in place over y
    report(f'rows_axpy in place {tag}', rel(gy.t, res + yb * srow), 1e-6)
    elem(f'rows_axpy in place {tag}', 'rows_axpy', gy.t, ref, bound)
    guard(f'rows_axpy in place {tag}', gy)
    kept(f'rows_axpy in place {tag} res', res, res0)
    # backward: the rows of a dropped sample are 0 x g.  IEEE 754 gives a product the xor of its factors' signs, so a negative g
    # there yields -0 in the kernel AND in torch's (g * s).to(bf16): the reference is torch's own result, compared bit for bit
    # (kc.exact counts a -0 against a +0 as a difference: tests/test_kcheck.py), not a +0 fill.  The -0 feeds a GEMM: harmless.
    gq = rnd(R, Dq, seed=seed + 2)
    gq[:rq] = -gq[:rq].abs()                                        # sample 0 is dropped (scale 0): all negative
    want = (gq * srow).to(BF16)
    go = kc.Guarded(R, Dq, BF16, device=dev)
    ops.rows_scale_cast(gq, sc, Bq, rq, Dq, go.t)
    report(f'rows_scale_cast exact {tag}', float((go.t != want).sum()), 0.0)
    same(f'rows_scale_cast {tag}', go.t, want)
    report(f'rows_scale_cast {tag} dropped rows are zeros', float(go.t[:rq].float().abs().max()), 0.0)
    guard(f'rows_scale_cast {tag}', go)


@check
def misc_kernels():
    # row movers, loss and pairs: a toy shape, then the bench workload's
    _row_movers(3, 3, 64, 96, 5, 64, 3, 'B3 3x64x96', seed=41)
    for C in (3, 1):
        _patch_loss(3, C, 64, 96, f'C{C} B3 64x96', seed=46)
    _pairs(3, 3, 2, 64, 'B3 3x2x64', seed=48)
    S = base_shapes()
    for (C, H, W, L, nk) in S['mods']:
        _row_movers(S['B'], C, H, W, nk, S['D'], S['nF'], f'B{S["B"]} {C}x{H}x{W} keep {nk}/{L}', seed=141)
        _patch_loss(S['B'], C, H, W, f'C{C} B{S["B"]} {H}x{W}', seed=146, edges=True)
    for Wd in S['widths']:
        _pairs(S['B'], S['nv'], S['na'], Wd, f'B{S["B"]} {S["nv"]}x{S["na"]}x{Wd}', seed=148)
    # DropPath row kernels: the toy shape, one float4 per row, four trips of the column loop with a ragged last one (D = 772),
    # and more rows than the grid has waves (9000 > 8192: the row-stride loop)
    for i, (Bq, rq, Dq) in enumerate([(5, 7, 192), (3, 2, 4), (2, 3, 772), (9, 1000, 8)]):
        _drop_path_rows(Bq, rq, Dq, seed=61 + 10 * i)
    # casts: n < 4 (the tail kernel alone), a ragged tail behind the float4 part, and one trip more than the grid cap of
    # 8192 x 256 float4 covers; every output guarded, bit-exact round-to-nearest-even
    x = rnd(1000, 77, seed=51)
    y = kc.poisoned((1000, 77), BF16, dev)
    ops.cast_bf16(x, y)
    report('cast_bf16 exact', float((y != x.to(BF16)).sum()), 0.0)
    for n in (1, 2, 3, 5, 77003, 8192 * 1024 + 1027):
        xs = drnd(n, seed=300 + n % 97)
        before = xs.clone()
        g = kc.Guarded(1, n, BF16, device=dev)
        ops.cast_bf16(xs, g.t)
        same(f'cast_bf16 n={n}', g.t.view(-1), xs.to(BF16))
        guard(f'cast_bf16 n={n}', g)
        kept(f'cast_bf16 n={n} input', xs, before)
    for shape in [(64, 16, 768), (3, 5, 128), (1, 4)]:
        a, b = rnd(*shape, seed=91), rnd(*shape, seed=92)
        o32, ob = ops.add_cast(a, b)
        report(f'add_cast {shape}', float((o32 != a + b).sum()) + float((ob != (a + b).to(BF16)).sum()), 0.0)
    for n in (4, 8192 * 1024 + 1028):                              # (ops.add_cast allocates its outputs: the C ABI directly, into guards)
        a, b = drnd(n, seed=93), drnd(n, seed=94)
        g32, gb = kc.Guarded(1, n, F32, device=dev), kc.Guarded(1, n, BF16, device=dev)
        ops._lib.check(ops._lib.load().dav_add_cast(a.data_ptr(), b.data_ptr(), g32.ptr(), gb.ptr(), n, ops._stream()), 'dav_add_cast')
        same(f'add_cast n={n} fp32', g32.t.view(-1), a + b)
        same(f'add_cast n={n} bf16', gb.t.view(-1), (a + b).to(BF16))
        guard(f'add_cast n={n} fp32', g32)
        guard(f'add_cast n={n} bf16', gb)
    yt = kc.poisoned((77, 1000), BF16, dev)
    ops.cast_transpose_bf16(x, yt)
    report('cast_transpose exact', float((yt != x.t().to(BF16)).sum()), 0.0)
    # grouped cast-transpose (dav_cast_transpose_grouped): every y bit-exact round-to-nearest-even of x^T, each inside its own guards
    pairs, gs = [], []
    for i, (R, Cc) in enumerate([(768, 2304), (3072, 768), (64, 192), (128, 64)]):
        xi = rnd(R, Cc, seed=200 + i)
        g = kc.Guarded(Cc, R, BF16, device=dev)
        pairs.append((xi, g.t))
        gs.append(g)
    ops.cast_transpose_grouped(pairs)
    for (xi, yi), g in zip(pairs, gs):
        n_bad = int((yi.view(torch.int16) != xi.t().contiguous().to(BF16).view(torch.int16)).sum())
        report(f'cast_transpose_grouped {tuple(xi.shape)} bit-exact', float(n_bad), 0.0)
        guard(f'cast_transpose_grouped {tuple(xi.shape)}', g)
    # ... and 100 items in one call (the library splits the list into launches of 96): ragged tiles, a single row, three columns
    pairs, gs = [], []
    for i in range(100):
        R, Cc = [(64, 64), (65, 3), (1, 130), (70, 129)][i % 4]
        xi = rnd(R, Cc, seed=400 + i)
        g = kc.Guarded(Cc, R, BF16, device=dev)
        pairs.append((xi, g.t))
        gs.append(g)
    ops.cast_transpose_grouped(pairs)
    bad = stray = 0
    for (xi, yi), g in zip(pairs, gs):
        bad += kc.exact(yi.reshape(-1), xi.t().to(BF16).reshape(-1))[0]      # (flat: a [130, 1] transpose keeps the strides of its source)
        stray += g.stray()[0]
    report('cast_transpose_grouped 100 items bit-exact', float(bad), 0.0)
    report('cast_transpose_grouped 100 items guards', float(stray), 0.0)


def _optimizer_one_shape():
    """the checks this family had before it was held per element (one size, two segments with equal hyper-parameters, whole-tensor
    norms against torch.optim.AdamW over three steps) — kept as they were"""
    flat = rnd(1234567, seed=52)
    out, ws = kc.poisoned((1,), F32, dev), torch.empty(1024, device=dev)
    ops.l2norm(flat, out, ws, 0.5)
    report('l2norm', abs(float(out) - 0.5 * float(flat.double().norm())) / float(flat.double().norm()), 1e-6)
    n = 100036                    # the flat buffers' contract: length and segment boundaries multiples of 4, 16-byte aligned
    p0, g0 = rnd(n, seed=53), rnd(n, seed=54)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([{'params': [pr], 'weight_decay': 0.05}], lr=1e-2, betas=(0.9, 0.95))
    p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = kc.poisoned((n,), BF16, dev)
    seg = torch.tensor([40000, n], device=dev, dtype=torch.int64)
    hyper = torch.tensor([1e-2, 0.05, 1e-2, 0.05], device=dev)
    for step in range(1, 4):
        pr.grad = g0 * step
        opt.step()
        bc = torch.tensor([1 - 0.9 ** step, math.sqrt(1 - 0.95 ** step)], device=dev)
        gcur = (g0 * step).clone()
        ssq = kc.poisoned((1,), F32, dev)                      # zeroed by the kernel first (header)
        keep = torch.tensor([0, 1 if step == 2 else 0], device=dev, dtype=torch.uint8)      # step 2: the second segment's gradient is kept
        ops.adamw_flat(p, gcur, m, v, pb, seg, hyper, 2, 0.9, 0.95, 1e-8, bc, sumsq_out=ssq, zero_grad=True, keep_grad=keep)
        report(f'adamw fused sumsq step{step}', abs(float(ssq) - float((g0 * step).double().pow(2).sum())) / float((g0 * step).double().pow(2).sum()), 1e-5)
        report(f'adamw fused zero_grad step{step}', float(gcur[:40000].abs().max()), 0.0)
        report(f'adamw fused zero_grad / keep_grad step{step}', float((gcur[40000:] - (g0 * step)[40000:] * (step == 2)).abs().max()), 0.0)
    report('adamw_flat vs torch.optim.AdamW', rel(p, pr.detach()), 1e-6)
    report('adamw bf16 mirror', rel(pb, p), 4e-3)
    # device-side step guard (dav_step_guard + dav_adamw_flat gscale_dev): clip factor as a device scalar == the same factor as
    # a host argument, bit for bit; scale 0 (non-finite loss / norm) leaves parameters, moments and mirror untouched, still
    # zero-fills the gradients and still reports sum(g^2)
    bc = torch.tensor([1 - 0.9 ** 4, math.sqrt(1 - 0.95 ** 4)], device=dev)
    one, nan, inf = torch.tensor([2.5], device=dev), torch.tensor([float('nan')], device=dev), torch.tensor([float('inf')], device=dev)
    gn, ws = kc.poisoned((1,), F32, dev), torch.empty(1024, device=dev)
    ops.l2norm(g0, gn, ws, 1.0)
    BAD0 = 7                                                                           # bad_count is incremented: a prefilled counter
    sc, bad = kc.poisoned((1,), F32, dev), torch.full((1,), BAD0, device=dev, dtype=torch.int32)
    clip = 0.25 * float(gn)
    ops.step_guard(one, one, gn, clip, 1.0, sc, bad)
    report('step_guard clip factor', abs(float(sc) - clip / (float(gn) + 1e-6)), 1e-7)
    ops.step_guard(one, None, gn, 10.0 * float(gn), 1.0, sc, bad)
    report('step_guard no clipping below the limit', abs(float(sc) - 1.0), 0.0)
    ops.step_guard(one, one, None, 0.0, 1.0, sc, bad)
    report('step_guard plain', abs(float(sc) - 1.0) + abs(int(bad) - BAD0), 0.0)
    for tag, (la, lb, nrm) in dict(nan_loss=(nan, one, None), inf_loss=(one, inf, gn), nan_norm=(one, one, nan)).items():
        bad.fill_(BAD0)
        ops.step_guard(la, lb, nrm, 1.0, 1.0, sc, bad)
        report(f'step_guard {tag} -> 0', abs(float(sc)) + abs(int(bad) - BAD0 - 1), 0.0)
    ops.step_guard(one, one, gn, clip, 1.0, sc, bad)
    pa, ma, va, pba, ga = p.clone(), m.clone(), v.clone(), pb.clone(), g0.clone()
    pc, mc, vc, pbc, gc = p.clone(), m.clone(), v.clone(), pb.clone(), g0.clone()
    ops.adamw_flat(pa, ga, ma, va, pba, seg, hyper, 2, 0.9, 0.95, 1e-8, bc, grad_scale=float(sc))
    ops.adamw_flat(pc, gc, mc, vc, pbc, seg, hyper, 2, 0.9, 0.95, 1e-8, bc, gscale_dev=sc)
    report('adamw gscale_dev == grad_scale (bit-equal)', float((pa != pc).sum() + (ma != mc).sum() + (va != vc).sum()), 0.0)
    sc.zero_()
    pz, mz, vz, pbz, gz, ssq = p.clone(), m.clone(), v.clone(), pb.clone(), g0.clone(), kc.poisoned((1,), F32, dev)
    ops.adamw_flat(pz, gz, mz, vz, pbz, seg, hyper, 2, 0.9, 0.95, 1e-8, bc, sumsq_out=ssq, zero_grad=True, gscale_dev=sc)
    report('adamw skipped step: p, m, v, mirror untouched', float((pz != p).sum() + (mz != m).sum() + (vz != v).sum() + (pbz != pb).sum()), 0.0)
    report('adamw skipped step: gradients zero-filled, sumsq reported', float(gz.abs().max()) + abs(float(ssq) / float(g0.double().pow(2).sum()) - 1.0), 1e-5)


B1, B2, EPS = 0.9, 0.95, 1e-8
OPT_SLICE = 1 << 22               # elements per float64 reference slice of the long buffers


def _bias_corr(step):
    return torch.tensor([1 - B1 ** step, math.sqrt(1 - B2 ** step)], device=dev)


def _table(sizes, decayed, n=None):
    """kcheck.seg_table on the device; n: the buffer's length where the last segment is cut short of its 64-element padding"""
    ends, hyper, real = kc.seg_table(sizes, decayed)
    if n is not None:
        assert (ends[-2] if len(ends) > 1 else 0) < n <= ends[-1] and n % 4 == 0
        ends[-1], real = n, real[:n]
    pad = (~real).nonzero().flatten().to(dev)
    return dict(ends=ends, n=ends[-1], nseg=len(ends), seg=torch.tensor(ends, device=dev, dtype=torch.int64),
                hyper=torch.tensor(hyper, device=dev), pad=pad, sizes=[e - s for s, e in zip([0] + ends[:-1], ends)])


def _per_seg(T, vals):
    """per-element copy of a per-segment list (repeat_interleave over the segment lengths)"""
    return torch.repeat_interleave(torch.as_tensor(vals, device=dev), torch.tensor(T['sizes'], device=dev))


def _flat_randn(T, seed, scale=1.0, seg_scale=None):
    """n normals drawn on the device, scaled per segment, exactly +0 on the padding"""
    x = drnd(T['n'], seed, scale)
    if seg_scale is not None:
        x *= _per_seg(T, seg_scale)
    x[T['pad']] = 0.0
    return x


def product_table():
    """A segment table of the kind util/flat.py builds for the product, from parameter sizes alone: two layers of a D = 192 block
    (norm, qkv, proj, norm, fc1, fc2 with their biases), three 1 x D tokens, a size that is no multiple of 64, a parameter that makes
    its end a multiple of 4096, one of 1024 behind it (an end on a multiple of 1024 that is none of 4096) and then 40 parameters of
    64 elements: the second 1024-element sweep of that workgroup crosses 16 of them.  wd = 0 on the 1-D sizes."""
    D = 192
    layer = [D, D, 3 * D * D, 3 * D, D * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D]
    dec = [s > 4 * D for s in layer]
    sizes, decayed = list(layer), list(dec)
    c = sum(sizes)                                                  # (all multiples of 64 so far)
    sizes += [(-c) % 4096 or 4096, 1024] + [64] * 40 + [D, D, D, 1000]
    decayed += [True, False] + [False] * 40 + [False, False, False, True]
    sizes += layer
    decayed += dec
    T = _table(sizes, decayed)
    e = T['ends']
    assert e[12] % 4096 == 0 and e[13] % 4096 == 1024 and all(e[13 + i] == e[13] + 64 * i for i in range(41))
    hy = T['hyper'].view(-1, 2).tolist()
    assert all(hy[i] != hy[i + 1] for i in range(len(hy) - 1))     # neighbours differ in lr or wd
    keep = [0] * T['nseg']
    keep[2], keep[-1] = 1, 1                                        # a 2-D weight and the last parameter
    for i in range(14, 54):
        keep[i] = i & 1                                             # alternating inside the run of 64-element segments
    T['keep'] = torch.tensor(keep, device=dev, dtype=torch.uint8)
    T['gscale'] = [10.0 ** ((i * 5) % 7 - 4) for i in range(T['nseg'])]      # gradient magnitude per parameter: 1e-4 .. 1e2
    return T


def adamw_call(tag, T, st, g, step, grad_scale=1.0, gscale_dev=None, mirror=True, zero_grad=False, keep=None, fam='adamw'):
    """ONE dav_adamw_flat call from the state ``st`` (p, m, v, pb: not modified — the kernel works on copies) with the gradient
    ``g``, judged against ONE kcheck.adamw_ref step from that same state: p, m, v per element, the mirror bit-exact against the
    rounding of the p the kernel stored, the padding exactly +0, the gradient untouched / zero-filled / kept, sum(g^2) within its
    depth bound, and every input the kernel only reads bit-identical afterwards.  Returns the new state (with 'g': the gradient
    buffer after the call)."""
    n, seg, hyper = T['n'], T['seg'], T['hyper']
    p, m, v, gin = st['p'].clone(), st['m'].clone(), st['v'].clone(), g.clone()
    pb = st['pb'].clone()
    bc = _bias_corr(step)
    ssq = kc.poisoned((1,), F32, dev)                              # zeroed by the kernel first (header)
    ro = [t for t in (seg, hyper, bc, keep, gscale_dev) if t is not None]
    ro0 = [t.clone() for t in ro]
    ops.adamw_flat(p, gin, m, v, pb if mirror else None, seg, hyper, T['nseg'], B1, B2, EPS, bc, grad_scale=grad_scale, sumsq_out=ssq,
                   zero_grad=zero_grad, keep_grad=keep, gscale_dev=gscale_dev)
    gs = kc.f32(grad_scale) * (float(gscale_dev) if gscale_dev is not None else 1.0)       # the kernel's fp32 product (exact here)

    def ref(lo, hi):
        return kc.adamw_ref(st['p'][lo:hi], g[lo:hi], st['m'][lo:hi], st['v'][lo:hi], seg, hyper, B1, B2, EPS, bc, gs, start=lo)
    worst, first = dict(p=0.0, m=0.0, v=0.0), dict(p='', m='', v='')
    for lo in range(0, n, OPT_SLICE):                               # (the long buffers: float64 temporaries of one slice at a time)
        hi = min(n, lo + OPT_SLICE)
        r = ref(lo, hi)
        for k, got in (('p', p), ('m', m), ('v', v)):
            ok, ratio, msg = kc.within(got[lo:hi], r[k], r['b' + k], f'{tag} {k} (flat index = {lo} +)')
            worst[k] = max(worst[k], ratio)                         # (inf for a non-finite element)
            first[k] = first[k] or msg
    for k in 'pmv':
        kc.note(f'{fam} {k}', worst[k])
        RESULTS.append((f'{tag} {k} elementwise', worst[k], 1.0, worst[k] <= 1.0))
        print(f'{"PASS" if worst[k] <= 1.0 else "FAIL"} {tag} {k} elementwise: worst err/bound={worst[k]:.3e}' + (f' — {first[k]}' if first[k] else ''), flush=True)
    if mirror:
        same(f'{tag} bf16 mirror == bf16(p stored)', pb, p.to(BF16))
    else:
        kept(f'{tag} no mirror given: the earlier mirror', pb, st['pb'])
    pad = T['pad']
    if pad.numel():
        same(f'{tag} padding of p, m, v stays +0', torch.cat([p[pad], m[pad], v[pad]]), torch.zeros(3 * pad.numel(), device=dev))
        if mirror:
            same(f'{tag} padding of the mirror stays +0', pb[pad], torch.zeros(pad.numel(), device=dev, dtype=BF16))
    if zero_grad:
        km = _per_seg(T, keep if keep is not None else torch.zeros(T['nseg'], device=dev, dtype=torch.uint8)).bool()
        same(f'{tag} zero_grad: gradients outside keep_grad are +0', gin[~km], torch.zeros(int((~km).sum()), device=dev))
        kept(f'{tag} zero_grad: gradients inside keep_grad', gin, g, km)
    else:
        kept(f'{tag} gradients (zero_grad off)', gin, g)
    want = float(g.double().pow(2).sum())
    elem(f'{tag} fused sumsq', f'{fam} sumsq', ssq[0], torch.tensor(want, dtype=torch.float64, device=dev), kc.adamw_sumsq_bound(n, want))
    for i, (t, t0) in enumerate(zip(ro, ro0)):
        kept(f'{tag} read-only input {i}', t, t0)
    return dict(p=p, m=m, v=v, pb=pb if mirror else st['pb'], g=gin)


def _fresh_state(T, seed, trained=False):
    """|p| ~ 0.02, the padding +0; m = v = 0 (step 1) or the moments of an earlier gradient; the mirror starts poisoned"""
    p = _flat_randn(T, seed, 0.02)
    if trained:
        g0 = _flat_randn(T, seed + 1, 1.0, T.get('gscale'))
        m, v = 0.1 * g0, 0.05 * g0 * g0
    else:
        m, v = torch.zeros(T['n'], device=dev), torch.zeros(T['n'], device=dev)
    return dict(p=p, m=m, v=v, pb=kc.poisoned((T['n'],), BF16, dev))


def _adamw_product_table():
    T = product_table()
    print(f'product-like table: {T["n"]} elements, {T["nseg"]} segments', flush=True)
    st = _fresh_state(T, 500)
    # three consecutive calls: bias corrections of steps 1 .. 3, the gradient changes sign and scale in between
    for step, scale, zg in ((1, 1.0, False), (2, -3e-3, True), (3, 40.0, True)):
        g = _flat_randn(T, 510 + step, scale, T['gscale'])
        if step == 1:
            g[::7] = 0.0                                            # zeros among the gradients (and m = v = 0: 0 / eps)
        st = adamw_call(f'adamw product table step{step}', T, st, g, step, zero_grad=zg, keep=T['keep'])
    base = dict(p=st['p'], m=st['m'], v=st['v'], pb=st['pb'])
    g = _flat_randn(T, 520, 0.5, T['gscale'])
    host = adamw_call('adamw product table grad_scale 0.37', T, base, g, 4, grad_scale=0.37)
    sc = torch.tensor([0.37], device=dev)
    devs = adamw_call('adamw product table gscale_dev 0.37', T, base, g, 4, gscale_dev=sc)
    same('adamw gscale_dev == grad_scale (bit-equal p, m, v, mirror)', torch.cat([devs[k].float() for k in ('p', 'm', 'v', 'pb')]),
         torch.cat([host[k].float() for k in ('p', 'm', 'v', 'pb')]))
    nomir = adamw_call('adamw product table without mirror', T, base, g, 4, grad_scale=0.37, mirror=False)
    same('adamw without mirror == with mirror (bit-equal p, m, v)', torch.cat([nomir[k] for k in 'pmv']), torch.cat([host[k] for k in 'pmv']))
    # the skipped step (gscale_dev = 0: a non-finite loss or norm): parameters, moments and mirror untouched, gradients still
    # zero-filled outside keep_grad, sum(g^2) still reported
    sc.zero_()
    pz, mz, vz, pbz, gz, ssq = base['p'].clone(), base['m'].clone(), base['v'].clone(), base['pb'].clone(), g.clone(), kc.poisoned((1,), F32, dev)
    ops.adamw_flat(pz, gz, mz, vz, pbz, T['seg'], T['hyper'], T['nseg'], B1, B2, EPS, _bias_corr(4), sumsq_out=ssq, zero_grad=True,
                   keep_grad=T['keep'], gscale_dev=sc)
    report('adamw skipped step: p, m, v, mirror untouched',
           float((pz != base['p']).sum() + (mz != base['m']).sum() + (vz != base['v']).sum() + (pbz != base['pb']).sum()), 0.0)
    kept('adamw skipped step: p, m, v', torch.cat([pz, mz, vz]), torch.cat([base[k] for k in 'pmv']))
    kept('adamw skipped step: mirror', pbz, base['pb'])
    km = _per_seg(T, T['keep']).bool()
    want = float(g.double().pow(2).sum())
    report('adamw skipped step: gradients zero-filled, sumsq reported', float(gz[~km].abs().max()) + abs(float(ssq) / want - 1.0), 1e-5)
    same('adamw skipped step: gradients outside keep_grad are +0', gz[~km], torch.zeros(int((~km).sum()), device=dev))
    kept('adamw skipped step: gradients inside keep_grad', gz, g, km)
    elem('adamw skipped step: fused sumsq', 'adamw sumsq', ssq[0], torch.tensor(want, dtype=torch.float64, device=dev), kc.adamw_sumsq_bound(T['n'], want))


def _adamw_degenerate_and_contract():
    for tag, sizes, dec, n in (('one segment of 4', [4], [True], 4),
                               ('4096 + 4: a second workgroup with one float4', [64, 4036], [False, True], 4100),
                               ('last segment of 64', [1000, 8192, 64], [True, True, False], None)):
        T = _table(sizes, dec, n)
        keep = torch.tensor([i & 1 for i in range(T['nseg'])], device=dev, dtype=torch.uint8)
        adamw_call(f'adamw {tag}', T, _fresh_state(T, 530, trained=True), _flat_randn(T, 531), 2, grad_scale=0.37, zero_grad=True, keep=keep)
    T = _table([64, 64], [True, False])
    st, g, bc = _fresh_state(T, 540), _flat_randn(T, 541), _bias_corr(1)
    wide = torch.zeros(T['n'] + 4, device=dev)
    snap = torch.cat([st['p'], st['m'], st['v'], g])

    def call(p, gg, m, v, nseg):
        ops.adamw_flat(p, gg, m, v, None, T['seg'], T['hyper'], nseg, B1, B2, EPS, bc)
    rejected('adamw n % 4 != 0', lambda: call(st['p'][:126], g[:126], st['m'][:126], st['v'][:126], 2))
    rejected('adamw p offset by one element (misaligned)', lambda: call(wide[1:1 + T['n']], g, st['m'], st['v'], 2))
    rejected('adamw nseg = 0', lambda: call(st['p'], g, st['m'], st['v'], 0))
    kept('adamw rejected calls: state', torch.cat([st['p'], st['m'], st['v'], g]), snap)


def _adamw_grid_cap():
    """n = 16384 x 4096 + 2 x 4096 + 1732: one element more than the capped grid covers in one trip would do; this size class has
    a ragged second trip of three workgroups, each searching its segment again.  About 300 segments; the 64-element ones sit at
    the head, and around and behind element 16384 x 4096 — the part only the second trip reaches.  One step, data drawn on the
    device, float64 reference in slices."""
    import random
    t0 = _now()
    n = kc.ADAMW_GRID_CAP * kc.ADAMW_CHUNK + 2 * 4096 + 1732
    rng = random.Random(5)
    head = [rng.choice([64] * 5 + [192, 576, 768, 2304, 36864, 147456, 589824]) for _ in range(240)]
    tail = [64] * 40 + [1000] + [64] * 8 + [192] * 4 + [2304] + [64] * 10 + [1152, 1988]
    pad = lambda s: -(-s // 64) * 64                                # noqa: E731
    t_start = kc.ADAMW_GRID_CAP * kc.ADAMW_CHUNK - 1024             # the run of 64s straddles the end of the first trip
    fill = t_start - sum(head)
    assert fill > 0 and fill % 64 == 0
    mid = [fill // 3 // 64 * 64, fill // 3 // 64 * 64]
    mid.append(fill - sum(mid))
    sizes = head + mid + tail
    T = _table(sizes, [s > 768 for s in sizes], n)
    assert T['n'] == n and sum(pad(s) for s in sizes[:-1]) + 1988 == n and T['ends'][len(head) + 2] == t_start
    assert sum(1 for e in T['ends'] if e > kc.ADAMW_GRID_CAP * kc.ADAMW_CHUNK) >= 40 and kc.adamw_grid(n) == (kc.ADAMW_GRID_CAP, 2)
    T['keep'] = torch.tensor([(i % 3 == 0) for i in range(T['nseg'])], device=dev, dtype=torch.uint8)
    T['gscale'] = [10.0 ** ((i * 5) % 7 - 4) for i in range(T['nseg'])]
    print(f'grid-cap table: {n} elements, {T["nseg"]} segments', flush=True)
    st = _fresh_state(T, 550, trained=True)
    g = _flat_randn(T, 552, 1.0, T['gscale'])
    adamw_call('adamw grid cap', T, st, g, 3, grad_scale=0.37, zero_grad=True, keep=T['keep'], fam='adamw grid cap')
    torch.cuda.synchronize()
    print(f'wall time of the grid-cap case: {_now() - t0:.2f} s', flush=True)


def _l2norm_sizes():
    for n in (1, 3, 4, 1023, 262144 + 1, 1234567):
        # magnitudes over six decades; the float4 part's first and last element and every tail element carry a visible share
        x = drnd(n, 560 + n % 89) * 10.0 ** (torch.arange(n, device=dev) % 7 - 3).float()
        big = float(x.double().norm()) + 1.0
        for i in {0, max(0, (n >> 2 << 2) - 1), *range(n >> 2 << 2, n)}:
            x[i] = 0.1 * big * (-1) ** i
        x0 = x.clone()
        out, ws = kc.poisoned((1,), F32, dev), torch.full((1024,), float('nan'), device=dev)
        ops.l2norm(x, out, ws, 0.5)
        want = kc.f32(0.5) * float(x.double().norm())
        report(f'l2norm n={n}', abs(float(out) - want) / want, 1e-6)
        elem(f'l2norm n={n}', 'l2norm', out[0], torch.tensor(want, dtype=torch.float64, device=dev), kc.l2norm_bound(n, want))
        kept(f'l2norm n={n} input', x, x0)
    for n in (3, 1027, 262144 + 3):                                 # zero everywhere but ONE element, in the tail workgroup 0 reads
        x = torch.zeros(n, device=dev)
        x[n - 1] = -3.25
        out, ws = kc.poisoned((1,), F32, dev), torch.full((1024,), float('nan'), device=dev)
        ops.l2norm(x, out, ws, 2.0)
        elem(f'l2norm n={n} one tail element', 'l2norm', out[0], torch.tensor(6.5, dtype=torch.float64, device=dev), kc.l2norm_bound(n, 6.5))
    x, out = drnd(64, 570), kc.poisoned((1,), F32, dev)
    rejected('l2norm n = 0', lambda: ops.l2norm(x[:0], out, torch.empty(1024, device=dev), 1.0))
    rejected('l2norm workspace of 1023 floats', lambda: ops.l2norm(x, out, torch.empty(1023, device=dev), 1.0))
    report('l2norm rejected calls leave out poisoned', 0.0 if bool(out.isnan().all()) else 1.0, 0.0)


def _step_guard_more():
    """beyond the cases of _optimizer_one_shape: clip = 0 with a norm given, grad_scale entering the clipped norm, a norm exactly at
    the limit.  s = min(1, clip / (norm grad_scale + 1e-6)): a product, a sum and a division in fp32 — 4 u of the float64 value."""
    gn, sc = torch.tensor([316.22775], device=dev), kc.poisoned((1,), F32, dev)
    one = torch.tensor([2.5], device=dev)
    ops.step_guard(one, one, gn, 0.0, 1.0, sc, None)
    report('step_guard clip = 0 with a norm given -> 1', abs(float(sc) - 1.0), 0.0)
    for tag, clip, gs in (('grad_scale 0.37 in the clipped norm', 50.0, 0.37), ('grad_scale 1/128: below the limit', 3.0, 1.0 / 128),
                          ('norm exactly at the limit', float(gn), 1.0), ('norm at the limit through grad_scale', 0.25 * float(gn), 0.25)):
        sc.fill_(float('nan'))
        ops.step_guard(one, None, gn, clip, gs, sc, None)
        want = min(1.0, kc.f32(clip) / (float(gn) * kc.f32(gs) + kc.f32(1e-6)))
        elem(f'step_guard {tag}', 'step_guard', sc[0], torch.tensor(want, dtype=torch.float64, device=dev), 4 * kc.U32 * want)
        report(f'step_guard {tag}: never above 1', max(0.0, float(sc) - 1.0), 0.0)


def _now():
    import time
    torch.cuda.synchronize()
    return time.perf_counter()


@check
def optimizer():
    """The optimizer pass over the flat buffers: dav_adamw_flat, dav_l2norm, dav_step_guard"""
    t0 = _now()
    _optimizer_one_shape()
    _l2norm_sizes()
    _step_guard_more()
    _adamw_product_table()
    _adamw_degenerate_and_contract()
    _adamw_grid_cap()
    print(f'wall time of optimizer(): {_now() - t0:.2f} s', flush=True)


def main():
    flt = sys.argv[1] if len(sys.argv) > 1 else ''
    print('device:', torch.cuda.get_device_name(0), flush=True)
    for kv in os.environ.get('DAV_TUNE', '').split(','):      # same launch-geometry knobs as bench.py (e.g. DAV_TUNE=4:1)
        if ':' in kv:
            from deepavfusion_amd import _lib
            _lib.check(_lib.load().dav_tune(int(kv.split(':')[0]), int(kv.split(':')[1])), 'dav_tune')
    for fn in (gemm_nt, gemm_tn, gemm_tn_gang, attention, dropout, window_attention, layernorm, ln_fused, masking, misc_kernels, optimizer, patch_gather3d):
        if flt in fn.__name__:
            fn()
    bad = [r for r in RESULTS if not r[3]]
    print('worst err / bound per family:', {k: float(f'{v:.3e}') for k, v in sorted(kc.RATIOS.items())})
    print(f'\n{len(RESULTS) - len(bad)}/{len(RESULTS)} checks passed')
    for r in bad:
        print('  FAILED:', r[0], r[1])
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
