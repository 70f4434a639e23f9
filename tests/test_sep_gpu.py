"""Source-separation audio on the device: dav_stft_c32, dav_istft_c32 and the fused dav_sep_mask_istft elementwise against the
float64 restatement (tests/stft_ref.py) fed the module's own fp32 window, twiddle and filterbank tables (widened: table rounding
is not in the error), with bounds propagated in float64 through the same chain; determinism; the reference's shapes through
util/separation.py.  Outputs are poisoned and guard-banded with a padded row stride (the complex one through its fp32 view).

Term counts (u = 2^-24, kcheck.sum_bound(sum|t_i|, n, ref) = n u sum|t_i| + 4 u |ref|):
  N_FWD = n_fft + 2        a part of a bin is a sum of n_fft products x w cos; + the rounding of x w and the combination of the
                           even / odd partial sums
  N_INV = 2 n_freqs + ceil(n_fft / hop) + 4
                           a sample of a frame is a sum of 2 n_freqs products (Re cos, Im sin), ceil(n_fft / hop) frames are added,
                           + the 1 / N scale, the window, the envelope and the division
  N_TAB = 3                only where the reference is NOT fed the fp32 tables (the round trip against x itself): the rounding of
                           the window, of the cos / sin table and of the window again in the envelope, one u per term each
Worst err / bound per family is printed and noted with kcheck.note."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kcheck  # noqa: E402
import stft_ref as R  # noqa: E402
from kcheck import FLT_MIN, U32, Guarded, sum_bound, within  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'

#        rate  n_fft hop n_mels   — the reference's geometries (n_fft = 0.05 rate, hop = rate / 64) at 16 kHz and 8 kHz
GEOMS = [(16000, 800, 250, 128), (8000, 400, 125, 64)]

# Relative error allowed to the kernel's sigmoid s(x) = 1.0f / (1.0f + expf(-x)), from the accuracy ROCm documents for the device
# functions it calls (HIP programming guide, "Math API", single precision): expf 1 ULP; the addition is correctly rounded (0.5
# ULP); the division is correctly rounded by default (-fhip-fp32-correctly-rounded-divide-sqrt) and 2.5 ULP where it is not — the
# looser figure is taken.  |ds / s| = e / (1 + e) |de / e| <= |de / e|, so the three add: 4 ULP of 2^-23.  Absolutely, a sigmoid
# below the smallest normal fp32 (x < -87.3: expf overflows to inf, 1 / inf = 0) may come out as 0: FLT_MIN.
SIGMOID_ULPS = 1.0 + 0.5 + 2.5
SIGMOID_REL = SIGMOID_ULPS * 2.0 ** -23
N_TAB = 3


def _n_fwd(n_fft):
    return n_fft + 2


def _n_inv(n_fft, hop):
    return 2 * (n_fft // 2 + 1) + -(-n_fft // hop) + 4


_MEL = {}


def _mel(rate):
    """MelSpectrogram of the geometry on the device (window, cos / sin tables, filterbank and bands: the kernels' operands), once"""
    if rate not in _MEL:
        from deepavfusion_amd.util import audio_transforms as aT
        _, n_fft, hop, n_mels = next(g for g in GEOMS if g[0] == rate)
        _MEL[rate] = aT.MelSpectrogram(rate, n_fft, hop, n_mels).to(DEV)
    return _MEL[rate]


def _tabs64(m):
    return tuple(t.double().cpu().numpy() for t in (m.window, m.cos_tab, m.sin_tab))


def _waves(B, S, seed):
    """noise in [-1, 1] with a tone on top of every second row (fp32)"""
    g = np.random.default_rng(seed)
    x = g.uniform(-1, 1, (B, S))
    x[::2] = 0.5 * x[::2] + 0.5 * np.sin(2 * np.pi * 0.013 * np.arange(S))[None]
    return x.astype(np.float32)


def _strided(x, pad):
    """numpy [B, S] -> a device view whose rows lie S + pad apart"""
    B, S = x.shape
    src = torch.zeros(B, S + pad, dtype=torch.float32, device=DEV)
    src[:, :S] = torch.from_numpy(x).to(DEV)
    return src[:, :S]


def _lengths(n_fft, hop):
    """n_fft / 2 + 1 (the shortest signal: two frames); hop F - 1, hop F, hop F + 1 around the seam of the forward kernel (F =
    STFT_FRAMES frames per workgroup) and around the seam of the inverse (a workgroup owns istft_tile = hop G samples; the output
    has hop (S // hop) of them, so hop (G + 1) gives the second workgroup its first hop); three workgroups and a partial fourth
    of both"""
    from deepavfusion_amd import ops
    F, G = ops.STFT_FRAMES, ops.istft_tile(n_fft, hop) // hop
    assert G >= 1 and ops.istft_tile(n_fft, hop) == G * hop
    out = {n_fft // 2 + 1, hop * (G + 1), hop * (3 * max(F, G) + 2) + 7}
    for f in (F, G):
        out |= {hop * f - 1, hop * f, hop * f + 1}
    return sorted(out)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_stft(m, x, pad):
    from deepavfusion_amd import ops
    B, S = x.shape
    F, frames = m.n_fft // 2 + 1, S // m.hop + 1
    out = Guarded(B * F, 2 * frames, torch.float32, ld=2 * frames + 2, device=DEV, fill='poison')
    ops.stft(_strided(x, pad), m.window, m.cos_tab, m.sin_tab, m.n_fft, m.hop, out=out.t)
    torch.cuda.synchronize()
    n_stray, where = out.stray()
    assert n_stray == 0, where
    return out.t[:, 0::2].reshape(B, F, frames), out.t[:, 1::2].reshape(B, F, frames)


def _run_istft(m, Z, pad):
    """Z numpy complex64 [B, F, frames]; the bin rows of the device copy lie frames + pad complex elements apart"""
    from deepavfusion_amd import ops
    B, F, frames = Z.shape
    L = m.hop * (frames - 1)
    src = torch.zeros(B, F, frames + pad, dtype=torch.complex64, device=DEV)
    src[:, :, :frames] = torch.from_numpy(Z).to(DEV)
    out = Guarded(B, L, torch.float32, ld=L + 3, device=DEV, fill='poison')
    ops.istft(src[:, :, :frames], m.window, m.cos_tab, m.sin_tab, m.n_fft, m.hop, out=out.t)
    torch.cuda.synchronize()
    n_stray, where = out.stray()
    assert n_stray == 0, where
    return out.t


def _run_fused(m, x, logits, pad):
    from deepavfusion_amd import ops
    B, S = x.shape
    K, T = logits.shape[1], logits.shape[3]
    out = Guarded(B * K, m.hop * T, torch.float32, ld=m.hop * T + 3, device=DEV, fill='poison')
    ops.sep_mask_istft(_strided(x, pad), torch.from_numpy(logits).to(DEV), m.window, m.cos_tab, m.sin_tab, m.fbank, m.band_lo, m.band_hi,
                       m.n_fft, m.hop, out=out.t)
    torch.cuda.synchronize()
    n_stray, where = out.stray()
    assert n_stray == 0, where
    return out.t.reshape(B, K, m.hop * T)


def _fwd_error(X, mag, n):
    """check 1's bound as arrays: each part of a bin within n u sum|x w| + 4 u |part|"""
    return n * U32 * mag + 4 * U32 * np.abs(X.real), n * U32 * mag + 4 * U32 * np.abs(X.imag)


def _inv_bound(re_mag, im_mag, e_re, e_im, ref, m, tabs, n):
    """An input spectrum known to (e_re, e_im) per part -> the bound of the inverse's output: the input error carried by the
    inverse map with absolute coefficients, plus check 2's bound on the spectrum as the kernel sees it (magnitudes + errors)"""
    carried = R.istft_abs(e_re, e_im, m.n_fft, m.hop, *tabs)
    A = R.istft_abs(re_mag + e_re, im_mag + e_im, m.n_fft, m.hop, *tabs)
    return _t(carried) + sum_bound(_t(A), n, _t(ref))


def _band_terms(m):
    """per bin f: the number of filters the kernel's band sum runs over — from the first to the last m with band_lo[m] <= f <
    band_hi[m] — as [F, 1]"""
    lo, hi = m.band_lo.cpu().numpy(), m.band_hi.cpu().numpy()
    F = m.n_fft // 2 + 1
    f = np.arange(F)[:, None]
    inside = (lo[None, :] <= f) & (f < hi[None, :])
    first = np.where(inside.any(1), inside.argmax(1), 0)
    last = np.where(inside.any(1), inside.shape[1] - inside[:, ::-1].argmax(1), 0)
    return (last - first)[:, None].astype(np.float64)


def _fused_ref_and_bound(m, x, logits):
    """The float64 chain fed the module's tables, and the error propagated through it:
      E_X  check 1's bound of each part of the mixture's spectrum
      E_M  = (nb + 1) u M + SIGMOID_REL M + FLT_MIN sum_m fb: a band sum of nb non-negative terms (the sum of absolute terms is M
             itself) + the rounding of each product, the sigmoid's relative allowance on every term, its absolute one times the weights
      E_Y  = M E_X + |X| E_M + E_M E_X + u |Y| per part (Y = M X, one rounding)
      out  the inverse map with absolute coefficients applied to E_Y, plus check 2's bound"""
    tabs = _tabs64(m)
    fb = m.fbank.double().cpu().numpy()
    X, mag = R.stft(x, m.n_fft, m.hop, *tabs, return_abs=True)                   # [B, F, T + 1]
    e_re, e_im = _fwd_error(X, mag, _n_fwd(m.n_fft))
    M = R.mel_mask(logits, fb)                                                   # [B, K, F, T + 1]
    e_M = (_band_terms(m) + 1) * U32 * M + SIGMOID_REL * M + FLT_MIN * fb.sum(1)[:, None]
    e_M[..., -1] = 0.0                                                           # the appended column is an exact zero on both sides
    Xb = X[:, None]
    Y = M * Xb
    ey_re = M * e_re[:, None] + np.abs(Xb.real) * e_M + e_M * e_re[:, None] + U32 * np.abs(Y.real)
    ey_im = M * e_im[:, None] + np.abs(Xb.imag) * e_M + e_M * e_im[:, None] + U32 * np.abs(Y.imag)
    ref = R.istft(Y, m.n_fft, m.hop, *tabs)
    return ref, _inv_bound(np.abs(Y.real), np.abs(Y.imag), ey_re, ey_im, ref, m, tabs, _n_inv(m.n_fft, m.hop))


def _logits(B, K, n_mels, T, seed):
    """N(0, 3) with planted entries at +-30 and +-100"""
    g = np.random.default_rng(seed)
    lg = 3.0 * g.normal(size=(B, K, n_mels, T))
    flat = lg.reshape(-1)
    idx = g.choice(flat.size, size=min(64, flat.size), replace=False)
    flat[idx] = np.resize(np.array([30.0, -30.0, 100.0, -100.0]), idx.size)
    return lg.astype(np.float32)


@pytest.mark.parametrize('rate,n_fft,hop,n_mels', GEOMS)
def test_stft_matches_the_float64_restatement_elementwise(rate, n_fft, hop, n_mels):
    """re and im of every bin within sum_bound(sum_n |x w|, n_fft + 2, ref) of the restatement fed the module's fp32 tables; B = 1
    dense and B = 3 with rows strided apart; lengths at the seams of the tiling (_lengths).
    Worst err / bound measured on an MI355X: 0.0089 at 800 / 250, 0.012 at 400 / 125 (a fixed-order fmaf chain errs like a
    random walk; the bound allows for the worst case of any order)."""
    m = _mel(rate)
    tabs = _tabs64(m)
    worst = 0.0
    for S in _lengths(n_fft, hop):
        for B, pad in ((1, 0), (3, 5)):
            x = _waves(B, S, seed=S * 7 + B)
            re, im = _run_stft(m, x, pad)
            X, mag = R.stft(x, n_fft, hop, *tabs, return_abs=True)
            assert re.shape == im.shape == X.shape == (B, n_fft // 2 + 1, S // hop + 1)
            for got, ref, part in ((re, X.real, 're'), (im, X.imag, 'im')):
                ref = _t(ref)
                ok, w, msg = within(got, ref, sum_bound(_t(np.broadcast_to(mag, X.shape)), _n_fwd(n_fft), ref), f'stft {n_fft}/{hop} S={S} B={B} {part}')
                assert ok, msg
                worst = max(worst, w)
    kcheck.note(f'stft {n_fft}/{hop}', worst)
    print(f'stft {n_fft}/{hop}: worst err / bound {worst:.3g}')


@pytest.mark.parametrize('rate,n_fft,hop,n_mels', GEOMS)
def test_istft_matches_the_float64_restatement_elementwise(rate, n_fft, hop, n_mels):
    """Random complex spectra (normal re and im, so the DC and Nyquist bins carry imaginary parts, which must be ignored): every
    sample within sum_bound(A, 2 n_freqs + ceil(n_fft / hop) + 4, ref), A[j] = (1 / env[j]) sum_t w sum_k c_k (|Re X||cos| +
    |Im X||sin|) / N from the restatement.  Frame counts S // hop + 1 of the same lengths; bin rows dense and strided.
    Worst err / bound measured on an MI355X: 0.0011 at 800 / 250, 0.0024 at 400 / 125."""
    m = _mel(rate)
    tabs = _tabs64(m)
    worst = 0.0
    for S in _lengths(n_fft, hop):
        frames = S // hop + 1
        for B, pad in ((1, 0), (3, 3)):
            g = np.random.default_rng(S * 5 + B)
            Z = (g.normal(size=(B, n_fft // 2 + 1, frames)) + 1j * g.normal(size=(B, n_fft // 2 + 1, frames))).astype(np.complex64)
            got = _run_istft(m, Z, pad)
            ref, A = R.istft(Z, n_fft, hop, *tabs, return_abs=True)
            assert got.shape == ref.shape == (B, hop * (frames - 1))
            ref = _t(ref)
            ok, w, msg = within(got, ref, sum_bound(_t(A), _n_inv(n_fft, hop), ref), f'istft {n_fft}/{hop} frames={frames} B={B}')
            assert ok, msg
            worst = max(worst, w)
            if S == _lengths(n_fft, hop)[1]:                                     # the imaginary DC / Nyquist parts change nothing
                Z2 = Z.copy()
                Z2[:, 0] = Z2[:, 0].real + 7j
                Z2[:, -1] = Z2[:, -1].real - 5j
                assert torch.equal(_run_istft(m, Z2, pad), got)
    kcheck.note(f'istft {n_fft}/{hop}', worst)
    print(f'istft {n_fft}/{hop}: worst err / bound {worst:.3g}')


@pytest.mark.parametrize('rate,n_fft,hop,n_mels', GEOMS)
def test_round_trip_returns_the_signal(rate, n_fft, hop, n_mels):
    """InverseSpectrogram(Spectrogram(x)) against x[:hop (frames - 1)] itself (the overlap-added Hann frames divided by their
    envelope reconstruct it), within the composition of the two bounds: the spectrum is known to check 1's bound, that error is
    carried through the inverse map with absolute coefficients, and check 2's bound is added.  The reference here is NOT fed the
    fp32 tables, so N_TAB more terms stand for their rounding in each direction.
    Worst err / bound measured on an MI355X: 5.5e-5 at 800 / 250, 1.5e-4 at 400 / 125 (worst cases multiplied through two
    transforms; the absolute error is a few 1e-7)."""
    from deepavfusion_amd.util import audio_transforms as aT
    spec_t, inv_t = aT.Spectrogram(n_fft, hop, power=None).to(DEV), aT.InverseSpectrogram(n_fft, hop).to(DEV)
    m = _mel(rate)
    S = _lengths(n_fft, hop)[-1]
    x = _waves(3, S, seed=17)
    L = hop * (S // hop)
    spec = spec_t(torch.from_numpy(x).to(DEV))
    assert spec.dtype == torch.complex64 and spec.shape == (3, n_fft // 2 + 1, S // hop + 1)
    got = inv_t(spec)
    assert got.shape == (3, L) and got.dtype == torch.float32
    X, mag = R.stft(x, n_fft, hop, return_abs=True)
    e_re, e_im = _fwd_error(X, mag, _n_fwd(n_fft) + N_TAB)
    ref = x[:, :L].astype(np.float64)
    bound = _inv_bound(np.abs(X.real), np.abs(X.imag), e_re, e_im, ref, m, (None, None, None), _n_inv(n_fft, hop) + N_TAB)
    ok, w, msg = within(got, _t(ref), bound, f'round trip {n_fft}/{hop}')
    assert ok, msg
    kcheck.note(f'stft round trip {n_fft}/{hop}', w)
    print(f'round trip {n_fft}/{hop}: worst err / bound {w:.3g}')
    assert torch.equal(spec_t(torch.from_numpy(x[:1]).to(DEV)[0])[None], spec[:1])           # [S] -> [F, frames]


@pytest.mark.parametrize('K', [1, 2])
@pytest.mark.parametrize('rate,n_fft,hop,n_mels', GEOMS)
def test_fused_masking_matches_the_propagated_bound(rate, n_fft, hop, n_mels, K):
    """dav_sep_mask_istft against the restatement's chain with the error propagated in float64 (_fused_ref_and_bound); logits
    N(0, 3) with planted +-30 and +-100.  Lengths: the shortest, the seams of the inverse's tiling, three workgroups and a
    partial fourth.  Planted: every logit at -100 returns exact zeros; with every logit at +100 the last frame still contributes
    nothing (and the restatement shows that an unmasked last frame would be far outside the bound).
    Worst err / bound measured on an MI355X: 8.7e-5 at 800 / 250, 2.2e-4 at 400 / 125, for K = 1 and K = 2 alike."""
    from deepavfusion_amd import ops
    m = _mel(rate)
    G = ops.istft_tile(n_fft, hop) // hop
    worst = 0.0
    for S in (n_fft // 2 + 1, hop * G, hop * (G + 1) + 1, hop * (3 * G + 2) + 7):
        T = S // hop
        for B, pad in ((1, 0), (3, 5)):
            x = _waves(B, S, seed=S * 3 + B)
            lg = _logits(B, K, n_mels, T, seed=S + K)
            got = _run_fused(m, x, lg, pad)
            ref, bound = _fused_ref_and_bound(m, x, lg)
            assert got.shape == ref.shape == (B, K, hop * T)
            ok, w, msg = within(got, _t(ref), bound, f'fused {n_fft}/{hop} S={S} B={B} K={K}')
            assert ok, msg
            worst = max(worst, w)
    kcheck.note(f'sep_mask_istft {n_fft}/{hop}', worst)
    print(f'sep_mask_istft {n_fft}/{hop} K={K}: worst err / bound {worst:.3g}')
    S = hop * (G + 1) + 1
    T = S // hop
    x = _waves(2, S, seed=5)
    off = _run_fused(m, x, np.full((2, K, n_mels, T), -100.0, np.float32), 0)
    assert bool((off == 0).all())
    on = np.full((2, K, n_mels, T), 100.0, np.float32)
    got = _run_fused(m, x, on, 0)
    ref, bound = _fused_ref_and_bound(m, x, on)
    ok, _, msg = within(got, _t(ref), bound, f'fused {n_fft}/{hop} all +100')
    assert ok, msg
    tabs = _tabs64(m)
    M = R.mel_mask(on, m.fbank.double().cpu().numpy())
    M[..., -1] = M[..., -2]                                                      # what an unmasked last frame would give
    leak = R.istft(M * R.stft(x, n_fft, hop, *tabs)[:, None], n_fft, hop, *tabs)
    assert float((np.abs(leak - ref) / np.maximum(bound.cpu().numpy(), 1e-300)).max()) > 100.0


@pytest.mark.parametrize('rate,n_fft,hop,n_mels', GEOMS)
def test_every_entry_point_is_deterministic(rate, n_fft, hop, n_mels):
    m = _mel(rate)
    S = _lengths(n_fft, hop)[-1]
    x = _waves(3, S, seed=2)
    a, b = _run_stft(m, x, 5), _run_stft(m, x, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    Z = torch.complex(a[0], a[1]).cpu().numpy()
    assert torch.equal(_run_istft(m, Z, 3), _run_istft(m, Z, 3))
    lg = _logits(3, 2, n_mels, S // hop, seed=4)
    assert torch.equal(_run_fused(m, x, lg, 5), _run_fused(m, x, lg, 5))


def test_spectrogram_masking_at_the_reference_shapes():
    """SpectrogramMasking(16000, 128) on [1, 48000] and [1, 128, 192] -> [1, 48000] within the bound of the fused check; the
    batched call with B = 2 and K = 2 returns the four rows of four single calls, bit for bit.
    Worst err / bound measured on an MI355X: 7.1e-5."""
    from deepavfusion_amd.util.separation import SpectrogramMasking
    sm = SpectrogramMasking(16000, 128).to(DEV)
    x = _waves(2, 48000, seed=31)
    lg = _logits(2, 2, 128, 192, seed=32)
    xd, lgd = torch.from_numpy(x).to(DEV), torch.from_numpy(lg).to(DEV)
    one = sm(xd[:1], lgd[:1, 0])
    assert one.shape == (1, 48000) and one.dtype == torch.float32 and one.is_cuda
    ref, bound = _fused_ref_and_bound(_mel(16000), x[:1], lg[:1, :1])
    ok, w, msg = within(one, _t(ref[:, 0]), bound[:, 0], 'SpectrogramMasking [1, 48000]')
    assert ok, msg
    kcheck.note('SpectrogramMasking 48000', w)
    print(f'SpectrogramMasking(16000, 128) on 3 s: worst err / bound {w:.3g}')
    both = sm(xd, lgd)
    assert both.shape == (2, 2, 48000)
    for b in range(2):
        for k in range(2):
            assert torch.equal(sm(xd[b:b + 1], lgd[b:b + 1, k]), both[b:b + 1, k])


def test_mixture_specs_equals_logmel_of_the_summed_and_single_waveforms():
    from deepavfusion_amd.util import audio_transforms as aT
    from deepavfusion_amd.util.separation import mixture_specs
    logmel = aT.LogMelSpectrogram(16000, 128).to(DEV)
    for N in (2, 3):
        w = torch.from_numpy(_waves(2 * N, 4000, seed=N).reshape(2, N, 4000)).to(DEV) * 0.5
        mix_spec, mel_specs = mixture_specs(w, logmel)
        assert mix_spec.shape == (2, 1, 128, 16) and mel_specs.shape == (2, N, 1, 128, 16)
        assert torch.equal(mix_spec, logmel(w.sum(1)))
        for n in range(N):
            assert torch.equal(mel_specs[:, n], logmel(w[:, n].contiguous()))
