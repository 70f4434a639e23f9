"""Float64 restatement of the source-separation audio chain (eval_avsrcsep.py:264-277 of the reference) for the tests of
csrc/sep/stft.hip, written from the definitions with dense DFT matrices, not from the package's code:

    frames   x_t[n] = xpad[t hop + n] w[n],  xpad = x reflected by N/2 at each end,  t = 0 .. S // hop         (torch.stft, center)
    stft     X_t[k] = sum_n x_t[n] (cos(2 pi k n / N) - i sin(2 pi k n / N)),  k = 0 .. N/2
    istft    x_t[n] = (1/N) sum_k c_k (Re X_t[k] cos(2 pi k n / N) - Im X_t[k] sin(2 pi k n / N)),  c = 1, 2, .., 2, 1 and the
             imaginary parts of k = 0 and k = N/2 ignored (irfft);  y[p] = sum_t w[p - t hop] x_t[p - t hop];
             env[p] = sum_t w[p - t hop]^2;  out[j] = y[j + N/2] / env[j + N/2],  j = 0 .. hop (frames - 1) - 1    (torch.istft)
    masking  M = einsum('bkmt,fm->bkft', cat(sigmoid(logits), one zero frame), fb);  out = istft(M stft(x))

Every function takes the window and the cos / sin tables (indexed at (k n) mod N) as arguments: the float64 ones by default, or
a kernel's own fp32 tables widened, so that table rounding is not charged to the kernel.  ``return_abs`` also returns the sum of
the absolute terms, the scale of a rounding bound (the pattern of tests/resample_ref.py)."""
import numpy as np


def tables64(n_fft):
    """(window, cos_tab, sin_tab) in float64: periodic Hann and cos / sin(2 pi n / N)"""
    a = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    return 0.5 - 0.5 * np.cos(a), np.cos(a), np.sin(a)


def _tabs(n_fft, window, cos_tab, sin_tab):
    w, c, s = tables64(n_fft)
    return (np.asarray(t, np.float64) if t is not None else d for t, d in ((window, w), (cos_tab, c), (sin_tab, s)))


def _dft_mats(n_fft, cos_tab, sin_tab):
    """C[k, n], S[k, n] = cos_tab / sin_tab[(k n) mod N] for k = 0 .. N/2"""
    idx = (np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :]) % n_fft
    return cos_tab[idx], sin_tab[idx]


def frames_of(x, n_fft, hop):
    """[.., S] -> the frames of the reflect-padded signal, [.., S // hop + 1, n_fft] (float64)"""
    x = np.asarray(x, np.float64)
    S = x.shape[-1]
    assert S > n_fft // 2, 'the reflect pad needs S > n_fft / 2'
    p = np.arange(-(n_fft // 2), S + n_fft // 2)
    p = np.where(p < 0, -p, p)
    p = np.where(p >= S, 2 * (S - 1) - p, p)
    xpad = x[..., p]
    idx = np.arange(S // hop + 1)[:, None] * hop + np.arange(n_fft)[None, :]
    return xpad[..., idx]


def stft(x, n_fft, hop, window=None, cos_tab=None, sin_tab=None, return_abs=False):
    """x [.., S] -> complex128 [.., N/2 + 1, frames]; with ``return_abs`` also sum_n |x_t[n]| as [.., 1, frames] (|cos|, |sin| <= 1:
    the bound of either part of every bin of the frame)"""
    w, c, s = _tabs(n_fft, window, cos_tab, sin_tab)
    C, Sn = _dft_mats(n_fft, c, s)
    fr = frames_of(x, n_fft, hop) * w                              # [.., T, N]
    X = (fr @ C.T - 1j * (fr @ Sn.T)).swapaxes(-1, -2)             # [.., K, T]
    if not return_abs:
        return X
    return X, np.abs(fr).sum(-1)[..., None, :]


def envelope(n_fft, hop, frames, window=None):
    """sum_t w[p - t hop]^2 trimmed by N/2 at each end, [hop (frames - 1)]"""
    w, _, _ = _tabs(n_fft, window, None, None)
    env = np.zeros(hop * (frames - 1) + n_fft)
    for t in range(frames):
        env[t * hop:t * hop + n_fft] += w * w
    return env[n_fft // 2:n_fft // 2 + hop * (frames - 1)]


def _overlap_add(fr, n_fft, hop):
    """[.., T, N] frames -> [.., hop (T - 1)]: added at t hop, trimmed by N/2 at each end (no envelope)"""
    T = fr.shape[-2]
    y = np.zeros(fr.shape[:-2] + (hop * (T - 1) + n_fft,))
    for t in range(T):
        y[..., t * hop:t * hop + n_fft] += fr[..., t, :]
    return y[..., n_fft // 2:n_fft // 2 + hop * (T - 1)]


def istft_abs(re_mag, im_mag, n_fft, hop, window=None, cos_tab=None, sin_tab=None):
    """The inverse map with absolute coefficients: magnitudes [.., N/2 + 1, frames] of the real and imaginary parts ->
    (1 / env[j]) sum_t w sum_k c_k (re_mag |cos| + im_mag |sin|) / N, [.., hop (frames - 1)]: the sum of the absolute terms of an
    output sample, and the map that carries a per-bin error to the output."""
    w, c, s = _tabs(n_fft, window, cos_tab, sin_tab)
    C, Sn = _dft_mats(n_fft, c, s)
    ck = np.full(n_fft // 2 + 1, 2.0)
    ck[0] = ck[-1] = 1.0
    re = np.asarray(re_mag, np.float64).swapaxes(-1, -2) * ck      # [.., T, K]
    im = np.asarray(im_mag, np.float64).swapaxes(-1, -2) * ck
    im[..., 0] = im[..., -1] = 0.0
    fr = (re @ np.abs(C) + im @ np.abs(Sn)) / n_fft * np.abs(w)
    return _overlap_add(fr, n_fft, hop) / envelope(n_fft, hop, fr.shape[-2], w)


def istft(X, n_fft, hop, window=None, cos_tab=None, sin_tab=None, return_abs=False):
    """complex [.., N/2 + 1, frames] -> float64 [.., hop (frames - 1)]; with ``return_abs`` also istft_abs(|Re X|, |Im X|)"""
    w, c, s = _tabs(n_fft, window, cos_tab, sin_tab)
    C, Sn = _dft_mats(n_fft, c, s)
    X = np.asarray(X, np.complex128)
    ck = np.full(n_fft // 2 + 1, 2.0)
    ck[0] = ck[-1] = 1.0
    re = X.real.swapaxes(-1, -2) * ck                              # [.., T, K]
    im = X.imag.swapaxes(-1, -2) * ck
    im[..., 0] = im[..., -1] = 0.0                                 # irfft ignores them
    fr = (re @ C - im @ Sn) / n_fft * w
    out = _overlap_add(fr, n_fft, hop) / envelope(n_fft, hop, fr.shape[-2], w)
    if not return_abs:
        return out
    return out, istft_abs(np.abs(X.real), np.abs(X.imag), n_fft, hop, w, c, s)


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def mel_mask(logits, fb):
    """logits [.., n_mels, T], fb [n_freqs, n_mels] -> M [.., n_freqs, T + 1] = fb . cat(sigmoid(logits), one zero frame); fb and the
    sigmoid are >= 0, so M is also the sum of its absolute terms"""
    sg = sigmoid(logits)
    sg = np.concatenate([sg, np.zeros(sg.shape[:-1] + (1,))], -1)
    return np.einsum('...mt,fm->...ft', sg, np.asarray(fb, np.float64))


def mask_istft(x, logits, fb, n_fft, hop, window=None, cos_tab=None, sin_tab=None):
    """x [B, S], logits [B, K, n_mels, T] -> [B, K, hop T]: the reference's SpectrogramMasking for K masks per mixture"""
    X = stft(x, n_fft, hop, window, cos_tab, sin_tab)              # [B, F, T + 1]
    M = mel_mask(logits, fb)                                       # [B, K, F, T + 1]
    return istft(M * X[:, None], n_fft, hop, window, cos_tab, sin_tab)
