"""Source-separation audio without a GPU: the float64 restatement (tests/stft_ref.py) against torch.stft / torch.istft and the
reference's masking formula written in torch, the C ABI's declarations and refusals (no pointer is dereferenced), and the module
surface (aT.Spectrogram, aT.InverseSpectrogram, util/separation.py)."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stft_ref as R  # noqa: E402

GEOMS = [(800, 250), (32, 10)]        # the reference's 16 kHz geometry; a small one whose hop does not divide n_fft


def _lengths(n_fft, hop):
    return [n_fft // 2 + 1, 3 * hop - 1, 3 * hop, 3 * hop + 1] + ([48000] if n_fft == 800 else [])


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _torch_stft(x, n_fft, hop):
    return torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, window=torch.hann_window(n_fft, dtype=torch.float64), center=True,
                      pad_mode='reflect', normalized=False, onesided=True, return_complex=True)


def _torch_istft(X, n_fft, hop):
    return torch.istft(X, n_fft, hop_length=hop, window=torch.hann_window(n_fft, dtype=torch.float64), center=True, normalized=False,
                       onesided=True, length=None)


@pytest.mark.parametrize('n_fft,hop', GEOMS)
def test_restatement_equals_torch_stft_and_istft_in_float64(n_fft, hop):
    """stft, istft (of a random complex spectrum whose DC / Nyquist bins carry imaginary parts) and the masking chain agree with
    torch's float64 CPU transforms to 1e-12 relative; the output length is hop (frames - 1)."""
    g = np.random.default_rng(n_fft)
    n_mels, F = 16, n_fft // 2 + 1
    fb = np.maximum(g.normal(size=(F, n_mels)), 0.0)
    for S in _lengths(n_fft, hop):
        x = g.uniform(-1, 1, (2, S))
        frames = S // hop + 1
        X = R.stft(x, n_fft, hop)
        want = _torch_stft(x, n_fft, hop)
        assert X.shape == tuple(want.shape) == (2, F, frames)
        assert _rel(X, want.numpy()) <= 1e-12
        Z = g.normal(size=(2, F, frames)) + 1j * g.normal(size=(2, F, frames))
        y = R.istft(Z, n_fft, hop)
        Zt = torch.from_numpy(Z)
        want_y = _torch_istft(Zt, n_fft, hop)
        assert y.shape == tuple(want_y.shape) == (2, hop * (frames - 1))
        assert _rel(y, want_y.numpy()) <= 1e-12
        assert _rel(R.istft(X, n_fft, hop), x[:, :hop * (frames - 1)]) <= 1e-12                # the round trip is the signal
        # the reference's formula (eval_avsrcsep.py:272-277), per sample and per mask
        logits = 3.0 * g.normal(size=(2, 2, n_mels, frames - 1))
        got = R.mask_istft(x, logits, fb, n_fft, hop)
        assert got.shape == (2, 2, hop * (frames - 1))
        for b in range(2):
            for k in range(2):
                pm = torch.from_numpy(logits[b, k])[None]
                pm = torch.cat((torch.sigmoid(pm), torch.zeros(*pm.shape[:2], 1, dtype=pm.dtype)), dim=2)
                pm = torch.einsum('bmt,fm->bft', pm, torch.from_numpy(fb))
                ref = _torch_istft(pm * want[b:b + 1], n_fft, hop)
                assert _rel(got[b, k], ref[0].numpy()) <= 1e-12


def test_lengths_and_envelope_of_the_reference_geometry():
    from deepavfusion_amd.util import audio_transforms as aT
    assert 250 * (48000 // 250) == 48000 and 250 * (777 // 250) == 750                        # hop (frames - 1)
    env = R.envelope(800, 250, 193)
    assert env.shape == (48000,) and abs(env.min() - 1.0953) < 1e-4
    assert np.array_equal(aT.istft_envelope(800, 250, 193), env)
    m = aT.InverseSpectrogram(800, 250)
    assert 1.0 < m.envelope_min <= env.min()
    y, a = R.istft(np.ones((1, 17, 4)) * (1 + 1j), 32, 10, return_abs=True)
    assert a.shape == y.shape == (1, 30) and bool((a >= np.abs(y) - 1e-12).all())             # the absolute sum dominates


def test_entry_points_are_declared_exported_and_refuse_without_a_gpu():
    """The three names in the header and in SIGNATURES, ABI 9; sizes are judged first (-1), then alignment (-5); the pointers
    are made-up addresses and are never dereferenced."""
    from deepavfusion_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'dav_kernels.h')).read()
    for name in ('dav_stft_c32', 'dav_istft_c32', 'dav_sep_mask_istft'):
        assert name in _lib.SIGNATURES and f'int {name}(' in header
    assert '#define DAV_ABI_VERSION 9 ' in header and _lib.ABI_VERSION == 9
    assert f'enum {{ dav_stft_frames = {ops.STFT_FRAMES} }};' in header and f'enum {{ dav_istft_frames = {ops.ISTFT_FRAMES} }};' in header
    assert 'SRCS += sep/stft.hip' in open(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', 'Makefile')).read()
    assert not any(n.endswith('workspace_bytes') and ('stft' in n or 'sep' in n) for n in _lib.SIGNATURES)
    assert ops.istft_tile(800, 250) == 9 * 250 and ops.istft_tile(400, 125) == 9 * 125 and ops.istft_tile(32, 10) == 90
    assert ops.istft_tile(801, 250) == 0 and ops.istft_tile(800, 30) == 0                    # odd n_fft; the halo alone fills the tile
    lib = _lib.load()
    p, i, l = C.c_void_p, C.c_int, C.c_long
    A = 1 << 20                                                                               # 8-byte aligned made-up addresses

    def stft(wave=A, B=2, S=1000, rs=1000, n_fft=800, hop=250, win=2 * A, ct=3 * A, st=4 * A, spec=5 * A, srs=5):
        return lib.dav_stft_c32(p(wave), i(B), i(S), l(rs), i(n_fft), i(hop), p(win), p(ct), p(st), p(spec), l(srs), p(None))

    def istft(spec=A, srs=5, B=2, frames=5, n_fft=800, hop=250, win=2 * A, ct=3 * A, st=4 * A, out=5 * A, ors=1000):
        return lib.dav_istft_c32(p(spec), l(srs), i(B), i(frames), i(n_fft), i(hop), p(win), p(ct), p(st), p(out), l(ors), p(None))

    def sep(wave=A, B=2, S=1000, rs=1000, lg=6 * A, K=2, n_mels=128, T=4, n_fft=800, hop=250, win=2 * A, ct=3 * A, st=4 * A, fb=7 * A,
            lo=8 * A, hi=9 * A, out=5 * A, ors=1000):
        return lib.dav_sep_mask_istft(p(wave), i(B), i(S), l(rs), p(lg), i(K), i(n_mels), i(T), i(n_fft), i(hop), p(win), p(ct), p(st),
                                      p(fb), p(lo), p(hi), p(out), l(ors), p(None))

    for name in ('dav_stft_c32', 'dav_istft_c32', 'dav_sep_mask_istft'):                      # all-zero arguments
        args = [t(0) if t is not p else p(None) for t in _lib.SIGNATURES[name]]
        assert getattr(lib, name)(*args) == -1
    # valid sizes otherwise: S == n_fft / 2 (torch refuses such a reflect pad), odd n_fft, hop <= 0, frames < 2, short strides
    assert stft(S=400, rs=400) == -1 and sep(S=400, rs=400, T=1) == -1
    assert stft(n_fft=801) == -1 and istft(n_fft=801) == -1 and sep(n_fft=801) == -1
    assert stft(hop=0) == -1 and istft(hop=0) == -1 and sep(hop=-1) == -1
    assert stft(S=401, rs=401, hop=500) == -1 and istft(frames=1) == -1                      # one frame only
    assert stft(B=0) == -1 and istft(B=0) == -1 and sep(B=0) == -1 and sep(K=0) == -1 and sep(n_mels=0) == -1
    assert stft(rs=999) == -1 and stft(srs=4) == -1 and istft(srs=4) == -1 and istft(ors=999) == -1 and sep(ors=999) == -1
    assert stft(wave=None) == -1 and stft(spec=None) == -1 and istft(out=None) == -1 and sep(lg=None) == -1 and sep(fb=None) == -1
    assert sep(T=3) == -1 and sep(T=5) == -1                                                  # T + 1 != frames
    assert istft(hop=30, ors=200) == -1 and sep(S=1000, hop=30, T=33, ors=1000) == -1        # 2 h + 1 halo frames >= the tile
    assert istft(n_fft=8000, hop=2500, ors=10000) == -1                                       # 12 frames of 8000 samples: beyond the LDS
    # alignment, judged after the sizes: the complex pointer at 4 mod 8, float pointers at 2 mod 4
    assert stft(spec=5 * A + 4) == -5 and istft(spec=A + 4) == -5
    assert stft(wave=A + 2) == -5 and stft(win=2 * A + 1) == -5 and istft(out=5 * A + 2) == -5 and istft(ct=3 * A + 2) == -5
    assert sep(wave=A + 2) == -5 and sep(lg=6 * A + 1) == -5 and sep(out=5 * A + 2) == -5 and sep(lo=8 * A + 2) == -5
    assert stft(spec=5 * A + 4, n_fft=801) == -1                                              # sizes first


def test_module_surface():
    from deepavfusion_amd import ops
    from deepavfusion_amd.util import audio_transforms as aT
    from deepavfusion_amd.util import separation
    with pytest.raises(ValueError, match='MelSpectrogram'):
        aT.Spectrogram(n_fft=800, hop_length=250, power=2.0)
    with pytest.raises(ValueError, match='MelSpectrogram'):
        aT.Spectrogram()                                                                      # torchaudio's default power is 2
    with pytest.raises(ValueError, match='overlap'):
        aT.InverseSpectrogram(16, 16)                                                         # the Hann envelope is 0 at the frame joins
    s, inv = aT.Spectrogram(800, 250, power=None), aT.InverseSpectrogram(800, 250)
    assert (s.n_fft, s.hop, inv.n_fft, inv.hop) == (800, 250, 800, 250) and aT.Spectrogram(400, power=None).hop == 200
    assert not s.state_dict() and not inv.state_dict()                                        # tables are non-persistent
    mel = aT.MelSpectrogram(16000, 800, 250, 128)
    for name in ('window', 'cos_tab', 'sin_tab'):                                             # one set of tables for all three
        assert torch.equal(getattr(s, name), getattr(mel, name)) and torch.equal(getattr(inv, name), getattr(mel, name))
    w64, c64, s64 = R.tables64(800)
    assert np.array_equal(mel.window.numpy(), w64.astype(np.float32)) and np.array_equal(mel.cos_tab.numpy(), c64.astype(np.float32))
    assert np.array_equal(mel.sin_tab.numpy(), s64.astype(np.float32))
    spec = torch.zeros(1, 401, 5, dtype=torch.complex64)
    with pytest.raises(ValueError, match='length'):
        inv(spec, length=1000)
    with pytest.raises(ValueError, match='length'):
        inv(spec, 1000)
    x = torch.zeros(1, 1000)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        s(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        inv(spec)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.stft(x, mel.window, mel.cos_tab, mel.sin_tab, 800, 250)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.istft(spec, mel.window, mel.cos_tab, mel.sin_tab, 800, 250)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sep_mask_istft(x, torch.zeros(1, 1, 128, 4), mel.window, mel.cos_tab, mel.sin_tab, mel.fbank, mel.band_lo, mel.band_hi, 800, 250)
    sm = separation.SpectrogramMasking(16000, 128)
    assert (sm.n_fft, sm.hop) == (800, 250) and tuple(sm.mel_spec.fbank.shape) == (401, 128)
    assert (separation.SpectrogramMasking(8000, 64).n_fft, separation.SpectrogramMasking(8000, 64).hop) == (400, 125)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        sm(x, torch.zeros(1, 128, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        separation.mixture_specs(torch.zeros(2, 2, 1000), aT.LogMelSpectrogram(16000, 128))


def test_kernel_source_hash_leaves_the_separation_kernels_out():
    """csrc/sep/ sits outside the hash the PMC records under profiles/ carry."""
    from deepavfusion_amd import _lib
    assert os.path.isfile(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', 'sep', 'stft.hip'))
    hashed = glob.glob(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', '*.hip')) + glob.glob(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', '*.h'))
    assert not any('stft' in os.path.basename(f) or os.sep + 'sep' + os.sep in f for f in hashed)
    assert len(_lib.kernel_source_hash()) == 16
