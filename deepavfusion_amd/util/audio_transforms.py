"""Audio transforms of the reference (util/audio_transforms.py:8-35 + the torchaudio MelSpectrogram it composes,
train.py:50-54) with the spectrogram computed ON THE GPU from raw waveforms instead of in CPU
data-loader workers.  Same class names and constructor arguments:

    aT.Compose([aT.Pad(rate=…, dur=…), aT.RandomVol(), aT.MelSpectrogram(sample_rate=…, n_fft=…, hop_length=…, n_mels=…), aT.Log()])

works on a batch of waveforms [B, S] (or [B, 1, S] / [1, S]) resident on the device and yields [B, 1, n_mels, frames];
``LogMelSpectrogram`` is the fused form (one kernel, incl. the ``[:, :, :-1]`` of datasets.py:242).
Pad / RandomVol are index / scale plumbing (torch); the STFT, mel projection and log run in csrc/mel.hip.
``Resample`` is the sinc resampler the reference's loader applies to every track (datasets.py:176-181), in csrc/data/resample.hip;
``PrepareWaveform`` is Resample -> Pad -> RandomVol in that kernel's one launch (data.audio_resample=gpu).
``Spectrogram(power=None)`` / ``InverseSpectrogram`` are the complex STFT and its inverse that the reference's source-separation
evaluation composes (eval_avsrcsep.py:268-269), in csrc/sep/stft.hip; util/separation.py holds the fused masking chain."""
import math
import random

import numpy as np
import torch

from .. import _lib
from ..ops import _ptr, _stream


class Compose(torch.nn.Module):
    def __init__(self, transforms):
        super().__init__()
        self.transforms = list(transforms)

    def forward(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class RandomVol(torch.nn.Module):
    """util/audio_transforms.py:8-17: a random gain in dB, then clamp to [-1, 1].  The reference applies this transform per
    SAMPLE inside the dataset: ONE draw per call, whatever the waveform's shape ([samples] or [channels, samples] — a stereo
    clip gets one gain for both channels).  ``per_sample=True`` (set by the GPU front-end of this package, which transforms a
    whole batch [B, samples] at once) draws one gain per row of the first dimension instead — what B per-sample calls would
    have drawn.  The mode is explicit: [channels, samples] and [B, samples] cannot be told apart by shape."""
    def __init__(self, gain=(-6, 6), per_sample=False):
        super().__init__()
        self.gain = gain
        self.per_sample = per_sample

    def forward(self, waveform):
        if self.per_sample and waveform.dim() >= 2:
            g = torch.tensor([random.uniform(self.gain[0], self.gain[1]) for _ in range(waveform.shape[0])],
                             dtype=waveform.dtype, device=waveform.device).view(-1, *([1] * (waveform.dim() - 1)))
            return torch.clamp(waveform * torch.pow(10.0, g / 20.0), -1, 1)
        g = random.uniform(self.gain[0], self.gain[1])
        return torch.clamp(waveform * (10.0 ** (g / 20.0)), -1, 1)


class Pad(torch.nn.Module):
    """util/audio_transforms.py:19-27 (note the reference's positional order: dur, rate)."""
    def __init__(self, dur, rate):
        super().__init__()
        self.samples = int(dur * rate)

    def forward(self, waveform):
        while waveform.shape[-1] < self.samples:
            waveform = torch.cat((waveform, torch.flip(waveform, dims=(-1,))), dim=-1)
        return waveform[..., :self.samples]


def resample_geometry(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """(o, n, width, taps per phase) of torchaudio's sinc resampler: the rates reduced by their gcd, the filter's half width in
    input samples, and K = 2 width + o."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1 or lowpass_filter_width < 1:
        raise ValueError('rates and the filter width must be positive')
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    width = int(math.ceil(lowpass_filter_width * o / (min(o, n) * rolloff)))
    return o, n, width, 2 * width + o


def resample_taps(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The fp32 tap table [n, K] of torchaudio.functional.resample (resampling_method='sinc_interp_hann', its default),
    restated from its published source and evaluated in float64: phase p, tap k weighs sinc(t) cos^2(pi t / (2 lpw)) base / o
    at t = clamp((k - width) / o - p / n, +-lpw / base) * base with base = min(o, n) rolloff."""
    o, n, width, K = resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    base = min(o, n) * rolloff
    idx = (np.arange(K, dtype=np.float64) - width) / o
    t = (-np.arange(n, dtype=np.float64)[:, None] / n + idx[None, :]) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    safe = np.where(t == 0, 1.0, t)
    sinc = np.where(t == 0, 1.0, np.sin(safe) / safe)
    return (sinc * window * (base / o)).astype(np.float32)


def resample_tile(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """Frames (of o input samples, n output samples) one workgroup of the resampling kernel owns for this pair of rates: outputs
    j and j + 1 with (j + 1) % (n * tile) == 0 come from different workgroups (asked of the library, not restated)."""
    from ..ops import wave_resample_tile
    o, n, width, _ = resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    return wave_resample_tile(o, n, width)


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults (windowed sinc, Hann, lowpass_filter_width 6,
    rolloff 0.99) — what the reference's loader applies to every track (datasets.py:176-181) — on dav_wave_resample: waveforms
    [B, S] (or [B, 1, S] / [1, S]; fp32 or int16, which is scaled by 2^-15) on the device -> fp32 with ceil(n S / o) samples per
    row.  Equal rates return the input object, no launch.  The table is computed in float64 (numpy) and held in fp32."""

    def __init__(self, orig_freq=16000, new_freq=16000, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann'):
        super().__init__()
        if resampling_method not in ('sinc_interp_hann', 'sinc_interpolation'):
            raise NotImplementedError(f'resampling_method={resampling_method}: only the Hann-windowed sinc (torchaudio\'s default) '
                                      'is on the MI355X path')
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.lowpass_filter_width, self.rolloff = lowpass_filter_width, rolloff
        self.o, self.n, self.width, self.ntaps = resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
        if self.orig_freq != self.new_freq:
            from ..ops import RESAMPLE_MAX_RATIO
            if max(self.o, self.n) > RESAMPLE_MAX_RATIO:
                raise ValueError(f'{orig_freq} -> {new_freq} Hz reduces to {self.o} : {self.n}; the kernel takes ratios up to '
                                 f'{RESAMPLE_MAX_RATIO}')
            taps = torch.from_numpy(resample_taps(orig_freq, new_freq, lowpass_filter_width, rolloff))
            self.register_buffer('taps', taps, persistent=False)                              # [n, K], torchaudio's layout
            self.register_buffer('taps_kn', taps.t().contiguous(), persistent=False)          # [K, n], the kernel's

    def out_samples(self, samples):
        return -(-self.n * int(samples) // self.o)

    def _rows(self, waveform):
        if not waveform.is_cuda:
            raise RuntimeError('the resampler runs on an MI355X (cuda) device; there is no CPU fallback')
        if waveform.dtype not in (torch.float32, torch.int16):
            waveform = waveform.to(torch.float32)
        x = waveform.reshape(-1, waveform.shape[-1]) if waveform.dim() != 2 else waveform
        if x.stride(-1) != 1:
            x = x.contiguous()
        if self.orig_freq != self.new_freq and self.taps_kn.device != x.device:
            self.to(x.device)
        return x

    def _launch(self, x, out_len, gain, clamp):
        from ..ops import wave_resample
        return wave_resample(x, self.taps_kn, self.o, self.n, self.width, out_len=out_len, gain=gain, clamp=clamp)

    def forward(self, waveform):
        if self.orig_freq == self.new_freq:
            return waveform
        x = self._rows(waveform)
        y = self._launch(x, self.out_samples(x.shape[-1]), None, False)
        return y.view(*waveform.shape[:-1], y.shape[-1])


class PrepareWaveform(Resample):
    """Compose([Resample(orig_freq, new_freq), Pad(dur, new_freq), RandomVol(gain, per_sample=True)]) in ONE launch: the mirror
    padding, the gain and the clamp are the resampling kernel's epilogue.  The gains are drawn and converted exactly as RandomVol
    does (random.uniform once per row in row order, torch.pow(10, g / 20) on an fp32 device tensor), so under the same
    random.seed the two forms agree bit for bit.  ``gain=None``: no gain and no clamp (the probe's eval transform).  With equal
    rates nothing is launched: Pad and RandomVol run as they are.  -> fp32 [B, int(dur * new_freq)] (leading dims kept)."""

    def __init__(self, orig_freq, new_freq, dur, gain=(-6, 6), lowpass_filter_width=6, rolloff=0.99):
        super().__init__(orig_freq, new_freq, lowpass_filter_width=lowpass_filter_width, rolloff=rolloff)
        self.samples = int(dur * self.new_freq)
        self.gain = gain
        self._pad = Pad(dur, self.new_freq)
        self._vol = RandomVol(gain, per_sample=True) if gain is not None else None

    def forward(self, waveform):
        if self.orig_freq == self.new_freq:
            if not waveform.is_cuda:
                raise RuntimeError('the waveform front-end runs on an MI355X (cuda) device; there is no CPU fallback')
            x = waveform if waveform.dtype == torch.float32 else waveform.to(torch.float32) * (1.0 / 32768.0 if waveform.dtype == torch.int16 else 1.0)
            x = self._pad(x)
            return self._vol(x) if self._vol is not None else x
        x = self._rows(waveform)
        g = None
        if self.gain is not None:
            db = torch.tensor([random.uniform(self.gain[0], self.gain[1]) for _ in range(x.shape[0])], dtype=torch.float32, device=x.device)
            g = torch.pow(10.0, db / 20.0)
        y = self._launch(x, self.samples, g, self.gain is not None)
        return y.view(*waveform.shape[:-1], self.samples)


def _fbank_htk(n_freqs, f_min, f_max, n_mels, sample_rate):
    all_freqs = np.linspace(0, sample_rate // 2, n_freqs)
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    m_pts = np.linspace(mel(f_min), mel(f_max), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    return np.maximum(0.0, np.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))


class MelSpectrogram(torch.nn.Module):
    """torchaudio.transforms.MelSpectrogram(sample_rate, n_fft, hop_length=…, n_mels=…) with its defaults (win_length = n_fft,
    periodic Hann, power 2, centre / reflect padding, HTK mel scale, no filter normalisation) on dav_logmel."""

    def __init__(self, sample_rate=16000, n_fft=400, hop_length=None, n_mels=128, f_min=0.0, f_max=None, log_eps=None, drop_last=False):
        super().__init__()
        self.sample_rate, self.n_fft, self.hop, self.n_mels = sample_rate, n_fft, hop_length or n_fft // 2, n_mels
        self.log_eps, self.drop_last = log_eps, drop_last
        fb = _fbank_htk(n_fft // 2 + 1, f_min, f_max if f_max is not None else sample_rate / 2.0, n_mels, sample_rate)
        nz = fb > 0
        lo = np.where(nz.any(0), nz.argmax(0), 0).astype(np.int32)
        hi = np.where(nz.any(0), fb.shape[0] - nz[::-1].argmax(0), 0).astype(np.int32)
        _register_dft_tables(self, n_fft)
        self.register_buffer('fbank', torch.from_numpy(fb).float().contiguous(), persistent=False)
        self.register_buffer('band_lo', torch.from_numpy(lo), persistent=False)
        self.register_buffer('band_hi', torch.from_numpy(hi), persistent=False)

    def forward(self, waveform):
        if not waveform.is_cuda:
            raise RuntimeError('the log-mel front-end runs on an MI355X (cuda) device; there is no CPU fallback')
        x = waveform.to(torch.float32)
        if x.dim() == 3:
            x = x.reshape(-1, x.shape[-1])
        x = x.contiguous()
        if self.window.device != x.device:
            self.to(x.device)
        B, S = x.shape
        frames = S // self.hop + 1 - (1 if self.drop_last else 0)
        out = torch.empty(B, 1, self.n_mels, frames, dtype=torch.float32, device=x.device)
        lib = _lib.load()
        _lib.check(lib.dav_logmel(_ptr(x), B, S, self.n_fft, self.hop, self.n_mels, _ptr(self.window), _ptr(self.cos_tab),
                                  _ptr(self.sin_tab), _ptr(self.fbank), _ptr(self.band_lo), _ptr(self.band_hi),
                                  float(self.log_eps if self.log_eps is not None else 0.0), int(self.log_eps is not None),
                                  int(self.drop_last), _ptr(out), _stream()), 'dav_logmel')
        return out


def _register_dft_tables(module, n_fft):
    """the periodic Hann window and the exact cos / sin tables of the DFT kernels, float64 values held in fp32 — MelSpectrogram's"""
    n = np.arange(n_fft, dtype=np.float64)
    module.register_buffer('window', torch.from_numpy(0.5 - 0.5 * np.cos(2.0 * math.pi * n / n_fft)).float(), persistent=False)
    module.register_buffer('cos_tab', torch.from_numpy(np.cos(2.0 * math.pi * n / n_fft)).float(), persistent=False)
    module.register_buffer('sin_tab', torch.from_numpy(np.sin(2.0 * math.pi * n / n_fft)).float(), persistent=False)


def _spec_geometry(n_fft, hop_length):
    n_fft = int(n_fft)
    hop = int(hop_length) if hop_length is not None else n_fft // 2          # torchaudio: win_length = n_fft, hop = win_length // 2
    if n_fft < 2 or n_fft % 2 or hop < 1:
        raise ValueError(f'n_fft={n_fft}, hop_length={hop}: the DFT kernels take an even n_fft and a positive hop')
    return n_fft, hop


class Spectrogram(torch.nn.Module):
    """torchaudio.transforms.Spectrogram(n_fft, hop_length=…, power=None) with its defaults (win_length = n_fft, periodic Hann,
    centre / reflect padding, one-sided, not normalised) — the complex STFT of eval_avsrcsep.py:268 — on dav_stft_c32:
    waveforms [..., S] on the device -> complex64 [..., n_fft / 2 + 1, S / hop + 1].  Only ``power=None``: the power
    spectrogram exists on the device as MelSpectrogram's first stage and is not exported on its own."""

    def __init__(self, n_fft=400, hop_length=None, power=2.0):
        super().__init__()
        if power is not None:
            raise ValueError(f'Spectrogram(power={power}): only power=None (the complex STFT) is on the MI355X path; the power '
                             'spectrogram is the first stage of MelSpectrogram')
        self.n_fft, self.hop = _spec_geometry(n_fft, hop_length)
        self.power = None
        _register_dft_tables(self, self.n_fft)

    def forward(self, waveform):
        if not waveform.is_cuda:
            raise RuntimeError('the STFT runs on an MI355X (cuda) device; there is no CPU fallback')
        from ..ops import stft
        x = waveform.to(torch.float32)
        x = x.reshape(-1, x.shape[-1])
        if x.stride(-1) != 1:
            x = x.contiguous()
        if self.window.device != x.device:
            self.to(x.device)
        spec = stft(x, self.window, self.cos_tab, self.sin_tab, self.n_fft, self.hop)
        return spec.view(*waveform.shape[:-1], *spec.shape[1:])


def istft_envelope(n_fft, hop, frames):
    """sum_t w[p - t hop]^2 of the periodic Hann window over ``frames`` frames, trimmed by n_fft / 2 at each end (float64):
    what torch.istft divides by, [hop * (frames - 1)]"""
    w2 = (0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(n_fft, dtype=np.float64) / n_fft)) ** 2
    env = np.zeros(hop * (frames - 1) + n_fft)
    for t in range(frames):
        env[t * hop:t * hop + n_fft] += w2
    return env[n_fft // 2:n_fft // 2 + hop * (frames - 1)]


class InverseSpectrogram(torch.nn.Module):
    """torchaudio.transforms.InverseSpectrogram(n_fft, hop_length=…) with its defaults — torch.istft(center=True,
    normalized=False, onesided=True), eval_avsrcsep.py:269 — on dav_istft_c32: complex64 [..., n_fft / 2 + 1, frames] on the
    device -> fp32 [..., hop * (frames - 1)].  ``length`` is not supported (the reference never passes one).  The constructor
    makes torch's NOLA check once for the geometry: the envelope of the overlapped squared windows, trimmed, must stay above
    1e-11 (its interior is periodic in hop, so the frames a full window spans decide it for every length)."""

    def __init__(self, n_fft=400, hop_length=None):
        super().__init__()
        self.n_fft, self.hop = _spec_geometry(n_fft, hop_length)
        env = istft_envelope(self.n_fft, self.hop, 2 * (-(-self.n_fft // self.hop)) + 2)
        two = istft_envelope(self.n_fft, self.hop, 2)                        # the shortest signal: both ends at once
        self.envelope_min = float(min(env.min(), two.min()))
        if not self.envelope_min > 1e-11:
            raise ValueError(f'InverseSpectrogram(n_fft={self.n_fft}, hop_length={self.hop}): the window overlap-add envelope '
                             f'reaches {self.envelope_min:.3g} (torch.istft: "window overlap add min" must exceed 1e-11)')
        _register_dft_tables(self, self.n_fft)

    def forward(self, spec, length=None):
        if length is not None:
            raise ValueError('InverseSpectrogram: length is not supported; the output has hop * (frames - 1) samples')
        if not spec.is_cuda:
            raise RuntimeError('the inverse STFT runs on an MI355X (cuda) device; there is no CPU fallback')
        from ..ops import istft
        if spec.dtype != torch.complex64:
            spec = spec.to(torch.complex64)
        x = spec.reshape(-1, *spec.shape[-2:]).contiguous()
        if self.window.device != x.device:
            self.to(x.device)
        y = istft(x, self.window, self.cos_tab, self.sin_tab, self.n_fft, self.hop)
        return y.view(*spec.shape[:-2], y.shape[-1])


class Log(torch.nn.Module):
    """util/audio_transforms.py:29-35: log10(spec + eps)."""
    def __init__(self, eps=1e-7):
        super().__init__()
        self.eps = eps

    def forward(self, spec):
        x = spec.contiguous()
        y = torch.empty_like(x)
        _lib.check(_lib.load().dav_log10_eps(_ptr(x), float(self.eps), x.numel(), _ptr(y), _stream()), 'dav_log10_eps')
        return y


class LogMelSpectrogram(MelSpectrogram):
    """MelSpectrogram -> Log -> [:, :, :-1] (train.py:50-54, datasets.py:242) in ONE kernel: waveforms [B, S] -> [B, 1, n_mels, S // hop]."""
    def __init__(self, sample_rate=16000, n_mels=128, eps=1e-7):
        super().__init__(sample_rate=sample_rate, n_fft=int(sample_rate * 0.05), hop_length=int(sample_rate / 64), n_mels=n_mels,
                         log_eps=eps, drop_last=True)
