"""The audio side of source-separation evaluation (eval_avsrcsep.py) on the device.

``SpectrogramMasking`` is the reference's class of that name (eval_avsrcsep.py:264-277): a predicted mel-domain mask and the
mixture's waveform -> the separated waveform,

    stft = Spectrogram(power=None)(mix);  mask = cat(sigmoid(pred), one zero frame);  mask = einsum('bmt,fm->bft', mask, mel fb)
    InverseSpectrogram(mask * stft)

The reference copies the mask to the host and runs this per sample and per source inside its evaluation loop (:245-254); here the
whole chain is ONE launch of dav_sep_mask_istft (csrc/sep/stft.hip) over a batch of mixtures with K masks each, and the result
stays on the device.  ``mixture_specs`` is the audio side of MixtureVideoDataset.get_sample (datasets.py:357-362).

Not here: the AVSrcSep U-Net head that predicts the masks, and bss_eval_sources (mir_eval) that scores the waveforms."""
import torch

from . import audio_transforms as aT


class SpectrogramMasking(torch.nn.Module):
    """SpectrogramMasking(audio_rate, audio_mels)(waveform_mix, pred_mask), the reference's constructor and call:
    waveform_mix [1, S], pred_mask [1, n_mels, T] -> [1, L] with L = hop * T (T + 1 == S // hop + 1: the mask of the last STFT
    frame is the zero column the reference appends).  Batched: waveform_mix [B, S], pred_mask [B, K, n_mels, T] -> [B, K, L], K
    masks sharing one mixture (the evaluation loop applies two).  Returns device tensors (the reference returns host tensors)."""

    def __init__(self, audio_rate, audio_mels):
        super().__init__()
        self.n_fft = int(audio_rate * 0.05)
        self.hop = int(audio_rate / 64)
        self.spectrogram_t = aT.Spectrogram(n_fft=self.n_fft, hop_length=self.hop, power=None)
        self.inv_spectrogram_t = aT.InverseSpectrogram(n_fft=self.n_fft, hop_length=self.hop)       # the NOLA check of the geometry
        self.mel_spec = aT.MelSpectrogram(sample_rate=audio_rate, n_fft=self.n_fft, hop_length=self.hop, n_mels=audio_mels)

    def forward(self, waveform_mix, pred_mask):
        if not waveform_mix.is_cuda or not pred_mask.is_cuda:
            raise RuntimeError('SpectrogramMasking runs on an MI355X (cuda) device; there is no CPU fallback')
        from ..ops import sep_mask_istft
        if waveform_mix.dim() != 2 or pred_mask.dim() not in (3, 4) or pred_mask.shape[0] != waveform_mix.shape[0]:
            raise ValueError('SpectrogramMasking takes waveform_mix [B, S] with pred_mask [B, n_mels, T] or [B, K, n_mels, T]')
        wave = waveform_mix.detach().to(torch.float32)
        if wave.stride(-1) != 1:
            wave = wave.contiguous()
        logits = pred_mask.detach().to(torch.float32)
        logits = (logits.unsqueeze(1) if pred_mask.dim() == 3 else logits).contiguous()
        m = self.mel_spec
        if m.window.device != wave.device:
            m.to(wave.device)
        out = sep_mask_istft(wave, logits, m.window, m.cos_tab, m.sin_tab, m.fbank, m.band_lo, m.band_hi, self.n_fft, self.hop)
        return out[:, 0] if pred_mask.dim() == 3 else out


def mixture_specs(waveforms, logmel):
    """The audio side of MixtureVideoDataset.get_sample (datasets.py:357-362) for a batch: waveforms [B, N, S] on the device (N
    sources per mixture) and a LogMelSpectrogram -> (mix_spec [B, 1, M, T] of the summed waveform, mel_specs [B, N, 1, M, T] of
    the sources).  The sum is formed on the device and all B * (N + 1) rows go through one dav_logmel launch."""
    if not waveforms.is_cuda:
        raise RuntimeError('mixture_specs runs on an MI355X (cuda) device; there is no CPU fallback')
    if waveforms.dim() != 3:
        raise ValueError('mixture_specs takes waveforms [B, N, S]')
    B, N, S = waveforms.shape
    x = waveforms.to(torch.float32)
    rows = torch.cat((x.sum(1, keepdim=True), x), dim=1)                      # [B, 1 + N, S]: the mixture first
    spec = logmel(rows.view(B * (N + 1), S))                                  # [B (1 + N), 1, M, T]
    spec = spec.view(B, N + 1, *spec.shape[1:])
    return spec[:, 0], spec[:, 1:]
