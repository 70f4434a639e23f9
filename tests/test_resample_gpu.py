"""The audio resampler on the device: dav_wave_resample elementwise against the float64 restatement (tests/resample_ref.py) fed
the module's own fp32 table, int16 against fp32 input, the fused PrepareWaveform against the composed modules bit for bit, a
clip-shard set stored at 8 kHz through ClipShards -> PrepareWaveform -> LogMelSpectrogram against the oracle, and train.py's
worker on such a set."""
import builtins
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kcheck  # noqa: E402
import resample_ref as R  # noqa: E402
from kcheck import Guarded, sum_bound, within  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'

PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (8000, 16000)]


def _module(orig, new):
    from deepavfusion_amd.util import audio_transforms as aT
    return aT.Resample(orig, new).to(DEV)


def _waves(B, L, seed):
    """noise in [-1, 1] with a tone on top of every second row (fp32)"""
    g = np.random.default_rng(seed)
    x = g.uniform(-1, 1, (B, L))
    x[::2] = 0.5 * x[::2] + 0.5 * np.sin(2 * np.pi * 0.013 * np.arange(L))[None]
    return x.astype(np.float32)


def _run(m, x, out_len=None, gain=None, clamp=False, in_pad=0):
    """x numpy [B, L] (fp32 or int16) -> the kernel's output in a poisoned, guard-banded buffer with a padded row stride; the input
    rows sit ``in_pad`` elements apart from dense."""
    from deepavfusion_amd import ops
    B, L = x.shape
    src = torch.zeros(B, L + in_pad, dtype=torch.from_numpy(x).dtype, device=DEV)
    src[:, :L] = torch.from_numpy(x).to(DEV)
    out_len = m.out_samples(L) if out_len is None else out_len
    out = Guarded(B, out_len, torch.float32, ld=out_len + 3, device=DEV, fill='poison')
    ops.wave_resample(src[:, :L], m.taps_kn, m.o, m.n, m.width, out_len=out_len, gain=gain, clamp=clamp, out=out.t)
    torch.cuda.synchronize()
    n_stray, where = out.stray()
    assert n_stray == 0, where
    return out.t


def _lengths(m, T):
    o = m.o
    return sorted({L for L in (1, 7, o - 1, o, o + 1, T * o - 1, T * o, T * o + 1, 3 * T * o + 5) if L >= 1})


@pytest.mark.parametrize('orig,new', PAIRS)
def test_kernel_matches_the_float64_restatement_elementwise(orig, new):
    """Every output within sum_bound(sum_k |taps x|, taps + 2, ref) of the float64 restatement fed the module's own fp32 table
    (widened: tap rounding is not in the error) — the bound of an fp32 sum of K terms in any order plus the stored value's
    rounding, derived, not fitted.  Lengths 1, 7, o - 1, o, o + 1 (the edges, L < width, one frame), T o - 1, T o, T o + 1 for the
    kernel's frames per workgroup T (asked of the library) and 3 T o + 5 (several workgroups, a partial last one); B = 1, and B = 3
    with input rows strided apart; outputs poisoned, guard-banded, row stride padded.
    Worst err / bound measured on an MI355X: 0.012 at 44100 -> 16000, 0.14 at 48000 -> 16000, 0.011 at 22050 -> 16000 and
    0.18 at 8000 -> 16000 (a k-ordered fmaf chain errs like a random walk; the bound allows for the worst case of any order)."""
    from deepavfusion_amd.util import audio_transforms as aT
    m = _module(orig, new)
    T = aT.resample_tile(orig, new)
    assert T >= 1
    taps = m.taps.cpu().numpy().astype(np.float64)
    worst = 0.0
    for L in _lengths(m, T):
        for B, in_pad in ((1, 0), (3, 5)):
            x = _waves(B, L, seed=L * 7 + B)
            got = _run(m, x, in_pad=in_pad)
            ref, mag = R.resample(x, taps, m.o, m.n, m.width, return_abs=True)
            assert got.shape == ref.shape == (B, -(-m.n * L // m.o))
            ref, mag = torch.from_numpy(ref).to(DEV), torch.from_numpy(mag).to(DEV)
            ok, w, msg = within(got, ref, sum_bound(mag, m.ntaps + 2, ref), f'{orig}->{new} L={L} B={B}')
            assert ok, msg
            worst = max(worst, w)
    kcheck.note(f'wave_resample {orig}->{new}', worst)
    print(f'wave_resample {orig} -> {new} (o {m.o}, n {m.n}, taps {m.ntaps}, T {T}): worst err / bound {worst:.3g}')


@pytest.mark.parametrize('orig,new', [(44100, 16000), (8000, 16000)])
def test_mirror_gain_and_clamp_of_the_epilogue(orig, new):
    """out[j] = clamp(gain_b r_b[m(j)]) for out_len > R (several periods of the mirror, a cut inside one) and out_len < R, against
    the float64 restatement mirrored with resample_ref.mirror_map: the bound of r scaled by the gain, plus one rounding of the
    product (one more term).  The clamp is the last step and exact: the clamped call equals the unclamped one clamped by torch."""
    from deepavfusion_amd.util import audio_transforms as aT
    m = _module(orig, new)
    T = aT.resample_tile(orig, new)
    L = T * m.o + 3
    Rn = m.out_samples(L)
    x = 1.5 * _waves(3, L, seed=11)
    taps = m.taps.cpu().numpy().astype(np.float64)
    gain = torch.tensor([0.5, 1.7, 1.0], dtype=torch.float32, device=DEV)
    r, mag = R.resample(x, taps, m.o, m.n, m.width, return_abs=True)
    for out_len in (5 * Rn + 7, 2 * Rn, Rn - 5):
        idx = R.mirror_map(Rn, out_len)
        g64 = gain.double().cpu().numpy()[:, None]
        ref = torch.from_numpy(g64 * r[:, idx]).to(DEV)
        bound = sum_bound(torch.from_numpy(g64 * mag[:, idx]).to(DEV), m.ntaps + 3, ref)
        got = _run(m, x, out_len=out_len, gain=gain, clamp=False, in_pad=2)
        ok, _, msg = within(got, ref, bound, f'{orig}->{new} mirror out_len={out_len}')
        assert ok, msg
        clamped = _run(m, x, out_len=out_len, gain=gain, clamp=True, in_pad=2)
        assert torch.equal(clamped, got.clamp(-1, 1)) and float(got.abs().max()) > 1.0       # the clamp is the last step, exact


@pytest.mark.parametrize('orig,new', [(44100, 16000), (48000, 16000)])
def test_int16_input_equals_fp32_input_of_x_over_32768(orig, new):
    from deepavfusion_amd.util import audio_transforms as aT
    m = _module(orig, new)
    L = aT.resample_tile(orig, new) * m.o + 1
    x = np.random.default_rng(3).integers(-32768, 32768, (3, L), dtype=np.int16)
    a = _run(m, x, in_pad=6)
    b = _run(m, x.astype(np.float32) / 32768.0, in_pad=1)
    assert torch.equal(a, b) and float(a.abs().max()) > 0.1
    assert torch.equal(m(torch.from_numpy(x).to(DEV)), a)                                    # the module takes int16 as it is


@pytest.mark.parametrize('orig,new,L,dur', [(8000, 16000, 5000, 1.0), (44100, 16000, 30000, 0.5)])
def test_prepare_waveform_equals_the_composed_modules_bit_for_bit(orig, new, L, dur):
    """PrepareWaveform == Compose([Resample, Pad, RandomVol(per_sample=True)]) under the same random.seed: R = 10000 < 16000
    samples (the mirror is used) and R = 10885 > 8000 (a plain cut); fp32 and int16 input; gain=None leaves values unclamped."""
    from deepavfusion_amd.util import audio_transforms as aT
    x = (1.2 * _waves(3, L, seed=5)).clip(-1, 1)
    xi = (x * 32767).astype(np.int16)
    fused = aT.PrepareWaveform(orig, new, dur)
    composed = aT.Compose([aT.Resample(orig, new), aT.Pad(dur, new), aT.RandomVol(per_sample=True)])
    Rn = fused.out_samples(L)
    assert (Rn < fused.samples) == (orig == 8000)
    for src in (torch.from_numpy(x).to(DEV), torch.from_numpy(xi).to(DEV)):
        random.seed(21)
        a = fused(src)
        random.seed(21)
        b = composed(src)
        assert a.shape == b.shape == (3, int(dur * new)) and a.dtype == torch.float32
        assert torch.equal(a, b)
        assert float(a.abs().max()) == 1.0                                                   # some gain of +-6 dB reached the clamp
        random.seed(22)
        assert not torch.equal(fused(src), a)                                                # another seed, other gains
    loud = torch.from_numpy(3.0 * x).to(DEV)
    plain = aT.PrepareWaveform(orig, new, dur, gain=None)
    state = random.getstate()
    y = plain(loud)
    assert random.getstate() == state                                                        # no draw without a gain
    assert torch.equal(y, aT.Pad(dur, new)(aT.Resample(orig, new)(loud))) and float(y.abs().max()) > 1.5
    assert plain(loud[:, None, :]).shape == (3, 1, int(dur * new)) and torch.equal(plain(loud[:, None, :])[:, 0], y)


def test_prepare_waveform_with_equal_rates_launches_nothing(monkeypatch):
    from deepavfusion_amd import ops
    from deepavfusion_amd.util import audio_transforms as aT

    def refuse(*a, **k):
        raise AssertionError('a resampling launch at equal rates')
    monkeypatch.setattr(ops, 'wave_resample', refuse)
    x = torch.from_numpy((1.2 * _waves(3, 3000, seed=9)).clip(-1, 1)).to(DEV)
    fused = aT.PrepareWaveform(16000, 16000, 0.5)
    assert not hasattr(fused, 'taps_kn')
    random.seed(21)                                                                          # gains -4.0, +2.3, +1.6 dB: two rows reach the clamp
    a = fused(x)
    random.seed(21)
    b = aT.Compose([aT.Pad(0.5, 16000), aT.RandomVol(per_sample=True)])(x)
    assert a.shape == (3, 8000) and torch.equal(a, b) and float(a.abs().max()) == 1.0
    assert torch.equal(aT.PrepareWaveform(16000, 16000, 0.5, gain=None)(x), aT.Pad(0.5, 16000)(x))
    xi = (x * 32767).to(torch.int16)
    assert torch.equal(aT.PrepareWaveform(16000, 16000, 0.5, gain=None)(xi), aT.Pad(0.5, 16000)(xi.float() / 32768.0))


def _write_shards(path, n, rate=8000, dur=2.0, seed=0):
    from deepavfusion_amd.util.clip_shards import ClipShardWriter
    g = np.random.default_rng(seed)
    F, hw = 4, (24, 32)
    t = np.arange(int(dur * rate)) / rate
    with ClipShardWriter(str(path), 'train', F, hw, [(k + 0.5) * dur / F for k in range(F)], rate, dur) as w:
        for k in range(n):
            audio = 0.3 * np.sin(2 * np.pi * (300 + 170 * (k % 5)) * t) + 0.1 * g.normal(size=t.size)
            w.add(g.integers(0, 256, (F, *hw, 3), dtype=np.uint8), (np.clip(audio, -1, 1) * 32767).astype(np.int16))


def _check_logmel(got, ref, eps=1e-7):
    """tests/test_audio_frontend_gpu.py::_check, restated: in mel power |got - ref| <= 5e-5 ref + 3e-6 (largest mel power of that
    waveform) + 1e-9, and <= 3e-5 in log10 units wherever a band is within 40 dB of the loudest one."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    pg, pr = 10.0 ** got - eps, 10.0 ** ref - eps
    peak = pr.amax(dim=(1, 2, 3), keepdim=True)
    assert bool(((pg - pr).abs() <= 5e-5 * pr + 3e-6 * peak + 1e-9).all()), float(((pg - pr).abs() / (5e-5 * pr + 3e-6 * peak + 1e-9)).max())
    near = pr > 1e-4 * peak
    if bool(near.any()):
        assert float((got - ref)[near].abs().max()) <= 3e-5


def test_shards_at_8_khz_to_logmel_matches_the_oracle(tmp_path):
    """ClipShards(resample=True) -> PrepareWaveform(gain=None) -> LogMelSpectrogram(16000) against oracle.audio_oracle.log_mel of
    the float64-resampled (tests/resample_ref.py, float64 table), mirror-padded window: a 1.3 s window of an 8 kHz set asked for
    1.5 s at 16 kHz, so the resampler's edges, the mirror and the log-mel all take part."""
    from deepavfusion_amd.util import audio_transforms as aT
    from deepavfusion_amd.util.clip_shards import ClipShards
    from oracle import audio_oracle as A
    _write_shards(tmp_path, 4, dur=1.3)
    ds = ClipShards(tmp_path, 'train', audio_dur=1.5, audio_rate=16000, train=False, resample=True)
    waves = torch.stack([ds[k][1] for k in range(len(ds))])
    assert waves.dtype == torch.int16 and waves.shape == (4, int(1.3 * 8000))
    front = aT.Compose([aT.PrepareWaveform(ds.stored_rate, ds.audio_rate, 1.5, gain=None), aT.LogMelSpectrogram(16000, 128).to(DEV)])
    got = front(waves.to(DEV))
    assert got.shape == (4, 1, 128, 96)
    x64 = R.pad_loop(R.resample_rates(waves.numpy().astype(np.float64) / 32768.0, 8000, 16000), 24000)
    _check_logmel(got, A.log_mel(torch.from_numpy(np.ascontiguousarray(x64)), 16000, 128))


@pytest.mark.timeout(120)
def test_train_worker_runs_on_a_set_stored_at_8_khz(tmp_path):
    """train.main_worker in this process on a 16-clip shard set stored at 8 kHz with data.audio_resample=gpu: vit_micro towers,
    64 px frames, 1 s of audio, eager steps (opt.graph=False), no probe — 3 epochs of 4 steps.  Asserts that every logged loss is
    FINITE (twelve steps on random crops and gains are too few to judge a decrease; first and last are printed) and that the
    worker built the fused front-end.  builtins.print and the RNG states the worker replaces are put back."""
    import train
    data = tmp_path / 'data'
    _write_shards(data, 16, dur=2.0)
    cfg = train.load_config('deepavfusion', [
        'model.image.backbone=vit_micro', 'model.audio.backbone=vit_micro', 'model.fusion.num_heads=2', 'data.image_size=64',
        'data.audio_dur=1.', 'opt.batch_size=4', 'opt.epochs=3', 'opt.warmup_epochs=1', 'opt.blr=0.05', 'opt.graph=False',
        'opt.resume=False', 'log.print_freq=1', f'output_dir={tmp_path}', 'job_name=t', 'env.workers=0', 'data.dataset=shards',
        f'data.data_path={data}', 'data.audio_resample=gpu', 'nn_probe.dataset=null'])
    assert cfg.data.audio_rate == 16000 and cfg.nn_probe.dataset is None
    saved = builtins.print, random.getstate(), torch.get_rng_state(), np.random.get_state()
    try:
        train.main_worker(0, cfg)
        torch.cuda.synchronize()
    finally:
        builtins.print = saved[0]
        random.setstate(saved[1]), torch.set_rng_state(saved[2]), np.random.set_state(saved[3])
    log = open(tmp_path / 't' / 'train.log').read()
    losses = [float(v) for v in re.findall(r'\[Train\]\[Ep-\d+/3\] step \d+/4  loss ([-\w.]+)', log)]
    assert len(losses) == 12 and all(np.isfinite(losses)), log[-3000:]
    print(f'worker on an 8 kHz set: loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    with pytest.raises(ValueError, match='no resampler'):                                    # the switch off: the set is refused as before
        off = train.load_config('deepavfusion', ['data.dataset=shards', f'data.data_path={data}', f'output_dir={tmp_path}', 'job_name=u',
                                                 'nn_probe.dataset=null'])
        try:
            train.main_worker(0, off)
        finally:
            builtins.print = saved[0]
            random.setstate(saved[1]), torch.set_rng_state(saved[2]), np.random.set_state(saved[3])
