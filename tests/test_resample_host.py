"""The audio resampler without a GPU: geometry and table against the float64 restatement (tests/resample_ref.py), what the
restatement itself means (tones, row sums, the mirror map), ClipShards(resample=True), the configuration keys, make_shards.py
--keep-rate and the C ABI's validation."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_ref as R  # noqa: E402

#         orig   new    o    n  width taps
PAIRS = [(44100, 16000, 441, 160, 17, 475),
         (48000, 16000, 3, 1, 19, 41),
         (22050, 16000, 441, 320, 9, 459),
         (11025, 16000, 441, 640, 7, 455),
         (8000, 16000, 1, 2, 7, 15),
         (16000, 8000, 2, 1, 13, 28)]


@pytest.mark.parametrize('orig,new,o,n,width,taps', PAIRS)
def test_geometry_and_table_equal_the_float64_restatement(orig, new, o, n, width, taps):
    """The reduced geometry of the six pairs, and the module's fp32 table == the restatement's float64 table cast to fp32, bit
    for bit; the kernel's k-major copy is its transpose."""
    from deepavfusion_amd.util import audio_transforms as aT
    assert aT.resample_geometry(orig, new) == (o, n, width, taps) == R.geometry(orig, new)
    m = aT.Resample(orig, new)
    assert (m.o, m.n, m.width, m.ntaps) == (o, n, width, taps)
    ref = R.taps64(orig, new).astype(np.float32)
    assert m.taps.dtype == torch.float32 and tuple(m.taps.shape) == (n, taps)
    assert np.array_equal(m.taps.numpy().view(np.uint32), ref.view(np.uint32))
    assert m.taps_kn.is_contiguous() and torch.equal(m.taps_kn, m.taps.t())
    assert 'taps' not in m.state_dict() and 'taps_kn' not in m.state_dict()          # non-persistent, like the mel tables
    assert m.out_samples(1000) == -(-n * 1000 // o)


def test_resample_module_surface():
    from deepavfusion_amd.util import audio_transforms as aT
    x = torch.zeros(2, 100)
    assert aT.Resample(16000, 16000)(x) is x and aT.Resample()(x) is x              # equal rates: the input object, on any device
    with pytest.raises(NotImplementedError):
        aT.Resample(44100, 16000, resampling_method='sinc_interp_kaiser')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aT.Resample(8000, 16000)(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aT.PrepareWaveform(8000, 16000, 1.0)(x)
    with pytest.raises(ValueError, match='ratios up to 1024'):
        aT.Resample(16000, 16001)
    p = aT.PrepareWaveform(8000, 16000, 1.5, gain=None)
    assert p.samples == 24000 and (p.o, p.n) == (1, 2)


@pytest.mark.parametrize('freq,orig,new', [(1000.0, 44100, 16000), (3000.0, 48000, 16000), (1000.0, 8000, 16000)])
def test_restatement_resamples_a_tone_to_the_analytic_tone(freq, orig, new):
    """A 0.5-amplitude tone of 0.5 s, resampled by the float64 restatement, is the analytic tone at the new rate within 1e-3 away
    from 200 samples at each end (measured: 2.0e-4, 2.6e-4, 8.5e-5; the filter's ripple and its 0.99 rolloff)."""
    L = orig // 2
    x = 0.5 * np.sin(2 * np.pi * freq * np.arange(L) / orig)
    y = R.resample_rates(x, orig, new)
    assert y.shape == (-(-new * L // orig),)
    want = 0.5 * np.sin(2 * np.pi * freq * np.arange(y.size) / new)
    err = np.abs(y - want)[200:-200].max()
    print(f'tone {freq:g} Hz {orig} -> {new}: interior max error {err:.3g}')
    assert err <= 1e-3


@pytest.mark.parametrize('orig,new', [p[:2] for p in PAIRS])
def test_every_phase_sums_to_one(orig, new):
    """Unit gain at DC: every phase's taps sum to 1.0000 .. 1.0010 (measured 1.00004 .. 1.00088)."""
    s = R.taps64(orig, new).sum(1)
    assert s.min() >= 1.0 and s.max() <= 1.0010, (s.min(), s.max())


def test_mirror_map_is_pads_loop():
    """m(j) = j' < R ? j' : 2 R - 1 - j', j' = j mod 2 R, is what 'append the flipped signal until long enough, then cut' gives:
    R = 5, out_len = 23 (two doublings and a cut), and the package's Pad on the same signal."""
    from deepavfusion_amd.util import audio_transforms as aT
    r = np.arange(5) + 10.0
    assert np.array_equal(R.pad_loop(r, 23), r[R.mirror_map(5, 23)])
    assert np.array_equal(aT.Pad(23, 1)(torch.from_numpy(r)).numpy(), r[R.mirror_map(5, 23)])
    assert np.array_equal(R.pad_loop(r, 3), r[R.mirror_map(5, 3)]) and R.mirror_map(5, 3).tolist() == [0, 1, 2]
    assert R.mirror_map(5, 12).tolist() == [0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 0, 1]


def _write_set(path, n=6, rate=8000, dur=3.0, seed=0):
    from deepavfusion_amd.util.clip_shards import ClipShardWriter
    g = np.random.default_rng(seed)
    F, hw = 6, (24, 32)
    audio = g.integers(-32768, 32768, (n, int(round(dur * rate))), dtype=np.int16)
    with ClipShardWriter(str(path), 'train', F, hw, [(k + 0.5) * dur / F for k in range(F)], rate, dur) as w:
        for k in range(n):
            w.add(g.integers(0, 256, (F, *hw, 3), dtype=np.uint8), audio[k])
    return audio


def test_clip_shards_cut_at_the_stored_rate_and_yield_int16(tmp_path):
    """Stored at 8000 Hz, asked for 16000: resample=True yields the int16 window of int(audio_dur * 8000) samples from
    round(start * 8000), with the (start, frame) draws of a reader at the stored rate; the default still refuses."""
    from deepavfusion_amd.util.clip_shards import ClipShards
    audio = _write_set(tmp_path)
    with pytest.raises(ValueError, match='no resampler'):
        ClipShards(tmp_path, 'train', audio_dur=1.3, audio_rate=16000)
    with pytest.raises(ValueError, match='no resampler'):
        ClipShards(tmp_path, 'train', audio_dur=1.3, audio_rate=16000, resample=False)
    for train in (True, False):
        ds = ClipShards(tmp_path, 'train', audio_dur=1.3, audio_rate=16000, train=train, seed=3, resample=True)
        plain = ClipShards(tmp_path, 'train', audio_dur=1.3, audio_rate=8000, train=train, seed=3)
        assert (ds.audio_rate, ds.stored_rate, plain.audio_rate, plain.stored_rate) == (16000, 8000, 8000, 8000)
        for epoch in (0, 2):
            ds.set_epoch(epoch), plain.set_epoch(epoch)
            for k in range(len(ds)):
                assert ds.sample(k) == plain.sample(k)
                start, f = ds.sample(k)
                fr, wv, idx = ds[k]
                fr0, wv0, _ = plain[k]
                s0 = int(round(start * 8000))
                assert wv.dtype == torch.int16 and wv.shape == (int(1.3 * 8000),) and idx == k
                assert np.array_equal(wv.numpy(), audio[k, s0:s0 + int(1.3 * 8000)])
                assert torch.equal(fr, fr0) and torch.equal(wv.float() / 32768.0, wv0) and wv0.dtype == torch.float32


def test_config_has_the_switch_off_and_the_probe_follows_it():
    import train
    cfg = train.load_config('deepavfusion')
    assert cfg.data.audio_resample == 'off' and cfg.nn_probe.audio_resample == 'off'
    cfg = train.load_config('deepavfusion', ['data.audio_resample=gpu'])
    assert cfg.data.audio_resample == 'gpu' and cfg.nn_probe.audio_resample == 'gpu'
    assert train.audio_resample_mode(train.load_config('deepavfusion', ['data.audio_resample=off']).data.audio_resample) == 'off'
    with pytest.raises(ValueError):
        train.audio_resample_mode('cpu')


def test_make_shards_keep_rate_records_the_tracks_own_rate(tmp_path):
    """--keep-rate: two 22050 Hz tracks -> meta.json says 22050 and the samples are the tracks'; a third at 16000 Hz is refused by
    name; without the flag a 22050 Hz track is refused as before."""
    Image = pytest.importorskip('PIL.Image')
    import wave
    from deepavfusion_amd.util.clip_shards import ClipShards
    src = tmp_path / 'src'
    g = np.random.default_rng(0)
    pcm = {}

    def clip(c, rate):
        os.makedirs(src / c / 'frames')
        for k in range(4):
            Image.fromarray(g.integers(0, 256, (20, 30, 3), dtype=np.uint8)).save(src / c / 'frames' / f'{k:03d}.png')
        pcm[c] = g.integers(-3000, 3000, (rate, 1), dtype=np.int16)                       # 1 s mono
        with wave.open(str(src / c / 'audio.wav'), 'wb') as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(rate)
            f.writeframes(pcm[c].tobytes())

    def tool(out, *extra):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_shards.py'), str(src), str(tmp_path / out), '--hw', '16', '24',
                               '--frames', '2', '--clip-dur', '1', *extra], capture_output=True, text=True)
    clip('a', 22050), clip('b', 22050)
    r = tool('kept', '--keep-rate')
    assert r.returncode == 0, r.stdout + r.stderr
    meta = json.load(open(tmp_path / 'kept' / 'train' / 'meta.json'))
    assert meta['audio_rate'] == 22050 and meta['num_clips'] == 2
    ds = ClipShards(tmp_path / 'kept', 'train', audio_dur=1.0, audio_rate=16000, train=False, resample=True)
    assert ds.stored_rate == 22050 and np.array_equal(ds[1][1].numpy(), pcm['b'][:, 0])
    r = tool('plain')
    assert r.returncode != 0 and 'a/audio.wav' in r.stdout + r.stderr and '22050 Hz' in r.stdout + r.stderr
    clip('c', 16000)
    r = tool('mixed', '--keep-rate')
    assert r.returncode != 0 and 'c/audio.wav' in r.stdout + r.stderr and '16000 Hz' in r.stdout + r.stderr


def test_entry_points_are_declared_exported_and_validate_without_a_gpu():
    """dav_wave_resample: sizes are judged first (-1: empty, a ratio above dav_resample_max_ratio, strides shorter than the rows),
    then alignment (-5); pointers are never dereferenced.  Pattern of test_error_codes_for_dtype_alignment_and_workspace."""
    from deepavfusion_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'dav_kernels.h')).read()
    for name in ('dav_wave_resample', 'dav_wave_resample_tile'):
        assert name in _lib.SIGNATURES and f'int {name}(' in header
    assert f'enum {{ dav_resample_max_ratio = {ops.RESAMPLE_MAX_RATIO} }};' in header and '#define DAV_ABI_VERSION 9 ' in header
    assert 'data/resample.hip' in open(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', 'Makefile')).read()
    lib = _lib.load()
    p, i, l = C.c_void_p, C.c_int, C.c_long

    def call(wave=4096, i16=0, B=2, L=1000, in_rs=1000, taps=8192, o=441, n=160, width=17, gain=None, clamp=0, out=1 << 20, out_len=400,
             out_rs=400):
        return lib.dav_wave_resample(p(wave), i(i16), i(B), i(L), l(in_rs), p(taps), i(o), i(n), i(width), p(gain), i(clamp), p(out),
                                     i(out_len), l(out_rs), p(None))
    assert call(o=1025) == -1 and call(n=1025) == -1 and call(o=1025, out=(1 << 20) + 2) == -1     # valid sizes, ratio above the cap
    assert call(B=0) == -1 and call(L=0) == -1 and call(out_len=0) == -1 and call(o=0) == -1 and call(n=0) == -1 and call(width=0) == -1
    assert call(in_rs=999) == -1 and call(out_rs=399) == -1 and call(wave=None) == -1 and call(taps=None) == -1 and call(out=None) == -1
    assert call(width=7000) == -1                                                                   # 2 width + o samples do not fit the LDS
    assert call(out=(1 << 20) + 2) == -5 and call(taps=8192 + 2) == -5 and call(wave=4096 + 2) == -5 and call(gain=12288 + 1) == -5
    assert call(wave=4096 + 1, i16=1) == -5                                                         # int16 rows: 2-byte alignment
    assert lib.dav_wave_resample_tile(0, 0, 0) == -1 and lib.dav_wave_resample_tile(1025, 1, 7) == -1
    assert ops.wave_resample_tile(441, 160, 17) >= 1 and ops.wave_resample_tile(3, 1, 19) >= 1


def test_kernel_source_hash_leaves_the_resampler_out():
    """csrc/data/ sits outside the hash the PMC records under profiles/ carry."""
    import glob
    from deepavfusion_amd import _lib
    assert os.path.isfile(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', 'data', 'resample.hip'))
    hashed = glob.glob(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', '*.hip')) + glob.glob(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', '*.h'))
    assert not any('resample' in os.path.basename(f) for f in hashed) and len(_lib.kernel_source_hash()) == 16
