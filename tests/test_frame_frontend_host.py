"""The image half of the input stage, device-free: the float64 restatement of the frame transform (tests/frame_ref.py) held to
torch's antialiased interpolate and to PIL's recorded results, the parameter samplers, the clip-shard writer / reader, the C ABI
of dav_frame_transform_u8 and the configuration keys."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_ref as R  # noqa: E402

PIL_BOUND = 1.0 + 5e-3      # grey levels: two roundings to uint8 of <= 0.5 each (the vertical weights sum to 1) + 22-bit coefficients


def test_restatement_equals_torch_antialiased_interpolate_in_float64():
    """The tap rule of tests/frame_ref.py against F.interpolate(mode='bilinear', antialias=True, align_corners=False) in float64
    on random frames, boxes and sizes, up- and down-scaling: <= 1e-9 grey levels."""
    g = np.random.default_rng(0)
    worst = 0.0
    for t in range(40):
        H, W = int(g.integers(8, 120)), int(g.integers(8, 140))
        frame = R.noise_frame(H, W, 100 + t) if t % 2 else R.smooth_frame(H, W, 100 + t)
        h, w = int(g.integers(1, H + 1)), int(g.integers(1, W + 1))
        i, j = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
        oh, ow = int(g.integers(2, 160)), int(g.integers(2, 160))            # larger and smaller than the box (torch special-cases 1)
        got = R.resample(frame, (i, j, h, w), (oh, ow))
        x = torch.from_numpy(frame[i:i + h, j:j + w].astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.nn.functional.interpolate(x, size=(oh, ow), mode='bilinear', antialias=True, align_corners=False)
        worst = max(worst, float(np.abs(got - ref[0].permute(1, 2, 0).numpy()).max()))
    print(f'restatement vs torch float64: worst {worst:.3g} grey levels')
    assert worst <= 1e-9


def test_restatement_agrees_with_pil_fixture(golden):
    """tests/golden/frame_transform.npz (written by tests/golden/gen_frame_golden.py with PIL): every element of PIL's uint8 result
    within 1 + 5e-3 grey levels of the restatement — PIL rounds to uint8 after each pass, the rule does not."""
    z = golden('frame_transform')
    rows, src_of, size = z['rows'], z['src_of'], z['size']
    assert len(rows) >= 8 and rows.shape[1] == 9
    nbytes = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'frame_transform.npz'))
    assert nbytes < 300 * 1024
    kinds = set()
    for n, (row, k, S) in enumerate(zip(rows, src_of, size)):
        src, pil = z[f'src{k}'], z[f'pil{n}']
        assert src.dtype == np.uint8 and src.shape[0] <= 96 and src.shape[1] <= 128 and pil.shape == (S, S, 3)
        i, j, h, w, RH, RW, top, left, flip = (int(v) for v in row)
        ref = R.resample(src, (i, j, h, w), (RH, RW))[top:top + S, left:left + S]
        ref = ref[:, ::-1] if flip else ref
        worst = float(np.abs(ref - pil).max())
        assert worst <= PIL_BOUND, (n, worst)
        kinds.add('eval' if (RH, RW) != (S, S) else 'train')
        # the normalised form the kernel is compared with is the same numbers, rescaled
        t = R.transform(src, row, int(S))
        back = (t * np.asarray(R.STD)[:, None, None] + np.asarray(R.MEAN)[:, None, None]) * 255.0
        assert np.abs(back.transpose(1, 2, 0) - ref).max() <= 1e-9
    assert kinds == {'eval', 'train'}


def test_random_resized_crop_params_follow_the_published_sampler():
    from deepavfusion_amd.util.frame_transforms import random_resized_crop_params
    ratio = (3. / 4., 4. / 3.)
    for scale in ((0.08, 1.0), (0.5, 1.0)):
        for (H, W) in ((256, 340), (360, 480), (96, 128)):
            g = torch.Generator().manual_seed(5)
            boxes = [random_resized_crop_params(H, W, scale, ratio, g) for _ in range(300)]
            g2 = torch.Generator().manual_seed(5)
            assert boxes == [random_resized_crop_params(H, W, scale, ratio, g2) for _ in range(300)]      # same state, same boxes
            assert len(set(boxes)) > 100
            for (i, j, h, w) in boxes:
                assert h >= 1 and w >= 1 and 0 <= i and 0 <= j and i + h <= H and j + w <= W
                if (h, w) == (H, W) and (i, j) == (0, 0):
                    continue                                     # may be the fallback: whole frame, ratio already inside
                # area and ratio up to the int(round()) of the two sides: each side is off by <= 0.5
                lo_a, hi_a = (h - 0.5) * (w - 0.5), (h + 0.5) * (w + 0.5)
                assert hi_a >= scale[0] * H * W and lo_a <= scale[1] * H * W, (h, w)
                assert (w + 0.5) / (h - 0.5) >= ratio[0] and (w - 0.5) / (h + 0.5) <= ratio[1], (h, w)
    # no box of the asked-for area fits a 1000 x 10 frame: the central crop, ratio clamped into [3/4, 4/3]
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        assert random_resized_crop_params(1000, 10, (0.08, 1.0), ratio, g) == ((1000 - 13) // 2, 0, int(round(10 / 0.75)), 10)
    assert random_resized_crop_params(10, 1000, (0.08, 1.0), ratio, g) == (0, (1000 - 13) // 2, 10, int(round(10 * 4. / 3.)))


def test_resize_center_crop_params_are_torchvisions():
    from deepavfusion_amd.util.frame_transforms import resize_center_crop_params
    assert resize_center_crop_params(256, 340, 224) == ((256, 340), (16, 58))
    assert resize_center_crop_params(480, 360, 224) == ((341, 256), (58, 16))        # int(round(58.5)) = 58: half to even
    assert resize_center_crop_params(96, 128, 64) == ((73, 97), (4, 16))             # int(round(4.5)) = 4
    with pytest.raises(ValueError):
        resize_center_crop_params(64, 64, 64, crop_pct=1.5)


def test_transform_modules_validate_on_the_host_and_have_no_cpu_fallback():
    from deepavfusion_amd.util import frame_transforms as FT
    tf = FT.TrainFrameTransform(64, scale=(0.5, 1.0), seed=3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tf(torch.zeros(2, 96, 128, 3, dtype=torch.uint8))
    a = tf.draw(16, 96, 128)
    assert a != tf.draw(16, 96, 128)                                  # a second call draws other boxes
    assert tf.seed(3).draw(16, 96, 128) == a                          # re-seeding repeats them
    assert {r[8] for r in a} == {0, 1} and all(r[4:8] == [64, 64, 0, 0] for r in a)
    FT.check_rows(a, 96, 128, 64)
    ev = FT.EvalFrameTransform(64).draw(2, 96, 128)
    assert ev == [[0, 0, 96, 128, 73, 97, 4, 16, 0]] * 2
    FT.check_rows(ev, 96, 128, 64)
    for bad in ([0, 0, 97, 128, 64, 64, 0, 0, 0], [-1, 0, 9, 9, 64, 64, 0, 0, 0], [0, 0, 9, 0, 64, 64, 0, 0, 0],
                [0, 0, 96, 128, 73, 97, 10, 16, 0], [0, 0, 96, 128, 64, 64, 0, 0, 2]):
        with pytest.raises(ValueError):
            FT.check_rows([bad], 96, 128, 64)
    with pytest.raises(ValueError):
        FT.TrainFrameTransform(24)


# ---- clip shards ----------------------------------------------------------------------------------------------------------

def _write_set(path, partition, n, F=6, hw=(24, 32), rate=8000, dur=3.0, labels='single', seed=0):
    from deepavfusion_amd.util.clip_shards import ClipShardWriter
    g = np.random.default_rng(seed)
    times = [(k + 0.5) * dur / F for k in range(F)]
    frames = g.integers(0, 256, (n, F, *hw, 3), dtype=np.uint8)
    audio = g.integers(-32768, 32768, (n, int(round(dur * rate))), dtype=np.int16)
    names = [f'c{k}' for k in range(5)] if labels else None
    if labels == 'multi':
        lab = g.integers(0, 2, (n, 5)).astype(np.uint8)
    elif labels:
        lab = g.integers(0, 5, n).astype(np.int64)
    else:
        lab = [None] * n
    with ClipShardWriter(str(path), partition, F, hw, times, rate, dur, names, labels == 'multi') as w:
        for k in range(n):
            w.add(frames[k], audio[k], lab[k])
    return frames, audio, (np.asarray(lab) if labels else None), times


def test_shards_round_trip_is_bit_exact_and_mismatches_are_refused(tmp_path):
    from deepavfusion_amd.util.clip_shards import ClipShards, ClipShardWriter
    for labels in ('single', 'multi', None):
        frames, audio, lab, times = _write_set(tmp_path / str(labels), 'train', 7, labels=labels)
        ds = ClipShards(tmp_path / str(labels), 'train', audio_dur=3.0, audio_rate=8000, train=False)
        assert len(ds) == 7
        ds._open()
        assert np.array_equal(np.asarray(ds._frames), frames) and np.array_equal(np.asarray(ds._audio), audio)
        assert ds.has_labels == (labels is not None)
        if labels:
            assert np.array_equal(ds.labels, lab) and ds.labels.dtype == (np.uint8 if labels == 'multi' else np.int64)
        for k in range(7):
            fr, wave, anno = ds[k]
            start, f = ds.sample(k)
            assert fr.dtype == torch.uint8 and torch.equal(fr, torch.from_numpy(frames[k, f]))
            assert wave.dtype == torch.float32 and np.array_equal(wave.numpy(), audio[k].astype(np.float32) / 32768.0)   # whole clip
            assert float(wave.abs().max()) <= 1.0
            if labels == 'multi':
                assert np.array_equal(anno['class'].numpy(), lab[k])
            elif labels:
                assert anno == {'class': int(lab[k])}
            else:
                assert anno == k
    with pytest.raises(ValueError, match='no resampler'):
        ClipShards(tmp_path / 'single', 'train', audio_dur=3.0, audio_rate=16000)
    with pytest.raises(FileNotFoundError):
        ClipShards(tmp_path / 'single', 'val', audio_dur=3.0, audio_rate=8000)
    w = ClipShardWriter(str(tmp_path / 'bad'), 'train', 2, (8, 8), [0.5, 1.5], 8000, 2.0)
    ok_f, ok_a = np.zeros((2, 8, 8, 3), np.uint8), np.zeros(16000, np.int16)
    w.add(ok_f, ok_a)
    for f, a, lab in ((np.zeros((2, 8, 9, 3), np.uint8), ok_a, None), (np.zeros((3, 8, 8, 3), np.uint8), ok_a, None),
                      (ok_f.astype(np.float32), ok_a, None), (ok_f, np.zeros(16001, np.int16), None),
                      (ok_f, ok_a.astype(np.float32), None), (ok_f, ok_a, 1)):
        with pytest.raises(ValueError):
            w.add(f, a, lab)
    w.close()
    assert len(ClipShards(tmp_path / 'bad', 'train', audio_dur=1.0, audio_rate=8000)) == 1
    with pytest.raises(ValueError):
        ClipShardWriter(str(tmp_path / 'bad2'), 'train', 2, (8, 8), [0.5], 8000, 2.0)


def test_shards_windows_frames_and_short_clips(tmp_path):
    from deepavfusion_amd.util.clip_shards import ClipShards
    frames, audio, lab, times = _write_set(tmp_path, 'train', 5, F=6, rate=8000, dur=3.0)
    times = np.asarray(times)
    ds = ClipShards(tmp_path, 'train', audio_dur=1.0, audio_rate=8000, train=True, seed=4)
    starts = []
    for d in range(200):
        ds.set_epoch(d)
        k = d % 5
        start, f = ds.sample(k)
        starts.append(start)
        assert 0.0 <= start and start + 1.0 <= 3.0 + 1e-12                        # the window lies inside the clip
        inside = (times >= start) & (times <= start + 1.0)
        assert inside.any() and inside[f]                                         # 0.5 s spacing: a stored frame is always inside
        fr, wave, anno = ds[k]
        s0 = int(round(start * 8000))
        assert wave.shape == (8000,) and np.array_equal(wave.numpy(), audio[k, s0:s0 + 8000].astype(np.float32) / 32768.0)
        assert torch.equal(fr, torch.from_numpy(frames[k, f]))
    assert max(starts) - min(starts) > 1.5 and len({round(s, 6) for s in starts}) > 150
    # a window too narrow to hold a stored frame takes the nearest one
    nar = ClipShards(tmp_path, 'train', audio_dur=0.1, audio_rate=8000, train=True, seed=1)
    for d in range(50):
        nar.set_epoch(d)
        start, f = nar.sample(0)
        dist = np.abs(times - np.clip(times, start, start + 0.1))
        assert dist[f] == dist.min()
    # eval: centred, the same at every epoch
    ev = ClipShards(tmp_path, 'train', audio_dur=1.0, audio_rate=8000, train=False, seed=4)
    first = [ev.sample(k) for k in range(5)]
    ev.set_epoch(9)
    assert [ev.sample(k) for k in range(5)] == first and all(s == 1.0 for s, _ in first)
    assert all(1.0 <= times[f] <= 2.0 for _, f in first)
    assert np.array_equal(ev[2][1].numpy(), audio[2, 8000:16000].astype(np.float32) / 32768.0)
    # a clip shorter than audio_dur comes back whole, from start 0, train or not
    for train in (True, False):
        sh = ClipShards(tmp_path, 'train', audio_dur=10.0, audio_rate=8000, train=train, seed=0)
        assert sh.sample(3)[0] == 0.0
        assert np.array_equal(sh[3][1].numpy(), audio[3].astype(np.float32) / 32768.0)


def test_shards_draws_depend_on_seed_epoch_index_not_on_workers(tmp_path):
    from deepavfusion_amd.util.clip_shards import ClipShards
    _write_set(tmp_path, 'train', 12, labels=None)

    def epoch(workers, seed, ep):
        ds = ClipShards(tmp_path, 'train', audio_dur=1.0, audio_rate=8000, train=True, seed=seed)
        ds.set_epoch(ep)
        dl = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=workers)
        out = [(f.clone(), w.clone(), i.clone()) for f, w, i in dl]
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out]), torch.cat([o[2] for o in out])
    a, b = epoch(0, 3, 1), epoch(2, 3, 1)
    assert a[0].shape == (12, 24, 32, 3) and a[0].dtype == torch.uint8 and a[1].shape == (12, 8000)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                 # 0 and 2 workers: the same bytes
    assert all(torch.equal(x, y) for x, y in zip(a, epoch(0, 3, 1)))
    assert not torch.equal(a[1], epoch(0, 3, 2)[1])                     # another epoch, other windows
    assert not torch.equal(a[1], epoch(0, 4, 1)[1])                     # another seed


def test_make_shards_tool_from_a_folder_of_decoded_clips(tmp_path):
    """tools/make_shards.py: frames/*.png + audio.wav per clip (+ labels.csv) -> a partition ClipShards reads."""
    Image = pytest.importorskip('PIL.Image')
    import wave
    from deepavfusion_amd.util.clip_shards import ClipShards
    src = tmp_path / 'src'
    g = np.random.default_rng(0)
    pcm = {}
    for c, (h, w) in (('a', (40, 60)), ('b', (50, 50))):
        os.makedirs(src / c / 'frames')
        for k in range(5):
            Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / c / 'frames' / f'{k:03d}.png')
        pcm[c] = g.integers(-3000, 3000, (8000, 2), dtype=np.int16)
        with wave.open(str(src / c / 'audio.wav'), 'wb') as f:
            f.setnchannels(2), f.setsampwidth(2), f.setframerate(4000)
            f.writeframes(pcm[c].tobytes())
    (src / 'labels.csv').write_text('a,dog\nb,cat\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_shards.py'), str(src), str(tmp_path / 'out'), '--partition', 'test',
                        '--hw', '32', '48', '--frames', '4', '--clip-dur', '2', '--audio-rate', '4000'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ds = ClipShards(tmp_path / 'out', 'test', audio_dur=2.0, audio_rate=4000, train=False)
    assert len(ds) == 2 and ds.hw == (32, 48) and ds.class_names == ['cat', 'dog'] and not ds.multi_label
    assert ds.labels.tolist() == [1, 0]
    fr, wv, anno = ds[0]
    assert fr.shape == (32, 48, 3) and anno == {'class': 1}
    mono = (pcm['a'].astype(np.int32).sum(1) // 2).astype(np.int16)
    assert np.array_equal(wv.numpy(), mono.astype(np.float32) / 32768.0)


# ---- C ABI and configuration ---------------------------------------------------------------------------------------------

def test_frame_transform_entry_point_is_declared_exported_and_validates_without_a_gpu():
    from deepavfusion_amd import _lib
    name = 'dav_frame_transform_u8'
    assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, 'include', 'dav_kernels.h')).read()
    assert f'int {name}(' in header and '#define DAV_ABI_VERSION 9 ' in header
    assert 'data/frames.hip' in open(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', 'Makefile')).read()
    lib = _lib.load()
    assert lib.dav_abi_version() == 9 == _lib.ABI_VERSION
    fn = getattr(lib, name)
    p, i, f = C.c_void_p, C.c_int, C.c_float
    norm = [f(0.485), f(0.456), f(0.406), f(0.229), f(0.224), f(0.225)]

    def call(frames=4096, B=2, H=96, W=128, params=8192, S=64, out=1 << 20, norm=norm):
        return fn(p(frames), i(B), i(H), i(W), p(params), i(S), *norm, p(out), p(None))
    assert call(S=24) == -1                                  # not a multiple of 16
    assert call(B=0) == -1 and call(H=0) == -1 and call(W=-3) == -1 and call(S=0) == -1
    assert call(out=(1 << 20) + 4) == -5                     # valid sizes, out only 4-byte aligned
    assert call(params=8192 + 2) == -5
    assert call(S=24, out=(1 << 20) + 4) == -1               # sizes are judged before alignment
    assert call(frames=None) == -1 and call(norm=norm[:3] + [f(0.0)] * 3) == -1
    assert call(H=1 << 15) == -1


def test_kernel_source_hash_leaves_the_frame_kernel_out():
    """csrc/data/ sits outside the hash the PMC records under profiles/ carry (csrc/*.hip, csrc/*.h + the tuned table)."""
    from deepavfusion_amd import _lib
    assert os.path.isfile(os.path.join(ROOT, 'deepavfusion_amd', 'csrc', 'data', 'frames.hip'))
    assert _lib.kernel_source_hash() == '9f46aa1bbd8d19b7'


def test_config_resolves_shards_and_defaults_stay_synthetic():
    import train
    cfg = train.load_config('deepavfusion')
    assert cfg.data.dataset == 'synthetic' and cfg.nn_probe.dataset is None and cfg.data.data_path is None
    assert cfg.data.crop_min == 0.5 and cfg.data.partition == 'train' and cfg.nn_probe.partition == 'test'
    cfg = train.load_config('deepavfusion', ['data.dataset=shards', 'data.data_path=/x', 'nn_probe.dataset=shards'])
    assert cfg.data.dataset == 'shards' and cfg.data.data_path == '/x' and cfg.nn_probe.data_path == '/x'
    assert cfg.nn_probe.dataset == 'shards' and 'shards' in cfg.job_name
    assert math.isclose(cfg.nn_probe.crop_min, 0.5)
