"""The frame transform on the device: dav_frame_transform_u8 elementwise against the float64 restatement (tests/frame_ref.py) and
against PIL's recorded results, the transform modules, and train.py on a clip-shard set end to end."""
import ast
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_ref as R  # noqa: E402
from kcheck import Guarded, within  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# Per element, in normalised units.  The widest case (360 x 480 -> 64, scale 7.5) sums <= 17 non-negative terms <= 255 per axis
# with weights summing to 1; two such fp32 passes err by about 5e-4 grey levels = 1e-5 after / (255 * 0.224).  1e-4 is ten times
# that and 175 x below one grey level (1.75e-2): a wrong tap, an un-normalised edge weight or a half-pixel shift (tens of levels
# on noise) cannot hide.
BOUND = 1e-4
PIL_LEVELS = 1.0 + 5e-3       # PIL rounds to uint8 after each pass (<= 0.5 each) and keeps 22-bit fixed-point coefficients


def _run(frames, rows, S):
    """frames uint8 [B, H, W, 3] (numpy), rows [B, 9] -> the kernel's output [B, 3, S, S], written into a poisoned, guard-banded
    buffer whose bands are checked."""
    from deepavfusion_amd import ops
    B = frames.shape[0]
    out = Guarded(B * 3 * S, S, torch.float32, device=DEV, fill='poison')
    ops.frame_transform(torch.from_numpy(frames).to(DEV), torch.tensor(np.asarray(rows), dtype=torch.int32, device=DEV), S,
                        R.MEAN, R.STD, out=out.t.view(B, 3, S, S))
    torch.cuda.synchronize()
    n_stray, where = out.stray()
    assert n_stray == 0, where
    return out.t.view(B, 3, S, S)


def _check(frames, rows, S, tag):
    got = _run(frames, rows, S)
    ref = torch.from_numpy(R.transform_batch(frames, rows, S)).to(DEV)
    ok, worst, msg = within(got, ref, BOUND, tag)
    assert ok, msg
    return worst * BOUND


def _frames(B, H, W, seed):
    return np.stack([R.noise_frame(H, W, seed + b) if b % 2 == 0 else R.smooth_frame(H, W, seed + b) for b in range(B)])


def _mixed_rows(B, H, W, S, seed):
    """Boxes of every kind in one batch: the sampler at scale (0.08, 1) and (0.5, 1), upscaling boxes (h, w < S), the whole frame,
    one-pixel-wide and one-pixel-high boxes; flips on and off."""
    from deepavfusion_amd.util.frame_transforms import random_resized_crop_params
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    boxes = []
    while len(boxes) < B:
        k = len(boxes) % 16
        if k < 6:
            boxes.append(random_resized_crop_params(H, W, (0.08, 1.0), generator=g))
        elif k < 12:
            boxes.append(random_resized_crop_params(H, W, (0.5, 1.0), generator=g))
        elif k == 12:
            boxes.append((0, 0, H, W))
        elif k == 13:
            h, w = int(rng.integers(2, S)), int(rng.integers(2, S))
            boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
        elif k == 14:
            h = int(rng.integers(S, H + 1))
            boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W)), h, 1))
        else:
            w = int(rng.integers(2, W + 1))
            boxes.append((int(rng.integers(0, H)), int(rng.integers(0, W - w + 1)), 1, w))
    return [[i, j, h, w, S, S, 0, 0, (n // 2 + n // 7) % 2] for n, (i, j, h, w) in enumerate(boxes)]


def test_kernel_matches_the_float64_restatement_elementwise(golden):
    """Every element within 1e-4 (normalised units) of tests/frame_ref.py, outputs poisoned and guard-banded: the fixture's cases;
    noise and smooth frames at 256 x 340 and 360 x 480 -> 224 and -> 64 with sampler boxes at scale (0.08, 1) and (0.5, 1),
    upscaling boxes, the whole frame, 1-pixel boxes, flips mixed in one batch; B = 1 and B = 64; the eval form.
    Measured on an MI355X: worst |kernel - float64| 1.17e-6 over all of these (360 x 480 -> 64; 9.4e-7 at 256 x 340 -> 224) — the
    weights are exact integers over a common denominator, so only the fp32 sums and the two divisions round."""
    from deepavfusion_amd.util.frame_transforms import resize_center_crop_params
    worst = {}
    z = golden('frame_transform')
    for n, (row, k, S) in enumerate(zip(z['rows'], z['src_of'], z['size'])):
        worst['fixture'] = max(worst.get('fixture', 0.0), _check(z[f'src{k}'][None], row[None], int(S), f'fixture case {n}'))
    for (H, W) in ((256, 340), (360, 480)):
        frames = _frames(64, H, W, 1000 + H)
        for S in (224, 64):
            rows = _mixed_rows(64, H, W, S, seed=S + H)
            assert {r[8] for r in rows} == {0, 1}
            worst[f'{H}x{W}->{S} B=64'] = _check(frames, rows, S, f'{H}x{W}->{S} B=64')
            for b in (0, 13, 14, 15):                           # B = 1: sampler box, upscaling, 1-pixel-wide, 1-pixel-high
                worst[f'{H}x{W}->{S} B=1'] = max(worst.get(f'{H}x{W}->{S} B=1', 0.0),
                                                 _check(frames[b:b + 1], rows[b:b + 1], S, f'{H}x{W}->{S} B=1 sample {b}'))
            (RH, RW), (top, left) = resize_center_crop_params(H, W, S)
            ev = [[0, 0, H, W, RH, RW, top, left, 0]] * 4
            worst[f'{H}x{W}->{S} eval'] = _check(frames[:4], ev, S, f'{H}x{W}->{S} eval')
    # portrait frames through the eval form: (480, 360) -> resized (341, 256), window at (58, 16)
    fr = _frames(2, 480, 360, 77)
    (RH, RW), (top, left) = resize_center_crop_params(480, 360, 224)
    worst['480x360->224 eval'] = _check(fr, [[0, 0, 480, 360, RH, RW, top, left, 0], [0, 0, 480, 360, RH, RW, top, left, 1]], 224, 'portrait eval')
    for k, v in worst.items():
        print(f'frame_transform {k}: worst |kernel - float64| = {v:.3g}')
    print(f'frame_transform overall worst {max(worst.values()):.3g} (bound {BOUND:g})')


def test_kernel_against_pil_fixture(golden):
    """Directly against PIL's recorded uint8 results: within (1 + 5e-3) / (255 std_c) per channel of PIL's normalised result."""
    z = golden('frame_transform')
    mean, std = np.asarray(R.MEAN)[:, None, None], np.asarray(R.STD)[:, None, None]
    worst = 0.0
    for n, (row, k, S) in enumerate(zip(z['rows'], z['src_of'], z['size'])):
        got = _run(z[f'src{k}'][None], row[None], int(S))[0]
        pil = (z[f'pil{n}'].astype(np.float64).transpose(2, 0, 1) / 255.0 - mean) / std
        bound = torch.from_numpy(np.broadcast_to(PIL_LEVELS / (255.0 * std), pil.shape).copy()).to(DEV)
        ok, w, msg = within(got, torch.from_numpy(pil).to(DEV), bound, f'PIL fixture case {n}')
        assert ok, msg
        worst = max(worst, w * PIL_LEVELS)
    print(f'frame_transform vs PIL: worst {worst:.4f} grey levels')


def test_transform_modules_draw_seeded_boxes_and_match_the_restatement():
    from deepavfusion_amd.util.frame_transforms import EvalFrameTransform, TrainFrameTransform
    frames = _frames(8, 96, 128, 5)
    dev_frames = torch.from_numpy(frames).to(DEV)
    tf = TrainFrameTransform(64, scale=(0.5, 1.0), seed=11)
    a = tf(dev_frames)
    rows_a = tf.last_rows.clone()
    assert a.shape == (8, 3, 64, 64) and a.dtype == torch.float32 and rows_a.shape == (8, 9) and rows_a.dtype == torch.int32
    ok, _, msg = within(a, torch.from_numpy(R.transform_batch(frames, rows_a.numpy(), 64)).to(DEV), BOUND, 'TrainFrameTransform')
    assert ok, msg
    assert len({tuple(r) for r in rows_a.tolist()}) > 4                       # one independent draw per sample
    b = tf(dev_frames)
    assert not torch.equal(tf.last_rows, rows_a) and not torch.equal(a, b)    # a second call draws other boxes
    c = tf.seed(11)(dev_frames)
    assert torch.equal(tf.last_rows, rows_a) and torch.equal(a, c)            # re-seeding repeats them, bit for bit
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tf(torch.from_numpy(frames))
    ev = EvalFrameTransform(64)
    e = ev(dev_frames)
    assert ev.last_rows.tolist() == [[0, 0, 96, 128, 73, 97, 4, 16, 0]] * 8
    ok, _, msg = within(e, torch.from_numpy(R.transform_batch(frames, ev.last_rows.numpy(), 64)).to(DEV), BOUND, 'EvalFrameTransform')
    assert ok, msg
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ev(torch.from_numpy(frames))


def _write_shards(path, partition, n, seed):
    from deepavfusion_amd.util.clip_shards import ClipShardWriter
    g = np.random.default_rng(seed)
    F, dur, rate, ncls = 6, 3.0, 16000, 4
    protos = g.integers(0, 256, (ncls, 96, 128, 3)).astype(np.float64)
    tone = np.arange(int(dur * rate)) / rate
    with ClipShardWriter(str(path), partition, F, (96, 128), [(k + 0.5) * dur / F for k in range(F)], rate, dur,
                         [f'class{c}' for c in range(ncls)]) as w:
        for k in range(n):
            c = k % ncls
            frames = np.clip(protos[c][None] + g.normal(0, 20, (F, 96, 128, 3)), 0, 255).astype(np.uint8)
            audio = 0.3 * np.sin(2 * np.pi * (300 + 400 * c) * tone) + 0.05 * g.normal(size=tone.size)
            w.add(frames, (np.clip(audio, -1, 1) * 32767).astype(np.int16), c)


@pytest.mark.fresh_process
@pytest.mark.timeout(360)
def test_train_py_trains_probes_and_resumes_on_clip_shards(tmp_path):
    """train.py on a 24-clip labelled shard set (96 x 128 frames, 3 s at 16 kHz) as a fresh process: ViT-Tiny, 64 px + 2 s audio,
    captured step, device-side frame and audio front-ends, the nearest-neighbour probe on the shard set's test partition,
    checkpoint written; a second invocation resumes from it."""
    data = tmp_path / 'data'
    _write_shards(data, 'train', 24, 0)
    _write_shards(data, 'test', 24, 1)
    over = ['model.image.backbone=vit_tiny', 'model.audio.backbone=vit_tiny', 'model.fusion.num_heads=3', 'data.image_size=64',
            'data.audio_dur=2.', 'opt.batch_size=4', 'opt.warmup_epochs=1', 'log.print_freq=1',
            f'output_dir={tmp_path}', 'job_name=t', 'env.workers=2', 'data.dataset=shards', f'data.data_path={data}',
            'nn_probe.dataset=shards', 'nn_probe.batch_size=16']
    ckpt = os.path.join(str(tmp_path), 't', 'checkpoints', 'checkpoint_latest.pth')
    for run, (epochs, n_steps) in enumerate(((2, 12), (3, 18))):
        proc = subprocess.Popen([sys.executable, os.path.join(ROOT, 'train.py')] + over + [f'opt.epochs={epochs}'], cwd=ROOT,
                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        try:
            stdout, stderr = proc.communicate(timeout=170)
        finally:
            if proc.poll() is None:                              # the child is always reaped
                proc.kill()
                proc.communicate()
        assert proc.returncode == 0, stdout[-3000:] + stderr[-3000:]
        losses = [float(v) for v in re.findall(r'\[Train\]\[Ep-\d+/\d+\] step \d+/6  loss ([-\w.]+)', stdout)]
        assert len(losses) == (12 if run == 0 else 6) and all(np.isfinite(losses)), stdout[-3000:]
        probes = re.findall(r'\[NN-probe\]\[Ep-(\d+)/\d+\] (\{.*\})$', stdout, re.M)
        assert probes, stdout[-3000:]
        last = ast.literal_eval(probes[-1][1])
        assert list(last) == ['audio_nn_acc', 'image_nn_acc', 'fusion_nn_acc', 'all_nn_acc']
        assert all(0.0 <= v <= 100.0 for v in last.values())
        ck = torch.load(ckpt, map_location='cpu')
        assert ck['epoch'] == epochs and int(ck['n_steps']) == n_steps        # 24 clips / batch 4 = 6 steps per epoch
