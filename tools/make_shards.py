#!/usr/bin/env python3
"""Builds a clip-shard partition (deepavfusion_amd/util/clip_shards.py, INTEGRATION.md "Clip shards") from decoded clips:

    <src>/<clip>/frames/*.jpg|*.png     the clip's frames in name order, evenly spaced over the clip
          <clip>/audio.wav              its sound track: 16-bit PCM (stereo is averaged to mono)
    <src>/labels.csv                    optional: "<clip>,<class name>[;<class name>...]" per line

    python tools/make_shards.py <src> <data_path> --partition train --hw 256 340 --frames 8 --clip-dur 10 --audio-rate 16000

Every frame is resized on its short side and centre-cropped on its long side to the one H x W of the set (PIL, bilinear); a clip
with fewer frames than --frames, a track at another rate (there is no resampler) or shorter than --clip-dur is refused by name.
--frames frames are taken evenly from those present, frame k at time (k + 0.5) clip_dur / frames.  More than one class on a line
makes the set multi-label.  --keep-rate stores the tracks at their OWN rate instead of --audio-rate (44.1 or 48 kHz as decoded; all
tracks of a set must share it, one at another rate is refused by name) and records it in meta.json: train.py resamples such a set
on the device (data.audio_resample=gpu), with the filter the reference's loader applies.  PIL and wave are needed by this tool only."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_frame(path, H, W):
    from PIL import Image
    im = Image.open(path).convert('RGB')
    s = max(H / im.height, W / im.width)                         # cover H x W: short side resized, long side cropped
    rw, rh = max(W, int(round(im.width * s))), max(H, int(round(im.height * s)))
    im = im.resize((rw, rh), Image.BILINEAR)
    left, top = (rw - W) // 2, (rh - H) // 2
    return np.asarray(im.crop((left, top, left + W, top + H)), np.uint8)


def load_wav(path, rate, samples):
    import wave
    with wave.open(path, 'rb') as w:
        if w.getsampwidth() != 2:
            raise ValueError(f'{path}: {8 * w.getsampwidth()}-bit samples, 16-bit PCM needed')
        if w.getframerate() != rate:
            raise ValueError(f'{path}: {w.getframerate()} Hz, the set holds {rate} Hz (resample it first: there is no resampler here)')
        x = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())
    if x.shape[0] < samples:
        raise ValueError(f'{path}: {x.shape[0]} samples, {samples} needed')
    x = x[:samples].astype(np.int32)
    return (x.sum(1) // x.shape[1]).astype(np.int16)


def wav_rate(path):
    import wave
    with wave.open(path, 'rb') as w:
        return w.getframerate()


def read_labels(path):
    out = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith('#'):
                clip, _, names = line.partition(',')
                out[clip.strip()] = [n.strip() for n in names.split(';') if n.strip()]
    return out


def main():
    from deepavfusion_amd.util.clip_shards import ClipShardWriter
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('src')
    ap.add_argument('data_path')
    ap.add_argument('--partition', default='train')
    ap.add_argument('--hw', type=int, nargs=2, default=(256, 340), metavar=('H', 'W'))
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--clip-dur', type=float, default=10.0)
    ap.add_argument('--audio-rate', type=int, default=16000)
    ap.add_argument('--keep-rate', action='store_true',
                    help="store the tracks at their own (shared) rate, not --audio-rate; resampled on the device (data.audio_resample=gpu)")
    a = ap.parse_args()
    H, W = a.hw
    clips = sorted(d for d in os.listdir(a.src) if os.path.isdir(os.path.join(a.src, d, 'frames')))
    if not clips:
        raise SystemExit(f'{a.src}: no <clip>/frames/ folders')
    labels = read_labels(os.path.join(a.src, 'labels.csv')) if os.path.isfile(os.path.join(a.src, 'labels.csv')) else None
    names, multi = None, False
    if labels is not None:
        missing = [c for c in clips if not labels.get(c)]
        if missing:
            raise SystemExit(f'labels.csv has no class for {missing[:5]}')
        names = sorted({n for c in clips for n in labels[c]})
        multi = any(len(labels[c]) > 1 for c in clips)
    if a.keep_rate:                                              # the set's rate is the first track's; load_wav refuses any other by name
        a.audio_rate = wav_rate(os.path.join(a.src, clips[0], 'audio.wav'))
    times = [(k + 0.5) * a.clip_dur / a.frames for k in range(a.frames)]
    samples = int(round(a.clip_dur * a.audio_rate))
    with ClipShardWriter(a.data_path, a.partition, a.frames, (H, W), times, a.audio_rate, a.clip_dur, names, multi) as wr:
        for c in clips:
            files = sorted(f for f in os.listdir(os.path.join(a.src, c, 'frames')) if f.lower().endswith(('.jpg', '.jpeg', '.png')))
            if len(files) < a.frames:
                raise SystemExit(f'{c}: {len(files)} frames, {a.frames} needed')
            pick = [files[int((k + 0.5) * len(files) / a.frames)] for k in range(a.frames)]
            frames = np.stack([load_frame(os.path.join(a.src, c, 'frames', f), H, W) for f in pick])
            audio = load_wav(os.path.join(a.src, c, 'audio.wav'), a.audio_rate, samples)
            label = None
            if labels is not None:
                ids = [names.index(n) for n in labels[c]]
                label = np.isin(np.arange(len(names)), ids).astype(np.uint8) if multi else ids[0]
            wr.add(frames, audio, label)
    print(f'{wr.dir}: {wr.n} clips, {a.frames} frames of {H} x {W}, {a.clip_dur} s at {a.audio_rate} Hz'
          + (f', {len(names)} classes' + (' (multi-label)' if multi else '') if names else ', no labels'))


if __name__ == '__main__':
    main()
