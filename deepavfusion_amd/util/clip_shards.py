"""Clip shards: pre-decoded audio-visual clips in flat, memory-mapped arrays — the dataset behind ``data.dataset=shards``.

The reference decodes mp4 files with PyAV inside its loader workers (datasets.py:222-243, avreader.py); PyAV is not a dependency
of this project.  Clips are decoded ONCE, offline (tools/make_shards.py), into

    <data_path>/<partition>/meta.json    version, num_clips N, frames_per_clip F, frame_hw [H, W], frame_times [F] (seconds from
                                         the clip's start), audio_rate, clip_dur, class_names | null, multi_label
                            frames.u8    raw uint8 [N, F, H, W, 3]
                            audio.i16    raw int16 mono [N, round(clip_dur * audio_rate)]
                            labels.npy   int64 [N], or uint8 multi-hot [N, C]   (only for labelled sets)

and ``ClipShards`` serves them as the reference's VideoDataset does: an audio window of ``audio_dur`` seconds (random position
with ``train=True``, centred otherwise), one stored frame from inside that window, and the annotation.  What it yields is RAW —
a uint8 frame [H, W, 3] and the waveform in [-1, 1] — because the transforms run on the device
(util/frame_transforms.py, util/audio_transforms.py).  One frame size, one frame-time grid and one audio rate per shard set;
there is no resampler in the loader: a set kept at its tracks' own rate (make_shards.py --keep-rate) is resampled on the device
(``ClipShards(resample=True)``, data.audio_resample=gpu)."""
import json
import os

import numpy as np
import torch

VERSION = 1
META, FRAMES, AUDIO, LABELS = 'meta.json', 'frames.u8', 'audio.i16', 'labels.npy'


class ClipShardWriter:
    """Appends clips to <path>/<partition>/.  ``add(frames uint8 [F, H, W, 3], audio int16 [round(clip_dur * audio_rate)],
    label)``; a clip of another shape, dtype or length is refused.  Labels: none at all, an int class per clip, or (multi_label)
    a multi-hot vector [len(class_names)] per clip.  ``close()`` writes meta.json and labels.npy (also on leaving a ``with``)."""

    def __init__(self, path, partition, frames_per_clip, frame_hw, frame_times, audio_rate, clip_dur, class_names=None,
                 multi_label=False):
        self.dir = os.path.join(path, partition)
        os.makedirs(self.dir, exist_ok=True)
        self.F, self.hw = int(frames_per_clip), (int(frame_hw[0]), int(frame_hw[1]))
        self.frame_times = [float(t) for t in frame_times]
        self.audio_rate, self.clip_dur = int(audio_rate), float(clip_dur)
        self.samples = int(round(self.clip_dur * self.audio_rate))
        if len(self.frame_times) != self.F or self.F < 1:
            raise ValueError(f'{len(self.frame_times)} frame times for {self.F} frames per clip')
        if any(not 0.0 <= t <= self.clip_dur for t in self.frame_times) or sorted(self.frame_times) != self.frame_times:
            raise ValueError('frame times must ascend inside [0, clip_dur]')
        if self.samples < 1:
            raise ValueError('an empty audio track')
        self.class_names = list(class_names) if class_names is not None else None
        self.multi_label = bool(multi_label)
        if self.multi_label and self.class_names is None:
            raise ValueError('multi-hot labels need class_names')
        self.labels = []
        self.n = 0
        self._frames = open(os.path.join(self.dir, FRAMES), 'wb')
        self._audio = open(os.path.join(self.dir, AUDIO), 'wb')

    def add(self, frames, audio, label=None):
        frames, audio = np.asarray(frames), np.asarray(audio)
        if frames.dtype != np.uint8 or frames.shape != (self.F, *self.hw, 3):
            raise ValueError(f'frames {frames.dtype} {frames.shape}: this shard set holds uint8 {(self.F, *self.hw, 3)}')
        if audio.dtype != np.int16 or audio.shape != (self.samples,):
            raise ValueError(f'audio {audio.dtype} {audio.shape}: this shard set holds int16 mono ({self.samples},) '
                             f'= {self.clip_dur} s at {self.audio_rate} Hz')
        if self.n > 0 and (label is not None) != bool(self.labels):
            raise ValueError('either every clip of a shard set has a label or none has')
        if label is not None:
            if self.multi_label:
                label = np.asarray(label)
                if label.shape != (len(self.class_names),) or not np.isin(label, (0, 1)).all():
                    raise ValueError(f'a multi-hot label of shape ({len(self.class_names)},) is needed, got {label.shape}')
                label = label.astype(np.uint8)
            else:
                label = int(label)
                if label < 0 or (self.class_names is not None and label >= len(self.class_names)):
                    raise ValueError(f'class {label} out of range')
            self.labels.append(label)
        self._frames.write(np.ascontiguousarray(frames).tobytes())
        self._audio.write(np.ascontiguousarray(audio).tobytes())
        self.n += 1

    def close(self):
        if self._frames is None:
            return
        self._frames.close()
        self._audio.close()
        self._frames = self._audio = None
        lab = os.path.join(self.dir, LABELS)
        if self.labels:
            np.save(lab, np.stack(self.labels).astype(np.uint8) if self.multi_label else np.asarray(self.labels, np.int64))
        elif os.path.exists(lab):
            os.remove(lab)
        meta = dict(version=VERSION, num_clips=self.n, frames_per_clip=self.F, frame_hw=list(self.hw), frame_times=self.frame_times,
                    audio_rate=self.audio_rate, clip_dur=self.clip_dur, class_names=self.class_names, multi_label=self.multi_label)
        with open(os.path.join(self.dir, META), 'w') as f:
            json.dump(meta, f, indent=1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ClipShards(torch.utils.data.Dataset):
    """``ds[k]`` -> (frame uint8 [H, W, 3], waveform fp32 [samples] in [-1, 1], anno), datasets.py:222-243 of the reference:
    with ``train`` the window's midpoint is uniform in [audio_dur / 2, clip_dur - audio_dur / 2], otherwise clip_dur / 2;
    start = midpoint - audio_dur / 2; the frame is a random stored frame with start <= t <= start + audio_dur (the reference's
    quick_random_frame), the nearest to the window if none lies inside; the waveform is the samples of [start, start + audio_dur).
    A clip no longer than ``audio_dur`` comes back whole from start = 0 (audio_transforms.Pad mirrors it out on the device).
    ``anno`` is {'class': label} for a labelled set, else the index.

    ``resample=True`` accepts a set stored at another rate than ``audio_rate`` (``stored_rate``, from meta.json): the window is cut
    at the stored rate, as the reference cuts before it resamples — int(audio_dur * stored_rate) samples from
    round(start * stored_rate) — and comes back as raw int16 (half the bytes to the device) for
    audio_transforms.PrepareWaveform(stored_rate, audio_rate, audio_dur), which scales, resamples and pads it there.

    The draws are a pure function of (seed, epoch, index) — ``set_epoch`` — not of worker scheduling: a run repeats with any number
    of loader workers.  With ``train=False`` the epoch is left out too: the same frame of the same clip at every call.  The arrays
    are memory-mapped lazily, in the process (loader worker) that first reads them."""

    def __init__(self, path, partition='train', audio_dur=3.0, audio_rate=16000, train=True, seed=0, resample=False):
        self.dir = os.path.join(str(path), partition)
        if not os.path.isfile(os.path.join(self.dir, META)):
            raise FileNotFoundError(f'{self.dir}: no {META} (write a shard set with tools/make_shards.py or ClipShardWriter)')
        with open(os.path.join(self.dir, META)) as f:
            m = json.load(f)
        if m.get('version') != VERSION:
            raise ValueError(f'{self.dir}: shard format version {m.get("version")}, this reader knows {VERSION}')
        self.n, self.F = int(m['num_clips']), int(m['frames_per_clip'])
        self.hw = tuple(int(v) for v in m['frame_hw'])
        self.frame_times = np.asarray(m['frame_times'], np.float64)
        self.audio_rate, self.clip_dur = int(m['audio_rate']), float(m['clip_dur'])
        self.class_names, self.multi_label = m.get('class_names'), bool(m.get('multi_label'))
        self.stored_rate = self.audio_rate
        self.resample = bool(resample)
        if int(audio_rate) != self.stored_rate and not resample:
            raise ValueError(f'{self.dir} holds audio at {self.audio_rate} Hz, {audio_rate} Hz asked for: there is no resampler, '
                             'set data.audio_rate to the stored rate or rebuild the shards (or resample on the device: '
                             'ClipShards(resample=True), data.audio_resample=gpu)')
        self.audio_rate = int(audio_rate)                          # the rate asked for; stored_rate is what the files hold
        self.samples = int(round(self.clip_dur * self.stored_rate))
        self.audio_dur, self.train, self.seed, self.epoch = float(audio_dur), bool(train), int(seed), 0
        self.window = min(int(self.audio_dur * self.stored_rate), self.samples)
        for name, size in ((FRAMES, self.n * self.F * self.hw[0] * self.hw[1] * 3), (AUDIO, self.n * self.samples * 2)):
            have = os.path.getsize(os.path.join(self.dir, name))
            if have != size:
                raise ValueError(f'{self.dir}/{name}: {have} bytes, {META} describes {size}')
        self.has_labels = os.path.isfile(os.path.join(self.dir, LABELS))
        self._frames = self._audio = self._labels = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d['_frames'] = d['_audio'] = d['_labels'] = None          # a worker maps the files itself
        return d

    def _open(self):
        if self._frames is None:
            self._frames = np.memmap(os.path.join(self.dir, FRAMES), np.uint8, 'r', shape=(self.n, self.F, *self.hw, 3))
            self._audio = np.memmap(os.path.join(self.dir, AUDIO), np.int16, 'r', shape=(self.n, self.samples))
            if self.has_labels:
                self._labels = np.load(os.path.join(self.dir, LABELS))
                if self._labels.shape[0] != self.n:
                    raise ValueError(f'{self.dir}/{LABELS}: {self._labels.shape[0]} labels for {self.n} clips')

    @property
    def labels(self):
        self._open()
        return self._labels

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.n

    def sample(self, idx):
        """The draw of clip ``idx`` under the current (seed, epoch): -> (start in seconds, index of the stored frame)."""
        rng = np.random.default_rng([self.seed, self.epoch if self.train else 0, int(idx), int(self.train)])
        if self.clip_dur <= self.audio_dur:
            start = 0.0
        elif self.train:
            start = float(rng.uniform(self.audio_dur / 2, self.clip_dur - self.audio_dur / 2)) - self.audio_dur / 2
        else:
            start = self.clip_dur / 2 - self.audio_dur / 2
        start = min(max(start, 0.0), max(self.clip_dur - self.audio_dur, 0.0))
        inside = np.nonzero((self.frame_times >= start) & (self.frame_times <= start + self.audio_dur))[0]
        if inside.size:
            f = int(inside[rng.integers(inside.size)])
        else:
            mid = np.clip(self.frame_times, start, start + self.audio_dur)
            f = int(np.argmin(np.abs(self.frame_times - mid)))
        return start, f

    def __getitem__(self, idx):
        idx = int(idx)
        if not 0 <= idx < self.n:
            raise IndexError(idx)
        self._open()
        start, f = self.sample(idx)
        s0 = min(int(round(start * self.stored_rate)), self.samples - self.window)
        frame = torch.from_numpy(np.array(self._frames[idx, f]))
        if self.resample:                                          # cut at the stored rate, raw: the device scales and resamples
            wave = torch.from_numpy(np.array(self._audio[idx, s0:s0 + self.window]))
        else:
            wave = torch.from_numpy(np.asarray(self._audio[idx, s0:s0 + self.window], np.float32) / 32768.0)
        if self._labels is None:
            return frame, wave, idx
        lab = self._labels[idx]
        return frame, wave, {'class': torch.from_numpy(np.array(lab)) if self.multi_label else int(lab)}
