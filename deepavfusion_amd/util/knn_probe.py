"""Nearest-neighbour probe of the pre-training worker: util/knn_probe.py of the reference (EvalAVNNProbe), on the MI355X path.

Every eval clip is encoded (``model.forward_encoder(image, spec)[:3]``), its image, audio and fusion tokens are mean-pooled and
L2-normalised (dav_mean_l2n_f32), gathered over the data-parallel group, and every clip is scored against every other in the three
modalities and their sum by ONE call of the fused similarity + top-k kernel (dav_knn_topk_f32, k = 2, no score matrix in memory).
As in the reference the prediction of a clip is the label of its 2nd neighbour (position 1: the 1st is normally the clip itself)
and the metrics are ``{audio,image,fusion,all}_nn_acc`` (single-label) or ``_nn_ap`` / ``_nn_auc`` (multi-hot labels).

Documented differences from the reference:
  - the features come from the product bf16 engine — the same forward the training step runs; the reference's ``evaluate`` runs
    its encoder in fp32 (it is called outside autocast).  The LayerNorm-folding path (DAV_LN_FUSE) is switched off for the
    probe's forward, so it neither makes nor reads gamma-folded weight copies next to a captured training step;
  - the scores are exact-fp32 FMA chains in the kernel's fixed order, ties go to the lower bank index (torch.topk leaves the
    order of ties unspecified);
  - the loader order is re-seeded at every call (the same clips, in the same order, at every epoch), and DataLoader workers
    follow ``env.workers`` (the reference forces at least one);
  - ``dataset=synthetic`` is a labelled synthetic set (seeded class prototypes + seeded noise); ``dataset=shards`` reads a labelled
    clip-shard partition (util/clip_shards.py: pre-decoded clips, ``train=False``) and runs the reference's eval transforms on the
    device (EvalFrameTransform; Pad -> LogMelSpectrogram, no RandomVol; with ``audio_resample=gpu`` a set stored at its tracks' own
    rate goes through PrepareWaveform(gain=None): Resample -> Pad in one launch).  VGGSound / AudioSet by name need PyAV and torchaudio,
    which are not dependencies of this project.  Python callers may pass any dataset that yields
    ``(image, spec, {'class': label})`` — the reference's contract; multi-hot labels ([num_classes] per clip) select the AP / AUC
    metrics.

Beyond the reference (off unless ``nn_probe.k`` is set; the four metrics above do not change): the weighted k-nearest-neighbour
classifier of Wu et al. 2018 / DINO.  The bank is a labelled train partition (``bank_partition``, shards; ``bank_samples``,
synthetic) or, without one, the eval set itself with each query's own row excluded; the k nearest bank rows of a query vote for
their classes with the weight exp(similarity / temperature) (the sum view on the MEAN similarity of its modalities), by
dav_knn_topk_wide_f32 + dav_knn_vote_f32.  New keys after the reference's: ``{audio,image,fusion,all}_knn{k}_acc``, or
``_knn{k}_ap`` / ``_knn{k}_auc`` on the vote scores of multi-hot sets.

``nn_probe.metrics`` (multi-hot sets only; ``host`` by default): where AP / AUC are computed.  ``host``: the predictions and vote
scores are copied back and ``average_precision`` / ``roc_auc`` below run in numpy, as in the reference; ``device``: dav_ap_auc_f64
(ops.ap_auc) computes them per class for all four views in one call per protocol and only [4, C] doubles and the positives per
class come back — the ``seen`` mask, the error for a class every clip has and the mean stay on the host (``device_metrics``), the
keys and their order are the same.
"""
import warnings
from collections import OrderedDict

import numpy as np
import torch

from .. import engine as E
from .. import ops
from . import distributed as dist_utils

MODALITIES = ('audio', 'image', 'fusion', 'all')          # the reference's key order
_VIEW = {'image': 0, 'audio': 1, 'fusion': 2, 'all': 3}   # kernel views: modalities passed as (image, audio, fusion), sum = view 3


class SyntheticLabelledAV(torch.utils.data.Dataset):
    """Class c has a fixed seeded prototype frame (ImageNet-normalised scale, N(0, 1)) and log-mel patch (about [-7, 4]); clip i
    is of class i % num_classes and is its prototype plus seeded Gaussian noise of std ``noise``.  ``offset`` shifts the indices:
    item i is clip offset + i of the same endless set (a bank disjoint from the eval clips: the same seed, the next indices)."""

    def __init__(self, n, num_classes, image_size, audio_size, seed=0, noise=0.5, offset=0):
        self.n, self.num_classes, self.seed, self.noise, self.offset = n, num_classes, seed, noise, int(offset)
        self.image_size, self.audio_size = tuple(image_size), tuple(audio_size)
        g = torch.Generator().manual_seed(seed * 1_000_003 + 7919)
        self.proto_image = torch.randn(num_classes, 3, *self.image_size, generator=g)
        self.proto_audio = (torch.randn(num_classes, 1, *self.audio_size, generator=g) * 2.0 - 3.0).clamp(-7, 4)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        i = i + self.offset
        c = i % self.num_classes
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + 104_729 + i)
        image = self.proto_image[c] + self.noise * torch.randn(3, *self.image_size, generator=g)
        spec = self.proto_audio[c] + self.noise * torch.randn(1, *self.audio_size, generator=g)
        return image, spec, {'class': c}


# ---- metrics: sklearn.metrics.average_precision_score / roc_auc_score (average=None), restated -------------------------------

def _binary_curve(y_true, y_score):
    """sklearn's _binary_clf_curve: cumulative true / false positives at every DISTINCT score, scores descending (ties grouped)."""
    order = np.argsort(y_score, kind='mergesort')[::-1]
    y_score, y_true = y_score[order], y_true[order].astype(np.float64)
    distinct = np.where(np.diff(y_score))[0]
    thr = np.r_[distinct, y_true.size - 1]
    tps = np.cumsum(y_true)[thr]
    fps = 1 + thr - tps
    return fps, tps


def average_precision(y_true, y_score):
    """Per-column AP of multi-hot labels [n, C] and scores [n, C]: sum over thresholds of (R_t - R_{t-1}) P_t."""
    out = np.empty(y_true.shape[1])
    for c in range(y_true.shape[1]):
        fps, tps = _binary_curve(y_true[:, c], y_score[:, c])
        precision = tps / (tps + fps)
        recall = tps / tps[-1] if tps[-1] > 0 else np.ones_like(tps)
        out[c] = np.sum(np.diff(np.r_[0.0, recall]) * precision)
    return out


def roc_auc(y_true, y_score):
    """Per-column ROC AUC (trapezoids over the distinct-threshold curve from (0, 0)); a column with one class only is an error,
    as in sklearn."""
    out = np.empty(y_true.shape[1])
    for c in range(y_true.shape[1]):
        fps, tps = _binary_curve(y_true[:, c], y_score[:, c])
        if tps[-1] <= 0 or fps[-1] <= 0:
            raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
        fpr, tpr = np.r_[0.0, fps / fps[-1]], np.r_[0.0, tps / tps[-1]]
        out[c] = np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2)
    return out


def probe_metrics(preds, labels, multi_label):
    """util/knn_probe.py:133-150: preds = {modality: (predicted labels [n] or [n, C], neighbour score [n])} (numpy), labels [n]
    or multi-hot [n, C] -> {'<mod>_nn_acc'} or {'<mod>_nn_ap', '<mod>_nn_auc'} in the order of ``preds``."""
    out = OrderedDict()
    if multi_label:
        seen = labels.sum(0) > 0
        for mod, (ypred, yscore) in preds.items():
            scores = ypred * yscore[:, None]
            out[f'{mod}_nn_ap'] = float(average_precision(labels[:, seen], scores[:, seen]).mean())
            out[f'{mod}_nn_auc'] = float(roc_auc(labels[:, seen], scores[:, seen]).mean())
    else:
        for mod, (ypred, _) in preds.items():
            out[f'{mod}_nn_acc'] = float(np.mean(ypred == labels) * 100)
    return dict(out)


def vote_metrics(scores, preds, labels, multi_label, k):
    """The weighted-vote keys, in the order of ``scores``: scores = {modality: vote scores [n, C]}, preds = {modality: voted
    class [n]} (single-label; unused for multi-hot), labels [n] or multi-hot [n, C] of the QUERIES (numpy) ->
    {'<mod>_knn<k>_acc'} or {'<mod>_knn<k>_ap', '<mod>_knn<k>_auc'} (AP / AUC over the classes that occur among the queries)."""
    out = OrderedDict()
    if multi_label:
        seen = labels.sum(0) > 0
        for mod, sc in scores.items():
            out[f'{mod}_knn{k}_ap'] = float(average_precision(labels[:, seen], sc[:, seen]).mean())
            out[f'{mod}_knn{k}_auc'] = float(roc_auc(labels[:, seen], sc[:, seen]).mean())
    else:
        for mod in scores:
            out[f'{mod}_knn{k}_acc'] = float(np.mean(preds[mod] == labels) * 100)
    return dict(out)


METRICS = ('host', 'device')                              # nn_probe.metrics


def metrics_mode(value):
    """nn_probe.metrics -> 'host' (also for a missing key) or 'device'; anything else is refused."""
    mode = 'host' if value is None else str(value)
    if mode not in METRICS:
        raise ValueError(f'nn_probe.metrics={value}: one of {", ".join(METRICS)}')
    return mode


def metrics_on_device(mode, multi_label, n):
    """Whether the AP / AUC of an evaluation over n clips run in dav_ap_auc_f64: asked for, a multi-hot set (single-label sets have
    accuracies only), and a column fits the kernel."""
    return metrics_mode(mode) == 'device' and bool(multi_label) and n <= ops.AP_AUC_MAX_ROWS


def device_metrics(ap, auc, pos, tag):
    """The host half of nn_probe.metrics=device: ap / auc [4, C] in the kernel's view order and pos [C] as ops.ap_auc returns
    them (numpy) -> {'<mod>_<tag>_ap', '<mod>_<tag>_auc'} over the classes that occur, the keys and their order as probe_metrics
    (tag 'nn') / vote_metrics (tag 'knn<k>') give them.  A class that occurs in every clip has no AUC: the error of roc_auc."""
    seen = pos > 0
    out = OrderedDict()
    for mod in MODALITIES:
        a = auc[_VIEW[mod]][seen]
        if np.isnan(a).any():
            raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
        out[f'{mod}_{tag}_ap'] = float(ap[_VIEW[mod]][seen].mean())
        out[f'{mod}_{tag}_auc'] = float(a.mean())
    return dict(out)


def knn_vote_scores(feats, bank_feats, bank_labels, num_classes, k, temperature, exclude_self):
    """feats / bank_feats = (image, audio, fusion) features [n, D] / [N, D]; bank_labels class ids [N] or multi-hot [N, C].
    -> (vote scores [4, n, C], voted class [4, n] or None) in the kernel's view order (device tensors).  ``exclude_self``: the bank
    IS the query set, row q of it is skipped for query q (one more entry is fetched for it)."""
    kk = k + int(bool(exclude_self))
    val, idx = ops.knn_topk(feats, bank_feats, k=kk, sum_view=True)
    M = len(feats)
    inv_t = [1.0 / temperature] * M + [1.0 / (temperature * M)]              # the sum view votes on the mean similarity
    lab = bank_labels.to(torch.uint8) if bank_labels.dim() == 2 else bank_labels
    return ops.knn_vote(val, idx, lab, num_classes, k, inv_t, self_offset=0 if exclude_self else -1)


def knn_vote_predictions(feats, bank_feats, bank_labels, num_classes, k, temperature, exclude_self):
    """knn_vote_scores by modality: -> {modality: (vote scores [n, C], voted class [n] or None)} (device tensors)."""
    scores, pred = knn_vote_scores(feats, bank_feats, bank_labels, num_classes, k, temperature, exclude_self)
    return OrderedDict((mod, (scores[_VIEW[mod]], None if pred is None else pred[_VIEW[mod]])) for mod in MODALITIES)


def knn_neighbours(v_feats, a_feats, mm_feats, k=2):
    """util/knn_probe.py:113-128 as ONE kernel call: -> (index [4, n] of every clip's 2nd neighbour, its score [4, n]) in the
    kernel's view order (device tensors)."""
    val, idx = ops.knn_topk((v_feats, a_feats, mm_feats), (v_feats, a_feats, mm_feats), k=k, sum_view=True)
    return idx[:, :, 1], val[:, :, 1]


def knn_predictions(v_feats, a_feats, mm_feats, labels, k=2):
    """util/knn_probe.py:113-131: -> {modality: (labels of the 2nd neighbour, its score)} (device tensors)."""
    idx, val = knn_neighbours(v_feats, a_feats, mm_feats, k)
    return OrderedDict((mod, (labels[idx[_VIEW[mod]]], val[_VIEW[mod]])) for mod in MODALITIES)


class EvalAVNNProbe:
    def __init__(self, probe_args, log_args, env_args, dataset=None, bank_dataset=None):
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.distributed = dist_utils.get_world_size() > 1
        self.eval_freq = int(log_args.eval_freq)
        self.print_freq = int(log_args.print_freq)
        self.dataset = probe_args.get('dataset') if dataset is None else 'custom'
        self.seed = int(env_args.get('seed') or 0)
        self.frame_frontend = self.audio_frontend = None       # shards: raw frames / waveforms in, transforms on the device
        self.k = None if probe_args.get('k') is None else int(probe_args.get('k'))            # None: the reference's protocol only
        self.temperature = float(probe_args.get('temperature') or 0.07)
        self.metrics = metrics_mode(probe_args.get('metrics'))                               # multi-hot sets: where AP / AUC run
        self._metrics_warned = False
        if self.k is not None and not 1 <= self.k < ops.KNN_MAX_K:
            raise ValueError(f'nn_probe.k={self.k}: the weighted vote takes 1 .. {ops.KNN_MAX_K - 1} neighbours')
        if self.k is not None and not self.temperature > 0:
            raise ValueError(f'nn_probe.temperature={self.temperature} must be positive')
        self.bank_db = bank_dataset
        bank_samples, bank_partition = probe_args.get('bank_samples'), probe_args.get('bank_partition')
        if self.k is None and (bank_dataset is not None or bank_samples or bank_partition):
            raise ValueError('a bank (nn_probe.bank_samples / bank_partition) is used by the weighted vote only: set nn_probe.k')
        if dataset is not None:
            self.db, self.multi_label = dataset, None          # decided by the label shape
        elif self.dataset == 'synthetic':
            image_size = (int(probe_args.image_size),) * 2
            audio_size = (int(probe_args.audio_mels), int(float(probe_args.audio_dur) * 64))
            self.db = SyntheticLabelledAV(int(probe_args.num_samples), int(probe_args.num_classes), image_size, audio_size,
                                          seed=self.seed)
            self.multi_label = False
            if bank_partition:
                raise ValueError('nn_probe.bank_partition names a shard partition; the synthetic set takes nn_probe.bank_samples')
        elif self.dataset == 'shards':
            from . import audio_transforms as aT
            from .clip_shards import ClipShards
            from .frame_transforms import EvalFrameTransform
            if not probe_args.get('data_path'):
                raise ValueError('nn_probe.dataset=shards needs nn_probe.data_path (default: data.data_path)')
            resample = probe_args.get('audio_resample', 'off') == 'gpu'      # a set stored at its tracks' own rate: resampled on the device
            self.db = ClipShards(probe_args.data_path, probe_args.get('partition') or 'test', audio_dur=float(probe_args.audio_dur),
                                 audio_rate=int(probe_args.audio_rate), train=False, seed=self.seed, resample=resample)
            if not self.db.has_labels:
                raise ValueError(f'{self.db.dir} has no labels.npy: the nearest-neighbour probe needs a labelled shard set')
            self.multi_label = self.db.multi_label
            if bank_samples:
                raise ValueError('nn_probe.bank_samples belongs to the synthetic set; shards take nn_probe.bank_partition')
            if bank_partition:
                self.bank_db = ClipShards(probe_args.data_path, bank_partition, audio_dur=float(probe_args.audio_dur),
                                          audio_rate=int(probe_args.audio_rate), train=False, seed=self.seed, resample=resample)
                if not self.bank_db.has_labels or self.bank_db.multi_label != self.multi_label:
                    raise ValueError(f'{self.bank_db.dir}: the bank needs labels of the same kind as {self.db.dir}')
                if self.bank_db.stored_rate != self.db.stored_rate:
                    raise ValueError(f'{self.bank_db.dir} holds audio at {self.bank_db.stored_rate} Hz, {self.db.dir} at '
                                     f'{self.db.stored_rate} Hz: the bank and the evaluation set share one front-end')
            self.frame_frontend = EvalFrameTransform(int(probe_args.image_size))
            if resample:                 # Resample -> Pad in one launch, no RandomVol (gain=None); int16 windows in
                pad = aT.PrepareWaveform(self.db.stored_rate, int(probe_args.audio_rate), float(probe_args.audio_dur), gain=None)
            else:
                pad = aT.Pad(float(probe_args.audio_dur), int(probe_args.audio_rate))
            self.audio_frontend = aT.Compose([pad, aT.LogMelSpectrogram(int(probe_args.audio_rate), int(probe_args.audio_mels))])
        elif self.dataset in ('vggsound', 'audioset'):
            raise NotImplementedError(f'nn_probe.dataset={self.dataset}: synthetic and shards are on the MI355X path '
                                      '(the reference datasets need PyAV/torchaudio; decode them with tools/make_shards.py)')
        else:
            raise NotImplementedError(f'nn_probe.dataset={self.dataset}')
        if bank_samples:                                       # the next bank_samples clips of the same synthetic set
            if not isinstance(self.db, SyntheticLabelledAV) or bank_dataset is not None:
                raise ValueError('nn_probe.bank_samples needs the synthetic set (and no bank_dataset)')
            d = self.db
            self.bank_db = SyntheticLabelledAV(int(bank_samples), d.num_classes, d.image_size, d.audio_size, seed=d.seed,
                                               noise=d.noise, offset=d.offset + len(d))
        if self.distributed:
            self.generator = None
            self.sampler = torch.utils.data.DistributedSampler(self.db, num_replicas=dist_utils.get_world_size(),
                                                               rank=dist_utils.get_rank(), shuffle=True, seed=self.seed)
        else:
            self.generator = torch.Generator()
            self.sampler = torch.utils.data.RandomSampler(self.db, generator=self.generator)
        self.loader = torch.utils.data.DataLoader(self.db, sampler=self.sampler, batch_size=max(int(probe_args.batch_size) // 4, 1),
                                                  num_workers=int(env_args.get('workers') or 0), pin_memory=False, drop_last=True)
        self.bank_loader = None
        if self.bank_db is not None:
            # every bank clip once, in order (no drop_last); ranks take contiguous runs of equal length for the gather, which leaves
            # out at most world_size - 1 clips at the end of the set
            world, rank = dist_utils.get_world_size(), dist_utils.get_rank()
            per = len(self.bank_db) // world
            self.bank_loader = torch.utils.data.DataLoader(
                torch.utils.data.Subset(self.bank_db, range(rank * per, (rank + 1) * per)), shuffle=False,
                batch_size=max(int(probe_args.batch_size) // 4, 1), num_workers=int(env_args.get('workers') or 0),
                pin_memory=False, drop_last=False)

    @torch.no_grad()
    def extract(self, model):
        """util/knn_probe.py:84-111: -> normalised (image, audio, fusion) features [n, D] and labels, gathered over the group."""
        model.train(False)
        if self.distributed:
            self.sampler.set_epoch(0)
        else:
            self.generator.manual_seed(self.seed)
        return self._extract(model, self.loader)

    @torch.no_grad()
    def extract_bank(self, model):
        """The bank's features and labels, as ``extract`` (eval transforms, LayerNorm folding off, gathered over the group)."""
        model.train(False)
        return self._extract(model, self.bank_loader)

    def _extract(self, model, loader):
        feats, labels = ([], [], []), []
        prev = E.LN_FUSE_MODE
        E.set_ln_fuse('off')
        try:
            for image, spec, anno in loader:
                spec = spec.to(self.device, non_blocking=True)
                if spec.dtype != torch.int16:                     # int16: raw windows of audio_resample=gpu, scaled by the kernel
                    spec = spec.float()
                image = image.to(self.device, non_blocking=True)
                image = self.frame_frontend(image) if self.frame_frontend is not None else image.float()
                if self.audio_frontend is not None:
                    spec = self.audio_frontend(spec)
                lbl = anno['class'].to(self.device, non_blocking=True).long()
                for f, x in zip(feats, model.forward_encoder(image, spec)[:3]):      # x_v, x_a, x_mm
                    f.append(ops.mean_l2n(x))
                labels.append(lbl)
        finally:
            E.set_ln_fuse(prev)
        v_feats, a_feats, mm_feats = (dist_utils.concat_all_gather(torch.cat(f)) for f in feats)
        return v_feats, a_feats, mm_feats, dist_utils.concat_all_gather(torch.cat(labels))

    @torch.no_grad()
    def evaluate(self, model, epoch=0):
        v_feats, a_feats, mm_feats, labels = self.extract(model)
        multi_label = self.multi_label if self.multi_label is not None else labels.dim() == 2
        truth = None                                           # metrics=device: the multi-hot labels as uint8, made once
        if metrics_on_device(self.metrics, multi_label, labels.shape[0]):
            # the reference's ypred * yscore[:, None] is formed inside the kernel from the neighbour's row of the labels
            truth = labels.to(torch.uint8)
            idx, val = knn_neighbours(v_feats, a_feats, mm_feats)
            ap, auc, pos = ops.ap_auc(truth, nbr=idx, nbr_val=val, nbr_labels=truth)
            out = device_metrics(ap.cpu().numpy(), auc.cpu().numpy(), pos.cpu().numpy(), 'nn')
        else:
            if self.metrics == 'device' and multi_label and not self._metrics_warned:
                self._metrics_warned = True
                warnings.warn(f'nn_probe.metrics=device holds up to {ops.AP_AUC_MAX_ROWS} clips, the set has {labels.shape[0]}: '
                              'AP / AUC run on the host')
            preds = knn_predictions(v_feats, a_feats, mm_feats, labels)
            out = probe_metrics(OrderedDict((m, (p.cpu().numpy(), s.cpu().numpy())) for m, (p, s) in preds.items()),
                                labels.cpu().numpy(), multi_label)
        if self.k is not None:
            out.update(self._vote(model, (v_feats, a_feats, mm_feats), labels, multi_label, truth))
        return out

    def _vote(self, model, feats, labels, multi_label, truth=None):
        """``truth``: the queries' multi-hot labels as uint8 when AP / AUC run on the device (evaluate), else None."""
        if self.bank_loader is not None:
            *bank, bank_labels = self.extract_bank(model)
        else:
            bank, bank_labels = feats, labels if truth is None else truth      # the eval set against itself, own rows excluded
        if multi_label:
            C = labels.shape[1]
        else:
            C = int(torch.maximum(labels.max(), bank_labels.max())) + 1
        if truth is not None:                                  # all four views in one call; [4, C] doubles and pos come back
            scores, _ = knn_vote_scores(feats, tuple(bank), bank_labels, C, self.k, self.temperature,
                                        exclude_self=self.bank_loader is None)
            ap, auc, pos = ops.ap_auc(truth, scores)
            return device_metrics(ap.cpu().numpy(), auc.cpu().numpy(), pos.cpu().numpy(), f'knn{self.k}')
        votes = knn_vote_predictions(feats, tuple(bank), bank_labels, C, self.k, self.temperature,
                                     exclude_self=self.bank_loader is None)
        return vote_metrics(OrderedDict((m, s.cpu().numpy()) for m, (s, _) in votes.items()),
                            None if multi_label else OrderedDict((m, p.cpu().numpy()) for m, (_, p) in votes.items()),
                            labels.cpu().numpy(), multi_label, self.k)
