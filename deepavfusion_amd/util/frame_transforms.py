"""Frame transforms of the reference on the GPU: the image half of the input stage, next to util/audio_transforms.py.

    train.py:45-49            RandomResizedCrop(size, scale=(crop_min, 1)) -> RandomHorizontalFlip -> ToTensor -> Normalize
    util/knn_probe.py:31-36   Resize(int(size / 0.875)) -> CenterCrop(size) -> ToTensor -> Normalize

The loader ships uint8 frames [B, H, W, 3]; the per-sample parameters (crop box, flip) are drawn on the host, one independent
draw per sample as B per-sample dataset calls would make, and ONE kernel (csrc/data/frames.hip, dav_frame_transform_u8) crops,
resamples, flips and normalises the whole batch into fp32 [B, 3, size, size].

torchvision is not a dependency of this project: ``random_resized_crop_params`` and ``resize_center_crop_params`` restate the
published algorithms of torchvision.transforms.RandomResizedCrop.get_params, Resize and CenterCrop (as the HTK filterbank of
audio_transforms.py restates torchaudio's).  Documented difference from PIL's resize, which the reference runs: no rounding to
uint8 between the two passes or at the end (at most 1 grey level)."""
import math

import torch

from .. import ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)       # train.py:49
IMAGENET_STD = (0.229, 0.224, 0.225)


def random_resized_crop_params(H, W, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), generator=None):
    """torchvision.transforms.RandomResizedCrop.get_params, restated from its published algorithm -> (i, j, h, w).
    Ten attempts: area = H W U(scale), aspect ratio log-uniform in ``ratio``, w = int(round(sqrt(area ratio))),
    h = int(round(sqrt(area / ratio))), accepted if the box fits, at a uniform position; otherwise the central crop with the
    frame's aspect ratio clamped into ``ratio``."""
    area = H * W
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect = math.exp(torch.empty(1).uniform_(log_lo, log_hi, generator=generator).item())
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            i = torch.randint(0, H - h + 1, size=(1,), generator=generator).item()
            j = torch.randint(0, W - w + 1, size=(1,), generator=generator).item()
            return i, j, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def resize_center_crop_params(H, W, size, crop_pct=0.875):
    """Resize(int(size / crop_pct)) on the shorter side (the longer one int(s long / short)) and CenterCrop(size)
    -> ((RH, RW), (top, left)); the offsets are torchvision's int(round((R - size) / 2.0)) — Python's round, half to even."""
    s = int(size / crop_pct)
    if H <= W:
        RH, RW = s, int(s * W / H)
    else:
        RH, RW = int(s * H / W), s
    if RH < size or RW < size:
        raise ValueError(f'a {H} x {W} frame resized to {RH} x {RW} is smaller than the {size} x {size} crop')
    return (RH, RW), (int(round((RH - size) / 2.0)), int(round((RW - size) / 2.0)))


def check_rows(rows, H, W, size):
    """Host-side validation of parameter rows [i, j, h, w, RH, RW, top, left, flip] before upload (the kernel clamps what it is
    given: a bad row would give a wrong picture silently)."""
    for r in rows:
        i, j, h, w, RH, RW, top, left, flip = r
        if not (0 <= i and 0 <= j and h >= 1 and w >= 1 and i + h <= H and j + w <= W):
            raise ValueError(f'source window {(i, j, h, w)} leaves the {H} x {W} frame')
        if not (0 <= top and 0 <= left and top + size <= RH and left + size <= RW):
            raise ValueError(f'the {size} x {size} window at {(top, left)} leaves the {RH} x {RW} resampled picture')
        if flip not in (0, 1):
            raise ValueError(f'flip flag {flip}')


class _FrameTransform(torch.nn.Module):
    def __init__(self, size, mean, std, seed):
        super().__init__()
        self.size = int(size)
        if self.size <= 0 or self.size % 16:
            raise ValueError(f'frame size {size}: the kernel emits squares whose side is a multiple of 16')
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self.generator = torch.Generator()
        self.generator.manual_seed(int(seed))
        self.last_rows = None          # int32 [B, 9] on the host: the rows of the last call

    def seed(self, seed):
        self.generator.manual_seed(int(seed))
        return self

    def draw(self, B, H, W):
        raise NotImplementedError

    def forward(self, frames):
        if not frames.is_cuda:
            raise RuntimeError('the frame front-end runs on an MI355X (cuda) device; there is no CPU fallback')
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError('the frame front-end takes uint8 frames [B, H, W, 3]')
        B, H, W, _ = frames.shape
        rows = self.draw(B, H, W)
        check_rows(rows, H, W, self.size)
        self.last_rows = torch.tensor(rows, dtype=torch.int32)
        params = self.last_rows.to(frames.device, non_blocking=True)
        return ops.frame_transform(frames.contiguous(), params, self.size, self.mean, self.std)


class TrainFrameTransform(_FrameTransform):
    """RandomResizedCrop(size, scale, ratio) -> RandomHorizontalFlip(p) -> ToTensor -> Normalize(mean, std) of uint8 frames
    [B, H, W, 3] on the device -> fp32 [B, 3, size, size].  One independent draw per sample from the module's own generator
    (``seed(n)`` re-seeds it); ``last_rows`` holds the rows of the last call."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), flip_p=0.5, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0):
        super().__init__(size, mean, std, seed)
        self.scale, self.ratio, self.flip_p = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1])), float(flip_p)

    def draw(self, B, H, W):
        rows = []
        for _ in range(B):
            i, j, h, w = random_resized_crop_params(H, W, self.scale, self.ratio, self.generator)
            flip = int(torch.rand(1, generator=self.generator).item() < self.flip_p)
            rows.append([i, j, h, w, self.size, self.size, 0, 0, flip])
        return rows


class EvalFrameTransform(_FrameTransform):
    """Resize(int(size / crop_pct)) -> CenterCrop(size) -> ToTensor -> Normalize(mean, std) of uint8 frames [B, H, W, 3] on the
    device -> fp32 [B, 3, size, size] (no randomness: the generator is unused)."""

    def __init__(self, size, crop_pct=0.875, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        super().__init__(size, mean, std, 0)
        self.crop_pct = float(crop_pct)

    def draw(self, B, H, W):
        (RH, RW), (top, left) = resize_center_crop_params(H, W, self.size, self.crop_pct)
        return [[0, 0, H, W, RH, RW, top, left, 0] for _ in range(B)]
