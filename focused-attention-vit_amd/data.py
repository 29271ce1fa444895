"""Device-side input pipeline: the reference's torchvision transform stacks
(utils/data_utils.py:21-81, ``get_transforms``) executed on the GPU on raw uint8 batches, plus an asynchronous
host->device loader.  The reference decodes and resizes every image with PIL inside DataLoader worker processes
and then blocks on ``images.to(device)`` (experiments/mhla_pretrained.py:357-358); here the host only hands over
uint8 HWC bytes (pinned memory, a copy stream, double buffering) and ONE kernel pair does crop / flip /
Pillow-exact bilinear resize / ToTensor / Normalize (csrc/image.hip) while the previous step computes.

Random parameters (crop origin, flip, RandomResizedCrop box) follow torchvision's distributions but are drawn
from a numpy generator owned by the transform: torch's global RNG stream order inside torchvision is not
reproduced (random augmentation has no parity target).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Iterable, Iterator, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from . import kernels as K
from . import streams

# CUs the loader's segmentation stream may occupy (of 256; read once).  Measured at the cfg3 batch (bench.py --config
# cfg3 --slic --slic-cus N): see DESIGN.md, round 4.
SEGMENTER_CUS = int(os.environ.get("FAVIT_SEGMENTER_CUS", "128"))

CIFAR10_MEAN, CIFAR10_STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _resized_size(h: int, w: int, size: int) -> Tuple[int, int]:
    """torchvision Resize(int): the smaller edge becomes `size`, the other int(size * long / short)."""
    if h <= w:
        return size, int(size * w / h)
    return int(size * h / w), size


# ---- checkpoint form of a numpy RandomState (plain containers and one tensor), shared by every drawing stage ----
def _rng_state(rng: np.random.RandomState) -> Dict:
    name, keys, pos, has_gauss, cached = rng.get_state()
    return {"bit_generator": str(name), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
            "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}


def _check_rng_state(who: str, state: Dict) -> None:
    for k in ("bit_generator", "keys", "pos", "has_gauss", "cached_gaussian"):
        if k not in state:
            raise ValueError(f"{who} state: entry '{k}' is missing")
    if state["bit_generator"] != "MT19937" or tuple(state["keys"].shape) != (624,):
        raise ValueError(f"{who} state: 'keys' is not the 624-word state of an MT19937 generator")


def _set_rng_state(rng: np.random.RandomState, state: Dict) -> None:
    rng.set_state(("MT19937", state["keys"].numpy().astype(np.uint32), int(state["pos"]), int(state["has_gauss"]),
                   float(state["cached_gaussian"])))


class RaggedBatch:
    """A batch of HWC uint8 images of different sizes, packed back to back (an ImageFolder batch).

    bytes   : uint8 1-D torch tensor, on the host or on the device
    offsets : int64 [B] byte offset of each image inside ``bytes``        (always HOST numpy arrays: the descriptors
    heights, widths : int32 [B]                                            are validated without touching the device)
    channels: bytes per pixel (3 for the readers of datasets.py)
    """

    def __init__(self, bytes, offsets, heights, widths, channels: int = 3):
        self.bytes = bytes if torch.is_tensor(bytes) else torch.as_tensor(np.asarray(bytes))
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.heights = np.asarray(heights, dtype=np.int32)
        self.widths = np.asarray(widths, dtype=np.int32)
        self.channels = int(channels)

    @classmethod
    def from_images(cls, images: Sequence[np.ndarray]) -> "RaggedBatch":
        """Pack a list of HWC uint8 arrays (all with the same channel count)."""
        if len(images) == 0:
            raise ValueError("RaggedBatch.from_images: empty list")
        imgs = [np.asarray(im) for im in images]
        ch = imgs[0].shape[2] if imgs[0].ndim == 3 else 0
        for i, im in enumerate(imgs):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != ch:
                raise TypeError(f"RaggedBatch.from_images: image {i} is not a uint8 [H, W, {ch}] array")
        sizes = np.array([im.size for im in imgs], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        buf = np.empty(int(sizes.sum()), dtype=np.uint8)
        for im, o, n in zip(imgs, offsets, sizes):
            buf[o:o + n] = im.reshape(-1)
        return cls(torch.from_numpy(buf), offsets, [im.shape[0] for im in imgs], [im.shape[1] for im in imgs], ch)

    def __len__(self) -> int:
        return len(self.offsets)

    @property
    def is_cuda(self) -> bool:
        return self.bytes.is_cuda

    def image(self, b: int) -> np.ndarray:
        """Image b as a HWC array (host batches)."""
        h, w, o = int(self.heights[b]), int(self.widths[b]), int(self.offsets[b])
        return self.bytes[o:o + h * w * self.channels].cpu().numpy().reshape(h, w, self.channels)

    def to(self, device, non_blocking: bool = False) -> "RaggedBatch":
        return RaggedBatch(self.bytes.to(device, non_blocking=non_blocking), self.offsets.copy(), self.heights.copy(),
                           self.widths.copy(), self.channels)

    def record_stream(self, stream) -> None:
        self.bytes.record_stream(stream)

    def descriptors(self) -> np.ndarray:
        """int64 [B,3] rows (byte offset, Hs, Ws) for favit_image_transform_ragged.  Every row is checked against the
        size of ``bytes`` here, on the host arrays: the kernel trusts them."""
        B = len(self.offsets)
        if self.bytes.dtype != torch.uint8 or self.bytes.dim() != 1:
            raise TypeError("RaggedBatch.bytes must be a 1-D uint8 tensor")
        if B == 0 or self.heights.shape != (B,) or self.widths.shape != (B,) or self.offsets.shape != (B,):
            raise ValueError("RaggedBatch: offsets, heights and widths must be non-empty [B] arrays of one length")
        if not 1 <= self.channels <= 4:
            raise ValueError(f"RaggedBatch: {self.channels} channels (1..4 supported)")
        d = np.stack([self.offsets, self.heights.astype(np.int64), self.widths.astype(np.int64)], axis=1)
        end = d[:, 0] + d[:, 1] * d[:, 2] * self.channels
        bad = (d[:, 0] < 0) | (d[:, 1] <= 0) | (d[:, 2] <= 0) | (end > self.bytes.numel())
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError(f"RaggedBatch: image {b} (offset {int(d[b, 0])}, {int(d[b, 1])}x{int(d[b, 2])}x{self.channels}) "
                             f"does not lie inside the {self.bytes.numel()}-byte buffer")
        return np.ascontiguousarray(d)


class DeviceTransform:
    """One of the reference's transform stacks, run by favit_image_transform (favit_image_transform_ragged for a
    RaggedBatch of mixed-size images).

    kind: 'cifar10_train'  RandomCrop(32, padding=4) -> RandomHorizontalFlip -> Resize(S) -> ToTensor -> Normalize
          'imagenet_train' RandomResizedCrop(S) -> RandomHorizontalFlip -> ToTensor -> Normalize
          'resize'         Resize(S) -> ToTensor -> Normalize                       (cifar10 / default test)
          'resize_flip'    Resize(S) -> RandomHorizontalFlip -> ToTensor -> Normalize   (default train)
          'imagenet_test'  Resize(int(1.14 S)) -> CenterCrop(S) -> ToTensor -> Normalize
    """

    def __init__(self, kind: str, img_size: int, mean: Sequence[float], std: Sequence[float], seed: int = 0):
        if kind not in ("cifar10_train", "imagenet_train", "resize", "resize_flip", "imagenet_test"):
            raise ValueError(f"unknown transform kind {kind!r}")
        self.kind, self.S = kind, int(img_size)
        self.mean = (C.c_float * 3)(*[float(m) for m in mean])
        self.std = (C.c_float * 3)(*[float(s) for s in std])
        self.rng = np.random.RandomState(seed)

    # ---- checkpoint state: the generator of the random crops / flips (plain containers and one tensor) ----
    def state_dict(self) -> Dict:
        return {"kind": self.kind, **_rng_state(self.rng)}

    def check_state_dict(self, state: Dict) -> None:
        _check_rng_state("DeviceTransform", state)
        if state.get("kind", self.kind) != self.kind:
            raise ValueError(f"DeviceTransform state: 'kind' is {state['kind']!r}, the transform is {self.kind!r}")

    def load_state_dict(self, state: Dict) -> None:
        self.check_state_dict(state)
        _set_rng_state(self.rng, state)

    # ---- per-image parameter rows (see include/favit.h: favit_image_transform) ----
    def params(self, B: int, H, W) -> np.ndarray:
        """H, W: the source size, scalars for a uniform batch or [B] arrays for a ragged one (every row is then drawn
        from that image's own size, image by image)."""
        if np.ndim(H) == 0 and np.ndim(W) == 0:
            p = self._rows(B, int(H), int(W))
        else:
            Hs, Ws = np.broadcast_to(np.asarray(H), (B,)), np.broadcast_to(np.asarray(W), (B,))
            p = np.zeros((B, 12), dtype=np.int32)
            for b in range(B):
                try:
                    p[b] = self._rows(1, int(Hs[b]), int(Ws[b]))[0]
                except ValueError as e:
                    raise ValueError(f"image {b} ({int(Hs[b])}x{int(Ws[b])}): {e}") from None
        self.check_params(p)
        return p

    def _rows(self, B: int, H: int, W: int) -> np.ndarray:
        S, r = self.S, self.rng
        p = np.zeros((B, 12), dtype=np.int32)
        if self.kind == "cifar10_train":
            pad, cs = 4, 32
            if H + 2 * pad < cs or W + 2 * pad < cs:
                raise ValueError("cifar10_train expects images of at least 24x24")
            p[:, 0] = r.randint(0, H + 2 * pad - cs + 1, B)
            p[:, 1] = r.randint(0, W + 2 * pad - cs + 1, B)
            p[:, 2], p[:, 3], p[:, 4] = cs, cs, pad
            p[:, 5], p[:, 6] = _resized_size(cs, cs, S)
            p[:, 9] = r.rand(B) < 0.5                      # flip BEFORE the resize (torchvision order)
        elif self.kind == "imagenet_train":
            for b in range(B):                             # RandomResizedCrop.get_params: scale (0.08, 1), ratio (3/4, 4/3)
                area = H * W
                box = None
                for _ in range(10):
                    ta = area * r.uniform(0.08, 1.0)
                    ar = math.exp(r.uniform(math.log(3.0 / 4.0), math.log(4.0 / 3.0)))
                    w, h = int(round(math.sqrt(ta * ar))), int(round(math.sqrt(ta / ar)))
                    if 0 < w <= W and 0 < h <= H:
                        box = (r.randint(0, H - h + 1), r.randint(0, W - w + 1), h, w)
                        break
                if box is None:                            # fallback: central crop with a clamped aspect ratio
                    ir = W / H
                    if ir < 3.0 / 4.0:
                        w, h = W, int(round(W / (3.0 / 4.0)))
                    elif ir > 4.0 / 3.0:
                        h, w = H, int(round(H * (4.0 / 3.0)))
                    else:
                        w, h = W, H
                    box = ((H - h) // 2, (W - w) // 2, h, w)
                p[b, 0:4] = box
            p[:, 5], p[:, 6] = S, S
            p[:, 10] = r.rand(B) < 0.5                     # flip AFTER the resize
        elif self.kind in ("resize", "resize_flip"):
            rh, rw = _resized_size(H, W, S)
            if (rh, rw) != (S, S):
                raise ValueError("Resize(S) of a non-square image gives a non-square tensor; use imagenet_test")
            p[:, 2], p[:, 3], p[:, 5], p[:, 6] = H, W, rh, rw
            if self.kind == "resize_flip":
                p[:, 10] = r.rand(B) < 0.5
        else:                                              # imagenet_test
            rh, rw = _resized_size(H, W, int(S * 1.14))
            p[:, 2], p[:, 3], p[:, 5], p[:, 6] = H, W, rh, rw
            p[:, 7], p[:, 8] = int(round((rh - S) / 2.0)), int(round((rw - S) / 2.0))
        return p

    MAX_TAPS = 64          # csrc/image.hip: filter taps per output position the resampling kernels hold

    @classmethod
    def check_params(cls, p: np.ndarray) -> None:
        """Pillow's triangle filter spans 2 * max(1, crop / resized) source pixels: beyond MAX_TAPS the kernels would
        truncate the window and silently stop being bit-identical to Pillow, so such a row is refused here (a crop box
        downscaled more than ~31x: a very large source image or crop)."""
        for ax, (c, r) in enumerate(((p[:, 2], p[:, 5]), (p[:, 3], p[:, 6]))):
            scale = np.maximum(1.0, c.astype(np.float64) / np.maximum(r, 1))
            taps = np.ceil(2.0 * scale).astype(np.int64) + 2
            if (taps > cls.MAX_TAPS).any():
                b = int(np.argmax(taps))
                raise ValueError(f"DeviceTransform: image {b} is downscaled {scale[b]:.1f}x along axis {ax} "
                                 f"({int(c[b])} -> {int(r[b])} pixels): {int(taps[b])} filter taps exceed the kernels' "
                                 f"{cls.MAX_TAPS}; resize such sources on the host first")

    def __call__(self, batch_u8, params: Optional[np.ndarray] = None, want_bytes: bool = False):
        """batch_u8: uint8 [B, H, W, C] on the GPU, or a RaggedBatch whose bytes are on the GPU
        -> fp32 [B, C, S, S] (and the resized bytes if want_bytes)."""
        if isinstance(batch_u8, RaggedBatch):
            return self._call_ragged(batch_u8, params, want_bytes)
        K.require_gpu(batch_u8)
        if batch_u8.dtype != torch.uint8 or batch_u8.dim() != 4:
            raise TypeError("DeviceTransform expects a uint8 [B, H, W, C] batch")
        batch_u8 = batch_u8.contiguous()
        B, H, W, Cc = batch_u8.shape
        if params is None:
            params = self.params(B, H, W)
        else:
            self.check_params(np.asarray(params))
        prm = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(batch_u8.device, non_blocking=True)
        ch_max = int(params[:, 2].max())
        S = self.S
        tmp = torch.empty((B, ch_max, S, Cc), dtype=torch.uint8, device=batch_u8.device)
        out = torch.empty((B, Cc, S, S), dtype=torch.float32, device=batch_u8.device)
        u8 = torch.empty((B, S, S, Cc), dtype=torch.uint8, device=batch_u8.device) if want_bytes else None
        _abi.check(_abi.lib().favit_image_transform(K._p(batch_u8), K._p(tmp), K._p(out), K._p(u8), K._p(prm), B, H, W, Cc,
                                                    ch_max, S, self.mean, self.std, K._st()), "favit_image_transform")
        return (out, u8) if want_bytes else out

    def _call_ragged(self, rb: RaggedBatch, params: Optional[np.ndarray], want_bytes: bool):
        K.require_gpu(rb.bytes)
        desc = rb.descriptors()                            # host-side bounds check, before anything is uploaded
        B, Cc, S, dev = len(rb), rb.channels, self.S, rb.bytes.device
        if params is None:
            params = self.params(B, rb.heights, rb.widths)
        else:
            params = np.asarray(params)
            if params.shape != (B, 12):
                raise ValueError(f"params must be [{B}, 12]")
            self.check_params(params)
        prm = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(dev, non_blocking=True)
        dsc = torch.from_numpy(desc).to(dev, non_blocking=True)
        ch_max = int(params[:, 2].max())
        tmp = torch.empty((B, ch_max, S, Cc), dtype=torch.uint8, device=dev)
        out = torch.empty((B, Cc, S, S), dtype=torch.float32, device=dev)
        u8 = torch.empty((B, S, S, Cc), dtype=torch.uint8, device=dev) if want_bytes else None
        _abi.check(_abi.lib().favit_image_transform_ragged(K._p(rb.bytes), K._p(dsc), K._p(tmp), K._p(out), K._p(u8), K._p(prm),
                                                           B, Cc, ch_max, S, self.mean, self.std, K._st()),
                   "favit_image_transform_ragged")
        return (out, u8) if want_bytes else out


def get_transforms(dataset_name: str, img_size: int = 224, seed: int = 0) -> Dict[str, DeviceTransform]:
    """Mirror of the reference's get_transforms (utils/data_utils.py:21-81): {'train', 'test'} device transforms."""
    name = dataset_name.lower()
    if name == "cifar10":
        return {"train": DeviceTransform("cifar10_train", img_size, CIFAR10_MEAN, CIFAR10_STD, seed),
                "test": DeviceTransform("resize", img_size, CIFAR10_MEAN, CIFAR10_STD, seed)}
    if name == "imagenet":
        return {"train": DeviceTransform("imagenet_train", img_size, IMAGENET_MEAN, IMAGENET_STD, seed),
                "test": DeviceTransform("imagenet_test", img_size, IMAGENET_MEAN, IMAGENET_STD, seed)}
    half = (0.5, 0.5, 0.5)
    return {"train": DeviceTransform("resize_flip", img_size, half, half, seed),
            "test": DeviceTransform("resize", img_size, half, half, seed)}


class MixedLabels(NamedTuple):
    """The labels of a batch mixed by BatchMix: row b's target is lam[b] * onehot(labels[b]) + (1 - lam[b]) *
    onehot(labels[B-1-b]) (train.cross_entropy(..., mix_lam=lam)).  labels: int64 [B], lam: fp32 [B], on the device."""
    labels: torch.Tensor
    lam: torch.Tensor


class BatchMix:
    """Mixup / CutMix of a device batch with its own flip (timm's Mixup): row b is paired with row B-1-b, the images
    are mixed in place by one kernel (favit_batch_mix) and the labels become MixedLabels.

    Per draw -- one for the whole batch (mode 'batch') or one per row ('elem'):
      with probability `prob` the row is mixed, otherwise left alone (lam = 1);
      CutMix is chosen with probability `switch_prob` when both alphas are > 0, else whichever alpha is > 0 is used;
      lam ~ Beta(alpha, alpha);  CutMix: r = sqrt(1 - lam), a box of int(S r) x int(S r) pixels around a uniform centre,
      clipped to the image, and lam = 1 - box_area / S^2 (an empty box leaves the row alone).
    The middle row of an odd batch is its own partner and is always left alone.  The draws come from a numpy generator
    owned by the object (as DeviceTransform's do) and are part of the checkpoint state."""

    def __init__(self, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch", seed: int = 0):
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0):
            raise ValueError(f"BatchMix: alphas must be >= 0, got {mixup_alpha}, {cutmix_alpha}")
        if mixup_alpha == 0.0 and cutmix_alpha == 0.0:
            raise ValueError("BatchMix: mixup_alpha and cutmix_alpha are both 0 (nothing to mix)")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"BatchMix: prob and switch_prob must be in [0, 1], got {prob}, {switch_prob}")
        if mode not in ("batch", "elem"):
            raise ValueError(f"BatchMix: unknown mode {mode!r} ('batch' or 'elem')")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.rng = np.random.RandomState(seed)

    # ---- checkpoint state: the generator of the draws (the form of DeviceTransform's) ----
    def state_dict(self) -> Dict:
        return {"mode": self.mode, **_rng_state(self.rng)}

    def check_state_dict(self, state: Dict) -> None:
        _check_rng_state("BatchMix", state)
        if state.get("mode", self.mode) != self.mode:
            raise ValueError(f"BatchMix state: 'mode' is {state['mode']!r}, the mix is {self.mode!r}")

    def load_state_dict(self, state: Dict) -> None:
        self.check_state_dict(state)
        _set_rng_state(self.rng, state)

    def _draw(self, S: int):
        """One draw: (lam, (y0, y1, x0, x1)); lam = 1 and a zero box mean 'leave the row alone'."""
        rng = self.rng
        if not rng.rand() < self.prob:
            return 1.0, (0, 0, 0, 0)
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = bool(rng.rand() < self.switch_prob)
        else:
            cut = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(rng.beta(alpha, alpha))
        if not cut:
            return lam, (0, 0, 0, 0)
        r = math.sqrt(1.0 - lam)
        ch, cw = int(S * r), int(S * r)
        cy, cx = int(rng.randint(S)), int(rng.randint(S))
        y0, y1 = min(max(cy - ch // 2, 0), S), min(max(cy + ch // 2, 0), S)
        x0, x1 = min(max(cx - cw // 2, 0), S), min(max(cx + cw // 2, 0), S)
        area = (y1 - y0) * (x1 - x0)
        if area == 0:
            return 1.0, (0, 0, 0, 0)
        return 1.0 - area / float(S * S), (y0, y1, x0, x1)

    def params(self, B: int, S: int) -> Tuple[np.ndarray, np.ndarray]:
        """Host parameters of one batch of B images of S x S pixels: (lam [B] fp32, box [B, 4] int32 = y0, y1, x0, x1)."""
        B, S = int(B), int(S)
        if B < 1 or S < 1:
            raise ValueError(f"BatchMix.params: B and S must be positive, got {B}, {S}")
        lam = np.ones(B, dtype=np.float32)
        box = np.zeros((B, 4), dtype=np.int32)
        if self.mode == "batch":
            lam[:], box[:] = self._draw(S)
        else:
            for b in range(B):
                lam[b], box[b] = self._draw(S)
        if B % 2:
            lam[B // 2], box[B // 2] = 1.0, 0
        return lam, box

    @staticmethod
    def check_params(lam: np.ndarray, box: np.ndarray, B: int) -> None:
        if lam.shape != (B,) or box.shape != (B, 4):
            raise ValueError(f"BatchMix: params must be (lam [{B}], box [{B}, 4])")
        if not (np.all(lam >= 0.0) and np.all(lam <= 1.0)):
            raise ValueError("BatchMix: every lam must lie in [0, 1]")

    def __call__(self, images: torch.Tensor, labels: torch.Tensor, params=None):
        """images: fp32 [B, C, S, S] on the GPU, mixed IN PLACE; labels: int64 [B].  params: (lam, box) as params()
        returns them, instead of a fresh draw.  Returns (images, MixedLabels(labels, lam on the device))."""
        K.require_gpu(images, labels)
        if images.dim() != 4 or images.shape[2] != images.shape[3]:
            raise TypeError("BatchMix expects a [B, C, S, S] batch of square images")
        B, S = images.shape[0], images.shape[3]
        if tuple(labels.shape) != (B,):
            raise TypeError(f"BatchMix: labels must be [{B}]")
        lam, box = self.params(B, S) if params is None else params
        lam = np.ascontiguousarray(lam, dtype=np.float32)
        box = np.ascontiguousarray(box, dtype=np.int32)
        self.check_params(lam, box, B)
        d_lam = torch.from_numpy(lam).to(images.device, non_blocking=True)
        d_box = torch.from_numpy(box).to(images.device, non_blocking=True)
        K.batch_mix(images, d_lam, d_box)
        return images, MixedLabels(labels, d_lam)


class RandAugment:
    """torchvision's RandAugment(num_ops, magnitude, num_magnitude_bins) on the device (favit_randaugment): per image
    num_ops ops drawn uniformly from `ops` (default: all of OPS), each at the magnitude bin `magnitude`, applied to
    the resized bytes of the transform in ONE launch; the augmented bytes are bit-identical to what Pillow gives
    for the same ops (torchvision's PIL path, NEAREST interpolation, `fill` outside the image).

    Per image, then per slot, the generator owned by the object draws op = randint(len(ops)) and sign = randint(2)
    (always drawn; only the signed ops -- shears, translations, Rotate and the four enhancements -- use it).
    Everything Pillow computes in Python doubles (matrices, fixed-point conversion, masks, thresholds, factors) is
    computed here and travels in the op table (include/favit.h); the device runs what Pillow runs in C."""

    OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
           "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
    SIGNED = frozenset(OPS[1:10])
    MAX_OPS = _abi.RANDAUGMENT_MAX_OPS
    # kernel op ids (include/favit.h)
    K_IDENTITY, K_AFFINE, K_BLEND, K_MASK = _abi.AUG_IDENTITY, _abi.AUG_AFFINE, _abi.AUG_BLEND, _abi.AUG_MASK
    K_SOLARIZE, K_AUTOCONTRAST, K_EQUALIZE = _abi.AUG_SOLARIZE, _abi.AUG_AUTOCONTRAST, _abi.AUG_EQUALIZE
    _BLEND_KIND = {"Brightness": 0, "Color": 1, "Contrast": 2, "Sharpness": 3}

    def __init__(self, num_ops: int = 2, magnitude: int = 9, num_magnitude_bins: int = 31,
                 fill: Sequence[int] = (0, 0, 0), ops: Optional[Sequence[str]] = None, seed: int = 0):
        if not 0 <= int(num_ops) <= self.MAX_OPS:
            raise ValueError(f"RandAugment: num_ops must be in 0..{self.MAX_OPS}, got {num_ops}")
        if int(num_magnitude_bins) < 2 or not 0 <= int(magnitude) < int(num_magnitude_bins):
            raise ValueError(f"RandAugment: magnitude {magnitude} is not a bin of {num_magnitude_bins} (at least 2) bins")
        ops = tuple(self.OPS if ops is None else ops)
        for name in ops:
            if name not in self.OPS:
                raise ValueError(f"RandAugment: unknown op {name!r} (one of {', '.join(self.OPS)})")
        if not ops:
            raise ValueError("RandAugment: empty op list")
        fill = tuple(int(v) for v in ((fill,) * 3 if np.ndim(fill) == 0 else fill))
        if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
            raise ValueError(f"RandAugment: fill must be three bytes, got {fill}")
        self.num_ops, self.magnitude, self.bins = int(num_ops), int(magnitude), int(num_magnitude_bins)
        self.fill, self.ops = fill, ops
        self.rng = np.random.RandomState(seed)

    # ---- checkpoint state: the generator of the draws (the form of DeviceTransform's) ----
    def state_dict(self) -> Dict:
        state = _rng_state(self.rng)
        state.update(num_ops=self.num_ops, ops=list(self.ops))
        return state

    def check_state_dict(self, state: Dict) -> None:
        _check_rng_state("RandAugment", state)
        if state.get("num_ops", self.num_ops) != self.num_ops or tuple(state.get("ops", self.ops)) != self.ops:
            raise ValueError("RandAugment state: it was saved with another num_ops / op list, so the generator would "
                             "not continue the same stream of draws")

    def load_state_dict(self, state: Dict) -> None:
        self.check_state_dict(state)
        _set_rng_state(self.rng, state)

    # ---- the op table ----
    def magnitude_value(self, name: str, S: int, sign: int = 0, bin_: Optional[int] = None):
        """The magnitude torchvision gives op `name` at the object's bin (or `bin_`) for S x S images; None for the
        ops without one.  Signed ops are negated when sign == 1."""
        k, bins = self.magnitude if bin_ is None else int(bin_), self.bins
        if name in ("Identity", "AutoContrast", "Equalize"):
            return None
        if name == "Posterize":
            return int((8 - np.round(np.arange(bins) / ((bins - 1) / 4)))[k])
        if name == "Solarize":
            return float(np.linspace(255.0, 0.0, bins)[k])
        top = {"ShearX": 0.3, "ShearY": 0.3, "TranslateX": 150.0 / 331.0 * S, "TranslateY": 150.0 / 331.0 * S,
               "Rotate": 30.0}.get(name, 0.9)
        m = float(np.linspace(0.0, top, bins)[k])
        return -m if sign else m

    @staticmethod
    def _affine_row(mt: Sequence[float], fill: Sequence[int]) -> list:
        """Pillow's affine_fixed set-up: FIX(v) = floor(v * 65536 + 0.5), the half-pixel centre folded into a2, a5."""
        a0, a1, a2, a3, a4, a5 = (float(v) for v in mt)
        fix = lambda v: int(math.floor(v * 65536.0 + 0.5))      # noqa: E731
        return [RandAugment.K_AFFINE, fix(a0), fix(a1), fix(a2 + a0 * 0.5 + a1 * 0.5), fix(a3), fix(a4),
                fix(a5 + a3 * 0.5 + a4 * 0.5), fill[0] | fill[1] << 8 | fill[2] << 16]

    def row(self, name: str, m, S: int) -> np.ndarray:
        """The int32 [8] table row of op `name` with magnitude value m on S x S images."""
        r = [self.K_IDENTITY] + [0] * 7
        if name == "ShearX":
            r = self._affine_row((1, m, 0, 0, 1, 0), self.fill)
        elif name == "ShearY":
            r = self._affine_row((1, 0, 0, m, 1, 0), self.fill)
        elif name == "TranslateX":
            r = self._affine_row((1, 0, -int(m), 0, 1, 0), self.fill)
        elif name == "TranslateY":
            r = self._affine_row((1, 0, 0, 0, 1, -int(m)), self.fill)
        elif name == "Rotate":
            # PIL.Image.rotate about the image centre, with its round(..., 15)
            ang = -math.radians(m % 360.0)
            mt = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0,
                  round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
            cx = cy = S / 2.0
            mt[2] = mt[0] * -cx + mt[1] * -cy + mt[2]
            mt[5] = mt[3] * -cx + mt[4] * -cy + mt[5]
            mt[2] += cx
            mt[5] += cy
            r = self._affine_row(mt, self.fill)
        elif name in self._BLEND_KIND:
            f = np.float32(1 + m)                               # ImageEnhance passes the factor to C as a float
            r = [self.K_BLEND, self._BLEND_KIND[name], int(f.view(np.int32))] + [0] * 5
        elif name == "Posterize":
            r = [self.K_MASK, ~(2 ** (8 - int(m)) - 1) & 0xFF] + [0] * 6
        elif name == "Solarize":
            r = [self.K_SOLARIZE, int(math.ceil(m))] + [0] * 6  # integer v < m  <=>  v < ceil(m)
        elif name == "AutoContrast":
            r = [self.K_AUTOCONTRAST] + [0] * 7
        elif name == "Equalize":
            r = [self.K_EQUALIZE] + [0] * 7
        elif name != "Identity":
            raise ValueError(f"RandAugment: unknown op {name!r}")
        return np.array(r, dtype=np.int64).astype(np.int32)

    def draw(self, B: int) -> np.ndarray:
        """The draws of one batch: int [B, num_ops, 2] = (index into self.ops, sign)."""
        d = np.zeros((B, self.num_ops, 2), dtype=np.int64)
        for b in range(B):
            for s in range(self.num_ops):
                d[b, s, 0] = self.rng.randint(len(self.ops))
                d[b, s, 1] = self.rng.randint(2)
        return d

    def table(self, draws: np.ndarray, S: int) -> np.ndarray:
        """int32 [B, num_ops, 8] op table of explicit draws."""
        B, n = draws.shape[0], draws.shape[1]
        cache: Dict = {}
        t = np.zeros((B, n, 8), dtype=np.int32)
        for b in range(B):
            for s in range(n):
                key = (int(draws[b, s, 0]), int(draws[b, s, 1]))
                if key not in cache:
                    name = self.ops[key[0]]
                    cache[key] = self.row(name, self.magnitude_value(name, S, key[1] if name in self.SIGNED else 0), S)
                t[b, s] = cache[key]
        return t

    def params(self, B: int, S: int) -> np.ndarray:
        """A fresh draw for B images of S x S pixels -> the int32 [B, num_ops, 8] op table."""
        B, S = int(B), int(S)
        if B < 1 or S < 1:
            raise ValueError(f"RandAugment.params: B and S must be positive, got {B}, {S}")
        t = self.table(self.draw(B), S)
        self.check_params(t, B)
        return t

    @classmethod
    def check_params(cls, t: np.ndarray, B: int) -> None:
        """Refuses a malformed table on the host, before the upload (the kernel would run an unknown op as identity
        and a non-finite factor as garbage, silently)."""
        t = np.asarray(t)
        if t.ndim != 3 or t.shape[0] != B or t.shape[2] != 8 or t.dtype != np.int32:
            raise ValueError(f"RandAugment: the op table must be int32 [{B}, num_ops, 8]")
        if t.shape[1] > cls.MAX_OPS:
            raise ValueError(f"RandAugment: {t.shape[1]} ops per image exceed the kernel's {cls.MAX_OPS}")
        op = t[:, :, 0]
        if ((op < 0) | (op > cls.K_EQUALIZE)).any():
            raise ValueError(f"RandAugment: unknown op id {int(op[(op < 0) | (op > cls.K_EQUALIZE)][0])} in the op table")
        bl = op == cls.K_BLEND
        if bl.any():
            if ((t[:, :, 1][bl] < 0) | (t[:, :, 1][bl] > 3)).any():
                raise ValueError("RandAugment: a blend row names an unknown degenerate image")
            if not np.isfinite(np.ascontiguousarray(t[:, :, 2][bl]).view(np.float32)).all():
                raise ValueError("RandAugment: a blend row carries a non-finite factor")
        lv = (op == cls.K_MASK) | (op == cls.K_SOLARIZE)
        if lv.any() and ((t[:, :, 1][lv] < 0) | (t[:, :, 1][lv] > 256)).any():
            raise ValueError("RandAugment: a Posterize mask / Solarize threshold lies outside 0..256")

    def __call__(self, u8: torch.Tensor, mean, std, params: Optional[np.ndarray] = None, erase_box=None,
                 erase_value=0.0, erase_seed: int = 0, want_bytes: bool = False):
        """u8: uint8 [B,S,S,3] on the GPU (the transform's resized bytes) -> fp32 [B,3,S,S], normalized with the
        transform's mean / std; erase_box (int32 [B,4] on the device) is filled in the same write."""
        K.require_gpu(u8)
        if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[1] != u8.shape[2] or u8.shape[3] != 3:
            raise TypeError("RandAugment expects the uint8 [B, S, S, 3] bytes of a DeviceTransform (RGB images)")
        B, S = u8.shape[0], u8.shape[1]
        if params is None:
            params = self.params(B, S)
        else:
            params = np.ascontiguousarray(params)
            self.check_params(params, B)
        if params.shape[1] == 0:                                # no ops: one identity slot keeps the table non-empty
            params = np.zeros((B, 1, 8), dtype=np.int32)
        ops = torch.from_numpy(params).to(u8.device, non_blocking=True)
        return K.randaugment(u8.contiguous(), ops, mean, std, erase_box, erase_value, erase_seed, want_bytes)


class RandomErasing:
    """torchvision's RandomErasing(p, scale, ratio, value) on the device: per image, with probability p, up to 10
    attempts at a box of area * uniform(scale) pixels and log-uniform aspect ratio (h = round(sqrt(a r)), w =
    round(sqrt(a / r)), accepted when h < H and w < W, origin by randint); an image without an accepted box is left
    alone.  value: a number, one per channel, or "normal" (one standard-normal value per element from the library's
    counter-based generator under a per-batch seed the object draws).  Applied after Normalize: by favit_randaugment's
    final write when a RandAugment runs, else by favit_random_erase in place."""

    def __init__(self, p: float = 0.25, scale: Sequence[float] = (0.02, 0.33), ratio: Sequence[float] = (0.3, 3.3),
                 value=0, seed: int = 0):
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"RandomErasing: p must be in [0, 1], got {p}")
        if len(scale) != 2 or len(ratio) != 2 or not 0.0 <= scale[0] <= scale[1] <= 1.0 or not 0.0 < ratio[0] <= ratio[1]:
            raise ValueError(f"RandomErasing: bad scale {scale} / ratio {ratio}")
        K._erase_fill(value, 3)                                 # refuses a malformed value now
        self.p, self.scale, self.ratio = float(p), (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.value = value if isinstance(value, str) or np.ndim(value) == 0 else tuple(float(v) for v in value)
        self.rng = np.random.RandomState(seed)

    def state_dict(self) -> Dict:
        return _rng_state(self.rng)

    def check_state_dict(self, state: Dict) -> None:
        _check_rng_state("RandomErasing", state)

    def load_state_dict(self, state: Dict) -> None:
        self.check_state_dict(state)
        _set_rng_state(self.rng, state)

    def params(self, B: int, H: int, W: int) -> Tuple[np.ndarray, int]:
        """(box int32 [B,4] = y0, y1, x0, x1 with an empty box meaning no erase, seed of the normal fill)."""
        B, H, W = int(B), int(H), int(W)
        if B < 1 or H < 1 or W < 1:
            raise ValueError(f"RandomErasing.params: B, H and W must be positive, got {B}, {H}, {W}")
        rng, area = self.rng, H * W
        lr = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        box = np.zeros((B, 4), dtype=np.int32)
        for b in range(B):
            if not rng.rand() < self.p:
                continue
            for _ in range(10):
                a = area * rng.uniform(self.scale[0], self.scale[1])
                r = math.exp(rng.uniform(lr[0], lr[1]))
                h, w = int(round(math.sqrt(a * r))), int(round(math.sqrt(a / r)))
                if not (h < H and w < W):
                    continue
                i, j = int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1))
                box[b] = (i, i + h, j, j + w)
                break
        seed = int(rng.randint(0, 2 ** 31 - 1)) << 31 | int(rng.randint(0, 2 ** 31 - 1))
        self.check_params(box, B, H, W)
        return box, seed

    @staticmethod
    def check_params(box: np.ndarray, B: int, H: int, W: int) -> None:
        if box.shape != (B, 4) or box.dtype != np.int32:
            raise ValueError(f"RandomErasing: the box table must be int32 [{B}, 4]")
        if ((box[:, 0] < 0) | (box[:, 1] > H) | (box[:, 2] < 0) | (box[:, 3] > W)).any():
            raise ValueError("RandomErasing: a box reaches outside the image")

    def __call__(self, images: torch.Tensor, params=None) -> torch.Tensor:
        """images: fp32 [B,C,H,W] on the GPU, erased IN PLACE (the stand-alone form)."""
        K.require_gpu(images)
        if images.dim() != 4:
            raise TypeError("RandomErasing expects a [B, C, H, W] batch")
        B, _, H, W = images.shape
        box, seed = self.params(B, H, W) if params is None else params
        box = np.ascontiguousarray(box, dtype=np.int32)
        self.check_params(box, B, H, W)
        d_box = torch.from_numpy(box).to(images.device, non_blocking=True)
        return K.random_erase(images, d_box, self.value, seed)


class DeviceLoader:
    """Iterates (images fp32 [B,C,S,S], labels int64 [B]) on the GPU from an iterable of HOST batches
    (uint8 [B,H,W,C] array / tensor, or a RaggedBatch of mixed-size images; integer labels).  Batch k+1 is copied (pinned staging buffers, a dedicated
    copy stream) and transformed while the consumer computes on batch k: no host-side blocking .to(device)."""

    mix = augment = erase = None          # the optional stages (class defaults: off)

    def __init__(self, host_batches: Iterable, transform: DeviceTransform, device: Optional[torch.device] = None,
                 segmenter=None, mix: Optional[BatchMix] = None, augment: Optional[RandAugment] = None,
                 erase: Optional[RandomErasing] = None):
        """augment (optional): a RandAugment, applied to the resized bytes of the transform before ToTensor / Normalize;
        erase (optional): a RandomErasing, applied after Normalize (inside the augment's launch when there is one).
        The order is transform -> RandAugment -> Normalize -> erase -> mix -> segmenter, on both staging paths and for
        uniform and ragged batches; the state carries their generators under "augment" / "erase".  Without them the
        loader issues exactly the launches it issues without these options.

        mix (optional): a BatchMix, applied to every batch directly after the transform (with a segmenter: before
        the segmentation, which therefore sees the image the model sees).  The loader then yields
        (images, MixedLabels(labels, lam)) and its state carries the mix's generator under "mix".

        segmenter (optional): a models.sppp.SuperpixelSegmentation (``model.segmentation`` of the SPPP models).  The
        label maps of batch k+1 are then computed by the device SLIC on the loader's preparation stream while the
        consumer trains on batch k, and installed (``set_label_maps``) when the batch is yielded -- the reference
        segments inside forward (models/sppp_mhla.py:278), on the critical path of every step.

        The preparation stream is confined to ``SEGMENTER_CUS`` compute units; such a stream is a BLOCKING stream (the HIP
        call has no flag), i.e. it synchronises with the default (null) stream in both directions.  A consumer that
        wants the overlap therefore runs its step under ``with torch.cuda.stream(loader.compute_stream):`` (a stream
        of torch's non-blocking pool; cfg3 batch: 3.38 ms per step + segmentation against 4.07 ms back to back); on
        the default stream the results are the same and the two simply run one after the other."""
        self.src, self.tf = host_batches, transform
        self.dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.segmenter, self.mix = segmenter, mix
        self.augment, self.erase = augment, erase
        # the segmentation stream is confined to SEGMENTER_CUS compute units (streams.py): its grids would otherwise
        # fill every CU and the consumer's short launches would queue behind them
        self.prep_stream = streams.cu_masked_stream(SEGMENTER_CUS, self.dev) if segmenter is not None else None
        self.compute_stream = torch.cuda.Stream(device=self.dev) if segmenter is not None else None
        self._pin = [None, None]
        self._pin_ragged = [None, None]     # [bytes (capacity of the largest batch seen), labels, copy-done event] per slot

    def __len__(self):
        return len(self.src)

    # ---- checkpoint state, between epochs: the transform's generator and the source's shuffle epoch ----
    def state_dict(self) -> Dict:
        state = {"transform": self.tf.state_dict(),
                 "batches": self.src.state_dict() if hasattr(self.src, "state_dict") else None}
        for key, part in self._optional_parts():
            if part is not None:
                state[key] = part.state_dict()
        return state

    def _optional_parts(self):
        return (("mix", self.mix), ("augment", self.augment), ("erase", self.erase))

    def check_state_dict(self, state: Dict) -> None:
        for k in ("transform", "batches"):
            if k not in state:
                raise ValueError(f"DeviceLoader state: entry '{k}' is missing")
        names = {"mix": "a batch mix", "augment": "a RandAugment", "erase": "a RandomErasing"}
        for key, part in self._optional_parts():
            if (key in state) != (part is not None):
                raise ValueError("DeviceLoader state: it was saved " + ("with " if key in state else "without ") +
                                 names[key] + " and this loader is built " + ("without" if key in state else "with") +
                                 " one")
        self.tf.check_state_dict(state["transform"])
        for key, part in self._optional_parts():
            if part is not None:
                part.check_state_dict(state[key])
        if state["batches"] is not None and hasattr(self.src, "check_state_dict"):
            self.src.check_state_dict(state["batches"])

    def load_state_dict(self, state: Dict) -> None:
        self.check_state_dict(state)
        self.tf.load_state_dict(state["transform"])
        for key, part in self._optional_parts():
            if part is not None:
                part.load_state_dict(state[key])
        if state["batches"] is not None and hasattr(self.src, "load_state_dict"):
            self.src.load_state_dict(state["batches"])

    def _stage_ragged_host(self, slot: int, rb: RaggedBatch, labels: torch.Tensor):
        """Pinned views holding a ragged host batch.  The staging buffers only ever grow (to the largest batch seen), and
        a buffer is rewritten only after the copy that last read it has finished."""
        n, B = rb.bytes.numel(), labels.numel()
        buf = self._pin_ragged[slot]
        if buf is not None and buf[2] is not None:
            buf[2].synchronize()
        if buf is None or buf[0].numel() < n or buf[1].numel() < B:
            buf = [torch.empty(max(n, buf[0].numel() if buf else 0), dtype=torch.uint8).pin_memory(),
                   torch.empty(max(B, buf[1].numel() if buf else 0), dtype=torch.int64).pin_memory(), None]
            self._pin_ragged[slot] = buf
        buf[0][:n].copy_(rb.bytes)
        buf[1][:B].copy_(labels)
        return RaggedBatch(buf[0][:n], rb.offsets, rb.heights, rb.widths, rb.channels), buf[1][:B]

    def _prepare(self, d_img, d_lab):
        """transform -> RandAugment -> Normalize -> erase -> mix of one device batch, on the current stream."""
        if self.augment is not None:
            _, u8 = self.tf(d_img, want_bytes=True)
            box, value, seed = None, 0.0, 0
            if self.erase is not None:
                S = u8.shape[1]
                hbox, seed = self.erase.params(u8.shape[0], S, S)
                box, value = torch.from_numpy(hbox).to(u8.device, non_blocking=True), self.erase.value
            x = self.augment(u8, self.tf.mean, self.tf.std, erase_box=box, erase_value=value, erase_seed=seed)
        else:
            x = self.tf(d_img)
            if self.erase is not None:
                x = self.erase(x)
        if self.mix is not None:
            return self.mix(x, d_lab)
        return x, d_lab

    def _stage(self, slot: int, imgs, labels):
        ragged = isinstance(imgs, RaggedBatch)
        if not ragged:
            imgs = torch.as_tensor(np.asarray(imgs)) if not torch.is_tensor(imgs) else imgs
        labels = torch.as_tensor(np.asarray(labels), dtype=torch.int64) if not torch.is_tensor(labels) else labels.to(torch.int64)
        if ragged and len(imgs) != labels.numel():
            raise ValueError(f"RaggedBatch of {len(imgs)} images with {labels.numel()} labels")
        if (imgs.bytes if ragged else imgs).is_pinned() and labels.is_pinned():
            # The producer already wrote into page-locked memory: no staging copy.  CONTRACT: the asynchronous
            # host-to-device copy reads that memory until the batch has been yielded, so the producer must not
            # rewrite a pinned buffer before the loader has yielded the batch made from it (hand out a fresh or a
            # rotated buffer per batch; bench.py --host-input rotates four).
            src = (imgs, labels)
        elif ragged:
            src = self._stage_ragged_host(slot, imgs, labels)
        else:
            buf = self._pin[slot]
            if buf is None or buf[0].shape != imgs.shape or buf[1].shape != labels.shape:
                buf = [torch.empty(imgs.shape, dtype=torch.uint8).pin_memory(), torch.empty(labels.shape, dtype=torch.int64).pin_memory(), None]
                self._pin[slot] = buf
            if buf[2] is not None:
                buf[2].synchronize()                      # the previous copy out of this staging buffer has finished
            buf[0].copy_(imgs)
            buf[1].copy_(labels)
            src = (buf[0], buf[1])
        with torch.cuda.stream(self.copy_stream):
            d_img = src[0].to(self.dev, non_blocking=True)
            d_lab = src[1].to(self.dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        if src[0] is not imgs:
            (self._pin_ragged if ragged else self._pin)[slot][2] = ev
        if self.segmenter is not None:
            # transform + SLIC of this (next) batch now, on a stream of their own, under the consumer's current step
            with torch.cuda.stream(self.prep_stream):
                self.prep_stream.wait_event(ev)
                x, d_lab = self._prepare(d_img, d_lab)
                maps = self.segmenter.segment_device(x)
                derived = self.segmenter.derive_for(maps)        # patch mapping + centroids: functions of the maps alone
                d_img.record_stream(self.prep_stream)
                ev2 = torch.cuda.Event()
                ev2.record(self.prep_stream)
            return (x, maps, derived), d_lab, ev2
        return d_img, d_lab, ev

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        it = iter(self.src)
        nxt = None
        slot = 0
        try:
            first = next(it)
        except StopIteration:
            return
        nxt = self._stage(slot, *first)
        for batch in it:
            cur, slot = nxt, slot ^ 1
            nxt = self._stage(slot, *batch)               # H2D of batch k+1 overlaps the consumer's work on batch k
            yield self._finish(cur)
        yield self._finish(nxt)

    def _finish(self, staged):
        d_img, d_lab, ev = staged
        cs = torch.cuda.current_stream(self.dev)
        cs.wait_event(ev)                                 # device-side wait, the host does not block
        for t_ in (d_lab if isinstance(d_lab, MixedLabels) else (d_lab,)):
            t_.record_stream(cs)
        if self.segmenter is not None:
            x, maps, derived = d_img
            x.record_stream(cs)
            maps.record_stream(cs)
            for tens in derived.values():
                for t_ in tens:
                    t_.record_stream(cs)
            # the model's next segment() call returns them; a captured step reads the installed tensors in place
            if getattr(self.segmenter, "_captured", False) and self.segmenter._maps is not None:
                self.segmenter.update_label_maps(maps, derived)
            else:
                self.segmenter.set_label_maps(maps, derived)
            return x, d_lab
        d_img.record_stream(cs)
        return self._prepare(d_img, d_lab)
