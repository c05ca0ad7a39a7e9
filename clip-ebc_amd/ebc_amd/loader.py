"""Training batches from stored uint8 images: `RawCropLoader`.

What the reference's train `DataLoader` yields (`Crowd.__getitem__` + `collate_fn`, datasets/crowd.py:134-175,
datasets/utils.py:31-47, in the order of its `DistributedSampler`, utils/data_utils.py) and what
`ebc_amd.train.train` unpacks: `(image [B*num_crops, 3, S, S]` normalised f32 on the device, the per-crop point
tensors, `target_density [B*num_crops, 1, S, S])`.  The images stay what they are stored as -- uint8 [H, W, 3] (a
decoded JPEG) or [3, H, W] (the reference's .npy files) -- and `CropAugment` cuts the crops straight from those bytes
(`ebc_augment_crops_raw`):
  * resident=True: the split is copied to the device once, as bytes, and every batch reads its windows in place; a
    step uploads descriptors, points and offsets only;
  * resident=False: the images stay on the CPU and a batch uploads its crop windows, packed into one pinned buffer
    (`pack_crop_windows`); with prefetch=True batch k+1 is drawn and packed into the other of two pinned buffers and
    copied on a side stream before batch k is handed out, so the copy runs beside batch k's training step.
No threads, no worker processes, no file I/O: decoding and reading the dataset stay with the caller.

The random draws are `CropAugment.plan_crop`'s, from torch's global CPU generator, batch after batch in the sampler's
order, with or without prefetch: the four modes give the same batches under one `torch.manual_seed`, and they are the
batches of `CropAugment.__call__` on `u8.float() / 255` of the same images.  (With prefetch the draws of batch k+1 come
before the caller's step k, so a caller that draws from the same generator inside its step sees another interleaving.)
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
from torch import Tensor

from ._raw import _raw_image
from .transforms import CropAugment, generate_density_map, pack_crop_windows


class RawCropLoader:
    def __init__(self, images: Sequence, labels: Sequence, augment: CropAugment, batch_size: int, num_crops: int = 1,
                 shuffle: bool = True, seed: int = 0, rank: int = 0, world: int = 1, device="cuda",
                 resident: bool = False, prefetch: bool = True):
        if len(images) != len(labels):
            raise ValueError(f"{len(images)} images but {len(labels)} labels")
        if batch_size <= 0 or num_crops <= 0:
            raise ValueError("batch_size and num_crops must be positive")
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside world {world}")
        self.raws = [_raw_image(im) for im in images]          # (contiguous uint8 tensor, layout, H, W)
        self.labels = [torch.as_tensor(l).reshape(-1, 2) for l in labels]
        self.augment, self.batch_size, self.num_crops = augment, int(batch_size), int(num_crops)
        self.shuffle, self.seed, self.rank, self.world = bool(shuffle), int(seed), int(rank), int(world)
        self.device, self.resident, self.prefetch = device, bool(resident), bool(prefetch)
        self.epoch = 0
        self._resident: Optional[List[Tensor]] = None          # the images as views of one device buffer
        self._pinned: List[Optional[Tensor]] = [None, None]
        self._copied: List[Optional[torch.cuda.Event]] = [None, None]
        self._side: Optional[torch.cuda.Stream] = None

    # ---------------------------------------------------------------- host only: the sampler's order
    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def indices(self) -> List[int]:
        """This rank's image indices for the current epoch: torch's `DistributedSampler(range(n), world, rank, shuffle,
        seed)` after `set_epoch` (its own generator, its padding by wrap-around)."""
        n = len(self.raws)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            idx = torch.randperm(n, generator=g).tolist()
        else:
            idx = list(range(n))
        total = math.ceil(n / self.world) * self.world
        pad = total - len(idx)
        if pad > 0 and idx:
            idx += idx[:pad] if pad <= len(idx) else (idx * math.ceil(pad / len(idx)))[:pad]
        return idx[self.rank:total:self.world]

    def batches(self) -> List[List[int]]:
        idx = self.indices()
        return [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]

    def __len__(self) -> int:
        return math.ceil(math.ceil(len(self.raws) / self.world) / self.batch_size)

    # ---------------------------------------------------------------- device half
    def _dev(self) -> torch.device:
        dev = torch.device(self.device)
        return torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev

    def _make_resident(self) -> List[Tensor]:
        """The whole split as bytes on the device, once: one buffer, every image a view at a 16-byte aligned start
        (copied image by image, so no second copy of the split is held in pinned memory)."""
        if self._resident is None:
            offs, total = [], 0
            for t, _, _, _ in self.raws:
                offs.append(total)
                total = (total + t.numel() + 15) & ~15
            buf = torch.empty(max(total, 16), dtype=torch.uint8, device=self._dev())
            views = []
            for (t, _, _, _), o in zip(self.raws, offs):
                views.append(buf[o:o + t.numel()].view(t.shape))
                views[-1].copy_(t)
            self._resident = views
        return self._resident

    def _plan(self, batch: List[int]):
        """Draw a batch's crops (Crowd.__getitem__'s num_crops crops of each image, in order) and move its labels."""
        plans, points = [], []
        for i, k in enumerate(batch):
            _, _, H, W = self.raws[k]
            for _ in range(self.num_crops):
                p, l = self.augment.plan_crop(i, H, W, self.labels[k].clone().float())
                plans.append(p)
                points.append(l)
        return plans, points

    def _stage(self, batch: List[int], slot: int, side: bool):
        """Draw `batch`, pack its windows into pinned buffer `slot` and start their copy, on the side stream or on the
        current one."""
        dev = self._dev()
        plans, points = self._plan(batch)
        images = [self.raws[k][0] for k in batch]
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()               # the copy that last read this pinned buffer has run
        packed = pack_crop_windows(plans, images, out=self._pinned[slot], pin=True)
        self._pinned[slot] = packed.buffer                 # (a larger one if this batch needed it)
        if side and self._side is None:
            self._side = torch.cuda.Stream(dev)
        stream = self._side if side else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            dwin = torch.empty(max(packed.nbytes, 16), dtype=torch.uint8, device=dev)
            dwin.copy_(packed.buffer[:dwin.numel()], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        self._copied[slot] = ev
        return images, plans, points, packed, dwin, ev

    def __iter__(self):
        size = self.augment.size
        batches = self.batches()
        if self.resident:
            src = self._make_resident()
            for batch in batches:
                plans, points = self._plan(batch)
                imgs = self.augment.apply([src[k] for k in batch], plans)
                yield imgs, points, generate_density_map(points, size[0], size[1], device=imgs.device)
            return
        staged = None
        for b in range(len(batches)):
            if staged is None:
                staged = self._stage(batches[b], b % 2, self.prefetch)
            images, plans, points, packed, dwin, ev = staged
            cur = torch.cuda.current_stream(dwin.device)
            cur.wait_event(ev)
            dwin.record_stream(cur)                        # allocated on the copy's stream, read on this one
            imgs = self.augment.apply(images, plans, windows=(packed, dwin))
            dens = generate_density_map(points, size[0], size[1], device=imgs.device)
            # batch b + 1 is drawn, packed and on its way before batch b is handed out: its copy runs beside step b
            staged = self._stage(batches[b + 1], (b + 1) % 2, True) if self.prefetch and b + 1 < len(batches) else None
            yield imgs, points, dens
