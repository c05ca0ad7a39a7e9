"""Sliding-window evaluation and error metrics (utils/eval_utils.py, eval.py), on device.

`sliding_window_predict(model, image, window_size, stride)` keeps the reference signature and
result (a CPU tensor [1, 1, H/r, W/r], overlaps averaged); tiles are gathered and the map assembled
by HIP kernels (`ebc_tile_gather` / `ebc_tile_assemble`) and the model runs once per tile batch.
Sharding the tiles of one image across ranks (BASELINE config 5) is OPT-IN (`shard=True`, every rank
of `group` must call): the reference trainer evaluates on rank 0 alone while the other ranks wait in
`dist.barrier()` (trainer.py:161-177,194), so a collective inside the default call would hang there.

`evaluate_raw` / `sliding_window_counts` run a split from raw uint8 images: what the reference's val split does on
the CPU before the model (`/255.`, `Resize2Multiple` or `ZeroPad2Multiple`, `Normalize`; datasets/crowd.py:141-162,
datasets/transforms.py:69-134, utils/data_utils.py:28-37) happens on the device, many images a call, with tile
batches that run across image boundaries and one read-back of the counts.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.distributed as dist
from torch import Tensor, nn

from . import _lib
from ._raw import _raw_image
from .distributed import gather_shards, shard_range
from .transforms import IMAGENET_MEAN, IMAGENET_STD, _upload


def calculate_errors(pred_counts: np.ndarray, gt_counts: np.ndarray) -> Dict[str, float]:
    """utils/eval_utils.py:8-16."""
    assert isinstance(pred_counts, np.ndarray), f"Expected numpy.ndarray, got {type(pred_counts)}"
    assert isinstance(gt_counts, np.ndarray), f"Expected numpy.ndarray, got {type(gt_counts)}"
    assert len(pred_counts) == len(gt_counts), f"Length of predictions and ground truths should be equal, but got {len(pred_counts)} and {len(gt_counts)}"
    return {"mae": np.mean(np.abs(pred_counts - gt_counts)), "rmse": np.sqrt(np.mean((pred_counts - gt_counts) ** 2))}


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, (int, float)) else tuple(int(x) for x in v)


def tile_grid(H: int, W: int, window: Tuple[int, int], stride: Tuple[int, int]) -> Tuple[int, int]:
    rows = int(np.ceil((H - window[0]) / stride[0]) + 1)
    cols = int(np.ceil((W - window[1]) / stride[1]) + 1)
    return rows, cols


def sliding_window_predict(model: nn.Module, image: Tensor, window_size: Union[int, Tuple[int, int]],
                           stride: Union[int, Tuple[int, int]], max_tiles_per_batch: int = 256,
                           shard: bool = False, group: Optional[object] = None) -> Tensor:
    """utils/eval_utils.py:26-96.  image [1, C, H, W] -> [1, Cp, H/r, W/r] (CPU tensor).

    shard=True (collective: every rank of `group` calls with the same image): each rank runs its
    contiguous share of the tiles and the predictions are all-gathered before the assembly."""
    assert len(image.shape) == 4, f"Image must be a 4D tensor (1, c, h, w), got {image.shape}"
    window, strd = _pair(window_size), _pair(stride)
    assert window[0] > 0 and window[1] > 0, f"Window size must be a positive integer tuple (h, w), got {window}"
    assert strd[0] > 0 and strd[1] > 0, f"Stride must be a positive integer tuple (h, w), got {strd}"
    assert strd[0] <= window[0] and strd[1] <= window[1], f"Stride must be smaller than window size, got {strd} and {window}"
    params = list(model.parameters())
    dev = params[0].device if params else (image.device if image.is_cuda else torch.device("cuda"))
    img = image.to(dev, torch.float32).contiguous()[0]
    C, H, W = img.shape
    rows, cols = tile_grid(H, W, window, strd)
    T = rows * cols
    reduction = getattr(model, "reduction", 1)
    world = dist.get_world_size(group) if shard and dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    t0, t1, per = shard_range(T, world, rank)
    L = _lib.lib()
    st = _lib.stream(dev)
    preds = None
    model.eval()
    with torch.no_grad(), _lib.on(dev):
        outs = []
        for b0 in range(t0, t1, max_tiles_per_batch):
            n = min(max_tiles_per_batch, t1 - b0)
            tiles = torch.empty(n, C, window[0], window[1], device=dev, dtype=torch.float32)
            _lib.check(L.ebc_tile_gather(_lib.ptr(img, dev), _lib.ptr(tiles), C, H, W, window[0], window[1], strd[0],
                                         strd[1], b0, n, st), "ebc_tile_gather")
            outs.append(model(tiles).float())
        if outs:
            preds = torch.cat(outs, 0)
        Cp = preds.shape[1] if preds is not None else 1
        ph, pw = window[0] // reduction, window[1] // reduction
        if world > 1:
            preds = gather_shards(preds, T, per, (Cp, ph, pw), dev, group)
        preds = preds.contiguous()
        out = torch.empty(Cp, H // reduction, W // reduction, device=dev)
        _lib.check(L.ebc_tile_assemble(_lib.ptr(preds, dev), _lib.ptr(out), Cp, H, W, window[0], window[1], strd[0],
                                       strd[1], reduction, st), "ebc_tile_assemble")
    return out.unsqueeze(0).cpu()


def evaluate(model: nn.Module, data_loader, device: torch.device, sliding_window: bool = False,
             window_size: Optional[int] = None, stride: Optional[int] = None) -> Dict[str, float]:
    """eval.py:11-40: per-image predicted count vs len(points); returns {"mae", "rmse"}."""
    model.eval()
    pred_counts, target_counts = [], []
    if sliding_window:
        assert window_size is not None, f"Window size must be provided when sliding_window is True, but got {window_size}"
        assert stride is not None, f"Stride must be provided when sliding_window is True, but got {stride}"
    for image, target_points, _ in data_loader:
        image = image.to(device)
        target_counts.append([len(p) for p in target_points])
        with torch.no_grad():
            if sliding_window:
                pred_density = sliding_window_predict(model, image, window_size, stride)
            else:
                pred_density = model(image)
            pred_counts.append(pred_density.sum(dim=(1, 2, 3)).cpu().numpy().tolist())
    pred_counts = np.array([x for s in pred_counts for x in s])
    target_counts = np.array([x for s in target_counts for x in s])
    return calculate_errors(pred_counts, target_counts)


# ------------------------------------------------------------------------------------------------------------------
# A split from raw uint8 images

FITS = (None, "zero_pad", "resize")


def fit_size(H: int, W: int, window, stride, fit: Optional[str] = None) -> Tuple[int, int]:
    """The size the val transform leaves an H x W image at: `ZeroPad2Multiple` (datasets/transforms.py:127-128),
    `Resize2Multiple` (:96-99, Python's round: half to even) or none (the image must hold one window)."""
    window, strd = _pair(window), _pair(stride)
    if fit is None:
        if H < window[0] or W < window[1]:
            raise ValueError(f"image {H}x{W} is smaller than the window {window}: pass fit='zero_pad' or fit='resize'")
        return int(H), int(W)
    if fit == "zero_pad":
        return (int(max(np.ceil((H - window[0]) / strd[0]), 0) * strd[0] + window[0]),
                int(max(np.ceil((W - window[1]) / strd[1]), 0) * strd[1] + window[1]))
    if fit == "resize":
        return (int(max(round((H - window[0]) / strd[0]), 0) * strd[0] + window[0]),
                int(max(round((W - window[1]) / strd[1]), 0) * strd[1] + window[1]))
    raise ValueError(f"fit must be one of {FITS}, got {fit!r}")


def _align16(n: int) -> int:
    return (n + 15) & ~15


def sliding_window_counts(model: nn.Module, images: Sequence[Tensor], window_size, stride, fit: Optional[str] = None,
                          max_tiles_per_batch: int = 256, return_maps: bool = False):
    """Predicted counts of a batch of raw images: `sliding_window_predict(...).sum()` of each image after the val
    transform `fit` and `Normalize`, all of it on the device.

    images: uint8 tensors [H,W,3] (a decoded JPEG) or [3,H,W] (the reference's .npy images), on the CPU or the device.
    The raw bytes go up in one packed copy; tiles are normalised straight from them (`ebc_tiles_from_raw`; zero
    padding is never materialised), the tile list runs across the images so every forward but the last is a full
    `max_tiles_per_batch`, and one launch pair assembles every map and sums it (`ebc_tiles_assemble_batch`).  With
    fit="resize" an image whose size changes is converted (`ebc_u8_to_chw01`) and resized by the augmentation's
    antialiased bicubic kernels (`ebc_augment_crops`, whole image as the crop) first.
    Returns counts [n] (CPU f32), and with return_maps the list of [1, Cp, Hf/r, Wf/r] CPU maps as well."""
    window, strd = _pair(window_size), _pair(stride)
    assert window[0] > 0 and window[1] > 0, f"Window size must be a positive integer tuple (h, w), got {window}"
    assert strd[0] > 0 and strd[1] > 0, f"Stride must be a positive integer tuple (h, w), got {strd}"
    assert strd[0] <= window[0] and strd[1] <= window[1], f"Stride must be smaller than window size, got {strd} and {window}"
    assert max_tiles_per_batch > 0, f"max_tiles_per_batch must be positive, got {max_tiles_per_batch}"
    if fit not in FITS:
        raise ValueError(f"fit must be one of {FITS}, got {fit!r}")
    raws = [_raw_image(im) for im in images]
    n = len(raws)
    if n == 0:
        return (torch.zeros(0), []) if return_maps else torch.zeros(0)
    fitted = [fit_size(H, W, window, strd, fit) for _, _, H, W in raws]
    params = list(model.parameters())
    on_dev = [t.device for t, _, _, _ in raws if t.is_cuda]
    dev = params[0].device if params else (on_dev[0] if on_dev else torch.device("cuda"))
    reduction = getattr(model, "reduction", 1)
    L = _lib.lib()
    st = _lib.stream(dev)

    # one device buffer: the raw bytes of every image (16-byte aligned starts), then the f32 planes of the resized ones
    src_off, resized, off = [], [], 0
    for k, (t, _, H, W) in enumerate(raws):
        src_off.append(off)
        off = _align16(off + t.numel())
        if fit == "resize" and fitted[k] != (H, W):      # (zero_pad stores nothing for the padding)
            resized.append(k)
    raw_bytes = off
    res_off = {}
    for k in resized:
        res_off[k] = off
        off = _align16(off + 4 * 3 * fitted[k][0] * fitted[k][1])
    descs = (_lib.EbcEvalImage * n)()
    tile0 = 0
    for k, (t, layout, H, W) in enumerate(raws):
        d = descs[k]
        Hf, Wf = fitted[k]
        if k in res_off:
            d.src_off, d.layout, d.H, d.W = res_off[k], _lib.EBC_EVAL_F32_CHW, Hf, Wf
        else:
            d.src_off, d.layout, d.H, d.W = src_off[k], layout, H, W
        d.Hf, d.Wf = Hf, Wf
        d.rows, d.cols = tile_grid(Hf, Wf, window, strd)
        d.tile0 = tile0
        tile0 += d.rows * d.cols
    T = tile0
    mean, std = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)

    def map_offsets(Cp: int) -> int:
        m = 0
        for d in descs:
            d.map_off = m
            m += Cp * (d.Hf // reduction) * (d.Wf // reduction)
        return m

    model.eval()
    with torch.no_grad(), _lib.on(dev):
        buf = torch.empty(off, dtype=torch.uint8, device=dev)
        if any(not t.is_cuda for t, _, _, _ in raws):
            host = torch.empty(raw_bytes, dtype=torch.uint8, pin_memory=True)
            for k, (t, _, _, _) in enumerate(raws):
                if not t.is_cuda:
                    host[src_off[k]:src_off[k] + t.numel()].copy_(t.reshape(-1))
            buf[:raw_bytes].copy_(host, non_blocking=True)
        for k, (t, _, _, _) in enumerate(raws):
            if t.is_cuda:
                buf[src_off[k]:src_off[k] + t.numel()].copy_(t.reshape(-1))
        if resized:
            _resize_on_device(L, buf, raws, fitted, src_off, res_off, resized, mean, std, dev, st)
        map_total = map_offsets(1)
        ddesc = _upload(descs, dev)
        outs = []
        for b0 in range(0, T, max_tiles_per_batch):
            nt = min(max_tiles_per_batch, T - b0)
            tiles = torch.empty(nt, 3, window[0], window[1], device=dev, dtype=torch.float32)
            _lib.check(L.ebc_tiles_from_raw(_lib.ptr(buf), _lib.ptr(ddesc), descs, n, window[0], window[1], strd[0],
                                            strd[1], b0, nt, mean, std, _lib.ptr(tiles), st), "ebc_tiles_from_raw")
            outs.append(model(tiles).float())
        preds = torch.cat(outs, 0).contiguous()
        Cp = int(preds.shape[1])
        if Cp != 1:                                  # the maps' offsets depend on the model's output channels
            map_total = map_offsets(Cp)
            ddesc = _upload(descs, dev)
        maps = torch.empty(map_total, device=dev, dtype=torch.float32)
        counts = torch.empty(n, device=dev, dtype=torch.float32)
        _lib.check(L.ebc_tiles_assemble_batch(_lib.ptr(preds, dev), _lib.ptr(ddesc), descs, n, Cp, window[0], window[1],
                                              strd[0], strd[1], reduction, _lib.ptr(maps), _lib.ptr(counts), st),
                   "ebc_tiles_assemble_batch")
        counts_cpu = counts.cpu()
        if not return_maps:
            return counts_cpu
        maps_cpu = maps.cpu()
    out_maps = []
    for d in descs:
        Ho, Wo = d.Hf // reduction, d.Wf // reduction
        out_maps.append(maps_cpu[d.map_off:d.map_off + Cp * Ho * Wo].view(1, Cp, Ho, Wo))
    return counts_cpu, out_maps


def _resize_on_device(L, buf: Tensor, raws, fitted, src_off, res_off, resized: List[int], mean, std, dev, st) -> None:
    """Resize2Multiple + Normalize of the images `resized`: u8 -> f32 [0, 1] planes, then `_resize`'s antialiased
    bicubic (datasets/transforms.py:34) as one whole-image crop each, normalised on the store, into buf + res_off."""
    in_off, ws_off, f01_n, ws_n = {}, {}, 0, 0
    for k in resized:
        _, _, H, W = raws[k]
        in_off[k], ws_off[k] = f01_n, ws_n
        f01_n += (3 * H * W + 3) & ~3
        ws_n += 3 * max(H, fitted[k][0]) * fitted[k][1]
    f01 = torch.empty(f01_n, device=dev, dtype=torch.float32)
    ws = torch.empty(ws_n, device=dev, dtype=torch.float32)
    base = min(res_off.values())
    cd = (_lib.EbcCropDesc * len(resized))()
    for i, k in enumerate(resized):
        _, layout, H, W = raws[k]
        _lib.check(L.ebc_u8_to_chw01(ctypes.c_void_p(buf.data_ptr() + src_off[k]), layout, H, W,
                                     ctypes.c_void_p(f01.data_ptr() + 4 * in_off[k]), st), "ebc_u8_to_chw01")
        d = cd[i]
        d.src_off, d.out_off, d.tmp_off, d.noise_off = in_off[k], (res_off[k] - base) // 4, ws_off[k], -1
        d.src_h, d.src_w, d.top, d.left, d.crop_h, d.crop_w = H, W, 0, 0, H, W
        d.out_h, d.out_w = fitted[k]
        d.brightness = d.contrast = d.saturation = 1.0
        d.normalize = 1
    const = _lib.EbcAugConst(mean, std, 1, 1.0, 1.0)
    _lib.check(L.ebc_augment_crops(_lib.ptr(f01), _lib.ptr(_upload(cd, dev)), len(resized),
                                   max(raws[k][2] for k in resized), max(fitted[k][0] for k in resized),
                                   ctypes.c_void_p(buf.data_ptr() + base), _lib.ptr(ws), None, const, st),
               "ebc_augment_crops (Resize2Multiple)")


def evaluate_raw(model: nn.Module, samples: Iterable, window_size, stride, fit: Optional[str] = None,
                 images_per_call: int = 32, max_tiles_per_batch: int = 256) -> Dict[str, float]:
    """`evaluate(..., sliding_window=True)` (eval.py:11-40) over `samples` = (uint8 image, points) pairs: the count of
    every image by `sliding_window_counts`, `images_per_call` images at a time, against len(points)."""
    assert images_per_call > 0, f"images_per_call must be positive, got {images_per_call}"
    pred_counts, target_counts, pending = [], [], []

    def flush():
        if pending:
            pred_counts.extend(sliding_window_counts(model, pending, window_size, stride, fit=fit,
                                                     max_tiles_per_batch=max_tiles_per_batch).numpy().tolist())
            pending.clear()

    for image, points in samples:
        pending.append(image)
        target_counts.append(len(points))
        if len(pending) == images_per_call:
            flush()
    flush()
    return calculate_errors(np.array(pred_counts), np.array(target_counts))
