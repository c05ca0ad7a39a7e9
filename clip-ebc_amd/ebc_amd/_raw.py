"""Raw stored images (uint8 [H,W,3] / [3,H,W]): the layout rules the evaluation and the training input path share."""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _lib


def _raw_image(img) -> Tuple[Tensor, int, int, int]:
    """A uint8 [H,W,3] or [3,H,W] image -> (contiguous tensor, layout code, H, W)."""
    if not isinstance(img, Tensor):
        img = torch.as_tensor(img)
    if img.dtype != torch.uint8 or img.dim() != 3 or 3 not in (img.shape[0], img.shape[-1]):
        raise ValueError(f"images must be uint8 [H,W,3] or [3,H,W], got {img.dtype} {tuple(img.shape)}")
    if img.shape[0] == 3 and img.shape[-1] == 3:
        raise ValueError(f"cannot tell [H,W,3] from [3,H,W] for an image of shape {tuple(img.shape)}")
    if img.shape[-1] == 3:
        return img.contiguous(), _lib.EBC_EVAL_U8_HWC, int(img.shape[0]), int(img.shape[1])
    return img.contiguous(), _lib.EBC_EVAL_U8_CHW, int(img.shape[1]), int(img.shape[2])
