"""Generate the raw-image evaluation fixture (F12) by running the REFERENCE (Yiming-M/CLIP-EBC) on the CPU.

    python tests/golden/make_golden_eval_raw.py

What the reference's val split does to an image before and after the model, run by the reference's own code:
`image / 255.` (datasets/crowd.py:144), `Resize2Multiple` / `ZeroPad2Multiple` (datasets/transforms.py:69-135, loaded
by path), `Normalize(ImageNet)` (crowd.py:64,162) and `sliding_window_predict` (utils/eval_utils.py:26-96, loaded by
path as make_golden.py does) with the stub model of tests/test_gpu_eval.py.

torchvision is absent here, so `datasets/transforms.py` is loaded under stub `torchvision` modules defined below:
  * `TF.pad(img, (l, t, r, b), fill)` -> `F.pad(img, (l, r, t, b), value=fill)` (constant mode),
  * `TF.resize(img, size, BICUBIC, antialias=True)` -> `F.interpolate(mode="bicubic", antialias=True,
    align_corners=False)`, the call torchvision's tensor path makes (parity with torchvision itself is unpinned,
    as for the training augmentation),
  * `Normalize` is restated as torchvision's `tensor.sub(mean[:, None, None]).div(std[:, None, None])` in f32.

The fixture holds arrays, scalars and seeds only.  Per case k: `cfg_k` = [fit code (0 none, 1 zero_pad, 2 resize), H, W,
window, stride, image seed, fitted H, fitted W], `map_k` the reference's density map, `count_k` its sum.  Images are
regenerable: uint8 [H, W, 3] = PCG64(seed).integers(0, 256).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import REF, save  # noqa: E402

WINDOW = 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)     # datasets/crowd.py:64
FIT_CODES = {None: 0, "zero_pad": 1, "resize": 2}
# (fit, H, W, stride): the smallest shapes at which each branch can go wrong
CASES = [
    ("zero_pad", 250, 331, 112),     # 336x336, 2x2 overlapping tiles, odd 3 W row pitch
    ("zero_pad", 100, 300, 112),     # image smaller than the window -> 224x336
    ("zero_pad", 449, 225, 224),     # 672x448, 6 tiles
    ("zero_pad", 224, 224, 224),     # unchanged, 1 tile
    ("resize", 280, 392, 112),       # both half-way cases: round(0.5) = 0, round(1.5) = 2 -> 224x448
    ("resize", 250, 331, 112),       # 224x336
    ("resize", 100, 300, 112),       # negative quotient clamped -> 224x336
    (None, 300, 500, 224),           # border-snapped tiles
    (None, 300, 500, 112),
]


def load_transforms():
    """datasets/transforms.py under stub torchvision modules (see the module docstring)."""
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tf = types.ModuleType("torchvision.transforms.functional")

    class InterpolationMode:
        BICUBIC = "bicubic"

    def pad(img, padding, fill=0):
        left, top, right, bottom = padding
        return F.pad(img, (left, right, top, bottom), mode="constant", value=fill)

    def resize(img, size, interpolation=None, antialias=None):
        assert interpolation == InterpolationMode.BICUBIC and antialias is True
        lead = img.dim() == 3
        out = F.interpolate(img[None] if lead else img, size=tuple(size), mode="bicubic", antialias=True,
                            align_corners=False)
        return out[0] if lead else out

    tf.InterpolationMode, tf.pad, tf.resize = InterpolationMode, pad, resize
    tvt.ColorJitter = type("ColorJitter", (), {})
    tvt.functional = tf
    tv.transforms = tvt
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional")}
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tf})
    try:
        return mg._load("ref_transforms", f"{REF}/datasets/transforms.py")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


class Stub(torch.nn.Module):
    reduction = 8

    def forward(self, x):
        return F.avg_pool2d(x.mean(1, keepdim=True).abs(), 8)


def raw_image(seed: int, H: int, W: int) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W, 3), dtype=np.uint8)


def eval_raw_cases():
    tr = load_transforms()
    eu = mg._load("ref_eval_utils", f"{REF}/utils/eval_utils.py")
    mean = torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    std = torch.tensor(STD, dtype=torch.float32)[:, None, None]
    out = {"n_cases": np.asarray(len(CASES))}
    for k, (fit, H, W, stride) in enumerate(CASES):
        seed = 1200 + k
        u8 = torch.from_numpy(raw_image(seed, H, W)).permute(2, 0, 1).contiguous()      # the .npy layout, crowd.py:143
        image = u8.float() / 255.                                                        # crowd.py:144
        label = torch.zeros(0, 2)
        if fit == "zero_pad":
            image, _ = tr.ZeroPad2Multiple(WINDOW, stride)(image, label)
        elif fit == "resize":
            image, _ = tr.Resize2Multiple(WINDOW, stride)(image, label)
        image = image.sub(mean).div(std)                                                 # Normalize, crowd.py:162
        pred = eu.sliding_window_predict(Stub(), image[None], WINDOW, stride)
        out[f"cfg_{k}"] = np.asarray([FIT_CODES[fit], H, W, WINDOW, stride, seed, image.shape[-2], image.shape[-1]])
        out[f"map_{k}"] = pred.numpy()
        out[f"count_{k}"] = np.asarray(pred.sum(dim=(1, 2, 3)).numpy()[0])               # eval.py:27-36
        print(f"case {k}: fit={fit} {H}x{W} stride {stride} -> {tuple(image.shape[-2:])}, count {float(out[f'count_{k}']):.4f}")
    return out


if __name__ == "__main__":
    save("f12_eval_raw.npz", **eval_raw_cases())
