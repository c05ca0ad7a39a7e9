"""CPU checks of the raw-image evaluation path: `fit_size` against the sizes the reference's own Resize2Multiple /
ZeroPad2Multiple produced (F12 fixture, tests/golden/make_golden_eval_raw.py), and the host checks of the three
exports (every bad argument is EBC_E_ARG before any device work, so they answer without a device)."""
import ctypes
import os
import subprocess

import pytest

from conftest import REPO, golden

EBC_E_ARG = -1
_X = 0x1000          # a non-NULL, 16-byte aligned pointer value; every call below is rejected before it is dereferenced
FITS = {0: None, 1: "zero_pad", 2: "resize"}
HWC, CHW, F32 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from ebc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "clip-ebc_amd")])
    return _lib.load()


def test_fit_size_matches_the_reference_for_every_fixture_case():
    from ebc_amd.eval_utils import fit_size
    d = golden("f12_eval_raw.npz")
    assert int(d["n_cases"]) == 9
    for k in range(int(d["n_cases"])):
        fit, H, W, win, stride, _, Hf, Wf = (int(v) for v in d[f"cfg_{k}"])
        assert fit_size(H, W, win, stride, FITS[fit]) == (Hf, Wf), (k, FITS[fit], H, W)


def test_fit_size_rounds_half_to_even_and_clamps():
    from ebc_amd.eval_utils import fit_size
    assert fit_size(280, 392, 224, 112, "resize") == (224, 448)        # round(0.5) = 0, round(1.5) = 2
    assert fit_size(100, 300, 224, 112, "resize") == (224, 336)        # round(-1.1) clamped to 0
    assert fit_size(100, 300, 224, 112, "zero_pad") == (224, 336)
    assert fit_size(225, 224, (224, 224), (224, 112), "zero_pad") == (448, 224)
    assert fit_size(300, 500, 224, 224, None) == (300, 500)


@pytest.mark.parametrize("H,W", [(100, 300), (300, 100), (223, 224)])
def test_fit_none_refuses_an_image_smaller_than_the_window(H, W):
    from ebc_amd.eval_utils import fit_size
    with pytest.raises(ValueError):
        fit_size(H, W, 224, 112, None)


def test_fit_size_refuses_an_unknown_fit():
    from ebc_amd.eval_utils import fit_size
    with pytest.raises(ValueError):
        fit_size(300, 500, 224, 112, "pad")


def _descs(images, win=224, stride=112):
    """Descriptors of (layout, H, W, Hf, Wf) images with the tiling's own rows / cols / tile0."""
    from ebc_amd import _lib
    arr = (_lib.EbcEvalImage * len(images))()
    t0 = off = moff = 0
    for d, (layout, H, W, Hf, Wf) in zip(arr, images):
        d.src_off, d.map_off, d.layout, d.H, d.W, d.Hf, d.Wf = off, moff, layout, H, W, Hf, Wf
        d.rows, d.cols = -(-(Hf - win) // stride) + 1, -(-(Wf - win) // stride) + 1
        d.tile0 = t0
        t0 += d.rows * d.cols
        off += (3 * H * W * (4 if layout == F32 else 1) + 15) & ~15
        moff += (Hf // 8) * (Wf // 8)
    return arr, t0


MEAN = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
STD = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
GOOD = [(HWC, 250, 331, 336, 336), (CHW, 100, 300, 224, 336)]


def _gather(lib, arr, n, begin, count, src=_X, ddesc=_X, tiles=_X, win=224, stride=112, mean=MEAN, std=STD):
    return lib.ebc_tiles_from_raw(src, ddesc, arr, n, win, win, stride, stride, begin, count, mean, std, tiles, None)


def _assemble(lib, arr, n, preds=_X, ddesc=_X, maps=_X, counts=_X, Cp=1, win=224, stride=112, r=8):
    return lib.ebc_tiles_assemble_batch(preds, ddesc, arr, n, Cp, win, win, stride, stride, r, maps, counts, None)


@pytest.mark.parametrize("bad", [
    dict(Hf=112),                    # Hf < wh
    dict(Wf=220),                    # Wf < ww
    dict(H=400, Hf=336),             # Hf < H
    dict(W=400, Wf=336),             # Wf < W
    dict(layout=3), dict(layout=-1),
    dict(H=0), dict(W=-5),
    dict(rows=7), dict(cols=0), dict(tile0=1),
    dict(src_off=-16), dict(map_off=-1),
    dict(Hf=1 << 15, Wf=1 << 15),    # 3 Hf Wf past int32
])
def test_batch_exports_reject_a_bad_descriptor_without_device(lib, bad):
    arr, T = _descs(GOOD)
    for k, v in bad.items():
        setattr(arr[0], k, v)
    assert _gather(lib, arr, 2, 0, 1) == EBC_E_ARG
    assert _assemble(lib, arr, 2) == EBC_E_ARG


def test_tiles_from_raw_rejects_without_device(lib):
    arr, T = _descs(GOOD)
    assert T == 4 + 2
    for begin, count in ((-1, 2), (0, T + 1), (T, 1), (5, 2), (0, -1), (2 ** 31 - 1, 2)):      # outside the list
        assert _gather(lib, arr, 2, begin, count) == EBC_E_ARG, (begin, count)
    for kw in (dict(src=None), dict(ddesc=None), dict(tiles=None), dict(mean=None), dict(std=None),
               dict(src=_X + 2), dict(tiles=_X + 4),                                          # alignment
               dict(win=0), dict(stride=0), dict(stride=225), dict(win=222, stride=111)):     # ww % 4
        assert _gather(lib, arr, 2, 0, 1, **kw) == EBC_E_ARG, kw
    assert _gather(lib, None, 2, 0, 1) == EBC_E_ARG and _gather(lib, arr, 0, 0, 0) == EBC_E_ARG
    f32, _ = _descs([(F32, 224, 336, 224, 336)])
    f32[0].src_off = 6                                       # f32 planes off a 4-byte boundary
    assert _gather(lib, f32, 1, 0, 1) == EBC_E_ARG
    big, Tb = _descs([(HWC, 224, 224, 224, 224)] * 15000, stride=224)                         # 3 wh ww tile_count past int32
    assert Tb == 15000 and _gather(lib, big, 15000, 0, 15000, stride=224) == EBC_E_ARG
    assert _gather(lib, arr, 2, 3, 0) == 0                   # an empty range of a valid list: nothing to launch


def test_u8_to_chw01_rejects_without_device(lib):
    for args in ((None, HWC, 8, 8, _X), (_X, HWC, 8, 8, None), (_X, F32, 8, 8, _X), (_X, -1, 8, 8, _X), (_X, HWC, 0, 8, _X),
                 (_X, CHW, 8, -1, _X), (_X + 1, HWC, 8, 8, _X), (_X, CHW, 8, 8, _X + 2), (_X, HWC, 1 << 15, 1 << 15, _X)):
        assert lib.ebc_u8_to_chw01(*args, None) == EBC_E_ARG, args


def test_tiles_assemble_batch_rejects_without_device(lib):
    arr, _ = _descs(GOOD)
    for kw in (dict(preds=None), dict(ddesc=None), dict(maps=None), dict(counts=None), dict(Cp=0), dict(r=0), dict(r=-8),
               dict(stride=0), dict(win=448)):
        assert _assemble(lib, arr, 2, **kw) == EBC_E_ARG, kw
    assert _assemble(lib, None, 2) == EBC_E_ARG and _assemble(lib, arr, 0) == EBC_E_ARG
    arr[1].map_off = 2 ** 31                                 # the maps past int32
    assert _assemble(lib, arr, 2) == EBC_E_ARG
    big, _ = _descs([(HWC, 224, 224, 224, 224)] * 3000, stride=224)
    assert _assemble(lib, big, 3000, Cp=1024, stride=224) == EBC_E_ARG                        # preds past int32
