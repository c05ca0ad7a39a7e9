"""CPU checks of the raw training input path: the window packing (`pack_crop_windows`, pure host), `RawCropLoader`'s
index order against torch's own `DistributedSampler`, and every EBC_E_ARG case of `ebc_augment_crops_raw` with the
library loaded without a device (bogus non-NULL pointers: a call that launched would not return)."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import REPO

HWC, CHW, F32 = 0, 1, 2


def _img(h, w, layout, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (h, w, 3) if layout == HWC else (3, h, w)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _plan(image, top, left, ch, cw, pre=None):
    from ebc_amd.transforms import CropPlan
    return CropPlan(image, top, left, ch, cw, pre, False)


# ------------------------------------------------------------------------------------------------ packing
def test_packing_holds_each_window_at_aligned_offsets(monkeypatch):
    from ebc_amd.transforms import pack_crop_windows
    images = [_img(23, 37, HWC, 1), _img(31, 29, CHW, 2), _img(9, 11, HWC, 3), _img(8, 13, CHW, 4)]
    plans = [_plan(0, 0, 0, 16, 13), _plan(0, 5, 7, 16, 20), _plan(0, 7, 17, 16, 20), _plan(1, 0, 3, 17, 5),
             _plan(1, 14, 9, 17, 20), _plan(2, 4, 2, 16, 16, pre=(33, 40)), _plan(3, 1, 1, 16, 16, pre=(20, 33)),
             _plan(2, 0, 0, 20, 20, pre=(41, 50))]

    def no_float(*a, **k):
        raise AssertionError("the packing made a float image")
    monkeypatch.setattr(torch.Tensor, "float", no_float)
    pk = pack_crop_windows(plans, images)
    monkeypatch.undo()
    assert pk.buffer.dtype == torch.uint8 and not pk.buffer.is_cuda
    expected_total, seen_whole = 0, {}
    for k, p in enumerate(plans):
        off, h, w = pk.offsets[k], pk.heights[k], pk.widths[k]
        assert off % 16 == 0 and off >= 0
        img = images[p.image]
        hwc = img.shape[-1] == 3
        assert pk.layouts[k] == (HWC if hwc else CHW)
        if p.pre_resize is not None:                                       # the whole image, once per image
            want = img
            assert (h, w) == ((img.shape[0], img.shape[1]) if hwc else (img.shape[1], img.shape[2]))
            if p.image in seen_whole:
                assert off == seen_whole[p.image]
            else:
                assert off == expected_total
                seen_whole[p.image] = off
                expected_total = (expected_total + img.numel() + 15) & ~15
        else:
            assert (h, w) == (p.crop_h, p.crop_w)
            want = (img[p.top:p.top + h, p.left:p.left + w, :] if hwc else img[:, p.top:p.top + h, p.left:p.left + w])
            assert off == expected_total
            expected_total = (expected_total + 3 * h * w + 15) & ~15
        got = pk.buffer[off:off + 3 * h * w].view(want.shape)
        assert torch.equal(got, want), k
    assert pk.nbytes == expected_total
    sizes = [3 * 16 * 13, 3 * 16 * 20, 3 * 16 * 20, 3 * 17 * 5, 3 * 17 * 20, 3 * 9 * 11, 3 * 8 * 13]
    assert pk.nbytes == sum((s + 15) & ~15 for s in sizes) and pk.nbytes - sum(sizes) < 16 * len(sizes)


def test_packing_skips_device_and_float_images_and_reuses_a_buffer():
    from ebc_amd.transforms import pack_crop_windows
    images = [torch.rand(3, 20, 20), _img(20, 21, CHW, 5)]
    plans = [_plan(0, 0, 0, 16, 16), _plan(1, 2, 3, 16, 16)]
    out = torch.empty(4096, dtype=torch.uint8)
    pk = pack_crop_windows(plans, images, out=out)
    assert pk.buffer is out and pk.offsets == [-1, 0] and pk.nbytes == 3 * 16 * 16
    assert torch.equal(out[:768].view(3, 16, 16), images[1][:, 2:18, 3:19])
    small = torch.empty(100, dtype=torch.uint8)
    assert pack_crop_windows(plans, images, out=small).buffer is not small
    with pytest.raises(ValueError):
        pack_crop_windows([_plan(1, 10, 0, 16, 16)], images)               # leaves its image
    with pytest.raises(ValueError):
        pack_crop_windows([_plan(0, 0, 0, 2, 2)], [torch.zeros(3, 8, 3, dtype=torch.uint8)])   # either layout


# ------------------------------------------------------------------------------------------------ loader order
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("n,world,batch", [(10, 1, 4), (10, 3, 4), (7, 2, 2)])
def test_loader_order_is_the_distributed_samplers(n, world, batch, shuffle):
    from torch.utils.data import DistributedSampler
    from ebc_amd.loader import RawCropLoader
    from ebc_amd.transforms import CropAugment
    images = [_img(20 + i, 24, HWC, i) for i in range(n)]
    labels = [torch.zeros(0, 2) for _ in range(n)]
    aug = CropAugment(16)
    for rank in range(world):
        loader = RawCropLoader(images, labels, aug, batch, shuffle=shuffle, seed=3, rank=rank, world=world)
        sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=3)
        for epoch in (0, 1):
            loader.set_epoch(epoch)
            sampler.set_epoch(epoch)
            want = list(sampler)
            assert loader.indices() == want
            assert [i for b in loader.batches() for i in b] == want
            assert len(loader) == len(loader.batches()) == -(-len(want) // batch)
            assert all(len(b) == batch for b in loader.batches()[:-1])


# ------------------------------------------------------------------------------------------------ argument checks
EBC_E_ARG = -1
_X = 0x1000          # a non-NULL pointer value; every call below is rejected before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    from ebc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "clip-ebc_amd")])
    return _lib.load()


def _call(lib, src=_X, csrc_dev=_X, desc_dev=_X, out=_X, ws=_X, n=1, blur_k=5, host=True, s=None, d=None):
    from ebc_amd import _lib
    cs, ds = (_lib.EbcCropSrc * 1)(), (_lib.EbcCropDesc * 1)()
    cs[0].src_off, cs[0].layout, cs[0].H, cs[0].W = 0, HWC, 100, 120
    ds[0].top, ds[0].left, ds[0].crop_h, ds[0].crop_w, ds[0].out_h, ds[0].out_w = 10, 20, 50, 60, 16, 16
    ds[0].noise_off = -1
    for key, v in (s or {}).items():
        setattr(cs[0], key, v)
    for key, v in (d or {}).items():
        setattr(ds[0], key, v)
    const = _lib.EbcAugConst((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), blur_k, 0.1, 5.0)
    return lib.ebc_augment_crops_raw(src, csrc_dev, cs if host else None, desc_dev, ds if host else None, n, out, ws,
                                     None, const, None)


BIG = 0x7FFFFFFF
_BAD = [dict(src=None), dict(csrc_dev=None), dict(desc_dev=None), dict(host=False), dict(out=None), dict(ws=None),
        dict(n=-1), dict(n=21846),
        dict(s=dict(layout=3)), dict(s=dict(layout=-1)),
        dict(s=dict(layout=F32, src_off=2)), dict(s=dict(layout=F32), src=0x1002), dict(s=dict(src_off=-16)),
        dict(d=dict(top=-1)), dict(d=dict(left=-1)), dict(d=dict(top=51)), dict(d=dict(left=61)),
        dict(d=dict(top=BIG)), dict(d=dict(left=BIG)), dict(s=dict(H=0)), dict(s=dict(W=0)),
        dict(d=dict(crop_h=0)), dict(d=dict(crop_w=0)), dict(d=dict(crop_h=-4)), dict(d=dict(crop_w=-4)),
        dict(d=dict(out_h=0)), dict(d=dict(out_w=0)), dict(d=dict(out_h=-1)), dict(d=dict(out_w=-1)),
        dict(blur_k=0), dict(blur_k=4), dict(blur_k=33), dict(blur_k=-1),
        dict(s=dict(H=40000, W=40000)),                                    # 3 H W past int32
        dict(s=dict(H=20000, W=20000), d=dict(crop_h=20000, crop_w=16, out_w=40000, top=0, left=0)),   # 3 crop_h out_w
        dict(d=dict(out_h=30000, out_w=30000))]                            # 3 out_h out_w


@pytest.mark.parametrize("kw", _BAD, ids=[str(i) for i in range(len(_BAD))])
def test_augment_crops_raw_rejects_without_device(lib, kw):
    """NULL pointers (either copy of the descriptors), n out of range, a layout that is none of the three, an F32
    source whose offset or base is not 4-byte aligned, a negative offset, a window that leaves its source, empty
    sizes, blur_k outside ebc_augment_crops' rule, sizes past int32."""
    assert _call(lib, **kw) == EBC_E_ARG


def test_augment_crops_raw_accepts_an_empty_batch_without_device(lib):
    assert _call(lib, n=0) == 0
