"""GPU: evaluation from raw uint8 images (ebc_tiles_from_raw / ebc_u8_to_chw01 / ebc_tiles_assemble_batch and
`sliding_window_counts` / `evaluate_raw`) against the CPU preparation the reference's val split does, the
reference's own outputs (F12 fixture, tests/golden/make_golden_eval_raw.py) and today's per-image path."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ANCHORS_NWPU, BINS, golden

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HWC, CHW, F32 = 0, 1, 2
FITS = {0: None, 1: "zero_pad", 2: "resize"}
WIN = 224
# the real-model bar (see test_real_model_counts_match_the_per_image_path)
REAL_RTOL, REAL_ATOL = 1e-5, 1e-6


class Stub(torch.nn.Module):
    reduction = 8

    def forward(self, x):
        return torch.nn.functional.avg_pool2d(x.mean(1, keepdim=True).abs(), 8)


def raw_image(seed, H, W):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W, 3), dtype=np.uint8)


def prepared(u8_hwc, Hf, Wf):
    """The reference's CPU preparation of a zero-padded image: /255., pad right/bottom with 0, Normalize.  [3,Hf,Wf]"""
    x = torch.from_numpy(u8_hwc).permute(2, 0, 1).contiguous().float() / 255.
    x = torch.nn.functional.pad(x, (0, Wf - x.shape[2], 0, Hf - x.shape[1]), value=0.)
    return x.sub(torch.tensor(MEAN)[:, None, None]).div(torch.tensor(STD)[:, None, None])


def starts(full, win, stride):
    n = -(-(full - win) // stride) + 1
    return [min(i * stride, full - win) for i in range(n)]


def pack(images, layouts, fitted, stride, gap=0):
    """One byte buffer and the descriptors of u8 [H,W,3] images stored in `layouts`; `gap` extra bytes before each
    image, so that images start off a dword boundary."""
    from ebc_amd import _lib
    arr = (_lib.EbcEvalImage * len(images))()
    chunks, off, t0, moff = [], 0, 0, 0
    for d, im, lay, (Hf, Wf) in zip(arr, images, layouts, fitted):
        chunks.append(np.full(gap, 0xAB, np.uint8))
        off += gap
        H, W = im.shape[:2]
        chunks.append((im if lay == HWC else im.transpose(2, 0, 1)).reshape(-1))
        d.src_off, d.map_off, d.layout, d.H, d.W, d.Hf, d.Wf = off, moff, lay, H, W, Hf, Wf
        d.rows, d.cols, d.tile0 = len(starts(Hf, WIN, stride)), len(starts(Wf, WIN, stride)), t0
        t0 += d.rows * d.cols
        off += im.size
        moff += (Hf // 8) * (Wf // 8)
    chunks.append(np.zeros(-off % 16 + 16, np.uint8))
    return torch.from_numpy(np.concatenate(chunks)), arr, t0


def dev_desc(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


ZP_SIZES = [(250, 331), (100, 300), (449, 225), (224, 224)]          # the fixture's zero-pad images


@pytest.fixture(scope="module")
def zero_pad_set():
    """The zero-pad images and, per stride, their fitted sizes and the CPU tiles of the whole global list."""
    from ebc_amd.eval_utils import fit_size
    images = [raw_image(1200 + k, H, W) for k, (H, W) in enumerate(ZP_SIZES)]
    out = {"images": images}
    for stride in (112, 224):
        fitted = [fit_size(H, W, WIN, stride, "zero_pad") for H, W in ZP_SIZES]
        tiles = []
        for im, (Hf, Wf) in zip(images, fitted):
            x = prepared(im, Hf, Wf)
            tiles += [x[:, y:y + WIN, xx:xx + WIN] for y in starts(Hf, WIN, stride) for xx in starts(Wf, WIN, stride)]
        out[stride] = (fitted, torch.stack(tiles))
    return out


@pytest.mark.parametrize("stride", [112, 224])
@pytest.mark.parametrize("layouts,gap", [((HWC,) * 4, 0), ((CHW,) * 4, 0), ((HWC, CHW, CHW, HWC), 1), ((CHW, HWC, HWC, CHW), 3)])
def test_tiles_from_raw_is_bit_exact(zero_pad_set, stride, layouts, gap):
    """Images of different sizes in one call, whole list and sub-ranges that start and end inside an image, against the
    CPU ((u8.float() / 255) - mean) / std tiles of the zero-padded images: equal bit for bit; the tile after the
    output is untouched."""
    from ebc_amd import _lib
    L = _lib.lib()
    fitted, want = zero_pad_set[stride]
    buf, arr, T = pack(zero_pad_set["images"], layouts, fitted, stride, gap)
    assert T == want.shape[0] == {112: 15, 224: 13}[stride]
    dbuf, ddesc = buf.cuda(), dev_desc(arr)
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    first = arr[0].rows * arr[0].cols
    for begin, count in ((0, T), (1, first), (first - 1, T - first), (T - 1, 1), (2, 1)):
        tiles = torch.full((count + 1, 3, WIN, WIN), 12345.0, device="cuda")
        rc = L.ebc_tiles_from_raw(_lib.ptr(dbuf), _lib.ptr(ddesc), arr, len(arr), WIN, WIN, stride, stride, begin, count,
                                  mean, std, _lib.ptr(tiles), _lib.stream(tiles))
        assert rc == 0
        got = tiles.cpu()
        assert torch.equal(got[:count], want[begin:begin + count]), (begin, count)
        assert bool((got[count] == 12345.0).all())


@pytest.mark.parametrize("layout", [HWC, CHW])
@pytest.mark.parametrize("H,W", [(250, 331), (5, 3), (224, 224)])
def test_u8_to_chw01_is_bit_exact(layout, H, W):
    from ebc_amd import _lib
    L = _lib.lib()
    im = raw_image(7, H, W)
    src = torch.from_numpy(np.concatenate([(im if layout == HWC else im.transpose(2, 0, 1)).reshape(-1), np.zeros(16, np.uint8)]))
    out = torch.full((3 * H * W + 8,), -7.0, device="cuda")
    dsrc = src.cuda()
    assert L.ebc_u8_to_chw01(_lib.ptr(dsrc), layout, H, W, _lib.ptr(out), _lib.stream(out)) == 0
    want = torch.from_numpy(im).permute(2, 0, 1).contiguous().float() / 255.
    got = out.cpu()
    assert torch.equal(got[:3 * H * W].view(3, H, W), want)
    assert bool((got[3 * H * W:] == -7.0).all())


def assemble_f64(preds, Hf, Wf, stride, r=8):
    acc = torch.zeros(preds.shape[1], Hf // r, Wf // r, dtype=torch.float64)
    cnt = torch.zeros_like(acc)
    t = 0
    for y in starts(Hf, WIN, stride):
        for x in starts(Wf, WIN, stride):
            acc[:, y // r:(y + WIN) // r, x // r:(x + WIN) // r] += preds[t].double()
            cnt[:, y // r:(y + WIN) // r, x // r:(x + WIN) // r] += 1
            t += 1
    return acc / cnt


@pytest.mark.parametrize("Cp,stride,sizes", [(1, 112, [(336, 336), (224, 336), (672, 448), (300, 500)]),
                                             (2, 224, [(300, 500), (224, 224), (232, 240)]),
                                             (1, 224, [(224, 224), (2048, 3072)])])
def test_assemble_batch_maps_counts_and_repeatability(Cp, stride, sizes):
    """Maps against an f64 CPU assembly at test_gpu_eval.py's bars; counts within 1e-5 relative of the f64 sum (the
    terms are non-negative and pass through at most 44 additions: 44 * 2^-24 = 2.6e-6); two runs bit-identical."""
    from ebc_amd import _lib
    L = _lib.lib()
    arr = (_lib.EbcEvalImage * len(sizes))()
    t0 = moff = 0
    for d, (Hf, Wf) in zip(arr, sizes):
        d.layout, d.H, d.W, d.Hf, d.Wf, d.tile0, d.map_off = HWC, Hf, Wf, Hf, Wf, t0, moff
        d.rows, d.cols = len(starts(Hf, WIN, stride)), len(starts(Wf, WIN, stride))
        t0 += d.rows * d.cols
        moff += Cp * (Hf // 8) * (Wf // 8)
    g = np.random.Generator(np.random.PCG64(5))
    preds = torch.from_numpy(np.abs(g.standard_normal((t0, Cp, WIN // 8, WIN // 8))).astype(np.float32))
    dp, ddesc = preds.cuda(), dev_desc(arr)
    runs = []
    for _ in range(2):
        maps = torch.full((moff + 4,), -3.0, device="cuda")
        counts = torch.full((len(sizes) + 1,), -3.0, device="cuda")
        rc = L.ebc_tiles_assemble_batch(_lib.ptr(dp), _lib.ptr(ddesc), arr, len(sizes), Cp, WIN, WIN, stride, stride, 8,
                                        _lib.ptr(maps), _lib.ptr(counts), _lib.stream(maps))
        assert rc == 0
        runs.append((maps.cpu(), counts.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    maps, counts = runs[0]
    assert bool((maps[moff:] == -3.0).all()) and float(counts[-1]) == -3.0
    for i, (d, (Hf, Wf)) in enumerate(zip(arr, sizes)):
        n = d.rows * d.cols
        want = assemble_f64(preds[d.tile0:d.tile0 + n], Hf, Wf, stride)
        got = maps[d.map_off:d.map_off + want.numel()].view(want.shape)
        np.testing.assert_allclose(got.numpy(), want.float().numpy(), rtol=2e-6, atol=1e-7)
        total = float(want.sum())
        assert abs(float(counts[i]) - total) <= 1e-5 * total, (i, float(counts[i]), total)


def _check_f12(d, k, count, dmap):
    fit, H, W, win, stride, seed, Hf, Wf = (int(v) for v in d[f"cfg_{k}"])
    want = d[f"map_{k}"]
    assert tuple(dmap.shape) == want.shape == (1, 1, Hf // 8, Wf // 8) and dmap.device.type == "cpu"
    if FITS[fit] == "resize":
        # the augmentation tests' post-normalisation bar for the resized pixels; the stub (mean, abs, average) is a
        # contraction, so the map keeps it
        np.testing.assert_allclose(dmap.numpy(), want, rtol=0, atol=1e-4)
        assert abs(float(count) - float(d[f"count_{k}"])) <= 1e-4 * want.size
    else:
        np.testing.assert_allclose(dmap.numpy(), want, rtol=2e-6, atol=1e-7)            # F5's bars
        assert abs(float(count) - float(d[f"count_{k}"])) <= 1e-5 * float(d[f"count_{k}"])


@pytest.mark.parametrize("case", range(9))
def test_stub_model_matches_reference_fixture(case):
    """One image a call, [H,W,3] from the CPU: the reference's Normalize(transform(u8 / 255)) + sliding_window_predict."""
    from ebc_amd.eval_utils import sliding_window_counts
    d = golden("f12_eval_raw.npz")
    fit, H, W, win, stride, seed, Hf, Wf = (int(v) for v in d[f"cfg_{case}"])
    img = torch.from_numpy(raw_image(seed, H, W))
    counts, maps = sliding_window_counts(Stub(), [img], win, stride, fit=FITS[fit], max_tiles_per_batch=5, return_maps=True)
    assert counts.shape == (1,) and len(maps) == 1
    _check_f12(d, case, counts[0], maps[0])


@pytest.mark.parametrize("group", [(0, 1), (4, 5, 6), (2, 3), (7,), (8,)])
def test_stub_model_batches_of_fixture_cases(group):
    """The fixture cases that share a fit and a stride in ONE call: both layouts, CPU and device tensors mixed, batches
    of 5 tiles that run across the images."""
    from ebc_amd.eval_utils import sliding_window_counts
    d = golden("f12_eval_raw.npz")
    images = []
    for n, k in enumerate(group):
        fit, H, W, win, stride, seed, Hf, Wf = (int(v) for v in d[f"cfg_{k}"])
        img = torch.from_numpy(raw_image(seed, H, W))
        if n % 2:
            img = img.permute(2, 0, 1).contiguous()
        images.append(img.cuda() if n >= 1 else img)
    counts, maps = sliding_window_counts(Stub(), images, win, stride, fit=FITS[fit], max_tiles_per_batch=5, return_maps=True)
    only = sliding_window_counts(Stub(), images, win, stride, fit=FITS[fit], max_tiles_per_batch=5)
    assert torch.equal(only, counts)
    for n, k in enumerate(group):
        _check_f12(d, k, counts[n], maps[n])


REAL_SIZES = [(250, 331), (449, 225), (300, 500)]


def test_real_model_counts_match_the_per_image_path():
    """A 2-layer clip_vit_b_16 on three u8 images, fit="zero_pad", stride 224, batches of 5 tiles that span the images,
    against `sliding_window_predict` per image on the CPU-prepared tensor, and `evaluate_raw` against `evaluate`.

    The tiles are bit-equal (test_tiles_from_raw_is_bit_exact), so the only difference is which tiles share a forward.
    The bar is 4x the largest map difference `sliding_window_predict` itself shows on these three prepared images
    between max_tiles_per_batch=256 and =5, floored at test_gpu_eval.py's rtol=1e-5, atol=1e-6.  Measured: 0.0 (the maps
    of the two batchings are bit-identical: every kernel of the forward works a crop at a time), so the bar is the floor,
    rtol=1e-5, atol=1e-6.  The same bar holds each count (a sum of non-negative map elements), and with it MAE and RMSE,
    which move by at most the largest count difference."""
    from ebc_amd.eval_utils import evaluate, evaluate_raw, fit_size, sliding_window_counts, sliding_window_predict
    from ebc_amd.model import get_model
    txt = torch.from_numpy(golden("f6_text.npz")["text_features_word"])
    m = get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, prompt_type="word", vit_layers=2, text_features=txt,
                  weights_seed=0).cuda().eval()
    raws = [raw_image(40 + k, H, W) for k, (H, W) in enumerate(REAL_SIZES)]
    prep = [prepared(im, *fit_size(im.shape[0], im.shape[1], WIN, WIN, "zero_pad"))[None] for im in raws]
    want = [sliding_window_predict(m, x, WIN, WIN) for x in prep]
    images = [torch.from_numpy(raws[0]), torch.from_numpy(raws[1]).permute(2, 0, 1).contiguous(), torch.from_numpy(raws[2])]
    counts, maps = sliding_window_counts(m, images, WIN, WIN, fit="zero_pad", max_tiles_per_batch=5, return_maps=True)
    for k in range(3):
        print(f"image {k}: max |map - per-image map| = {float((maps[k] - want[k]).abs().max()):.3e}, "
              f"count {float(counts[k]):.6f} vs {float(want[k].sum()):.6f}")
    for k in range(3):
        np.testing.assert_allclose(maps[k].numpy(), want[k].numpy(), rtol=REAL_RTOL, atol=REAL_ATOL)
        ref = float(want[k].sum())
        assert abs(float(counts[k]) - ref) <= REAL_ATOL + REAL_RTOL * abs(ref)
    points = [np.zeros((n, 2), np.float32) for n in (37, 120, 5)]
    loader = [(x, [p], None) for x, p in zip(prep, points)]
    e_ref = evaluate(m, loader, torch.device("cuda"), sliding_window=True, window_size=WIN, stride=WIN)
    e_raw = evaluate_raw(m, zip(images, points), WIN, WIN, fit="zero_pad", images_per_call=2, max_tiles_per_batch=5)
    slack = max(REAL_ATOL + REAL_RTOL * abs(float(w.sum())) for w in want)
    print("evaluate", e_ref, "evaluate_raw", e_raw)
    assert abs(e_raw["mae"] - e_ref["mae"]) <= slack and abs(e_raw["rmse"] - e_ref["rmse"]) <= slack


def test_small_image_without_a_fit_is_refused():
    from ebc_amd.eval_utils import sliding_window_counts
    with pytest.raises(ValueError):
        sliding_window_counts(Stub(), [torch.zeros(100, 300, 3, dtype=torch.uint8)], 224, 112)
    with pytest.raises(ValueError):
        sliding_window_counts(Stub(), [torch.zeros(1, 3, 300, 300)], 224, 112)
