"""The float64 references of tests/_conv_refs.py against F.conv2d, torch.nn.grad.conv2d_weight, autograd and plain torch
(no GPU), to 1e-12 relative; geometry against the library's own host-only ebc_dec_geometry; and the facts the bounds of
tests/test_gpu_conv_kernels.py lean on."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _conv_refs as R
from ebc_amd import _lib

F64 = torch.float64
SHAPES = [(1, 3, 5, 64, 64), (3, 4, 7, 64, 64), (2, 6, 3, 64, 128)]          # (B, H, W, C, N), H != W


def _close(a, b, tol=1e-12):
    a, b = a.detach().to(F64), b.detach().to(F64)
    scale = max(float(b.abs().max()), 1e-300)
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_fwd_reads_the_image_as_given(shape):
    """A non-zero frame is part of the sum (padding = 0 on the padded image); the slack columns are never read (NaN)."""
    B, H, W, C, N = shape
    geo = R.geometry(B, H, W)
    x, wk = _rand(B, H, W, C, seed=1), _rand(N, 3, 3, C, seed=2)
    xpad = R.pad_image(x, geo, pad_fill=_rand(B, geo["Hp"], geo["Wp"], C, seed=3), slack_fill=float("nan"))
    assert bool(xpad[:, :, W + 2:].isnan().all()) and not bool(xpad[:, :, :W + 2].isnan().any())
    assert torch.equal(xpad[:, 1:H + 1, 1:W + 1], x) and float(xpad[:, 0, :W + 2].abs().min()) > 0
    P, Sp = R.conv_fwd(xpad, wk, geo)
    img = xpad[:, :, :W + 2].permute(0, 3, 1, 2)
    w = wk.permute(0, 3, 1, 2)                                             # [N][C][3][3]
    _close(P, F.conv2d(img, w, padding=0).permute(0, 2, 3, 1).reshape(-1, N))
    _close(Sp, F.conv2d(img.abs(), w.abs(), padding=0).permute(0, 2, 3, 1).reshape(-1, N))
    assert R.conv_fwd(xpad, wk, geo, with_abs=False)[1] is None
    # with a zero frame it is nn.Conv2d(C, N, 3, padding=1)
    P0, _ = R.conv_fwd(R.pad_image(x, geo), wk, geo)
    _close(P0, F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, N))


def test_pad_image_fills():
    geo = R.geometry(2, 3, 5)
    x = _rand(2, 3, 5, 8, seed=4)
    p = R.pad_image(x, geo, pad_fill=2.0, slack_fill=-3.0)
    assert p.shape == (2, 5, 32, 8) and torch.equal(p[:, 1:4, 1:6], x)
    assert bool((p[:, :, 7:] == -3.0).all()) and bool((p[:, 0, :7] == 2.0).all()) and bool((p[:, 4, :7] == 2.0).all())
    assert bool((p[:, :, 0] == 2.0).all()) and bool((p[:, :, 6] == 2.0).all())
    assert int((p == 2.0).sum()) == 2 * 8 * (5 * 7 - 3 * 5)


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_wgrad_is_the_weight_gradient(shape):
    B, H, W, C, N = shape
    x, dz = _rand(B, H, W, C, seed=5), _rand(B, H, W, N, seed=6)
    dW, Sp = R.conv_wgrad(dz, x)
    xi, gi = x.permute(0, 3, 1, 2), dz.permute(0, 3, 1, 2)
    _close(dW, torch.nn.grad.conv2d_weight(xi, (N, C, 3, 3), gi, padding=1))
    _close(Sp, torch.nn.grad.conv2d_weight(xi.abs(), (N, C, 3, 3), gi.abs(), padding=1))
    w = _rand(N, C, 3, 3, seed=7).requires_grad_(True)
    (g,) = torch.autograd.grad((F.conv2d(xi, w, padding=1) * gi).sum(), w)
    _close(dW, g)


def test_stats_and_add_relu_grad():
    P = _rand(37, 64, seed=8)
    s, q = R.stats(P)
    _close(s, P.sum(0))
    _close(q, P.pow(2).sum(0))
    gy = _rand(37, 64, seed=9)
    y = _rand(37, 64, seed=10)
    y[0, :4] = torch.tensor([-0.0, 0.0, -1.0, 1.0], dtype=F64)
    ref = R.add_relu_grad(P, gy, y)
    _close(ref, P + gy * (y > 0).to(F64))
    assert torch.equal(ref[0, :3], P[0, :3]) and torch.equal(ref[0, 3], P[0, 3] + gy[0, 3])
    yy = y.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((torch.relu(yy) * gy).sum(), yy)           # relu'(0) = 0
    _close(ref, P + g)


@pytest.mark.parametrize("dcode", [_lib.EBC_F32, _lib.EBC_F16])
def test_geometry_is_the_librarys(dcode):
    L = _lib.load()
    out = (ctypes.c_long * 6)()
    for B in (1, 2, 3, 5, 16, 31):
        for H in (1, 2, 6, 7, 10, 14, 28, 31, 56):
            for W in (2, 5, 6, 7, 10, 14, 29, 30, 31, 56, 62):
                assert L.ebc_dec_geometry(dcode, B, H, W, 64, out) == 0
                g = R.geometry(B, H, W)
                assert tuple(out) == (g["Hp"], g["Wp"], g["HWp"], g["Kq"], g["Q"], g["Qs"]), (B, H, W)
                # what conv_gemm requires of MODE 2, and room for the last chunk's reads
                assert g["HWp"] >= 64 and g["HWp"] % 8 == 0 and g["Pimg"] >= g["HWp"] and g["Qs"] >= g["Kq"]
                assert g["Wp"] % 8 == 0 and g["Wp"] >= W + 2
    assert [R.geometry(1, 4, w)["Wp"] for w in (10, 30, 31, 56)] == [32, 32, 40, 64]


def test_mode2_operand_layouts():
    B, H, W, N = 3, 3, 5, 8
    geo = R.geometry(B, H, W)
    dz = _rand(B, H, W, N, seed=11)
    t = R.dz_transposed(dz, geo, fill=0.0, tail_fill=7.0)
    assert t.shape == (N, geo["Qs"]) and bool((t[:, geo["Kq"]:] == 7.0).all())
    for b in range(B):
        assert torch.equal(t[:, b * geo["HWp"]:b * geo["HWp"] + H * W], dz[b].reshape(H * W, N).t())
        assert bool((t[:, b * geo["HWp"] + H * W:(b + 1) * geo["HWp"]] == 0).all())
    assert bool((t[:, B * geo["HWp"]:geo["Kq"]] == 0).all())
    m = R.xT3_padding_mask(geo)
    assert m.shape == (geo["Qs"],) and not bool(m[:(H + 2) * W].any()) and bool(m[(H + 2) * W:geo["Pimg"]].all())
    assert bool(m[B * geo["Pimg"]:].all()) and int((~m).sum()) == B * (H + 2) * W


def test_bounds_are_monotone_and_cover_the_gemm_counts():
    Sp = _rand(16, 8, seed=12).abs() + 0.1
    ref = _rand(16, 8, seed=13)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        for K in (64, 576, 4608, 6912):
            last = None
            for pieces in (1, 2, 3, 4, 8, 64):
                u = R.acc_units(K, pieces, dt)
                assert u >= 2 * K and (pieces == 1 or u >= 2 * K + pieces)
                b = R.held(ref, R.acc_bound(Sp, K, pieces, dt), dt)
                assert last is None or bool((b > last).all())
                last = b
        for pieces in (1, 2, 4):
            bs = [R.acc_bound(Sp, K, pieces, dt) for K in (64, 576, 4608)]
            assert bool((bs[0] < bs[1]).all()) and bool((bs[1] < bs[2]).all())
            assert bool((R.add_relu_grad_bound(Sp, ref, 576, pieces, dt) > bs[1]).all())
    # an even split of s pieces: _gemm_refs counts 2 K / s + s, never more than this module's 2 K + s
    assert all(2.0 * K / s + s <= R.acc_units(K, s, torch.float16) for K in (64, 4096) for s in (2, 8, 64))
    assert bool((R.held(ref, Sp, torch.float32) == Sp).all())
    assert bool((R.held(ref, Sp, torch.float16) == 0.5 * R.ulp(ref, torch.float16) + 2 * Sp).all())


def test_stats_bound_counts_tile_rows():
    P = _rand(300, 8, seed=14)
    d = P.abs() * 1e-6
    for bm in (128, 224, 256):
        bs, bq = R.stats_bound(P, d, bm)
        a = P.abs() + d
        nt = -(-300 // bm)
        ws, wq = torch.zeros(8, dtype=F64), torch.zeros(8, dtype=F64)
        for t in range(nt):
            sl = slice(t * bm, min(300, (t + 1) * bm))
            rows = sl.stop - sl.start
            ws += d[sl].sum(0) + R.units(rows) * a[sl].sum(0)
            wq += (2 * P[sl].abs() * d[sl] + d[sl] ** 2).sum(0) + R.units(rows) * (a[sl] ** 2).sum(0)
        _close(bs, ws)
        _close(bq, wq)
        b0 = R.stats_bound(P, 0.0, bm)
        assert bool((b0[0] < bs).all()) and bool((b0[1] < bq).all()) and bool((b0[0] > 0).all())
    # an f32 sum in row order stays inside the bound (d = 0: the summands are exact f32 values)
    Pf = P.to(torch.float32)
    s32, q32 = torch.zeros(8), torch.zeros(8)
    for r in range(300):
        s32 = s32 + Pf[r]
        q32 = q32 + Pf[r] * Pf[r]                                          # (two roundings: the kernel's fmaf has one)
    rs, rq = R.stats(Pf)
    bs, bq = R.stats_bound(Pf, 0.0, 300)
    assert bool(((s32.to(F64) - rs).abs() <= bs).all()) and bool(((q32.to(F64) - rq).abs() <= 2 * bq).all())
    ok = R.stats_exact_in_f32(torch.full((300, 2), 0.125, dtype=F64), 128, 0.125)
    assert bool(ok.all()) and not bool(R.stats_exact_in_f32(torch.full((300, 2), 2.0 ** 22, dtype=F64), 128, 1.0).any())
