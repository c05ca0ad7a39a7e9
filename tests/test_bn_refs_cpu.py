"""The float64 references of tests/_bn_refs.py against torch's own float64 ops and autograd (no GPU): the GPU
kernel tests (test_gpu_bn_kernels.py) are only as good as these, so they are pinned here to 1e-12 relative at the
small shapes those tests use."""
import pytest
import torch
import torch.nn.functional as F

import _bn_refs as R

F64 = torch.float64
SHAPES = [(3, 6, 10, 40), (1, 2, 2, 2048)]        # the flat elementwise shapes of the GPU tests (B, H, W, C)


def _close(a, b, tol=1e-12):
    a, b = a.detach().to(F64), b.detach().to(F64)
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("P,C", [(2, 8), (50, 1032), (513, 64), (60, 40)])
def test_batchnorm_train_and_running_stats(P, C):
    z = _rand(P, C, seed=1) * 1.5 + torch.linspace(-8, 8, C, dtype=F64)
    gamma, beta = _rand(C, seed=2) * 0.2 + 1, _rand(C, seed=3) * 0.3
    rm0, rv0 = _rand(C, seed=4), _rand(C, seed=5).abs() + 0.5
    eps, mom = 1e-5, 0.1
    rm, rv = rm0.clone(), rv0.clone()
    y = F.batch_norm(z.t().reshape(1, C, P), rm, rv, gamma, beta, True, mom, eps).reshape(C, P).t()
    ref = R.bn_train(z, gamma, beta, eps, mom, rm0, rv0)
    _close(ref["y"], y)
    _close(ref["running_mean"], rm)
    _close(ref["running_var"], rv)
    _close(z * ref["scale"] + ref["shift"], y)
    # the same statistics from the column sums (what ebc_bn_finalize is given); the variance by cancellation
    S, Q, _ = R.bn_sums(z)
    fs = R.bn_from_sums(S, Q, float(P), gamma, beta, eps, mom, rm0, rv0)
    for k in ("mean", "running_mean"):
        _close(fs[k], ref[k])
    for k in ("rstd", "scale", "shift", "running_var"):
        _close(fs[k], ref[k], 1e-10)                    # 65 * 2^-53 relative to a variance of ~2: cancellation
    # eval mode: running statistics used, nothing updated
    rm, rv = rm0.clone(), rv0.clone()
    ye = F.batch_norm(z.t().reshape(1, C, P), rm, rv, gamma, beta, False, mom, eps).reshape(C, P).t()
    ev = R.bn_eval(rm0, rv0, gamma, beta, eps)
    _close(z * ev["scale"] + ev["shift"], ye)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)


def test_batchnorm_two_rank_sums():
    """SyncBatchNorm: the sums of two row sets of different sizes added, count P1 + P2 = BatchNorm over the
    concatenation (unbiased running_var factor (P1+P2)/(P1+P2-1))."""
    C, P1, P2 = 300, 7, 12
    z1, z2 = _rand(P1, C, seed=1) + 2, _rand(P2, C, seed=2) * 2 - 1
    gamma, beta, rm0, rv0 = _rand(C, seed=3), _rand(C, seed=4), _rand(C, seed=5), _rand(C, seed=6).abs()
    S1, Q1, _ = R.bn_sums(z1)
    S2, Q2, _ = R.bn_sums(z2)
    fs = R.bn_from_sums(S1 + S2, Q1 + Q2, float(P1 + P2), gamma, beta, 1e-5, 0.1, rm0, rv0)
    z = torch.cat([z1, z2])
    rm, rv = rm0.clone(), rv0.clone()
    y = F.batch_norm(z.t().reshape(1, C, -1), rm, rv, gamma, beta, True, 0.1, 1e-5).reshape(C, -1).t()
    _close(z * fs["scale"] + fs["shift"], y, 1e-11)
    _close(fs["running_mean"], rm)
    _close(fs["running_var"], rv, 1e-11)


@pytest.mark.parametrize("stored_mask", [True, False])
@pytest.mark.parametrize("P,C", [(60, 40), (4, 2048), (50, 1032)])
def test_batchnorm_relu_backward_matches_autograd(P, C, stored_mask):
    z = (_rand(P, C, seed=1) * 1.5 + 0.3).requires_grad_(True)
    gamma = (_rand(C, seed=2) * 0.2 + 1).requires_grad_(True)
    beta = (_rand(C, seed=3) * 0.3).requires_grad_(True)
    gy = _rand(P, C, seed=4)
    eps = 1e-5
    bn = F.batch_norm(z.t().reshape(1, C, P), None, None, gamma, beta, True, 0.1, eps).reshape(C, P).t()
    y = torch.relu(bn)
    gz, gg, gb = torch.autograd.grad(y, (z, gamma, beta), gy)
    zd = z.detach()
    st = R.bn_train(zd, gamma.detach(), beta.detach(), eps)
    m = y.detach() if stored_mask else zd * st["scale"] + st["shift"]
    sg, sgx, _, _ = R.bn_bwd_sums(gy, m, zd, st["mean"], st["rstd"])
    coef = R.bn_bwd_coef(sg, sgx, float(P), gamma.detach(), st["rstd"])
    dz, g, A = R.bn_bwd_dz(gy, m, zd, st["mean"], st["rstd"], coef)
    _close(dz, gz, 1e-11)
    _close(sgx, gg, 1e-11)                              # dgamma
    _close(sg, gb)                                      # dbeta
    _close(g, gy * (y.detach() > 0))
    assert bool((A >= dz.abs() * (1 - 1e-12)).all())


def test_relu_grad_at_zero_is_zero():
    m = torch.tensor([-1.0, -0.0, 0.0, 1e-300, 2.0], dtype=F64, requires_grad=True)
    g = torch.tensor([3.0, 4.0, 5.0, 6.0, 7.0], dtype=F64)
    (ga,) = torch.autograd.grad(torch.relu(m), m, g)
    assert torch.equal(R.relu_grad(g, m.detach()), ga)
    assert torch.equal(R.relu_grad(g, m.detach()), torch.tensor([0.0, 0.0, 0.0, 6.0, 7.0], dtype=F64))
    assert torch.equal(R.relu(m.detach()), torch.relu(m.detach()))


@pytest.mark.parametrize("up", [1, 2, 3, 4])
@pytest.mark.parametrize("B,h,w,C", [(3, 6, 10, 40), (1, 2, 2, 2048), (3, 3, 5, 64), (3, 7, 7, 64), (3, 2, 10, 12)])
def test_upsample_and_adjoint(B, h, w, C, up):
    feat = _rand(B, h, w, C, seed=up).requires_grad_(True)
    t = F.interpolate(feat.permute(0, 3, 1, 2), scale_factor=up, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    out, A = R.upsample(feat.detach(), up)
    _close(out, t)
    assert bool((A >= out.abs() * (1 - 1e-12)).all())
    g = _rand(B, h * up, w * up, C, seed=9)
    (gf,) = torch.autograd.grad(t, feat, g)
    _close(R.upsample_adjoint(g, up), gf)
    # rows of the interpolation matrix sum to 1; at up = 1, 2, 4 the weights are multiples of 1/8 per axis
    M = R.upsample_matrix(h, up)
    _close(M.sum(1), torch.ones(h * up, dtype=F64))
    if up != 3:
        assert torch.equal(M * 8, (M * 8).round())


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_avgpool_and_adjoint(B, H, W, C):
    x = _rand(B, H, W, C, seed=1).requires_grad_(True)
    t = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    _close(R.avgpool2(x.detach()), t)
    g = _rand(B, H // 2, W // 2, C, seed=2)
    (gx,) = torch.autograd.grad(t, x, g)
    _close(R.avgpool2_bwd(g, H, W), gx)
    sc, sh = _rand(C, seed=3), _rand(C, seed=4)
    t2 = F.avg_pool2d(torch.relu(x.detach() * sc + sh).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    _close(R.avgpool2(R.bn_relu(x.detach(), sc, sh)), t2)


def test_layouts():
    B, H, W, C, N = 3, 6, 10, 64, 32
    Hp, Wp, HWp = H + 2, 32, 64                       # the decoder geometry of this shape (ebc_hip.h)
    Kq = 192
    x = _rand(B, H, W, C, seed=1)
    rows, inter = R.pad_nhwc(x, Hp, Wp)
    t = F.pad(x, (0, 0, 1, Wp - W - 1, 1, 1)).reshape(B * Hp * Wp, C)
    assert torch.equal(rows, t)
    assert int(inter.sum()) == B * H * W and torch.equal(rows[inter], x.reshape(-1, C))
    assert bool((rows[~inter] == 0).all())
    d = R.dzT_layout(x, HWp, Kq)
    t = torch.zeros(C, B, HWp, dtype=F64)
    t[:, :, :H * W] = x.reshape(B, H * W, C).permute(2, 0, 1)
    assert torch.equal(d, F.pad(t.reshape(C, B * HWp), (0, Kq - B * HWp)))
    w = _rand(N, C, 3, 3, seed=2)
    wk, wf = R.conv_weight_layouts(w)
    assert torch.equal(wk, w.permute(0, 2, 3, 1))
    assert torch.equal(wf, w.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9, N))
    # the flipped operand is the weight of the data-gradient convolution: conv(g, wf) = conv_transpose(g, w)
    g = _rand(1, N, 5, 7, seed=3)
    wd = wf.reshape(C, 3, 3, N).permute(0, 3, 1, 2)
    _close(F.conv2d(g, wd, padding=1), F.conv_transpose2d(g, w, padding=1))
    w1 = _rand(N, 96, seed=4)
    k1, t1 = R.weight_1x1_layouts(w1)
    assert torch.equal(k1, w1) and torch.equal(t1, w1.t())


@pytest.mark.parametrize("dt,p,tiny", [(torch.float32, 24, 2.0 ** -149), (torch.float16, 11, 2.0 ** -24),
                                      (torch.bfloat16, 8, 2.0 ** -133)])
def test_ulp(dt, p, tiny):
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, -3.0, 0.75, 0.0, 2.0 ** -20, 100.0], dtype=F64)
    u = R.ulp(x, dt)
    assert u[0] == 2.0 ** (1 - p) and u[2] == 2.0 ** (1 - p) and u[3] == 2.0 ** (2 - p) and u[4] == 2.0 ** (2 - p)
    assert u[5] == 2.0 ** (-p) and u[6] == tiny and u[8] == 2.0 ** (7 - p)
    # against the type itself: the next representable value above |x|
    xs = torch.tensor([1.0, 3.0, 0.75, 100.0], dtype=F64)
    nxt = torch.nextafter(xs.to(dt), torch.tensor(1e30, dtype=F64).to(dt)) if dt != torch.float16 else \
        torch.nextafter(xs.to(dt), torch.tensor(60000.0, dtype=dt))
    assert torch.equal(nxt.to(F64) - xs, R.ulp(xs, dt))
    assert R.rows_per_block(8) == 4096 and R.rows_per_block(192) == 168 and R.rows_per_block(1032) == 24
    assert R.rows_per_block(2048) == 16 and R.rows_per_block(4096) == 8
