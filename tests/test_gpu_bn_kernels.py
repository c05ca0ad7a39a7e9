"""The BatchNorm / pooling / upsample / weight-prep entry points of decoder.hip, one kernel at a time, against the
float64 references of tests/_bn_refs.py (themselves pinned to torch in tests/test_bn_refs_cpu.py).

Two kinds of input per kernel:

* "dyadic": every operand on a coarse binary grid (activations and gradients k/8 with |k| <= 16, means k/8 with
  |k| <= 8, rstd / scale in {1, 2}, shift / coef k/8), so that every product and every partial sum is exact in f32
  whatever the summation order or fma choice; the kernel must then reproduce the float64 reference bit for bit
  (16-bit outputs: the reference rounded once).  One missed, duplicated or misplaced element fails.
* random normal inputs, checked per element (never a norm) against bounds derived from the arithmetic:
    reductions   |sum - sum64| <= rpb * 2^-24 * sum|term| per column, rpb = the rows of one block's f32 chain
    stores       |out - ref| <= ulp_T(ref) / 2 + k * 2^-24 * A, A = the sum of the absolute values of the expression's
                 terms, k = the number of f32 operations of the kernel's expression (stated at each test)
    finalize     one f32 rounding of the float64 formula applied to the kernel's own float64 sums
  Each check prints "RATIO <kernel> <largest error / bound>" before it asserts.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _bn_refs as R
from _kernel_checks import GUARD_ROWS, SENT, _Hold, _elem, _exact, _f32, _guard_ok, _guarded, _report
from conftest import rel_l2
from ebc_amd import _lib

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
F64 = torch.float64
U = R.U32
D53 = 2.0 ** -53
EPS = float(torch.tensor(1e-5, dtype=torch.float32))       # the kernels take eps / momentum as C floats
MOM = float(torch.tensor(0.1, dtype=torch.float32))
EBC_E_ARG, EBC_E_UNSUPPORTED = -1, -3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dy(shape, kmax, seed, den=8.0):
    """k / den with integer |k| <= kmax (float64, CPU)."""
    return torch.randint(-kmax, kmax + 1, tuple(shape), generator=_gen(seed)).to(F64) / den


def _pow2(shape, seed):
    return torch.randint(0, 2, tuple(shape), generator=_gen(seed)).to(F64) + 1.0           # 1 or 2


def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=_gen(seed), dtype=F64)


hold = _Hold()


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    hold.clear()


# ----------------------------------------------------------------------------------------------- reductions
PAIRS = [(8, 2), (8, 4095), (8, 4097), (64, 511), (64, 513), (64, 1541), (192, 167), (192, 169), (192, 700),
         (1032, 50), (2048, 15), (2048, 17), (2048, 1000), (4096, 7), (4096, 9), (4096, 100)]
RED_CASES = [(C, P, "f16") for C, P in PAIRS] + [(C, P, d) for C, P in PAIRS if C in (64, 2048) for d in ("f32", "bf16")]
WS_GUARD = 256


def _workspace(P, C):
    """Exactly 16384 + ceil(P / rpb) * 8 * C bytes (first 16 KiB zero, partials NaN) followed by guard bytes."""
    rpb = R.rows_per_block(C)
    need = 16384 + -(-P // rpb) * 8 * C
    ws = torch.empty(need + WS_GUARD, dtype=torch.uint8, device="cuda")
    ws[:16384] = 0
    ws[16384:need].view(torch.float32).fill_(float("nan"))
    ws[need:] = 0xA5
    return ws, need


def _assert_exact_sums(terms, units_per_one, rpb):
    """Every term is an integer number of 1/units_per_one, and one block's rows of them sum to less than 2^24
    units: any f32 summation order of a block gives the exact partial sum (the cross-block part is f64)."""
    assert torch.equal(terms * units_per_one, (terms * units_per_one).round())
    assert rpb * float(terms.abs().max()) * units_per_one < 2 ** 24


def _workspace_ok(ws, need):
    return bool((ws[:16384] == 0).all()) and bool((ws[need:] == 0xA5).all())


def _bn_params(C, seed, dyadic):
    """gamma, beta, running_mean, running_var (f32 device tensors)."""
    if dyadic:
        return (_f32(_pow2((C,), seed)), _f32(_dy((C,), 16, seed + 1)), _f32(_dy((C,), 8, seed + 2)),
                _f32(_dy((C,), 8, seed + 3).abs() + 0.5))
    return (_f32(_randn((C,), seed) * 0.2 + 1), _f32(_randn((C,), seed + 1) * 0.3), _f32(_randn((C,), seed + 2)),
            _f32(_randn((C,), seed + 3).abs() + 0.5))


def _fwd_outs(C):
    return [torch.full((C + GUARD_ROWS,), SENT, device="cuda") for _ in range(4)]


def _check_fwd_finalize(tag, outs, S, Q, count, gamma, beta, eps, mom, rm0, rv0, rm, rv):
    """mean, rstd, scale, shift (and the running statistics) against the float64 formula applied to the float64 sums
    S, Q: one f32 rounding (relative 2^-24) for the directly cast values, scale = the f32 product gamma * rstd
    exactly, shift within 4 * 2^-24 * (|beta| + |mean * scale|).  The float64 formula's own error is added: the
    variance Q/count - mean^2 cancels, 4 * 2^-53 * (Q/count + mean^2) whichever way it is evaluated (fma or not),
    which rstd = (var + eps)^-1/2 sees as half of its relative size."""
    C = S.numel()
    mean, rstd, scale, shift = (o[:C].to(F64).cpu() for o in outs)
    assert all(_guard_ok(o, C) for o in outs)
    g64, b64 = gamma.to(F64).cpu(), beta.to(F64).cpu()
    ref = R.bn_from_sums(S, Q, count, g64, b64, eps, mom, rm0, rv0)
    dvar = 4 * D53 * (Q / count + ref["mean"] ** 2)
    drel = 0.5 * dvar / (ref["var"] + eps) + 8 * D53
    _report(f"{tag}.mean", (mean - ref["mean"]).abs(), U * ref["mean"].abs() + 2.0 ** -149)
    _report(f"{tag}.rstd", (rstd - ref["rstd"]).abs(), ref["rstd"] * (U + drel))
    assert torch.equal(scale, (g64 * rstd).to(torch.float32).to(F64))
    ms = (ref["mean"] * ref["scale"]).abs()
    _report(f"{tag}.shift", (shift - ref["shift"]).abs(), 4 * U * (b64.abs() + ms) + ms * drel + 2.0 ** -149)
    if rm0 is not None:
        _report(f"{tag}.running_mean", (rm.to(F64).cpu() - ref["running_mean"]).abs(),
                U * ref["running_mean"].abs() + 8 * D53 * ((1 - mom) * rm0.abs() + mom * ref["mean"].abs()) + 2.0 ** -149)
        _report(f"{tag}.running_var", (rv.to(F64).cpu() - ref["running_var"]).abs(),
                (U + 8 * D53) * ref["running_var"].abs() + mom * dvar * count / (count - 1.0) + 2.0 ** -149)


@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("C,P,dname", RED_CASES)
def test_bn_stats(C, P, dname, kind):
    """ebc_bn_stats and ebc_bn_stats_finalize: the column sums of z and z^2 (f64) and the statistics from them.
    Fused and unfused forms must agree bit for bit in every output; the workspace is sized exactly."""
    dt = DT[dname]
    L = _lib.lib()
    rpb = R.rows_per_block(C)
    if kind == "dyadic":
        z = _dy((P, C), 16, 1).to(dt)
        # exactness: a block's partial sums are integers in units of 1/8 (sum) and 1/64 (squares), below 2^24
        _assert_exact_sums(z.to(F64), 8, rpb)
        _assert_exact_sums(z.to(F64) ** 2, 64, rpb)
    else:
        z = ((_randn((P, C), 1) + torch.linspace(-8, 8, C, dtype=F64)) * 1.5).to(dt)    # mean up to 8 sigma
    z64 = z.to(F64)
    zd = z.cuda()
    S, Q, SA = R.bn_sums(z64)
    gamma, beta, rm0, rv0 = _bn_params(C, 10, kind == "dyadic")
    code = _lib.dtype_code(dt)

    # unfused: ebc_bn_stats, then ebc_bn_finalize
    ws, need = _workspace(P, C)
    colsum = torch.full((2 * C + GUARD_ROWS,), SENT, dtype=F64, device="cuda")
    outs = _fwd_outs(C)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.tensor([41], dtype=torch.int64, device="cuda")
    _lib.check(L.ebc_bn_stats(code, _lib.ptr(zd), _lib.ptr(colsum), _lib.ptr(ws), need, P, C, _lib.stream()), "stats")
    _lib.check(L.ebc_bn_finalize(_lib.ptr(colsum), float(P), EPS, MOM, _lib.ptr(gamma), _lib.ptr(beta),
                                 *[_lib.ptr(o) for o in outs], _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt), C,
                                 _lib.stream()), "finalize")
    assert _workspace_ok(ws, need) and _guard_ok(colsum, 2 * C)
    got = colsum[:2 * C].cpu()
    if kind == "dyadic":
        assert torch.equal(got, torch.cat([S, Q])), int((got != torch.cat([S, Q])).sum())
    else:
        _report("bn_stats.sum", (got[:C] - S).abs(), rpb * U * SA)
        _report("bn_stats.sumsq", (got[C:] - Q).abs(), rpb * U * Q)
    assert int(nbt) == 42
    _check_fwd_finalize("bn_finalize", outs, got[:C], got[C:], float(P), gamma, beta, EPS, MOM, rm0.to(F64).cpu(),
                        rv0.to(F64).cpu(), rm, rv)

    # fused: ebc_bn_stats_finalize, bitwise equal in every output
    ws2, _ = _workspace(P, C)
    colsum2 = torch.full((2 * C + GUARD_ROWS,), SENT, dtype=F64, device="cuda")
    outs2 = _fwd_outs(C)
    rm2, rv2 = rm0.clone(), rv0.clone()
    nbt2 = torch.tensor([41], dtype=torch.int64, device="cuda")
    _lib.check(L.ebc_bn_stats_finalize(code, _lib.ptr(zd), _lib.ptr(ws2), need, P, C, EPS, MOM, _lib.ptr(gamma),
                                       _lib.ptr(beta), *[_lib.ptr(o) for o in outs2], _lib.ptr(rm2), _lib.ptr(rv2),
                                       _lib.ptr(colsum2), _lib.ptr(nbt2), _lib.stream()), "stats_finalize")
    assert _workspace_ok(ws2, need)
    assert torch.equal(colsum2, colsum)
    for a, b in zip(outs2 + [rm2, rv2, nbt2], outs + [rm, rv, nbt]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("form", ["mask_y", "recomputed"])
@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("C,P,dname", RED_CASES)
def test_bn_bwd_reduce(C, P, dname, kind, form):
    """ebc_bn_bwd_reduce and ebc_bn_bwd_reduce_finalize: sum g and sum g * xhat (f64), g = gy * relu'(.), with the
    ReLU mask from the stored output or recomputed as fma(z, scale, shift); relu'(0) = 0.  (The recomputed mask is
    one correctly rounded fma, so its sign is the exact expression's: the float64 reference masks the same
    elements.)"""
    dt = DT[dname]
    L = _lib.lib()
    rpb = R.rows_per_block(C)
    if kind == "dyadic":
        gy, z = _dy((P, C), 16, 1).to(dt), _dy((P, C), 16, 2).to(dt)
        mean, rstd = _dy((C,), 8, 3), _pow2((C,), 4)
        scale = _pow2((C,), 5)
        shift = scale * _dy((C,), 8, 6)                      # k/8, and z*scale + shift = 0 for z = -shift/scale
        gamma = _pow2((C,), 7)
        z[0] = (-shift / scale).to(dt)                       # a whole row with z*scale + shift = 0 exactly
        my = R.relu(_dy((P, C), 16, 8)).to(dt)               # a stored ReLU output: about half exact zeros
    else:
        gy = _randn((P, C), 1).to(dt)
        z = ((_randn((P, C), 2) + torch.linspace(-2, 2, C, dtype=F64)) * 1.5).to(dt)
        gamma = _randn((C,), 7) * 0.2 + 1
        st = R.bn_train(z.to(F64), gamma, _randn((C,), 9) * 0.3, EPS)
        mean, rstd, scale, shift = (st[k].to(torch.float32).to(F64) for k in ("mean", "rstd", "scale", "shift"))
        my = R.bn_relu(z, scale, shift).to(dt)
    m = my.to(F64) if form == "mask_y" else z.to(F64) * scale + shift
    if kind == "dyadic":
        assert int((m == 0).sum()) > 0                       # relu'(0) = 0 is exercised
        # exactness: g in units of 1/8, g * xhat in units of 1/64, a block's sums below 2^24 units
        g64 = R.relu_grad(gy.to(F64), m)
        _assert_exact_sums(g64, 8, rpb)
        _assert_exact_sums(g64 * ((z.to(F64) - mean) * rstd), 64, rpb)
    sg, sgx, ag, agx = R.bn_bwd_sums(gy, m, z, mean, rstd)
    code = _lib.dtype_code(dt)
    gyd, zd, myd = gy.cuda(), z.cuda(), (my.cuda() if form == "mask_y" else None)
    mean_d, rstd_d, scale_d, shift_d, gamma_d = (_f32(t) for t in (mean, rstd, scale, shift, gamma))

    ws, need = _workspace(P, C)
    sums = torch.full((2 * C + GUARD_ROWS,), SENT, dtype=F64, device="cuda")
    _lib.check(L.ebc_bn_bwd_reduce(code, _lib.ptr(gyd), _lib.ptr(myd), _lib.ptr(zd), _lib.ptr(mean_d), _lib.ptr(rstd_d),
                                   _lib.ptr(scale_d), _lib.ptr(shift_d), _lib.ptr(sums), _lib.ptr(ws), need, P, C,
                                   _lib.stream()), "bwd_reduce")
    assert _workspace_ok(ws, need) and _guard_ok(sums, 2 * C)
    got = sums[:2 * C].cpu()
    if kind == "dyadic":
        assert torch.equal(got, torch.cat([sg, sgx])), int((got != torch.cat([sg, sgx])).sum())
    else:
        _report("bn_bwd_reduce.sum_g", (got[:C] - sg).abs(), rpb * U * ag + 2.0 ** -149)
        _report("bn_bwd_reduce.sum_gx", (got[C:] - sgx).abs(), rpb * U * agx + 2.0 ** -149)
    dg, db = torch.full((C + GUARD_ROWS,), SENT, device="cuda"), torch.full((C + GUARD_ROWS,), SENT, device="cuda")
    coef = torch.full((3 * C + GUARD_ROWS,), SENT, device="cuda")
    _lib.check(L.ebc_bn_bwd_finalize(_lib.ptr(sums), float(P), _lib.ptr(gamma_d), _lib.ptr(rstd_d), _lib.ptr(dg),
                                     _lib.ptr(db), _lib.ptr(coef), C, _lib.stream()), "bwd_finalize")
    _check_bwd_finalize("bn_bwd_finalize", got, float(P), gamma_d, rstd_d, dg, db, coef)

    ws2, _ = _workspace(P, C)
    dg2, db2, coef2 = torch.full_like(dg, SENT), torch.full_like(db, SENT), torch.full_like(coef, SENT)
    _lib.check(L.ebc_bn_bwd_reduce_finalize(code, _lib.ptr(gyd), _lib.ptr(myd), _lib.ptr(zd), _lib.ptr(mean_d),
                                            _lib.ptr(rstd_d), _lib.ptr(scale_d), _lib.ptr(shift_d), _lib.ptr(gamma_d),
                                            _lib.ptr(dg2), _lib.ptr(db2), _lib.ptr(coef2), _lib.ptr(ws2), need, P, C,
                                            _lib.stream()), "bwd_reduce_finalize")
    assert _workspace_ok(ws2, need)
    assert torch.equal(dg2, dg) and torch.equal(db2, db) and torch.equal(coef2, coef)


def _check_bwd_finalize(tag, sums, count, gamma, rstd, dg, db, coef):
    """dgamma = (float) sum g*xhat, dbeta = (float) sum g: direct casts, exact.  coef = [gamma*rstd (one f32
    product), sum g / count, sum g*xhat / count (one f64 division, one f32 rounding)]."""
    C = gamma.numel()
    sg, sgx = sums[:C], sums[C:2 * C]
    if dg is not None:
        assert torch.equal(dg[:C].cpu(), sgx.to(torch.float32)) and _guard_ok(dg, C)
        assert torch.equal(db[:C].cpu(), sg.to(torch.float32)) and _guard_ok(db, C)
    assert _guard_ok(coef, 3 * C)
    c = coef[:3 * C].to(F64).cpu().view(3, C)
    ref = R.bn_bwd_coef(sg, sgx, count, gamma.cpu(), rstd.cpu())
    assert torch.equal(c[0], ref[0].to(torch.float32).to(F64))
    _report(f"{tag}.coef1", (c[1] - ref[1]).abs(), (U + 4 * D53) * ref[1].abs() + 2.0 ** -149)
    _report(f"{tag}.coef2", (c[2] - ref[2]).abs(), (U + 4 * D53) * ref[2].abs() + 2.0 ** -149)


def test_conv3x3_fwd_bn_equals_unfused():
    """ebc_conv3x3_fwd_bn = ebc_conv3x3_fwd(colsum) + ebc_bn_finalize, bit for bit in every output."""
    L = _lib.lib()
    B, H, W, C, N = 1, 8, 8, 64, 64
    x = torch.randn(B, C, H, W, generator=_gen(3))
    wt = torch.randn(N, C, 3, 3, generator=_gen(4)) / 24
    geo = (ctypes.c_long * 6)()
    _lib.check(L.ebc_dec_geometry(_lib.EBC_F16, B, H, W, C, geo), "geo")
    Hp, Wp, Q = geo[0], geo[1], geo[4]
    xpad, _ = R.pad_nhwc(x.permute(0, 2, 3, 1).contiguous(), Hp, Wp)
    xpad = xpad.half().cuda()
    wk = R.conv_weight_layouts(wt)[0].half().contiguous().cuda()
    gamma, beta, rm0, rv0 = _bn_params(N, 20, False)
    wsb = L.ebc_dec_workspace_bytes(_lib.EBC_F16, B, H, W, C, N)
    res = []
    for fused in (False, True):
        ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
        out = torch.full((B * H * W + GUARD_ROWS, N), SENT, dtype=torch.float16, device="cuda")
        colsum = torch.full((2 * N + GUARD_ROWS,), SENT, dtype=F64, device="cuda")
        outs = _fwd_outs(N)
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.tensor([5], dtype=torch.int64, device="cuda")
        if fused:
            _lib.check(L.ebc_conv3x3_fwd_bn(_lib.EBC_F16, _lib.ptr(xpad), _lib.ptr(wk), _lib.ptr(out), _lib.ptr(ws), wsb,
                                            B, H, W, C, N, EPS, MOM, _lib.ptr(gamma), _lib.ptr(beta),
                                            *[_lib.ptr(o) for o in outs], _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt),
                                            _lib.ptr(colsum), _lib.stream()), "conv_bn")
        else:
            _lib.check(L.ebc_conv3x3_fwd(_lib.EBC_F16, _lib.ptr(xpad), _lib.ptr(wk), _lib.ptr(out), _lib.ptr(colsum), None,
                                         None, _lib.ptr(ws), wsb, B, H, W, C, N, _lib.stream()), "conv")
            _lib.check(L.ebc_bn_finalize(_lib.ptr(colsum), float(B * H * W), EPS, MOM, _lib.ptr(gamma), _lib.ptr(beta),
                                         *[_lib.ptr(o) for o in outs], _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt), N,
                                         _lib.stream()), "finalize")
        res.append([out, colsum] + outs + [rm, rv, nbt])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    out, colsum, nbt = res[0][0], res[0][1], res[0][-1]
    assert _guard_ok(out, B * H * W) and _guard_ok(colsum, 2 * N) and int(nbt) == 6
    ref = F.conv2d(x.half().double(), wt.half().double(), padding=1).permute(0, 2, 3, 1).reshape(-1, N)
    assert rel_l2(out[:B * H * W], ref) < 2e-3
    # the statistics are those of the f32 accumulators: within the f16 rounding of the stored outputs
    zs = out[:B * H * W].to(F64).cpu()
    assert bool(((colsum[:N].cpu() - zs.sum(0)).abs() <= 2.0 ** -11 * zs.abs().sum(0)).all())
    _check_fwd_finalize("conv3x3_fwd_bn", res[1][2:6], colsum[:N].cpu(), colsum[N:2 * N].cpu(), float(B * H * W), gamma,
                        beta, EPS, MOM, rm0.to(F64).cpu(), rv0.to(F64).cpu(), res[1][6], res[1][7])


# ----------------------------------------------------------------------------------------------- finalize
def _finalize(L, colsum, count, eps, mom, gamma, beta, rm, rv, nbt, C):
    outs = _fwd_outs(C)
    _lib.check(L.ebc_bn_finalize(_lib.ptr(colsum), count, eps, mom, _lib.ptr(gamma), _lib.ptr(beta),
                                 *[_lib.ptr(o) for o in outs], _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt), C,
                                 _lib.stream()), "finalize")
    return outs


@pytest.mark.parametrize("C", [8, 300, 768])
def test_bn_finalize_dyadic(C):
    """Sums built so that every statistic is a short binary fraction: count 5 (unbiased factor 5/4), mean k/8,
    variance 1 or 1/4 with eps = 0 (rstd 1 or 2), momentum 1/2.  mean, rstd, scale, shift, running_mean and
    running_var (with its count / (count - 1)) must come out exact; the device count (count = -1, the value at
    colsum[2C]) gives the same bits as the host count."""
    L = _lib.lib()
    count, mom = 5.0, 0.5
    m, v = _dy((C,), 8, 1), 1.0 / _pow2((C,), 2) ** 2
    colsum = torch.cat([count * m, count * (v + m * m), torch.tensor([count], dtype=F64)])
    gamma, beta, rm0, rv0 = _bn_params(C, 3, True)
    ref = R.bn_from_sums(colsum[:C], colsum[C:2 * C], count, gamma.cpu(), beta.cpu(), 0.0, mom, rm0.to(F64).cpu(),
                         rv0.to(F64).cpu())
    assert torch.equal(ref["mean"], m) and torch.equal(ref["var"], v)
    assert torch.equal(ref["running_var"], 0.5 * rv0.to(F64).cpu() + 0.5 * v * 1.25)
    cs = colsum.cuda()
    res = []
    for cnt in (count, -1.0):
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.tensor([0], dtype=torch.int64, device="cuda")
        outs = _finalize(L, cs, cnt, 0.0, mom, gamma, beta, rm, rv, nbt, C)
        for o, k in zip(outs + [rm, rv], ("mean", "rstd", "scale", "shift", "running_mean", "running_var")):
            _exact(o[:C], ref[k], torch.float32)
        assert all(_guard_ok(o, C) for o in outs) and int(nbt) == 1
        res.append(outs + [rm, rv])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("C", [8, 300, 768])
def test_bn_finalize_two_ranks_dyadic(C):
    """SyncBatchNorm with ranks of 2 and 3 rows: the two ranks' sums added, the count 2 + 3 on the device; the result
    is BatchNorm2d over the 5 rows together (variance as the mean squared deviation, running_var * 5/4).  The rows
    are mean + a permutation of s * (1.5, -1.5, 0.5, -0.5, 0), s in {1, 1/2}: variance s^2 exactly."""
    L = _lib.lib()
    mom = 0.5
    m, s = _dy((C,), 8, 1), 1.0 / _pow2((C,), 2)
    d = torch.tensor([1.5, -1.5, 0.5, -0.5, 0.0], dtype=F64)
    perm = torch.stack([torch.randperm(5, generator=_gen(10 + c)) for c in range(C)], 1)        # [5][C]
    z = m + d[perm] * s
    S1, Q1, _ = R.bn_sums(z[:2])
    S2, Q2, _ = R.bn_sums(z[2:])
    colsum = torch.cat([S1 + S2, Q1 + Q2, torch.tensor([5.0], dtype=F64)]).cuda()
    gamma, beta, rm0, rv0 = _bn_params(C, 3, True)
    ref = R.bn_train(z, gamma.cpu(), beta.cpu(), 0.0, mom, rm0.cpu(), rv0.cpu())
    assert torch.equal(ref["var"], s * s)
    rm, rv = rm0.clone(), rv0.clone()
    outs = _finalize(L, colsum, -1.0, 0.0, mom, gamma, beta, rm, rv, None, C)
    for o, k in zip(outs + [rm, rv], ("mean", "rstd", "scale", "shift", "running_mean", "running_var")):
        _exact(o[:C], ref[k], torch.float32)


@pytest.mark.parametrize("C", [8, 300, 768])
def test_bn_finalize_random(C):
    """Training (host and device count, bitwise equal), two ranks of different sizes against BatchNorm over the
    concatenation, and eval mode (colsum = NULL: the running statistics are read, nothing is updated)."""
    L = _lib.lib()
    P1, P2 = 23, 14
    z1 = (_randn((P1, C), 1) + torch.linspace(-8, 8, C, dtype=F64)) * 1.5
    z2 = (_randn((P2, C), 2) * 0.5 + torch.linspace(-8, 8, C, dtype=F64)) * 1.5 + 1
    S1, Q1, _ = R.bn_sums(z1)
    S2, Q2, _ = R.bn_sums(z2)
    gamma, beta, rm0, rv0 = _bn_params(C, 3, False)
    rm64, rv64 = rm0.to(F64).cpu(), rv0.to(F64).cpu()
    # one rank, host count and device count
    cs = torch.cat([S1, Q1, torch.tensor([float(P1)], dtype=F64)]).cuda()
    res = []
    for cnt in (float(P1), -1.0):
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.tensor([7], dtype=torch.int64, device="cuda")
        outs = _finalize(L, cs, cnt, EPS, MOM, gamma, beta, rm, rv, nbt, C)
        assert int(nbt) == 8
        res.append(outs + [rm, rv])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    _check_fwd_finalize("bn_finalize", res[0][:4], S1, Q1, float(P1), gamma, beta, EPS, MOM, rm64, rv64, res[0][4],
                        res[0][5])
    # two ranks: sums added, device count P1 + P2, against BatchNorm over the concatenation (mean squared deviation;
    # the sums' cancellation, 4 * 2^-53 * (Q/count + mean^2), is what _check_fwd_finalize allows for)
    cs = torch.cat([S1 + S2, Q1 + Q2, torch.tensor([float(P1 + P2)], dtype=F64)]).cuda()
    rm, rv = rm0.clone(), rv0.clone()
    outs = _finalize(L, cs, -1.0, EPS, MOM, gamma, beta, rm, rv, None, C)
    _check_fwd_finalize("bn_finalize", outs, S1 + S2, Q1 + Q2, float(P1 + P2), gamma, beta, EPS, MOM, rm64, rv64, rm, rv)
    ref = R.bn_train(torch.cat([z1, z2]), gamma.cpu(), beta.cpu(), EPS, MOM, rm64, rv64)
    # the reference's other route to the variance: 4 * 2^-53 * (Q/count + mean^2) / var < 2^-40 relative here
    cat_slack = 1.0 + 2.0 ** -16
    for o, k in zip(outs[:2] + [rm, rv], ("mean", "rstd", "running_mean", "running_var")):
        _report(f"bn_finalize.two_ranks.{k}", (o[:C].to(F64).cpu() - ref[k]).abs(), U * cat_slack * ref[k].abs() + 2.0 ** -149)
    # eval: no sums; the counter is only advanced through a non-NULL pointer, which eval callers do not pass
    rm, rv = rm0.clone(), rv0.clone()
    outs = _fwd_outs(C)
    _lib.check(L.ebc_bn_finalize(None, 0.0, EPS, MOM, _lib.ptr(gamma), _lib.ptr(beta), *[_lib.ptr(o) for o in outs],
                                 _lib.ptr(rm), _lib.ptr(rv), None, C, _lib.stream()), "finalize(eval)")
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and all(_guard_ok(o, C) for o in outs)
    ev = R.bn_eval(rm64, rv64, gamma.cpu(), beta.cpu(), EPS)
    mean, rstd, scale, shift = (o[:C].to(F64).cpu() for o in outs)
    assert torch.equal(mean, rm64)
    _report("bn_finalize.eval.rstd", (rstd - ev["rstd"]).abs(), (U + 8 * D53) * ev["rstd"])
    assert torch.equal(scale, (gamma.to(F64).cpu() * rstd).to(torch.float32).to(F64))
    _report("bn_finalize.eval.shift", (shift - ev["shift"]).abs(),
            4 * U * (beta.to(F64).cpu().abs() + (ev["mean"] * ev["scale"]).abs()) + 2.0 ** -149)


@pytest.mark.parametrize("C", [8, 300, 768])
def test_bn_bwd_finalize(C):
    """Host count, device count at sums[2C] (bitwise equal), and dgamma / dbeta = NULL (coef unchanged)."""
    L = _lib.lib()
    count = 37.0
    sums = torch.cat([_randn((2 * C,), 1) * 40, torch.tensor([count], dtype=F64)])
    gamma, rstd = _f32(_randn((C,), 2) * 0.2 + 1), _f32(_randn((C,), 3).abs() + 0.3)
    sd = sums.cuda()
    res = []
    for cnt, with_grads in ((count, True), (-1.0, True), (-1.0, False)):
        dg, db = torch.full((C + GUARD_ROWS,), SENT, device="cuda"), torch.full((C + GUARD_ROWS,), SENT, device="cuda")
        coef = torch.full((3 * C + GUARD_ROWS,), SENT, device="cuda")
        _lib.check(L.ebc_bn_bwd_finalize(_lib.ptr(sd), cnt, _lib.ptr(gamma), _lib.ptr(rstd),
                                         _lib.ptr(dg) if with_grads else None, _lib.ptr(db) if with_grads else None,
                                         _lib.ptr(coef), C, _lib.stream()), "bwd_finalize")
        _check_bwd_finalize("bn_bwd_finalize", sums[:2 * C], count, gamma, rstd, dg if with_grads else None,
                            db if with_grads else None, coef)
        if not with_grads:
            assert bool((dg == SENT).all()) and bool((db == SENT).all())
        res.append((dg, db, coef))
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    assert torch.equal(res[2][2], res[0][2])


# ----------------------------------------------------------------------------------------------- flat elementwise
FLAT = [(3, 6, 10, 40), (1, 2, 2, 2048)]          # non-square, P*C/8 no multiple of 256; one block row of 2048


def _acts(kind, shape, seed, dt, kmax=16):
    return (_dy(shape, kmax, seed) if kind == "dyadic" else _randn(shape, seed) * 1.5).to(dt)


def _affine(kind, C, seed):
    """per-channel scale, shift as f64 values that are exact f32."""
    if kind == "dyadic":
        sc = _pow2((C,), seed)
        return sc, sc * _dy((C,), 8, seed + 1)
    return ((_randn((C,), seed) * 0.3 + 1).to(torch.float32).to(F64), (_randn((C,), seed + 1) * 0.5).to(torch.float32).to(F64))


def _store_check(name, kind, out, rows, ref, A, k, dt, extra=None):
    assert _guard_ok(out, rows)
    if kind == "dyadic":
        _exact(out[:rows], ref, dt)
    else:
        _elem(name, out[:rows], ref, A, k, dt, extra)


@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,H,W,C", FLAT)
def test_bn_relu_and_add_relu_flat(B, H, W, C, dname, kind):
    """ebc_bn_relu: out = max(fma(z, scale, shift), 0), k = 1.  ebc_bn_add_relu_flat: max(fma(z, scale, shift) + idn,
    0) with idn = fma(idt, iscale, ishift) (k = 3: two fma, one add) or idt itself (k = 2)."""
    dt, L, P = DT[dname], _lib.lib(), B * H * W
    code = _lib.dtype_code(dt)
    z, idt = _acts(kind, (P, C), 1, dt), _acts(kind, (P, C), 2, dt)
    (sc, sh), (isc, ish) = _affine(kind, C, 3), _affine(kind, C, 5)
    zd, idd, scd, shd, iscd, ishd = z.cuda(), idt.cuda(), _f32(sc), _f32(sh), _f32(isc), _f32(ish)
    z64, i64 = z.to(F64), idt.to(F64)
    out = _guarded(P, C, dt)
    _lib.check(L.ebc_bn_relu(code, _lib.ptr(zd), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(out), P, C, _lib.stream()), "bn_relu")
    if kind == "dyadic":
        assert int((z64 * sc + sh == 0).sum()) > 0
    _store_check("bn_relu", kind, out, P, R.bn_relu(z64, sc, sh), (z64 * sc).abs() + sh.abs(), 1, dt)
    for with_affine in (True, False):
        out = _guarded(P, C, dt)
        _lib.check(L.ebc_bn_add_relu_flat(code, _lib.ptr(zd), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(idd),
                                          _lib.ptr(iscd) if with_affine else None, _lib.ptr(ishd) if with_affine else None,
                                          _lib.ptr(out), P, C, _lib.stream()), "bn_add_relu_flat")
        idn = i64 * isc + ish if with_affine else i64
        A = (z64 * sc).abs() + sh.abs() + ((i64 * isc).abs() + ish.abs() if with_affine else i64.abs())
        _store_check("bn_add_relu_flat", kind, out, P, R.relu(z64 * sc + sh + idn), A, 3 if with_affine else 2, dt)


def _bwd_apply_inputs(kind, P, C, dt, form):
    gy, z = _acts(kind, (P, C), 1, dt), _acts(kind, (P, C), 2, dt)
    if kind == "dyadic":
        mean, rstd = _dy((C,), 8, 3), _pow2((C,), 4)
        sc, sh = _affine(kind, C, 5)
        coef = torch.stack([_pow2((C,), 7), _dy((C,), 8, 8), _dy((C,), 8, 9)])
        z[0] = (-sh / sc).to(dt)                             # a whole row with z*scale + shift = 0 exactly
        my = R.relu(_dy((P, C), 16, 10)).to(dt)
    else:
        gamma = _randn((C,), 7) * 0.2 + 1
        st = R.bn_train(z.to(F64), gamma, _randn((C,), 9) * 0.3, EPS)
        mean, rstd, sc, sh = (st[k].to(torch.float32).to(F64) for k in ("mean", "rstd", "scale", "shift"))
        my = R.bn_relu(z, sc, sh).to(dt)
        m0 = my.to(F64) if form == "mask_y" else z.to(F64) * sc + sh
        sg, sgx, _, _ = R.bn_bwd_sums(gy, m0, z, mean, rstd)
        coef = R.bn_bwd_coef(sg, sgx, float(P), gamma, rstd).to(torch.float32).to(F64)
    m = my.to(F64) if form == "mask_y" else z.to(F64) * sc + sh
    if kind == "dyadic":
        assert int((m == 0).sum()) > 0
    return gy, z, my, mean, rstd, sc, sh, coef, m


@pytest.mark.parametrize("gmask", [True, False])
@pytest.mark.parametrize("form", ["mask_y", "recomputed"])
@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,H,W,C", FLAT)
def test_bn_bwd_apply_flat(B, H, W, C, dname, kind, form, gmask):
    """dz = k0 * (g - k1 - (z - mean) * rstd * k2): k = 6 f32 operations (two subtractions and two products for
    xhat * k2, the subtraction from g - k1, the product with k0); gmask = g exactly."""
    dt, L, P = DT[dname], _lib.lib(), B * H * W
    gy, z, my, mean, rstd, sc, sh, coef, m = _bwd_apply_inputs(kind, P, C, dt, form)
    dz = _guarded(P, C, dt)
    gm = _guarded(P, C, torch.float32) if gmask else None
    _lib.check(L.ebc_bn_bwd_apply_flat(_lib.dtype_code(dt), hold(gy), hold(my) if form == "mask_y" else None,
                                       hold(z), hold(mean, True), hold(rstd, True), hold(sc, True),
                                       hold(sh, True), hold(coef, True), _lib.ptr(dz), _lib.ptr(gm), P, C,
                                       _lib.stream()), "bwd_apply_flat")
    ref, g, A = R.bn_bwd_dz(gy, m, z, mean, rstd, coef)
    _store_check("bn_bwd_apply_flat", kind, dz, P, ref, A, 6, dt)
    if gmask:
        assert _guard_ok(gm, P) and torch.equal(gm[:P].cpu().to(F64), g)


def _feat(kind, shape, seed):
    return (_dy(shape, 16, seed) if kind == "dyadic" else _randn(shape, seed) * 1.5).to(torch.float32)


def _upsample_extra(feat64, up, B, H, W):
    """The tap positions are computed in f32 as scale * (o + 0.5) - 0.5 with scale = (float)(1 / up): exact for
    up = 1, 2, 4; for other factors three roundings, |d src| <= 3 * 2^-24 * n along an axis of n cells, and the
    interpolant is continuous and piecewise linear in src with slope at most 2 * max|feat| of the channel."""
    if up in (1, 2, 4):
        return None
    h, w = feat64.shape[1:3]
    fmax = feat64.abs().amax(dim=(1, 2), keepdim=True)               # [B][1][1][C]
    return (3 * U * (h + w) * 2 * fmax).expand(B, H, W, feat64.shape[3])


# thirds are no binary fractions: up = 3 runs with the random inputs only
@pytest.mark.parametrize("up,kind", [(u, k) for u in (1, 2, 3, 4) for k in ("dyadic", "random") if (u, k) != (3, "dyadic")])
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,h,w,C", FLAT)
def test_dec_upsample(B, h, w, C, dname, up, kind):
    """ebc_dec_upsample (unpadded rows), any integer factor: ly0*(lx0*a + lx1*b) + ly1*(lx0*c + lx1*d) with
    l0 = 1 - l1 per axis: k = 8 f32 operations when every product before a sum is fused (the two 1 - l, two products
    and two fma inside, one product and one fma outside)."""
    dt, L = DT[dname], _lib.lib()
    H, W = h * up, w * up
    feat = _feat(kind, (B, h, w, C), 1)
    out = _guarded(B * H * W, C, dt)
    _lib.check(L.ebc_dec_upsample(_lib.dtype_code(dt), hold(feat), _lib.ptr(out), B, h, w, C, up, _lib.stream()),
               "upsample")
    ref, A = R.upsample(feat, up)
    _store_check("dec_upsample", kind, out, B * H * W, ref.reshape(-1, C), A.reshape(-1, C), 8, dt,
                 None if kind == "dyadic" or up != 3 else _upsample_extra(feat.to(F64), up, B, H, W).reshape(-1, C))


@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,H,W,C", FLAT)
def test_avgpools(B, H, W, C, dname, kind):
    """ebc_bn_relu_avgpool: (((a + b) + c) + d) / 4 of four max(fma, 0): k = 7 (four fma, three sums; / 4 is exact).
    ebc_avgpool2: k = 3.  ebc_avgpool2_bwd: g * 0.25, exact (k = 0), T -> T and f32 -> T."""
    dt, L = DT[dname], _lib.lib()
    code = _lib.dtype_code(dt)
    Po = B * (H // 2) * (W // 2)
    z = _acts(kind, (B, H, W, C), 1, dt)
    sc, sh = _affine(kind, C, 3)
    z64 = z.to(F64)
    out = _guarded(Po, C, dt)
    _lib.check(L.ebc_bn_relu_avgpool(code, hold(z), hold(sc, True), hold(sh, True), _lib.ptr(out), B, H, W,
                                     C, _lib.stream()), "bn_relu_avgpool")
    _store_check("bn_relu_avgpool", kind, out, Po, R.avgpool2(R.bn_relu(z64, sc, sh)).reshape(-1, C),
                 R.avgpool2((z64 * sc).abs() + sh.abs()).reshape(-1, C), 7, dt)
    out = _guarded(Po, C, dt)
    _lib.check(L.ebc_avgpool2(code, code, hold(z), _lib.ptr(out), B, H, W, C, _lib.stream()), "avgpool2")
    _store_check("avgpool2", kind, out, Po, R.avgpool2(z64).reshape(-1, C), R.avgpool2(z64.abs()).reshape(-1, C), 3, dt)
    for src_dt in (dt, torch.float32):
        g = _acts(kind, (B, H // 2, W // 2, C), 5, src_dt)
        gx = _guarded(B * H * W, C, dt)
        _lib.check(L.ebc_avgpool2_bwd(_lib.dtype_code(src_dt), code, hold(g), _lib.ptr(gx), B, H, W, C,
                                      _lib.stream()), "avgpool2_bwd")
        ref = R.avgpool2_bwd(g, H, W).reshape(-1, C)
        assert _guard_ok(gx, B * H * W)
        assert torch.equal(gx[:B * H * W].cpu(), ref.to(torch.float32).to(dt))      # g / 4 is exact in f32: one rounding


# ----------------------------------------------------------------------------------------------- padded / row grid
PADDED = [(3, 5, 2), (7, 7, 1), (2, 10, 4)]       # (h, w, up): W + 2 < 32; H*W < 64 and no multiple of 8; Wp = 48
PB = 3                                            # B * Hp no multiple of 8: the XCD remap's remainder path


def _geometry(L, code, B, H, W, C):
    geo = (ctypes.c_long * 6)()
    _lib.check(L.ebc_dec_geometry(code, B, H, W, C, geo), "geo")
    Hp, Wp, HWp, Kq, Q, Qs = (int(v) for v in geo)
    assert Hp == H + 2 and Wp >= W + 2 and Wp % 8 == 0 and Q == B * Hp * Wp
    assert HWp >= H * W and HWp % 8 == 0 and Kq >= B * HWp and Kq % 64 == 0 and Qs >= Kq
    return Hp, Wp, HWp, Kq, Q, Qs


def _padded_check(name, kind, out, Q, ref_img, A_img, k, dt, Hp, Wp, extra_img=None):
    """out [Q + guard][C]: interior = the reference, every border / pad cell exactly 0, guard rows untouched."""
    assert _guard_ok(out, Q)
    ref, inter = R.pad_nhwc(ref_img, Hp, Wp)
    got = out[:Q].cpu()
    assert bool((got[~inter] == 0).all()), "a pad cell is not zero"
    if kind == "dyadic":
        _exact(got, ref, dt)
    else:
        C = ref.shape[1]
        _elem(name, got[inter], ref_img.reshape(-1, C), A_img.reshape(-1, C), k, dt,
              None if extra_img is None else extra_img.reshape(-1, C))


@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("h,w,up", PADDED)
def test_upsample_pad_and_bn_relu_pad(h, w, up, C, dname, kind):
    """ebc_dec_upsample_pad (k = 8, as ebc_dec_upsample) and ebc_bn_relu_pad (k = 1) into the zero-padded NHWC image:
    the whole padded image is written, pad columns beyond W + 1 included."""
    dt, L, B = DT[dname], _lib.lib(), PB
    code = _lib.dtype_code(dt)
    H, W = h * up, w * up
    Hp, Wp, HWp, Kq, Q, Qs = _geometry(L, code, B, H, W, C)
    feat = _feat(kind, (B, h, w, C), 1)
    xpad = _guarded(Q, C, dt)
    _lib.check(L.ebc_dec_upsample_pad(code, hold(feat), _lib.ptr(xpad), B, h, w, C, up, _lib.stream()), "upsample_pad")
    ref, A = R.upsample(feat, up)
    _padded_check("dec_upsample_pad", kind, xpad, Q, ref, A, 8, dt, Hp, Wp)
    z = _acts(kind, (B, H, W, C), 2, dt)
    sc, sh = _affine(kind, C, 3)
    z64 = z.to(F64)
    hpad = _guarded(Q, C, dt)
    _lib.check(L.ebc_bn_relu_pad(code, hold(z), hold(sc, True), hold(sh, True), _lib.ptr(hpad), B, H, W, C,
                                 _lib.stream()), "bn_relu_pad")
    if kind == "dyadic":
        assert int((z64 * sc + sh == 0).sum()) > 0
    _padded_check("bn_relu_pad", kind, hpad, Q, R.bn_relu(z64, sc, sh), (z64 * sc).abs() + sh.abs(), 1, dt, Hp, Wp)


@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [64, 128, 12])
@pytest.mark.parametrize("h,w,up", PADDED)
def test_bn_add_relu(h, w, up, C, dname, kind):
    """ebc_bn_add_relu: y = max(fma(z, scale, shift) + bilinear_up(feat), 0): k = 10 (the fma, the 8 of the
    interpolation, the sum).  C = 12: the 4-channel instantiation (C % 8 != 0)."""
    dt, L, B = DT[dname], _lib.lib(), PB
    H, W = h * up, w * up
    P = B * H * W
    feat = _feat(kind, (B, h, w, C), 1)
    z = _acts(kind, (B, H, W, C), 2, dt)
    sc, sh = _affine(kind, C, 3)
    y = _guarded(P, C, dt)
    _lib.check(L.ebc_bn_add_relu(_lib.dtype_code(dt), hold(z), hold(sc, True), hold(sh, True),
                                 hold(feat), up, _lib.ptr(y), B, H, W, C, _lib.stream()), "bn_add_relu")
    res, Ares = R.upsample(feat, up)
    z64 = z.to(F64)
    _store_check("bn_add_relu", kind, y, P, R.relu(z64 * sc + sh + res).reshape(-1, C),
                 ((z64 * sc).abs() + sh.abs() + Ares).reshape(-1, C), 10, dt)


@pytest.mark.parametrize("form", ["mask_y", "recomputed"])
@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("h,w,up", PADDED)
def test_bn_bwd_apply(h, w, up, C, dname, kind, form):
    """ebc_bn_bwd_apply (k = 6, as the flat form): dzpad = the padded NHWC image of dz with an exactly zero border,
    dzT [C][Qs] = its transpose over the weight gradient's K: column b*HWp + r for pixel r of image b, 0 from H*W to
    HWp and up to Kq; columns >= Kq and rows >= C are not written."""
    dt, L, B = DT[dname], _lib.lib(), PB
    code = _lib.dtype_code(dt)
    H, W = h * up, w * up
    P = B * H * W
    Hp, Wp, HWp, Kq, Q, Qs = _geometry(L, code, B, H, W, C)
    gy, z, my, mean, rstd, sc, sh, coef, m = _bwd_apply_inputs(kind, P, C, dt, form)
    dzpad = _guarded(Q, C, dt)
    dzT = _guarded(C, Qs, dt)
    _lib.check(L.ebc_bn_bwd_apply(code, hold(gy), hold(my) if form == "mask_y" else None,
                                  hold(z), hold(mean, True), hold(rstd, True), hold(sc, True),
                                  hold(sh, True), hold(coef, True), _lib.ptr(dzpad), _lib.ptr(dzT), B, H, W, C,
                                  _lib.stream()), "bwd_apply")
    ref, g, A = R.bn_bwd_dz(gy, m, z, mean, rstd, coef)
    ref_img, A_img = ref.reshape(B, H, W, C), A.reshape(B, H, W, C)
    _padded_check("bn_bwd_apply.dzpad", kind, dzpad, Q, ref_img, A_img, 6, dt, Hp, Wp)
    assert _guard_ok(dzT, C)
    got = dzT[:C].cpu()
    assert bool((got[:, Kq:] == SENT).all()), "columns past Kq were written"
    refT, AT = R.dzT_layout(ref_img, HWp, Kq), R.dzT_layout(A_img, HWp, Kq)
    live = R.dzT_layout(torch.ones(B, H, W, 1, dtype=F64), HWp, Kq)[0] > 0            # [Kq]
    assert bool((got[:, :Kq][:, ~live] == 0).all()), "dzT is not zero past an image's H*W"
    if kind == "dyadic":
        _exact(got[:, :Kq], refT, dt)
    else:
        _elem("bn_bwd_apply.dzT", got[:, :Kq][:, live], refT[:, live], AT[:, live], 6, dt)
    # the two outputs hold the same rounded values
    assert torch.equal(got[:, :Kq][:, live].t().contiguous(), dzpad[:Q].cpu()[R.pad_nhwc(ref_img, Hp, Wp)[1]])


# ----------------------------------------------------------------------------------------------- weights, scale, cast
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("N,C", [(32, 64), (96, 32)])
def test_dec_prep_weights(N, C, dname):
    dt, L = DT[dname], _lib.lib()
    w = torch.randn(N, C, 3, 3, generator=_gen(1))
    wk, wf = _guarded(N * 9, C, dt), _guarded(C * 9, N, dt)
    _lib.check(L.ebc_dec_prep_weights(_lib.dtype_code(dt), hold(w), _lib.ptr(wk), _lib.ptr(wf), N, C, _lib.stream()),
               "prep_weights")
    rk, rf = R.conv_weight_layouts(w.to(dt))
    assert _guard_ok(wk, N * 9) and _guard_ok(wf, C * 9)
    assert torch.equal(wk[:N * 9].cpu(), rk.reshape(N * 9, C))
    assert torch.equal(wf[:C * 9].cpu(), rf.reshape(C * 9, N))


@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
def test_prep_weights_1x1(dname):
    dt, L, N, K = DT[dname], _lib.lib(), 32, 96
    w = torch.randn(N, K, generator=_gen(1))
    wk, wt = _guarded(N, K, dt), _guarded(K, N, dt)
    _lib.check(L.ebc_prep_weights_1x1(_lib.dtype_code(dt), hold(w), _lib.ptr(wk), _lib.ptr(wt), N, K, _lib.stream()),
               "prep_1x1")
    rk, rt = R.weight_1x1_layouts(w.to(dt))
    assert _guard_ok(wk, N) and _guard_ok(wt, K)
    assert torch.equal(wk[:N].cpu(), rk) and torch.equal(wt[:K].cpu(), rt)


@pytest.mark.parametrize("na,nb", [(1000, 0), (0, 7), (300001, 5)])
def test_scale2(na, nb):
    """a * s and b * s in one launch; 300001 + 5 elements is past the 1024-block cap (the stride loop) with the a / b
    seam inside one block."""
    L = _lib.lib()
    s = torch.tensor([1.7], device="cuda")
    a, b = torch.randn(na, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)), \
        torch.randn(nb, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    ao, bo = torch.full((na + 64,), SENT, device="cuda"), torch.full((nb + 64,), SENT, device="cuda")
    _lib.check(L.ebc_scale2(_lib.ptr(s), _lib.ptr(a) if na else None, _lib.ptr(ao) if na else None, na,
                            _lib.ptr(b) if nb else None, _lib.ptr(bo) if nb else None, nb, _lib.stream()), "scale2")
    assert torch.equal(ao[:na], a * s) and torch.equal(bo[:nb], b * s)
    assert bool((ao[na:] == SENT).all()) and bool((bo[nb:] == SENT).all())


@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("n", [4, 8192 * 256 * 4 + 4])
def test_cast_f32(n, dname):
    """n = 8192 * 256 * 4 + 4 is one vector past the grid cap: the stride loop's second trip."""
    dt, L = DT[dname], _lib.lib()
    x = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 3
    out = torch.full((n + 64,), SENT, dtype=dt, device="cuda")
    _lib.check(L.ebc_cast_f32(_lib.dtype_code(dt), _lib.ptr(x), _lib.ptr(out), n, _lib.stream()), "cast")
    assert torch.equal(out[:n], x.to(dt)) and bool((out[n:] == SENT).all())


# ----------------------------------------------------------------------------------------------- rejections
def test_argument_rejections():
    """Host-side returns: nothing is launched (every buffer is nevertheless as large as the launch would need)."""
    L = _lib.lib()
    st = _lib.stream()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")          # any operand
    p = _lib.ptr(buf)
    f16, f32 = _lib.EBC_F16, _lib.EBC_F32
    # C / 8 > 512 in the reductions
    assert L.ebc_bn_stats(f16, p, p, p, buf.numel(), 4, 4104, st) == EBC_E_UNSUPPORTED
    assert L.ebc_bn_stats_finalize(f16, p, p, buf.numel(), 4, 4104, EPS, MOM, p, p, p, p, p, p, p, p, p, p, st) == EBC_E_UNSUPPORTED
    assert L.ebc_bn_bwd_reduce(f16, p, p, p, p, p, p, p, p, p, buf.numel(), 4, 4104, st) == EBC_E_UNSUPPORTED
    assert L.ebc_bn_bwd_reduce_finalize(f16, p, p, p, p, p, p, p, p, p, p, p, p, buf.numel(), 4, 4104, st) == EBC_E_UNSUPPORTED
    # C % 8 != 0 in the backward reduction (one 8-channel vector per thread)
    assert L.ebc_bn_bwd_reduce(f16, p, p, p, p, p, p, p, p, p, buf.numel(), 4, 12, st) == EBC_E_UNSUPPORTED
    assert L.ebc_bn_bwd_reduce_finalize(f16, p, p, p, p, p, p, p, p, p, p, p, p, buf.numel(), 4, 12, st) == EBC_E_UNSUPPORTED
    # no rows
    for P in (0, -3):
        assert L.ebc_bn_bwd_reduce(f16, p, p, p, p, p, p, p, p, p, buf.numel(), P, 64, st) == EBC_E_ARG
        assert L.ebc_bn_bwd_reduce_finalize(f16, p, p, p, p, p, p, p, p, p, p, p, p, buf.numel(), P, 64, st) == EBC_E_ARG
        assert L.ebc_bn_stats(f16, p, p, p, buf.numel(), P, 64, st) == EBC_E_ARG
    # odd H / W in the pools
    assert L.ebc_bn_relu_avgpool(f16, p, p, p, p, 1, 3, 4, 8, st) == EBC_E_ARG
    assert L.ebc_avgpool2(f16, f16, p, p, 1, 3, 4, 8, st) == EBC_E_ARG
    assert L.ebc_avgpool2(f16, f16, p, p, 1, 4, 3, 8, st) == EBC_E_ARG
    assert L.ebc_avgpool2_bwd(f16, f16, p, p, 1, 3, 4, 8, st) == EBC_E_ARG
    # element types
    assert L.ebc_avgpool2(f32, f16, p, p, 1, 4, 4, 8, st) == EBC_E_ARG
    assert L.ebc_avgpool2_bwd(f16, f32, p, p, 1, 4, 4, 8, st) == EBC_E_ARG
    assert L.ebc_cast_f32(f16, p, p, 6, st) == EBC_E_ARG
    # workspace one byte short: 16384 + ceil(100 / 512) * 8 * 64
    need = 16384 + 8 * 64
    assert L.ebc_bn_stats(f16, p, p, p, need - 1, 100, 64, st) == EBC_E_ARG
    assert L.ebc_bn_bwd_reduce(f16, p, p, p, p, p, p, p, p, p, need - 1, 100, 64, st) == EBC_E_ARG
    # a batch of one element has no unbiased variance
    assert L.ebc_bn_finalize(p, 1.0, EPS, MOM, p, p, p, p, p, p, p, p, None, 8, st) == EBC_E_ARG
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
