"""The LayerNorm, attention and similarity-head entry points (vit_misc.hip, attention.hip, head.hip), one kernel at a
time, per element against the float64 references of tests/_enc_refs.py (pinned to torch in tests/test_enc_refs_cpu.py).

Every output buffer carries sentinel guard rows / elements that must survive, every workspace is sized exactly from its
*_workspace_bytes call plus guard bytes, and every check prints "RATIO <name> <largest error / bound>" before it asserts.

Bounds are derived from the kernels' rounding points as read in the code, first order in u = 2^-24 (the unit roundoff of
f32), in the form  ulp_T(ref) / 2 + k u A  (A = the sum of the absolute terms of the expression, k = the f32 operations
counted in the kernel, stated at each bound) plus the propagated error of every computed operand.  A sum of n terms in
any order is charged depth * u * sum|terms| with depth = the longest chain of additions.  No ulp figure for the device
library's exp2 / expf / logf / sqrtf / division is documented with the toolchain, so each is allowed 2 f32 ulp
(relative 4 u) -- TRANS below.  16-bit MFMA operands rounded in flight (the probabilities before P V, P and dS before the
dV / dQ / dK products) add u_T |a b| per product, u_T = 2^-11 (f16) or 2^-8 (bf16), and for f16 2^-25 |b| where the
operand is below the normal range."""
import math

import pytest
import torch

import _bn_refs as BR
import _enc_refs as R
from _kernel_checks import GUARD_ROWS, SENT, _Hold, _elem, _exact, _guard_ok, _guarded, _report
from ebc_amd import _lib

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DNAMES = ["f32", "f16", "bf16"]
F64 = torch.float64
U = BR.U32
TRANS = 4 * U                        # 2 f32 ulp, relative: exp2f, expf, logf, sqrtf, 1 / x, x / y
TINY = 2.0 ** -149
UT = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
EPS = float(torch.tensor(1e-5, dtype=torch.float32))         # LN_EPS as the kernel's C float
WS_GUARD = 256

hold = _Hold()


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    hold.clear()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=_gen(seed), dtype=F64)


def _vec(n, dt=torch.float32, fill=SENT):
    """[n + GUARD_ROWS] device vector full of the sentinel."""
    return torch.full((n + GUARD_ROWS,), fill, dtype=dt, device="cuda")


def _cpu64(t):
    return t.detach().to(F64).cpu()


def _untouched(t):
    return bool((t == SENT).all())


# ================================================================================================ LayerNorm
D = 768
# (M, rows_per_group, group_stride, group_offset); rpg = 0 is the identity.  M = 1, 3, 5, 1001: the last workgroup of
# four rows is partial.  (100, 49, 82, 33): M is no multiple of rpg, the last group has 2 rows.
LN_CASES = [(1, 0, 0, 0), (3, 0, 0, 0), (4, 0, 0, 0), (5, 0, 0, 0), (1001, 0, 0, 0),
            (2 * 196, 196, 229, 33), (3 * 49, 49, 82, 33), (5, 1, 7, 6), (100, 49, 82, 33)]


def _ln_inputs(M, rpg, gs, go):
    """x [N][768] f32 (as float64): every source row has its own offset and scale, so a row read from or written to the
    wrong place misses its bound; mapped row 1 is constant (variance 0, rstd = 1 / sqrt(eps)), mapped row 2 has
    magnitude 1e4 with spread 1 (the cancellation the two-pass variance is there for)."""
    rows = R.ln_rows(M, rpg, gs, go)
    N = M if rpg <= 0 else -(-M // rpg) * gs
    r = torch.arange(N, dtype=F64)[:, None]
    x = _randn((N, D), 1) * (0.5 + (r % 7) * 0.5) + (r % 11 - 5) * 0.7
    if M >= 3:
        x[rows[1]] = 3.5
        x[rows[2]] = 1e4 + _randn((D,), 2)
    x = x.to(torch.float32).to(F64)
    gamma = (_randn((D,), 3) * 0.1 + 1).to(torch.float32).to(F64)
    beta = (_randn((D,), 4) * 0.1).to(torch.float32).to(F64)
    return x, gamma, beta, rows, N


def _ln_stat_bounds(f):
    """mean: one tree of depth 11 (3 float4 a lane: 2 + 3, six butterfly levels) and the product with 1/768: 12 u
    mean|x|.  variance: x - mean, the square (2 u + 1 u relative to each positive term), the same tree and product
    (12 u), + eps (1 u): 16 u, and sum (x - m')^2 = sum (x - m)^2 + n (m' - m)^2 shifts it by dmean^2.  rstd = 1 /
    sqrtf(.): half the variance's relative error plus two TRANS (8 u) and the half-ulp of the result (1 u)."""
    dmean = 12 * U * f["xs"].abs().mean(1)
    rho = 0.5 * (16 * U * f["var"] + dmean ** 2) / (f["var"] + EPS) + 9 * U
    return dmean, rho


@pytest.mark.parametrize("M,rpg,gs,go", LN_CASES)
@pytest.mark.parametrize("dname", DNAMES)
def test_layernorm_fwd(dname, M, rpg, gs, go):
    """ebc_layernorm_fwd: y = ((x - mean) * rstd) * gamma + beta per element (k = 4 on A = |xhat gamma| + |beta|, plus
    the propagated |gamma| rstd dmean + |xhat gamma| rho_rstd), mean and rstd per row; out only / out_f32 only / both,
    with and without mean / rstd (rstd alone is never written)."""
    dt = DT[dname]
    L = _lib.lib()
    x, gamma, beta, rows, N = _ln_inputs(M, rpg, gs, go)
    f = R.layernorm_fwd(x, gamma, beta, M, rpg, gs, go, EPS)
    dmean, rho = _ln_stat_bounds(f)
    if M >= 3:
        assert float(f["var"][1]) == 0.0 and abs(float(f["rstd"][1]) * math.sqrt(EPS) - 1) < 1e-12
        assert float(f["mean"][2]) > 9e3 and 0.5 < float(f["var"][2]) < 2
    xg = (f["xs"] - f["mean"][:, None]) * f["rstd"][:, None] * gamma
    A = xg.abs() + beta.abs()
    extra = gamma.abs() * (f["rstd"] * dmean)[:, None] + xg.abs() * rho[:, None]
    px, pg, pb = hold(x, True), hold(gamma, True), hold(beta, True)
    code = _lib.dtype_code(dt)
    for outs in ("out", "outf", "both"):
        for stats in (True, False):
            out = _guarded(M, D, dt) if outs != "outf" else None
            outf = _guarded(M, D, torch.float32) if outs != "out" else None
            mean, rstd = _vec(M), _vec(M)
            _lib.check(L.ebc_layernorm_fwd(code, px, rpg, gs, go, pg, pb, _lib.ptr(out), _lib.ptr(outf),
                                           _lib.ptr(mean) if stats else None, _lib.ptr(rstd), M, D, _lib.stream()), "ln_fwd")
            tag = f"ln_fwd[{outs},{'stats' if stats else 'nostats'}]"
            if out is not None:
                assert _guard_ok(out, M)
                _elem(f"{tag}.out", out[:M], f["y"], A, 4, dt, extra)
            if outf is not None:
                assert _guard_ok(outf, M)
                _elem(f"{tag}.out_f32", outf[:M], f["y"], A, 4, torch.float32, extra)
            if stats:
                assert _guard_ok(mean, M) and _guard_ok(rstd, M)
                _report(f"{tag}.mean", (_cpu64(mean[:M]) - f["mean"]).abs(), dmean + U * f["mean"].abs() + TINY)
                _report(f"{tag}.rstd", (_cpu64(rstd[:M]) - f["rstd"]).abs(), f["rstd"] * rho)
            else:
                assert _untouched(mean) and _untouched(rstd)


@pytest.mark.parametrize("M,rpg,gs,go", LN_CASES)
@pytest.mark.parametrize("dname", DNAMES)
def test_layernorm_bwd(dname, M, rpg, gs, go):
    """ebc_layernorm_bwd: dx = rstd * ((g - s1) - xhat * s2) + dx_in, g = dy * gamma, from the mean / rstd it is handed.
    dy, mean, rstd are read dense; x and dx_in are read, and dx_out / dx_out_t written, at the mapped row: every row
    outside the groups, and the guard rows, keep their sentinel.
    k = 8 on A = rstd (|g| + |s1| + |xhat s2|) + |dx_in| (g 1, xhat 2, the product with s2 1, two subtractions, the
    product with rstd, the addition of dx_in); s1 within 13 u mean|g| (g 1, tree 11, / 768 1), s2 within 16 u
    mean|g xhat| (g xhat 4), propagated as rstd (ds1 + |xhat| ds2).  dy as T and as f32, dx_in given / NULL,
    dx_out_t given / NULL."""
    dt = DT[dname]
    L = _lib.lib()
    x, gamma, beta, rows, N = _ln_inputs(M, rpg, gs, go)
    f = R.layernorm_fwd(x, gamma, beta, M, rpg, gs, go, EPS)
    mean, rstd = f["mean"].to(torch.float32).to(F64), f["rstd"].to(torch.float32).to(F64)
    r = torch.arange(M, dtype=F64)[:, None]
    dy0 = _randn((M, D), 5) * (0.5 + (r % 5) * 0.5)
    dx_in = (_randn((N, D), 6) * 2).to(torch.float32).to(F64)
    px, pg, pm, pr, pdi = hold(x, True), hold(gamma, True), hold(mean, True), hold(rstd, True), hold(dx_in, True)
    code = _lib.dtype_code(dt)
    other = torch.ones(N + GUARD_ROWS, dtype=torch.bool)
    other[rows] = False
    for dy_f32 in (0, 1):
        dyt = torch.float32 if (dy_f32 or dt == torch.float32) else dt
        dy = dy0.to(dyt)
        pdy = hold(dy)
        for with_in in (True, False):
            sent = torch.full((N, D), SENT, dtype=F64)
            b = R.layernorm_bwd(dy.to(F64), x, mean, rstd, gamma, dx_in if with_in else None, M, rpg, gs, go, sent)
            rs = rstd[:, None]
            A = rs * (b["g"].abs() + b["s1"].abs() + (b["xh"] * b["s2"]).abs()) + b["din"].abs()
            ds1 = 13 * U * b["g"].abs().mean(1, keepdim=True)
            ds2 = 16 * U * (b["g"] * b["xh"]).abs().mean(1, keepdim=True)
            extra = rs * (ds1 + b["xh"].abs() * ds2)
            for with_t in (True, False):
                dx = _guarded(N, D, torch.float32)
                dxt = _guarded(N, D, dt)
                _lib.check(L.ebc_layernorm_bwd(code, dy_f32, pdy, px, rpg, gs, go, pm, pr, pg, pdi if with_in else None,
                                               _lib.ptr(dx), _lib.ptr(dxt) if with_t else None, M, D, _lib.stream()), "ln_bwd")
                tag = f"ln_bwd[dy_f32={dy_f32},{'dx_in' if with_in else 'no_dx_in'},{'t' if with_t else 'no_t'}]"
                assert _untouched(dx[other.cuda()])
                _elem(f"{tag}.dx_out", dx[:N][rows.cuda()], b["dense"], A, 8, torch.float32, extra)
                if with_t:
                    assert _untouched(dxt[other.cuda()])
                    _elem(f"{tag}.dx_out_t", dxt[:N][rows.cuda()], b["dense"], A, 8, dt, extra)
                else:
                    assert _untouched(dxt)


# ================================================================================================ attention
LOG2E = math.log2(math.e)
NS = 64            # a 64-term dot product through the MFMA accumulator: at most 64 u sum|a b|
ATTN_CUS = 256


def _fwd_path(B, H, L):
    """The forward kernel ebc_attention_fwd takes, from attention.hip's host dispatch."""
    if L > 256:
        return "long"
    return "w16" if (L > 128 and B * H <= ATTN_CUS) else "w8"


def _bwd_path(dname, L):
    if L > 256:
        return "long"
    if dname != "f32":
        return "one"
    return "w16" if L > 128 else "w8"


def _writes_delta(dname, L):
    """delta_ws: written by the f32 dQ kernel (8 and 16 waves) and by the streamed dQ kernel of every dtype; the 16-bit
    one-workgroup backward keeps delta in LDS and must leave the buffer alone."""
    return _bwd_path(dname, L) != "one"


# the paths every later dispatch change must keep reachable from this module (asserted next to the cases)
ATTN_SHAPES = [(1, 1, 1), (2, 3, 15), (2, 3, 16), (2, 3, 17), (1, 12, 128), (1, 12, 129), (2, 2, 255), (1, 2, 256),
               (1, 2, 257), (1, 2, 512), (1, 1, 768), (1, 2, 1025)]
ATTN_FWD_ONLY = [(3, 100, 130), (22, 12, 197)]          # the generic-length 8-wave forward: B * H > 256, 128 < L <= 256
SEL_EXACT_L = {1, 15, 16, 17, 128, 256, 512}            # every query's m is a power of two (test_enc_refs_cpu.py)


def test_attention_cases_reach_every_path():
    for B, H, L in ATTN_FWD_ONLY:
        assert B * H > ATTN_CUS and 128 < L <= 256 and L != 229 and _fwd_path(B, H, L) == "w8"
    fwd = {_fwd_path(B, H, L) for B, H, L in ATTN_SHAPES}
    assert fwd == {"w8", "w16", "long"}
    assert _fwd_path(1, 12, 128) == "w8" and _fwd_path(1, 12, 129) == "w16" and _fwd_path(1, 2, 257) == "long"
    bwd = {(d, _bwd_path(d, L)) for d in DNAMES for _, _, L in ATTN_SHAPES}
    assert {("f32", "w8"), ("f32", "w16"), ("f16", "one"), ("bf16", "one"), ("f32", "long"), ("f16", "long"),
            ("bf16", "long")} <= bwd
    assert _bwd_path("f32", 128) == "w8" and _bwd_path("f32", 129) == "w16" and _bwd_path("f16", 256) == "one"
    assert all(_fwd_path(1, 2, L) == "long" for L in (513, 768, 1025)) and _fwd_path(1, 2, 229) == "w16"


def _attn_fwd(dname, qkv, B, L, H):
    dt = DT[dname]
    out = _guarded(B * L, H * 64, dt)
    lse = _vec(B * H * L)
    _lib.check(_lib.lib().ebc_attention_fwd(_lib.dtype_code(dt), hold(qkv), _lib.ptr(out), _lib.ptr(lse), B, L, H,
                                            _lib.stream()), "attn_fwd")
    assert _guard_ok(out, B * L) and _guard_ok(lse, B * H * L)
    return R.heads(_cpu64(out[:B * L]), B, L, H), _cpu64(lse[:B * H * L]).view(B, H, L), out


def _attn_bwd(dname, qkv, dout, out, lse, B, L, H):
    """out [B*L][H*64] in T and lse [B][H][L] f32 as handed to the kernel (CPU tensors)."""
    dt = DT[dname]
    dqkv = _guarded(B * L, 3 * H * 64, dt)
    delta = _vec(B * H * L)
    _lib.check(_lib.lib().ebc_attention_bwd(_lib.dtype_code(dt), hold(qkv), hold(dout), hold(out), hold(lse),
                                            _lib.ptr(delta), _lib.ptr(dqkv), B, L, H, _lib.stream()), "attn_bwd")
    assert _guard_ok(dqkv, B * L) and _guard_ok(delta, B * H * L)
    if not _writes_delta(dname, L):
        assert _untouched(delta)
    dq, dk, dv = R.split_qkv(_cpu64(dqkv[:B * L]), B, L, H)
    return dq, dk, dv, _cpu64(delta[:B * H * L]).view(B, H, L), dqkv


def _sub16(x, dname):
    """f16 operands below the normal range are rounded to a multiple of 2^-24: at most 2^-25 absolute."""
    if dname != "f16":
        return torch.zeros_like(x)
    return (x.abs() < 2.0 ** -13).to(F64) * 2.0 ** -25


def _check_attn_fwd(tag, dname, q, k, v, o_got, lse_got):
    """Forward against the float64 forward.  In natural-log units, with smax = the row's largest |score|:
      score      ds_ij = NS u (|q| . |k|) / 8; the row maximum is one of the computed scores: ds_i* = max_j ds_ij
      exponent   fma(s, c2, -(m c2)) with c2 = log2(e) / 8 rounded: 5 u smax (c2 1 on |s - m| <= 2 smax, m c2 1, fma 2)
      p          rho_ij = ds_ij + ds_i* + 5 u smax + TRANS (exp2); flushed below 2^-126
      streamed   per 256-key chunk alpha = exp2((m - mn) c2) and the rescales: 7 u (TRANS, o alpha, sum alpha + cs, the
                 subtraction and product of the exponent) + the exponents' rounding 4 u smax over the row
      N = P V    sum_j p |v| (rho + u_T + L u) (+ the f16 subnormal term); S = sum p: sum_j p (rho + L u)
      o          (dN + |o| dS) / S + 5 u |o| (1 / S TRANS, the product 1) + ulp_T / 2
      lse        m / 8 (exact) + logf(S): ds_i* + dS / S + TRANS |log S| + u |lse| (+ the streamed term)"""
    dt = DT[dname]
    L = q.shape[2]
    f = R.attention_fwd(q, k, v)
    ds = NS * U * (q.abs() @ k.abs().transpose(-1, -2)) / 8.0
    smax = f["s"].abs().max(-1, keepdim=True).values
    rho = ds + ds.max(-1, keepdim=True).values + 5 * U * smax + TRANS
    if L > 256:
        rho = rho + (-(-L // 256)) * 7 * U + 4 * U * smax
    p = f["p"]
    S = f["l"]
    dN = (p * (rho + UT[dname] + L * U) + _sub16(p, dname) + 2.0 ** -126) @ v.abs()
    dS = (p * (rho + L * U)).sum(-1, keepdim=True)
    bound = (dN + f["o"].abs() * dS) / S + 5 * U * f["o"].abs() + 0.5 * BR.ulp(f["o"], dt)
    assert bool(torch.isfinite(o_got).all()) and bool(torch.isfinite(lse_got).all())
    _report(f"{tag}.out", (o_got - f["o"]).abs(), bound)
    lse = f["lse"]
    lb = (ds.max(-1).values + (dS / S).squeeze(-1) + TRANS * torch.log(S).abs().squeeze(-1) + U * lse.abs()
          + 0.5 * BR.ulp(lse, torch.float32))
    if L > 256:
        lb = lb + (-(-L // 256)) * 7 * U + 4 * U * smax.squeeze(-1)
    _report(f"{tag}.lse", (lse_got - lse).abs(), lb)
    return f


def _check_attn_bwd(tag, dname, q, k, v, do, o, lse, got):
    """Backward against the restated backward on the kernel's own out / lse.  With P = exp(s - lse):
      exponent   fma(s, c2, -(lse log2 e)): ds_ij + 3 u (|s_ij| + |lse_i|); rho_ij = that + TRANS
      dP, delta  64-term products: NS u (|dO| . |v|)_ij and NS u sum|dO o|_i; their difference (one subtraction, or the
                 accumulator started at -delta): E_ij = (NS + 1) u ((|dO| . |v|)_ij + sum|dO o|_i) + u |dP - delta|
      dS         P (rho |dP - delta| + E + u |dP - delta|)
      dQ         sum_j (ddS + u_T |dS| + sub) |k| / 8 + L u sum_j |dS k| / 8 + u |dQ| (the 1/8 product is exact, the
                 conversion's rounding is ulp_T / 2); dK the same over the queries with |q|
      dV         sum_i (P (rho + u_T) + sub) |dO| + L u sum_i P |dO| + ulp_T / 2"""
    dt = DT[dname]
    L = q.shape[2]
    r = R.attention_bwd(q, k, v, do, o, lse)
    dq, dk, dv, delta = got
    uT = UT[dname]
    ds = NS * U * (q.abs() @ k.abs().transpose(-1, -2)) / 8.0
    rho = ds + 3 * U * (r["s"].abs() + lse.abs()[..., None]) + TRANS
    adv = do.abs() @ v.abs().transpose(-1, -2)
    ado = (do * o).abs().sum(-1)
    diff = (r["dP"] - r["delta"][..., None]).abs()
    E = (NS + 1) * U * (adv + ado[..., None]) + U * diff
    P = r["P"]
    ddS = P * (rho * diff + E + U * diff) + 2.0 ** -126 * diff
    w = ddS + uT * r["dS"].abs() + _sub16(r["dS"], dname)
    bq = (w @ k.abs() + L * U * (r["dS"].abs() @ k.abs())) / 8.0 + U * r["dq"].abs() + 0.5 * BR.ulp(r["dq"], dt)
    bk = ((w.transpose(-1, -2) @ q.abs() + L * U * (r["dS"].abs().transpose(-1, -2) @ q.abs())) / 8.0 + U * r["dk"].abs()
          + 0.5 * BR.ulp(r["dk"], dt))
    wp = P * (rho + uT) + _sub16(P, dname) + 2.0 ** -126
    bv = wp.transpose(-1, -2) @ do.abs() + L * U * (P.transpose(-1, -2) @ do.abs()) + 0.5 * BR.ulp(r["dv"], dt)
    for t in (dq, dk, dv):
        assert bool(torch.isfinite(t).all())
    _report(f"{tag}.dq", (dq - r["dq"]).abs(), bq)
    _report(f"{tag}.dk", (dk - r["dk"]).abs(), bk)
    _report(f"{tag}.dv", (dv - r["dv"]).abs(), bv)
    if _writes_delta(dname, L):
        _report(f"{tag}.delta", (delta - r["delta"]).abs(), NS * U * ado + 0.5 * BR.ulp(r["delta"], torch.float32))
    return r


def _fwd_then_bwd(tag, dname, q, k, v, do, B, L, H):
    """The forward per element; then the backward fed out = the float64 forward rounded once to T and lse rounded to
    f32, so the backward kernel is held apart from the forward's error."""
    dt = DT[dname]
    qkv = R.pack_qkv(q, k, v).to(dt)
    o_got, lse_got, _ = _attn_fwd(dname, qkv, B, L, H)
    f = _check_attn_fwd(tag, dname, q, k, v, o_got, lse_got)
    if do is None:
        return
    o_in = R.unheads(f["o"]).to(dt)
    lse_in = f["lse"].to(torch.float32)
    got = _attn_bwd(dname, qkv, R.unheads(do).to(dt), o_in, lse_in.contiguous(), B, L, H)
    _check_attn_bwd(tag, dname, q, k, v, do, R.heads(o_in, B, L, H), lse_in.to(F64), got[:4])


@pytest.mark.parametrize("B,H,L", ATTN_SHAPES + ATTN_FWD_ONLY)
@pytest.mark.parametrize("dname", DNAMES)
def test_attention_random(dname, B, H, L):
    """(a) random normal inputs (std 1.5: scores of std ~2), forward and backward per element."""
    dt = DT[dname]
    q, k, v = (R.rounded(_randn((B, H, L, 64), s) * 1.5, dt) for s in (1, 2, 3))
    do = R.rounded(_randn((B, H, L, 64), 4), dt) if (B, H, L) in ATTN_SHAPES else None
    _fwd_then_bwd(f"attn_random[{_fwd_path(B, H, L)},{_bwd_path(dname, L)}]", dname, q, k, v, do, B, L, H)


@pytest.mark.parametrize("B,H,L", ATTN_SHAPES + ATTN_FWD_ONLY)
@pytest.mark.parametrize("dname", DNAMES)
def test_attention_selection(dname, B, H, L):
    """(b) selection inputs (_enc_refs.selection_inputs): each query attends uniformly to its m keys and every other
    probability is exactly 0.  Where every m is a power of two (L in SEL_EXACT_L) out must equal the reference rounded
    once, bit for bit, in every dtype, and lse must be 128 + log m to logf's bound (TRANS |log m|, the addition's half
    ulp); the 16-bit backward, whose P and dS round to their exact values on the way into the MFMA, must give dQ, dK
    and dV bit for bit.  The f32 backward computes P = exp2(s c2 - lse log2 e) from an lse that f32 cannot hold exactly
    (128 + log 2), and keeps that P unrounded: it is held to the bound, as are the lengths with an m that is no power
    of two.  One misplaced key, value, query row, head or swizzle chunk fails either way."""
    dt = DT[dname]
    qkv64, dout64, mult = R.selection_inputs(B, L, H, 5)
    q, k, v = R.split_qkv(qkv64, B, L, H)
    exact = L in SEL_EXACT_L
    assert exact == bool(((mult & (mult - 1)) == 0).all())
    tag = f"attn_select[{_fwd_path(B, H, L)},{_bwd_path(dname, L)}]"
    qkv = qkv64.to(dt)
    o_got, lse_got, out_dev = _attn_fwd(dname, qkv, B, L, H)
    do = R.heads(dout64, B, L, H)
    f = R.selection_reference(q, k, v, do, mult)
    if exact:
        _exact(out_dev[:B * L], R.unheads(f["o"]), dt)
        lm = torch.log(mult.to(F64))
        _report(f"{tag}.lse", (lse_got - (128.0 + lm)).abs(), TRANS * lm + 0.5 * BR.ulp(128.0 + lm, torch.float32))
    else:
        _check_attn_fwd(tag, dname, q, k, v, o_got, lse_got)
    if (B, H, L) not in ATTN_SHAPES:
        return
    o_in = R.unheads(f["o"]).to(dt)
    lse_in = f["lse"].to(torch.float32)
    got = _attn_bwd(dname, qkv, dout64.to(dt), o_in, lse_in.contiguous(), B, L, H)
    if exact and dname != "f32":
        assert torch.equal(o_in.to(F64), R.unheads(f["o"]))              # out as handed over is the exact reference
        _exact(got[4][:B * L], R.pack_qkv(f["dq"], f["dk"], f["dv"]), dt)
    else:
        _check_attn_bwd(tag, dname, q, k, v, do, R.heads(o_in, B, L, H), lse_in.to(F64), got[:4])


@pytest.mark.parametrize("kind", ["rising", "falling", "peak"])
@pytest.mark.parametrize("L", [229, 513, 768, 1025])
@pytest.mark.parametrize("dname", DNAMES)
def test_attention_drift(dname, L, kind):
    """(c) peaked and drifting softmax (_enc_refs.drift_inputs): the per-chunk maximum rises by about 30 from each
    256-key chunk to the next (every chunk rescales sum and o by alpha = 2^((m - mn) c2)), falls by as much, or one
    dominant key per query sits in the last partial tile.  Per element to the bounds, outputs finite."""
    dt = DT[dname]
    B, H = 1, 2
    q, k, v = (R.rounded(t, dt) for t in R.drift_inputs(B, L, H, kind, 9))
    do = R.rounded(_randn((B, H, L, 64), 4), dt)
    _fwd_then_bwd(f"attn_{kind}[{_fwd_path(B, H, L)},{_bwd_path(dname, L)}]", dname, q, k, v, do, B, L, H)


# ================================================================================================ head
def _head_inputs(P, NB, embed, zdt, special, seed=3):
    Z = _randn((P, embed), seed)
    if special:
        Z[1] = 0                                               # the fmaxf(nrm, 1e-12f) clamp
        Z[2] *= 1e-3 / float(Z[2].norm())                      # a row of norm ~1e-3
    Z = R.rounded(Z, zdt)
    text = _randn((NB, embed), seed + 1).to(torch.float32).to(F64)
    ls = torch.tensor([2.3], dtype=torch.float32).to(F64)
    anchors = (torch.arange(NB, dtype=F64) * 0.9).to(torch.float32).to(F64)
    return Z, text, ls, anchors


def _head_fwd_bounds(f, embed, NB):
    """One wave a pixel, NV = embed / 64 channels a lane.
      norms      sum of squares: product 1, lane chain NV, six butterfly levels, all terms positive: (NV + 7) u; sqrtf
                 halves it and adds TRANS, the clamp constant 1e-12f is within u of 1e-12, 1 / x adds TRANS:
                 rho_n = (0.5 (NV + 7) + 9) u, for the pixel and for each text row
      s          expf(logit_scale): rho_s = TRANS
      logits     zs = s (z inv) [rho_n + 2 u + rho_s], tn = t inv [rho_n + u], their product 1, lane chain <= NV, six
                 levels: dlg = (2 rho_n + rho_s + (NV + 10) u) A, A = s sum|zn tn|
      softmax    expf(lg - mx): dlg_k + max_k dlg + u |lg_k - mx| + TRANS; the sum NB u; the quotient TRANS:
                 rho'_k = that for k, the largest of them for the sum, (NB + 4) u
      exp        sum_k p_k a_k (product 1, chain NB): sum_k p_k |a_k| (rho'_k + (NB + 1) u)"""
    NV = embed // 64
    rho_n = (0.5 * (NV + 7) + 9) * U
    rho_s = TRANS
    A = f["s"] * (f["zn"].abs() @ f["tn"].abs().t())
    dlg = (2 * rho_n + rho_s + (NV + 10) * U) * A
    dL = dlg.max(1, keepdim=True).values
    mx = f["lg"].max(1, keepdim=True).values
    rho_p = dlg + dL + U * (f["lg"] - mx).abs() + TRANS
    rho_q = rho_p + rho_p.max(1, keepdim=True).values + NB * U + TRANS
    return {"rho_n": rho_n, "rho_s": rho_s, "dlg": dlg, "rho_q": rho_q, "NV": NV}


# P in {1, 3, 4, 5, 2 * 49}: the forward's four pixels a workgroup, partial and full; B = 2 wherever P is even
HEAD_FWD = [(1, 1), (3, 5), (4, 16), (5, 5), (98, 16), (98, 1)]


@pytest.mark.parametrize("P,NB", HEAD_FWD)
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname", DNAMES)
def test_head_fwd(zname, embed, P, NB):
    """ebc_head_fwd called directly: logits [B][NB][HW] and exp [B][HW] per element, Z in f32 / f16 / bf16 (what the
    AMP path hands it), with a zero row (logits exactly 0) and a row of norm 1e-3 where P allows."""
    B = 2 if P % 2 == 0 else 1
    HW = P // B
    Z, text, ls, anchors = _head_inputs(P, NB, embed, DT[zname], special=P >= 3)
    f = R.head_fwd(Z, text, ls, anchors, B, HW)
    hb = _head_fwd_bounds(f, embed, NB)
    logits = _vec(B * NB * HW)
    expo = _vec(B * HW)
    _lib.check(_lib.lib().ebc_head_fwd(_lib.dtype_code(DT[zname]), hold(Z.to(DT[zname])), hold(text, True), hold(ls, True),
                                       hold(anchors, True), _lib.ptr(logits), _lib.ptr(expo), P, HW, NB, embed,
                                       _lib.stream()), "head_fwd")
    assert _guard_ok(logits, B * NB * HW) and _guard_ok(expo, B * HW)
    lg = _cpu64(logits[:B * NB * HW]).view(B, NB, HW).permute(0, 2, 1).reshape(P, NB)
    _report("head_fwd.logits", (lg - f["lg"]).abs(), hb["dlg"] + 0.5 * BR.ulp(f["lg"], torch.float32))
    pa = f["pr"] * anchors.abs()
    de = (pa * (hb["rho_q"] + (NB + 1) * U)).sum(1)
    _report("head_fwd.exp", (_cpu64(expo[:P]) - f["e"]).abs(), de + 0.5 * BR.ulp(f["e"], torch.float32))
    if P >= 3:
        assert bool((lg[1] == 0).all())


# nblk = ceil(P / 32) in {1, 2, 8, 9, 57, 64, 65, 121}: head_bias_finalize_kernel's eight waves with fewer blocks than
# waves, its tail alone (nblk <= 56), the 64-block main loop entered exactly (57, 64), main loop plus tail (65, 121);
# P a multiple of 32 and not.  (P, NB, special rows)
HEAD_BWD = [(27, 5, False), (64, 16, True), (250, 1, False), (270, 12, True), (1810, 5, False), (2048, 16, False),
            (2050, 5, False), (3850, 16, False)]
HEAD_DTYPES = [("f32", "f32"), ("f32", "f16"), ("f32", "bf16"), ("f16", "f16"), ("bf16", "bf16"), ("f16", "f32")]


def test_head_bwd_cases_reach_every_finalize_path():
    nblk = [-(-P // 32) for P, _, _ in HEAD_BWD]
    assert nblk == [1, 2, 8, 9, 57, 64, 65, 121]
    assert [n for n in nblk if n - 56 > 0] == [57, 64, 65, 121]            # wave 0 enters the main loop: 0 + 56 < nblk
    assert any(n > 64 for n in nblk) and any(P % 32 for P, _, _ in HEAD_BWD) and any(P % 32 == 0 for P, _, _ in HEAD_BWD)


@pytest.mark.parametrize("P,NB,special", HEAD_BWD)
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname,dzname", HEAD_DTYPES)
def test_head_bwd(zname, dzname, embed, P, NB, special):
    """ebc_head_bwd: dZ per element, d bias and d logit_scale against the float64 sums, with gscale = 0.625, every
    (dbias, dscale) NULL combination (dZ and the sums bit-equal across them and across two runs), the workspace sized
    exactly and guarded.  On top of the forward's errors (_head_fwd_bounds; the kernel recomputes it):
      dl_k       dlogits gs [1] + (dexp gs) p_k (a_k - e) [rho'_k + 3 u, |de p| (de_err + u |a - e|)], their sum 1
      dzn        sum_k (dl_k s) tn_k: ddl s |tn| + |dl s tn| (rho_s + rho_n + (NB + 3) u)
      dot        sum_c zn dzn: |zn| ddzn + |zn dzn| (rho_n + (NV + 8) u)
      dz         (dzn - zn dot) inv: inv (ddzn + |zn| ddot + |zn dot| (rho_n + 2 u) + u (|dzn| + |zn dot|))
                 + |dz| (rho_n + u) + ulp_T / 2; a zero row takes dzn / 1e-12
      d bias     the f32 dz summed: 8 pixels a wave, 2 levels over the waves (one f32 chain a block), then the
                 fixed-order combine, ceil(nblk / 64) a chain and 3 + 8 over chains and waves: depth 21 + ceil(nblk / 64)
      d scale    sum dl lg: ddl |lg| + |dl| dlg + u |dl lg|, depth 8 NB + 13 + ceil(nblk / 64)"""
    zdt, dzdt = DT[zname], DT[dzname]
    Lb = _lib.lib()
    B = 2 if P % 2 == 0 else 1
    HW = P // B
    nblk = -(-P // 32)
    Z, text, ls, anchors = _head_inputs(P, NB, embed, zdt, special)
    dl_up = _randn((B, NB, HW), 7).to(torch.float32).to(F64)
    de_up = _randn((B, HW), 8).to(torch.float32).to(F64)
    gs = 0.625
    r = R.head_bwd(Z, text, ls, anchors, dl_up, de_up, gs, B, HW)
    hb = _head_fwd_bounds(r, embed, NB)
    NV, rho_n, rho_s = hb["NV"], hb["rho_n"], hb["rho_s"]
    if special:
        assert float(r["nrm"][1]) == 0 and torch.equal(r["dz"][1], r["dzn"][1] / 1e-12)
        assert abs(float(r["nrm"][2]) / 1e-3 - 1) < 1e-2
    # bounds
    pa = r["pr"] * anchors.abs()
    dee = (pa * (hb["rho_q"] + (NB + 1) * U)).sum(1, keepdim=True)
    T1 = r["dlg"].abs()
    ame = (anchors - r["e"][:, None]).abs()
    T2 = (r["de"] * r["pr"]).abs() * ame
    ddl = U * T1 + T2 * (hb["rho_q"] + 3 * U) + (r["de"] * r["pr"]).abs() * (dee + U * ame) + U * (T1 + T2)
    tna = r["tn"].abs()
    ddzn = r["s"] * (ddl @ tna) + r["s"] * (r["dl"].abs() @ tna) * (rho_s + rho_n + (NB + 3) * U)
    zna = r["zn"].abs()
    ddot = (zna * ddzn + (r["zn"] * r["dzn"]).abs() * (rho_n + (NV + 8) * U)).sum(1, keepdim=True)
    inv = 1.0 / r["den"][:, None]
    zd = zna * r["dot"].abs()[:, None]
    ddz = inv * (ddzn + zna * ddot + zd * (rho_n + 2 * U) + U * (r["dzn"].abs() + zd)) + r["dz"].abs() * (rho_n + U)
    depth = -(-nblk // 64)
    dbias_b = ddz.sum(0) + (21 + depth) * U * r["dz"].abs().sum(0) + 0.5 * BR.ulp(r["dbias"], torch.float32)
    dllg = (r["dl"] * r["lg"]).abs()
    dsc_b = float((ddl * r["lg"].abs() + r["dl"].abs() * hb["dlg"] + U * dllg).sum() + (8 * NB + 13 + depth) * U * dllg.sum()
                  + 0.5 * BR.ulp(r["dscale"], torch.float32))
    # the call, in every (dbias, dscale) combination
    need = Lb.ebc_head_bwd_workspace_bytes(P, embed)
    assert need == nblk * (embed + 1) * 4
    pZ, pt, pls, pa_, pdl, pde = (hold(Z.to(zdt)), hold(text, True), hold(ls, True), hold(anchors, True), hold(dl_up, True),
                                  hold(de_up, True))
    pgs = hold(torch.tensor([gs]), True)
    first = None
    for combo in ("both", "both", "dbias", "dscale", "none"):
        ws = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        ws[:need].view(torch.float32).fill_(float("nan"))
        dZ = _guarded(P, embed, dzdt)
        dbias, dsc = _vec(embed), _vec(1)
        use_b, use_s = combo in ("both", "dbias"), combo in ("both", "dscale")
        _lib.check(Lb.ebc_head_bwd(_lib.dtype_code(zdt), _lib.dtype_code(dzdt), pZ, pt, pls, pa_, pdl, pde, pgs, _lib.ptr(dZ),
                                   _lib.ptr(dbias) if use_b else None, _lib.ptr(dsc) if use_s else None, P, HW, NB, embed,
                                   _lib.ptr(ws) if combo != "none" else None, need if combo != "none" else 0,
                                   _lib.stream()), "head_bwd")
        assert _guard_ok(dZ, P) and _guard_ok(dbias, embed) and _guard_ok(dsc, 1)
        assert bool((ws[need:] == 0xA5).all())
        if combo == "none":
            assert bool(torch.isnan(ws[:need].view(torch.float32)).all())          # no workspace given, none written
        if not use_b:
            assert _untouched(dbias)
        if not use_s:
            assert _untouched(dsc)
        if first is None:
            first = (dZ, dbias, dsc)
            tag = f"head_bwd[nblk={nblk}]"
            # a clamped row's dzn / 1e-12 is beyond f16: there the stored value is the reference rounded once (inf)
            fits = r["dz"].abs() < float(torch.finfo(dzdt).max) * (1 - 2.0 ** -8)
            assert torch.equal(dZ[:P].cpu()[~fits], r["dz"].to(dzdt)[~fits])
            err = torch.where(fits, (_cpu64(dZ[:P]) - r["dz"]).abs(), torch.zeros_like(ddz))
            _report(f"{tag}.dz", err, ddz + 0.5 * BR.ulp(r["dz"], dzdt))
            _report(f"{tag}.dbias", (_cpu64(dbias[:embed]) - r["dbias"]).abs(), dbias_b)
            _report(f"{tag}.dscale", (_cpu64(dsc[:1]) - r["dscale"]).abs(), torch.tensor([dsc_b], dtype=F64))
        else:
            assert torch.equal(dZ.view(torch.uint8), first[0].view(torch.uint8))   # bit-equal (NaN-free or not)
            if use_b:
                assert torch.equal(dbias, first[1])
            if use_s:
                assert torch.equal(dsc, first[2])
