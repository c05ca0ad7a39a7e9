"""The text-tower kernels (text.hip, the D = 512 LayerNorm instances of vit_misc.hip) through the C ABI, one kernel at a
time, per element against the float64 references of tests/_text_refs.py and tests/_enc_refs.py.

Every output sits in a sentinel-guarded buffer, and every check prints "RATIO <name> <largest error / bound>" before it
asserts.  The bounds follow tests/test_gpu_encoder_kernels.py: first order in u = 2^-24, ulp_T(ref) / 2 + k u A with k
the f32 operations counted in the kernel, a sum in any order charged its longest chain of additions, TRANS = 4 u for
exp2f / logf / sqrtf / division, 16-bit MFMA operands rounded in flight charged u_T."""
import pytest
import torch

import _bn_refs as BR
import _enc_refs as R
import _text_refs as TR
from _kernel_checks import GUARD_ROWS, SENT, _Framed, _Hold, _elem, _exact, _guard_ok, _guarded, _report
from ebc_amd import _lib

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DNAMES = ["f32", "f16", "bf16"]
F64 = torch.float64
U = BR.U32
TRANS = 4 * U
UT = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
NS = 64

hold = _Hold()


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    hold.clear()


def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=F64)


def _vec(n, dt=torch.float32, fill=SENT):
    return torch.full((n + GUARD_ROWS,), fill, dtype=dt, device="cuda")


def _cpu64(t):
    return t.detach().to(F64).cpu()


def _untouched(t):
    return bool((t == SENT).all())


# ================================================================================================ causal attention
# a single token, one exact tile, a ragged tile on either side of it, the 64 boundary, the full context on the largest grid
CA_SHAPES = [(1, 1, 1), (2, 3, 15), (2, 3, 16), (2, 3, 17), (2, 8, 64), (2, 8, 65), (16, 8, 77)]


def _ca_fwd(dname, qkv, B, L, H, with_lse=True):
    dt = DT[dname]
    out = _guarded(B * L, H * 64, dt)
    lse = _vec(B * H * L)
    _lib.check(_lib.lib().ebc_attention_causal_fwd(_lib.dtype_code(dt), hold(qkv), _lib.ptr(out),
                                                   _lib.ptr(lse) if with_lse else None, B, L, H, _lib.stream()), "ca_fwd")
    assert _guard_ok(out, B * L) and _guard_ok(lse, B * H * L)
    return R.heads(_cpu64(out[:B * L]), B, L, H), _cpu64(lse[:B * H * L]).view(B, H, L), out, lse


def _ca_bwd(dname, qkv, dout, out, lse, B, L, H):
    dt = DT[dname]
    dqkv = _guarded(B * L, 3 * H * 64, dt)
    delta = _vec(B * H * L)
    _lib.check(_lib.lib().ebc_attention_causal_bwd(_lib.dtype_code(dt), hold(qkv), hold(dout), hold(out), hold(lse),
                                                   _lib.ptr(delta), _lib.ptr(dqkv), B, L, H, _lib.stream()), "ca_bwd")
    assert _guard_ok(dqkv, B * L) and _untouched(delta)              # delta stays in LDS at every dtype
    dq, dk, dv = R.split_qkv(_cpu64(dqkv[:B * L]), B, L, H)
    return dq, dk, dv, dqkv


def _sub16(x, dname):
    if dname != "f16":
        return torch.zeros_like(x)
    return (x.abs() < 2.0 ** -13).to(F64) * 2.0 ** -25


def _check_ca_fwd(tag, dname, q, k, v, o_got, lse_got):
    """test_gpu_encoder_kernels._check_attn_fwd with every sum restricted to the support j <= i (L <= 77: no streamed
    term): score ds_ij = NS u (|q| . |k|) / 8, exponent fma(s, c2, -(m c2)): 5 u smax, p: rho_ij = ds_ij + ds_i* + 5 u
    smax + TRANS, flushed below 2^-126; N = P V: sum_j p |v| (rho + u_T + L u) (+ the f16 subnormal term), S = sum p:
    sum_j p (rho + L u); o: (dN + |o| dS) / S + 5 u |o| + ulp_T / 2; lse: ds_i* + dS / S + TRANS |log S| + u |lse|."""
    dt = DT[dname]
    L = q.shape[2]
    f = TR.attention_causal_fwd(q, k, v)
    mk = f["mask"].to(F64)
    ds = NS * U * (q.abs() @ k.abs().transpose(-1, -2)) / 8.0 * mk
    smax = (f["s"].abs() * mk).max(-1, keepdim=True).values
    rho = ds + ds.max(-1, keepdim=True).values + 5 * U * smax + TRANS
    p, S = f["p"], f["l"]
    dN = ((p * (rho + UT[dname] + L * U) + _sub16(p, dname) + 2.0 ** -126) * mk) @ v.abs()
    dS = (p * (rho + L * U)).sum(-1, keepdim=True)
    bound = (dN + f["o"].abs() * dS) / S + 5 * U * f["o"].abs() + 0.5 * BR.ulp(f["o"], dt)
    assert bool(torch.isfinite(o_got).all()) and bool(torch.isfinite(lse_got).all())
    _report(f"{tag}.out", (o_got - f["o"]).abs(), bound)
    lse = f["lse"]
    lb = (ds.max(-1).values + (dS / S).squeeze(-1) + TRANS * torch.log(S).abs().squeeze(-1) + U * lse.abs()
          + 0.5 * BR.ulp(lse, torch.float32))
    _report(f"{tag}.lse", (lse_got - lse).abs(), lb)
    return f


def _check_ca_bwd(tag, dname, q, k, v, do, o, lse, got):
    """test_gpu_encoder_kernels._check_attn_bwd on the support j <= i: P = exp2(fma(s, c2, -(lse log2 e))): rho_ij =
    ds_ij + 3 u (|s_ij| + |lse_i|) + TRANS; dP and delta are 64-term products, E_ij = (NS + 1) u ((|dO| . |v|)_ij +
    sum|dO o|_i) + u |dP - delta|; dS: P (rho |dP - delta| + E + u |dP - delta|); dQ: sum_j (ddS + u_T |dS| + sub) |k|
    / 8 + L u sum_j |dS k| / 8 + u |dQ|, dK alike over the queries; dV: sum_i (P (rho + u_T) + sub) |dO| + L u sum_i P
    |dO|; each + ulp_T / 2."""
    dt = DT[dname]
    L = q.shape[2]
    r = TR.attention_causal_bwd(q, k, v, do, o, lse)
    mk = r["mask"].to(F64)
    dq, dk, dv = got
    uT = UT[dname]
    ds = NS * U * (q.abs() @ k.abs().transpose(-1, -2)) / 8.0
    rho = ds + 3 * U * (r["s"].abs() + lse.abs()[..., None]) + TRANS
    adv = do.abs() @ v.abs().transpose(-1, -2)
    ado = (do * o).abs().sum(-1)
    diff = (r["dP"] - r["delta"][..., None]).abs()
    E = (NS + 1) * U * (adv + ado[..., None]) + U * diff
    P = r["P"]
    ddS = (P * (rho * diff + E + U * diff) + 2.0 ** -126 * diff) * mk
    w = (ddS + uT * r["dS"].abs() + _sub16(r["dS"], dname)) * mk
    bq = (w @ k.abs() + L * U * (r["dS"].abs() @ k.abs())) / 8.0 + U * r["dq"].abs() + 0.5 * BR.ulp(r["dq"], dt)
    bk = ((w.transpose(-1, -2) @ q.abs() + L * U * (r["dS"].abs().transpose(-1, -2) @ q.abs())) / 8.0 + U * r["dk"].abs()
          + 0.5 * BR.ulp(r["dk"], dt))
    wp = (P * (rho + uT) + _sub16(P, dname) + 2.0 ** -126) * mk
    bv = wp.transpose(-1, -2) @ do.abs() + L * U * (P.transpose(-1, -2) @ do.abs()) + 0.5 * BR.ulp(r["dv"], dt)
    for t in (dq, dk, dv):
        assert bool(torch.isfinite(t).all())
    _report(f"{tag}.dq", (dq - r["dq"]).abs(), bq)
    _report(f"{tag}.dk", (dk - r["dk"]).abs(), bk)
    _report(f"{tag}.dv", (dv - r["dv"]).abs(), bv)


def _ca_fwd_then_bwd(tag, dname, q, k, v, do, B, L, H):
    """The forward per element; then the backward fed out = the float64 forward rounded once to T and lse rounded to
    f32 (as test_gpu_encoder_kernels._fwd_then_bwd).  Both kernels run twice: bit-identical outputs."""
    dt = DT[dname]
    qkv = R.pack_qkv(q, k, v).to(dt)
    o_got, lse_got, out_dev, lse_dev = _ca_fwd(dname, qkv, B, L, H)
    f = _check_ca_fwd(tag, dname, q, k, v, o_got, lse_got)
    _, _, out2, lse2 = _ca_fwd(dname, qkv, B, L, H)
    assert torch.equal(out_dev, out2) and torch.equal(lse_dev, lse2)
    _, _, out3, lse3 = _ca_fwd(dname, qkv, B, L, H, with_lse=False)
    assert torch.equal(out_dev, out3) and _untouched(lse3)
    o_in = R.unheads(f["o"]).to(dt)
    lse_in = f["lse"].to(torch.float32).contiguous()
    dout = R.unheads(do).to(dt)
    got = _ca_bwd(dname, qkv, dout, o_in, lse_in, B, L, H)
    _check_ca_bwd(tag, dname, q, k, v, do, R.heads(o_in, B, L, H), lse_in.to(F64), got[:3])
    again = _ca_bwd(dname, qkv, dout, o_in, lse_in, B, L, H)
    assert torch.equal(got[3], again[3])


@pytest.mark.parametrize("B,H,L", CA_SHAPES)
@pytest.mark.parametrize("dname", DNAMES)
def test_causal_attention_random(dname, B, H, L):
    """Random normal inputs (std 1.5: scores of std ~2), forward and backward per element."""
    dt = DT[dname]
    q, k, v = (R.rounded(_randn((B, H, L, 64), s) * 1.5, dt) for s in (1, 2, 3))
    do = R.rounded(_randn((B, H, L, 64), 4), dt)
    _ca_fwd_then_bwd("ca_random", dname, q, k, v, do, B, L, H)


@pytest.mark.parametrize("B,H,L", CA_SHAPES)
@pytest.mark.parametrize("dname", DNAMES)
def test_causal_attention_selection(dname, B, H, L):
    """_enc_refs.selection_inputs under the causal mask: scores of 128, 0 and -128, so a query whose matching keys lie
    inside its support attends to them alone (every other probability underflows to 0) and one whose matches are all
    masked spreads over its zero-score keys; sparse +-1 values and dout.  One misplaced key, value, query row, head or
    mask bit moves whole probabilities."""
    dt = DT[dname]
    qkv64, dout64, _ = R.selection_inputs(B, L, H, 5)
    q, k, v = R.split_qkv(qkv64, B, L, H)
    _ca_fwd_then_bwd("ca_select", dname, q, k, v, R.heads(dout64, B, L, H), B, L, H)


@pytest.mark.parametrize("dname", DNAMES)
def test_causal_attention_is_causal(dname):
    """Rewriting the Q / K / V rows j > i leaves out[i] and lse[i] bit-identical; rewriting the dout rows i < j leaves
    dK[j] and dV[j] bit-identical (L = 37: two whole tiles and a ragged one)."""
    dt = DT[dname]
    B, H, L, i0 = 2, 3, 37, 20
    q, k, v = (R.rounded(_randn((B, H, L, 64), s) * 1.5, dt) for s in (1, 2, 3))
    q2, k2, v2 = (t.clone() for t in (q, k, v))
    for t, s in ((q2, 11), (k2, 12), (v2, 13)):
        t[:, :, i0 + 1:] = R.rounded(_randn((B, H, L - i0 - 1, 64), s) * 3, dt)
    _, _, o_a, l_a = _ca_fwd(dname, R.pack_qkv(q, k, v).to(dt), B, L, H)
    _, _, o_b, l_b = _ca_fwd(dname, R.pack_qkv(q2, k2, v2).to(dt), B, L, H)
    rows = (torch.arange(B * L) % L <= i0).cuda()
    assert torch.equal(o_a[:B * L][rows], o_b[:B * L][rows]) and not torch.equal(o_a[:B * L][~rows], o_b[:B * L][~rows])
    la, lb = l_a[:B * H * L].view(B, H, L), l_b[:B * H * L].view(B, H, L)
    assert torch.equal(la[..., :i0 + 1], lb[..., :i0 + 1])
    f = TR.attention_causal_fwd(q, k, v)
    o_in, lse_in = R.unheads(f["o"]).to(dt), f["lse"].to(torch.float32).contiguous()
    do = R.rounded(_randn((B, H, L, 64), 4), dt)
    do2 = do.clone()
    do2[:, :, :i0] = R.rounded(_randn((B, H, i0, 64), 14) * 3, dt)
    qkv = R.pack_qkv(q, k, v).to(dt)
    g_a = _ca_bwd(dname, qkv, R.unheads(do).to(dt), o_in, lse_in, B, L, H)[3][:B * L].view(B, L, 3, H * 64)
    g_b = _ca_bwd(dname, qkv, R.unheads(do2).to(dt), o_in, lse_in, B, L, H)[3][:B * L].view(B, L, 3, H * 64)
    assert torch.equal(g_a[:, i0:, 1:], g_b[:, i0:, 1:]) and not torch.equal(g_a[:, :i0, 1:], g_b[:, :i0, 1:])


# ================================================================================================ LayerNorm, D = 512
D = 512
# (M, rows_per_group, group_stride, group_offset); rpg = 0 is the identity.  M = 1, 5, 63, 65: the last workgroup of
# four rows is partial; 1232 = 16 prompts x 77 tokens.  (1232, 77, 80, 2) and (61, 9, 14, 3): mapped rows, the second
# with a last group of 61 % 9 = 7 rows.
LN_CASES = [(1, 0, 0, 0), (5, 0, 0, 0), (63, 0, 0, 0), (64, 0, 0, 0), (65, 0, 0, 0), (1232, 0, 0, 0),
            (5, 1, 7, 6), (61, 9, 14, 3), (1232, 77, 80, 2)]
LN_M = [1, 5, 63, 64, 65, 1232]


def _ln_inputs(M, rpg, gs, go):
    """test_gpu_encoder_kernels._ln_inputs at D = 512: every source row its own offset and scale, mapped row 1
    constant (variance 0), mapped row 2 of magnitude 1e4 with spread 1."""
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
    """mean: one tree of depth at most 10 (2 float4 a lane: 2 + 2, six butterfly levels) and the product with 1 / 512:
    charged 12 u mean|x| as at D = 768.  variance: x - mean, the square, the same tree and product, + eps: 16 u, shifted
    by dmean^2.  rstd = 1 / sqrtf(.): half the variance's relative error plus two TRANS and the half-ulp of the result."""
    dmean = 12 * U * f["xs"].abs().mean(1)
    rho = 0.5 * (16 * U * f["var"] + dmean ** 2) / (f["var"] + EPS) + 9 * U
    return dmean, rho


@pytest.mark.parametrize("M,rpg,gs,go", LN_CASES)
@pytest.mark.parametrize("dname", DNAMES)
def test_layernorm512_fwd(dname, M, rpg, gs, go):
    """ebc_layernorm_fwd at D = 512: y = ((x - mean) * rstd) * gamma + beta per element (k = 4 on A = |xhat gamma| +
    |beta|, plus |gamma| rstd dmean + |xhat gamma| rho_rstd), mean and rstd per row; two launches bit-identical."""
    dt = DT[dname]
    L = _lib.lib()
    x, gamma, beta, rows, N = _ln_inputs(M, rpg, gs, go)
    f = R.layernorm_fwd(x, gamma, beta, M, rpg, gs, go, EPS)
    dmean, rho = _ln_stat_bounds(f)
    xg = (f["xs"] - f["mean"][:, None]) * f["rstd"][:, None] * gamma
    A = xg.abs() + beta.abs()
    extra = gamma.abs() * (f["rstd"] * dmean)[:, None] + xg.abs() * rho[:, None]
    px, pg, pb = hold(x, True), hold(gamma, True), hold(beta, True)
    code = _lib.dtype_code(dt)
    prev = None
    for _ in range(2):
        out, outf = _guarded(M, D, dt), _guarded(M, D, torch.float32)
        mean, rstd = _vec(M), _vec(M)
        _lib.check(L.ebc_layernorm_fwd(code, px, rpg, gs, go, pg, pb, _lib.ptr(out), _lib.ptr(outf), _lib.ptr(mean),
                                       _lib.ptr(rstd), M, D, _lib.stream()), "ln_fwd")
        assert all(_guard_ok(t, M) for t in (out, outf, mean, rstd))
        if prev is not None:
            assert all(torch.equal(a, b) for a, b in zip(prev, (out, outf, mean, rstd)))
        prev = (out, outf, mean, rstd)
    _elem("ln512_fwd.out", out[:M], f["y"], A, 4, dt, extra)
    _elem("ln512_fwd.out_f32", outf[:M], f["y"], A, 4, torch.float32, extra)
    _report("ln512_fwd.mean", (_cpu64(mean[:M]) - f["mean"]).abs(), dmean + U * f["mean"].abs() + 2.0 ** -149)
    _report("ln512_fwd.rstd", (_cpu64(rstd[:M]) - f["rstd"]).abs(), f["rstd"] * rho)


@pytest.mark.parametrize("M,rpg,gs,go", LN_CASES)
@pytest.mark.parametrize("dname", DNAMES)
def test_layernorm512_bwd(dname, M, rpg, gs, go):
    """ebc_layernorm_bwd at D = 512: dx = rstd * ((g - s1) - xhat * s2) + dx_in from the mean / rstd it is handed, k = 8
    on A = rstd (|g| + |s1| + |xhat s2|) + |dx_in|; s1 within 13 u mean|g|, s2 within 16 u mean|g xhat|.  dy as T and
    as f32; rows outside the groups and the guards keep their sentinel; two launches bit-identical."""
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
        sent = torch.full((N, D), SENT, dtype=F64)
        b = R.layernorm_bwd(dy.to(F64), x, mean, rstd, gamma, dx_in, M, rpg, gs, go, sent)
        rs = rstd[:, None]
        A = rs * (b["g"].abs() + b["s1"].abs() + (b["xh"] * b["s2"]).abs()) + b["din"].abs()
        ds1 = 13 * U * b["g"].abs().mean(1, keepdim=True)
        ds2 = 16 * U * (b["g"] * b["xh"]).abs().mean(1, keepdim=True)
        extra = rs * (ds1 + b["xh"].abs() * ds2)
        prev = None
        for _ in range(2):
            dx, dxt = _guarded(N, D, torch.float32), _guarded(N, D, dt)
            _lib.check(L.ebc_layernorm_bwd(code, dy_f32, pdy, px, rpg, gs, go, pm, pr, pg, pdi, _lib.ptr(dx), _lib.ptr(dxt),
                                           M, D, _lib.stream()), "ln_bwd")
            if prev is not None:
                assert torch.equal(prev[0], dx) and torch.equal(prev[1], dxt)
            prev = (dx, dxt)
        assert _untouched(dx[other.cuda()]) and _untouched(dxt[other.cuda()])
        _elem(f"ln512_bwd[dy_f32={dy_f32}].dx_out", dx[:N][rows.cuda()], b["dense"], A, 8, torch.float32, extra)
        _elem(f"ln512_bwd[dy_f32={dy_f32}].dx_out_t", dxt[:N][rows.cuda()], b["dense"], A, 8, dt, extra)


# ================================================================================================ sums over rows
def _depth(M):
    """colsum_kernel's longest chain: ceil(M / 8) rows in a group, then the eight partials."""
    return -(-M // 8) + 8


@pytest.mark.parametrize("M", LN_M)
@pytest.mark.parametrize("dname", DNAMES)
def test_layernorm_param_grad(dname, M):
    """ebc_layernorm_param_grad at D = 512 and 768: dgamma = sum_r dy xhat, dbeta = sum_r dy, to test_head_bwd's bound
    for sums over rows, k u sum|terms| + half an ulp: k = depth for dbeta, depth + 3 for dgamma (x - mean, the product
    with rstd, the product with dy).  dy as T and as f32; two launches bit-identical."""
    dt = DT[dname]
    L = _lib.lib()
    code = _lib.dtype_code(dt)
    for Dn in (512, 768):
        x = (_randn((M, Dn), 1) * 2 + 0.5).to(torch.float32).to(F64)
        mean = x.mean(1).to(torch.float32).to(F64)
        rstd = (1.0 / torch.sqrt(x.var(1, unbiased=False) + EPS)).to(torch.float32).to(F64)
        px, pm, pr = hold(x, True), hold(mean, True), hold(rstd, True)
        for dy_f32 in (0, 1):
            dyt = torch.float32 if (dy_f32 or dt == torch.float32) else dt
            dy = _randn((M, Dn), 7).to(dyt)
            f = TR.ln_param_grad(dy, x, mean, rstd)
            pdy = hold(dy)
            prev = None
            for _ in range(2):
                dg, db = _vec(Dn), _vec(Dn)
                _lib.check(L.ebc_layernorm_param_grad(code, dy_f32, pdy, px, pm, pr, _lib.ptr(dg), _lib.ptr(db), M, Dn,
                                                      _lib.stream()), "ln_param_grad")
                assert _guard_ok(dg, Dn) and _guard_ok(db, Dn)
                if prev is not None:
                    assert torch.equal(prev[0], dg) and torch.equal(prev[1], db)
                prev = (dg, db)
            tag = f"ln_param_grad[{Dn},dy_f32={dy_f32}]"
            _elem(f"{tag}.dgamma", dg[:Dn], f["dgamma"], f["terms"].abs().sum(0), _depth(M) + 3, torch.float32)
            _elem(f"{tag}.dbeta", db[:Dn], f["dbeta"], dy.to(F64).abs().sum(0), _depth(M), torch.float32)


@pytest.mark.parametrize("M", LN_M)
@pytest.mark.parametrize("dname", DNAMES)
def test_colsum(dname, M):
    """ebc_colsum over [M][N], N = 512, 1536, 2048 (the four bias gradients) and 40 (a partial block of columns): depth u
    sum|a| + half an ulp; the input as T and as f32; two launches bit-identical."""
    dt = DT[dname]
    L = _lib.lib()
    code = _lib.dtype_code(dt)
    for N in (512, 1536, 2048, 40):
        for in_f32 in (0, 1):
            a = _randn((M, N), 3).to(torch.float32 if in_f32 else dt)
            pa = hold(a)
            prev = None
            for _ in range(2):
                out = _vec(N)
                _lib.check(L.ebc_colsum(code, in_f32, pa, _lib.ptr(out), M, N, _lib.stream()), "colsum")
                assert _guard_ok(out, N)
                assert prev is None or torch.equal(prev, out)
                prev = out
            _elem(f"colsum[{N},in_f32={in_f32}]", out[:N], a.to(F64).sum(0), a.to(F64).abs().sum(0), _depth(M), torch.float32)


@pytest.mark.parametrize("dname", DNAMES)
def test_row_sums_dyadic(dname):
    """Small integers: every partial sum is exact in f32, so the results equal the float64 sums bit for bit (mean 0,
    rstd 1 handed over, so xhat = x)."""
    dt = DT[dname]
    L = _lib.lib()
    code = _lib.dtype_code(dt)
    g = torch.Generator().manual_seed(1)
    for M in (5, 65, 1232):
        a = torch.randint(-8, 9, (M, 512), generator=g).to(F64)
        x = torch.randint(-4, 5, (M, 512), generator=g).to(F64)
        out, dg, db = _vec(512), _vec(512), _vec(512)
        _lib.check(L.ebc_colsum(code, 0, hold(a.to(dt)), _lib.ptr(out), M, 512, _lib.stream()), "colsum")
        _exact(out[:512], a.sum(0), torch.float32)
        _lib.check(L.ebc_layernorm_param_grad(code, 0, hold(a.to(dt)), hold(x, True), hold(torch.zeros(M), True),
                                              hold(torch.ones(M), True), _lib.ptr(dg), _lib.ptr(db), M, 512, _lib.stream()),
                   "ln_param_grad")
        _exact(dg[:512], (a * x).sum(0), torch.float32)
        _exact(db[:512], a.sum(0), torch.float32)


# ================================================================================================ embedding
VOCAB = 49408


def _ids(kind, NB, Lt, vocab, seed=2):
    g = torch.Generator().manual_seed(seed)
    if kind == "one":                                    # one id owns every row
        return torch.full((NB, Lt), 320, dtype=torch.int32)
    if kind == "distinct":
        return torch.randperm(vocab, generator=g)[:NB * Lt].view(NB, Lt).to(torch.int32)
    ids = torch.randint(0, vocab, (NB, Lt), generator=g).to(torch.int32)       # "prompts": shared head, vocab's last id
    ids[:, 0] = vocab - 2
    ids[:, Lt - 1] = vocab - 1
    if Lt > 3:
        ids[:, 1:3] = torch.tensor([997, 631], dtype=torch.int32)
    return ids


@pytest.mark.parametrize("NB,Lt", [(1, 1), (3, 14), (5, 77), (16, 77)])
def test_text_embed_fwd_is_exact(NB, Lt):
    """x = token_embedding[ids] + positional_embedding[t]: one f32 addition, so bit-equal to the f32 sum."""
    L = _lib.lib()
    vocab = 1000
    tok, pos = _randn((vocab, D), 1).float(), _randn((77, D), 2).float()
    ids = _ids("prompts", NB, Lt, vocab)
    x = _Framed(NB * Lt, D, torch.float32)
    _lib.check(L.ebc_text_embed_fwd(hold(tok), hold(pos), hold(ids), _lib.ptr(x.mid), NB, Lt, D, vocab, _lib.stream()),
               "embed_fwd")
    assert x.ok()
    assert torch.equal(x.mid.cpu(), TR.embed_fwd(tok, pos, ids).reshape(NB * Lt, D))


@pytest.mark.parametrize("kind,NB,Lt,vocab", [("one", 16, 77, 1000), ("distinct", 16, 77, 2000), ("prompts", 3, 14, 1000),
                                               ("prompts", 1, 1, 1000), ("prompts", 5, 77, VOCAB)])
def test_text_embed_bwd(kind, NB, Lt, vocab):
    """The dense gradients on NaN-poisoned, sentinel-framed outputs: a token row is the sum of its dx rows in list order
    (count u sum|terms| + half an ulp), the rows of unused ids and the dpos rows >= Lt are exact zeros (which proves the
    zero fill: no NaN survives), dpos[t] sums NB rows; two launches bit-identical."""
    L = _lib.lib()
    ids = _ids(kind, NB, Lt, vocab)
    ix = TR.inverted_index(ids.numpy())
    dx = _randn((NB, Lt, D), 3).float()
    f = TR.embed_bwd(dx, ids, vocab, 77)
    pdx = hold(dx)
    pu, po, pr = (hold(torch.from_numpy(ix[k])) for k in ("uniq", "offs", "rows"))
    nu = len(ix["uniq"])
    prev = None
    for _ in range(2):
        dtok = _Framed(vocab, D, torch.float32)
        dpos = _Framed(77, D, torch.float32)
        dtok.mid.fill_(float("nan"))
        dpos.mid.fill_(float("nan"))
        _lib.check(L.ebc_text_embed_bwd(pdx, pu, po, pr, nu, _lib.ptr(dtok.mid), _lib.ptr(dpos.mid), NB, Lt, 77, D, vocab,
                                        _lib.stream()), "embed_bwd")
        assert dtok.ok() and dpos.ok()
        if prev is not None:
            assert torch.equal(prev[0], dtok.mid) and torch.equal(prev[1], dpos.mid)
        prev = (dtok.mid.clone(), dpos.mid.clone())
    got_t, got_p = dtok.mid.cpu(), dpos.mid.cpu()
    unused = f["count"] == 0
    assert int(unused.sum()) == vocab - nu
    assert bool((got_t[unused] == 0).all()) and bool((got_p[Lt:] == 0).all())
    used = ~unused
    cnt = f["count"][used].to(F64)[:, None]
    _report(f"embed_bwd[{kind}].dtok", (got_t[used].to(F64) - f["dtok"][used]).abs(),
            cnt * U * f["atok"][used] + 0.5 * BR.ulp(f["dtok"][used], torch.float32))
    _report(f"embed_bwd[{kind}].dpos", (got_p[:Lt].to(F64) - f["dpos"][:Lt]).abs(),
            NB * U * f["apos"][:Lt] + 0.5 * BR.ulp(f["dpos"][:Lt], torch.float32))
