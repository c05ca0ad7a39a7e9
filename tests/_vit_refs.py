"""The encoder as ebc_vit_forward / ebc_vit_backward execute it (csrc/vit.hip), one stage at a time: a plain-Python mirror
of the workspace layout, float64 restatements of every stage from the operands as the kernel received them (read back
from the workspace after the call), and the per-element bounds tests/test_gpu_vit_stages.py holds the stages to.

Everything is plain torch on whatever device its operands live on; tests/test_vit_refs_cpu.py pins the mirror to
ebc_vit_workspace_bytes_p and the references to torch's own float64 ops and autograd on the CPU.

Error model: tests/_gemm_refs.py (u = 2^-24; 2 units per K step of |A|.|B|^T, one unit per add / fma, ulp_T / 2 + 2 d
for a 16-bit store, gelu_arith / gelu_grad_arith) and, for the LayerNorm arithmetic, the counts of
tests/test_gpu_encoder_kernels.py: a sum is charged depth * u * sum|terms| with depth its longest chain of additions,
and the hardware division, sqrtf and reciprocal 2 f32 ulp each (TRANS = 4 u).  Each stage is checked from the stored
operands of that stage alone, so no bound models a chain of 16-bit roundings; the one exception (a LayerNorm launch whose
16-bit output feeds a product and is overwritten later) is handled by `flip_mask`: the launch's f32 value is within a
few u of the float64 one, so its rounding to T can differ from the reference's only where the reference lies that close
to a rounding boundary, and only there one ulp_T of the operand is charged through the product.
"""
import math

import torch

import _enc_refs as ER
import _gemm_refs as GR

F64 = torch.float64
U = GR.U
TRANS = 4 * U
WIDTH, HEADS, MLP, QKVW = 768, 12, 3072, 2304
LN_PMAX, LN_PMAX_B = 16, 32                 # kernels.h GEMM_LN_PMAX / GEMM_LN_PMAX_B
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
FLAG_FULL_LAYER0, FLAG_NO_LN_FOLD = 1, 2    # include/ebc_hip.h EBC_VIT_BWD_*
WGN = 2                                     # wave columns of every tile pick_cfg names (gemm.hip Tile<>)


def align_up(x):
    return (x + 255) & ~255


def geometry(B, H, W, patch, nv):
    G = (H // patch) * (W // patch)
    L = 1 + nv + G
    return G, L, B * L


# ------------------------------------------------------------------------------------------------ workspace mirror
def carve(B, L, G, KP, layers, es, training, parts_out, parts_proj, parts_gelu):
    """Byte offsets of vit.hip's carve().  es: bytes of the compute type; the part counts are inputs (N / BN * WGN of
    the producing product's tile, 0 for f32).  Returns (offsets, total): offsets["X"] is a list of layers + 1,
    offsets["layer"] a list of per-layer dicts, every other name a byte offset (None where carve() leaves nullptr)."""
    M = B * L
    off = [0]

    def take(nbytes):
        o = off[0]
        off[0] += align_up(nbytes)
        return o
    lay = {"X": [None] * (layers + 1), "layer": []}
    for l in range(layers + 1):
        lay["X"][l] = take(M * WIDTH * 4) if (training or l < 2) else lay["X"][l & 1]
    nsave = layers if training else 1
    for l in range(layers):
        if l < nsave:
            s = {}
            s["X1"] = take(M * WIDTH * 4)
            for k in ("m1", "r1", "m2", "r2"):
                s[k] = take(M * 4)
            s["lse"] = take(B * HEADS * L * 4)
            s["QKV"] = take(M * QKVW * es)
            s["O"] = take(M * WIDTH * es)
            s["A"] = take(M * MLP * es)
        else:
            s = lay["layer"][0]
        lay["layer"].append(s)
    lay["H"] = take(M * WIDTH * es)
    lay["G"] = take(M * MLP * es)
    lay["patch_t"] = take(B * G * KP * es)
    lay["patch_f"] = take(B * G * WIDTH * 4)
    lay["mpost"] = take(B * G * 4)
    lay["rpost"] = take(B * G * 4)
    for k in ("dXa", "dXb", "delta", "dXt", "dH", "dA", "dO", "dQKV", "vpt_rows", "bpart", "rpart"):
        lay[k] = None
    if training:
        lay["dXa"] = take(M * WIDTH * 4)
        lay["dXb"] = take(M * WIDTH * 4)
        lay["delta"] = take(B * HEADS * L * 4)
        lay["dXt"] = take(M * WIDTH * es)
        lay["dH"] = take(M * WIDTH * es)
        lay["dA"] = take(M * MLP * es)
        lay["dO"] = take(M * WIDTH * es)
        lay["dQKV"] = take(M * QKVW * es)
        NV = L - 1 - G
        if NV > 0:
            lay["vpt_rows"] = take(layers * B * NV * WIDTH * 4)
    if es != 4 and training and parts_gelu <= LN_PMAX_B:
        lay["bpart"] = take(M * parts_gelu * 2 * 4)
    if es != 4:
        lay["rpart"] = take(M * max(parts_out, parts_proj) * 2 * 4)
    return lay, off[0]


def tile_of(lib, dtcode, M, N, K):
    """(cfg id, BM, BN) ebc_gemm_tile_config reports for a product (host only)."""
    import ctypes
    out = (ctypes.c_int * 3)()
    cfg = lib.ebc_gemm_tile_config(dtcode, M, N, K, out)
    return cfg, out[0], out[1]


def part_counts(lib, dtcode, M):
    """(parts_out, parts_proj, parts_gelu) of vit.hip's carve(): one pair per tile column and wave column."""
    if dtcode == 0:
        return 0, 0, 0
    return tuple(N // tile_of(lib, dtcode, M, N, K)[2] * WGN for N, K in ((WIDTH, WIDTH), (WIDTH, MLP), (MLP, WIDTH)))


class Workspace:
    """Typed views of a workspace byte tensor by the mirror's offsets."""

    def __init__(self, ws, B, L, G, KP, layers, dt, training, parts):
        self.ws, self.B, self.L, self.G, self.KP, self.layers, self.dt = ws, B, L, G, KP, layers, dt
        self.M, self.NV = B * L, L - 1 - G
        self.parts_out, self.parts_proj, self.parts_gelu = parts
        self.es = 4 if dt == torch.float32 else 2
        self.lay, self.total = carve(B, L, G, KP, layers, self.es, training, *parts)

    def _view(self, off, shape, dt):
        n = int(math.prod(shape)) * (4 if dt == torch.float32 else 2)
        return self.ws[off:off + n].view(dt).view(shape)

    def get(self, name, l=None):
        M, B, L, G, T, f = self.M, self.B, self.L, self.G, self.dt, torch.float32
        per_layer = {"X1": ((M, WIDTH), f), "m1": ((M,), f), "r1": ((M,), f), "m2": ((M,), f), "r2": ((M,), f),
                     "lse": ((B, HEADS, L), f), "QKV": ((M, QKVW), T), "O": ((M, WIDTH), T), "A": ((M, MLP), T)}
        once = {"H": ((M, WIDTH), T), "G": ((M, MLP), T), "patch_t": ((B * G, self.KP), T),
                "patch_f": ((B * G, WIDTH), f), "mpost": ((B * G,), f), "rpost": ((B * G,), f),
                "dXa": ((M, WIDTH), f), "dXb": ((M, WIDTH), f), "delta": ((B, HEADS, L), f), "dXt": ((M, WIDTH), T),
                "dH": ((M, WIDTH), T), "dA": ((M, MLP), T), "dO": ((M, WIDTH), T), "dQKV": ((M, QKVW), T),
                "vpt_rows": ((self.layers, B, max(self.NV, 1), WIDTH), f), "bpart": ((M, max(self.parts_gelu, 1), 2), f),
                "rpart": ((M, max(self.parts_out, self.parts_proj, 1), 2), f)}
        if name == "X":
            return self._view(self.lay["X"][l], (M, WIDTH), f)
        if name in per_layer:
            shape, dt = per_layer[name]
            return self._view(self.lay["layer"][l][name], shape, dt)
        shape, dt = once[name]
        assert self.lay[name] is not None, name
        return self._view(self.lay[name], shape, dt)


# ------------------------------------------------------------------------------------------------ small pieces
def rn(x, dt):
    """x rounded once to dt, as float64."""
    return x.to(dt).to(F64)


def held(ref, d, t):
    """(ref, bound) of a value computed within d in f32 and stored as t (_gemm_refs: ulp_T / 2 + 2 d for 16 bits)."""
    if t == torch.float32:
        return ref, d
    return ref, 0.5 * GR.ulp(ref, t) + 2.0 * d


def binade_aware(ref, bound, dt):
    """A bound of the form d + ulp_T(ref) / 2 (a value computed within d of ref, then rounded to T) with the rounding
    term taken where the computed value can lie: ulp_T(|ref| + d) / 2.  It differs from the given bound only where ref
    is within d below a power of two, where the computed value may fall into the binade above and round on a spacing
    twice as coarse."""
    u = GR.ulp(ref, dt)
    d = torch.clamp(bound - 0.5 * u, min=0.0)
    return bound + 0.5 * (GR.ulp(ref.abs() + d, dt) - u)


def prompt_rows(B, L, NV, device=None):
    """Rows r of [B][L] with 1 <= r % L <= NV, crop-major."""
    r = torch.arange(B * L, device=device)
    return r[(r % L >= 1) & (r % L <= NV)]


def prompt_values(vpt, bstride, B, NV):
    """[B * NV][768]: the rows the prompt tensor (shared [NV][768], or per crop [B][NV][768]) puts at prompt_rows."""
    v = vpt.reshape(-1, WIDTH)
    if bstride == 0:
        return v[:NV].repeat(B, 1)
    assert bstride == NV * WIDTH
    return v[:B * NV]


def flip_mask(y, d, dt):
    """1.0 where rounding to dt of a value within d of the float64 y may differ from rounding y itself: y lies within d
    of the midpoint of two neighbouring dt values (spacing ulp_dt(y); the finer spacing below a power of two only moves
    midpoints onto multiples of ulp / 4, covered by also testing the half spacing)."""
    if dt == torch.float32:
        return torch.zeros_like(y)
    m = torch.zeros_like(y, dtype=torch.bool)
    for sp in (GR.ulp(y, dt), 0.5 * GR.ulp(y, dt)):
        frac = torch.remainder(y.abs() / sp, 1.0)
        m |= (frac - 0.5).abs() * sp <= d
    return m.to(F64)


# ------------------------------------------------------------------------------------------------ LayerNorm statistics
def stats64(x):
    x = x.to(F64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def launch_stat_bounds(x, mean, var):
    """vit_misc.hip ln_row (test_gpu_encoder_kernels._ln_stat_bounds): mean within 12 u mean|x| (a tree of depth 11 and
    the product with 1 / 768), the two-pass variance within 16 u var + dmean^2, rstd = 1 / sqrtf(.): half of that
    relative plus two TRANS and the result's half ulp (9 u).  Returns (dmean, rho), rho relative to rstd."""
    dmean = 12 * U * x.to(F64).abs().mean(1)
    rho = 0.5 * (16 * U * var + dmean ** 2) / (var + EPS) + 9 * U
    return dmean, rho


def fold_depth(bn, parts):
    """Longest chain of additions of gemm.hip's row statistics: a lane adds its bn / (4 WGN) values of a part one after
    the other, the part's 4 lanes meet by two lane swaps (RESID / GELU' epilogue); the consumer's lane adds the two
    pairs of a float4 (1), its ceil(parts / 8) float4 one after the other, and two lane swaps again."""
    return bn // (4 * WGN) + 2 + 1 + -(-parts // 8) + 2


def fold_stat_bounds(x, mean, var, bn, parts):
    """EPI_LN's statistics from the RESID partials of the stored f32 rows x: mean = s1 / 768 with s1 a sum of depth
    `fold_depth` and the hardware division (TRANS); var = s2 / 768 - mean * mean in f32, s2 the same sum of fma'd
    squares (one more unit a term): (depth + 1 + 4) u E[x^2], the square of the mean (1 u mean^2 + 2 |mean| dmean), the
    subtraction and the + eps (1 u each of var + eps) -- the cancellation term c u E[x^2] / (var + eps) -- and
    rstd = 1 / sqrtf(.) as in the launch (9 u)."""
    x = x.to(F64)
    dep = fold_depth(bn, parts)
    dmean = dep * U * x.abs().mean(1) + TRANS * mean.abs()
    e2 = (x * x).mean(1)
    dvar = (dep + 5) * U * e2 + U * mean ** 2 + 2 * mean.abs() * dmean + dmean ** 2 + 2 * U * (var + EPS)
    rho = 0.5 * dvar / (var + EPS) + 9 * U
    return dmean, rho


def fold_partials(x, bn):
    """[M][768 / bn * WGN][2] float64: the (sum, sum of squares) pair of part p = tile column * WGN + wave column, the
    columns [p * bn / WGN, (p + 1) * bn / WGN) of the row."""
    x = x.to(F64)
    w = bn // WGN
    xp = x.view(x.shape[0], x.shape[1] // w, w)
    return torch.stack([xp.sum(2), (xp * xp).sum(2)], 2)


def stats_from_partials(parts, K=WIDTH):
    """mean and rstd as EPI_LN rebuilds them, in float64."""
    mean = parts[:, :, 0].sum(1) / K
    var = torch.clamp(parts[:, :, 1].sum(1) / K - mean * mean, min=0.0)
    return mean, 1.0 / torch.sqrt(var + EPS)


# ------------------------------------------------------------------------------------------------ forward stages
def im2col(image, patch):
    """[B][3][H][W] -> [B * gh * gw][3 * patch^2], k = c * patch^2 + kh * patch + kw (conv1's weight order)."""
    B, C, H, W = image.shape
    gh, gw = H // patch, W // patch
    x = image.view(B, C, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B * gh * gw, C * patch * patch)


def embed(patch_f, cls, pos, g, b, vpt0, bstride, B, L, G, NV):
    """X_0 [B * L][768] from the stored patch_f: ln_pre(cls + pos[0]), the prompt rows, ln_pre(patch + pos[1 + p]);
    returns (ref, bound): the LayerNorm rows within the launch's bound (the statistics, 4 operations; e + q is one f32
    add, restated as the float64 sum rounded once), the prompt rows exact (bound 0)."""
    pf = patch_f.to(F64).view(B, G, WIDTH)
    pos, cls = pos.to(F64), cls.to(F64)
    tok = torch.cat([(cls + pos[0]).expand(B, 1, WIDTH), pf + pos[1:1 + G]], 1).reshape(B * (1 + G), WIDTH)
    tok32 = rn(tok, torch.float32)          # the kernel's e + q, rounded once
    mean, var, rstd = stats64(tok32)
    dmean, rho = launch_stat_bounds(tok32, mean, var)
    xg = (tok32 - mean[:, None]) * rstd[:, None] * g.to(F64)
    y = xg + b.to(F64)
    bound = 4 * U * (xg.abs() + b.to(F64).abs()) + g.to(F64).abs() * (rstd * dmean)[:, None] + xg.abs() * rho[:, None]
    # tok32 is the reference's own rounding of e + q: the kernel's is the same f32 add of the same operands (exact)
    ref = torch.zeros(B, L, WIDTH, dtype=F64, device=pf.device)
    bnd = torch.zeros_like(ref)
    keep = torch.ones(L, dtype=torch.bool, device=pf.device)
    keep[1:1 + NV] = False
    ref[:, keep] = y.view(B, 1 + G, WIDTH)
    bnd[:, keep] = bound.view(B, 1 + G, WIDTH)
    if NV:
        ref[:, 1:1 + NV] = prompt_values(vpt0, bstride, B, NV).to(F64).view(B, NV, WIDTH)
    return ref.view(B * L, WIDTH), bnd.view(B * L, WIDTH)


def ln_product(x, mean_s, rstd_s, gamma, beta, W, bias, dt, gelu=False):
    """A LayerNorm launch followed by a STORE / GELU product (layer 0's ln_1, and every LayerNorm of the unfolded path),
    from the stored f32 rows and the stored statistics.  The launch computes y = ((x - mean) rstd) gamma + beta within
    4 u A (A = |xhat gamma| + |beta|) and stores rn_T of it: equal to rn_T(y64) except where `flip_mask` allows one
    ulp_T.  The product of that operand is _gemm_refs' STORE / GELU from there."""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    xg = (x - mean_s.to(F64)[:, None]) * rstd_s.to(F64)[:, None] * gamma
    y = xg + beta
    dy = GR.units(4) * (xg.abs() + beta.abs())
    Hq = rn(y, dt)
    # (f32: the launch's own f32 value is the operand, within dy of y and so within dy + u |y| of rn_f32(y))
    dH = flip_mask(y, dy, dt) * GR.ulp(y, dt) if dt != torch.float32 else dy + U * y.abs()
    P, Sp = GR.product(Hq, W)
    out = GR.epilogue(GR.GELU if gelu else GR.STORE, P, Sp, WIDTH, dt, dt, bias=bias)
    extra = dH @ W.to(F64).abs().t()
    res = {}
    for k, (ref, bound) in out.items():
        slope = GR.GELU_SLOPE if (gelu and k == "C") else 1.0
        res[k] = (ref, bound + (2.0 if dt != torch.float32 else 1.0) * slope * extra)
    return res, Hq


def ln_fold_product(x, mean_s, rstd_s, Wf, s, bf, dt, gelu=False):
    """EPI_LN / EPI_LN_GELU from the stored f32 rows (the product's A operand is their 16-bit copy rn_T(x), written by
    the same RESID epilogue from the same f32 value) and the stored statistics: rstd (acc - mean s) + b' as
    fma(rstd, acc, -(rstd mean) s) + b'.  acc within 2 K u |A|.|B|^T; rstd mean, its product with s, the fma and the
    bias add round once each (4 u of S = rstd |A|.|B|^T + |rstd mean s| + |b'|)."""
    A = rn(x.to(F64), dt)
    P, Sp = GR.product(A, Wf)
    r, mu, s, bf = rstd_s.to(F64)[:, None], mean_s.to(F64)[:, None], s.to(F64)[None, :], bf.to(F64)[None, :]
    pre = r * (P - mu * s) + bf
    S = r * Sp + (r * mu * s).abs() + bf.abs()
    d = GR.units(2 * WIDTH + 4) * S
    if not gelu:
        return {"C": held(pre, d, dt)}
    dc = GR.GELU_SLOPE * d + U * GR.gelu_arith(pre)
    return {"aux": held(pre, d, dt), "C": held(GR.quick_gelu(pre), dc, dt)}


def resid_product(A, W, bias, resid, dt):
    """EPI_RESID with an f32 output: (ref, bound)."""
    P, Sp = GR.product(A, W)
    return GR.epilogue(GR.RESID, P, Sp, A.shape[1], dt, torch.float32, bias=bias, resid=resid)["C"]


def mlp_out(A_s, X1, w_proj, b_proj, dt):
    """X_l+1 from the stored pre-activation A = rn_T(pre): the kernel's G = rn_T(gelu(pre)) is within
    GELU_SLOPE ulp_T(A) / 2 (the pre-activation's rounding through |QuickGELU'| <= 1.1), the evaluation's own roundings
    (gelu_arith) and ulp_T(G) / 2 of gelu(A), per term, summed through |w_proj|; then the RESID product of the f64 G."""
    a = A_s.to(F64)
    g = GR.quick_gelu(a)
    dg = GR.GELU_SLOPE * 0.5 * GR.ulp(a, dt) + U * GR.gelu_arith(a)
    dg = dg + 0.5 * GR.ulp(g.abs() + dg, dt)             # (the spacing where the kernel's own value can lie)
    if dt == torch.float32:
        dg = U * GR.gelu_arith(a) + GR.units(1) * g.abs()
    ref, bound = resid_product(g, w_proj, b_proj, X1, dt)
    return ref, bound + dg @ w_proj.to(F64).abs().t(), g


def ln_post(X, gamma, beta, mpost, rpost, B, L, G, NV):
    """feat [B * G][768] f32 from the stored X_layers and the stored mpost / rpost (rows 1 + NV.. of every crop)."""
    rows = ER.ln_rows(B * G, G, L, 1 + NV).to(X.device)
    x = X.to(F64)[rows]
    xg = (x - mpost.to(F64)[:, None]) * rpost.to(F64)[:, None] * gamma.to(F64)
    return xg + beta.to(F64), GR.units(4) * (xg.abs() + beta.to(F64).abs()), x


# ------------------------------------------------------------------------------------------------ backward stages
def ln_bwd(dy, x, mean, rstd, gamma, dx_in):
    """rstd (g - mean(g) - xhat mean(g xhat)) + dx_in, g = dy gamma, dense rows; and the bound of
    test_gpu_encoder_kernels.test_layernorm_bwd: k = 8 on A = rstd (|g| + |s1| + |xhat s2|) + |dx_in|, s1 within
    13 u mean|g|, s2 within 16 u mean|g xhat|."""
    g = dy.to(F64) * gamma.to(F64)
    r = rstd.to(F64)[:, None]
    xh = (x.to(F64) - mean.to(F64)[:, None]) * r
    s1 = g.mean(1, keepdim=True)
    s2 = (g * xh).mean(1, keepdim=True)
    din = dx_in.to(F64) if dx_in is not None else torch.zeros_like(g)
    ref = r * (g - s1 - xh * s2) + din
    A = r * (g.abs() + s1.abs() + (xh * s2).abs()) + din.abs()
    extra = r * (13 * U * g.abs().mean(1, keepdim=True) + xh.abs() * 16 * U * (g * xh).abs().mean(1, keepdim=True))
    return ref, 8 * U * A + extra


def bpart_ref(dA_s, A_s, s, c, bn, dt):
    """bpart [M][3072 / bn * WGN][2] from the stored dA and A: (sum dA s, sum dA (A - c)) over part p's columns
    [p bn / WGN, (p + 1) bn / WGN).  The kernel sums the unrounded dA (within ulp_T(dA) / 2 of the stored one), a lane
    fma's its bn / (4 WGN) terms one after the other and the 4 lanes meet by two lane swaps; A - c rounds once more."""
    dA, A, s, c = dA_s.to(F64), A_s.to(F64), s.to(F64)[None, :], c.to(F64)[None, :]
    w = bn // WGN
    dep = bn // (4 * WGN) + 2

    def psum(t):
        return t.view(t.shape[0], t.shape[1] // w, w).sum(2)
    hu = 0.5 * GR.ulp(dA, dt)
    t1, t2 = dA * s, dA * (A - c)
    ref = torch.stack([psum(t1), psum(t2)], 2)
    bound = torch.stack([psum(hu * s.abs()) + dep * U * psum(t1.abs()),
                         psum(hu * (A - c).abs()) + (dep + 1) * U * psum(t2.abs())], 2) + 2.0 ** -149
    return ref, bound


def ln_bwd_fold(dA_s, WtT, bpart_s, X1, m2, r2, dX, dt):
    """EPI_LN_BWD from the stored operands: g = dA (W_fc')  (the product's B operand is (W_fc')^T, so WtT [768][3072]),
    out = fma(rstd, g - la - (x - mean) lb, dX), la = S1 / 768, lb = rstd (S2 / 768), S1 / S2 the stored partial pairs
    summed.  g within 2 K u |dA|.|W'| (K = 3072); S1, S2 a sum of depth ceil(parts / 8) + 3 and the division (TRANS),
    lb one more product; x - mean, its product with lb, the two subtractions and the fma: 5 u of
    A = rstd (|g| + |la| + |x - mean| |lb|) + |dX|.  Returns {"dX1": f32, "xh": its 16-bit copy}."""
    P, Sp = GR.product(dA_s, WtT)
    bp = bpart_s.to(F64)
    parts = bp.shape[1]
    dep = -(-parts // 8) + 3
    r, mu = r2.to(F64)[:, None], m2.to(F64)[:, None]
    S1, S2 = bp[:, :, 0].sum(1, keepdim=True), bp[:, :, 1].sum(1, keepdim=True)
    la, lb = S1 / WIDTH, r * S2 / WIDTH
    dla = (dep * U * bp[:, :, 0].abs().sum(1, keepdim=True) + TRANS * S1.abs()) / WIDTH
    dlb = r * (dep * U * bp[:, :, 1].abs().sum(1, keepdim=True) + (TRANS + U) * S2.abs()) / WIDTH
    xc = X1.to(F64) - mu
    din = dX.to(F64)
    ref = r * (P - la - xc * lb) + din
    A = r * (P.abs() + la.abs() + (xc * lb).abs()) + din.abs()
    d = r * (GR.units(2 * MLP) * Sp + dla + xc.abs() * dlb) + GR.units(5) * A
    return {"dX1": held(ref, d, torch.float32), "xh": held(ref, d, dt)}


def vpt_sum(rows):
    """dvpt = sum over crops of rows [B][NV][768], in crop order; bound: the B - 1 sequential f32 additions."""
    r = rows.to(F64)
    return r.sum(0), (r.shape[0] - 1) * U * r.abs().sum(0) + 2.0 ** -149


# ------------------------------------------------------------------------------------------------ parameters
def params_from_cache(cache, gh, gw):
    """The operands ebc_vit_forward / ebc_vit_backward are handed, as tensors: _EncoderCache's own (every pointer of
    its EbcVitWeights / EbcVitLayer structs looked up among the tensors it keeps), the folded ones included."""
    cache.weights(gh, gw)
    by_ptr = {t.data_ptr(): t for t in cache.keep}
    P = {"patch": cache.patch, "w_patch": cache.w_patch, "cls": cache.cls, "pos": cache.structs[(gh, gw)][1],
         "ln_pre_g": cache.ln[0], "ln_pre_b": cache.ln[1], "ln_post_g": cache.ln[2], "ln_post_b": cache.ln[3], "layers": []}
    for i in range(cache.layers):
        lay = {}
        for name, _ in type(cache.layer_arr[i])._fields_:
            p = getattr(cache.layer_arr[i], name)
            lay[name] = by_ptr[p] if p else None
        P["layers"].append(lay)
    return P


# ------------------------------------------------------------------------------------------------ the walkers
TINY = 1e-300


class Walk:
    """How a walker treats a stage's (stored view, reference, bound): "check" reports |view - ref| / bound,
    "simulate" stores the reference rounded once to the view's type (tests/test_vit_refs_cpu.py builds a workspace this
    way, as a kernel with no error beyond the final rounding would leave it)."""

    def __init__(self, mode, report=None, tag=""):
        assert mode in ("check", "simulate")
        self.mode, self.report, self.tag = mode, report, tag

    @property
    def check(self):
        return self.mode == "check"

    def emit(self, name, view, ref, bound):
        if self.check:
            self.report(f"{self.tag}.{name}", (view.to(F64) - ref).abs(), bound + TINY)
        else:
            view.copy_(ref.to(view.dtype))

    def exact(self, name, view, ref):
        """Bit for bit (ref holds values exact in the view's type)."""
        if self.check:
            want = ref.to(view.dtype)
            assert torch.equal(view, want), (f"{self.tag}.{name}", int((view != want).sum()))
        else:
            view.copy_(ref.to(view.dtype))


def _stats(wk, name, x, mview, rview, fold, bn, parts):
    """The stored mean / rstd of the f32 rows x."""
    mean, var, rstd = stats64(x)
    dmean, rho = fold_stat_bounds(x, mean, var, bn, parts) if fold else launch_stat_bounds(x, mean, var)
    wk.emit(f"{name}.mean", mview, mean, dmean + U * mean.abs() + 2.0 ** -149)
    wk.emit(f"{name}.rstd", rview, rstd, rstd * rho)


def _attn_sim(ws, l):
    q, k, v = ER.split_qkv(ws.get("QKV", l), ws.B, ws.L, HEADS)
    f = ER.attention_fwd(q, k, v)
    ws.get("O", l).copy_(ER.unheads(f["o"]).to(ws.dt))
    ws.get("lse", l).copy_(f["lse"].to(torch.float32))


def walk_forward(wk, ws, P, image, vpts, bstride, feat, fold, training=True, bn_out=96, bn_proj=96, attn_check=None):
    """Every stage of ebc_vit_forward in execution order, each from the stored operands of that stage alone.  vpts: one
    tensor or None a layer (shared [NV][768], or per crop [B][NV][768] with bstride = NV * 768).  A check of an eval
    workspace (training = 0: the layers' buffers alias) covers the last stage only."""
    B, L, G, NV, M, dt, layers = ws.B, ws.L, ws.G, ws.NV, ws.M, ws.dt, ws.layers
    dev = ws.ws.device
    prow = prompt_rows(B, L, NV, dev)
    stages = not wk.check or training
    if stages:
        # 1. patch embedding and X_0
        wk.exact("patch_t", ws.get("patch_t"), rn(im2col(image.to(F64), P["patch"]), dt))
        Pp, Sp = GR.product(ws.get("patch_t"), P["w_patch"])
        wk.emit("patch_f", ws.get("patch_f"), *GR.epilogue(GR.STORE, Pp, Sp, ws.KP, dt, torch.float32)["C"])
        wk.emit("X0", ws.get("X", 0), *embed(ws.get("patch_f"), P["cls"], P["pos"], P["ln_pre_g"], P["ln_pre_b"],
                                              vpts[0] if NV else None, bstride, B, L, G, NV))
    for l in range(layers if stages else 0):
        p = P["layers"][l]
        sl = l if training else 0
        X = ws.get("X", l)
        # 3. the prompt rows of X_l are vpt_l bit for bit (and, through 2., so are their statistics and 16-bit copy)
        deep = NV > 0 and vpts[l] is not None
        if deep and wk.check:
            wk.exact(f"l{l}.X.prompt_rows", X[prow], prompt_values(vpts[l], bstride, B, NV))
        # 2. ln_1 and the QKV product
        f1 = fold and l > 0
        _stats(wk, f"l{l}.ln1", X, ws.get("m1", sl), ws.get("r1", sl), f1, bn_proj, ws.parts_proj)
        if f1:
            out = ln_fold_product(X, ws.get("m1", sl), ws.get("r1", sl), p["w_qkv_ln"], p["s_qkv_ln"], p["b_qkv_ln"], dt)
        else:
            out, _ = ln_product(X, ws.get("m1", sl), ws.get("r1", sl), p["ln1_g"], p["ln1_b"], p["w_qkv"], p["b_qkv"], dt)
        wk.emit(f"l{l}.QKV", ws.get("QKV", sl), *out["C"])
        # 4. attention
        if wk.check:
            if attn_check is not None:
                attn_check(f"{wk.tag}.l{l}.attn", ws.get("QKV", sl), ws.get("O", sl), ws.get("lse", sl))
        else:
            _attn_sim(ws, sl)
        # 5. out-proj + residual, ln_2 and the c_fc product
        X1 = ws.get("X1", sl)
        wk.emit(f"l{l}.X1", X1, *resid_product(ws.get("O", sl), p["w_out"], p["b_out"], X, dt))
        _stats(wk, f"l{l}.ln2", X1, ws.get("m2", sl), ws.get("r2", sl), fold, bn_out, ws.parts_out)
        if fold:
            out = ln_fold_product(X1, ws.get("m2", sl), ws.get("r2", sl), p["w_fc_ln"], p["s_fc_ln"], p["b_fc_ln"], dt, True)
            Hq = rn(X1.to(F64), dt)
        else:
            out, Hq = ln_product(X1, ws.get("m2", sl), ws.get("r2", sl), p["ln2_g"], p["ln2_b"], p["w_fc"], p["b_fc"], dt, True)
        if training:
            wk.emit(f"l{l}.A", ws.get("A", sl), *out["aux"])
        last = l == layers - 1
        if last or not wk.check:
            # the transients still hold the last layer's values after the call
            wk.emit(f"l{l}.G", ws.get("G"), *out["C"])
            if fold:
                wk.exact(f"l{l}.H", ws.get("H"), Hq)
            elif not wk.check:
                ws.get("H").copy_(Hq.to(dt))
        # 6. c_proj + residual from the stored pre-activation (eval keeps none: from the stored G)
        Xn = ws.get("X", l + 1)
        if training:
            ref, bound, _ = mlp_out(ws.get("A", sl), X1, p["w_proj"], p["b_proj"], dt)
        else:
            ref, bound = resid_product(ws.get("G"), p["w_proj"], p["b_proj"], X1, dt)
        if NV > 0 and not last and vpts[l + 1] is not None:
            # deep VPT: block l + 1's prompt rows in place of the product's (the folded c_proj epilogue, or the unfolded
            # path's ln_1 launch of block l + 1, which writes them into X_l+1 too)
            ref = ref.clone()
            bound = bound.clone()
            ref[prow] = prompt_values(vpts[l + 1], bstride, B, NV).to(F64)
            bound[prow] = 0.0
        wk.emit(f"l{l}.Xnext", Xn, ref, bound)
    # 7. ln_post on the patch rows
    XL = ws.get("X", layers)
    rows = ER.ln_rows(B * G, G, L, 1 + NV).to(dev)
    _stats(wk, "ln_post", XL[rows], ws.get("mpost"), ws.get("rpost"), False, 0, 0)
    ref, bound, _ = ln_post(XL, P["ln_post_g"], P["ln_post_b"], ws.get("mpost"), ws.get("rpost"), B, L, G, NV)
    wk.emit("feat", feat.view(B * G, WIDTH), ref, bound)


def walk_backward(wk, ws, P, dfeat, dvpt, bstride, flags, fold_b, bn_gelu=192, attn_check=None):
    """Every stage of ebc_vit_backward on a one-layer encoder, in execution order.  dvpt: [tensor or None] (shared
    [NV][768] or per crop [B][NV][768]).  flags 0: layer 0's trimmed path, the MLP half and ln_post's backward are
    checked (dX_L is still in the workspace); EBC_VIT_BWD_FULL_LAYER0: the full attention half and layernorm_bwd_vpt
    (which reuses dX_L's buffer, so the MLP half is not checked there)."""
    assert ws.layers == 1
    B, L, G, NV, M, dt = ws.B, ws.L, ws.G, ws.NV, ws.M, ws.dt
    dev = ws.ws.device
    p = P["layers"][0]
    prow = prompt_rows(B, L, NV, dev)
    per_batch = bstride != 0
    want = NV > 0 and dvpt is not None and dvpt[0] is not None
    trimmed = want and not (flags & FLAG_FULL_LAYER0)
    mlp_half = not wk.check or trimmed            # (the untrimmed ln_1 backward writes dX_0 over dX_L)
    dXa, dXb, dXt = ws.get("dXa"), ws.get("dXb"), ws.get("dXt")
    X0, X1, XL = ws.get("X", 0), ws.get("X1", 0), ws.get("X", 1)
    nrows = B * NV
    if mlp_half:
        # 1. ln_post's backward into the patch rows; every other row an exact zero
        rows = ER.ln_rows(B * G, G, L, 1 + NV).to(dev)
        ref, bound = ln_bwd(dfeat.view(B * G, WIDTH), XL[rows], ws.get("mpost"), ws.get("rpost"), P["ln_post_g"], None)
        full = torch.zeros(M, WIDTH, dtype=F64, device=dev)
        fb = torch.zeros_like(full)
        full[rows] = ref
        fb[rows] = bound
        wk.emit("dX_L", dXa, full, fb)
        dXt_L = rn(dXa.to(F64), dt)                 # the launch's 16-bit copy of the same f32 value
        if not wk.check:
            dXt.copy_(dXt_L.to(dt))
        # 2. GELU' product (and its row partials)
        A = ws.get("A", 0)
        Pg, Sg = GR.product(dXt_L, p["wt_proj"])
        wk.emit("dA", ws.get("dA"), *GR.epilogue(GR.GELU_BWD, Pg, Sg, WIDTH, dt, dt, aux=A)["C"])
        dA = ws.get("dA")
        # 3. c_fc dX and ln_2's backward
        if fold_b:
            wk.emit("bpart", ws.get("bpart"), *bpart_ref(dA, A, p["s_fc_ln"], p["b_fc_ln"], bn_gelu, dt))
            out = ln_bwd_fold(dA, p["wt_fc_ln"], ws.get("bpart"), X1, ws.get("m2", 0), ws.get("r2", 0), dXa, dt)
            wk.emit("dX1", dXb, *out["dX1"])
            wk.emit("dX1.xh", dXt, *out["xh"])
        else:
            lo = nrows if wk.check else 0       # a check: the rows the trimmed dH product has not overwritten
            Ph, Sh = GR.product(dA, p["wt_fc"])
            href, hbound = GR.epilogue(GR.STORE, Ph, Sh, MLP, dt, dt)["C"]
            dH = ws.get("dH")
            wk.emit("dH2", dH[lo:], href[lo:], hbound[lo:])
            ref, bound = ln_bwd(dH[lo:], X1[lo:], ws.get("m2", 0)[lo:], ws.get("r2", 0)[lo:], p["ln2_g"], dXa[lo:])
            if not wk.check:
                dXb.copy_(ref.to(torch.float32))
                dXt.copy_(dXb.to(dt))
            else:
                wk.emit("dX1", dXb[lo:], ref, bound)
                wk.emit("dX1.t", dXt[lo:], *held(ref, bound, dt))
    # 4. dO, the attention backward, dH
    # (the 16-bit copy of dX1 the product read: the untrimmed path writes dX_0's copy over it, from the same f32 value)
    Po, So = GR.product(rn(dXb.to(F64), dt), p["wt_out"])
    wk.emit("dO", ws.get("dO"), *GR.epilogue(GR.STORE, Po, So, WIDTH, dt, dt)["C"])
    lim = 1 + NV if (trimmed and dt != torch.float32 and L <= 256) else L
    if wk.check:
        if attn_check is not None:
            attn_check(f"{wk.tag}.attn_bwd", ws.get("QKV", 0), ws.get("dO"), ws.get("O", 0), ws.get("lse", 0),
                       ws.get("dQKV"), ws.get("delta"), lim)
    else:
        q, k, v = ER.split_qkv(ws.get("QKV", 0), B, L, HEADS)
        r = ER.attention_bwd(q, k, v, ER.heads(ws.get("dO"), B, L, HEADS), ER.heads(ws.get("O", 0), B, L, HEADS),
                             ws.get("lse", 0))
        ws.get("dQKV").copy_(ER.pack_qkv(r["dq"], r["dk"], r["dv"]).to(dt))
    dQKV = ws.get("dQKV")
    dH = ws.get("dH")
    if trimmed:
        # layer 0 trimmed: dH on the B * NV prompt rows (row-mapped A operand), ln_1's backward of those rows
        rmap = GR.row_map(nrows, NV, L, 1, dev)
        Ph, Sh = GR.product(dQKV[rmap], p["wt_qkv"])
        wk.emit("dH.rows", dH[:nrows], *GR.epilogue(GR.STORE, Ph, Sh, QKVW, dt, dt)["C"])
        ref, bound = ln_bwd(dH[:nrows], X0[rmap], ws.get("m1", 0)[rmap], ws.get("r1", 0)[rmap], p["ln1_g"], dXb[rmap])
        rows_view = dvpt[0].view(nrows, WIDTH) if per_batch else ws.get("vpt_rows")[0].view(nrows, WIDTH)
        wk.emit("vpt_rows", rows_view, ref, bound)
    else:
        Ph, Sh = GR.product(dQKV, p["wt_qkv"])
        wk.emit("dH", dH, *GR.epilogue(GR.STORE, Ph, Sh, QKVW, dt, dt)["C"])
        ref, bound = ln_bwd(dH, X0, ws.get("m1", 0), ws.get("r1", 0), p["ln1_g"], dXb)
        if want:
            rows_view = dvpt[0].view(nrows, WIDTH) if per_batch else ws.get("vpt_rows")[0].view(nrows, WIDTH)
            wk.emit("vpt_rows", rows_view, ref[prow], bound[prow])
            # 6. the prompt rows of the outgoing gradient are exact zeros
            ref = ref.clone()
            bound = bound.clone()
            ref[prow] = 0.0
            bound[prow] = 0.0
        if wk.check:
            wk.emit("dX0", dXa, ref, bound)
            wk.emit("dX0.t", dXt, *held(ref, bound, dt))
        else:
            dXa.copy_(ref.to(torch.float32))
            dXt.copy_(dXa.to(dt))
    # 5. shared prompts: the per-crop rows summed in crop order
    if want and not per_batch:
        wk.emit("dvpt", dvpt[0], *vpt_sum(ws.get("vpt_rows")[0]))


# ------------------------------------------------------------------------------------------------ the cases
# name: (patch, H, W, NV, B, layers).  M = B * (1 + NV + (H / patch)(W / patch)); the tiles each reaches are asserted
# from ebc_gemm_tile_config in tests/test_vit_refs_cpu.py and again inside every GPU test.
CASES = {
    "tiny": (32, 64, 64, 3, 2, 3),          # M = 16: one ragged tile
    "tiny_nv0": (32, 64, 64, 0, 2, 3),      # no prompts
    "ragged135": (32, 64, 64, 4, 15, 2),    # M = 135: rows 127, 128 are prompt rows on either side of the tile edge
    "ragged261": (32, 64, 64, 4, 29, 2),    # M = 261: rows 255 (s = 3), 256 (s = 4) likewise
    "fold_b_low": (32, 64, 64, 3, 170, 2),  # M = 1360
    "fold_b_high": (32, 64, 64, 3, 300, 2), # M = 2400
    "many_tiles": (32, 64, 64, 3, 513, 2),  # M = 4104
    "patch16": (16, 32, 32, 3, 2, 3),       # K = 768 patch GEMM
    "L229": (16, 224, 224, 32, 1, 2),       # the model's own L
}
# 16-bit tiles (cfg ids) of (qkv, out-proj, c_fc / GELU', c_proj, LN_BWD = c_fc dX) per case
TILES16 = {
    "tiny": (2, 15, 2, 16, 16), "tiny_nv0": (2, 15, 2, 16, 16), "ragged135": (2, 15, 2, 16, 16),
    "ragged261": (2, 15, 2, 16, 16), "fold_b_low": (2, 15, 4, 16, 16), "fold_b_high": (4, 15, 3, 16, 16),
    "many_tiles": (4, 5, 3, 5, 5), "patch16": (2, 15, 2, 16, 16), "L229": (2, 15, 2, 16, 16),
}
PRODUCTS = ((QKVW, WIDTH), (WIDTH, WIDTH), (MLP, WIDTH), (WIDTH, MLP), (WIDTH, MLP))


def case_dims(name):
    patch, H, W, NV, B, layers = CASES[name]
    G, L, M = geometry(B, H, W, patch, NV)
    return patch, H, W, NV, B, layers, G, L, M


def case_tiles(lib, dtcode, name):
    M = case_dims(name)[-1]
    return tuple(tile_of(lib, dtcode, M, N, K)[0] for N, K in PRODUCTS)


def fold_b_taken(lib, dtcode, M, flags=0):
    """vit.hip's fold_b: 16-bit, the GELU' product leaves at most 32 partials, and the c_fc dX product runs on a
    loader-wave tile (gemm_ln_bwd_fold_pays: cfg 15 / 16)."""
    if dtcode == 0 or (flags & FLAG_NO_LN_FOLD):
        return False
    return part_counts(lib, dtcode, M)[2] <= LN_PMAX_B and tile_of(lib, dtcode, M, WIDTH, MLP)[0] in (15, 16)


# ------------------------------------------------------------------------------------------------ input generators
def make_encoder(name, stats="benign", layers=None):
    """The case's VisionTransformer with the synthetic loader's weights (ebc_amd.synthetic.vit_state); "outlier":
    synthetic.outlier_stats -- massive-activation channels and a common row offset (|mean| / std around 3), which
    loads the one-pass variance's cancellation term."""
    from ebc_amd import synthetic as syn
    from ebc_amd.model import VisionTransformer
    patch, H, W, NV, B, nl, G, L, M = case_dims(name)
    nl = layers or nl
    assert H == W
    sd = syn.vit_state(0, nl, H, patch)
    if stats == "outlier":
        sd = syn.outlier_stats(sd)
    elif stats == "offset":
        # the same without the massive channels (which widen the rows' std): the common offset 3 on rows of std ~1
        sd = syn.outlier_stats(sd, n_channels=0, dc=3.0)
    else:
        assert stats == "benign"
    enc = VisionTransformer(input_resolution=H, patch_size=patch, layers=nl)
    pre = "image_encoder."
    enc.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)}, strict=True)
    return enc.eval().requires_grad_(False)


def make_inputs(name, mode, per_crop, layers=None, seed=0, stats="benign"):
    """(image [B][3][H][W] f32, vpts, bstride) on the CPU.  mode "deep": prompts for every layer, "shallow": layer 0
    only, "none" (NV = 0).  Every prompt row has its own offset (layer, crop, row), so a row from the wrong layer or
    crop differs in every element and in its mean.  stats "offset": 1.5 more on rows of std 0.5, |mean| / std >= 3 --
    the prompt rows of X_l enter the folded statistics as they are."""
    patch, H, W, NV, B, nl, G, L, M = case_dims(name)
    nl = layers or nl
    g = torch.Generator().manual_seed(1000 + seed)
    image = torch.randn(B, 3, H, W, generator=g, dtype=torch.float32)
    vpts = [None] * nl
    if NV == 0:
        assert mode == "none"
        return image, vpts, 0
    nb = B if per_crop else 1
    for l in range(nl if mode == "deep" else 1):
        v = 0.5 * torch.randn(nb, NV, WIDTH, generator=g, dtype=torch.float32)
        off = 0.25 * (l + 1) + 0.0625 * (torch.arange(nb) % 8)[:, None, None] + 0.015625 * torch.arange(NV)[None, :, None]
        off = off + (1.5 if stats == "offset" else 0.0)
        vpts[l] = (v + off * (1 - 2 * (l % 2))).contiguous()
        if not per_crop:
            vpts[l] = vpts[l][0].contiguous()
    return image, vpts, (NV * WIDTH if per_crop else 0)


def make_dfeat(name, seed=0):
    patch, H, W, NV, B, nl, G, L, M = case_dims(name)
    g = torch.Generator().manual_seed(2000 + seed)
    r = torch.arange(B * G, dtype=torch.float32)[:, None]
    return (torch.randn(B * G, WIDTH, generator=g, dtype=torch.float32) * (0.5 + (r % 5) * 0.25)).view(B, G, WIDTH)
