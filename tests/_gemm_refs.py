"""Plain float64 restatements of what ebc_gemm / ebc_gemm_rows / ebc_gemm_wgrad / ebc_transpose compute
(include/ebc_hip.h), from the operands as the kernel receives them (already rounded to `dtype`), and the per-element
error bounds tests/test_gpu_gemm_kernels.py holds the kernels to.

Every function is plain torch on whatever device its operands live on: tests/test_gemm_refs_cpu.py pins them on the CPU
against torch's own float64 ops, autograd and plain indexing; the GPU module runs the same code on the device (the
products reach 8000 x 3072 elements, too many to bring to the host per case).

Error model.  u = 2^-24 is the unit roundoff of f32 and every count below is in units of u relative to the magnitude
named with it:
  * the K-step accumulation: products of two 16-bit values are exact in f32; how an MFMA rounds inside its own
    accumulation is not documented (it may truncate), so each of the K steps gets 2 units: 2K units of
    Sp = |A|.|B|^T.  f32 operands round each product once more: one further unit of Sp;
  * the bias add and the residual add: one rounding each, of a value no larger than S = Sp + |bias| + |resid|;
  * a split K of s pieces: each piece accumulates K/s steps, the s - 1 additions of the pieces round once each
    (a partial that passes through f32 memory is not rounded): 2K/s + s units of Sp;
  * the store to a 16-bit T: the nearest T to the computed value x~.  With |x~ - ref| <= d and r* the nearest T to ref,
    |rd(x~) - x~| <= |r* - x~| <= ulp_T(ref)/2 + d, so |rd(x~) - ref| <= ulp_T(ref)/2 + 2d: the f32-side error counts
    twice for a 16-bit output, once for an f32 output (no ulp term there);
  * QuickGELU and its derivative: see gelu_arith / gelu_grad_arith.
First-order counts c are applied as c * u * (1 + c * u), which covers (1 + u)^c - 1.
"""
import torch

F64 = torch.float64
U = 2.0 ** -24
SIG_BITS = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}
MIN_EXP = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}
GELU_SLOPE = 1.1                    # max |QuickGELU'| = 1.0998.. (test_gemm_refs_cpu.py)
STORE, GELU, RESID, GELU_BWD = 0, 1, 2, 3


def ulp(ref, dt):
    """Spacing of dtype `dt` at the float64 values `ref` (subnormal spacing below the smallest normal), with exact
    arithmetic only: |x| / frexp-mantissa is the power of two 2^e exactly, whatever the device's pow does."""
    x = ref.to(F64).abs()
    m, _ = torch.frexp(x)                                              # |x| = m * 2^e, m in [0.5, 1)
    p2 = torch.where(x == 0, torch.zeros_like(x), x / torch.where(x == 0, torch.ones_like(x), m))     # 2^e
    return torch.clamp(p2 * 2.0 ** -SIG_BITS[dt], min=2.0 ** (MIN_EXP[dt] - (SIG_BITS[dt] - 1)))


def units(c):
    return c * U * (1.0 + c * U)


# ------------------------------------------------------------------------------------------------ QuickGELU
def sigmoid1702(a):
    return 1.0 / (1.0 + torch.exp(-1.702 * a.to(F64)))


def quick_gelu(a):
    """x * sigmoid(1.702 x)."""
    a = a.to(F64)
    return a * sigmoid1702(a)


def quick_gelu_grad(a):
    """d/dx of it: s + 1.702 x s (1 - s), s = sigmoid(1.702 x)."""
    a = a.to(F64)
    s = sigmoid1702(a)
    return s + 1.702 * a * s * (1.0 - s)


def _sigmoid_err(a, s):
    """Absolute error, in units of u, of s = rcp(1 + exp2(t)), t = (-1.702f * log2e_f) * a in f32:
    the folded constant carries 3 units (1.702f, log2e as f32, their product) and the multiply by a one more, so
    t is off by 4 u |t| and exp2(t) by the factor 4 u ln2 |t| = 4 * 1.702 |a| u, plus the hardware exp2's 2 ulp =
    4 units; that relative error of e = exp2(t) reaches s scaled by e / (1 + e) = 1 - s.  1 + e rounds once (1 unit)
    and the hardware reciprocal is 2 ulp (4 units)."""
    return s * ((1.0 - s) * (4.0 * 1.702 * a.abs() + 4.0) + 5.0)


def gelu_arith(a):
    """Units of u (absolute) the f32 evaluation of QuickGELU at `a` is off by: the sigmoid's, times |a|, and the final
    multiply's rounding of |a| s."""
    a = a.to(F64)
    s = sigmoid1702(a)
    return a.abs() * (_sigmoid_err(a, s) + s)


def gelu_grad_arith(a):
    """Units of u (absolute) of g = s + ((1.702f a) s) (1 - s) in f32: ds = the sigmoid's; 1 - s rounds once and
    inherits ds; p = 1.702 a s (1 - s) carries 1.702f (1 unit), three multiplies (3 units), ds / s and
    (ds + (1 - s)) / (1 - s), written without the divisions (|p| / s = 1.702 |a| (1 - s), |p| / (1 - s) = 1.702 |a| s);
    the final add rounds |g| once."""
    a = a.to(F64)
    s = sigmoid1702(a)
    ds = _sigmoid_err(a, s)
    p = (1.702 * a * s * (1.0 - s)).abs()
    g = (s + 1.702 * a * s * (1.0 - s)).abs()
    return ds + 4.0 * p + 1.702 * a.abs() * (1.0 - s) * ds + 1.702 * a.abs() * s * ds + p + g


# ------------------------------------------------------------------------------------------------ the products
def row_map(M, rpg, gstride, goff, device=None):
    """A row of output row r: (r / rpg) * gstride + goff + r % rpg (rpg 0: r)."""
    r = torch.arange(M, device=device)
    if rpg == 0:
        return r
    return torch.div(r, rpg, rounding_mode="floor") * gstride + goff + r % rpg


def product(A, B):
    """(A.B^T, |A|.|B|^T) in float64."""
    A, B = A.to(F64), B.to(F64)
    return A @ B.t(), A.abs() @ B.abs().t()


def epilogue(epi, P, Sp, K, dt, out_dt, bias=None, resid=None, aux=None, splits=1):
    """Reference outputs and bounds of one epilogue from the float64 product P and Sp = |A|.|B|^T.
    Returns {name: (ref, bound)} for "C" and, for GELU, "aux".  `dt` is the operand type, `out_dt` the type of C;
    aux (GELU': the stored pre-activation, as given) is of `dt`."""
    acc_units = 2.0 * K / splits + (splits if splits > 1 else 0) + (1 if dt == torch.float32 else 0)
    pre = P
    S = Sp
    n = 0
    if bias is not None and epi != GELU_BWD:
        pre = pre + bias.to(F64)
        S = S + bias.to(F64).abs()
        n += 1
    if epi == RESID:
        pre = pre + resid.to(F64)
        S = S + resid.to(F64).abs()
        n += 1

    def held(ref, d, t):
        if t == torch.float32:
            return ref, d
        return ref, 0.5 * ulp(ref, t) + 2.0 * d

    if epi in (STORE, RESID):
        # K accumulation steps at 2 units, the bias add and the residual add at one unit each
        return {"C": held(pre, units(acc_units + n) * S, out_dt)}
    if epi == GELU:
        d = units(acc_units + n) * S
        # the pre-activation's error through |QuickGELU'| <= 1.1 (mean value theorem; the 1.6e-4 between 1.0998 and 1.1
        # also covers evaluating gelu_arith at the reference pre-activation), plus the evaluation's own roundings
        dc = GELU_SLOPE * d + U * gelu_arith(pre)
        return {"aux": held(pre, d, dt), "C": held(quick_gelu(pre), dc, out_dt)}
    if epi == GELU_BWD:
        a = aux.to(F64)
        g = quick_gelu_grad(a)
        d = units(acc_units) * Sp                   # acc (the kernel adds no bias here: none is passed)
        dg = U * gelu_grad_arith(a)
        # (acc + d)(g + dg) rounded once
        dc = g.abs() * d + P.abs() * dg + d * dg + U * (P * g).abs()
        return {"C": held(P * g, dc, out_dt)}
    raise ValueError(epi)


def transpose_padded(x, ld, fill):
    """out [C][ld]: out[c][r] = x[r][c] for r < R, the padding columns r >= R keep `fill`."""
    R, C = x.shape
    out = torch.full((C, ld), fill, dtype=x.dtype, device=x.device)
    out[:, :R] = x.t()
    return out
