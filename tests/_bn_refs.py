"""Plain float64 restatements of the operations behind the BatchNorm / pooling / upsample kernels of decoder.hip.

Written from the reference project's semantics (nn.BatchNorm2d train / eval, F.interpolate(bilinear,
align_corners=False), nn.AvgPool2d(2), ReLU with relu'(0) = 0) and from the layouts include/ebc_hip.h documents,
with explicit loops / indexing and no shortcut through the kernels' arithmetic.  tests/test_bn_refs_cpu.py checks
them against torch's own float64 ops and autograd; tests/test_gpu_bn_kernels.py checks the kernels against them.
Everything here is CPU float64 (activations are NHWC rows [P][C] or images [B][H][W][C]).
"""
import math

import torch

F64 = torch.float64
U32 = 2.0 ** -24                                   # unit roundoff of f32 (half an ulp, relative)
SIG_BITS = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}
MIN_EXP = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}


def ulp(ref: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """Spacing of dtype `dt` at the (float64) values `ref`: 2^(floor(log2|x|) - (p - 1)), subnormal spacing below
    the smallest normal."""
    x = ref.to(F64).abs()
    _, e = torch.frexp(x)                                              # |x| = m * 2^e, m in [0.5, 1)
    e = torch.clamp(e.to(F64) - 1.0, min=float(MIN_EXP[dt]))
    e = torch.where(x == 0, torch.full_like(e, float(MIN_EXP[dt])), e)
    return torch.pow(torch.tensor(2.0, dtype=F64), e - (SIG_BITS[dt] - 1))


def rows_per_block(C: int) -> int:
    """Rows one block of the two column-reduction kernels sums in f32 (ebc_hip.h: the workspace formula)."""
    return 8 * max(1, 512 // (C // 8))


# --------------------------------------------------------------------------------------------- BatchNorm2d
def bn_sums(z):
    """(sum z, sum z*z) per channel of rows z [P][C], and the sums of |terms| (the error bounds' scale)."""
    z = z.to(F64)
    return z.sum(0), (z * z).sum(0), z.abs().sum(0)


def bn_from_sums(S, Q, count, gamma, beta, eps, momentum=None, rmean=None, rvar=None):
    """nn.BatchNorm2d in training mode from the column sums: batch mean, biased variance, rstd, the folded
    scale = gamma*rstd and shift = beta - mean*scale, and the running statistics (momentum, unbiased variance)."""
    S, Q, gamma, beta = S.to(F64), Q.to(F64), gamma.to(F64), beta.to(F64)
    mean = S / count
    var = torch.clamp(Q / count - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    out = {"mean": mean, "var": var, "rstd": rstd, "scale": gamma * rstd, "shift": beta - mean * gamma * rstd}
    if rmean is not None:
        out["running_mean"] = (1.0 - momentum) * rmean.to(F64) + momentum * mean
        out["running_var"] = (1.0 - momentum) * rvar.to(F64) + momentum * var * (count / (count - 1.0))
    return out


def bn_train(z, gamma, beta, eps, momentum=None, rmean=None, rvar=None):
    """The same from the rows themselves, with the variance as the mean squared deviation (no cancellation)."""
    z = z.to(F64)
    P = z.shape[0]
    mean = z.sum(0) / P
    var = ((z - mean) ** 2).sum(0) / P
    rstd = 1.0 / torch.sqrt(var + eps)
    gamma, beta = gamma.to(F64), beta.to(F64)
    out = {"mean": mean, "var": var, "rstd": rstd, "scale": gamma * rstd, "shift": beta - mean * gamma * rstd,
           "y": (z - mean) * rstd * gamma + beta}
    if rmean is not None:
        out["running_mean"] = (1.0 - momentum) * rmean.to(F64) + momentum * mean
        out["running_var"] = (1.0 - momentum) * rvar.to(F64) + momentum * var * P / (P - 1.0)
    return out


def bn_eval(rmean, rvar, gamma, beta, eps):
    """Eval mode: the running statistics are the statistics; nothing is updated."""
    mean, var = rmean.to(F64), rvar.to(F64)
    rstd = 1.0 / torch.sqrt(var + eps)
    return {"mean": mean, "var": var, "rstd": rstd, "scale": gamma.to(F64) * rstd,
            "shift": beta.to(F64) - mean * gamma.to(F64) * rstd}


def relu(x):
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_grad(g, m):
    """g * relu'(m) with relu'(0) = 0 (torch's threshold_backward: grad where m > 0)."""
    return torch.where(m > 0, g, torch.zeros_like(g))


def bn_relu(z, scale, shift):
    return relu(z.to(F64) * scale.to(F64) + shift.to(F64))


def bn_bwd_sums(gy, m, z, mean, rstd):
    """(sum g, sum g*xhat) per channel, g = gy * relu'(m), xhat = (z - mean) * rstd; and the sums of |terms|."""
    g = relu_grad(gy.to(F64), m.to(F64))
    t = g * ((z.to(F64) - mean.to(F64)) * rstd.to(F64))
    return g.sum(0), t.sum(0), g.abs().sum(0), t.abs().sum(0)


def bn_bwd_coef(sg, sgx, count, gamma, rstd):
    """coef[3][C] = [gamma*rstd, mean(g), mean(g*xhat)]; dgamma = sum g*xhat, dbeta = sum g."""
    return torch.stack([gamma.to(F64) * rstd.to(F64), sg.to(F64) / count, sgx.to(F64) / count])


def bn_bwd_dz(gy, m, z, mean, rstd, coef):
    """BatchNorm input gradient dz = gamma*rstd * (g - mean(g) - xhat * mean(g*xhat)) and g itself; also the sum of
    the absolute values of the expression's terms (the elementwise bound's A)."""
    g = relu_grad(gy.to(F64), m.to(F64))
    xhat = (z.to(F64) - mean.to(F64)) * rstd.to(F64)
    k0, k1, k2 = coef[0].to(F64), coef[1].to(F64), coef[2].to(F64)
    dz = k0 * (g - k1 - xhat * k2)
    A = k0.abs() * (g.abs() + k1.abs() + (z.to(F64).abs() + mean.to(F64).abs()) * rstd.to(F64).abs() * k2.abs())
    return dz, g, A


# --------------------------------------------------------------------------------------------- bilinear upsample
def bilinear_taps(n_out: int, n_in: int, up: int):
    """F.interpolate(bilinear, align_corners=False, scale_factor=up) along one axis: output o reads
    src = max((o + 0.5) / up - 0.5, 0), taps i0 = floor(src), i1 = min(i0 + 1, n_in - 1), weights 1 - l, l."""
    taps = []
    for o in range(n_out):
        src = max((o + 0.5) / up - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        lam = src - i0
        taps.append((i0, i1, 1.0 - lam, lam))
    return taps


def upsample_matrix(n_in: int, up: int) -> torch.Tensor:
    """[n_in*up][n_in] float64 matrix of the one-axis interpolation."""
    M = torch.zeros(n_in * up, n_in, dtype=F64)
    for o, (i0, i1, l0, l1) in enumerate(bilinear_taps(n_in * up, n_in, up)):
        M[o, i0] += l0
        M[o, i1] += l1
    return M


def upsample(feat, up: int):
    """feat [B][h][w][C] -> [B][h*up][w*up][C]; also the sum of |weight * value| per output (the bound's A)."""
    feat = feat.to(F64)
    My, Mx = upsample_matrix(feat.shape[1], up), upsample_matrix(feat.shape[2], up)
    out = torch.einsum("yi,xj,bijc->byxc", My, Mx, feat)
    A = torch.einsum("yi,xj,bijc->byxc", My, Mx, feat.abs())
    return out, A


def upsample_adjoint(g, up: int):
    """The adjoint: g [B][H][W][C] -> dfeat [B][H/up][W/up][C]."""
    g = g.to(F64)
    My, Mx = upsample_matrix(g.shape[1] // up, up), upsample_matrix(g.shape[2] // up, up)
    return torch.einsum("yi,xj,byxc->bijc", My, Mx, g)


# --------------------------------------------------------------------------------------------- AvgPool2d(2)
def avgpool2(x):
    """x [B][H][W][C] -> [B][H/2][W/2][C], the mean of each 2x2 window."""
    x = x.to(F64)
    return (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) / 4.0


def avgpool2_bwd(g, H: int, W: int):
    """g [B][H/2][W/2][C] -> gx [B][H][W][C] = g[b][y//2][x//2] / 4."""
    g = g.to(F64)
    gx = torch.empty(g.shape[0], H, W, g.shape[3], dtype=F64)
    for y in range(H):
        for x in range(W):
            gx[:, y, x] = g[:, y // 2, x // 2] / 4.0
    return gx


# --------------------------------------------------------------------------------------------- layouts
def pad_nhwc(x, Hp: int, Wp: int, fill=None):
    """Interior image x [B][H][W][C] -> padded rows [B*Hp*Wp][C]: pixel (y, x) at row (b*Hp + y + 1)*Wp + x + 1,
    every other cell 0.  Returns the rows and the boolean interior-row mask [B*Hp*Wp]."""
    B, H, W, C = x.shape
    out = torch.zeros(B, Hp, Wp, C, dtype=x.dtype)
    inter = torch.zeros(B, Hp, Wp, dtype=torch.bool)
    for b in range(B):
        for y in range(H):
            for xx in range(W):
                out[b, y + 1, xx + 1] = x[b, y, xx]
                inter[b, y + 1, xx + 1] = True
    return out.reshape(B * Hp * Wp, C), inter.reshape(-1)


def dzT_layout(dz, HWp: int, Kq: int):
    """dz [B][H][W][C] -> [C][Kq]: column b*HWp + y*W + x holds pixel (y, x) of image b, every other column 0."""
    B, H, W, C = dz.shape
    out = torch.zeros(C, Kq, dtype=dz.dtype)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                out[:, b * HWp + y * W + x] = dz[b, y, x]
    return out


def conv_weight_layouts(w):
    """nn.Conv2d weight [N][C][3][3] -> wk [N][3][3][C] (wk[o][ky][kx][c] = w[o][c][ky][kx]) and the flipped
    data-gradient operand wf [C][9][N] (wf[c][t][o] = w[o][c][8 - t], t = ky*3 + kx)."""
    N, C = w.shape[:2]
    wk = torch.empty(N, 3, 3, C, dtype=w.dtype)
    wf = torch.empty(C, 9, N, dtype=w.dtype)
    w9 = w.reshape(N, C, 9)
    for t in range(9):
        wk[:, t // 3, t % 3, :] = w9[:, :, t]
        wf[:, t, :] = w9[:, :, 8 - t].t()
    return wk, wf


def weight_1x1_layouts(w):
    """1x1 conv weight [N][K] -> wk [N][K] and wt [K][N] (wt[k][n] = w[n][k])."""
    N, K = w.shape
    wt = torch.empty(K, N, dtype=w.dtype)
    for n in range(N):
        wt[:, n] = w[n, :]
    return w.clone(), wt
