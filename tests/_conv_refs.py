"""Plain float64 restatements of what ebc_conv3x3_fwd / ebc_conv3x3_wgrad compute (include/ebc_hip.h; conv_gemm MODE 1 and
MODE 2 in csrc/gemm.hip), from the operands as the kernels receive them (already rounded to `dtype`), and the per-element
error bounds tests/test_gpu_conv_kernels.py holds them to.  ulp, units and the store rule are tests/_gemm_refs.py's.

Every function is plain torch on whatever device its operands live on: tests/test_conv_refs_cpu.py pins them on the CPU
against F.conv2d, torch.nn.grad.conv2d_weight, autograd and plain torch; the GPU module runs the same code on the device.

Error model, in units of u = 2^-24 (_gemm_refs.units) of the magnitude named with each count:
  * the K-step accumulation: 2 units of Sp (the same sum over absolute values) per K step, as _gemm_refs counts an MFMA
    step.  K = 9 C for MODE 1; for MODE 2 the Kq columns the loop actually walks (B * HWp rounded up to 64: the padding
    columns multiply zeros but are steps all the same);
  * pieces: a tile whose K is cut into p > 1 pieces (a stream-K tile: at most 4; the last-arriver split: 2; s f32
    partials summed by splitk_reduce_kernel: s) adds its pieces in f32, one rounding of at most Sp each: p further units.
    The pieces' own steps add up to K, so the count is 2 K + p whatever the cut (the even splits' 2 K / s + s of
    _gemm_refs is smaller; this one is monotone in K and in p and is the one used);
  * f32 operands round each product once more: one further unit of Sp, as in _gemm_refs;
  * the store to a 16-bit T: `held` -- half an ulp of T at the reference plus twice the f32-side error; an f32 output
    carries the f32-side error once;
  * EPI_ADD_RELU_GRAD: acc + gy * (y > 0) is one f32 add: one further unit of Sp + |gy|.  The mask is exactly y > 0
    (-0.0, +0.0 and negative values give no gradient), no error term;
  * EPI_STATS: thread `col` of a tile adds the tile's rows of its column in row order from the staged f32
    accumulators: col_s += x (one rounding per row), col_q = fmaf(x, x, col_q) (one rounding per row).  With d_r the
    accumulator's own error bound at row r and a_r = |P_r| + d_r, every partial sum is at most sum a_r resp. sum a_r^2
    over the tile's rows, so a tile of `rows` rows is off by at most
        sum d_r + units(rows) * sum a_r            and            sum (2 |P_r| d_r + d_r^2) + units(rows) * sum a_r^2;
    the tile rows are BM = ebc_conv_tile_config's out[0] rows each (the last one ragged); their partials are added in
    float64 (reduce_partials_kernel), which adds nothing at this scale.
No step here needed the "2 ulp for an undocumented rounding" allowance beyond the MFMA step's 2 units.
"""
import torch

import _gemm_refs as G

F64 = G.F64
ulp, units = G.ulp, G.units


# ------------------------------------------------------------------------------------------------ geometry
def geometry(B, H, W):
    """make_geo of csrc/decoder.hip: the padded NHWC image is Hp rows of Wp positions; a weight-gradient image has HWp
    K columns (Kq in all) and Pimg positions in a row of xT3; Qs is the row stride of dzT and xT3."""
    r8 = lambda v: (v + 7) // 8 * 8                                            # noqa: E731
    Hp, Wp = H + 2, max(r8(W + 2), 32)
    HWp = max(r8(H * W), 64)
    Kq = (B * HWp + 63) // 64 * 64
    Pimg = r8(max((H + 2) * W, HWp))
    tail = (B + 2 + 64 // HWp) * Pimg + HWp + 2 * W + 64
    return {"B": B, "H": H, "W": W, "Hp": Hp, "Wp": Wp, "HWp": HWp, "Kq": Kq, "Q": B * Hp * Wp, "Pimg": Pimg,
            "Qs": (max(Kq, tail) + 63) // 64 * 64}


def pad_image(x, geo, pad_fill=0.0, slack_fill=0.0):
    """[B][Hp][Wp][C] from x [B][H][W][C]: the one-pixel frame around the interior takes `pad_fill`, the alignment
    columns xp >= W + 2 take `slack_fill`.  A fill is a number or a tensor that broadcasts to [B][Hp][Wp][C]."""
    B, H, W, C = x.shape
    assert (B, H, W) == (geo["B"], geo["H"], geo["W"])
    Hp, Wp = geo["Hp"], geo["Wp"]

    def full(fill):
        if torch.is_tensor(fill):
            return fill.to(x.dtype).to(x.device).expand(B, Hp, Wp, C).clone()
        return torch.full((B, Hp, Wp, C), fill, dtype=x.dtype, device=x.device)

    out = full(pad_fill)
    out[:, :, W + 2:] = full(slack_fill)[:, :, W + 2:]
    out[:, 1:H + 1, 1:W + 1] = x
    return out


# ------------------------------------------------------------------------------------------------ the products
def conv_fwd(xpad, wk, geo, with_abs=True):
    """(P, Sp) in float64, [B*H*W][N]: P[(b,y,x)][n] = sum_{ky,kx,c} xpad[b][y+ky][x+kx][c] * wk[n][ky][kx][c], the image
    read as given (frame cells included), and the same sum over absolute values (None without `with_abs`).  Nine
    shifted [M][C] @ [C][N] products: no im2col is materialised."""
    B, H, W = geo["B"], geo["H"], geo["W"]
    C, N = xpad.shape[-1], wk.shape[0]
    assert xpad.shape == (B, geo["Hp"], geo["Wp"], C) and wk.shape == (N, 3, 3, C)
    P = torch.zeros(B * H * W, N, dtype=F64, device=xpad.device)
    Sp = torch.zeros_like(P) if with_abs else None
    for ky in range(3):
        for kx in range(3):
            a = xpad[:, ky:ky + H, kx:kx + W, :].reshape(B * H * W, C).to(F64)
            w = wk[:, ky, kx, :].to(F64).t()
            P += a @ w
            if with_abs:
                Sp += a.abs() @ w.abs()
    return P, Sp


def conv_wgrad(dz, x, with_abs=True):
    """(dW, Sp) in float64, [N][C][3][3]: dW[n][c][ky][kx] = sum over the interior pixels (b, y, x) of
    dz[b][y][x][n] * x[b][y+ky-1][x+kx-1][c] (zero outside the image), dz [B][H][W][N], x [B][H][W][C]."""
    B, H, W, N = dz.shape
    C = x.shape[-1]
    assert x.shape == (B, H, W, C)
    xz = torch.zeros(B, H + 2, W + 2, C, dtype=F64, device=x.device)
    xz[:, 1:H + 1, 1:W + 1] = x.to(F64)
    d = dz.reshape(B * H * W, N).to(F64).t()
    dW = torch.zeros(N, C, 3, 3, dtype=F64, device=x.device)
    Sp = torch.zeros_like(dW) if with_abs else None
    for ky in range(3):
        for kx in range(3):
            a = xz[:, ky:ky + H, kx:kx + W, :].reshape(B * H * W, C)
            dW[:, :, ky, kx] = d @ a
            if with_abs:
                Sp[:, :, ky, kx] = d.abs() @ a.abs()
    return dW, Sp


def stats(P):
    """Column sums and sums of squares of the float64 product (the kernel sums its f32 accumulators, not the stored
    16-bit values)."""
    P = P.to(F64)
    return P.sum(0), (P * P).sum(0)


def add_relu_grad(P, gy, y):
    """P + gy * (y > 0)."""
    gy = gy.to(F64)
    return P.to(F64) + torch.where(y.to(F64) > 0, gy, torch.zeros_like(gy))


# ------------------------------------------------------------------------------------------------ the bounds
def acc_units(K, pieces, dt):
    """Units of Sp the f32 accumulator of a tile is off by: 2 per K step, one per piece added, one for f32 operands."""
    return 2.0 * K + (pieces if pieces > 1 else 0) + (1 if dt == torch.float32 else 0)


def acc_bound(Sp, K, pieces, dt):
    return units(acc_units(K, pieces, dt)) * Sp


def held(ref, d, t):
    """The stored value's bound from the f32-side bound d: _gemm_refs' store rule."""
    if t == torch.float32:
        return d
    return 0.5 * ulp(ref, t) + 2.0 * d


def add_relu_grad_bound(Sp, gy, K, pieces, dt):
    """f32-side bound of acc + gy * (y > 0): the accumulator's, and one rounding of the add."""
    return units(acc_units(K, pieces, dt) + 1) * (Sp + gy.to(F64).abs())


def _tile_rows(v, bm):
    """Sums of v [M][N] over tile rows of bm rows (the last one ragged): [ceil(M / bm)][N]."""
    M, N = v.shape
    nt = -(-M // bm)
    if nt * bm != M:
        v = torch.cat([v, torch.zeros(nt * bm - M, N, dtype=v.dtype, device=v.device)])
    return v.reshape(nt, bm, N).sum(1)


def stats_bound(P, d, bm):
    """Bounds of the column sums / sums of squares EPI_STATS takes over tile rows of `bm` rows from accumulators that
    are within d (a tensor like P, or 0.0) of P; see the module docstring."""
    P = P.to(F64).abs()
    M = P.shape[0]
    d = d if torch.is_tensor(d) else torch.full_like(P, d)
    a = P + d
    nt = -(-M // bm)
    rows = torch.full((nt, 1), float(bm), dtype=F64, device=P.device)
    rows[-1] = M - (nt - 1) * bm
    bs = _tile_rows(d, bm) + units(rows) * _tile_rows(a, bm)
    bq = _tile_rows(2.0 * P * d + d * d, bm) + units(rows) * _tile_rows(a * a, bm)
    return bs.sum(0), bq.sum(0)


def stats_exact_in_f32(P, bm, spacing):
    """Per column: every tile row's running sum of |v| stays below 2^24 * spacing, so f32 adds the multiples of
    `spacing` v [M][N] exactly in any order (the dyadic runs' premise)."""
    return (_tile_rows(P.to(F64).abs(), bm) < 2.0 ** 24 * spacing).all(0)


# ------------------------------------------------------------------------------------------------ MODE 2 operands
def dz_transposed(dz, geo, fill=0.0, tail_fill=0.0):
    """dzT [N][Qs] as include/ebc_hip.h documents it: column b * HWp + r = interior pixel r of image b; the padding
    columns inside Kq (r >= H*W of each image, and past B * HWp) take `fill`, the columns >= Kq `tail_fill`."""
    B, H, W, N = dz.shape
    HWp, Kq, Qs = geo["HWp"], geo["Kq"], geo["Qs"]
    out = torch.full((N, Qs), tail_fill, dtype=dz.dtype, device=dz.device)
    out[:, :Kq] = fill
    img = out[:, :B * HWp].view(N, B, HWp)
    img[:, :, :H * W] = dz.reshape(B, H * W, N).permute(2, 0, 1)
    return out


def xT3_padding_mask(geo, device=None):
    """[Qs] bool: the positions of an xT3 row that belong to no image row (past (H + 2) * W inside an image's Pimg,
    and past the last image)."""
    pos = torch.arange(geo["Qs"], device=device)
    return (pos >= geo["B"] * geo["Pimg"]) | (pos % geo["Pimg"] >= (geo["H"] + 2) * geo["W"])
