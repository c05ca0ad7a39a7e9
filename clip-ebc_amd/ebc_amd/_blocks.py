"""The sequencing of libebc_hip.so's BatchNorm / convolution entry points that the three block Functions share
(model._DecoderFn, resnet._ResBlockFn, resnet._BottleneckFn): workspaces, weight preparation, ONE BatchNorm
forward / backward protocol (SyncBatchNorm exchange included) and the 3x3 / 1x1 conv + BatchNorm stages.

A stage is `conv -> BatchNorm statistics`; what follows the statistics (ReLU, padding, pooling, the residual
add) differs per block and stays with the Function.  The weight preparation is a call of its own: the resnet
Functions prepare every weight of a block before its first product."""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib

_DEC_WS: Dict[Tuple[torch.device, int], Tensor] = {}


def _dec_workspace(dev: torch.device, nbytes: int, slot: int = 0) -> Tensor:
    """Scratch of the block calls on the caller's stream; its first 16 KiB (split-K counters) start zeroed and every
    kernel leaves them zero.  Slots: 0 the convolutions and BatchNorm partials (the resnet Functions size it by
    resnet._ws), 1 _DecoderFn's 3x3 weight gradients, 2 _wgrad_rows, 3 the head's backward.  (The weight gradients
    on a side stream beside the data-gradient chain measured 2.7 % slower per step, r01: the data-gradient chain is
    the critical path.)"""
    ws = _DEC_WS.get((dev, slot))
    if ws is None or ws.numel() < nbytes:
        ws = torch.zeros(max(nbytes, 1 << 20), device=dev, dtype=torch.uint8)
        _DEC_WS[(dev, slot)] = ws
    return ws


class Geometry(NamedTuple):
    """One 3x3 conv's shapes: B images of H x W, C -> N channels, P = B*H*W rows; the zero-padded image is
    [B, Hp, Wp] = Q rows, its K-contiguous transposes hold Qs columns (ebc_dec_geometry)."""
    B: int
    H: int
    W: int
    C: int
    N: int
    P: int
    Hp: int
    Wp: int
    Q: int
    Qs: int


def _geometry(L, dt: int, B: int, H: int, W: int, C: int, N: int) -> Geometry:
    geo = (ctypes.c_long * 6)()
    _lib.check(L.ebc_dec_geometry(dt, B, H, W, C, geo), "ebc_dec_geometry")
    return Geometry(B, H, W, C, N, B * H * W, geo[0], geo[1], geo[4], geo[5])


def _wgrad_rows(L, dZ: Tensor, Y: Tensor, cdtype: torch.dtype, dev: torch.device, st) -> Tensor:
    """dW [E, C] f32 = dZ^T Y for row matrices dZ [P, E], Y [P, C] (a 1x1 conv's weight gradient over
    K = B*H*W pixels): both operands transposed to K-contiguous, then the split-K MFMA GEMM (K padded with
    zero columns to the GEMM's K step when P is not a multiple of it)."""
    dt = _lib.dtype_code(cdtype)
    P, E = dZ.shape
    C = Y.shape[1]
    kstep = 32 if cdtype == torch.float32 else 64
    Pp = -(-P // kstep) * kstep
    alloc = torch.empty if Pp == P else torch.zeros
    dZT = alloc(E, Pp, device=dev, dtype=cdtype)
    YT = alloc(C, Pp, device=dev, dtype=cdtype)
    _lib.check(L.ebc_transpose(dt, _lib.ptr(dZ), _lib.ptr(dZT), P, E, Pp, st), "ebc_transpose(dZ)")
    _lib.check(L.ebc_transpose(dt, _lib.ptr(Y), _lib.ptr(YT), P, C, Pp, st), "ebc_transpose(Y)")
    dW = torch.empty(E, C, device=dev, dtype=torch.float32)
    ws = _dec_workspace(dev, L.ebc_gemm_wgrad_workspace_bytes(dt, E, C, Pp), slot=2)
    _lib.check(L.ebc_gemm_wgrad(dt, _lib.ptr(dZT), _lib.ptr(YT), _lib.ptr(dW), E, C, Pp, _lib.ptr(ws), ws.numel(), st),
               "ebc_gemm_wgrad")
    return dW


def _prep_1x1(L, w: Tensor, cdtype: torch.dtype, st) -> Tuple[Tensor, Tensor]:
    """1x1 conv weight [N, K, 1, 1] f32 -> ([N, K], [K, N]) in the compute dtype, one launch (ebc_prep_weights_1x1)."""
    N, K = w.shape[0], w.shape[1]
    wk = torch.empty(N, K, device=w.device, dtype=cdtype)
    wt = torch.empty(K, N, device=w.device, dtype=cdtype)
    _lib.check(L.ebc_prep_weights_1x1(_lib.dtype_code(cdtype), _lib.ptr(w.detach().float().contiguous()), _lib.ptr(wk),
                                      _lib.ptr(wt), N, K, st), "ebc_prep_weights_1x1")
    return wk, wt


def _prep_3x3(L, w: Tensor, cdtype: torch.dtype, st) -> Tuple[Tensor, Tensor]:
    """3x3 conv weight [N, C, 3, 3] f32 -> ([N][3][3][C], and [C][3][3][N] flipped for the data gradient) in the
    compute dtype, one launch (ebc_dec_prep_weights)."""
    N, C = w.shape[0], w.shape[1]
    wk = torch.empty(N, 3, 3, C, device=w.device, dtype=cdtype)
    wf = torch.empty(C, 3, 3, N, device=w.device, dtype=cdtype)
    _lib.check(L.ebc_dec_prep_weights(_lib.dtype_code(cdtype), _lib.ptr(w.detach().float().contiguous()), _lib.ptr(wk),
                                      _lib.ptr(wf), N, C, st), "ebc_dec_prep_weights")
    return wk, wf


# ----------------------------------------------------------------------------- BatchNorm
def _bn_group(bn: nn.Module):
    """The process group a SyncBatchNorm exchanges its statistics over, None for no exchange.  Asked of
    model._bn_group at call time: `bench.py --syncbn-world1` replaces that module attribute at run time to force the
    exchange on a one-rank group, and the replacement must reach every BatchNorm of every block Function (the one
    function-level import between model.py and its helpers)."""
    from . import model
    return model._bn_group(bn)


def _bn_momentum(bn: nn.Module) -> float:
    """nn.BatchNorm2d's exponential_average_factor (momentum None: cumulative average)."""
    if bn.momentum is not None:
        return float(bn.momentum)
    return 1.0 / float(bn.num_batches_tracked.item())


class BNState(NamedTuple):
    """One BatchNorm's forward: its input rows z [P, N], the f32 statistics (scale = gamma * rstd, shift = beta -
    mean * scale), the count the finalize launch took (-1: read on device), the SyncBatchNorm group (None: no
    exchange) and the f64 [sum | sum of squares | count] buffer (None: normalised with the running statistics)."""
    z: Tensor
    mean: Tensor
    rstd: Tensor
    scale: Tensor
    shift: Tensor
    count: float
    pg: object
    colsum: Optional[Tensor]


def _batch_norm_fwd(L, bn: nn.Module, z: Tensor, training: bool, dt: int, ws: Tensor, st,
                    conv: Optional[Tuple[Tensor, Tensor, Geometry]] = None, fuse: bool = False) -> BNState:
    """BatchNorm2d statistics of the rows z [P, N].  Where the batch statistics come from:
      (a) conv = (padded input, prepared weight, geometry): z is still to be computed -- ebc_conv3x3_fwd writes it and
          leaves the column sums in its epilogue, ebc_bn_finalize follows;
      (b) conv None: z is given (a 1x1 product) -- without an exchange ebc_bn_stats_finalize, else ebc_bn_stats
          before the all-reduce and ebc_bn_finalize after it;
      (c) conv and fuse: as (a) in ONE launch (ebc_conv3x3_fwd_bn), taken only when nothing has to happen between
          the conv and the finalize (no exchange) and the launch's fixed protocol fits (running statistics updated
          with a host-known momentum, num_batches_tracked incremented by the launch).
    SyncBatchNorm: [sum | sum of squares | this rank's count] all-reduced in ONE f64 buffer, the total count read on
    device (count = -1), so ranks may hold different batch sizes (torch.nn.SyncBatchNorm gathers the per-rank counts
    the same way).  With the running statistics (eval mode of a BatchNorm that tracks them) there are no sums:
    ebc_bn_finalize(colsum NULL) reads the running buffers."""
    P, N = z.shape
    f32 = dict(device=z.device, dtype=torch.float32)
    use_batch = training or not bn.track_running_stats
    pg = _bn_group(bn) if use_batch else None
    colsum = torch.empty(2 * N + (pg is not None), device=z.device, dtype=torch.float64) if use_batch else None
    upd = training and bn.track_running_stats
    fuse = fuse and conv is not None and pg is None and upd and bn.momentum is not None
    rows = conv is None and use_batch              # (b): the statistics are still to be taken, over z
    if conv is not None and not fuse:
        inp, wk, g = conv
        _lib.check(L.ebc_conv3x3_fwd(dt, _lib.ptr(inp), _lib.ptr(wk), _lib.ptr(z), _lib.ptr(colsum), None, None,
                                     _lib.ptr(ws), ws.numel(), g.B, g.H, g.W, g.C, g.N, st), "ebc_conv3x3_fwd")
    elif rows and pg is not None:
        _lib.check(L.ebc_bn_stats(dt, _lib.ptr(z), _lib.ptr(colsum), _lib.ptr(ws), ws.numel(), P, N, st), "ebc_bn_stats")
    count = float(P)
    if pg is not None:
        colsum[2 * N].fill_(float(P))
        torch.distributed.all_reduce(colsum, group=pg)
        count = -1.0
    mean, rstd, scale, shift = (torch.empty(N, **f32) for _ in range(4))
    nbt = None                                     # num_batches_tracked += 1 inside the finalize launch
    if upd:
        if bn.momentum is None:                    # cumulative average: the factor needs the updated count now
            bn.num_batches_tracked.add_(1)
        else:
            nbt = _lib.ptr(bn.num_batches_tracked)
    mom = _bn_momentum(bn) if upd else 0.0
    gamma, beta = _lib.ptr(bn.weight.detach()), _lib.ptr(bn.bias.detach())
    out = (_lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(scale), _lib.ptr(shift))
    if fuse:
        inp, wk, g = conv
        _lib.check(L.ebc_conv3x3_fwd_bn(dt, _lib.ptr(inp), _lib.ptr(wk), _lib.ptr(z), _lib.ptr(ws), ws.numel(), g.B, g.H,
                                        g.W, g.C, g.N, float(bn.eps), mom, gamma, beta, *out, _lib.ptr(bn.running_mean),
                                        _lib.ptr(bn.running_var), nbt, _lib.ptr(colsum), st), "ebc_conv3x3_fwd_bn")
    elif rows and pg is None:
        # column sums and finalize in one launch; the sums themselves are not kept (colsum_out NULL)
        _lib.check(L.ebc_bn_stats_finalize(dt, _lib.ptr(z), _lib.ptr(ws), ws.numel(), P, N, float(bn.eps), mom, gamma,
                                           beta, *out, _lib.ptr(bn.running_mean) if upd else None,
                                           _lib.ptr(bn.running_var) if upd else None, None, nbt, st),
                   "ebc_bn_stats_finalize")
    else:
        running = upd or not use_batch             # updated, or read in place of the batch statistics
        _lib.check(L.ebc_bn_finalize(_lib.ptr(colsum), count, float(bn.eps), mom, gamma, beta, *out,
                                     _lib.ptr(bn.running_mean) if running else None,
                                     _lib.ptr(bn.running_var) if running else None, nbt, N, st), "ebc_bn_finalize")
    return BNState(z, mean, rstd, scale, shift, count, pg, colsum)


def _eval_coef(coef: Tensor, colsum: Optional[Tensor]) -> Tensor:
    """BatchNorm normalised with its running statistics (eval mode, or track_running_stats with use of the running
    estimates: no batch statistics, colsum None) has the input gradient gamma * rstd * g: the batch-mean terms
    coef[1] = mean(g), coef[2] = mean(g * xhat) of the train-mode backward are zero (torch batch_norm_backward with
    training=False); d gamma / d beta are the same column sums."""
    if colsum is None:
        coef[1:].zero_()
    return coef


def _batch_norm_bwd(L, gamma: Tensor, s: BNState, g: Tensor, mask: Optional[Tensor], dt: int, ws: Tensor, st
                    ) -> Tuple[Tensor, Tensor, Tensor]:
    """Column sums of the BatchNorm backward -> (d gamma, d beta, coef) for the gradient g at the BatchNorm's ReLU
    (mask: the ReLU's output, None: recomputed from z)."""
    P, N = s.z.shape
    f32 = dict(device=s.z.device, dtype=torch.float32)
    dg, db, coef = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(3, N, **f32)
    operands = (dt, _lib.ptr(g), _lib.ptr(mask), _lib.ptr(s.z), _lib.ptr(s.mean), _lib.ptr(s.rstd), _lib.ptr(s.scale),
                _lib.ptr(s.shift))
    gm = _lib.ptr(gamma.detach())
    if s.pg is None:                  # no exchange: column sums and finalize in one launch (count = P)
        _lib.check(L.ebc_bn_bwd_reduce_finalize(*operands, gm, _lib.ptr(dg), _lib.ptr(db), _lib.ptr(coef),
                                                _lib.ptr(ws), ws.numel(), P, N, st), "ebc_bn_bwd_reduce_finalize")
        return dg, db, _eval_coef(coef, s.colsum)
    # SyncBatchNorm backward (torch nn/modules/_functions.py): d gamma / d beta come from THIS rank's sums (DDP then
    # averages them over the ranks); the input gradient uses the all-reduced sums and the all-reduced count
    sums = torch.empty(2 * N + 1, device=s.z.device, dtype=torch.float64)
    _lib.check(L.ebc_bn_bwd_reduce(*operands, _lib.ptr(sums), _lib.ptr(ws), ws.numel(), P, N, st), "ebc_bn_bwd_reduce")
    _lib.check(L.ebc_bn_bwd_finalize(_lib.ptr(sums), float(P), gm, _lib.ptr(s.rstd), _lib.ptr(dg), _lib.ptr(db),
                                     _lib.ptr(coef), N, st), "ebc_bn_bwd_finalize")
    torch.distributed.all_reduce(sums[: 2 * N], group=s.pg)       # sum_dy, sum_dy_xmu
    sums[2 * N:].copy_(s.colsum[2 * N:])                          # the forward's all-reduced count
    _lib.check(L.ebc_bn_bwd_finalize(_lib.ptr(sums), s.count, gm, _lib.ptr(s.rstd), None, None, _lib.ptr(coef), N, st),
               "ebc_bn_bwd_finalize(sync)")
    return dg, db, _eval_coef(coef, s.colsum)


# ----------------------------------------------------------------------------- conv + BatchNorm stages
def _conv3x3_fwd(L, bn: nn.Module, inp: Tensor, wk: Tensor, g: Geometry, training: bool, dt: int, ws: Tensor, st,
                 fuse: bool = False) -> BNState:
    """3x3 conv of the padded image inp [Q, C] with the BatchNorm statistics of its output in the epilogue, then bn's
    statistics.  fuse: allow the one-launch conv + finalize (_batch_norm_fwd (c)).  Only _DecoderFn passes it: the
    resnet Functions' 3x3 stays on the unfused pair until a change of its own measures the other launch."""
    z = torch.empty(g.P, g.N, device=inp.device, dtype=inp.dtype)
    return _batch_norm_fwd(L, bn, z, training, dt, ws, st, conv=(inp, wk, g), fuse=fuse)


def _conv3x3_bwd(L, s: BNState, gamma: Tensor, gz: Tensor, mask: Optional[Tensor], inp: Tensor, wf: Tensor,
                 g: Geometry, dt: int, ws: Tensor, ws_wgrad: Tensor, st, add_gy: Optional[Tensor] = None,
                 add_y: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Backward of _conv3x3_fwd (+ the ReLU after it, see _batch_norm_bwd) -> (dx [P, C], dW [N, C, 3, 3] f32,
    d gamma, d beta).  inp: the conv's padded input, wf: its flipped weight.  add_gy / add_y: the data gradient also
    takes a residual branch's gradient add_gy * (add_y > 0)."""
    dev, cdtype = inp.device, inp.dtype
    dgm, dbt, coef = _batch_norm_bwd(L, gamma, s, gz, mask, dt, ws, st)
    dzpad = torch.empty(g.Q, g.N, device=dev, dtype=cdtype)
    dzT = torch.empty(g.N, g.Qs, device=dev, dtype=cdtype)
    _lib.check(L.ebc_bn_bwd_apply(dt, _lib.ptr(gz), _lib.ptr(mask), _lib.ptr(s.z), _lib.ptr(s.mean), _lib.ptr(s.rstd),
                                  _lib.ptr(s.scale), _lib.ptr(s.shift), _lib.ptr(coef), _lib.ptr(dzpad), _lib.ptr(dzT),
                                  g.B, g.H, g.W, g.N, st), "ebc_bn_bwd_apply")
    xT3 = torch.empty(3, g.C, g.Qs, device=dev, dtype=cdtype)
    _lib.check(L.ebc_dec_transpose3(dt, _lib.ptr(inp), _lib.ptr(xT3), g.B, g.H, g.W, g.C, st), "ebc_dec_transpose3")
    dw = torch.empty(g.N, g.C, 3, 3, device=dev, dtype=torch.float32)
    _lib.check(L.ebc_conv3x3_wgrad(dt, _lib.ptr(dzT), _lib.ptr(xT3), _lib.ptr(dw), _lib.ptr(ws_wgrad), ws_wgrad.numel(),
                                   g.B, g.H, g.W, g.C, g.N, st), "ebc_conv3x3_wgrad")
    del xT3, dzT
    dx = torch.empty(g.P, g.C, device=dev, dtype=cdtype)
    _lib.check(L.ebc_conv3x3_fwd(dt, _lib.ptr(dzpad), _lib.ptr(wf), _lib.ptr(dx), None, _lib.ptr(add_gy), _lib.ptr(add_y),
                                 _lib.ptr(ws), ws.numel(), g.B, g.H, g.W, g.N, g.C, st), "ebc_conv3x3_fwd(dgrad)")
    return dx, dw, dgm, dbt


def _conv1x1_fwd(L, bn: nn.Module, x: Tensor, wk: Tensor, training: bool, dt: int, ws: Tensor, st) -> BNState:
    """1x1 conv of the rows x [P, K] with the prepared weight wk [N, K] (an MFMA GEMM), then bn's statistics."""
    P, (N, K) = x.shape[0], wk.shape
    z = torch.empty(P, N, device=x.device, dtype=wk.dtype)
    _lib.check(L.ebc_gemm(dt, 0, 0, _lib.ptr(x), _lib.ptr(wk), _lib.ptr(z), None, None, None, P, N, K, st), "ebc_gemm(1x1)")
    return _batch_norm_fwd(L, bn, z, training, dt, ws, st)


def _conv1x1_bwd(L, s: BNState, gamma: Tensor, gz: Tensor, mask: Optional[Tensor], x: Tensor, wt: Tensor, dt: int,
                 ws: Tensor, st, gmask: Optional[Tensor] = None, resid: Optional[Tensor] = None,
                 out: Optional[Tensor] = None, out_f32: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Backward of _conv1x1_fwd (+ the ReLU after it) -> (dx [P, K], dW [N, K] f32, d gamma, d beta).  x: the conv's
    input rows, wt: its transposed weight [K, N].  gmask: also receives gz * relu' in f32 (an identity branch's
    gradient); resid (f32): added to dx; out / out_f32: where and in which type dx is written (default: new rows in
    the compute dtype; out may be resid itself)."""
    dev, cdtype = s.z.device, s.z.dtype
    P, N = s.z.shape
    K = x.shape[1]
    dgm, dbt, coef = _batch_norm_bwd(L, gamma, s, gz, mask, dt, ws, st)
    dz = torch.empty(P, N, device=dev, dtype=cdtype)
    _lib.check(L.ebc_bn_bwd_apply_flat(dt, _lib.ptr(gz), _lib.ptr(mask), _lib.ptr(s.z), _lib.ptr(s.mean), _lib.ptr(s.rstd),
                                       _lib.ptr(s.scale), _lib.ptr(s.shift), _lib.ptr(coef), _lib.ptr(dz), _lib.ptr(gmask),
                                       P, N, st), "ebc_bn_bwd_apply_flat")
    dw = _wgrad_rows(L, dz, x, cdtype, dev, st)
    if out is None:
        out = torch.empty(P, K, device=dev, dtype=torch.float32 if out_f32 else cdtype)
    _lib.check(L.ebc_gemm(dt, 0 if resid is None else 2, int(out_f32), _lib.ptr(dz), _lib.ptr(wt), _lib.ptr(out), None,
                          _lib.ptr(resid), None, P, K, N, st), "ebc_gemm(1x1 dX)")
    return out, dw, dgm, dbt
