"""Plain float64 restatement of one crop of the fused DACE / DMCount loss (csrc/dace_loss.hip).

Written from the reference project's lines, with a dense K = exp(C / -reg) of shape [n, g*g] and no shortcut through
the kernel's arithmetic (no separable factors, no windows, no buckets):
  block sums      losses/utils.py:4-9
  bin labels      losses/dace_loss.py:42-47   inclusive bins, later bins win, label 0 when no bin matches
  cross-entropy   losses/dace_loss.py:49-55   summed over the cells, mean over the batch
  DMLoss          losses/dm_loss.py:99-124    normed pred / target (1e-8), TV * n, |count difference|
  OTLoss          losses/dm_loss.py:38-79     cost from cood = k*red + red/2 (optionally norm_cood), gradient, wd
  sinkhorn        losses/bregman_pytorch.py:11-144   v then u, err every eval_freq, 1e-16, non-finite roll-back
Inputs are f32 arrays taken as exact; all arithmetic is numpy float64.  tests/test_loss_refs_cpu.py pins this file
against the reference project's recorded outputs, torch float64 autograd and the f32 C restatement (oracle.ref);
tests/test_gpu_loss_kernels.py checks the kernel against it.
"""
import numpy as np

F64 = np.float64
EPS = 1e-8            # dm_loss.py:7
M_EPS = 1e-16         # bregman_pytorch.py:8
DMCOUNT, MAE, MSE, OT_ONLY = 0, 1, 2, 3       # include/ebc_hip.h EBC_COUNT_*


def block_sums(dot_map, red):
    """losses/utils.py:4-9: red x red block sums of a [S][S] map."""
    S = dot_map.shape[0]
    g = S // red
    out = np.zeros((g, g), F64)
    for i in range(g):
        for j in range(g):
            out[i, j] = dot_map[i * red:(i + 1) * red, j * red:(j + 1) * red].astype(F64).sum()
    return out


def bin_labels(density, bins_lo, bins_hi):
    """dace_loss.py:42-47: label = the last bin k with lo[k] <= d <= hi[k] (both ends inclusive), 0 when none."""
    d = np.asarray(density, F64)
    cls = np.zeros(d.shape, np.int64)
    for k in range(len(bins_lo)):
        cls[(d >= F64(bins_lo[k])) & (d <= F64(bins_hi[k]))] = k
    return cls


def cross_entropy(logits, labels):
    """Per-cell CE [g][g] and softmax - onehot [N][g][g] for logits [N][g][g] (no 1/B yet)."""
    z = logits.astype(F64)
    mx = z.max(0)
    lse = mx + np.log(np.exp(z - mx).sum(0))
    N = z.shape[0]
    onehot = (np.arange(N)[:, None, None] == labels[None]).astype(F64)
    ce = lse - (z * onehot).sum(0)
    return ce, np.exp(z - lse) - onehot


def cood(g, size, red, norm):
    """dm_loss.py:31-34: cell centres arange(0, size, red) + red / 2, mapped to [-1, 1] when norm_cood."""
    c = np.arange(g, dtype=F64) * red + red / 2.0
    return c / size * 2.0 - 1.0 if norm else c


def cost_matrix(points, g, size, red, norm):
    """dm_loss.py:51-59: C[i, iy*g + jx] = (y_i - c[iy])^2 + (x_i - c[jx])^2, written as the reference expands it."""
    c = cood(g, size, red, norm)
    p = points.astype(F64).reshape(-1, 2)
    if norm:
        p = p / size * 2.0 - 1.0                     # dm_loss.py:51
    x, y = p[:, 0:1], p[:, 1:2]
    xd = -2.0 * x * c[None] + x * x + c[None] * c[None]         # [n][g]
    yd = -2.0 * y * c[None] + y * y + c[None] * c[None]
    return (yd[:, :, None] + xd[:, None, :]).reshape(len(p), g * g)


def sinkhorn(a, b, C, reg, max_iter, stop_thr, eval_freq):
    """bregman_pytorch.py:11-144 in float64, with the reference's control flow."""
    K = np.exp(C / -reg)
    n, M = K.shape
    u = np.full(n, 1.0 / n, F64)
    v = np.full(M, 1.0 / M, F64)
    it, err, rolled, errs, resid = 1, 1.0, False, [], None
    while err > stop_thr and it <= max_iter:                     # :102
        upre, vpre = u, v
        with np.errstate(all="ignore"):
            v = b / (K.T @ u + M_EPS)
            u = a / (K @ v + M_EPS)
        if not (np.isfinite(u).all() and np.isfinite(v).all()):  # :111-115
            u, v, rolled = upre, vpre, True
            break
        if it % eval_freq == 0:                                  # :117-126
            resid = b - (K.T @ u) * v
            err = float((resid ** 2).sum())
            errs.append(err)
        it += 1
    return dict(u=u, v=v, K=K, iters=it if rolled else it - 1, rolled_back=rolled, err=np.array(errs, F64),
                resid_last=resid)


def ot_crop(points, pred_density, size, red, reg=10.0, max_iter=100, stop_thr=1e-9, eval_freq=10, norm=False):
    """OTLoss.forward for one crop with n > 0 points (dm_loss.py:49-77): beta, the gradient w.r.t. pred_density,
    the surrogate loss sum(pd * grad) and wd = sum(P * C)."""
    pd = pred_density.astype(F64).reshape(-1)
    g = int(round(np.sqrt(pd.size)))
    n = len(points)
    pc = pd.sum()
    C = cost_matrix(points, g, size, red, norm)
    s = sinkhorn(np.full(n, 1.0 / n, F64), pd / (pc + EPS), C, F64(np.float32(reg)), max_iter, F64(np.float32(stop_thr)),
                 eval_freq)
    beta = F64(np.float32(reg)) * np.log(s["v"] + M_EPS)         # bregman_pytorch.py:137
    den = pc * pc + EPS
    grad = (pc * beta - (pd * beta).sum()) / den                 # dm_loss.py:65-74
    P = s["u"][:, None] * s["K"] * s["v"][None]
    return dict(beta=beta, ot_grad=grad, loss=float((pd * grad).sum()), wd=float((P * C).sum()), u=s["u"], v=s["v"],
                err=s["err"], resid_last=s["resid_last"], iters=s["iters"], rolled_back=s["rolled_back"],
                loss_abs=float(np.abs(pd * grad).sum()), wd_abs=float(np.abs(P * C).sum()))


def sgn(x):
    return np.sign(x)


def crop(pred_class, pred_density, target, points, bins_lo, bins_hi, size, red, B, mode=DMCOUNT, norm=False,
         w_count=1.0, w_ot=0.1, w_tv=0.01, reg=10.0, max_iter=100, stop_thr=1e-9, eval_freq=10):
    """One crop of the loss, everything the kernel writes for it.

    pred_class [N][g][g], pred_density [g][g], target: the [size][size] dot map or the reduced [g][g] map,
    points [n][2] (x, y).  B is the batch size (the gradients carry 1/B).  The weights, reg and stop_thr are taken
    at their f32 values (what the ABI passes).  Returns a dict of float64 arrays / scalars:
      td, labels, ce_cell, ce, grad_class, tv_n (TV * n), count, ot, wd, beta (zeros for n = 0), iters, rolled_back,
      err (every check), err_last (-1 if none), resid_last (b - K^T u * v per cell at the last check; crops with a
      check only), ot_grad, tv_grad, count_grad, grad_density, d (normed pred - normed target: the TV gradient's sign
      argument), pc, and the sums of |terms| behind ot and wd (ot_abs, wd_abs).
    """
    w_count, w_ot, w_tv = (F64(np.float32(w)) for w in (w_count, w_ot, w_tv))
    pd = pred_density.astype(F64)
    g = pd.shape[0]
    n = len(points)
    td = target.astype(F64) if target.shape[0] == g else block_sums(target, red)
    labels = bin_labels(td, bins_lo, bins_hi)
    ce_cell, dce = cross_entropy(pred_class, labels)
    out = dict(td=td, labels=labels, ce_cell=ce_cell, ce=float(ce_cell.sum()), grad_class=dce / B, n=n)
    pc = pd.sum()
    out["pc"] = pc
    zeros = np.zeros((g, g), F64)
    out.update(beta=zeros.reshape(-1), ot=0.0, wd=0.0, iters=0, rolled_back=False, err=np.zeros(0), err_last=-1.0,
               ot_grad=zeros, tv_grad=zeros, count_grad=zeros, ot_abs=0.0, wd_abs=0.0)
    if mode in (MAE, MSE):                                       # dace_loss.py:57-62
        d = pd - td
        out["d"] = d
        out["count"] = float((np.abs(d) if mode == MAE else d * d).sum())
        out["count_abs"] = out["count"]
        out["tv_n"] = 0.0
        out["count_grad"] = (sgn(d) if mode == MAE else 2.0 * d) / B
        out["grad_density"] = w_count * out["count_grad"]
        return out
    tc = F64(n)
    d = pd / (pc + EPS) - td / (tc + EPS)                        # dm_loss.py:105-110
    out["d"] = d
    out["tv_n"] = float(np.abs(d).sum() * tc)
    out["count"] = float(abs(pc - tc))
    tvk = (sgn(d) * pd).sum()
    out["tv_grad"] = tc / B * (sgn(d) / (pc + EPS) - tvk / (pc + EPS) ** 2)
    out["count_grad"] = np.full((g, g), sgn(pc - tc) / B)
    if n > 0:
        o = ot_crop(points, pd, size, red, reg, max_iter, stop_thr, eval_freq, norm)
        out.update(beta=o["beta"], ot=o["loss"], wd=o["wd"], iters=o["iters"], rolled_back=o["rolled_back"], err=o["err"],
                   err_last=float(o["err"][-1]) if len(o["err"]) else -1.0, ot_grad=o["ot_grad"].reshape(g, g),
                   ot_abs=o["loss_abs"], wd_abs=o["wd_abs"], resid_last=o["resid_last"])
    if mode == OT_ONLY:
        out["grad_density"] = w_count * (w_ot * out["ot_grad"])
    else:
        out["grad_density"] = w_count * (w_ot * out["ot_grad"] + w_tv * out["tv_grad"] + out["count_grad"])
    return out


def finalize(stats, mode, w_count, w_ot, w_tv):
    """losses[5] = loss, ot, tv, count, ce from the per-crop stats [B][>=4] (ce, tv*n, count, ot):
    dace_loss.py:64-70, dm_loss.py:111-122 (OT summed over the crops, the others batch means)."""
    s = np.asarray(stats, F64)
    B = s.shape[0]
    w_count, w_ot, w_tv = (F64(np.float32(w)) for w in (w_count, w_ot, w_tv))
    ce, tv, cnt, ot = s[:, 0].sum() / B, s[:, 1].sum() / B, s[:, 2].sum() / B, s[:, 3].sum()
    if mode == DMCOUNT:
        return np.array([ce + w_count * (ot * w_ot + tv * w_tv + cnt), ot, tv, cnt, ce])
    if mode == OT_ONLY:
        return np.array([w_count * w_ot * ot, ot, 0.0, 0.0, ce])
    return np.array([ce + w_count * cnt, 0.0, 0.0, cnt, ce])


def windows(points, size, red, reg, norm=False, slack=0.0):
    """Per point, how many cells of each axis (ny [n], nx [n]) have a nonzero f32 exp(d / -reg), with d the f32
    squared distance the kernel forms: (-2 (p c) + p p) + c c.  The kernel reads its windows off such f32 factors;
    a window wider than 9 cells sends the crop from the bucketed to the dense path.  `slack` is added to the
    exponent first: +s gives an upper bound, -s a lower bound that no rounding of the device's expf can cross."""
    f = np.float32
    g = size // red
    c = (np.arange(g) * red).astype(f) + f(0.5) * f(red)
    p = points.astype(f).reshape(-1, 2)
    if norm:
        c = c / f(size) * f(2.0) - f(1.0)
        p = p / f(size) * f(2.0) - f(1.0)
    out = []
    for a in (1, 0):                                             # y, then x
        q = p[:, a:a + 1]
        d = (f(-2.0) * (q * c[None]) + q * q) + c[None] * c[None]
        with np.errstate(under="ignore"):
            e = np.exp((d / f(-reg) + f(slack)).astype(f))
        out.append((e != 0).sum(1))
    return out[0], out[1]
