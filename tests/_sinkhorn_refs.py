"""Float64 numpy restatement of the reference's sinkhorn() (losses/bregman_pytorch.py:11-144) as csrc/sinkhorn.hip
states it, the per-element error bounds of the kernel's outputs, the case list of tests/test_gpu_sinkhorn_kernel.py, and
an f32 numpy stand-in of the kernel that can be corrupted.

The restatement takes the same f32 a, b, C and reg and keeps the reference's operands: u0 = 1 / na and v0 = 1 / nb as
f32 quotients, the 1e-16 epsilons as the f32 the reference's tensors hold, K = exp(C / -reg), the err check every
eval_freq iterations (log only), the stop rule `err > stop_thr and it <= max_iter` with err starting at 1, the rollback
to the previous (u, v) when a new one is not finite in f32 (NaN, inf, or past FLT_MAX), alpha = reg log(u + eps), beta = reg log(v + eps), P = u K v.

Bounds, in log space (UL = -log(1 - 2^-24): one f32 rounding moves a positive value by a factor within e^(+-UL)).  With
K > 0, v_j = b_j / (sum_i K_ij u_i + eps) is b_j over a positive-weighted sum, so operands within e^(+-d) of the
reference's move v_j by at most e^(+-d); the same holds for u.  Per update, from the code:

  k_K  K = expf(C / -reg): the quotient's rounding moves the exponent by |C / reg| 2^-24, expf is taken at 2 ulp = 4
       roundings' worth: k_K = max |C / reg| + 4.
  d_v  the column's na fused multiply-adds (each term passes through at most na roundings), the epsilon add, the
       division: (na + 2 + k_K) UL.
  d_u  the lane's stride-64 sum of ceil(nb / 64) fused multiply-adds, six butterfly adds, the epsilon add, the
       division: (ceil(nb / 64) + 8 + k_K) UL.

After T iterations u is within T (d_v + d_u) and v within T (d_v + d_u) - d_u (v is updated first).  From these:

  alpha, beta   reg (d + UL + 2 ulp(log)) + half an ulp of the result, absolute: the epsilon add, logf at 2 ulp, the
                product's rounding.
  P             d_u + d_v + (|C_ij / reg| + 4 + 2) UL: the element's own K and the two products.
  err           the kernel's b_hat_j = (K^T u)_j v_j is within e^(+-(d_u + d_v + (na + k_K + 1) UL)) of the reference's
                and the difference b_j - b_hat_j rounds once: E_j = b_hat_j expm1(..) + 2^-24 |b_j - b_hat_j|;
                |err - err_ref| <= sum_j (2 |r_j| E_j + E_j^2)  (<= 2 sqrt(err_ref) E + E^2 with E^2 = sum E_j^2), plus
                the sum itself: ceil(nb / 1024) fused multiply-adds per thread, 6 butterfly adds and 16 wave results.

expf and logf are taken at 2 ulp each; ROCm's device library documents 1 ulp for both (the OCML accuracy table of the
ROCm device-libs documentation).  The allowance is the looser one on purpose: it is not a measured figure.
"""
import math

import numpy as np
import torch

import _bn_refs as R

U = R.U32
UL = -math.log1p(-U)
F32, F64 = np.float32, np.float64
EPS = F64(F32(1e-16))
LDS_MAX = 160 * 1024


def ulp32(x):
    return R.ulp(torch.from_numpy(np.ascontiguousarray(np.asarray(x, F64))), torch.float32).numpy()


# ------------------------------------------------------------------------------------------------ the restatement
def _finite32(x):
    """The reference's isnan / isinf test is made on f32 tensors: a value past FLT_MAX is an inf there."""
    return bool((np.abs(x) <= F64(np.finfo(F32).max)).all())          # (NaN compares false)


def sinkhorn_f64(a, b, C, reg, max_iter, stop_thr, eval_freq, log):
    a, b, C = (np.asarray(x, F32).astype(F64) for x in (a, b, C))
    reg, thr = F64(F32(reg)), F64(F32(stop_thr))
    na, nb = C.shape
    with np.errstate(all="ignore"):
        K = np.exp(C / -reg)
        u = np.full(na, F64(F32(1.0) / F32(na)))
        v = np.full(nb, F64(F32(1.0) / F32(nb)))
        it, err, errs, bhats, rolled = 1, 1.0, [], [], False
        while err > thr and it <= max_iter:
            upre, vpre = u, v
            v = b / (u @ K + EPS)
            u = a / (K @ v + EPS)
            if not (_finite32(u) and _finite32(v)):
                u, v, rolled = upre, vpre, True
                break
            if log and it % eval_freq == 0:
                bhat = (u @ K) * v
                err = float(((b - bhat) ** 2).sum())
                errs.append(err)
                bhats.append(bhat)
            it += 1
        iters = it if rolled else it - 1
        return dict(bhat=bhats, K=K, u=u, v=v, alpha=reg * np.log(u + EPS), beta=reg * np.log(v + EPS), P=u[:, None] * K * v[None, :],
                    err=np.array(errs, F64), info=(-iters if rolled else iters, len(errs)), T=0 if rolled else iters,
                    rolled=rolled)


# ------------------------------------------------------------------------------------------------ the bounds
def k_K(C, reg):
    return float(np.abs(np.asarray(C, F64) / F64(F32(reg))).max()) + 4.0


def d_steps(na, nb, kk):
    return (na + 2 + kk) * UL, (-(-nb // 64) + 8 + kk) * UL


def d_uv(na, nb, kk, T):
    dv, du = d_steps(na, nb, kk)
    d_u = T * (dv + du)
    return d_u, max(d_u - du, 0.0)


def bounds(a, b, C, reg, r, eval_freq=1):
    """Per output kind: (what is compared, the bound).  u, v and P are compared as |log(out / ref)|."""
    na, nb = np.asarray(C).shape
    reg64 = F64(F32(reg))
    kk = k_K(C, reg)
    d_u, d_v = d_uv(na, nb, kk, r["T"])
    q = np.abs(np.asarray(C, F32).astype(F64) / reg64)
    out = dict(u=np.full(na, d_u), v=np.full(nb, d_v), P=d_u + d_v + (q + 6.0) * UL)
    for name, x, d in (("alpha", r["u"], d_u), ("beta", r["v"], d_v)):
        lg = np.log(x + EPS)
        pre = reg64 * (d + UL + 2 * ulp32(lg))
        out[name] = pre + 0.5 * ulp32(np.abs(reg64 * lg) + pre)
    eb = []
    for k in range(len(r["err"])):
        T_at = (k + 1) * eval_freq
        bhat = r["bhat"][k]
        res = np.asarray(b, F32).astype(F64) - bhat
        du_k, dv_k = d_uv(na, nb, kk, T_at)
        E = np.abs(bhat) * np.expm1(du_k + dv_k + (na + kk + 1) * UL) + U * np.abs(res)
        e = float((2 * np.abs(res) * E + E * E).sum())
        eb.append(e + (-(-nb // 1024) + 22) * U * (r["err"][k] + e))
    out["err"] = np.array(eb, F64)
    return out


def log_err(out, ref):
    """|log(out / ref)| per element; a non-positive or non-finite output is an infinite error."""
    out, ref = np.asarray(out, F64), np.asarray(ref, F64)
    with np.errstate(all="ignore"):
        e = np.abs(np.log(out) - np.log(ref))
    return np.where(np.isfinite(e), e, np.inf)


def compare(got, r, B):
    """{kind: (err, bound)} of a kernel's outputs `got` (those it was asked for) against the reference r."""
    res = {}
    for k in ("u", "v", "P"):
        if k in got:
            res[k] = (log_err(got[k], r[k]).reshape(-1), np.broadcast_to(B[k], r[k].shape).reshape(-1))
    for k in ("alpha", "beta"):
        if k in got:
            res[k] = (np.abs(np.asarray(got[k], F64) - r[k]), B[k])
    if "err" in got and len(r["err"]):
        res["err"] = (np.abs(np.asarray(got["err"], F64) - r["err"]), B["err"])
    return res


def ratio(err, bound):
    err, bound = np.asarray(err, F64).reshape(-1), np.asarray(bound, F64).reshape(-1)
    if not err.size:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    return float(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ sizes
def uv_bytes(na, nb):
    return 4 * (2 * na + 3 * nb + 64)


def workspace_bytes(na, nb):
    """ebc_sinkhorn_workspace_bytes: K goes to the workspace when both u, both v, K^T u, 64 scratch words and K together
    pass 160 KiB of LDS (csrc/sinkhorn.hip uv_bytes, k_in_lds)."""
    return 0 if uv_bytes(na, nb) + 4 * na * nb <= LDS_MAX else 4 * na * nb


# ------------------------------------------------------------------------------------------------ cases
FAMILIES = {
    "tiny": [(1, 1), (1, 70), (70, 1)],
    "small": [(17, 63), (33, 65)],
    "wide": [(5, 1025), (3, 2051)],
    "lds": [(199, 199)],
    "ws": [(200, 200)],
    "switch": [(40, 1000), (41, 1000)],
    "big": [(1, 13631)],
}
SHAPES = [(fam, na, nb) for fam, shapes in FAMILIES.items() for na, nb in shapes]
REG = 0.5
QMAX = 20.0            # max |C / reg| of every case but the epsilon one


def problem(na, nb, seed=0):
    """a, b > 0 summing to 1 and the cost 20 reg (x_i - y_j)^2 of sorted points on [0, 1): C / reg in [0, 20), K >= e^-20
    > 1e-9.  (A cost of independent random entries converges within ten iterations; this one is still moving at the
    third err check of the 100-iteration runs.)"""
    g = np.random.Generator(np.random.PCG64(1000 * na + nb + seed))
    a = g.random(na) + 0.2
    b = g.random(nb) + 0.2
    x, y = np.sort(g.random(na)), np.sort(g.random(nb))
    C = (x[:, None] - y[None, :]) ** 2 * (QMAX * REG * 0.999)
    return (a / a.sum()).astype(F32), (b / b.sum()).astype(F32), C.astype(F32)


def epsilon_problem():
    """(8, 64): column 5 of C has C / reg = 36.8 in every row, so its K^T u is near 1e-16 and the epsilon in the
    denominator moves v_5 by a factor near 2."""
    a, b, C = problem(8, 64, seed=3)
    C[:, 5] = F32(36.8 * REG)
    return a, b, C


class Run:
    def __init__(self, name, max_iter, eval_freq, log, thr=-1.0):
        self.name, self.max_iter, self.eval_freq, self.log, self.thr = name, max_iter, eval_freq, log, thr

    def nerr_cap(self):
        return self.max_iter // self.eval_freq


def stop_threshold(a, b, C):
    """The geometric mean of the second and third err check of the 100-iteration run (eval_freq 10) where both, and the
    first, are a factor 10 or more from it; None where they are not (the run was at rounding level before the third
    check).  The iteration count is then the inputs', not the rounding's."""
    e = sinkhorn_f64(a, b, C, REG, 100, -1.0, 10, 1)["err"]
    thr = math.sqrt(e[1] * e[2])
    if min(e[0], e[1]) >= 10 * thr and e[2] * 10 <= thr and e[2] >= 1e-15:
        return float(F32(thr))
    return None


def runs(a, b, C):
    out = [Run("T1", 1, 1, 1), Run("T2", 2, 1, 1), Run("T4", 4, 1, 1), Run("T100", 100, 10, 1),
           Run("T25", 25, 10, 1), Run("T5f7", 5, 7, 1), Run("T4f2", 4, 2, 1), Run("T4nolog", 4, 1, 0), Run("T0", 0, 1, 1),
           Run("thr1", 100, 1, 1, thr=1.0)]
    thr = stop_threshold(a, b, C)
    if thr is not None:
        out.append(Run("T100stop", 100, 10, 1, thr=thr))
    return out


STOP_SHAPES = [(17, 63), (33, 65), (199, 199), (200, 200), (40, 1000), (41, 1000)]   # the shapes that must have a stop run


# ------------------------------------------------------------------------------------------------ f32 stand-in
def sinkhorn_standin(a, b, C, reg, max_iter, stop_thr, eval_freq, log, bug=None):
    """The kernel's loop in f32 numpy (sums in numpy's order).  bug: "swap_ij", "row_stop_64", "col_stop_1024",
    "eps_1e-12", "ktu_stale", "err_shift", "info_it"."""
    a, b, C = (np.asarray(x, F32) for x in (a, b, C))
    reg, thr = F32(reg), F32(stop_thr)
    eps = F32(1e-12) if bug == "eps_1e-12" else F32(1e-16)
    na, nb = C.shape
    with np.errstate(all="ignore"):
        K = np.exp(C / -reg).astype(F32)
        u = np.full(na, F32(1.0) / F32(na), F32)
        v = np.full(nb, F32(1.0) / F32(nb), F32)
        it, err, rolled, ktu, uses = 1, F32(1.0), False, None, 0
        errs = np.full(max_iter // eval_freq + 2, 7.0, F32)
        nerr = 0
        nbr = nb & ~63 if bug == "row_stop_64" else nb
        nbc = min(nb, 1024) if bug == "col_stop_1024" else nb
        while err > thr and it <= max_iter:
            upre, vpre = u, v
            s = ktu if uses > 0 else (u @ K).astype(F32)
            uses -= 1
            v = vpre.copy()
            v[:nbc] = (b / (s + eps)).astype(F32)[:nbc]
            u = (a / ((K[:, :nbr] @ v[:nbr]).astype(F32) + eps)).astype(F32)
            if not (_finite32(u) and _finite32(v)):
                u, v, rolled = upre, vpre, True
                break
            if log and it % eval_freq == 0:
                ktu, uses = (u @ K).astype(F32), (2 if bug == "ktu_stale" else 1)
                err = F32(((b - ktu * v) ** 2).sum(dtype=F32))
                errs[nerr + (1 if bug == "err_shift" else 0)] = err
                nerr += 1
            it += 1
        iters = it if (rolled or bug == "info_it") else it - 1
        P = u[:, None] * K * v[None, :]
        if bug == "swap_ij":
            P = u[np.arange(nb) % na][None, :] * K * v[np.arange(na) % nb][:, None]      # (the kernel would read past u)
        return dict(u=u, v=v, alpha=reg * np.log(u + eps), beta=reg * np.log(v + eps), P=P.astype(F32),
                    err=errs[:nerr].copy(), err_buf=errs, info=(-iters if rolled else iters, nerr))
