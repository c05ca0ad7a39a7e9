"""The fused DACE / DMCount loss kernel (csrc/dace_loss.hip) against the float64 reference of tests/_loss_refs.py, at
the ABI level (ebc_dace_loss_h / ebc_dace_loss), per crop and per cell, on every LDS grid and Sinkhorn path.

The launches (tests/_loss_cases.py) cover the nine LDS grids at an exact and a padded density grid, g = 1 and g = 3,
cell pitches 16 and 32, the LDS capacity boundaries ebc_dace_plan reports, and every setting off its default at least
once on a grid no other module runs (G = 24, 32, 40); tests/test_loss_refs_cpu.py asserts their input conditions and
their coverage of the plan without a GPU.  Every output lives in a framed sentinel buffer, the workspace is framed at
exactly ebc_dace_workspace_bytes.  Each check prints "RATIO <launch>.<quantity> <largest error / bound>".

u = 2^-24 below.  A block sum is the kernel's 1024-thread sum: a thread adds at most 4 of the 64 x 64 cells (4
roundings, the first onto 0), the wave sum 6 more, the 16 wave results 16 more: at most 26 roundings, so its error is
at most 26 u times the sum of |terms|.  expf and logf are taken at 1 ulp (2 u relative).
"""
import ctypes

import numpy as np
import pytest
import torch

import _bn_refs as R
import _kernel_checks as KC
import _loss_cases as LC
import _loss_refs as LR
from ebc_amd import _lib

pytestmark = pytest.mark.gpu

U = LC.U
F32 = torch.float32
BS = 26                       # roundings of a block sum (module docstring)


def _ulp32(x):
    return R.ulp(torch.as_tensor(np.asarray(x, np.float64)), F32).numpy()


def _report(name, out, ref, bound):
    out, ref, bound = (np.atleast_1d(np.asarray(a, np.float64)).reshape(-1) for a in (out, ref, bound))
    KC._report(name, torch.from_numpy(np.abs(out - ref)), torch.from_numpy(bound + 0.5 * _ulp32(ref)))


def _launch(L, reverse=False, device_meta=False):
    """One call; returns the outputs as numpy arrays.  Asserts the return code and that every frame is intact."""
    lib = _lib.lib()
    I = LC.inputs(L)
    B, g, N = L.B, L.g, len(L.bins)
    H = KC._Hold()
    fr = dict(gc=KC._Framed(B, N * g * g, F32), gd=KC._Framed(B, g * g, F32), stats=KC._Framed(B, 8, F32),
              losses=KC._Framed(1, 5, F32), status=KC._Framed(B, 1, torch.int32))
    with_beta = L.mode not in (LR.MAE, LR.MSE)             # (the mae / mse modes run no OT and write no beta)
    if with_beta:
        fr["beta"] = KC._Framed(B, g * g, F32)
    total = int(L.offsets[-1])
    ws_bytes = lib.ebc_dace_workspace_bytes(B, total, L.size, L.red)
    assert ws_bytes % 8 == 0
    fr["ws"] = KC._Framed(ws_bytes // 8, 8, torch.uint8)
    pts = np.concatenate(I["points"], 0) if total else np.zeros((1, 2), np.float32)
    order = list(range(B))[::-1] if reverse else sorted(range(B), key=lambda i: -L.counts[i])
    if device_meta:
        fn = lib.ebc_dace_loss
        offs = H(torch.from_numpy(L.offsets.copy()))
        ordr = H(torch.tensor(order, dtype=torch.int32))
    else:
        fn = lib.ebc_dace_loss_h
        offs = (ctypes.c_int * (B + 1))(*[int(o) for o in L.offsets])
        ordr = (ctypes.c_int * B)(*order)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rc = fn(H(t(I["pred_class"])), H(t(I["pred_density"])), H(t(I["target"])), int(L.reduced), H(t(pts)), offs, ordr,
            H(t(I["bins_lo"])), H(t(I["bins_hi"])), B, N, L.size, L.red, L.mode, int(L.norm), *L.w, L.reg, L.max_iter,
            L.stop_thr, L.eval_freq, _lib.ptr(fr["gc"].mid), _lib.ptr(fr["gd"].mid), _lib.ptr(fr["losses"].mid),
            _lib.ptr(fr["stats"].mid), _lib.ptr(fr["beta"].mid) if with_beta else None, _lib.ptr(fr["status"].mid),
            _lib.ptr(fr["ws"].mid), ws_bytes, _lib.stream(fr["gc"].full))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, f in fr.items():
        assert f.ok(), f"{L.name}: a write outside {k}"
    out = {k: f.mid.cpu().numpy() for k, f in fr.items() if k != "ws"}
    out["gc"] = out["gc"].reshape(B, N, g, g)
    out["gd"] = out["gd"].reshape(B, g, g)
    out["status"] = out["status"].reshape(B)
    return out


def _class_bounds(L, b, r):
    """Per cell: D = max - min logit, lse the log-sum-exp.
    lse: each exp(l - max) carries the rounded difference (u D relative) and expf (2 u), the N-term sum N - 1 more, logf
    2 u ln N absolute, the final add u |lse|:  E_lse = (D + N + 1 + 2 ln N + |lse|) u.
    grad_class = (exp(l - lse) - onehot) / B: the exponent carries E_lse and the rounded difference (u (D + ln N)), expf
    2 u, the subtraction, 1/B and the product one each on a value <= 1:  k = 2 D + N + 3 ln N + |lse| + 6, plus 2 for the
    second-order terms, times u / B.
    CE of the crop = block sum of lse - l[label]: the sum of the E_lse, the rounded differences and the block sum
    (1 + 26 on the sum of |terms|), plus 1 for second order."""
    z = LC.inputs(L)["pred_class"][b].astype(np.float64)
    N = z.shape[0]
    D = z.max(0) - z.min(0)
    lse = z.max(0) + np.log(np.exp(z - z.max(0)).sum(0))
    e_lse = (D + N + 1 + 2 * np.log(N) + np.abs(lse)) * U
    k = 2 * D + N + 3 * np.log(N) + np.abs(lse) + 8
    return np.broadcast_to(k * U / L.B, z.shape), float(e_lse.sum() + (BS + 2) * U * np.abs(r["ce_cell"]).sum())


def _dm_terms(L, b, r):
    """Bounds of the DMLoss pieces that involve no Sinkhorn.
    1/(pc + eps): the block sum of pc (26 u on sum |pd|), the add, the division: R_pc = 26 sum|pd| / pc + 2 (in u).
    normed pred = pd * that: R_pc + 1; normed target: add, division, product 3 u; d = their difference, one more.
    TV * n = n * block sum |d|:  n u [(R_pc + 1) sum|np| + 3 sum|nt| + (1 + 26 + 1) sum|d|].
    count = |pc - n|: 26 u sum|pd| + u |pc - n|.
    TV gradient = (n / B) (sgn(d) / pc' - tvk / pc'^2), tvk = block sum of sgn(d) pd, pc' = pc + eps:
      n / B two roundings, sgn / pc' R_pc, tvk 26 u sum|pd| + its two factors 2 R_pc + 2, the subtraction and the product
      one each on the result; a cell excluded for its sign (LC.tv_excluded) may move tvk by 2 |pd| of that cell."""
    pd = LC.inputs(L)["pred_density"][b, 0].astype(np.float64)
    n, pc = r["n"], r["pc"]
    sabs = np.abs(pd).sum()
    pcp = pc + LR.EPS
    r_pc = BS * sabs / abs(pc) + 2
    np_, nt = pd / pcp, r["td"] / (n + LR.EPS)
    e_tv = n * U * ((r_pc + 1) * np.abs(np_).sum() + 3 * np.abs(nt).sum() + (BS + 2) * np.abs(r["d"]).sum())
    e_cnt = U * (BS * sabs + abs(pc - n))
    ex = LC.tv_excluded(L, b, r)
    ktv = n / L.B
    tvk = (np.sign(r["d"]) * pd).sum()
    e_gtv = ktv * (U * (r_pc / abs(pcp) + (BS * sabs + (2 * r_pc + 2) * abs(tvk)) / pcp ** 2)
                   + 2 * np.abs(pd[ex]).sum() / pcp ** 2) + 4 * U * np.abs(r["tv_grad"])
    return e_tv, e_cnt, e_gtv, ex


def _ot_bounds(L, b, r, o):
    """4 delta + floor for the Sinkhorn outputs, delta = the deviation of oracle.ref.ot_crop (f32, dense K) from the
    float64 reference on this crop (max norm for beta and the gradient, absolute for the scalars).
    Floors (the rounding after the iteration, for crops whose delta happens to be tiny):
      beta = reg * logf(v + eps): the add, logf (2 u), the product: 4 u |beta|;
      gradient = g1 beta - g2, g1 = pc / den, g2 = sb / den, den = pc^2 + eps, sb = block sum of pd beta: pc carries
        R = 26 sum|pd| / pc, den 2 R + 2, so g1 3 R + 3 and g1 beta one more; g2: (26 + 1) sum|pd beta| / den + (2 R + 3)
        |g2|; the subtraction one on the result;
      ot = block sum of pd * gradient.  It is 0 in exact arithmetic for ANY beta (sum pd (pc beta - sb) = 0), so beta's
        own error cancels and only the roundings of the gradient formula and of the sum remain: sum |pd| * (gradient
        floor without beta's 4 u) + (26 + 1) u sum |pd gradient|;
      wd = sum P C over the windows: per point row a serial sum of up to g products with one fma each (2 g), the cost
        and factor products (8), the block sum (26), plus the u Ey v products (4) and 2 for second order: (2 g + 40) u
        sum |P C|;
      err = block sum of (b - ktu v)^2: ktu is a sum of n products in some order (n u), v = b / (ktu + eps) and the
        product 4 more, so ktu v carries E = (n + 4) u |b| per cell; err moves by sum (2 |d| E + E^2) with d the
        reference's residual at that check, plus the squares and the block sum (26 + 3) u err."""
    pd = LC.inputs(L)["pred_density"][b, 0].astype(np.float64).reshape(-1)
    pc, n, g = r["pc"], r["n"], L.g
    beta, og = r["beta"], r["ot_grad"].reshape(-1)
    d_beta = np.abs(o["beta"] - beta).max()
    d_grad = np.abs(o["ot_grad"] - og).max()
    d_ot, d_wd = abs(o["loss"] - r["ot"]), abs(o["wd"] - r["wd"])
    sabs = np.abs(pd).sum()
    Rr = BS * sabs / abs(pc)
    den = pc * pc + LR.EPS
    g1, sb = pc / den, (pd * beta).sum()
    f_beta = 4 * U * np.abs(beta)
    f_grad_nb = U * ((3 * Rr + 4) * np.abs(g1 * beta) + ((BS + 1) * np.abs(pd * beta).sum() + (2 * Rr + 3) * abs(sb)) / den
                     + np.abs(og))
    f_grad = f_grad_nb + np.abs(g1) * f_beta
    f_ot = (np.abs(pd) * f_grad_nb).sum() + (BS + 1) * U * r["ot_abs"]
    f_wd = (2 * g + 40) * U * r["wd_abs"]
    out = dict(beta=4 * d_beta + f_beta, grad=4 * d_grad + f_grad, ot=4 * d_ot + f_ot, wd=4 * d_wd + f_wd)
    if len(r["err"]):
        bn = pd / (pc + LR.EPS)
        resid = np.abs(r["resid_last"])
        E = (n + 4) * U * np.abs(bn)
        out["err"] = 4 * abs(float(o["err"][-1]) - r["err_last"]) + float((2 * resid * E + E * E).sum()) + (BS + 3) * U * r["err_last"]
    return out


class _Acc(dict):
    """Collects (out, ref, bound) per quantity over the crops of a launch; one RATIO line per quantity."""

    def add(self, key, out, ref, bound):
        o, r_, b_ = (np.atleast_1d(np.asarray(a, np.float64)).reshape(-1) for a in (out, ref, bound))
        self.setdefault(key, []).append((o, r_, np.broadcast_to(b_, r_.shape)))

    def report(self, prefix):
        fails = []
        for key, items in self.items():
            try:
                _report(f"{prefix}.{key}", *(np.concatenate([it[i] for it in items]) for i in range(3)))
            except AssertionError as e:
                fails.append(e.args[0] if e.args else key)
        assert not fails, fails


@pytest.mark.parametrize("name", LC.names())
def test_launch_matches_float64_reference(name):
    L = LC.BY_NAME[name]
    refs, orc = LC.reference(L), LC.oracle_f32(L)
    I = LC.inputs(L)
    out = _launch(L)
    wc, wot, wtv = (np.float64(np.float32(w)) for w in L.w)
    A = _Acc()
    for b, r in enumerate(refs):
        n = r["n"]
        st = out["stats"][b].astype(np.float64)
        # labels: exactly one negative entry per cell of grad_class, at the reference's label (block sums of an integer
        # dot map are exact; a reduced target is compared as given)
        neg = out["gc"][b] < 0
        assert np.array_equal(neg.sum(0), np.ones((L.g, L.g), np.int64)), (name, b)
        assert np.array_equal(neg.argmax(0), r["labels"]), (name, b)
        kc, e_ce = _class_bounds(L, b, r)
        A.add("grad_class", out["gc"][b], r["grad_class"], kc)
        A.add("ce", st[0], r["ce"], e_ce)
        if L.mode in (LR.MAE, LR.MSE):
            # sum of |d| or d^2, d = pd - td: the difference (and the square) 2 u per term, the block sum 26, 1 for second
            # order: 29 u count.  Gradient sgn(d) or 2 d, times w_count and 1/B (itself rounded): 4 u |value|.
            A.add("count", st[2], r["count"], (BS + 3) * U * r["count"])
            A.add("grad_density", out["gd"][b], r["grad_density"], 4 * U * np.abs(r["grad_density"]))
            assert st[1] == 0 and st[3] == 0 and st[4] == 0 and st[5] == 0 and st[6] == 0 and st[7] == -1
            assert out["status"][b] == 0
            continue
        e_tv, e_cnt, e_gtv, ex = _dm_terms(L, b, r)
        A.add("tv_n", st[1], r["tv_n"], e_tv)
        A.add("count", st[2], r["count"], e_cnt)
        if n == 0:
            assert not out["beta"][b].any(), (name, b, "beta of an empty crop")
            assert tuple(st[3:]) == (0, 0, 0, 0, -1) and out["status"][b] == 0
            ob = dict(grad=np.zeros(L.g * L.g))
        else:
            o = orc[b]
            ob = _ot_bounds(L, b, r, o)
            A.add("beta", out["beta"][b], r["beta"], ob["beta"])
            A.add("ot", st[3], r["ot"], ob["ot"])
            A.add("wd", st[4], r["wd"], ob["wd"])
            if "err" in ob:
                A.add("err_last", st[7], r["err_last"], ob["err"])
            else:
                assert st[7] == -1
            # the control flow is the f32 restatement's exactly (test_loss_refs_cpu.py: every err check is 2x away from
            # stop_thr, and the float64 reference stops where the restatement stops)
            assert (int(st[5]), bool(st[6])) == (o["iters"], o["rolled_back"]) == (r["iters"], r["rolled_back"]), (name, b, st[5:7])
            assert out["status"][b] == (-o["iters"] if o["rolled_back"] else o["iters"])
        # grad_density = w_count (w_ot ot + w_tv tv + count): the three pieces' bounds with their weights, the count
        # gradient sgn(pc - n) / B (1/B rounded: u / B), and the combination's products and adds (4 u on the |pieces|)
        eg = ob["grad"].reshape(L.g, L.g)
        if L.mode == LR.OT_ONLY:
            bound = wc * wot * eg + 3 * U * np.abs(r["grad_density"])
            keep = np.ones((L.g, L.g), bool)
        else:
            pieces = wot * np.abs(r["ot_grad"]) + wtv * np.abs(r["tv_grad"]) + np.abs(r["count_grad"])
            bound = wc * (wot * eg + wtv * e_gtv + U / L.B) + 4 * U * wc * pieces
            keep = ~ex
            assert ex.sum() <= 1e-3 * L.g * L.g
        A.add("grad_density", out["gd"][b][keep], r["grad_density"][keep], bound[keep])
    # losses[5] from the kernel's own crop_stats: a 256-thread block sum of B <= 8 values per term (B + 6 + 4 roundings
    # at most), 1/B and the mean, the weights' products and adds: 24 u on the sum of |terms|
    want = LR.finalize(out["stats"], L.mode, *L.w)
    scale = LR.finalize(np.abs(out["stats"]), L.mode, *L.w)
    A.add("losses", out["losses"].reshape(-1), want, 24 * U * np.abs(scale))
    A.report(name)


@pytest.mark.parametrize("name", ["p32", "b24"])
def test_crops_do_not_depend_on_batch_order_or_metadata_path(name):
    """A crop runs in its own workgroup on fixed-order sums: its crop_stats[:, :6] and gradients are bit-identical with
    the processing order reversed and with the offsets / order in device memory (ebc_dace_loss)."""
    L = LC.BY_NAME[name]
    a = _launch(L)
    for kw in (dict(reverse=True), dict(device_meta=True), dict(reverse=True, device_meta=True)):
        b = _launch(L, **kw)
        assert np.array_equal(a["stats"][:, :6], b["stats"][:, :6]), kw
        assert np.array_equal(a["gc"], b["gc"]) and np.array_equal(a["gd"], b["gd"]) and np.array_equal(a["beta"], b["beta"]), kw
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["losses"], b["losses"]), kw
