"""Float64 restatement of one step of csrc/optim.hip (adam_kernel / amp_check_kernel) for one tensor, its per-element
error bounds, the scaler update as a pure function, and an f32 numpy stand-in of the kernels that can be corrupted.

The step is torch.optim.Adam's (L2 weight decay, bias corrections of step + 1) under torch.amp.GradScaler:

    g'  = g / scale                                   (the unscaled gradient; stored when write_unscaled_grad)
    gr  = g' + wd * p                                 (rounded to f32 in the kernel, not stored)
    m'  = beta1 * m + (1 - beta1) * gr
    v'  = beta2 * v + (1 - beta2) * gr^2
    bc1 = 1 - beta1^(step + 1),  bc2_sqrt = sqrt(1 - beta2^(step + 1)),  step_size = lr / bc1
    p'  = p - step_size * m' / (sqrt(v') / bc2_sqrt + eps)

tests/test_optim_refs_cpu.py pins `adam_f64` to torch.optim.Adam on float64 tensors and `scaler_next` to
torch.amp.GradScaler; tests/test_gpu_optim_kernels.py holds the kernels to `step_ratios`.

Bounds, counted from the rounding points of adam_elem (U = 2^-24 is half an f32 ulp, relative; D = 2^-53 the same of a
double; hulp(x, e) is half the f32 spacing at |x| + e, the largest value the kernel can have rounded when the reference
is x and the error before the rounding is e).  Each stage is checked from the operands the kernel itself stored, so no
stage inherits the error of the one before it:

  g'   from the stored g and scale: the double quotient (D |g'|) rounded to f32: hulp; 0 where the quotient is an f32
       (a power-of-two scale: checked bit for bit).  With write_unscaled_grad = 0 nothing is stored and e_g = that bound
       is carried into gr; otherwise gr starts from the stored g' and e_g = 0.
  gr   (wd != 0): the double product and sum (D (|wd p| + |gr|)) and its f32 rounding: e_gr = e_g + D (..) + hulp(gr).
       wd == 0 is a separate branch without the rounding: e_gr = e_g.
  m'   e_gr scaled by (1 - beta1); the double products and the sum: D (|beta1 m| + 2 |(1 - beta1) gr| + |m'|) (1 - beta1
       is itself a rounded double); the f32 rounding of the stored value: hulp(m').
  v'   e_gr enters as (1 - beta2) (2 |gr| e_gr + e_gr^2); D (|beta2 v| + 3 |(1 - beta2) gr^2| + |v'|); hulp(v').
  p'   from the stored m', v': bc1 and bc2_sqrt are rounded to f32 (U each), step_size = lr / bc1 once more (2 U on
       step_size); sqrtf (U), the division by bc2_sqrt (U) on the first term of the denominator, the f32 rounding of the
       denominator (U; the double sum before it D): 4 U on the denominator; the product step_size * m' (U) and the
       division (U): x = step_size m' / denom carries 8 U (1 + 16 U) |x| (second-order terms included), and the
       subtraction rounds once: hulp(p').  pow() and sqrt() in double are taken at 2 D.
"""
import numpy as np
import torch

import _bn_refs as R

U = R.U32
D = 2.0 ** -53
CHUNK = 4096
F32 = np.float32
F64 = np.float64


def ulp32(x):
    return R.ulp(torch.from_numpy(np.ascontiguousarray(np.asarray(x, F64))), torch.float32).numpy()


def hulp(x, e=0.0):
    return 0.5 * ulp32(np.abs(np.asarray(x, F64)) + e)


def is_pow2(s):
    m, _ = np.frexp(float(s))
    return m == 0.5


class Hyper:
    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, growth=2.0, backoff=0.5, interval=2000):
        self.lr, self.beta1, self.beta2, self.eps, self.wd = lr, beta1, beta2, eps, wd
        self.growth, self.backoff, self.interval = growth, backoff, interval


# ------------------------------------------------------------------------------------------------ the float64 step
def adam_f64(p, g, m, v, step, h, scale=None):
    """One whole step in float64 from (p, g, m, v) and the step count before it; every stage returned."""
    p, g, m, v = (np.asarray(a, F64) for a in (p, g, m, v))
    g1 = g / F64(scale) if scale is not None else g
    gr = g1 + h.wd * p if h.wd != 0.0 else g1
    m1 = h.beta1 * m + (1.0 - h.beta1) * gr
    v1 = h.beta2 * v + (1.0 - h.beta2) * gr * gr
    p1 = param_f64(p, m1, v1, step, h)
    return dict(g1=g1, gr=gr, m1=m1, v1=v1, p1=p1)


def bias_corrections(step, h):
    sd = float(step) + 1.0
    bc1 = 1.0 - h.beta1 ** sd
    bc2_sqrt = np.sqrt(1.0 - h.beta2 ** sd)
    return bc1, bc2_sqrt, h.lr / bc1


def param_f64(p, m1, v1, step, h):
    _, bc2_sqrt, step_size = bias_corrections(step, h)
    return np.asarray(p, F64) - step_size * np.asarray(m1, F64) / (np.sqrt(np.asarray(v1, F64)) / bc2_sqrt + h.eps)


def step_ratios(before, after, step, h, scale=None, write_grad=1):
    """(error, bound) per output kind of one applied step of one tensor: `before` / `after` are the f32 arrays
    (p, g, m, v) the kernel read / left.  g' is checked from the stored g, m' and v' from the stored g' (from g / scale
    with its bound carried where nothing is stored), p' from the stored m' and v'."""
    p0, g0, m0, v0 = (np.asarray(a, F64) for a in before)
    p1, g1, m1, v1 = (np.asarray(a, F64) for a in after)
    out = {}
    if scale is None:
        gs, e_g = g0, np.zeros_like(g0)
    else:
        gq = g0 / F64(scale)
        b_g = D * np.abs(gq) + hulp(gq, D * np.abs(gq))
        b_g = np.where(gq.astype(F32).astype(F64) == gq, 0.0, b_g)       # an exact quotient (a power-of-two scale)
        if write_grad:
            out["g"] = (np.abs(g1 - gq), b_g)
            gs, e_g = g1, np.zeros_like(g0)
        else:
            gs, e_g = gq, b_g
    if h.wd != 0.0:
        gr = gs + h.wd * p0
        e_gr = e_g + D * (np.abs(h.wd * p0) + np.abs(gr))
        e_gr = e_gr + hulp(gr, e_gr)
    else:
        gr, e_gr = gs, e_g
    a1, a2 = 1.0 - h.beta1, 1.0 - h.beta2
    mr = h.beta1 * m0 + a1 * gr
    e_m = a1 * e_gr + D * (np.abs(h.beta1 * m0) + 2 * np.abs(a1 * gr) + np.abs(mr))
    out["m"] = (np.abs(m1 - mr), e_m + hulp(mr, e_m))
    vr = h.beta2 * v0 + a2 * gr * gr
    e_v = a2 * (2 * np.abs(gr) * e_gr + e_gr * e_gr) + D * (np.abs(h.beta2 * v0) + 3 * np.abs(a2 * gr * gr) + np.abs(vr))
    out["v"] = (np.abs(v1 - vr), e_v + hulp(vr, e_v))
    pr = param_f64(p0, m1, v1, step, h)
    x = np.abs(p0 - pr)
    e_x = x * (8 * U * (1 + 16 * U) + 8 * D)
    out["p"] = (np.abs(p1 - pr), e_x + hulp(pr, e_x))
    return out


def ratio(err, bound):
    """Largest err / bound; an error of 0 passes a bound of 0 (lr = 0: the update is exactly nothing)."""
    err, bound = np.asarray(err, F64).reshape(-1), np.asarray(bound, F64).reshape(-1)
    if not np.isfinite(err).all():
        return float("inf")
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ the scaler
def scaler_next(scale, tracker, found, step, h):
    """torch._amp_update_scale_ and the optimizer's step count after one call: (scale', tracker', found' = 0, step').
    The scale is an f32, the factors are doubles, the product is rounded to f32 once."""
    scale, tracker, step = F32(scale), F32(tracker), F32(step)
    if found:
        return F32(F64(scale) * h.backoff), F32(0), F32(0), step
    succ = tracker + F32(1)
    if succ == F32(h.interval):
        with np.errstate(over="ignore"):
            grown = F32(F64(scale) * h.growth)
        return (grown if np.isfinite(grown) else scale), F32(0), F32(0), step + F32(1)
    return scale, succ, F32(0), step + F32(1)


# ------------------------------------------------------------------------------------------------ case lists
SIZES = [1, 3, 4, 5, 1023, 4095, 4096, 4097, 5123, 8199]
LAYOUTS = ["aligned", "grad+1", "param+1"]           # which operand starts one element past a 16-byte boundary
BAD = [float("inf"), float("-inf"), float("nan")]


def check_positions(n, aligned):
    """The elements at which the inf check is given its one non-finite value: the first and last element of the tensor
    and of each chunk, the last element of the float4 part and the first of the scalar remainder of the partial chunk,
    an element of its float4 loop's second pass, and in a whole chunk one element owned by each of waves 0..3 (piece q
    of thread 64 w, q = w)."""
    pos = {0, n - 1}
    for c0 in range(0, n, CHUNK):
        cn = min(CHUNK, n - c0)
        pos |= {c0, c0 + cn - 1}
        if cn == CHUNK:
            for w in range(4):
                pos.add(c0 + 4 * (64 * w + 256 * w) + (w + 1) % 4)
        else:
            n4 = cn & ~3
            if n4:
                pos.add(c0 + n4 - 1)
            if n4 < cn:
                pos.add(c0 + n4)
            if cn > 1024:
                pos.add(c0 + 1024 + 1)
    return sorted(pos)


# ------------------------------------------------------------------------------------------------ f32 stand-in
def check_standin(g_ext, lo, n, aligned, bug=None):
    """amp_check_kernel's traversal of g = g_ext[lo : lo + n] (g_ext holds what lies around it): True when a wave that
    read a non-finite value writes the flag.  bug: "skip_remainder", "drop_piece3", "wave0_only", "n4_up"."""
    hit = False
    for c0 in range(0, n, CHUNK):
        cn = min(CHUNK, n - c0)
        if aligned and cn == CHUNK:                       # (element of the chunk, thread) of every read
            idx = np.arange(1024 * (3 if bug == "drop_piece3" else 4))
            thr = (idx // 4) % 256
        elif aligned:
            n4 = (cn + 3) & ~3 if bug == "n4_up" else cn & ~3
            idx = np.arange(n4)
            thr = (idx // 4) % 256
            if bug != "skip_remainder" and n4 < cn:
                rem = np.arange(n4, cn)
                idx, thr = np.concatenate([idx, rem]), np.concatenate([thr, (rem - n4) % 256])
        else:
            idx = np.arange(cn)
            thr = idx % 256
        bad = ~np.isfinite(g_ext[lo + c0 + idx])
        if bug == "wave0_only":
            bad &= thr < 64
        hit |= bool(bad.any())
    return hit


def step_standin(p, g, m, v, step, h, scale=None, write_grad=1, bug=None):
    """adam_elem in f32 / double numpy, operation for operation.  bug: "bc_step", "wd_after_m", "eps_in_sqrt",
    "write_grad_always"."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    gr = g
    g_out = g
    if scale is not None:
        gr = (g.astype(F64) / F64(F32(scale))).astype(F32)
        if write_grad or bug == "write_grad_always":
            g_out = gr
    g_plain = gr
    if h.wd != 0.0:
        gr = (gr.astype(F64) + p.astype(F64) * h.wd).astype(F32)
    gm = g_plain if bug == "wd_after_m" else gr
    m1 = (h.beta1 * m.astype(F64) + (1.0 - h.beta1) * gm.astype(F64)).astype(F32)
    v1 = (h.beta2 * v.astype(F64) + (1.0 - h.beta2) * gr.astype(F64) * gr.astype(F64)).astype(F32)
    sd = float(F32(step)) + (0.0 if bug == "bc_step" else 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1 = F32(1.0 - h.beta1 ** sd)
        bc2_sqrt = F32(np.sqrt(1.0 - h.beta2 ** sd))
        step_size = F32(h.lr / F64(bc1))
        if bug == "eps_in_sqrt":
            denom = (np.sqrt((v1.astype(F64) + h.eps)).astype(F32) / bc2_sqrt).astype(F32)
        else:
            denom = ((np.sqrt(v1) / bc2_sqrt).astype(F64) + h.eps).astype(F32)
        p1 = (p - (step_size * m1) / denom).astype(F32)
    return p1, g_out, m1, v1


def scaler_standin(scale, tracker, found, step, h, bug=None):
    """The thread-0 block of adam_kernel.  bug: "step_on_skip", "no_reset_on_refused"."""
    scale, tracker, step = F32(scale), F32(tracker), F32(step)
    ns, nt = scale, tracker
    if found:
        ns, nt = F32(F64(scale) * h.backoff), F32(0)
    else:
        succ = tracker + F32(1)
        if succ == F32(h.interval):
            with np.errstate(over="ignore"):
                grown = F32(F64(scale) * h.growth)
            if np.isfinite(grown):
                ns, nt = grown, F32(0)
            else:
                nt = succ if bug == "no_reset_on_refused" else F32(0)
        else:
            nt = succ
    nstep = step if (found and bug != "step_on_skip") else step + F32(1)
    return ns, nt, F32(0), nstep


# ------------------------------------------------------------------------------------------------ inputs
HYPERS = {
    "default_wd": Hyper(wd=1e-4),
    "wd0": Hyper(wd=0.0),
    "betas": Hyper(beta1=0.8, beta2=0.95, eps=1e-6, wd=1e-4),
    "lr0": Hyper(lr=0.0, wd=1e-4),
}
MODES = {                                            # name -> (scale or None, write_unscaled_grad)
    "noscaler": (None, 1),
    "s65536": (65536.0, 1),
    "s3": (3.0, 1),
    "nowrite": (65536.0, 0),
    "nowrite3": (3.0, 0),
}
STEPS0 = [0.0, 1.0, 99999.0]


def tensor_inputs(n, seed):
    """(p, m, v) of one tensor: parameters of order 1, non-zero moments (v >= 0)."""
    g = np.random.Generator(np.random.PCG64(seed))
    p = g.standard_normal(n).astype(F32)
    m = (0.01 * g.standard_normal(n)).astype(F32)
    v = (1e-4 * g.random(n) + 1e-7).astype(F32)
    return p, m, v


def grad_inputs(n, seed, scale):
    """A scaled gradient: true gradients of order 1e-2 times the scale, rounded to f32."""
    g = np.random.Generator(np.random.PCG64(seed))
    return (0.01 * g.standard_normal(n) * (1.0 if scale is None else float(scale))).astype(F32)


def clean_edge_grad(n, seed):
    """A finite gradient holding FLT_MAX, -FLT_MAX, a denormal and -0.0 (the no-false-positive cases)."""
    g = np.random.Generator(np.random.PCG64(seed)).standard_normal(n).astype(F32)
    edge = [np.finfo(F32).max, -np.finfo(F32).max, F32(1e-41), F32(-0.0)]
    for i, e in enumerate(edge):
        g[(n - 1 - i * max(1, n // 5)) % n] = e
    g[n - 1] = np.finfo(F32).max
    g[0] = -np.finfo(F32).max
    return g
