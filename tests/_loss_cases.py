"""The launches tests/test_gpu_loss_kernels.py runs, their inputs and references, shared with tests/test_loss_refs_cpu.py
(which asserts each launch's input conditions on the float64 reference alone, so a badly chosen input fails without a
GPU).  Point counts at the LDS capacity boundaries come from ebc_dace_plan (host-only), never from restated LDS
arithmetic."""
import ctypes
import functools
import zlib

import numpy as np

import _loss_refs as LR
from oracle import ref as oracle

BINS = [(0.0, 0.0), (1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (4.0, float("inf"))]
# fractional (reduced) targets: a gap (0.25, 0.5) and (2.5, 3) -> label 0; bin 3 overlaps bin 1 at 1.0 and bin 2 on
# [1.5, 2.0] and wins there (later bins win)
BINS_FRAC = [(0.0, 0.25), (0.5, 1.0), (1.5, 2.5), (1.0, 2.0), (3.0, float("inf"))]
W = (0.5, 0.3, 0.07)                 # (w_count, w_ot, w_tv) off their defaults (1, 0.1, 0.01)
WD = (1.0, 0.1, 0.01)
EXACT = {8: 64, 16: 128, 24: 192, 28: 224, 32: 256, 40: 320, 48: 384, 56: 448, 64: 512}
PADDED = {8: 48, 16: 96, 24: 160, 28: 208, 32: 240, 40: 288, 48: 352, 56: 416, 64: 480}
NEW = (24, 32, 40)                   # the LDS grids no other module launches
U = 2.0 ** -24


def plan(size, red, n):
    """(G, first path, lanes, dense path, lds_cap_s, lds_cap_c, lds_cap) of one crop, from the library."""
    from ebc_amd import _lib
    out = (ctypes.c_int * 6)()
    G = _lib.load().ebc_dace_plan(size, red, n, out)
    return (G, *out)


def path_taken(size, red, n, wide):
    """(path, lanes) a crop of n > 0 points runs: the first path, or the plan's dense path when it is bucketed and
    a window is wider than 9 cells."""
    G, first, lanes, dense, *_ = plan(size, red, n)
    return (dense, 0) if (first <= 1 and wide) else (first, lanes)


def edge_values(bins):
    """Targets on and around every finite bin edge, in the gaps and in the overlaps (f32)."""
    f = np.float32
    vals = []
    for lo, hi in bins:
        for e in (lo, hi):
            if np.isfinite(e):
                e = f(e)
                vals += [e, np.nextafter(e, f(-np.inf)), np.nextafter(e, f(np.inf))]
    vals += [f(0.375), f(2.75), f(1.75), f(7.5), f(0.0)]
    return np.array([v for v in vals if v >= 0], f)


class Launch:
    def __init__(self, name, size, crops, red=8, reduced=False, mode=LR.DMCOUNT, norm=False, w=W, reg=10.0,
                 max_iter=100, stop_thr=1e-9, eval_freq=10, bins=BINS):
        self.name, self.size, self.red, self.reduced, self.mode, self.norm = name, size, red, reduced, mode, norm
        self.w, self.reg, self.max_iter, self.stop_thr, self.eval_freq, self.bins = w, reg, max_iter, stop_thr, eval_freq, bins
        self.crops = [(c, "rand") if isinstance(c, int) else c for c in crops]
        self.g = size // red
        self.B = len(self.crops)
        assert self.B <= 8
        self.counts = [c[0] for c in self.crops]
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)

    def __repr__(self):
        return self.name


def _points(rng, n, kind, size, red):
    f = np.float32
    hi = f(size) - f(2.0 ** -10)
    if kind == "border":                                  # on the crop border: 0 and size - 2^-10 on either axis
        p = (rng.random((n, 2)) * size).astype(f)
        side = rng.integers(0, 4, n)
        p[side == 0, 0] = 0.0; p[side == 1, 0] = hi; p[side == 2, 1] = 0.0; p[side == 3, 1] = hi
        p[:4] = [[0.0, 0.0], [hi, hi], [0.0, hi], [hi, 0.0]][:len(p[:4])]
        return p
    if kind == "dup":                                     # every point at least twice
        base = (rng.random(((n + 2) // 3, 2)) * size).astype(f)
        return base[np.arange(n) % len(base)]
    if kind == "onecell":                                 # all in one cell
        c = rng.integers(0, size // red, 2)
        return ((c + rng.random((n, 2))) * red).astype(f)
    if kind == "lastrow":                                 # the last live row / column, next to the dead cells
        p = (rng.random((n, 2)) * size).astype(f)
        last = (size - red + rng.random(n) * red).astype(f)
        half = np.arange(n) % 2 == 0
        p[half, 1] = np.minimum(last[half], hi); p[~half, 0] = np.minimum(last[~half], hi)
        return p
    return np.minimum((rng.random((n, 2)) * size).astype(f), hi)


def dot_map(points, size):
    """Integer dot map: +1 at each point's truncated pixel (duplicates add up)."""
    m = np.zeros((size, size), np.float32)
    if len(points):
        p = np.clip(points.astype(np.int64), 0, size - 1)
        np.add.at(m, (p[:, 1], p[:, 0]), 1.0)
    return m


@functools.lru_cache(maxsize=None)
def _inputs(name):
    L = BY_NAME[name]
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))
    g, N = L.g, len(L.bins)
    pts = [_points(rng, n, kind, L.size, L.red) for n, kind in L.crops]
    pcl = (rng.standard_normal((L.B, N, g, g)) * 1.5).astype(np.float32)
    pde = (0.05 + rng.random((L.B, 1, g, g)) * 1.95).astype(np.float32)     # continuous: no TV sign ties
    for b, (n, kind) in enumerate(L.crops):
        if kind == "sparse":                              # zero on all but a few cells
            keep = rng.choice(g * g, min(5, g * g), replace=False)
            z = np.zeros(g * g, np.float32); z[keep] = pde[b].reshape(-1)[keep]
            pde[b] = z.reshape(1, g, g)
    if L.reduced:
        ev = edge_values(L.bins)
        tgt = np.zeros((L.B, 1, g, g), np.float32)
        for b in range(L.B):
            t = ev[(np.arange(g * g) + 7 * b) % len(ev)].copy()
            rnd = rng.random(g * g) < 0.3
            t[rnd] = (rng.random(int(rnd.sum())) * 4).astype(np.float32)
            tgt[b, 0] = t.reshape(g, g)
    else:
        tgt = np.stack([dot_map(p, L.size)[None] for p in pts])
    lo = np.array([b[0] for b in L.bins], np.float32)
    hi = np.array([b[1] for b in L.bins], np.float32)
    return dict(pred_class=pcl, pred_density=pde, target=tgt, points=pts, bins_lo=lo, bins_hi=hi)


def inputs(L):
    return _inputs(L.name)


def crop_ref(L, b, with_ot=True):
    """The float64 reference of crop b (with_ot=False: no Sinkhorn, for the cheap input-condition checks)."""
    I = inputs(L)
    pts = I["points"][b] if with_ot else I["points"][b][:0]
    r = LR.crop(I["pred_class"][b], I["pred_density"][b, 0], I["target"][b, 0], pts, I["bins_lo"], I["bins_hi"],
                L.size, L.red, L.B, L.mode, L.norm, *L.w, L.reg, L.max_iter, L.stop_thr, L.eval_freq)
    return r


@functools.lru_cache(maxsize=None)
def _reference(name):
    L = BY_NAME[name]
    return [crop_ref(L, b) for b in range(L.B)]


def reference(L):
    return _reference(L.name)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """oracle.ref.ot_crop (the f32 C restatement, dense K) per crop with points; None elsewhere."""
    L = BY_NAME[name]
    I = inputs(L)
    out = []
    for b, n in enumerate(L.counts):
        if n == 0 or L.mode in (LR.MAE, LR.MSE):
            out.append(None)
            continue
        out.append(oracle.ot_crop(I["points"][b], I["pred_density"][b, 0], L.size, L.red, L.reg, L.max_iter, L.stop_thr,
                                  L.eval_freq, L.norm))
    return out


def oracle_f32(L):
    return _oracle(L.name)


def wide(L, b, slack):
    """Whether crop b has a factor window wider than 9 cells (slack > 0: it may have; slack < 0: it surely has)."""
    p = inputs(L)["points"][b]
    if len(p) == 0:
        return False
    ny, nx = LR.windows(p, L.size, L.red, L.reg, L.norm, slack)
    return bool(max(ny.max(), nx.max()) > 9)


def tv_excluded(L, b, r=None):
    """Cells whose TV sign argument d = pd/pc - td/tc is smaller than the f32 rounding of its two terms, so the kernel's
    sign may differ (flagged at twice that rounding): pc is a 1024-thread block sum (<= 26 roundings), 1/(pc + eps) two more, the product one
    (29u |pd/pc|); 1/(tc + eps) two and the product one (3u |td/tc|); the subtraction rounds d itself."""
    r = r or crop_ref(L, b, with_ot=False)
    I = inputs(L)
    pd = I["pred_density"][b, 0].astype(np.float64)
    n = L.counts[b]
    tau = U * (29.0 * np.abs(pd / (r["pc"] + LR.EPS)) + 3.0 * np.abs(r["td"] / (n + LR.EPS)))
    return np.abs(r["d"]) < 2.0 * tau


def _with_odd_offset(crops, heavy):
    """Append crop `heavy` so that its first point sits at an odd offset (a 1-point crop goes in front if needed)."""
    total = sum(c if isinstance(c, int) else c[0] for c in crops)
    return crops + ([heavy] if total % 2 else [1, heavy])


def _build():
    Ls = []
    for G, size in EXACT.items():
        _, _, _, _, cap_s, cap_c, cap = plan(size, 8, 1)
        if G in NEW:
            Ls.append(Launch(f"x{G}", size, [0, 1, 2, 17]))
            # the full boundary set: full-row and compact-row capacities, the 256 / 257 lane switch where 16 lanes exist
            lanes = [256, 257] if plan(size, 8, 257)[2] == 16 else []
            Ls.append(Launch(f"b{G}", size, _with_odd_offset([cap_s, cap_s + 1, cap_c] + lanes, cap_c + 1)))
            # reg = 20: windows wider than 9 cells, so the bucketed path refuses the crop: dense in LDS up to lds_cap
            Ls.append(Launch(f"w{G}", size, _with_odd_offset([5, cap], cap + 1), reg=20.0))
        else:
            crops = [0, 1, 2, 17] + ([257] if plan(size, 8, 257)[1:3] == (0, 16) else [])
            crops += [cap_s + 1] if cap_c > cap_s else []
            Ls.append(Launch(f"x{G}", size, _with_odd_offset(crops, cap_c + 1), w=WD if G == 28 else W))
            if G > 8:                                     # (g <= 9: no window can be wider than 9 cells)
                Ls.append(Launch(f"w{G}", size, [33, 2], reg=20.0))
    edges = [(12, "border"), (20, "dup"), (9, "onecell"), (15, "lastrow")]
    for G, size in PADDED.items():
        kw = {24: dict(reg=5.0), 32: dict(max_iter=25), 40: dict(eval_freq=1)}.get(G, {})
        Ls.append(Launch(f"p{G}", size, [0, 1, 2, 17] + (edges if size >= 96 else [(12, "border"), (20, "dup")]), **kw))
    # g = 1: with a dot map, normed pred and normed target are both 1 up to rounding whenever the crop has points, so
    # the TV sign is undefined there: the DMCount launch keeps the empty crops, the crops with points run OT alone
    # (no TV gradient) and DMCount on a reduced target that differs from the point count
    Ls.append(Launch("g1", 8, [0, 0]))
    Ls.append(Launch("g1ot", 8, [1, 2, 17], mode=LR.OT_ONLY))
    Ls.append(Launch("g1red", 8, [1, 2, 17], reduced=True, bins=BINS_FRAC))
    # (19 points, not 17: on 3 x 3 cells the iteration converges, and with 17 the err of a check lands within 2x of
    # stop_thr; with 19 it stops at iteration 70 with the checks at 4.9e-9 and 3.8e-10)
    Ls.append(Launch("g3", 24, [0, 1, 2, 19, (6, "border")]))
    Ls.append(Launch("sparse32", 240, [(17, "sparse"), (60, "sparse"), (300, "sparse")]))
    Ls.append(Launch("sparse40", 288, [(2, "sparse"), (40, "sparse")], w=WD))
    Ls.append(Launch("norm32", 240, _with_odd_offset([3, 17, 60], plan(240, 8, 1)[6] + 1), norm=True))
    for mode, nm in ((LR.MAE, "mae"), (LR.MSE, "mse"), (LR.OT_ONLY, "ot")):
        Ls.append(Launch(f"{nm}40", 288, [0, 2, 17, (40, "dup")], mode=mode))
    Ls.append(Launch("iter1_24", 192, [1, 17, 300], max_iter=1))
    Ls.append(Launch("iter0_32", 240, [1, 17], max_iter=0))
    Ls.append(Launch("stop40", 320, [17, 50, plan(320, 8, 1)[4] + 40], stop_thr=STOP40))
    Ls.append(Launch("red40", 640, [0, 5, 37, 120], red=16, reduced=True, bins=BINS_FRAC))
    Ls.append(Launch("red24", 768, [3, 17, 64], red=32, reduced=True, bins=BINS_FRAC))
    Ls.append(Launch("pitch24", 320, [0, 1, 17, 90], red=16))
    Ls.append(Launch("pitch32", 512, [2, 17, 130], red=16))
    return Ls


# stop40: a loose threshold that stops every crop at its first check (iteration 10).  The float64 reference's err there
# is 1.4e-4 ... 2.9e-3 over the three crops (test_loss_refs_cpu.py asserts each is below STOP40 / 2).
STOP40 = 1e-2
LAUNCHES = []
BY_NAME = {}


def launches():
    if not LAUNCHES:
        LAUNCHES.extend(_build())
        BY_NAME.update({L.name: L for L in LAUNCHES})
        assert len(BY_NAME) == len(LAUNCHES)
    return LAUNCHES


def names():
    return [L.name for L in launches()]
