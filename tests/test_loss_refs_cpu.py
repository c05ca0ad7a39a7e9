"""tests/_loss_refs.py (the float64 reference of the fused DACE / DMCount loss) pinned without a GPU: against the
reference project's recorded outputs, torch float64 autograd and the f32 C restatement; then the input conditions of
every launch of tests/test_gpu_loss_kernels.py, asserted on the reference alone, and the coverage of the launch list
against ebc_dace_plan."""
import numpy as np
import pytest
import torch

import _loss_cases as LC
import _loss_refs as LR
from conftest import golden
from ebc_amd import synthetic as syn
from oracle import ref as oracle

F64 = np.float64


# ------------------------------------------------------------------------- the reference project's recorded outputs
def _fixture(name, prefix=""):
    d = golden(name)
    k = lambda s: d[prefix + s]
    size = int(k("size"))
    red = int(k("red")) if prefix else (int(d["reduction"]) if "reduction" in d.files else 8)
    norm = bool(int(k("norm"))) if prefix else False
    offs, pts = k("offsets"), k("points")
    points = [pts[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    return d, k, size, red, norm, points


FIXTURES = [("f1_loss_224.npz", ""), ("f1_loss_448.npz", ""), ("f1g_loss_224_r16.npz", ""), ("f1g_loss_224_r32.npz", ""),
            ("f1g_loss_448_r16.npz", ""), ("f1g_loss_448_r32.npz", ""), ("f1g_loss_384_r8.npz", ""),
            ("f1g_loss_512_r8.npz", ""), ("f1c_loss_extra.npz", "r16_"), ("f1c_loss_extra.npz", "norm_")]


@pytest.mark.parametrize("name,prefix", FIXTURES)
def test_reference_matches_recorded_outputs(name, prefix):
    """The recorded values are the reference project's own f32 run (its Sinkhorn in f32, up to 100 iterations), so
    the f64 restatement agrees with them to f32 accuracy, not to its own: 1e-6 of the largest value where no Sinkhorn
    is involved (CE gradient), 1e-4 where it is (the bounds tests/test_gpu_loss.py holds the kernel to)."""
    d, k, size, red, norm, points = _fixture(name, prefix)
    pcl, pde = k("pred_class"), k("pred_density")
    B = len(points)
    lo = np.array([b[0] for b in LC.BINS], np.float32); hi = np.array([b[1] for b in LC.BINS], np.float32)
    crops = [LR.crop(pcl[b], pde[b, 0], syn.point_map(points[b], size, size), points[b], lo, hi, size, red, B, norm=norm)
             for b in range(B)]
    stats = [[c["ce"], c["tv_n"], c["count"], c["ot"]] for c in crops]
    losses = LR.finalize(stats, LR.DMCOUNT, 1.0, 0.1, 0.01)
    for i, key in ((0, "loss"), (2, "tv_loss"), (3, "count_loss"), (4, "ce_loss")):
        want = float(k("info_" + key))
        assert abs(losses[i] - want) <= 2e-5 * abs(want), (key, losses[i], want)
    assert abs(float(k("info_ot_loss"))) < 1e-3 and abs(losses[1]) < 1e-9      # sum(pd * grad) is 0 in exact arithmetic
    gc = np.stack([c["grad_class"] for c in crops])
    gd = np.stack([c["grad_density"] for c in crops])[:, None]
    assert np.abs(gc - k("grad_pred_class")).max() <= 1e-6 * np.abs(k("grad_pred_class")).max()
    assert np.abs(gd - k("grad_pred_density")).max() <= 1e-4 * np.abs(k("grad_pred_density")).max()
    beta = np.stack([c["beta"] for c in crops])
    # beta follows the cost: the recorded run forms C = (-2 p c + p p) + c c in f32, three roundings of values up to
    # 2 size^2 (1 when norm_cood), and so do the potentials it is a difference of
    scale = 1.0 if norm else float(size)
    assert np.abs(beta - k("beta")).max() <= 1e-4 * np.abs(k("beta")).max() + 2 * 3 * 2.0 ** -23 * scale * scale
    if not prefix:
        for b, c in enumerate(crops):
            if c["n"] == 0:
                continue
            assert abs(c["wd"] - float(d["wd"][b])) <= 1e-4 * abs(float(d["wd"][b])) + 1e-6, (b, c["wd"], d["wd"][b])
            rec = d["err"][b][:len(c["err"])]
            assert len(c["err"]) == c["iters"] // 10
            # the recorded err is an f32 sum of squares of f32 residuals: it floors near 1e-14, the f64 one does not
            big = rec > 1e-9
            assert np.all(np.abs(c["err"][big] - rec[big]) <= 1e-2 * rec[big]), (b, c["err"], rec)
            assert np.all(c["err"][~big] <= 2e-9)


# ------------------------------------------------------------------------------------------- torch float64 autograd
@pytest.mark.parametrize("mode", [LR.DMCOUNT, LR.MAE, LR.MSE, LR.OT_ONLY])
@pytest.mark.parametrize("size,red,n", [(48, 8, 7), (40, 8, 0), (64, 16, 3)])
def test_reference_gradients_match_autograd(mode, size, red, n):
    """CE, TV, count, mae / mse as torch float64 expressions, differentiated by autograd; the OT term goes in through a
    detached gradient, as oracle.ref._OTGrad does (dm_loss.py:76)."""
    rng = np.random.Generator(np.random.PCG64(size + n))
    g, N, B = size // red, 5, 3
    pcl = rng.standard_normal((N, g, g)).astype(np.float32)
    pde = (0.05 + rng.random((g, g)) * 2).astype(np.float32)
    pts = (rng.random((n, 2)) * size).astype(np.float32)
    dm = LC.dot_map(pts, size)
    lo = np.array([b[0] for b in LC.BINS], np.float32); hi = np.array([b[1] for b in LC.BINS], np.float32)
    wc, wot, wtv = 0.5, 0.3, 0.07
    r = LR.crop(pcl, pde, dm, pts, lo, hi, size, red, B, mode, False, wc, wot, wtv, reg=7.0, max_iter=30)
    wc, wot, wtv = (float(np.float32(w)) for w in (wc, wot, wtv))
    pc = torch.tensor(pcl, dtype=torch.float64, requires_grad=True)
    pd = torch.tensor(pde, dtype=torch.float64, requires_grad=True)
    td = oracle.reshape_density(torch.tensor(dm, dtype=torch.float64)[None, None], red)[0, 0]
    assert np.array_equal(td.numpy(), r["td"])
    cls = oracle.bin_count(td[None, None], LC.BINS)[0]
    assert np.array_equal(cls.numpy(), r["labels"])
    ce = torch.nn.functional.cross_entropy(pc[None], cls[None], reduction="none").sum()
    ot = oracle._OTGrad.apply(pd, torch.tensor(r["ot_grad"]))
    if mode in (LR.MAE, LR.MSE):
        cnt = ((pd - td).abs() if mode == LR.MAE else (pd - td) ** 2).sum()
        loss = (ce + wc * cnt) / B
    else:
        cntp = pd.sum()
        tv = (pd / (cntp + 1e-8) - td / (n + 1e-8)).abs().sum() * n
        cnt = (cntp - n).abs()
        loss = (ce + wc * (ot.sum() * wot * B + tv * wtv + cnt)) / B if mode == LR.DMCOUNT else ce / B + wc * wot * ot.sum()
        assert abs(float(tv.detach()) - r["tv_n"]) <= 1e-12 * max(1.0, abs(r["tv_n"]))
    loss.backward()
    assert abs(float(ce) - r["ce"]) <= 1e-12 * abs(r["ce"])
    assert abs(float(cnt) - r["count"]) <= 1e-12 * max(1.0, abs(r["count"]))
    assert np.abs(pc.grad.numpy() - r["grad_class"]).max() <= 1e-14
    gd = pd.grad.numpy()
    assert np.abs(gd - r["grad_density"]).max() <= 1e-12 * max(1e-3, np.abs(r["grad_density"]).max())


# ------------------------------------------------------------------------ the f32 C restatement, non-default settings
@pytest.mark.parametrize("kw", [dict(reg=5.0), dict(reg=20.0), dict(max_iter=25), dict(eval_freq=1, max_iter=12),
                                dict(max_iter=1), dict(max_iter=0), dict(stop_thr=1e-4), dict(eval_freq=7, max_iter=40),
                                dict(norm=True)])
def test_reference_matches_f32_restatement(kw):
    """Same control flow: the iteration count, the number of err checks and the roll-back flag are equal; the values
    agree to f32 accuracy of a short iteration (1e-4 of the largest beta; err to 1 %)."""
    rng = np.random.Generator(np.random.PCG64(11))
    size, red = 96, 8
    pts = (rng.random((23, 2)) * size).astype(np.float32)
    pde = (0.05 + rng.random((12, 12)) * 2).astype(np.float32)
    a = dict(reg=10.0, max_iter=100, stop_thr=1e-9, eval_freq=10, norm=False); a.update(kw)
    r = LR.ot_crop(pts, pde, size, red, a["reg"], a["max_iter"], a["stop_thr"], a["eval_freq"], a["norm"])
    o = oracle.ot_crop(pts, pde, size, red, a["reg"], a["max_iter"], a["stop_thr"], a["eval_freq"], a["norm"])
    assert r["iters"] == o["iters"] and r["rolled_back"] == o["rolled_back"] and len(r["err"]) == len(o["err"])
    for e64, e32 in zip(r["err"], o["err"]):
        assert not (0.5 < e64 / a["stop_thr"] < 2.0), "err too close to stop_thr for the f32 run to agree: pick another case"
        assert abs(e64 - e32) <= 1e-2 * e64 + 1e-12
    assert np.abs(r["beta"] - o["beta"]).max() <= 1e-4 * np.abs(r["beta"]).max()
    # (the gradient is a difference of betas over the count: all but zero when no iteration ran)
    assert np.abs(r["ot_grad"] - o["ot_grad"]).max() <= 1e-4 * np.abs(r["ot_grad"]).max() + 1e-6 * np.abs(r["beta"]).max() / pde.sum()
    assert abs(r["wd"] - o["wd"]) <= 1e-4 * abs(r["wd"])


def test_nonfinite_iterate_rolls_back_and_stops():
    """A negative mass makes K v + 1e-16 cross zero on the way: the iterate turns non-finite, the previous (u, v)
    is kept and the loop stops, as bregman_pytorch.py:111-115."""
    C = np.array([[0.0, 1.0], [1.0, 0.0]])
    b = np.array([np.inf, 1.0])
    s = LR.sinkhorn(np.array([0.5, 0.5]), b, C, 1.0, 10, 1e-9, 10)
    assert s["rolled_back"] and s["iters"] == 1
    assert np.array_equal(s["u"], [0.5, 0.5]) and np.array_equal(s["v"], [0.5, 0.5])


# ----------------------------------------------------------------------------------------------------------- bin edges
def test_bin_labels_on_the_edges():
    f = np.float32
    lo = np.array([b[0] for b in LC.BINS_FRAC], f); hi = np.array([b[1] for b in LC.BINS_FRAC], f)
    below, above = (lambda x: np.nextafter(f(x), f(-np.inf))), (lambda x: np.nextafter(f(x), f(np.inf)))
    cases = [(f(0.0), 0), (f(0.25), 0), (above(0.25), 0), (f(0.375), 0),        # the gap labels 0 as bin 0 does
             (below(0.5), 0), (f(0.5), 1), (above(0.5), 1), (below(1.0), 1),
             (f(1.0), 3),                                                       # bins 1 and 3 overlap: the later wins
             (above(1.0), 3), (below(1.5), 3), (f(1.5), 3), (f(1.75), 3), (f(2.0), 3),
             (above(2.0), 2), (f(2.5), 2), (above(2.5), 0), (f(2.75), 0),       # gap -> 0
             (below(3.0), 0), (f(3.0), 4), (above(3.0), 4), (f(7.5), 4), (f(1e30), 4)]
    vals = np.array([c[0] for c in cases], f)
    assert LR.bin_labels(vals, lo, hi).tolist() == [c[1] for c in cases]
    ev = LC.edge_values(LC.BINS_FRAC)
    for lo_k, hi_k in LC.BINS_FRAC:                                             # the GPU launches carry every edge
        for e in (lo_k, hi_k):
            if np.isfinite(e):
                assert f(e) in ev and above(e) in ev and (e == 0 or below(e) in ev)
    # integer counts and the standard bins
    lo = np.array([b[0] for b in LC.BINS], f); hi = np.array([b[1] for b in LC.BINS], f)
    assert LR.bin_labels(np.array([0, 1, 2, 3, 4, 5, 0.5, 3.5], f), lo, hi).tolist() == [0, 1, 2, 3, 4, 4, 0, 0]


def test_windows_helper():
    """reg = 10, pitch 8: exp underflows beyond ~32 px, at most 9 cells; reg = 20: wider; border points are cut."""
    p = np.array([[100.0, 100.0], [0.0, 223.99], [4.0, 4.0]], np.float32)
    ny, nx = LR.windows(p, 224, 8, 10.0)
    assert ny.tolist() == [9, 4, 5] and nx.tolist() == [9, 4, 5]
    ny, nx = LR.windows(p, 224, 8, 20.0)
    assert ny[0] > 9 and nx[0] > 9
    ny, nx = LR.windows(p, 224, 8, 10.0, norm=True)
    assert ny.tolist() == [28] * 3 and nx.tolist() == [28] * 3


# ------------------------------------------------------------------- the GPU launches: coverage and input conditions
def test_launches_reach_every_plan_combination():
    """Every (G, path, lanes) the plan offers is run by some crop: per LDS grid the bucketed path with full rows at 8
    lanes and, where the plan offers them, 16; compact rows (where they are shorter than full rows); dense in LDS
    (reached as the wide-window fallback, so only where g > 9 can occur: G > 8) and dense from the workspace."""
    want, got = set(), {}
    for G, size in LC.EXACT.items():
        _, _, _, _, cap_s, cap_c, cap = LC.plan(size, 8, 1)
        for n in {1, 256, 257, cap, cap + 1, cap_s, cap_s + 1, cap_c, cap_c + 1}:
            g_, first, lanes, dense, *_ = LC.plan(size, 8, n)
            assert g_ == G
            want.add((G, first, lanes))
            if first <= 1 and G > 8:
                want.add((G, dense, 0))
    for L in LC.launches():
        for b, n in enumerate(L.counts):
            if n == 0 or L.mode in (LR.MAE, LR.MSE):
                continue
            sure, may = LC.wide(L, b, -0.5), LC.wide(L, b, 0.5)
            assert sure == may, (L, b, "a factor window within half a unit of exp's underflow: the path is not certain")
            G = LC.plan(L.size, L.red, n)[0]
            got.setdefault((G, *LC.path_taken(L.size, L.red, n, sure)), []).append((L.name, b))
    assert want <= set(got), sorted(want - set(got))
    for G in LC.NEW:                                        # all four paths, both lane widths where they exist
        for path in (0, 1, 2, 3):
            assert any(k[0] == G and k[1] == path for k in got), (G, path)
        assert (G, 0, 8) in got and ((G, 1, 16) in got) == (G != 40) and ((G, 0, 16) in got) == (G != 40)
    # every size of the table, padded and exact, g = 1 and g = 3, and both wider cell pitches on a new grid
    sizes = {(L.size, L.red) for L in LC.launches() if not L.reduced or L.red > 8}
    assert {(s, 8) for s in list(LC.EXACT.values()) + list(LC.PADDED.values()) + [8, 24]} <= sizes
    assert {(320, 16), (512, 16), (640, 16), (768, 32)} <= sizes
    # the workspace crops start on an 8-byte but not 16-byte boundary: an odd point offset
    for L in LC.launches():
        for b, n in enumerate(L.counts):
            if n and L.mode not in (LR.MAE, LR.MSE) and LC.path_taken(L.size, L.red, n, LC.wide(L, b, 0.0))[0] == 3:
                assert L.offsets[b] % 2 == 1, (L, b)


def test_reg20_launches_fall_back_and_the_others_do_not():
    for L in LC.launches():
        for b, n in enumerate(L.counts):
            if n == 0:
                continue
            if L.name.startswith("w") and n > 2:
                ny, nx = LR.windows(LC.inputs(L)["points"][b], L.size, L.red, L.reg, L.norm, -0.5)
                assert max(ny.max(), nx.max()) > 9, (L, b)
            if L.reg <= 10.0 and not L.norm:
                assert not LC.wide(L, b, 0.5), (L, b)


@pytest.mark.parametrize("name", LC.names())
def test_launch_input_conditions(name):
    """What the GPU module relies on, per crop, on the float64 reference alone:
      * at most 0.1 % of the live cells have a TV sign argument within the f32 rounding of its terms;
      * pc - tc is not within the rounding of the 1024-thread sum of pc (its sign is the count gradient);
      * every err check of the Sinkhorn run is at least 2x away from stop_thr, and the f32 restatement stops where
        the f64 reference stops (so iters / rolled_back / status are well defined);
      * the loose threshold of `stop40` stops every crop at its first check."""
    L = LC.BY_NAME[name]
    refs = LC.reference(L)
    orc = LC.oracle_f32(L)
    I = LC.inputs(L)
    for b, r in enumerate(refs):
        pd = I["pred_density"][b, 0].astype(F64)
        if L.mode in (LR.MAE, LR.MSE):
            continue
        if L.mode == LR.DMCOUNT:                                # (OT alone has no TV or count gradient)
            ex = LC.tv_excluded(L, b, r)
            assert ex.sum() <= 1e-3 * L.g * L.g, (b, int(ex.sum()))
            assert abs(r["pc"] - r["n"]) > 64 * LC.U * np.abs(pd).sum(), (b, r["pc"], r["n"])
        if r["n"] == 0:
            continue
        for e in r["err"]:
            assert not (0.5 < e / L.stop_thr < 2.0), (b, r["err"])
        assert (r["iters"], r["rolled_back"]) == (orc[b]["iters"], orc[b]["rolled_back"]), (b, r["iters"], orc[b]["iters"])
        assert not r["rolled_back"]
        if name == "stop40":
            assert r["iters"] == 10 and len(r["err"]) == 1 and r["err"][0] <= L.stop_thr / 2
