"""CPU pins of tests/_sinkhorn_refs.py: the float64 loop against the C oracle, the recorded reference outputs and exact
solutions; the input conditions of every case of tests/test_gpu_sinkhorn_kernel.py; the f32 stand-in inside every bound;
each corruption the GPU module has to catch leaving a bound (or a discrete check) on one of that module's cases."""
import numpy as np
import pytest

import _sinkhorn_refs as SR
from conftest import golden, rel_l2, rel_max
from oracle import ref

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("na,nb,it,thr,log", [(17, 63, 40, 1e-7, 1), (33, 65, 25, -1.0, 0), (8, 200, 7, -1.0, 1)])
def test_f64_loop_is_the_c_oracle(na, nb, it, thr, log):
    a, b, C = SR.problem(na, nb)
    o = ref.sinkhorn(a, b, C, SR.REG, it, thr, eval_freq=10, log=bool(log))
    r = SR.sinkhorn_f64(a, b, C, SR.REG, it, thr, 10, log)
    assert o["iters"] == abs(r["info"][0]) and not o["rolled_back"] and len(o["err"]) == r["info"][1]
    for k in ("u", "v", "alpha", "beta", "P"):
        assert rel_max(o[k], r[k]) < 1e-4, k
    assert rel_l2(o["P"], r["P"]) < 2e-5
    np.testing.assert_allclose(o["err"], r["err"], rtol=2e-3, atol=1e-12)


@pytest.mark.parametrize("i", range(6))
def test_f64_loop_matches_recorded_reference(i):
    """The six F1b fixtures at the tolerances tests/test_gpu_sinkhorn.py holds the kernel to."""
    d = golden("f1b_sinkhorn.npz")
    reg, it, thr, log = (float(x) for x in d[f"cfg_{i}"])
    r = SR.sinkhorn_f64(d[f"a_{i}"], d[f"b_{i}"], d[f"C_{i}"], reg, int(it), thr, 10, int(log))
    roll = int(d[f"roll_{i}"])
    assert r["info"][0] == (-roll if roll else r["info"][0]) and r["rolled"] == bool(roll)
    P, Pref = r["P"], np.asarray(d[f"P_{i}"], F64)
    assert np.array_equal(np.isnan(P), np.isnan(Pref)) and np.array_equal(np.isinf(P), np.isinf(Pref))
    m = np.isfinite(Pref)
    assert rel_l2(P[m], Pref[m]) < 2e-5
    if log:
        for k in ("u", "v", "alpha", "beta"):
            assert rel_max(r[k], d[f"{k}_{i}"]) < 1e-4, k
        assert len(r["err"]) == len(d[f"err_{i}"])
        np.testing.assert_allclose(r["err"], d[f"err_{i}"], rtol=2e-3, atol=1e-12)


def test_exact_solutions():
    """One row: P = a_0 b / sum b.  One column: P = a b_0 / sum a after the v update, a after the u update.  A constant
    cost: P = a b^T / sum b.  The costs are a tenth of the cases' (K >= e^-2), so that the 1e-16 epsilons, which act
    relative to u K, move these by 1e-13 at most."""
    a, b, C = SR.problem(1, 70)
    r = SR.sinkhorn_f64(a, b, 0.1 * C, SR.REG, 3, -1.0, 1, 1)
    np.testing.assert_allclose(r["P"][0], F64(a[0]) * b.astype(F64) / b.astype(F64).sum(), rtol=1e-12)
    a, b, C = SR.problem(70, 1)
    r = SR.sinkhorn_f64(a, b, 0.1 * C, SR.REG, 3, -1.0, 1, 1)
    np.testing.assert_allclose(r["P"][:, 0], a.astype(F64), rtol=1e-12)
    a, b, _ = SR.problem(17, 63)
    r = SR.sinkhorn_f64(a, b, np.full((17, 63), 1.25, F32), SR.REG, 2, -1.0, 1, 1)
    np.testing.assert_allclose(r["P"], np.outer(a.astype(F64), b.astype(F64)) / b.astype(F64).sum(), rtol=1e-12)
    assert r["info"] == (2, 2) and r["err"][1] < 1e-18


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.fixture(scope="module")
def lib():
    from ebc_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("fam,na,nb", SR.SHAPES)
def test_case_input_conditions(lib, fam, na, nb):
    a, b, C = SR.problem(na, nb)
    q = np.abs(C.astype(F64) / SR.REG)
    assert q.max() <= SR.QMAX and np.exp(-q).min() >= 1e-9 and a.min() > 0 and b.min() > 0
    assert lib.ebc_sinkhorn_workspace_bytes(na, nb) == SR.workspace_bytes(na, nb)
    names = set()
    for run in SR.runs(a, b, C):
        names.add(run.name)
        r = SR.sinkhorn_f64(a, b, C, SR.REG, run.max_iter, run.thr, run.eval_freq, run.log)
        assert not r["rolled"] and all(np.isfinite(r[k]).all() for k in ("u", "v", "alpha", "beta", "P", "err"))
        assert r["info"][1] <= run.nerr_cap()
        B = SR.bounds(a, b, C, SR.REG, r, run.eval_freq)
        thr = F64(F32(run.thr))
        for e in r["err"]:                                   # the iteration count is the inputs', not the rounding's
            assert e > 2 * thr or 2 * e < thr, (run.name, e, thr)
        if run.name == "T100stop":
            assert r["info"] == (30, 3)
        elif run.name in ("T0", "thr1"):
            assert r["info"] == (0, 0) and r["T"] == 0
        else:
            assert r["info"] == (run.max_iter, run.nerr_cap() if run.log else 0)
    assert ("T100stop" in names) or (na, nb) not in SR.STOP_SHAPES
    assert SR.uv_bytes(na, nb) <= SR.LDS_MAX


def test_switch_and_limit_shapes(lib):
    assert SR.workspace_bytes(199, 199) == 0 and SR.workspace_bytes(200, 200) == 4 * 200 * 200
    assert SR.uv_bytes(1, 13631) <= SR.LDS_MAX < SR.uv_bytes(1, 13632)
    a, b, C = SR.epsilon_problem()
    r = SR.sinkhorn_f64(a, b, C, SR.REG, 1, -1.0, 1, 1)
    s = (np.full(8, F64(F32(1) / F32(8))) @ r["K"])[5]
    assert 0.5 < s / 1e-16 < 2.0                              # the epsilon doubles this column's denominator
    for rb in rollback_problems(17, 63):
        r = SR.sinkhorn_f64(*rb, SR.REG, 10, -1.0, 1, 1)
        assert r["info"] == (-1, 0) and r["T"] == 0 and np.isfinite(r["P"]).all()


def rollback_problems(na, nb):
    a, b, C = SR.problem(na, nb)
    b2, a2 = b.copy(), a.copy()
    b2[nb - 1] = np.nan
    a2[na - 1] = np.inf
    return (a, b2, C), (a2, b, C)


# ------------------------------------------------------------------------------------------------ stand-in, corruptions
def _verdicts(shapes, bug=None, run_names=None):
    """{(shape, run, kind): ratio} of the stand-in, plus (shape, run, 'info') -> 0 / inf for the discrete outputs."""
    out = {}
    for na, nb in shapes:
        a, b, C = SR.problem(na, nb)
        for run in SR.runs(a, b, C):
            if run_names and run.name not in run_names:
                continue
            r = SR.sinkhorn_f64(a, b, C, SR.REG, run.max_iter, run.thr, run.eval_freq, run.log)
            got = SR.sinkhorn_standin(a, b, C, SR.REG, run.max_iter, run.thr, run.eval_freq, run.log, bug=bug)
            out[(na, nb, run.name, "info")] = 0.0 if got["info"] == r["info"] else float("inf")
            if len(got["err"]) != len(r["err"]):
                continue
            B = SR.bounds(a, b, C, SR.REG, r, run.eval_freq)
            for kind, (e, bd) in SR.compare(got, r, B).items():
                out[(na, nb, run.name, kind)] = SR.ratio(e, bd)
    return out


def test_standin_is_inside_every_bound():
    v = _verdicts([(17, 63), (5, 1025), (199, 199), (1, 70), (70, 1)])
    worst = {}
    for (na, nb, run, kind), r in v.items():
        worst[kind] = max(worst.get(kind, 0.0), r)
    print({k: round(x, 4) for k, x in worst.items()})
    assert all(r <= 1.0 for r in v.values()), {k: r for k, r in v.items() if r > 1.0}


CORRUPTIONS = [("swap_ij", (17, 63), "T1", "P"), ("row_stop_64", (17, 63), "T1", "u"), ("col_stop_1024", (5, 1025), "T1", "v"),
               ("ktu_stale", (17, 63), "T4f2", "v"), ("err_shift", (17, 63), "T2", "err"), ("info_it", (17, 63), "T1", "info")]


@pytest.mark.parametrize("bug,shape,run,kind", CORRUPTIONS)
def test_corruptions_leave_a_bound(bug, shape, run, kind):
    v = _verdicts([shape], bug=bug, run_names={run})
    assert v[(*shape, run, kind)] > 1.0, (bug, v)


def test_epsilon_corruption_fails_the_epsilon_case_and_no_other():
    a, b, C = SR.epsilon_problem()
    r = SR.sinkhorn_f64(a, b, C, SR.REG, 1, -1.0, 1, 1)
    B = SR.bounds(a, b, C, SR.REG, r, 1)
    ok = SR.compare(SR.sinkhorn_standin(a, b, C, SR.REG, 1, -1.0, 1, 1), r, B)
    assert all(SR.ratio(e, bd) <= 1.0 for e, bd in ok.values())
    bad = SR.compare(SR.sinkhorn_standin(a, b, C, SR.REG, 1, -1.0, 1, 1, bug="eps_1e-12"), r, B)
    assert SR.ratio(*bad["v"]) > 1.0
    v = _verdicts([(17, 63), (5, 1025)], bug="eps_1e-12", run_names={"T1", "T2", "T4", "T25"})
    assert all(x <= 1.0 for x in v.values())
