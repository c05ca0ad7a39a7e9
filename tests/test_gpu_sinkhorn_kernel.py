"""csrc/sinkhorn.hip (ebc_sinkhorn) per element against the float64 loop of tests/_sinkhorn_refs.py, whose module
docstring counts the bounds: u, v and P in log space, alpha, beta and err absolutely.  Shapes on both sides of every
stride and of the K-in-LDS / K-in-workspace switch, iteration counts 0, 1, 2, 4, 25, 100, stops, rollbacks, the 1e-16
epsilon, NULL outputs.  Every output is the middle of a framed sentinel buffer; the err buffer is exactly
floor(max_iter / eval_freq) long, the workspace exactly ebc_sinkhorn_workspace_bytes.  tests/test_sinkhorn_refs_cpu.py
asserts the cases' input conditions.  Each check prints "RATIO sk.<family>.<shape>.<run>.<output> <error / bound>"."""
import ctypes

import numpy as np
import pytest
import torch

import _kernel_checks as KC
import _sinkhorn_refs as SR
from ebc_amd import _lib

pytestmark = pytest.mark.gpu

EBC_E_ARG, EBC_E_UNSUPPORTED = -1, -3
F32 = np.float32
OUTS = ("P", "u", "v", "alpha", "beta", "err")


def _mid_ptr(fr):
    """The pointer of fr.mid (torch gives an empty view no pointer: the err buffer of a run without checks)."""
    cols = fr.full.shape[1]
    return ctypes.c_void_p(fr.full.data_ptr() + KC.GUARD_ROWS * cols * fr.full.element_size())


def _report(name, err, bound):
    r = SR.ratio(err, bound)
    print(f"RATIO {name} {r:.4f}")
    assert r <= 1.0, (name, r)


def _call(a, b, C, reg, run, null=(), short_ws=0, expect=0):
    """One launch.  Returns the outputs asked for (err cut to the entries written) and info, after checking every frame."""
    lib = _lib.lib()
    na, nb = C.shape
    H = KC._Hold()
    f32 = torch.float32
    fr = dict(P=KC._Framed(na, nb, f32), u=KC._Framed(na, 1, f32), v=KC._Framed(nb, 1, f32), alpha=KC._Framed(na, 1, f32),
              beta=KC._Framed(nb, 1, f32), err=KC._Framed(run.nerr_cap(), 1, f32), info=KC._Framed(2, 1, torch.int32))
    need = lib.ebc_sinkhorn_workspace_bytes(na, nb)
    assert need in (0, 4 * na * nb)
    ws = KC._Framed(need // 4, 4, torch.uint8) if need else None
    ptr = {k: (None if k in null else _mid_ptr(f)) for k, f in fr.items()}
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, F32))
    rc = lib.ebc_sinkhorn(H(t(a)), H(t(b)), H(t(C)), na, nb, reg, run.max_iter, run.thr, run.eval_freq, run.log,
                          ptr["P"], ptr["u"], ptr["v"], ptr["alpha"], ptr["beta"], ptr["err"], ptr["info"],
                          _mid_ptr(ws) if ws is not None else None, need - short_ws, _lib.stream(fr["P"].full))
    torch.cuda.synchronize()
    assert rc == expect, rc
    for k, f in fr.items():
        assert f.ok(), f"a write outside {k}"
    assert ws is None or ws.ok(), "a write outside the workspace"
    if expect:
        assert all(bool((f.mid == f.fill).all()) for f in fr.values()), "a refused call wrote an output"
        return None
    got = {k: fr[k].mid.cpu().numpy().reshape(-1) for k in OUTS if k not in null}
    for k in null:
        assert bool((fr[k].mid == KC.SENT).all()), f"{k} was NULL and its buffer was written"
    info = tuple(int(x) for x in fr["info"].mid.cpu().numpy().reshape(-1))
    got["info"] = info
    if "P" in got:
        got["P"] = got["P"].reshape(na, nb)
    if "err" in got:
        assert 0 <= info[1] <= run.nerr_cap() and bool((got["err"][info[1]:] == KC.SENT).all())
        got["err"] = got["err"][:info[1]]
    return got


def _check(tag, a, b, C, run, got):
    r = SR.sinkhorn_f64(a, b, C, SR.REG, run.max_iter, run.thr, run.eval_freq, run.log)
    assert got["info"] == r["info"], (tag, got["info"], r["info"])
    B = SR.bounds(a, b, C, SR.REG, r, run.eval_freq)
    for kind, (e, bd) in SR.compare(got, r, B).items():
        _report(f"{tag}.{kind}", e, bd)
    return r


@pytest.mark.parametrize("fam,na,nb", SR.SHAPES)
def test_runs_per_element(fam, na, nb):
    lib = _lib.lib()
    a, b, C = SR.problem(na, nb)
    need = lib.ebc_sinkhorn_workspace_bytes(na, nb)
    print(f"{na}x{nb}: K in {'the workspace' if need else 'LDS'}")
    if (na, nb) in ((199, 199), (200, 200)):
        assert (need == 0) == (na == 199)
    got = {}
    for run in SR.runs(a, b, C):
        got[run.name] = _call(a, b, C, SR.REG, run)
        _check(f"sk.{fam}.{na}x{nb}.{run.name}", a, b, C, run, got[run.name])
    assert ("T100stop" in got) or (na, nb) not in SR.STOP_SHAPES
    # without the log every iteration runs and nothing is reused: the same bits as the logged run that reuses K^T u
    for k in ("P", "u", "v", "alpha", "beta"):
        assert got["T4nolog"][k].tobytes() == got["T4"][k].tobytes(), k
    for name in ("T0", "thr1"):                       # no iteration: the initial u and v, P = K / (na nb)
        assert got[name]["info"] == (0, 0)
        assert got[name]["u"].tobytes() == np.full(na, F32(1) / F32(na), F32).tobytes()
        assert got[name]["v"].tobytes() == np.full(nb, F32(1) / F32(nb), F32).tobytes()
    if need:                                          # a byte less than the workspace, or none, is refused
        _call(a, b, C, SR.REG, SR.Run("T1", 1, 1, 1), short_ws=1, expect=EBC_E_ARG)
        ws_null = lib.ebc_sinkhorn(0x1000, 0x1000, 0x1000, na, nb, SR.REG, 1, -1.0, 1, 1, *([None] * 6), 0x1000, None, need, None)
        assert ws_null == EBC_E_ARG


@pytest.mark.parametrize("na,nb", [(17, 63), (200, 200)])
def test_null_outputs(na, nb):
    a, b, C = SR.problem(na, nb)
    run = SR.Run("T25", 25, 10, 1)
    full = _call(a, b, C, SR.REG, run)
    for null in [(k,) for k in OUTS] + [OUTS]:
        got = _call(a, b, C, SR.REG, run, null=null)
        assert got["info"] == full["info"] == (25, 2)
        for k in OUTS:
            assert k in null or got[k].tobytes() == full[k].tobytes(), (null, k)


def test_oversize_is_unsupported_without_a_launch():
    a, b, C = SR.problem(1, 13633)
    _call(a, b, C, SR.REG, SR.Run("T1", 1, 1, 1), expect=EBC_E_UNSUPPORTED)


def test_epsilon_case():
    """K^T u of one column is near 1e-16: the epsilon in the denominator halves that v_j."""
    a, b, C = SR.epsilon_problem()
    run = SR.Run("T1", 1, 1, 1)
    got = _call(a, b, C, SR.REG, run)
    r = _check("sk.epsilon.8x64.T1", a, b, C, run, got)
    no_eps = F32(b[5]) / (np.full(8, 0.125) @ r["K"][:, 5])
    assert 1.5 < no_eps / got["v"][5] < 3.0


@pytest.mark.parametrize("na,nb", [(32, 63), (208, 200)])
@pytest.mark.parametrize("where", ["b_nan", "a_inf"])
def test_rollback(na, nb, where):
    """A NaN in b[nb - 1] (the last active thread's column) or an inf in a[na - 1] (a row of the last wave): iteration 1
    is not finite, the initial u and v stay and info[0] = -1; every output per element against the restated loop."""
    lib = _lib.lib()
    assert (na - 1) % 16 == 15 and (lib.ebc_sinkhorn_workspace_bytes(na, nb) > 0) == (na == 208)
    a, b, C = SR.problem(na, nb)
    if where == "b_nan":
        b[nb - 1] = np.nan
    else:
        a[na - 1] = np.inf
    run = SR.Run("T10", 10, 1, 1)
    got = _call(a, b, C, SR.REG, run)
    assert got["info"] == (-1, 0)
    _check(f"sk.rollback.{na}x{nb}.{where}", a, b, C, run, got)
    assert got["u"].tobytes() == np.full(na, F32(1) / F32(na), F32).tobytes()
    assert got["v"].tobytes() == np.full(nb, F32(1) / F32(nb), F32).tobytes()


def test_two_runs_are_the_same_bits():
    a, b, C = SR.problem(41, 1000)
    run = SR.Run("T100", 100, 10, 1)
    x, y = _call(a, b, C, SR.REG, run), _call(a, b, C, SR.REG, run)
    assert x["info"] == y["info"] == (100, 10)
    for k in OUTS:
        assert x[k].tobytes() == y[k].tobytes(), k
