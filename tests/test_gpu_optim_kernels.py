"""csrc/optim.hip at the ABI level (ebc_amp_check, ebc_adam_update, ebc_adam_step) against tests/_optim_refs.py: the inf
check at every element position its three paths can miss, the update per element against float64 with bounds counted from
adam_elem's rounding points, a dyadic case that is bit-exact, a skipped step that changes nothing, and the scaler
sequence against the restated torch._amp_update_scale_.  Every operand (parameters, gradients, both moments, the step
count, the scaler words) is the middle of a framed sentinel buffer whose bits outside the operand must not change.
Each per-element check prints "RATIO <case>.<output> <largest error / bound>" before it asserts."""
import numpy as np
import pytest
import torch

import _kernel_checks as KC
import _optim_refs as OR
from ebc_amd import _lib

pytestmark = pytest.mark.gpu

EBC_E_ARG = -1
F32 = np.float32
I32 = torch.int32


class _Op:
    """n f32 elements in the middle of a KC._Framed buffer, starting `off` elements past a 16-byte boundary."""

    def __init__(self, n, off=0):
        self.fr = KC._Framed(1, n + off, torch.float32)
        self.flat = self.fr.full.view(-1)
        self.lo, self.n = KC.GUARD_ROWS * (n + off) + off, n
        self.t = self.flat[self.lo:self.lo + n]
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 4 * off
        self.before = None

    def put(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, F32).reshape(-1)))

    def get(self):
        return self.t.cpu().numpy()

    def snap(self):
        self.before = self.flat.clone()

    def frame_ok(self):
        a, b, hi = self.flat.view(I32), self.before.view(I32), self.lo + self.n
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[hi:], b[hi:])

    def same(self):
        return torch.equal(self.flat.view(I32), self.before.view(I32))


class _Tensor:
    def __init__(self, n, layout):
        self.n, self.layout = n, layout
        self.p, self.g = _Op(n, int(layout == "param+1")), _Op(n, int(layout == "grad+1"))
        self.m, self.v = _Op(n), _Op(n)
        self.ops = (self.p, self.g, self.m, self.v)
        # the layout, from the pointers: the vector paths need all four operands on a 16-byte boundary
        self.aligned = all(o.ptr % 16 == 0 for o in self.ops)
        assert self.aligned == (layout == "aligned")
        assert [o.ptr % 16 for o in self.ops] == [4 * (layout == "param+1"), 4 * (layout == "grad+1"), 0, 0]

    def desc(self):
        return _lib.EbcAdamTensor(self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.n)


def _array(ts):
    return (_lib.EbcAdamTensor * len(ts))(*[t.desc() if isinstance(t, _Tensor) else t for t in ts])


def _stream():
    return _lib.stream(torch.device("cuda:0"))


def _report(name, pairs):
    r = max(OR.ratio(e, b) for e, b in pairs)
    print(f"RATIO {name} {r:.4f}")
    assert r <= 1.0, (name, r)


def _bits(a):
    return np.ascontiguousarray(a, F32).tobytes()


SC_WORDS = np.array([65536.0, 3.0, 0.0, 1024.0, 7.0, 0.0], F32)


# ------------------------------------------------------------------------------------------------ a. the inf check
@pytest.mark.parametrize("layout", OR.LAYOUTS)
def test_inf_check_reaches_every_element(layout):
    """One call per position with exactly one non-finite gradient element, and one call per size with none (FLT_MAX,
    -FLT_MAX, a denormal, -0.0 inside, NaN in the frame elements on both sides: a read outside numel raises the flag)."""
    lib = _lib.lib()
    sc = _Op(6)
    calls = 0
    for n in OR.SIZES:
        T = _Tensor(n, layout)
        clean = OR.clean_edge_grad(n, n)
        T.g.flat[T.g.lo - 1] = float("nan")
        T.g.flat[T.g.lo + n] = float("nan")
        arr = _array([T])
        for k, pos in enumerate([None] + OR.check_positions(n, T.aligned)):
            g = clean.copy()
            if pos is not None:
                g[pos] = OR.BAD[(k - 1) % 3]
            T.g.put(g)
            par = k & 1
            sc.put(SC_WORDS)
            for o in (*T.ops, sc):
                o.snap()
            assert lib.ebc_amp_check(arr, 1, sc.ptr, par, _stream()) == 0
            torch.cuda.synchronize()
            want = SC_WORDS.copy()
            if pos is not None:
                want[3 * par + 2] = 1.0
            assert _bits(sc.get()) == _bits(want), (n, layout, pos, sc.get())
            assert sc.frame_ok() and all(o.same() for o in T.ops), (n, layout, pos)
            calls += 1
    assert calls >= len(OR.SIZES) * 2


@pytest.mark.parametrize("count", [32, 33, 64, 65])
def test_inf_check_pack_boundaries(count):
    """32 tensors go into one launch: the bad element in the last tensor of a list of 32, 33, 64, 65, and in the first."""
    lib = _lib.lib()
    sc, p, m, v = _Op(6), _Op(5), _Op(5), _Op(5)
    gs = [_Op(5) for _ in range(count)]
    rng = np.random.Generator(np.random.PCG64(count))
    for g in gs:
        g.put(rng.standard_normal(5))
    arr = _array([_lib.EbcAdamTensor(p.ptr, g.ptr, m.ptr, v.ptr, 5) for g in gs])
    for k, where in enumerate([None, count - 1] + ([0] if count in (33, 65) else [])):
        if where is not None:
            gs[where].t[4 - k] = OR.BAD[k % 3]
        sc.put(SC_WORDS)
        for o in (sc, p, m, v, *gs):
            o.snap()
        assert lib.ebc_amp_check(arr, count, sc.ptr, 1, _stream()) == 0
        torch.cuda.synchronize()
        want = SC_WORDS.copy()
        want[5] = 0.0 if where is None else 1.0
        assert _bits(sc.get()) == _bits(want), (count, where)
        assert all(o.same() for o in (p, m, v, *gs)) and sc.frame_ok()
        if where is not None:
            gs[where].t[4 - k] = 0.5
    if count == 33:
        for bad in (_lib.EbcAdamTensor(p.ptr, None, m.ptr, v.ptr, 5), _lib.EbcAdamTensor(None, gs[32].ptr, m.ptr, v.ptr, 5),
                    _lib.EbcAdamTensor(p.ptr, gs[32].ptr, m.ptr, v.ptr, 0)):
            arr[32] = bad
            assert lib.ebc_amp_check(arr, 33, sc.ptr, 0, _stream()) == EBC_E_ARG
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ b. the update
@pytest.fixture(scope="module")
def tensors():
    ts = [_Tensor(n, layout) for layout in OR.LAYOUTS for n in OR.SIZES]
    return ts + [_Tensor(2, "aligned"), _Tensor(7, "grad+1"), _Tensor(4100, "param+1")]


class _State:
    """The step count float[2] and the scaler float[2][3], framed, with their parities; the entries a launch does not
    read hold junk (a raised flag among it), so a launch that reads the wrong entry shows."""

    def __init__(self, step0, scale, spar, tracker=5.0):
        self.step, self.sc = _Op(2), (_Op(6) if scale is not None else None)
        self.spar, self.cpar = spar, 1 - spar
        w = np.full(2, 777.0, F32)
        w[spar] = step0
        self.step.put(w)
        if self.sc is not None:
            w = np.array([123.0, 9.0, 1.0] * 2, F32)
            w[3 * self.cpar:3 * self.cpar + 3] = [scale, tracker, 0.0]
            self.sc.put(w)

    def words(self):
        return self.step.get(), (self.sc.get() if self.sc is not None else None)

    def scale(self):
        return None if self.sc is None else float(self.sc.get()[3 * self.cpar])


def _launch(lib, ts, S, h, wg, split):
    arr = _array(ts)
    hyper = (h.lr, h.beta1, h.beta2, h.eps, h.wd, h.growth, h.backoff, h.interval, wg, _stream())
    scp = S.sc.ptr if S.sc is not None else None
    if split:
        if S.sc is not None:
            assert lib.ebc_amp_check(arr, len(ts), scp, S.cpar, _stream()) == 0
        rc = lib.ebc_adam_update(arr, len(ts), S.step.ptr, S.spar, scp, S.cpar, *hyper)
    else:
        rc = lib.ebc_adam_step(arr, len(ts), S.step.ptr, S.spar, scp, S.cpar, *hyper)
    assert rc == 0, rc
    torch.cuda.synchronize()


def _applied_step(lib, name, ts, host, S, h, wg, split, seed):
    """One clean step of the list: launches, then holds every tensor to the bounds and the state to the scaler
    function.  `host` holds the (p, m, v) the device has; it is replaced by what the kernel left."""
    st0, sc0 = S.words()
    step, scale = float(st0[S.spar]), S.scale()
    grads = [OR.grad_inputs(t.n, seed + 31 * i, scale) for i, t in enumerate(ts)]
    for t, g in zip(ts, grads):
        t.g.put(g)
    ops = [o for t in ts for o in t.ops] + [S.step] + ([S.sc] if S.sc is not None else [])
    for o in ops:
        o.snap()
    _launch(lib, ts, S, h, wg, split)
    assert all(o.frame_ok() for o in ops), name
    st1, sc1 = S.words()
    # the entry read keeps its bits, the other one is the restated update
    want_st = st0.copy()
    if S.sc is not None:
        cur = sc0[3 * S.cpar:3 * S.cpar + 3]
        ns, nt, nf, nstep = OR.scaler_next(cur[0], cur[1], False, step, h)
        want_sc = sc0.copy()
        want_sc[3 * (1 - S.cpar):3 * (1 - S.cpar) + 3] = [ns, nt, nf]
        assert _bits(sc1) == _bits(want_sc), (name, sc1, want_sc)
    else:
        nstep = F32(step) + F32(1)
    want_st[1 - S.spar] = nstep
    assert _bits(st1) == _bits(want_st), (name, st1, want_st)
    kinds = {}
    for i, (t, g) in enumerate(zip(ts, grads)):
        p0, m0, v0 = host[i]
        after = tuple(o.get() for o in t.ops)
        for kind, eb in OR.step_ratios((p0, g, m0, v0), after, step, h, scale, wg).items():
            kinds.setdefault(kind, []).append(eb)
        if scale is None or not wg:
            assert _bits(after[1]) == _bits(g), (name, i, "the gradient buffer was written")
        elif OR.is_pow2(scale):
            assert _bits(after[1]) == _bits((g.astype(np.float64) / scale).astype(F32)), (name, i)
        if h.lr == 0.0:
            assert _bits(after[0]) == _bits(p0), (name, i, "lr = 0 moved a parameter")
            assert _bits(after[2]) != _bits(m0) and _bits(after[3]) != _bits(v0)
        host[i] = (after[0], after[2], after[3])
    for kind, pairs in sorted(kinds.items()):
        _report(f"adam.{name}.{kind}", pairs)
    S.spar, S.cpar = 1 - S.spar, 1 - S.cpar


def _fresh(ts, seed=0):
    host = [OR.tensor_inputs(t.n, seed + 1000 + 17 * i) for i, t in enumerate(ts)]
    for t, (p, m, v) in zip(ts, host):
        t.p.put(p), t.m.put(m), t.v.put(v)
    return host


RUNS = [(hn, mn, OR.STEPS0[(hi + mi) % 3], (hi + mi) % 2)
        for hi, hn in enumerate(OR.HYPERS) for mi, mn in enumerate(OR.MODES)]


@pytest.mark.parametrize("hn,mn,step0,split", RUNS)
def test_update_per_element(tensors, hn, mn, step0, split):
    """Three consecutive steps of the ten sizes in the three layouts (one launch of 30 tensors), from non-zero moments."""
    lib = _lib.lib()
    h, (scale, wg) = OR.HYPERS[hn], OR.MODES[mn]
    ts = tensors[:30]
    host = _fresh(ts)
    S = _State(step0, scale, spar=split)
    for k in range(3):
        _applied_step(lib, f"{hn}.{mn}.s{int(step0) + k}", ts, host, S, h, wg, bool(split), seed=100 * k + 7)


def test_update_33_mixed_tensors(tensors):
    """Two launches: the scaler and the step count are written by the second one only, the first reads the same entry."""
    lib = _lib.lib()
    host = _fresh(tensors, seed=5)
    S = _State(1.0, 3.0, spar=1)
    for k in range(2):
        _applied_step(lib, f"list33.s{1 + k}", tensors, host, S, OR.HYPERS["default_wd"], 1, False, seed=900 + k)


# ------------------------------------------------------------------------------------------------ c. dyadic
def test_dyadic_step_is_bit_exact(tensors):
    """Powers of two for lr, the betas' complements, wd and the scale, small integers times powers of two for the
    operands, step 0: g', gr, m' and v' are exact in f32, so the stored bits are the reference's."""
    lib = _lib.lib()
    h = OR.Hyper(lr=2.0 ** -10, beta1=0.5, beta2=0.25, eps=2.0 ** -20, wd=2.0 ** -3)
    rng = np.random.Generator(np.random.PCG64(11))
    S = _State(0.0, 65536.0, spar=0)
    host, grads = [], []
    for t in tensors:
        p = rng.integers(-8, 9, t.n) * 0.5
        m = rng.integers(-16, 17, t.n) * 0.125
        v = rng.integers(0, 17, t.n) * 2.0 ** -6
        g = rng.integers(-16, 17, t.n) * 0.125 * 65536.0
        t.p.put(p), t.m.put(m), t.v.put(v), t.g.put(g)
        host.append((p, m, v))
        grads.append(g)
    ops = [o for t in tensors for o in t.ops]
    for o in ops:
        o.snap()
    _launch(lib, tensors, S, h, 1, False)
    assert all(o.frame_ok() for o in ops)
    pairs = []
    for t, (p, m, v), g in zip(tensors, host, grads):
        r = OR.adam_f64(p, g, m, v, 0.0, h, 65536.0)
        for o, k in ((t.g, "g1"), (t.m, "m1"), (t.v, "v1")):
            KC._exact(o.t, torch.from_numpy(r[k]), torch.float32)
        after = tuple(o.get() for o in t.ops)
        pairs.append(OR.step_ratios((p, g, m, v), after, 0.0, h, 65536.0, 1)["p"])
    _report("adam.dyadic.p", pairs)


# ------------------------------------------------------------------------------------------------ d. a skipped step
def test_skipped_step_changes_nothing_then_a_clean_step_uses_the_backed_off_scale(tensors):
    lib = _lib.lib()
    h = OR.Hyper(wd=1e-4, growth=1.5, backoff=0.25, interval=3)
    host = _fresh(tensors, seed=9)
    S = _State(4.0, 3.0, spar=0, tracker=2.0)               # a growth is due: the skip must win
    for i, t in enumerate(tensors):
        t.g.put(OR.grad_inputs(t.n, 40 + i, 3.0))
    last = tensors[-1]
    last.g.t[last.n - 1] = float("nan")
    st0, sc0 = S.words()
    ops = [o for t in tensors for o in t.ops]
    for o in ops + [S.step, S.sc]:
        o.snap()
    _launch(lib, tensors, S, h, 1, False)
    assert all(o.same() for o in ops), "a skipped step wrote a tensor"
    assert S.step.frame_ok() and S.sc.frame_ok()
    st1, sc1 = S.words()
    ns, nt, nf, nstep = OR.scaler_next(3.0, 2.0, True, 4.0, h)
    assert (float(ns), float(nt), float(nstep)) == (0.75, 0.0, 4.0)
    want_sc = sc0.copy()
    want_sc[3 * S.cpar + 2] = 1.0                            # the flag the check raised, in the entry it read
    want_sc[3 * (1 - S.cpar):3 * (1 - S.cpar) + 3] = [ns, nt, nf]
    want_st = st0.copy()
    want_st[1 - S.spar] = nstep                              # not advanced
    assert _bits(sc1) == _bits(want_sc) and _bits(st1) == _bits(want_st), (sc1, st1)
    S.spar, S.cpar = 1 - S.spar, 1 - S.cpar
    assert S.scale() == 0.75
    _applied_step(lib, "afterskip.s4", tensors, host, S, h, 1, False, seed=77)


# ------------------------------------------------------------------------------------------------ e. scaler sequence
@pytest.mark.parametrize("name,scale0,skips", [("issue", 2.0 ** 127, {2, 7}), ("refused", 1.5 * 2.0 ** 127, {7})])
def test_scaler_sequence(name, scale0, skips):
    """12 steps, interval 3, growth 1.5, backoff 0.25; all eight state words after every step.  From 2^127 with skips
    at steps 2 and 7 every growth is finite; from 1.5 * 2^127 the growth of step 2 overflows: the scale stays and the
    tracker still resets (test_optim_refs_cpu.py asserts that the reference sequence holds such a step)."""
    lib = _lib.lib()
    h = OR.Hyper(growth=1.5, backoff=0.25, interval=3)
    T = _Tensor(5, "aligned")
    p, m, v = OR.tensor_inputs(5, 1)
    T.p.put(p), T.m.put(m), T.v.put(v)
    S = _State(0.0, scale0, spar=1, tracker=0.0)
    want_st, want_sc = S.words()
    refused = 0
    for i in range(12):
        g = np.ones(5, F32)
        if i in skips:
            g[i % 5] = OR.BAD[i % 3]
        T.g.put(g)
        for o in (S.step, S.sc):
            o.snap()
        _launch(lib, [T], S, h, 1, bool(i & 1))
        cur = want_sc[3 * S.cpar:3 * S.cpar + 3].copy()
        ns, nt, nf, nstep = OR.scaler_next(cur[0], cur[1], i in skips, want_st[S.spar], h)
        refused += int(i not in skips and cur[1] == 2.0 and ns == cur[0])
        if i in skips:
            want_sc[3 * S.cpar + 2] = 1.0
        want_sc[3 * (1 - S.cpar):3 * (1 - S.cpar) + 3] = [ns, nt, nf]
        want_st[1 - S.spar] = nstep
        st1, sc1 = S.words()
        assert _bits(sc1) == _bits(want_sc) and _bits(st1) == _bits(want_st), (name, i, sc1, want_sc, st1, want_st)
        assert S.step.frame_ok() and S.sc.frame_ok()
        S.spar, S.cpar = 1 - S.spar, 1 - S.cpar
    assert (refused >= 1) == (name == "refused")             # (the scale stays, so later growths are refused again)
    assert np.isfinite(T.p.get()).all()
