"""The float64 references of tests/_gemm_refs.py against torch's own float64 ops, autograd and plain indexing (no GPU),
to 1e-12 relative, and the facts the bounds of tests/test_gpu_gemm_kernels.py lean on."""
import pytest
import torch
import torch.nn.functional as F

import _bn_refs
import _gemm_refs as R

F64 = torch.float64
DTS = [torch.float32, torch.float16, torch.bfloat16]


def _close(a, b, tol=1e-12):
    a, b = a.detach().to(F64), b.detach().to(F64)
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def test_quick_gelu_and_its_derivative():
    x = torch.cat([_rand(4096, seed=1) * 4, torch.linspace(-30, 30, 2001, dtype=F64)]).requires_grad_(True)
    y = x * torch.sigmoid(1.702 * x)
    _close(R.quick_gelu(x.detach()), y)
    (g,) = torch.autograd.grad(y.sum(), x)
    _close(R.quick_gelu_grad(x.detach()), g)
    _close(R.sigmoid1702(x.detach()), torch.sigmoid(1.702 * x.detach()))


def test_quick_gelu_slope_is_below_the_constant_the_bound_uses():
    x = torch.linspace(-40, 40, 800001, dtype=F64)
    m = float(R.quick_gelu_grad(x).abs().max())
    assert 1.0998 < m <= R.GELU_SLOPE - 1e-4


def test_arithmetic_error_terms_are_finite_and_bounded():
    """The f32 evaluation's own error stays a few units of (1 + |x|) over the whole range: no blow-up where s -> 0 or 1
    (the derivative's 1 - s inherits the sigmoid's absolute error, which 1.702 x then scales)."""
    x = torch.linspace(-60, 60, 240001, dtype=F64)
    ga, gg = R.gelu_arith(x), R.gelu_grad_arith(x)
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gg).all())
    assert float((ga / (1.0 + x.abs())).max()) < 8.0 and float((gg / (1.0 + x.abs())).max()) < 16.0
    assert float(ga.min()) >= 0.0 and float(gg.min()) >= 0.0


@pytest.mark.parametrize("dt", DTS)
def test_ulp_equals_the_spacing_of_the_type(dt):
    x = torch.cat([_rand(2000, seed=3) * 50, _rand(500, seed=4) * 1e-6, torch.tensor([0.0, 1.0, -2.0, 0.5, 65504.0, 1e-7],
                                                                                       dtype=F64)])
    assert torch.equal(R.ulp(x, dt), _bn_refs.ulp(x, dt))
    p = R.SIG_BITS[dt]
    spot = torch.tensor([1.0, -1.5, 3.0, 0.0, 2.0 ** -130], dtype=F64)
    sub = 2.0 ** (R.MIN_EXP[dt] - (p - 1))
    assert R.ulp(spot, dt).tolist() == [2.0 ** (1 - p), 2.0 ** (1 - p), 2.0 ** (2 - p), sub, sub]
    v = x.to(dt)                                        # v + ulp(v) is the next value of the type
    v = v[torch.isfinite(v) & (v.abs() < 6e4)].to(F64).abs()
    nxt = v + R.ulp(v, dt)
    assert torch.equal(nxt.to(dt).to(F64), nxt) and torch.equal((v + 0.25 * R.ulp(v, dt)).to(dt).to(F64), v)


@pytest.mark.parametrize("M,rpg,gs,go", [(7, 0, 0, 0), (15, 5, 23, 1), (13, 5, 23, 1), (8, 4, 7, 3), (3, 1, 7, 6)])
def test_row_map_is_plain_indexing(M, rpg, gs, go):
    rows = R.row_map(M, rpg, gs, go).tolist()
    want = [r if rpg == 0 else (r // rpg) * gs + go + r % rpg for r in range(M)]
    assert rows == want and len(set(rows)) == M


@pytest.mark.parametrize("Rr,C,pad", [(1, 8, 7), (7, 8, 9), (9, 72, 7), (65, 200, 15)])
def test_transpose_padded(Rr, C, pad):
    x = _rand(Rr, C, seed=5)
    ld = Rr + pad
    out = R.transpose_padded(x, ld, 7.0)
    assert out.shape == (C, ld)
    for c in range(C):
        for r in range(ld):
            assert float(out[c, r]) == (float(x[r, c]) if r < Rr else 7.0)


@pytest.mark.parametrize("dt", DTS)
def test_epilogues_against_torch(dt):
    M, N, K = 9, 16, 24
    A, B = _rand(M, K, seed=1).to(dt), (_rand(N, K, seed=2) / K ** 0.5).to(dt)
    bias, resid, aux = _rand(N, seed=3).float(), _rand(M, N, seed=4).float(), _rand(M, N, seed=5).to(dt)
    P, Sp = R.product(A, B)
    lin = F.linear(A.to(F64), B.to(F64))
    _close(P, lin)
    _close(Sp, F.linear(A.to(F64).abs(), B.to(F64).abs()))
    pre = F.linear(A.to(F64), B.to(F64), bias.to(F64))
    out = R.epilogue(R.STORE, P, Sp, K, dt, torch.float32, bias=bias)
    _close(out["C"][0], pre)
    _close(R.epilogue(R.STORE, P, Sp, K, dt, dt)["C"][0], lin)
    out = R.epilogue(R.GELU, P, Sp, K, dt, dt, bias=bias)
    _close(out["aux"][0], pre)
    _close(out["C"][0], pre * torch.sigmoid(1.702 * pre))
    _close(R.epilogue(R.RESID, P, Sp, K, dt, torch.float32, bias=bias, resid=resid)["C"][0], resid.to(F64) + pre)
    a = aux.to(F64).requires_grad_(True)
    (g,) = torch.autograd.grad((a * torch.sigmoid(1.702 * a)).sum(), a)
    _close(R.epilogue(R.GELU_BWD, P, Sp, K, dt, dt, aux=aux)["C"][0], lin * g)


@pytest.mark.parametrize("dt", DTS)
def test_bounds_have_the_stated_form(dt):
    """STORE / RESID: c * u * S with c = 2K (+1 for f32 products) + one per add, doubled behind a 16-bit store and
    with ulp_T(ref) / 2 added there; a split K: 2K / s + s."""
    M, N, K = 5, 8, 64
    A, B = _rand(M, K, seed=1).to(dt), _rand(N, K, seed=2).to(dt)
    bias, resid = _rand(N, seed=3).float(), _rand(M, N, seed=4).float()
    P, Sp = R.product(A, B)
    f = 1 if dt == torch.float32 else 0
    S = Sp + bias.to(F64).abs() + resid.to(F64).abs()
    ref, b = R.epilogue(R.RESID, P, Sp, K, dt, torch.float32, bias=bias, resid=resid)["C"]
    _close(b, R.units(2 * K + f + 2) * S)
    if dt != torch.float32:
        ref, bt = R.epilogue(R.RESID, P, Sp, K, dt, dt, bias=bias, resid=resid)["C"]
        _close(bt, 0.5 * R.ulp(ref, dt) + 2 * b)
    _, b = R.epilogue(R.STORE, P, Sp, K, dt, torch.float32, splits=4)["C"]
    _close(b, R.units(2 * K / 4 + 4 + f) * Sp)
    assert R.units(6146) < 6146 * R.U * 1.0004
