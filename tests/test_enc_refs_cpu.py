"""The float64 references of tests/_enc_refs.py against torch's own float64 ops and autograd (no GPU), to 1e-12
relative, and the stated conditions of the input generators of tests/test_gpu_encoder_kernels.py."""
import math

import pytest
import torch
import torch.nn.functional as F

import _enc_refs as R

F64 = torch.float64
DTS = [torch.float32, torch.float16, torch.bfloat16]


def _close(a, b, tol=1e-12, floor=1e-300):
    """max |a - b| <= tol * max(max |b|, floor); floor is the size of the terms where b itself cancels to 0."""
    a, b = a.detach().to(F64), b.detach().to(F64)
    scale = max(float(b.abs().max()), floor)
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ LayerNorm
MAPS = [(5, 0, 0, 0, 5), (8, 4, 7, 3, 14), (7, 3, 5, 2, 13), (3, 1, 7, 6, 21)]       # M, rpg, gstride, goff, source rows


@pytest.mark.parametrize("M,rpg,gs,go,N", MAPS)
def test_layernorm_forward_and_backward(M, rpg, gs, go, N):
    D = 48
    x = (_rand(N, D, seed=1) * 3 + 1).requires_grad_(True)
    gamma, beta = _rand(D, seed=2) * 0.1 + 1, _rand(D, seed=3) * 0.1
    rows = R.ln_rows(M, rpg, gs, go)
    assert int(rows.max()) < N and len(set(rows.tolist())) == M
    if rpg > 0:
        assert rows.tolist() == [(r // rpg) * gs + go + r % rpg for r in range(M)]
    y = F.layer_norm(x[rows], (D,), gamma, beta, 1e-5)
    f = R.layernorm_fwd(x.detach(), gamma, beta, M, rpg, gs, go, 1e-5)
    _close(f["y"], y)
    _close(f["mean"], x.detach()[rows].mean(1))
    _close(f["rstd"], 1.0 / torch.sqrt(x.detach()[rows].var(1, unbiased=False) + 1e-5))
    dy = _rand(M + 3, D, seed=4)                                 # dense; rows past M are never read
    (gx,) = torch.autograd.grad(y, x, dy[:M])                    # zero at the rows outside the map
    dx_in = _rand(N, D, seed=5)
    sent = torch.full((N, D), 7.0, dtype=F64)
    b = R.layernorm_bwd(dy, x.detach(), f["mean"], f["rstd"], gamma, dx_in, M, rpg, gs, go, sent)
    _close(b["dx"][rows], (gx + dx_in)[rows])
    other = torch.ones(N, dtype=torch.bool)
    other[rows] = False
    assert bool((b["dx"][other] == 7.0).all()) and int(other.sum()) == N - M
    b0 = R.layernorm_bwd(dy, x.detach(), f["mean"], f["rstd"], gamma, None, M, rpg, gs, go, sent)
    _close(b0["dx"][rows], gx[rows])
    _close(b0["dense"], gx[rows])


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("B,H,L", [(1, 1, 1), (2, 3, 17), (1, 2, 70)])
def test_attention_forward_and_backward(B, H, L):
    q, k, v = (_rand(B, H, L, 64, seed=s).requires_grad_(True) for s in (1, 2, 3))
    qkv = R.pack_qkv(q.detach(), k.detach(), v.detach())
    for a, b in zip(R.split_qkv(qkv, B, L, H), (q, k, v)):
        assert torch.equal(a, b.detach())
    o = F.scaled_dot_product_attention(q, k, v)
    s = q @ k.transpose(-1, -2) / 8.0
    _close(s.softmax(-1) @ v, o)
    f = R.attention_fwd(q.detach(), k.detach(), v.detach())
    _close(f["o"], o)
    _close(f["lse"], torch.logsumexp(s, -1))
    dout = _rand(B, H, L, 64, seed=4)
    assert torch.equal(R.heads(R.unheads(dout), B, L, H), dout)
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), dout)
    b = R.attention_bwd(q.detach(), k.detach(), v.detach(), dout, f["o"], f["lse"])
    terms = float(b["dP"].abs().max() * max(q.detach().abs().max(), k.detach().abs().max()))     # L = 1: dS = dP - delta = 0
    _close(b["dq"], gq, floor=terms)
    _close(b["dk"], gk, floor=terms)
    _close(b["dv"], gv)
    _close(b["delta"], (dout * o.detach()).sum(-1))


SEL_SHAPES = [(1, 1, 1), (2, 3, 15), (2, 3, 16), (2, 3, 17), (1, 12, 128), (1, 12, 129), (2, 2, 255), (1, 2, 256),
              (1, 2, 257), (1, 2, 512), (1, 1, 768), (1, 2, 1025), (3, 100, 130), (22, 12, 197)]
SEL_EXACT_L = {1, 15, 16, 17, 128, 256, 512}           # every query's m is a power of two at these lengths


def _representable(x, dt):
    return torch.equal(x.to(dt).to(F64), x)


@pytest.mark.parametrize("B,H,L", [s for s in SEL_SHAPES if s[0] * s[1] <= 24])
def test_selection_inputs(B, H, L):
    qkv, dout, mult = R.selection_inputs(B, L, H, 5)
    q, k, v = R.split_qkv(qkv, B, L, H)
    s = q @ k.transpose(-1, -2) / 8.0
    assert set(torch.unique(s).tolist()) <= {128.0, 0.0, -128.0}
    assert bool((s.max(-1).values == 128.0).all())
    assert torch.equal((s == 128.0).sum(-1), mult) and int(mult.min()) >= 1
    # every other key is 128 log2(e) = 184.7 binades below the row maximum: under the smallest f32 denormal
    assert 128 * math.log2(math.e) > 149 + 24
    # the queries of each (crop, head) put a row maximum on every key position
    assert bool((s == 128.0).any(-2).all())
    pow2 = (mult & (mult - 1)) == 0
    assert bool(pow2.all()) == (L in SEL_EXACT_L)
    if L == 128:
        assert bool((mult == 2).all())
    for dt in DTS:
        assert _representable(qkv, dt) and _representable(dout, dt)
    # the reference with the other probabilities set to exactly 0 (what every dtype computes) against the full one
    do = R.heads(dout, B, L, H)
    ex = R.selection_reference(q, k, v, do, mult)
    o, p, dS, delta = ex["o"], ex["P"], ex["dS"], ex["delta"]
    f = R.attention_fwd(q, k, v)
    _close(f["o"], o, 1e-15)
    _close(f["lse"], ex["lse"], 1e-15)
    b = R.attention_bwd(q, k, v, do, o, ex["lse"])
    for key in ("dq", "dk", "dv"):
        _close(b[key], ex[key], 1e-12, floor=1.0)
    if L == 128:
        assert float(dS.abs().max()) > 0                             # m = 2: the dQ / dK checks are not vacuous
        assert float(ex["dq"].abs().max()) > 0 and float(ex["dk"].abs().max()) > 0
    if L in SEL_EXACT_L:
        # exactly representable: out, P, dS (the 16-bit MFMA operands) and the three gradients in every dtype
        for dt in DTS:
            for t in (o, p, dS, ex["dq"], ex["dk"], ex["dv"]):
                assert _representable(t, dt)
        # and every product and partial sum of the kernel's f32 accumulations is an integer multiple of 2^-12 below 2^12
        for t in (o, dS, ex["dq"] * 8, ex["dk"] * 8, ex["dv"], delta):
            assert torch.equal(t * 4096, (t * 4096).round()) and float(t.abs().max()) < 4096


DRIFT = [(L, kind) for L in (229, 513, 768, 1025) for kind in ("rising", "falling", "peak")]


@pytest.mark.parametrize("L,kind", DRIFT)
def test_drift_inputs(L, kind):
    """No overflow (inputs inside the f16 range, scores far inside f32), and at least two probabilities above 2^-10
    in every row, for the inputs as each dtype rounds them."""
    B, H = 1, 2
    q0, k0, v0 = R.drift_inputs(B, L, H, kind, 9)
    for dt in DTS:
        q, k, v = (R.rounded(t, dt) for t in (q0, k0, v0))
        assert max(float(t.abs().max()) for t in (q, k, v)) < 65504 / 256
        f = R.attention_fwd(q, k, v)
        assert float(f["s"].abs().max()) < 1000 and bool(torch.isfinite(f["o"]).all())
        p = f["p"] / f["l"]
        top2 = p.topk(2, -1).values[..., 1]
        assert float(top2.min()) > 2.0 ** -10, float(top2.min())
        m = f["s"].max(-1)
        blk = 256 if L > 256 else 64
        if kind == "rising":
            assert bool((m.indices // blk == (L - 1) // blk).all()) or L - (L - 1) // blk * blk < 16
            cm = torch.stack([f["s"][..., c * blk:(c + 1) * blk].max(-1).values for c in range(-(-L // blk))], -1)
            assert bool((cm[..., 1:] > cm[..., :-1]).all())           # every chunk raises the running maximum
        elif kind == "falling":
            assert bool((m.indices < blk).all())
        else:
            assert bool((m.indices >= 16 * ((L - 1) // 16)).all())    # the dominant key is in the last partial tile
            assert float(p.max(-1).values.min()) > 0.5


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("embed,NB,B,HW", [(512, 5, 2, 3), (1024, 16, 1, 5), (512, 1, 2, 1)])
def test_head_forward_and_backward(embed, NB, B, HW):
    P = B * HW
    Z = _rand(P, embed, seed=1)
    Z[1] *= 1e-3 / float(Z[1].norm())                            # a row of norm 1e-3
    text = _rand(NB, embed, seed=2)
    ls = torch.tensor([2.3], dtype=F64)
    anchors = torch.arange(NB, dtype=F64) * 0.9
    dl, de = _rand(B, NB, HW, seed=3), _rand(B, HW, seed=4)
    gs = 0.625
    Zr, lsr = Z.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    # the expression of test_head_bwd_dz_dtypes
    zn = F.normalize(Zr, dim=-1)
    tn = F.normalize(text, dim=-1)
    logits = (lsr.exp() * zn @ tn.t()).view(B, HW, NB).permute(0, 2, 1)
    exp = (logits.softmax(1) * anchors.view(1, -1, 1)).sum(1)
    gz, gls = torch.autograd.grad((logits * dl * gs).sum() + (exp * de * gs).sum(), (Zr, lsr))
    r = R.head_bwd(Z, text, ls, anchors, dl, de, gs, B, HW)
    _close(r["logits"], logits)
    _close(r["exp"], exp)
    _close(r["dz"], gz)
    _close(r["dbias"], gz.sum(0))
    _close(r["dscale"], gls)


def test_head_zero_row_takes_the_clamp():
    """A zero row of Z: F.normalize divides by the clamp 1e-12, its backward is dzn / 1e-12 (no projection term)."""
    embed, NB, B, HW = 512, 5, 1, 3
    Z = _rand(3, embed, seed=1)
    Z[2] = 0
    text = _rand(NB, embed, seed=2)
    ls = torch.tensor([1.0], dtype=F64)
    anchors = torch.arange(NB, dtype=F64)
    dl, de = _rand(B, NB, HW, seed=3), _rand(B, HW, seed=4)
    Zr = Z.clone().requires_grad_(True)
    logits = (ls.exp() * F.normalize(Zr, dim=-1) @ F.normalize(text, dim=-1).t()).view(B, HW, NB).permute(0, 2, 1)
    exp = (logits.softmax(1) * anchors.view(1, -1, 1)).sum(1)
    (gz,) = torch.autograd.grad((logits * dl).sum() + (exp * de).sum(), Zr)
    r = R.head_bwd(Z, text, ls, anchors, dl, de, 1.0, B, HW)
    _close(r["dz"], gz)
    assert torch.equal(r["dz"][2], r["dzn"][2] / 1e-12) and float(r["dz"][2].abs().max()) > 1e9
    assert bool((r["logits"][0, :, 2] == 0).all())
