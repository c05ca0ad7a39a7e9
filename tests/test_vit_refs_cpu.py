"""tests/_vit_refs.py pinned on the CPU: the workspace mirror against ebc_vit_workspace_bytes_p (host only, no device),
the case list against ebc_gemm_tile_config, the fold identities and the stage chain against torch's own float64 ops and
autograd, and every bound shown tight enough to catch the faults the per-stage GPU module exists for: a workspace is
built by `simulate` (every stage's reference rounded once to its storage type), must pass the same walker
tests/test_gpu_vit_stages.py runs, and must fail it after each seeded corruption."""
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import _gemm_refs as GR
import _vit_refs as V
from conftest import REPO, rel_l2

F64 = torch.float64
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f32": 0, "f16": 1, "bf16": 2}


@pytest.fixture(scope="module")
def lib():
    from ebc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "clip-ebc_amd")])
    return _lib.load()


# ------------------------------------------------------------------------------------------------ mirror and cases
@pytest.mark.parametrize("name", list(V.CASES))
def test_workspace_mirror_matches_library(lib, name):
    """The mirror's total is the library's for every case, type and mode (and for one layer, the backward cases)."""
    patch, H, W, NV, B, layers, G, L, M = V.case_dims(name)
    for dname, code in CODE.items():
        parts = V.part_counts(lib, code, M)
        for nl in {layers, 1}:
            for training in (0, 1):
                _, total = V.carve(B, L, G, 3 * patch * patch, nl, 4 if code == 0 else 2, training, *parts)
                assert total == lib.ebc_vit_workspace_bytes_p(B, H, W, patch, nl, NV, code, training), (dname, nl, training)
                assert total % 256 == 0


def test_workspace_mirror_offsets_are_disjoint_and_alias_only_in_eval():
    lay, total = V.carve(2, 8, 4, 3072, 3, 2, 1, 16, 16, 96)
    offs = lay["X"] + [v for s in lay["layer"] for v in s.values()] + [v for k, v in lay.items()
                                                                         if k not in ("X", "layer") and v is not None]
    assert len(set(offs)) == len(offs) and all(o % 256 == 0 and o < total for o in offs)
    assert lay["bpart"] is None and lay["rpart"] is not None
    ev, tev = V.carve(2, 8, 4, 3072, 3, 2, 0, 16, 16, 96)
    assert ev["X"][2] == ev["X"][0] and ev["X"][3] == ev["X"][1] and ev["layer"][2] is ev["layer"][0] and tev < total
    assert ev["dXa"] is None and ev["vpt_rows"] is None and ev["bpart"] is None


def test_case_list_reaches_every_tile_and_fold_class(lib):
    """The tiles the issue's table names, from the library's own dispatch; both values of fold_b; the fold limits."""
    for name, want in V.TILES16.items():
        M = V.case_dims(name)[-1]
        for code in (1, 2):
            assert V.case_tiles(lib, code, name) == want, (name, V.case_tiles(lib, code, name))
            po, pp, pg = V.part_counts(lib, code, M)
            assert po == pp == 16 <= V.LN_PMAX                     # the forward fold is on in every case
        assert set(V.case_tiles(lib, 0, name)) == {2} and V.part_counts(lib, 0, M) == (0, 0, 0)
    fb = {n: V.fold_b_taken(lib, 1, V.case_dims(n)[-1]) for n in V.CASES}
    assert fb == {"tiny": False, "tiny_nv0": False, "ragged135": False, "ragged261": False, "fold_b_low": True,
                  "fold_b_high": True, "many_tiles": False, "patch16": False, "L229": False}
    assert V.part_counts(lib, 1, V.case_dims("tiny")[-1])[2] == 96 and V.part_counts(lib, 1, 1360)[2] == 32
    assert V.part_counts(lib, 1, 4104)[2] == 32 and V.tile_of(lib, 1, 4104, 768, 3072)[0] == 5   # off by fold_pays
    assert not V.fold_b_taken(lib, 1, 1344) and V.fold_b_taken(lib, 1, 1352) and V.fold_b_taken(lib, 1, 4096)
    assert not V.fold_b_taken(lib, 1, 1360, V.FLAG_NO_LN_FOLD)
    # ragged cases: a partial second / third row tile with a prompt row on each side of the 128-row edge
    for name, edge in (("ragged135", 128), ("ragged261", 256)):
        patch, H, W, NV, B, layers, G, L, M = V.case_dims(name)
        assert edge < M < edge + 128 and 1 <= (edge - 1) % L <= NV and 1 <= edge % L <= NV


def test_row_maps_agree():
    """The prompt rows (r % L in 1..NV) are _gemm_refs.row_map(B * NV, NV, L, 1): the trimmed backward's A rows."""
    for B, L, NV in ((2, 8, 3), (15, 9, 4), (1, 229, 32)):
        assert torch.equal(V.prompt_rows(B, L, NV), GR.row_map(B * NV, NV, L, 1))
    assert V.prompt_rows(2, 5, 0).numel() == 0


def test_binade_aware_rounding_term():
    """A reference just below a power of two whose computed value lands above it: the stored bf16 value is on a
    spacing twice ulp_T(ref).  Figures of the attention backward's dK as measured (see test_gpu_vit_stages.py): err
    2.03 ulp against a bound of 1.97 ulp, d = 1.47 ulp.  Elsewhere the bound is unchanged."""
    bf = torch.bfloat16
    ref = torch.tensor([3.124604852e-02, 1.0e-02], dtype=F64)
    got = torch.tensor([3.149414062e-02, 1.0e-02], dtype=F64)
    u = GR.ulp(ref, bf)
    assert float(u[0]) == 2.0 ** -13 and float(GR.ulp(got[:1], bf)) == 2.0 ** -12
    bound = 0.5 * u + torch.tensor([1.4666, 1.4666], dtype=F64) * u
    err = (got - ref).abs()
    assert float(err[0] / bound[0]) > 1.0
    fixed = V.binade_aware(ref, bound, bf)
    assert float(fixed[0]) == float(bound[0] + 0.5 * u[0]) and float(err[0] / fixed[0]) < 1.0
    assert float(fixed[1]) == float(bound[1])


# ------------------------------------------------------------------------------------------------ fold identities
def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def test_fold_forward_identity_f64():
    """rstd (x W'^T - mean s) + b' is linear(layer_norm(x)) when W' = W diag(gamma) exactly."""
    M, N = 7, 192
    x = (_rand((M, 768), 1) + 3.0).to(torch.float32)
    W, b = _rand((N, 768), 2, 768 ** -0.5), _rand((N,), 3, 0.02)
    g, be = 1 + _rand((768,), 4, 0.05), _rand((768,), 5, 0.05)
    want = F.linear(F.layer_norm(x.to(F64), (768,), g, be, V.EPS), W, b)
    mean, var, rstd = V.stats64(x)
    Wf = W * g[None, :]
    out = V.ln_fold_product(x, mean, rstd, Wf, Wf.sum(1), b + W @ be, torch.float32)
    assert float((out["C"][0] - want).abs().max()) < 1e-12
    out = V.ln_fold_product(x, mean, rstd, Wf, Wf.sum(1), b + W @ be, torch.float32, gelu=True)
    assert float((out["aux"][0] - want).abs().max()) < 1e-12
    assert float((out["C"][0] - want * torch.sigmoid(1.702 * want)).abs().max()) < 1e-12
    # the partials restate the same statistics
    m2, r2 = V.stats_from_partials(V.fold_partials(x, 96))
    assert float((m2 - mean).abs().max()) < 1e-12 and float((r2 / rstd - 1).abs().max()) < 1e-9


def test_fold_backward_identity_f64():
    """EPI_LN_BWD's expression with the two partial sums is autograd's LayerNorm backward of dA . W_fc'."""
    M = 5
    x = (_rand((M, 768), 1) * 2 + 1.0).to(torch.float32).to(F64).requires_grad_(True)
    W, b = _rand((3072, 768), 2, 768 ** -0.5), _rand((3072,), 3, 0.02)
    g, be = 1 + _rand((768,), 4, 0.05), _rand((768,), 5, 0.05)
    dA, dX = _rand((M, 3072), 6).to(torch.float32).to(F64), _rand((M, 768), 7).to(torch.float32).to(F64)
    A = F.linear(F.layer_norm(x, (768,), g, be, V.EPS), W, b)
    (A * dA).sum().backward()
    want = x.grad + dX
    mean, var, rstd = V.stats64(x.detach())
    Wf = W * g[None, :]
    s, c = Wf.sum(1), b + W @ be
    bp, _ = V.bpart_ref(dA, A.detach(), s, c, 192, torch.float32)
    assert bp.shape == (M, 32, 2)
    out = V.ln_bwd_fold(dA, Wf.t().contiguous(), bp, x.detach(), mean, rstd, dX, torch.float32)
    assert float((out["dX1"][0] - want).abs().max()) < 1e-10
    # ... and the unfolded restatement is the same backward
    dH = dA @ W
    ref, _ = V.ln_bwd(dH, x.detach(), mean, rstd, g, dX)
    assert float((ref - want).abs().max()) < 1e-10


@pytest.mark.parametrize("dname", ["f16", "bf16"])
def test_encoder_cache_folded_operands(dname):
    """_EncoderCache's own folded operands (built on the CPU): W' = rn_T(W diag(gamma)), s = rowsum(W') in f32,
    b' = b + W beta, (W')^T; with them both identities hold up to the rounding of W'."""
    from ebc_amd.model import _EncoderCache
    dt = DT[dname]
    enc = V.make_encoder("tiny", layers=1)
    cache = _EncoderCache(enc, 3, dt, torch.device("cpu"))
    P = V.params_from_cache(cache, 2, 2)
    p, blk = P["layers"][0], enc.transformer.resblocks[0]
    for pre, w, bias, ln in (("qkv", blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.ln_1),
                             ("fc", blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, blk.ln_2)):
        w64, g, be = w.to(F64), ln.weight.to(F64), ln.bias.to(F64)
        Wf = p[f"w_{pre}_ln"]
        assert Wf.dtype == dt and torch.equal(Wf, (w64 * g[None, :]).to(dt))
        assert torch.equal(p[f"s_{pre}_ln"], Wf.to(F64).sum(1).to(torch.float32))
        assert torch.equal(p[f"b_{pre}_ln"], (bias.to(F64) + w64 @ be).to(torch.float32))
        x = (_rand((6, 768), 11) + 0.5).to(torch.float32)
        mean, var, rstd = V.stats64(x)
        got = V.ln_fold_product(x, mean, rstd, Wf, p[f"s_{pre}_ln"], p[f"b_{pre}_ln"], torch.float32)["C"][0]
        want = F.linear(F.layer_norm(x.to(F64), (768,), g, be, V.EPS), w64, bias.to(F64))
        xh = ((x.to(F64) - mean[:, None]) * rstd[:, None]).abs()
        slack = xh @ (Wf.to(F64) - w64 * g[None, :]).abs().t() + 1e-6 * (1 + want.abs())
        assert bool(((got - want).abs() <= slack).all())
    assert torch.equal(p["wt_fc_ln"], p["w_fc_ln"].t()) and p["wt_fc_ln"].is_contiguous()
    assert p["wt_qkv_ln"] is None                           # the struct's slot is not filled by the model
    f32 = _EncoderCache(enc, 3, torch.float32, torch.device("cpu"))
    assert V.params_from_cache(f32, 2, 2)["layers"][0]["w_fc_ln"] is None
    assert V.params_from_cache(_EncoderCache(enc, 3, dt, torch.device("cpu"), ln_fold=False), 2, 2)["layers"][0]["s_fc_ln"] is None


# ------------------------------------------------------------------------------------------------ the stage chain
def _quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def plain_vit(enc, image, vpts, NV, patch):
    """A plain float64 CLIP ViT with deep / shallow VPT insertion: conv1, cls + pos, ln_pre, per block the prompt rows
    replaced, x + out_proj(softmax(q k^T / 8) v), x + c_proj(QuickGELU(c_fc(ln_2 x))), ln_post on the patch rows."""
    enc = enc.double()
    B = image.shape[0]
    x = F.conv2d(image.to(F64), enc.conv1.weight, stride=patch).flatten(2).transpose(1, 2)          # [B][G][768]
    x = torch.cat([enc.class_embedding.expand(B, 1, -1), x], 1) + enc.positional_embedding
    x = enc.ln_pre(x)
    for l, blk in enumerate(enc.transformer.resblocks):
        if NV and vpts[l] is not None:
            v = vpts[l].to(F64)
            v = v if v.dim() == 3 else v.expand(B, -1, -1)
            x = torch.cat([x[:, :1], v, x[:, 1:] if l == 0 else x[:, 1 + NV:]], 1)
        h = blk.ln_1(x)
        L = x.shape[1]
        qkv = F.linear(h, blk.attn.in_proj_weight, blk.attn.in_proj_bias).view(B, L, 3, 12, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / 8.0, -1) @ qkv[2]
        x = x + blk.attn.out_proj(a.permute(0, 2, 1, 3).reshape(B, L, 768))
        x = x + blk.mlp.c_proj(_quick_gelu(blk.mlp.c_fc(blk.ln_2(x))))
    return enc.ln_post(x[:, 1 + NV:])


def _simulated(name, dname, mode, per_crop, fold, layers=None, training=True, parts=None, stats="benign"):
    from ebc_amd.model import _EncoderCache
    dt = DT[dname]
    patch, H, W, NV, B, nl, G, L, M = V.case_dims(name)
    nl = layers or nl
    enc = V.make_encoder(name, stats, nl)
    cache = _EncoderCache(enc, NV, dt, torch.device("cpu"), ln_fold=fold)
    P = V.params_from_cache(cache, H // patch, W // patch)
    image, vpts, bstride = V.make_inputs(name, mode, per_crop, nl, stats=stats)
    parts = parts or ((0, 0, 0) if dt == torch.float32 else (16, 16, 96))
    _, total = V.carve(B, L, G, 3 * patch * patch, nl, 4 if dt == torch.float32 else 2, training, *parts)
    ws = V.Workspace(torch.zeros(total, dtype=torch.uint8), B, L, G, 3 * patch * patch, nl, dt, training, parts)
    feat = torch.zeros(B, G, 768, dtype=torch.float32)
    fold = fold and dt != torch.float32
    V.walk_forward(V.Walk("simulate"), ws, P, image, vpts, bstride, feat, fold, training)
    return dict(enc=enc, cache=cache, P=P, image=image, vpts=vpts, bstride=bstride, ws=ws, feat=feat, fold=fold, dims=(
        patch, H, W, NV, B, nl, G, L, M), dt=dt)


class Ratios(dict):
    def __call__(self, name, err, bound):
        self[name] = float((err / bound).max())

    def worst(self):
        return max(self.items(), key=lambda kv: kv[1] if kv[1] == kv[1] else float("inf"))


def _check_fwd(s, training=True):
    r = Ratios()
    V.walk_forward(V.Walk("check", r, "sim"), s["ws"], s["P"], s["image"], s["vpts"], s["bstride"], s["feat"], s["fold"],
                   training)
    return r


@pytest.mark.parametrize("mode,per_crop", [("deep", True), ("deep", False), ("shallow", False)])
def test_forward_chain_is_a_plain_vit(mode, per_crop):
    """The stage references chained in f32 storage (no fold: f32 has none) reproduce the plain float64 ViT."""
    s = _simulated("tiny", "f32", mode, per_crop, fold=False)
    patch, H, W, NV = s["dims"][:4]
    want = plain_vit(s["enc"], s["image"], s["vpts"], NV, patch)
    assert rel_l2(s["feat"], want) < 1e-5
    r = _check_fwd(s)
    assert r.worst()[1] <= 1.0, r.worst()


def test_forward_chain_no_prompts_and_patch16():
    for name, mode in (("tiny_nv0", "none"), ("patch16", "deep")):
        s = _simulated(name, "f32", mode, False, fold=False)
        want = plain_vit(s["enc"], s["image"], s["vpts"], s["dims"][3], s["dims"][0])
        assert rel_l2(s["feat"], want) < 1e-5


@pytest.mark.parametrize("dname", ["f16", "bf16"])
@pytest.mark.parametrize("fold", [True, False])
def test_simulated_16bit_workspace_passes_and_tracks_the_plain_vit(dname, fold):
    """16-bit storage, folded and unfolded: the walker passes on its own simulation (every ratio <= 1: a rounding alone
    never exceeds a bound) and the result stays a ViT (16-bit activations: rel_l2 of a few 1e-3)."""
    s = _simulated("tiny", dname, "deep", True, fold)
    want = plain_vit(s["enc"], s["image"], s["vpts"], 3, 32)
    err = rel_l2(s["feat"], want)
    print(f"rel_l2 simulated[{dname},fold={fold}] {err:.2e}")
    assert err < (4e-3 if dname == "f16" else 3e-2)
    r = _check_fwd(s)
    assert r.worst()[1] <= 1.0, r.worst()
    assert (any(k.endswith("l1.QKV") for k in r) and "sim.feat" in r and "sim.l2.G" in r)


def test_simulated_eval_workspace_gives_the_training_feat():
    """training = 0: X ping-pongs, every layer shares LayerSave 0; the walker on the aliased mirror gives the training
    workspace's feat (to 16-bit rounding: the simulation's c_proj reads the stored G there, gelu of the stored A here;
    the kernels read the same unrounded value in both modes), and an eval check covers the last stage."""
    a = _simulated("tiny", "bf16", "deep", True, True)
    b = _simulated("tiny", "bf16", "deep", True, True, training=False)
    assert b["ws"].total < a["ws"].total and rel_l2(b["feat"], a["feat"]) < 1e-2
    r = _check_fwd(b, training=False)
    assert set(r) == {"sim.ln_post.mean", "sim.ln_post.rstd", "sim.feat"} and r.worst()[1] <= 1.0


# ------------------------------------------------------------------------------------------------ backward chain
def _simulated_bwd(mode, per_crop, dname, flags, fold_b, name="tiny"):
    parts = None if dname == "f32" else (16, 16, 32 if fold_b else 96)
    s = _simulated(name, dname, mode, per_crop, fold=True, layers=1, parts=parts)
    patch, H, W, NV, B, nl, G, L, M = s["dims"]
    s["dfeat"] = V.make_dfeat(name)
    s["dvpt"] = [torch.zeros_like(v) if v is not None else None for v in s["vpts"]]
    s["flags"], s["fold_b"] = flags, fold_b
    V.walk_backward(V.Walk("simulate"), s["ws"], s["P"], s["dfeat"], s["dvpt"], s["bstride"], flags, fold_b)
    return s


def _check_bwd(s):
    r = Ratios()
    V.walk_backward(V.Walk("check", r, "sim"), s["ws"], s["P"], s["dfeat"], s["dvpt"], s["bstride"], s["flags"], s["fold_b"])
    return r


@pytest.mark.parametrize("per_crop", [True, False])
@pytest.mark.parametrize("flags", [0, V.FLAG_FULL_LAYER0])
def test_backward_chain_is_autograd(per_crop, flags):
    """The backward stage references chained in f32 storage give autograd's prompt gradient of the plain ViT, through
    the trimmed layer-0 path and through the full one, per crop and shared."""
    s = _simulated_bwd("deep", per_crop, "f32", flags, False)
    v = s["vpts"][0].to(F64).requires_grad_(True)
    out = plain_vit(s["enc"], s["image"], [v], 3, 32)
    (out * s["dfeat"].to(F64)).sum().backward()
    assert rel_l2(s["dvpt"][0], v.grad) < 1e-5
    r = _check_bwd(s)
    assert r.worst()[1] <= 1.0, r.worst()
    assert ("sim.dvpt" in r) == (not per_crop) and ("sim.dX_L" in r) == (flags == 0) and ("sim.dX0" in r) == (flags != 0)


@pytest.mark.parametrize("dname", ["f16", "bf16"])
@pytest.mark.parametrize("fold_b", [True, False])
def test_simulated_16bit_backward_passes(dname, fold_b):
    for flags in (0, V.FLAG_FULL_LAYER0):
        s = _simulated_bwd("deep", False, dname, flags, fold_b)
        v = s["vpts"][0].to(F64).requires_grad_(True)
        (plain_vit(s["enc"], s["image"], [v], 3, 32) * s["dfeat"].to(F64)).sum().backward()
        err = rel_l2(s["dvpt"][0], v.grad)
        print(f"rel_l2 simulated dvpt[{dname},fold_b={fold_b},flags={flags}] {err:.2e}")
        assert err < (1e-2 if dname == "f16" else 8e-2)
        r = _check_bwd(s)
        assert r.worst()[1] <= 1.0, r.worst()
        assert ("sim.bpart" in r) == (fold_b and flags == 0)


# ------------------------------------------------------------------------------------------------ corruptions
def _fails_at(r, *names):
    bad = {k for k, v in r.items() if not v <= 1.0}
    assert bad and bad <= set(names), (bad, names)
    return max(r[k] for k in bad)


def _requantised_qkv(s, l, mean, rstd):
    """QKV_l as EPI_LN leaves it from the given statistics."""
    p = s["P"]["layers"][l]
    ref = V.ln_fold_product(s["ws"].get("X", l), mean, rstd, p["w_qkv_ln"], p["s_qkv_ln"], p["b_qkv_ln"], s["dt"])["C"][0]
    return ref.to(s["dt"])


@pytest.mark.parametrize("kind", ["dropped_pair", "neighbour_wave_column", "mean_of_next_row"])
@pytest.mark.parametrize("dname", ["f16", "bf16"])
def test_statistics_corruptions_fail(dname, kind):
    """Row statistics rebuilt wrongly for one row of layer 1 (one of the 16 partial pairs dropped; one pair taken from
    the neighbouring wave column; the last row of the ragged tile given the next row's mean -- M = 16, so row 15 reads
    what the clamp min(., M - 1) would keep in range, row 14 is given row 15's): the row's QKV follows the wrong
    statistics, as the kernel's would.  rel_l2 of QKV_1 is printed (below 5e-3 where the statistic barely moves)."""
    s = _simulated("tiny", dname, "deep", True, True)
    ws, l = s["ws"], 1
    clean = ws.get("QKV", l).clone()
    parts = V.fold_partials(ws.get("X", l), 96)
    assert parts.shape[1] == 16
    for row in range(ws.M):
        ws.get("QKV", l).copy_(clean)
        m0, r0 = ws.get("m1", l).clone(), ws.get("r1", l).clone()
        pc = parts.clone()
        if kind == "dropped_pair":
            pc[row, 5] = 0.0
        elif kind == "neighbour_wave_column":
            pc[row, 4] = parts[row, 5]
        mean, rstd = V.stats_from_partials(pc)
        if kind == "mean_of_next_row":
            if row == ws.M - 1:
                continue
            mean[row] = mean[row + 1]
        assert float(parts[row, 5, 0]) != 0.0 and float(parts[row, 4, 0]) != float(parts[row, 5, 0])   # nothing skipped
        ws.get("m1", l)[row], ws.get("r1", l)[row] = mean[row].float(), rstd[row].float()
        ws.get("QKV", l)[row] = _requantised_qkv(s, l, ws.get("m1", l), ws.get("r1", l))[row]
        r = _check_fwd(s)
        worst = _fails_at(r, f"sim.l{l}.ln1.mean", f"sim.l{l}.ln1.rstd")
        if row == 0:
            print(f"rel_l2 {kind}[{dname}] QKV_1 {rel_l2(ws.get('QKV', l), clean):.2e} ratio {worst:.0f}")
        ws.get("m1", l).copy_(m0)
        ws.get("r1", l).copy_(r0)
    ws.get("QKV", l).copy_(clean)
    assert _check_fwd(s).worst()[1] <= 1.0


@pytest.mark.parametrize("fold", [True, False])
def test_prompt_row_from_the_next_crop_fails(fold):
    """One prompt row of one crop of X_1 taken from crop b + 1 (and everything computed from it consistent)."""
    s = _simulated("tiny", "bf16", "deep", True, fold)
    ws = s["ws"]
    row = 1 * ws.L + 2                                                        # crop 1, prompt row 1 -> crop 0's
    clean = s["feat"].clone()
    s["vpts"][1] = s["vpts"][1].clone()
    good = s["vpts"][1].clone()
    s["vpts"][1][1, 1] = good[0, 1]
    feat = torch.zeros_like(clean)
    V.walk_forward(V.Walk("simulate"), ws, s["P"], s["image"], s["vpts"], s["bstride"], feat, s["fold"])
    print(f"rel_l2 prompt_row_from_next_crop feat {rel_l2(feat, clean):.2e}")
    s["vpts"][1], s["feat"] = good, feat
    assert not torch.equal(ws.get("X", 1)[row], good[1, 1])
    with pytest.raises(AssertionError, match="prompt_rows"):
        _check_fwd(s)


def test_unreplaced_prompt_row_fails():
    """The folded c_proj epilogue leaving one prompt row of X_1 as the product's own output."""
    s = _simulated("tiny", "bf16", "deep", True, True)
    ws = s["ws"]
    p = s["P"]["layers"][0]
    ref, _, _ = V.mlp_out(ws.get("A", 0), ws.get("X1", 0), p["w_proj"], p["b_proj"], s["dt"])
    ws.get("X", 1)[3] = ref[3].float()
    with pytest.raises(AssertionError, match="prompt_rows"):
        _check_fwd(s)


@pytest.mark.parametrize("dname", ["f16", "bf16"])
def test_bpart_and_vpt_sum_corruptions_fail(dname):
    """One bpart pair swapped with its neighbour (every patch row in turn: with one layer, dX_L and with it dA and the
    partials of the CLS and prompt rows are zeros by construction, so a swap changes nothing there; no patch row is
    skipped); vpt_sum missing one crop."""
    s = _simulated_bwd("deep", False, dname, 0, True)
    ws = s["ws"]
    assert _check_bwd(s).worst()[1] <= 1.0
    bp = ws.get("bpart")
    clean = bp.clone()
    patch_rows = [r for r in range(ws.M) if r % ws.L > ws.NV]
    assert len(patch_rows) == ws.B * ws.G and not bool(clean[V.prompt_rows(ws.B, ws.L, ws.NV)].any())
    for row in patch_rows:
        assert not torch.equal(clean[row, 6], clean[row, 7])
        bp[row, 6], bp[row, 7] = clean[row, 7], clean[row, 6]
        r = _check_bwd(s)
        # (the sums S1, S2 do not change: only the per-pair check can see it)
        _fails_at(r, "sim.bpart")
        bp.copy_(clean)
    good = s["dvpt"][0].clone()
    rows = ws.get("vpt_rows")[0].to(F64)
    s["dvpt"][0].copy_((rows.sum(0) - rows[1]).float())
    print(f"rel_l2 vpt_sum_missing_crop[{dname}] {rel_l2(s['dvpt'][0], good):.2e}")
    _fails_at(_check_bwd(s), "sim.dvpt")
    s["dvpt"][0].copy_(good)
    # dyadic per-crop rows: the crop-order sum is exact
    d = torch.randint(-64, 65, rows.shape, generator=torch.Generator().manual_seed(3)).to(F64) / 16
    ref, bound = V.vpt_sum(d)
    assert torch.equal(ref.float().to(F64), ref) and torch.equal(ref, d[0] + d[1])
