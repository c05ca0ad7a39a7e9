"""GPU end-to-end checks of more than 16 bins through get_model: the reference's 20-bin reduction-32 table
(configs/reduction_32.json, truncation 19, qnrf, fine) on clip_vit_b_32 against the reference's own run
(tests/golden/f13_b32_r32_bins20.npz, written by tests/golden/make_golden_bins20.py) with a frozen text tower, a
trainable torch tower and a trainable HIP tower (20 prompts: two library calls of 16 and 4); the same table on
clip_resnet50 (the width-1024 head) and 17 bins on clip_vit_b_16 against the oracle.

Bars: tests/test_gpu_vit_b32.py (fp32 train step, eval, autocast), tests/test_gpu_text_train.py /
tests/test_gpu_text_tower_train.py (the trainable tower), tests/test_gpu_text_tower.py (the HIP tower's features),
tests/test_gpu_resnet.py (clip_resnet50), unchanged."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_vit_b32 as V
from conftest import golden, rel_l2, rel_max
from ebc_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F64 = torch.float64
FIX = "f13_b32_r32_bins20.npz"


def _table(d):
    return [(float(lo), float(hi)) for lo, hi in d["bins"]], [float(a) for a in d["anchors"]]


def _b32(d, **kw):
    from ebc_amd.model import get_model
    bins, anchors = _table(d)
    m = get_model("clip_vit_b_32", int(d["input_size"]), int(d["reduction"]), bins, anchors, prompt_type="word",
                  vit_layers=int(d["layers"]), weights_seed=int(d["weights_seed"]), **kw)
    return m.cuda(), bins


def _step(m, d, bins, pre="", autocast=None):
    """One training step on the fixture's crops: logits, exp, the loss terms, d loss / d text_features (if trainable)."""
    from ebc_amd.losses import DACELoss
    size, red = int(d["input_size"]), int(d["reduction"])
    img, pts, dens = syn.synthetic_crops(int(d[pre + "batch"]), size, seed=int(d[pre + "seed"]), counts=list(d[pre + "counts"]))
    m.train()
    m.zero_grad(set_to_none=True)
    kept = {}

    def hook(mod, inp, out):
        if out.requires_grad:
            out.register_hook(lambda g: kept.__setitem__("grad_text", g.detach().float().cpu().numpy()))
    h = m.text_encoder.register_forward_hook(hook)
    loss_fn = DACELoss(bins, red, weight_count_loss=1.0, count_loss="dmcount", input_size=size)
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        logits, exp = m(torch.from_numpy(img).cuda())
        loss, info = loss_fn(logits, exp, torch.from_numpy(dens).cuda(), [torch.from_numpy(p).cuda() for p in pts])
    h.remove()
    loss.backward()
    torch.cuda.synchronize()
    return (img, logits.detach().float().cpu().numpy(), exp.detach().float().cpu().numpy(),
            {k: float(v) for k, v in info.items()}, kept.get("grad_text"))


def _check_fp32_step(m, d, pre, logits, exp, info):
    """test_gpu_vit_b32.py::test_b32_train_step_fp32_matches_reference's assertions on the keys both cases store."""
    L = int(d["layers"])
    want = d[pre + "logits"]
    assert logits.shape == want.shape == (int(d[pre + "batch"]), 20, 7, 7)
    per_patch = V._per_patch(logits, want)
    print(f"per-patch logits rel err: max {per_patch.max():.2e} median {np.median(per_patch):.2e}")
    assert per_patch.max() < 1e-3
    assert rel_max(logits, want) < 1e-3
    ok, frac = V._argmax_ok(logits, want, 1e-3)
    assert ok and frac > 0.9
    assert rel_max(exp, d[pre + "exp"]) < 1e-3
    for k in ("loss", "tv_loss", "count_loss", "ce_loss"):
        assert abs(info[k] - float(d[pre + "info_" + k])) <= 1e-3 * abs(float(d[pre + "info_" + k])), k
    gv = np.stack([getattr(m, f"vpt_{i}").grad.cpu().numpy() for i in range(L)])
    e_v = rel_l2(gv[:, :, ::4], d[pre + "grad_vpt_sub"])
    print(f"prompt gradients rel-L2 {e_v:.2e}")
    assert e_v < 5e-3
    np.testing.assert_allclose(np.linalg.norm(gv, axis=(1, 2)), d[pre + "grad_vpt_norm"], rtol=5e-3)
    assert abs(float(m.logit_scale.grad) - float(d[pre + "grad_logit_scale"])) < 1e-3 * abs(float(d[pre + "grad_logit_scale"]))


# ----------------------------------------------------------------------------- clip_vit_b_32, frozen text
def test_bins20_train_step_and_eval_fp32_match_reference():
    d = golden(FIX)
    m, bins = _b32(d, text_features=torch.from_numpy(d["text_features"]))
    img, logits, exp, info, gtext = _step(m, d, bins)
    assert gtext is None
    _check_fp32_step(m, d, "", logits, exp, info)
    dec = m.image_decoder[0]
    errs = {"projection": rel_l2(m.projection.weight.grad.cpu().numpy()[::4, ::4], d["grad_proj_w_sub"]),
            "conv1": rel_l2(dec.conv1.weight.grad.cpu().numpy()[::12, ::12], d["grad_dec_conv1_sub"]),
            "conv2": rel_l2(dec.conv2.weight.grad.cpu().numpy()[::16, ::16], d["grad_dec_conv2_sub"])}
    print(f"gradient rel-L2 {errs}")
    for k, e in errs.items():
        assert e < 5e-3, (k, e)
    m.eval()                                      # the fixture's eval ran after the train step (BN running stats)
    with torch.no_grad():
        ev = m(torch.from_numpy(img).cuda()).cpu().numpy()
    assert ev.shape == d["exp_eval"].shape and rel_max(ev, d["exp_eval"]) < 1e-3


def test_bins20_own_text_features_match_the_references():
    """Without text_features=: the frozen features of the 20 prompts from the model's own (torch) tower, 12 layers."""
    d = golden(FIX)
    m, _ = _b32(d)
    assert rel_l2(m.text_features, d["text_features"]) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_bins20_train_step_autocast_vs_reference_fp32(dtype):
    """Tolerances of test_gpu_vit_b32.py::test_b32_train_step_autocast_vs_reference_fp32."""
    d = golden(FIX)
    L = int(d["layers"])
    m, bins = _b32(d, text_features=torch.from_numpy(d["text_features"]))
    _, logits, exp, info, _ = _step(m, d, bins, autocast=dtype)
    tol = 2e-2 if dtype == torch.float16 else 6e-2
    e = rel_l2(logits, d["logits"])
    print(f"{dtype}: logits rel-L2 {e:.3e}")
    assert e < tol
    ok, frac = V._argmax_ok(logits, d["logits"], 5 * tol)
    assert ok
    assert abs(info["loss"] - float(d["info_loss"])) <= tol * abs(float(d["info_loss"]))
    gv = np.stack([getattr(m, f"vpt_{i}").grad.cpu().numpy() for i in range(L)])
    ev = rel_l2(gv[:, :, ::4], d["grad_vpt_sub"])
    print(f"{dtype}: prompt gradients rel-L2 {ev:.3e}")
    assert ev < 5 * tol


# ----------------------------------------------------------------------------- clip_vit_b_32, trainable text
def _count_text_calls(monkeypatch):
    """Counts ebc_text_forward / ebc_text_backward calls and their prompt counts through _lib.lib()."""
    from ebc_amd import _lib
    real = _lib.lib()
    calls = {"fwd": [], "bwd": []}

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name == "ebc_text_forward":
                return lambda *a: (calls["fwd"].append(a[3]), fn(*a))[1]          # (w, ids, eot, NB, ...)
            if name == "ebc_text_backward":
                return lambda *a: (calls["bwd"].append(a[8]), fn(*a))[1]          # (w, g, ids, eot, uniq, offs, rows, nu, NB, ..)
            return fn
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    return calls


@pytest.mark.parametrize("tower", ["torch", "hip"])
def test_bins20_train_step_fp32_with_trainable_text(tower, monkeypatch):
    """Every assertion and bar of test_gpu_text_train.py::test_train_step_fp32_matches_reference_with_trainable_text on
    the keys F13 stores; with the HIP tower, the 20 prompts must have run as two library calls each way (16 + 4)."""
    d = golden(FIX)
    m, bins = _b32(d, text_layers=int(d["t_text_layers"]), freeze_text_encoder=False, text_tower=tower)
    assert m.text_encoder.impl == tower
    calls = _count_text_calls(monkeypatch)
    _, logits, exp, info, gtext = _step(m, d, bins, pre="t_")
    if tower == "hip":
        assert calls["fwd"] == [16, 4] and sorted(calls["bwd"]) == [4, 16], calls
        from ebc_amd.text import prompt_index
        own = [prompt_index(d["prompt_tokens"][k0:k0 + 16]) for k0 in (0, 16)]      # each chunk's own Lt, uniq, offs, rows
        for c, o in zip(m.text_encoder._hip_index[3], own):
            assert int(c["Lt"]) == o["Lt"] and all(np.array_equal(c[k].cpu().numpy(), o[k]) for k in o if k != "Lt")
    else:
        assert calls == {"fwd": [], "bwd": []}
    _check_fp32_step(m, d, "t_", logits, exp, info)
    assert rel_l2(m.projection.weight.grad.cpu().numpy()[::6, ::6], d["t_grad_proj_w_sub"]) < 5e-3
    assert sorted(n for n, p in m.named_parameters() if p.grad is not None) == [str(n) for n in d["t_trainable"]]
    assert gtext is not None and gtext.shape == (20, 512)
    te = m.text_encoder
    blk = te.transformer.resblocks[0]
    got = {"grad_text_features": gtext, "grad_text_projection_rows8": te.text_projection.grad[::8],
           "grad_ln_final_w": te.ln_final.weight.grad, "grad_ln_final_b": te.ln_final.bias.grad,
           "grad_blk0_in_proj_w_sub": blk.attn.in_proj_weight.grad[::8, ::8],
           "grad_blk0_c_fc_w_sub": blk.mlp.c_fc.weight.grad[::8, ::8],
           "grad_token_rows": te.token_embedding.weight.grad[torch.from_numpy(d["t_token_ids"]).cuda()]}
    errs = {k: rel_l2(v, d["t_" + k]) for k, v in got.items()}
    print("text gradients rel-L2:", " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < 5e-3 for v in errs.values()), errs
    np.testing.assert_allclose(float(te.text_projection.grad.norm()), float(d["t_grad_text_projection_norm"]), rtol=5e-3)
    np.testing.assert_allclose(float(te.token_embedding.weight.grad.norm()), float(d["t_grad_token_norm"]), rtol=5e-3)
    assert rel_l2(m.text_features, d["t_text_features"]) < 1e-5 and not m.text_features.requires_grad


def test_bins20_chunked_hip_features_match_the_torch_tower():
    """tests/test_gpu_text_tower.py's fp32 bar: the HIP tower's rel-L2 distance to the float64 tower (CPU) is at most 4x
    the torch tower's on the same device, for the features of the 20 prompts run as two chunks."""
    from ebc_amd.text import CLIPTextEncoder, format_count, prompt_tokens
    d = golden(FIX)
    bins, _ = _table(d)
    ids = prompt_tokens([format_count(b[0] if b[0] == b[1] else b, "word") for b in bins])
    assert np.array_equal(ids.numpy(), d["prompt_tokens"])
    sd = {k[len("text_encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in syn.text_state(0, 2, 512).items()}
    feats = {}
    for name, impl, dev, dt in (("ref", "torch", "cpu", F64), ("torch", "torch", "cuda", torch.float32),
                                ("hip", "hip", "cuda", torch.float32)):
        enc = CLIPTextEncoder(512, 77, 49408, 512, 8, 2, impl=impl)
        enc.load_state_dict(sd)
        enc = enc.to(device=dev, dtype=dt)
        with torch.no_grad():
            feats[name] = enc(ids.to(dev)).detach().cpu().to(F64)
        if name == "hip":
            assert len(enc._hip_index[3]) == 2
    assert feats["hip"].shape == (20, 512)
    err = lambda a: float((a - feats["ref"]).norm() / feats["ref"].norm())
    e_hip, e_tor = err(feats["hip"]), err(feats["torch"])
    print(f"RATIO bins20_text.features {e_hip / (4 * e_tor):.4f}   (hip {e_hip:.3e}, torch {e_tor:.3e})")
    assert e_hip <= 4 * e_tor


# ----------------------------------------------------------------------------- clip_resnet50: the width-1024 head
def test_resnet50_bins20_step_matches_the_oracle():
    """One fp32 step of B = 2 at 224, reduction 32 (7 x 7 grid, 20 bins, embed 1024), against oracle.ref.resnet_forward
    on the CPU with the model's own frozen text features; the bars of
    tests/test_gpu_resnet.py::test_resnet_train_step_fp32_matches_reference for the tensors compared here."""
    from ebc_amd.losses import DACELoss
    from ebc_amd.model import get_model
    from oracle import ref
    d = golden(FIX)
    bins, anchors = _table(d)
    m = get_model("clip_resnet50", 224, 32, bins, anchors, prompt_type="word", text_layers=2, weights_seed=0).cuda().train()
    assert m.clip_embed_dim == 1024 and m.text_features.shape == (20, 1024)
    img, pts, dens = syn.synthetic_crops(2, 224, seed=9, counts=[60, 3])
    x = torch.from_numpy(img).cuda()
    with torch.backends.cudnn.flags(enabled=True, allow_tf32=False):
        logits, exp = m(x)
        loss, info = DACELoss(bins, 32, weight_count_loss=1.0, count_loss="dmcount", input_size=224)(
            logits, exp, torch.from_numpy(dens).cuda(), [torch.from_numpy(p).cuda() for p in pts])
        loss.backward()
    torch.cuda.synchronize()
    p = ref.resnet_params_from_state(syn.resnet50_full_state(0, include_text=False))
    ol, oe, _ = ref.resnet_forward(p, torch.from_numpy(img), m.text_features.detach().cpu(), anchors, reduction=32)
    oloss, oinfo = ref.dace_loss(ol, oe, torch.from_numpy(dens), pts, bins, reduction=32, input_size=224)
    oloss.backward()
    lg, want = logits.detach().cpu().numpy(), ol.detach().numpy()
    assert lg.shape == want.shape == (2, 20, 7, 7)
    per_patch = np.linalg.norm(lg - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f"clip_resnet50 20 bins: per-patch logits rel err max {per_patch.max():.2e}")
    assert per_patch.max() < 1e-3
    top2 = np.sort(want, axis=1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 1e-3 * np.abs(top2[:, 1]).clip(min=1.0)
    assert (lg.argmax(1) == want.argmax(1))[sure].all()
    assert rel_max(exp, oe) < 1e-3
    for k in ("loss", "tv_loss", "count_loss", "ce_loss"):
        assert abs(float(info[k]) - float(oinfo[k])) <= 1e-3 * abs(float(oinfo[k])), k
    dec = m.image_decoder[0]
    checks = {"grad_proj_w": (m.projection.weight.grad, p["projection.weight"].grad, 1e-4),
              "grad_proj_b": (m.projection.bias.grad, p["projection.bias"].grad, 1e-4),
              "grad_dec_bn3_w": (dec.bn3.weight.grad, p["image_decoder.0.bn3.weight"].grad, 1e-3),
              "grad_dec_conv1": (dec.conv1.weight.grad, p["image_decoder.0.conv1.weight"].grad, 1e-2),
              "grad_dec_conv3": (dec.conv3.weight.grad, p["image_decoder.0.conv3.weight"].grad, 1e-2),
              "grad_enc_conv1": (m.image_encoder.conv1.weight.grad, p["image_encoder.conv1.weight"].grad, 2e-2)}
    bad = []
    for k, (got, ref_g, t) in checks.items():
        e = rel_l2(got, ref_g.reshape(got.shape))
        print(f"  {k}: rel L2 {e:.2e} (tol {t:.0e})")
        if not e < t:
            bad.append(k)
    assert not bad, bad
    assert abs(float(m.logit_scale.grad) - float(p["logit_scale"].grad)) < 1e-3 * abs(float(p["logit_scale"].grad))
    m.eval()                                      # the eval-mode forward (running statistics) through the same head
    with torch.no_grad():
        ev = m(x)
    assert tuple(ev.shape) == (2, 1, 7, 7) and bool(torch.isfinite(ev).all()) and float(ev.min()) >= 0


# ----------------------------------------------------------------------------- clip_vit_b_16, 17 bins
@pytest.mark.parametrize("reduction", [8, 16])
def test_vit_b16_17_bins_forward_backward_match_the_oracle(reduction):
    """Bins [k, k] for k < 16 and [16, inf]: the first count past the 16-slot head, 2 layers, B = 4 at 224.  Reduction 8
    is oracle.ref.forward as it stands; its decoder is written for the x2 adapt, so reduction 16 (no adapt) composes
    ref.vit_vpt_forward, the BasicBlock lines of ref.decoder without the interpolation, and ref.head.  fp32 bars of
    tests/test_gpu_model.py: logits per patch and exp 1e-3, gradients 5e-3."""
    from ebc_amd.model import get_model
    from oracle import ref
    bins = [(float(k), float(k)) for k in range(16)] + [(16.0, float("inf"))]
    anchors = [float(k) for k in range(16)] + [18.5]
    L = 2
    m = get_model("clip_vit_b_16", 224, reduction, bins, anchors, prompt_type="word", vit_layers=L, text_layers=2,
                  weights_seed=0).cuda().train()
    assert m.text_features.shape == (17, 512)
    img = syn.synthetic_crops(4, 224, seed=77, counts=[3, 40, 0, 250])[0]
    logits, exp = m(torch.from_numpy(img).cuda())
    g = syn.crop_rng(1077)
    R1 = torch.from_numpy(g.standard_normal(tuple(logits.shape)).astype(np.float32))
    R2 = torch.from_numpy(g.standard_normal(tuple(exp.shape)).astype(np.float32))
    ((logits * R1.cuda()).sum() + (exp * R2.cuda()).sum()).backward()
    torch.cuda.synchronize()
    p = ref.params_from_state(syn.full_state(0, layers=L, include_text=False))
    txt = m.text_features.detach().cpu()
    if reduction == 8:
        ol, oe, _ = ref.forward(p, torch.from_numpy(img), txt, anchors, L)
    else:
        x = ref.vit_vpt_forward(p, torch.from_numpy(img), L)
        dd = "image_decoder.0."
        o = F.relu(ref.batch_norm_train(F.conv2d(x, p[dd + "conv1.weight"], padding=1), p[dd + "bn1.weight"], p[dd + "bn1.bias"]))
        o = ref.batch_norm_train(F.conv2d(o, p[dd + "conv2.weight"], padding=1), p[dd + "bn2.weight"], p[dd + "bn2.bias"])
        ol, oe = ref.head(p, F.relu(o + x), txt, anchors)
    ((ol * R1).sum() + (oe * R2).sum()).backward()
    lg, want = logits.detach().cpu().numpy(), ol.detach().numpy()
    side = 224 // reduction
    assert lg.shape == want.shape == (4, 17, side, side)
    per_patch = V._per_patch(lg, want)
    print(f"vit_b_16 17 bins r{reduction}: per-patch logits rel err max {per_patch.max():.2e}")
    assert per_patch.max() < 1e-3
    ok, _ = V._argmax_ok(lg, want, 1e-3)
    assert ok
    assert rel_max(exp, oe) < 1e-3
    gv = torch.stack([getattr(m, f"vpt_{i}").grad.cpu() for i in range(L)])
    ov = torch.stack([p[f"vpt_{i}"].grad for i in range(L)])
    errs = {"vpt": rel_l2(gv, ov), "projection": rel_l2(m.projection.weight.grad, p["projection.weight"].grad),
            "logit_scale": rel_l2(m.logit_scale.grad, p["logit_scale"].grad)}
    print(f"vit_b_16 17 bins r{reduction}: gradient rel-L2 {errs}")
    for k, e in errs.items():
        assert e < 5e-3, (k, e)
