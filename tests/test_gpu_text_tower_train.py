"""GPU end-to-end checks of freeze_text_encoder=False with text_tower="hip": the whole training step with the text tower
in the library (ebc_text_forward / ebc_text_backward).  The assertions and bars are those of tests/test_gpu_text_train.py
(whose step, fixture F11 and helpers are used as they are), on the model built with the keyword."""
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

import _ddp_text_hip_worker as HW
import _ddp_worker as W
import test_gpu_text_train as T
from conftest import ANCHORS_NWPU, BINS, rel_l2, rel_max

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _model():
    m, d = T._model(text_tower="hip")
    assert m.text_encoder.impl == "hip"
    return m, d


def test_train_step_fp32_matches_reference_with_the_hip_text_tower():
    """Every assertion and bar of test_train_step_fp32_matches_reference_with_trainable_text."""
    m, d = _model()
    L = int(d["layers"])
    logits, exp, info, gtext = T._step(m, d)
    per_patch = np.linalg.norm(logits - d["logits"], axis=1) / np.linalg.norm(d["logits"], axis=1)
    print(f"per-patch logits rel err: max {per_patch.max():.2e}")
    assert per_patch.max() < 1e-3 and rel_max(logits, d["logits"]) < 1e-3
    ok, frac = T._argmax_ok(logits, d["logits"], 1e-3)
    assert ok and frac > 0.9
    assert rel_max(exp, d["exp"]) < 1e-3
    for k in ("loss", "tv_loss", "count_loss", "ce_loss"):
        assert abs(info[k] - float(d["info_" + k])) <= 1e-3 * abs(float(d["info_" + k])), k
    gv = np.stack([getattr(m, f"vpt_{i}").grad.cpu().numpy() for i in range(L)])
    assert rel_l2(gv[:, :, ::4], d["grad_vpt_sub"]) < 5e-3
    np.testing.assert_allclose(np.linalg.norm(gv, axis=(1, 2)), d["grad_vpt_norm"], rtol=5e-3)
    assert rel_l2(m.projection.weight.grad.cpu().numpy()[::3, ::3], d["grad_proj_w_sub"]) < 5e-3
    assert abs(float(m.logit_scale.grad) - float(d["grad_logit_scale"])) < 1e-3 * abs(float(d["grad_logit_scale"]))
    # the text tower
    assert sorted(n for n, p in m.named_parameters() if p.grad is not None) == [str(n) for n in d["trainable"]]
    assert gtext is not None
    errs = {"grad_text_features": rel_l2(gtext, d["grad_text_features"])}
    errs.update({k: rel_l2(v, d[k]) for k, v in T._text_grads(m).items()})
    g_tok = m.text_encoder.token_embedding.weight.grad
    errs["grad_token_rows"] = rel_l2(g_tok[torch.from_numpy(d["token_ids"]).cuda()], d["grad_token_rows"])
    print("text gradients rel-L2:", " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < 5e-3 for v in errs.values()), errs
    np.testing.assert_allclose(float(m.text_encoder.text_projection.grad.norm()), float(d["grad_text_projection_norm"]),
                               rtol=5e-3)
    np.testing.assert_allclose(float(g_tok.norm()), float(d["grad_token_norm"]), rtol=5e-3)
    # the buffer follows the forward's features (detached), in eval mode too
    assert rel_l2(m.text_features, d["text_features"]) < 1e-5 and not m.text_features.requires_grad
    with torch.no_grad():
        m.text_encoder.text_projection.mul_(0.5)
    m.eval()
    with torch.no_grad():
        m(torch.zeros(1, 3, 224, 224, device="cuda"))
    assert rel_l2(m.text_features, 0.5 * d["text_features"]) < 1e-5


def test_train_step_fp16_autocast_trains_the_hip_text_tower():
    """The assertions of test_train_step_fp16_autocast_trains_the_text_tower (loss scale 2^4, as reasoned there)."""
    from ebc_amd import optim as eo
    m, d = _model()
    opt = eo.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    sc = eo.GradScaler(init_scale=2.0 ** 4)
    logits, exp, info, gtext = T._step(m, d, autocast=torch.float16, scaler=sc)
    tol = 2e-2
    e = rel_l2(logits, d["logits"])
    print(f"fp16 logits rel-L2 {e:.3e}")
    assert e < tol
    assert T._argmax_ok(logits, d["logits"], 5 * tol)[0]
    assert gtext is not None and np.isfinite(gtext).all() and np.abs(gtext).max() > 0
    for n, p in m.text_encoder.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
    before = m.text_encoder.text_projection.detach().clone()
    sc.step(opt)
    sc.update()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(m.text_encoder.text_projection).all())
    assert not torch.equal(before, m.text_encoder.text_projection.detach())


def test_resnet50_hip_text_gradients_match_the_torch_tower():
    """clip_resnet50 (embed 1024, 2 text layers): the same d / d text_features through both towers, each text-parameter
    gradient of the HIP tower within the fp32 bar of tests/test_gpu_text_tower.py (4x the torch tower's own distance to
    the float64 tower on the CPU)."""
    from ebc_amd import model as M
    from ebc_amd.text import CLIPTextEncoder
    mk = lambda tower: M.get_model("clip_resnet50", 224, 8, BINS, ANCHORS_NWPU, prompt_type="word", text_layers=2,
                                   weights_seed=0, freeze_text_encoder=False, text_tower=tower).cuda().train()
    hip, tor = mk("hip"), mk("torch")
    assert hip.text_encoder.impl == "hip" and hip.clip_embed_dim == 1024
    ids = hip._prompt_ids(torch.device("cuda"))
    df = torch.randn(len(BINS), 1024, generator=torch.Generator().manual_seed(5))
    ref = CLIPTextEncoder(1024, 77, 49408, 512, 8, 2)
    ref.load_state_dict(tor.text_encoder.state_dict())
    ref = ref.to(F64)
    res = {}
    for name, enc, dev in (("hip", hip.text_encoder, "cuda"), ("torch", tor.text_encoder, "cuda"), ("ref", ref, "cpu")):
        f = enc(ids.to(dev))
        f.backward(df.to(device=dev, dtype=f.dtype))
        res[name] = {"features": f.detach().cpu(), **{n: p.grad.detach().cpu() for n, p in enc.named_parameters()}}
    err = lambda a, b: float((a.to(F64) - b).norm() / b.norm().clamp_min(1e-300))
    bad = []
    for n, r in res["ref"].items():
        e_hip, e_tor = err(res["hip"][n], r), err(res["torch"][n], r)
        print(f"RATIO resnet50_text.{n} {e_hip / (4 * e_tor) if e_tor else 0.0:.4f}   (hip {e_hip:.3e}, torch {e_tor:.3e})")
        if not e_hip <= 4 * e_tor:
            bad.append((n, e_hip, e_tor))
    assert not bad, bad
    # and through the whole model: one train-mode step reaches every text parameter
    x = torch.from_numpy(T.syn.synthetic_crops(2, 224, seed=3)[0]).cuda()
    hip.zero_grad(set_to_none=True)
    logits, exp = hip(x)
    (logits.square().mean() + exp.mean()).backward()
    torch.cuda.synchronize()
    for n, p in hip.text_encoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n


def test_ddp_hip_text_gradients_match_single_process(tmp_path):
    """test_ddp_text_gradients_match_single_process with the HIP tower on the ranks and in the single process: the bar is
    that test's, rel-L2 2e-4 for every trainable parameter."""
    from multiprocessing import forkserver
    if getattr(forkserver._forkserver, "_forkserver_pid", None) is None:
        pytest.skip("run with -m gpu: the ranks need the forkserver conftest.py starts before GPU init")
    ctx = mp.get_context("forkserver")
    port = T._free_port()
    procs = [ctx.Process(target=HW.rank_main, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=110)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert codes == [0, 0], codes
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"), weights_only=True)
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"), weights_only=True)
    from ebc_amd.losses import DACELoss
    from ebc_amd.model import DecoderMaskTap
    dev = torch.device("cuda:0")
    m = HW.build(dev)
    assert m.text_encoder.impl == "hip"
    img, pts, dens = W.batch()
    logits, exp = m(torch.from_numpy(img).to(dev))
    DecoderMaskTap.replay = [(torch.cat([r0["mask1"], r1["mask1"]]).to(dev), torch.cat([r0["mask2"], r1["mask2"]]).to(dev))]
    fn = DACELoss(W.BINS, 8, count_loss="dmcount", input_size=224)
    total, b0 = 0.0, 0
    for n in W.SPLIT:
        sl = slice(b0, b0 + n)
        loss, _ = fn(logits[sl], exp[sl], torch.from_numpy(dens[sl]).to(dev), [torch.from_numpy(p).to(dev) for p in pts[sl]])
        total = total + loss / len(W.SPLIT)
        b0 += n
    try:
        total.backward()
        assert not DecoderMaskTap.replay
    finally:
        DecoderMaskTap.replay = None
    bad, worst, n_text = [], (None, 0.0), 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        n_text += k.startswith("text_encoder.")
        g = p.grad.detach().cpu()
        for rank, r in enumerate((r0, r1)):
            if k == "text_encoder.token_embedding.weight":
                assert torch.equal(r["tok_rows"], g.abs().amax(1).nonzero().flatten())
                errs = [rel_l2(r["tok_grad"].numpy(), g[r["tok_rows"]].numpy()),
                        abs(float(r["tok_norm"]) / float(g.norm()) - 1)]
            else:
                errs = [rel_l2(r[k].numpy(), g.numpy())]
            worst = max(worst, (k, max(errs)), key=lambda e: e[1])
            if max(errs) >= 2e-4:
                bad.append((k, rank, errs))
    print("worst gradient rel-L2", worst)
    assert n_text == 5 + 12 * HW.TEXT_LAYERS and not bad, bad
