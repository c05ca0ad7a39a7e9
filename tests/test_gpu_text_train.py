"""GPU end-to-end checks of freeze_text_encoder=False: the text tower runs in every forward and the loss's gradient
reaches its parameters through the HIP head (ebc_head_bwd_text).

fp32 against the reference's own run with a trainable text tower (tests/golden/f11_text_train_l2.npz, written by
tests/golden/make_golden_text.py): test_gpu_model.py's bars for logits / exp / loss terms / prompt and projection
gradients; the text-feature gradient and every stored text-parameter gradient rel-L2 < 5e-3, the project's bar for the
projection weight, which sits at the same depth (below it both sides run torch in f32)."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import _ddp_text_worker as TW
import _ddp_worker as W
import _enc_refs as R
from conftest import ANCHORS_NWPU, BINS, golden, rel_l2, rel_max
from ebc_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _model(**kw):
    from ebc_amd.model import get_model
    d = golden("f11_text_train_l2.npz")
    m = get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, prompt_type="word", vit_layers=int(d["layers"]),
                  text_layers=int(d["text_layers"]), weights_seed=int(d["weights_seed"]), freeze_text_encoder=False, **kw)
    return m.cuda(), d


def _step(m, d, autocast=None, scaler=None):
    """One training step on the fixture's crops; returns logits, exp, the loss terms and d loss / d text_features."""
    from ebc_amd.losses import DACELoss
    img, pts, dens = syn.synthetic_crops(int(d["batch"]), 224, seed=int(d["seed"]), counts=list(d["counts"]))
    m.train()
    m.zero_grad(set_to_none=True)
    kept = {}

    def hook(mod, inp, out):
        out.register_hook(lambda g: kept.__setitem__("grad_text", g.detach().float().cpu().numpy()))
    h = m.text_encoder.register_forward_hook(hook)
    loss_fn = DACELoss(BINS, 8, weight_count_loss=1.0, count_loss="dmcount", input_size=224)
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        logits, exp = m(torch.from_numpy(img).cuda())
        loss, info = loss_fn(logits, exp, torch.from_numpy(dens).cuda(), [torch.from_numpy(p).cuda() for p in pts])
    h.remove()
    (scaler.scale(loss) if scaler is not None else loss).backward()
    torch.cuda.synchronize()
    return (logits.detach().float().cpu().numpy(), exp.detach().float().cpu().numpy(),
            {k: float(v) for k, v in info.items()}, kept.get("grad_text"))


def _argmax_ok(logits, ref_logits, tol):
    top2 = np.sort(ref_logits, axis=1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > tol * np.abs(top2[:, 1]).clip(min=1.0)
    return (logits.argmax(1) == ref_logits.argmax(1))[sure].all(), sure.mean()


def _text_grads(m):
    te = m.text_encoder
    blk = te.transformer.resblocks[0]
    return {"grad_text_projection_rows2": te.text_projection.grad[::2], "grad_ln_final_w": te.ln_final.weight.grad,
            "grad_ln_final_b": te.ln_final.bias.grad, "grad_blk0_in_proj_w_sub": blk.attn.in_proj_weight.grad[::8, ::8],
            "grad_blk0_c_fc_w_sub": blk.mlp.c_fc.weight.grad[::8, ::8]}


def test_train_step_fp32_matches_reference_with_trainable_text():
    m, d = _model()
    L = int(d["layers"])
    logits, exp, info, gtext = _step(m, d)
    per_patch = np.linalg.norm(logits - d["logits"], axis=1) / np.linalg.norm(d["logits"], axis=1)
    print(f"per-patch logits rel err: max {per_patch.max():.2e}")
    assert per_patch.max() < 1e-3 and rel_max(logits, d["logits"]) < 1e-3
    ok, frac = _argmax_ok(logits, d["logits"], 1e-3)
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
    errs.update({k: rel_l2(v, d[k]) for k, v in _text_grads(m).items()})
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


def test_train_step_fp16_autocast_trains_the_text_tower():
    """Logits inside test_gpu_vit_b32.py's fp16 band (rel-L2 2e-2, argmax at 5x) of the fp32 fixture; the text tower,
    under the caller's autocast, gets finite non-zero gradients and one GradScaler.step(Adam) moves text_projection.

    The loss scale is 2^4.  d loss / d text_features is a sum over all pixels (largest element 46 in the reference's
    fp32 run of this step, the fixture's grad_text_features), the tower's fp16 activations take their gradients in
    fp16, as the reference's do, and the largest gradient element inside the tower is 1.9e3 in fp32 (the stored
    gradients reach 1.8e3, a token_embedding row).  1.9e3 x 2^16 (GradScaler's initial scale) is far beyond fp16's 65504: a real run skips its
    first steps while the scaler backs off to 2^5 or below.  A one-step test starts where that settles."""
    from ebc_amd import optim as eo
    m, d = _model()
    stored = max(float(np.abs(d[k]).max()) for k in d.files if k.startswith("grad_") and d[k].ndim > 0)
    assert stored * 2.0 ** 4 < 65504 / 2
    opt = eo.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    sc = eo.GradScaler(init_scale=2.0 ** 4)
    logits, exp, info, gtext = _step(m, d, autocast=torch.float16, scaler=sc)
    tol = 2e-2
    e = rel_l2(logits, d["logits"])
    print(f"fp16 logits rel-L2 {e:.3e}")
    assert e < tol
    assert _argmax_ok(logits, d["logits"], 5 * tol)[0]
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


def test_resnet50_text_gradient_matches_f64_head(monkeypatch):
    """clip_resnet50 (embed 1024) with the flag, one train-mode forward + backward at 224 (the smallest input of
    test_gpu_resnet.py): finite non-zero gradients on every text parameter, and d / d text_features against autograd of
    a torch-f64 restatement of the head on the same Z (the projection GEMM repeated on the same operands), to the
    kernel test's bound."""
    import test_gpu_head_text_kernel as K
    from ebc_amd import _lib, model as M
    m = M.get_model("clip_resnet50", 224, 8, BINS, ANCHORS_NWPU, prompt_type="word", text_layers=2, weights_seed=0,
                    freeze_text_encoder=False).cuda().train()
    seen = {}
    real = M._HeadFn

    class Spy:                                   # records the head's operands and the gradient of its text operand
        _forward, _backward = staticmethod(real._forward), staticmethod(real._backward)

        @staticmethod
        def apply(y, weight, bias, logit_scale, text, anchors, cdt, nhwc):
            seen.update(y=y.detach(), text=text.detach())
            text.register_hook(lambda g: seen.__setitem__("dtext", g.detach()))
            return real.apply(y, weight, bias, logit_scale, text, anchors, cdt, nhwc)
    monkeypatch.setattr(M, "_HeadFn", Spy)
    x =torch.from_numpy(syn.synthetic_crops(2, 224, seed=3)[0]).cuda()
    logits, exp = m(x)
    g = torch.Generator().manual_seed(11)
    R1 = torch.randn(logits.shape, generator=g).cuda()
    R2 = torch.randn(exp.shape, generator=g).cuda()
    ((logits * R1).sum() + (exp * R2).sum()).backward()
    torch.cuda.synchronize()
    for n, p in m.text_encoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    # the same Z: the projection GEMM on the same operands (deterministic)
    y = seen["y"]
    B, Hh, Ww, C = y.shape
    P, HW, E, NB = B * Hh * Ww, Hh * Ww, 1024, len(BINS)
    assert y.dtype == torch.float32 and y.is_contiguous()
    Wc = m.projection.weight.detach().reshape(E, C).contiguous()
    bf = m.projection.bias.detach().float().contiguous()
    Z = torch.empty(P, E, device="cuda", dtype=torch.float32)
    _lib.check(_lib.lib().ebc_gemm(_lib.EBC_F32, 0, 1, _lib.ptr(y.reshape(P, C)), _lib.ptr(Wc), _lib.ptr(Z), _lib.ptr(bf),
                                   None, None, P, E, C, _lib.stream()), "ebc_gemm")
    Z, text = Z.cpu().to(F64), seen["text"].detach().cpu().to(F64)
    ls = m.logit_scale.detach().cpu().to(F64).reshape(1)
    anchors = torch.tensor(ANCHORS_NWPU, dtype=torch.float32).to(F64)
    # torch-f64 restatement of models/clip/model.py:203-212 and its autograd
    t64 = text.clone().requires_grad_(True)
    zi = torch.nn.functional.normalize(Z.view(B, Hh, Ww, E), p=2, dim=-1)
    lg = (ls.exp() * zi @ torch.nn.functional.normalize(t64, p=2, dim=-1).t()).permute(0, 3, 1, 2)
    ex = (lg.softmax(dim=1) * anchors.view(1, -1, 1, 1)).sum(dim=1, keepdim=True)
    ((lg * R1.cpu().to(F64)).sum() + (ex * R2.cpu().to(F64)).sum()).backward()
    r = R.head_bwd(Z, text, ls, anchors, R1.cpu().to(F64).view(B, NB, HW), R2.cpu().to(F64).view(B, HW), 1.0, B, HW)
    t = K.text_grad_ref(r, text)
    assert rel_l2(t["dt"], t64.grad) < 1e-12                    # the kernel test's restatement is that autograd
    bound = K.text_grad_bound(r, t, K.E._head_fwd_bounds(r, E, NB), anchors, NB, -(-P // K.PPB))
    K._report("resnet50.dtext", (seen["dtext"].cpu().to(F64) - t64.grad).abs(), bound)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_ddp_text_gradients_match_single_process(tmp_path):
    """World 2 on one GPU over gloo, as test_gpu_ddp.py (uneven ranks, the ranks' decoder ReLU decisions replayed in
    the single process): the text-parameter gradients after wrap_ddp equal the single-process gradients of the mean of
    the ranks' losses on the concatenated batch, to that test's bar for every trainable parameter (rel-L2 2e-4)."""
    from multiprocessing import forkserver
    if getattr(forkserver._forkserver, "_forkserver_pid", None) is None:
        pytest.skip("run with -m gpu: the ranks need the forkserver conftest.py starts before GPU init")
    ctx = mp.get_context("forkserver")
    port = _free_port()
    procs = [ctx.Process(target=TW.rank_main, args=(r, 2, port, str(tmp_path))) for r in range(2)]
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
    m = TW.build(dev)
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
    assert n_text == 5 + 12 * TW.TEXT_LAYERS and not bad, bad
