"""Generate the 20-bin reduction-32 parity fixture (F13) by running the REFERENCE (Yiming-M/CLIP-EBC) on the CPU.

    python tests/golden/make_golden_bins20.py

Same method as make_golden_b32.py (whose helpers this imports; neither it nor make_golden.py is changed).  The bin table
is the reference's own `configs/reduction_32.json["19"]["qnrf"]`, granularity `fine` with the `average` anchors: 20 bins
`[0,0] .. [18,18], [19,inf]`, more than the 16 the similarity head used to take.  Both arrays are stored (settings; the
open end as np.inf).

Case `frozen`: `_clip_ebc("vit_b_32", bins, anchors, reduction=32, prompt_type="word", input_size=224, num_vpt=32,
deep_vpt=True, vpt_drop=0.0)`, 2 layers, `ebc_amd.synthetic.full_state(0, layers=2, input_size=224, patch=32)`, B = 4:
the train step with `DACELoss(bins, 32, count_loss="dmcount", input_size=224)` (logits, exp, the loss terms, the
gradients subsampled as F10's grid cases store them), the eval-mode exp, and the 20 prompts' token ids from the reference tokenizer.

Case `text` (keys prefixed `t_`): the same with `freeze_text_encoder=False` and a 2-layer text tower
(`full_state(0, layers=2, text_layers=2, ...)`, as F11): text features, their gradient and the text-parameter gradient
slices F11 holds (`text_projection`'s gradient every 8th row, the projection weight's every 6th row and column, no
decoder convolution gradients: the file stays under 1 MiB).

Both of make_golden_b32.py's conditions are enforced per case, and a crop seed that misses one is passed over:
  * the share of patches with a sure argmax (`sure_share`) must be above 0.9,
  * the summed effect of the unsure decoder-ReLU decisions (`relu_flip_bound`, on (logits * R1).sum() + (exp * R2).sum()
    with seeded R1 / R2) must be under FLIP_BUDGET = 2.5e-3: a BatchNorm channel sees only 4 x 49 pixels here, so one
    decision taken the other way moves the gradients visibly.
The seed used, the share, the count of unsure decisions and the flip sum are stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import save, syn  # noqa: E402
import make_golden_b32 as b32  # noqa: E402
from make_golden_b32 import FLIP_BUDGET, PATCH, RELU_TOL, WEIGHTS_SEED, relu_flip_bound, sure_share  # noqa: E402

LAYERS, TEXT_LAYERS, REDUCTION, SIZE, B = 2, 2, 32, 224, 4
COUNTS = (3, 40, 0, 250)
SEEDS = range(7, 107)


def reference_bins():
    with open(os.path.join(mg.REF, "configs", f"reduction_{REDUCTION}.json")) as f:
        cfg = json.load(f)["19"]["qnrf"]
    bins = [(float(b[0]), float(b[1])) for b in cfg["bins"]["fine"]]                 # trainer.py:105-106
    anchors = [float(p) for p in cfg["anchor_points"]["fine"]["average"]]
    assert len(bins) == len(anchors) == 20
    return bins, anchors


def load_reference():
    ref = b32.load_reference()
    ref.text_layers = 12
    _clip = sys.modules["models.clip._clip"]
    te = sys.modules["models.clip._clip.text_encoder"]
    _clip.vit_b_32_txt = lambda: te.CLIPTextEncoder(512, 77, 49408, 512, 8, ref.text_layers)
    return ref


def build_ref_model(ref, bins, anchors, freeze_text: bool):
    ref.state["vit_layers"] = LAYERS
    ref.text_layers = 12 if freeze_text else TEXT_LAYERS
    torch.manual_seed(0)
    m = ref.model_mod._clip_ebc("vit_b_32", bins, anchors, reduction=REDUCTION, freeze_text_encoder=freeze_text,
                                prompt_type="word", input_size=SIZE, num_vpt=32, deep_vpt=True, vpt_drop=0.0)
    kw = {} if freeze_text else {"text_layers": TEXT_LAYERS}
    sd = syn.full_state(WEIGHTS_SEED, layers=LAYERS, input_size=SIZE, patch=PATCH, **kw)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("num_batches_tracked") for k in missing) or not missing, missing
    if freeze_text:
        m._extract_text_features()
    else:
        assert m.text_features is None
    return m


def case(ref, bins, anchors, freeze_text: bool):
    loss_fn = ref.losses.DACELoss(bins, REDUCTION, weight_count_loss=1.0, count_loss="dmcount", input_size=SIZE)
    tag = "frozen" if freeze_text else "text"

    def forward(seed):
        m = build_ref_model(ref, bins, anchors, freeze_text).train()
        img, points, density = syn.synthetic_crops(B, SIZE, seed=seed, counts=list(COUNTS))
        kept = {}

        def hook(mod, inp, out):
            kept["text"] = out.detach().clone()
            out.register_hook(lambda g: kept.__setitem__("grad_text", g.detach().clone()))
        h = None if freeze_text else m.text_encoder.register_forward_hook(hook)
        logits, exp = m(torch.from_numpy(img))
        if h is not None:
            h.remove()
        return m, torch.from_numpy(img), points, density, kept, logits, exp

    for seed in SEEDS:
        m, x, points, density, kept, logits, exp = forward(seed)
        share = sure_share(logits.detach().numpy())
        if share <= 0.9:
            print(f"bins20 {tag} seed {seed}: sure-patch share {share:.3f}", flush=True)
            continue
        g = syn.crop_rng(seed + 1000)
        R1 = torch.from_numpy(g.standard_normal(tuple(logits.shape)).astype(np.float32))
        R2 = torch.from_numpy(g.standard_normal(tuple(exp.shape)).astype(np.float32))
        if not freeze_text:
            m.text_features = kept["text"]           # the restated decoder + head of the bound reads it
        n_unsure, flip_sum, own_err = relu_flip_bound(m, x, R1, R2, LAYERS)
        if not freeze_text:
            m.text_features = None
        print(f"bins20 {tag} seed {seed}: sure-patch share {share:.3f}; {n_unsure} unsure ReLU decisions, flip sum "
              f"{flip_sum:.2e}; own f32 pre-activation error {own_err:.1e}", flush=True)
        if flip_sum < FLIP_BUDGET:
            break
    else:
        raise AssertionError("no crop seed meets the argmax and ReLU-decision conditions")
    # the bound ran the model again in train mode (BatchNorm running statistics moved twice): the stored step and the
    # eval forward after it come from a fresh model that has seen the crops once
    m, x, points, density, kept, logits, exp = forward(seed)
    loss, info = loss_fn(logits, exp, torch.from_numpy(density), [torch.from_numpy(p) for p in points])
    loss.backward()
    dec = m.image_decoder[0]
    out = dict(layers=LAYERS, seed=seed, weights_seed=WEIGHTS_SEED, counts=np.asarray(COUNTS), batch=B,
               sure_share=share, relu_unsure=n_unsure, relu_flip_sum=flip_sum, relu_own_err=own_err,
               logits=logits.detach().numpy(), exp=exp.detach().numpy(),
               grad_vpt_sub=np.stack([getattr(m, f"vpt_{i}").grad.numpy() for i in range(LAYERS)])[:, :, ::4],
               grad_vpt_norm=np.asarray([np.linalg.norm(getattr(m, f"vpt_{i}").grad.numpy()) for i in range(LAYERS)]),
               grad_proj_b=m.projection.bias.grad.numpy(), grad_logit_scale=m.logit_scale.grad.numpy(),
               grad_dec_bn1_w=dec.bn1.weight.grad.numpy(), grad_dec_bn2_b=dec.bn2.bias.grad.numpy())
    for k, v in info.items():
        out["info_" + k] = v.detach().numpy().reshape(())
    if freeze_text:
        out.update(grad_proj_w_sub=m.projection.weight.grad.numpy()[::4, ::4],
                   grad_dec_conv1_sub=dec.conv1.weight.grad.numpy()[::12, ::12],
                   grad_dec_conv2_sub=dec.conv2.weight.grad.numpy()[::16, ::16], text_features=m.text_features.detach().numpy(),
                   prompt_tokens=m.text_prompts.numpy().astype(np.int32))
        m.eval()
        with torch.no_grad():
            out["exp_eval"] = m(x).numpy()
        return out
    te = m.text_encoder
    blk = te.transformer.resblocks[0]
    ids = np.unique(m.text_prompts.numpy())
    g_tok = te.token_embedding.weight.grad.numpy()
    g_tp = te.text_projection.grad.numpy()
    out.update(text_layers=TEXT_LAYERS, grad_proj_w_sub=m.projection.weight.grad.numpy()[::6, ::6],
               trainable=np.asarray(sorted(n for n, p in m.named_parameters() if p.requires_grad)),
               text_features=kept["text"].numpy(), grad_text_features=kept["grad_text"].numpy(),
               grad_text_projection_rows8=g_tp[::8], grad_text_projection_norm=np.linalg.norm(g_tp),
               grad_ln_final_w=te.ln_final.weight.grad.numpy(), grad_ln_final_b=te.ln_final.bias.grad.numpy(),
               grad_blk0_in_proj_w_sub=blk.attn.in_proj_weight.grad.numpy()[::8, ::8],
               grad_blk0_c_fc_w_sub=blk.mlp.c_fc.weight.grad.numpy()[::8, ::8],
               token_ids=ids.astype(np.int64), grad_token_rows=g_tok[ids], grad_token_norm=np.linalg.norm(g_tok))
    return {"t_" + k: v for k, v in out.items()}


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    bins, anchors = reference_bins()
    out = dict(bins=np.asarray(bins, np.float64), anchors=np.asarray(anchors, np.float64), reduction=REDUCTION,
               input_size=SIZE, relu_tol=RELU_TOL, relu_flip_budget=FLIP_BUDGET)
    out.update(case(ref, bins, anchors, True))
    out.update(case(ref, bins, anchors, False))
    save("f13_b32_r32_bins20.npz", **out)


if __name__ == "__main__":
    main()
