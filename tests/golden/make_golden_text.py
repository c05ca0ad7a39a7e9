"""Generate the trainable-text-tower parity fixture (F11) by running the REFERENCE (Yiming-M/CLIP-EBC) on the CPU.

    python tests/golden/make_golden_text.py

Same method as make_golden.py (whose helpers this imports; it is not changed).  The case is the reference's
`_clip_ebc("vit_b_16", ..., freeze_text_encoder=False)` (models/clip/model.py:37,100-115,201): `text_features` stays
None, `text_encoder(text_prompts)` runs inside the forward and the loss's gradient reaches every text parameter.
  * weights: `ebc_amd.synthetic.full_state(0, layers=2, text_layers=2)`; the stub `vit_b_16_txt` factory builds the
    reference's own `CLIPTextEncoder(512, 77, 49408, 512, 8, 2)` (a 2-layer text tower),
  * batch 2 at 224, reduction 8, DACE + dmcount, fp32.
Stored: logits, exp, the loss terms, the sorted names of the trainable parameters, the prompt / projection gradients as
F4 stores them, and for the text tower
  * the gradient of the text features [NB, 512] (a tensor hook on the text encoder's output),
  * `ln_final` gradients whole; `text_projection`'s gradient: every second row (the whole f32 matrix alone is the
    1 MiB a committed file may have) and its Frobenius norm,
  * `transformer.resblocks.0` `attn.in_proj_weight` / `mlp.c_fc.weight` gradients, every 8th row and column,
  * `token_embedding` gradient rows of the token ids the prompts use, and the norm of the whole gradient.
The case must leave the tests' argmax check meaningful (make_golden_b32.py `sure_share` > 0.9 on the reference's own
logits); it moves on to the next crop seed otherwise and stores the seed used.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import ANCHORS_NWPU, BINS, save, syn  # noqa: E402
from make_golden_b32 import sure_share  # noqa: E402

LAYERS, TEXT_LAYERS, WEIGHTS_SEED = 2, 2, 0


def load_reference():
    ref = mg.load_reference()
    _clip = sys.modules["models.clip._clip"]
    te = sys.modules["models.clip._clip.text_encoder"]
    _clip.vit_b_16_txt = lambda: te.CLIPTextEncoder(512, 77, 49408, 512, 8, TEXT_LAYERS)
    return ref


def build_ref_model(ref):
    ref.state["vit_layers"] = LAYERS
    torch.manual_seed(0)
    m = ref.model_mod._clip_ebc("vit_b_16", BINS, ANCHORS_NWPU, reduction=8, freeze_text_encoder=False,
                                prompt_type="word", input_size=224, num_vpt=32, deep_vpt=True, vpt_drop=0.0)
    assert m.text_features is None
    sd = syn.full_state(WEIGHTS_SEED, layers=LAYERS, text_layers=TEXT_LAYERS)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("num_batches_tracked") for k in missing) or not missing, missing
    return m


def text_case(ref, B=2, counts=(37, 5), seeds=(7, 8, 9, 10)):
    loss_fn = ref.losses.DACELoss(BINS, 8, weight_count_loss=1.0, count_loss="dmcount", input_size=224)
    for seed in seeds:
        m = build_ref_model(ref).train()
        img, points, density = syn.synthetic_crops(B, 224, seed=seed, counts=list(counts))
        kept = {}

        def hook(mod, inp, out):
            kept["text"] = out.detach().clone()
            out.register_hook(lambda g: kept.__setitem__("grad_text", g.detach().clone()))
        h = m.text_encoder.register_forward_hook(hook)
        logits, exp = m(torch.from_numpy(img))
        h.remove()
        share = sure_share(logits.detach().numpy())
        print(f"text l{LAYERS}/t{TEXT_LAYERS} seed {seed}: sure-patch share {share:.3f}")
        if share > 0.9:
            break
    else:
        raise AssertionError("no crop seed leaves > 0.9 of the patches with a sure argmax")
    loss, info = loss_fn(logits, exp, torch.from_numpy(density), [torch.from_numpy(p) for p in points])
    loss.backward()
    te = m.text_encoder
    blk = te.transformer.resblocks[0]
    ids = np.unique(m.text_prompts.numpy())
    g_tok = te.token_embedding.weight.grad.numpy()
    g_tp = te.text_projection.grad.numpy()
    out = dict(layers=LAYERS, text_layers=TEXT_LAYERS, seed=seed, weights_seed=WEIGHTS_SEED, counts=np.asarray(counts),
               batch=B, sure_share=share, logits=logits.detach().numpy(), exp=exp.detach().numpy(),
               trainable=np.asarray(sorted(n for n, p in m.named_parameters() if p.requires_grad)),
               grad_vpt_sub=np.stack([getattr(m, f"vpt_{i}").grad.numpy() for i in range(LAYERS)])[:, :, ::4],
               grad_vpt_norm=np.asarray([np.linalg.norm(getattr(m, f"vpt_{i}").grad.numpy()) for i in range(LAYERS)]),
               grad_proj_w_sub=m.projection.weight.grad.numpy()[::3, ::3], grad_proj_b=m.projection.bias.grad.numpy(),
               grad_logit_scale=m.logit_scale.grad.numpy(),
               text_features=kept["text"].numpy(), grad_text_features=kept["grad_text"].numpy(),
               grad_text_projection_rows2=g_tp[::2], grad_text_projection_norm=np.linalg.norm(g_tp),
               grad_ln_final_w=te.ln_final.weight.grad.numpy(), grad_ln_final_b=te.ln_final.bias.grad.numpy(),
               grad_blk0_in_proj_w_sub=blk.attn.in_proj_weight.grad.numpy()[::8, ::8],
               grad_blk0_c_fc_w_sub=blk.mlp.c_fc.weight.grad.numpy()[::8, ::8],
               token_ids=ids.astype(np.int64), grad_token_rows=g_tok[ids], grad_token_norm=np.linalg.norm(g_tok))
    for k, v in info.items():
        out["info_" + k] = v.detach().numpy().reshape(())
    return out


def main():
    torch.set_num_threads(8)
    save("f11_text_train_l2.npz", **text_case(load_reference()))


if __name__ == "__main__":
    main()
