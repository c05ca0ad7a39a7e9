"""Host-side checks of freeze_text_encoder=False (models/clip/model.py:37,100-115,201): the trainable set, the argument
checks, the new exports' validation without a device, and the text tower's own backward against the reference's
text-parameter gradients (tests/golden/f11_text_train_l2.npz, written by tests/golden/make_golden_text.py)."""
import numpy as np
import pytest
import torch

from conftest import ANCHORS_NWPU, BINS, golden, rel_l2

KW = dict(prompt_type="word", num_vpt=32, deep_vpt=True, vpt_drop=0.0, vit_layers=2, text_layers=2)


def _trainable(m):
    return sorted(n for n, p in m.named_parameters() if p.requires_grad)


def test_unfrozen_model_has_the_references_trainable_names():
    from ebc_amd.model import get_model
    d = golden("f11_text_train_l2.npz")
    m = get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, freeze_text_encoder=False, **KW)
    names = _trainable(m)
    assert names == [str(n) for n in d["trainable"]]
    assert sum(n.startswith("text_encoder.") for n in names) == 5 + 12 * 2
    assert "text_features" not in m.state_dict()                    # the buffer stays non-persistent


@pytest.mark.parametrize("backbone", ["clip_vit_b_16", "clip_vit_b_32", "clip_resnet50"])
def test_default_trainable_set_is_unchanged(backbone):
    """Frozen by default and with freeze_text_encoder=True; unfreezing adds exactly the text tower's parameters."""
    from ebc_amd.model import get_model
    size = 448 if backbone == "clip_resnet50" else 224
    kw = {k: v for k, v in KW.items() if backbone != "clip_resnet50" or k in ("prompt_type", "text_layers")}
    base = _trainable(get_model(backbone, size, 8, BINS, ANCHORS_NWPU, **kw))
    assert not any(n.startswith("text_encoder.") for n in base)
    assert _trainable(get_model(backbone, size, 8, BINS, ANCHORS_NWPU, freeze_text_encoder=True, **kw)) == base
    m = get_model(backbone, size, 8, BINS, ANCHORS_NWPU, freeze_text_encoder=False, **kw)
    text = sorted("text_encoder." + n for n, _ in m.text_encoder.named_parameters())
    assert _trainable(m) == sorted(base + text) and len(text) == 29


def test_given_text_features_with_a_trainable_tower_is_an_error():
    from ebc_amd.model import get_model
    txt = torch.zeros(len(BINS), 512)
    with pytest.raises(ValueError, match="freeze_text_encoder=False"):
        get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, freeze_text_encoder=False, text_features=txt, **KW)
    get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, text_features=txt, **KW)        # frozen: as before


EBC_E_ARG, EBC_E_UNSUPPORTED = -1, -3
_X = 0x1000          # a non-NULL pointer value; every call below is rejected before anything dereferences it


def _text_bwd(lib, Z=_X, text=_X, ls=_X, anchors=_X, dl=_X, de=_X, dtext=_X, P=8, HW=4, NB=5, embed=512, dtype=0, ws=_X,
              wsb=1 << 30):
    return lib.ebc_head_bwd_text(dtype, Z, text, ls, anchors, dl, de, None, dtext, P, HW, NB, embed, ws, wsb, None)


@pytest.mark.parametrize("kw,rc", [
    (dict(Z=None), EBC_E_ARG), (dict(text=None), EBC_E_ARG), (dict(ls=None), EBC_E_ARG), (dict(anchors=None), EBC_E_ARG),
    (dict(dl=None), EBC_E_ARG), (dict(de=None), EBC_E_ARG), (dict(dtext=None), EBC_E_ARG), (dict(P=0), EBC_E_ARG),
    (dict(HW=0), EBC_E_ARG), (dict(P=8, HW=3), EBC_E_ARG), (dict(dtype=3), EBC_E_ARG), (dict(ws=None), EBC_E_ARG),
    (dict(wsb=(5 * 512 + 16) * 4 - 1), EBC_E_ARG), (dict(NB=17), EBC_E_UNSUPPORTED), (dict(NB=0), EBC_E_UNSUPPORTED),
    (dict(embed=768), EBC_E_UNSUPPORTED)])
def test_head_bwd_text_rejects_without_device(kw, rc):
    from ebc_amd import _lib
    lib = _lib.load()
    assert _text_bwd(lib, **kw) == rc


def test_head_bwd_text_workspace_is_host_arithmetic():
    from ebc_amd import _lib
    lib = _lib.load()
    assert lib.ebc_head_bwd_text_workspace_bytes(16 * 784, 5, 512) == 196 * (5 * 512 + 16) * 4
    assert lib.ebc_head_bwd_text_workspace_bytes(65, 16, 1024) == 2 * (16 * 1024 + 16) * 4
    for bad in ((0, 5, 512), (64, 17, 512), (64, 5, 768), (64, 0, 512)):
        assert lib.ebc_head_bwd_text_workspace_bytes(*bad) == 0


def test_text_tower_backward_matches_the_reference_from_its_own_text_gradient():
    """The text tower is plain torch: fed the reference's d loss / d text_features, its backward must give the
    reference's text-parameter gradients (fp32 on both sides), and its forward the reference's text features.
    Bars: both sides are fp32 torch on the CPU and differ only in summation order (nn.MultiheadAttention there, explicit
    products here), i.e. by a few f32 roundoffs (6e-8) through two blocks: 1e-5 forward, 1e-4 on the gradients, which
    pass the LayerNorm backward's cancellation; a wrong mask, head split or activation is off by 1e-1 or more."""
    from ebc_amd.model import get_model
    d = golden("f11_text_train_l2.npz")
    m = get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, freeze_text_encoder=False, weights_seed=0, **KW)
    te = m.text_encoder
    tf = te(m._prompt_ids(torch.device("cpu")))
    assert rel_l2(tf, d["text_features"]) < 1e-5
    tf.backward(torch.from_numpy(d["grad_text_features"]))
    blk = te.transformer.resblocks[0]
    assert rel_l2(te.text_projection.grad[::2], d["grad_text_projection_rows2"]) < 1e-4
    assert rel_l2(te.ln_final.weight.grad, d["grad_ln_final_w"]) < 1e-4
    assert rel_l2(blk.attn.in_proj_weight.grad[::8, ::8], d["grad_blk0_in_proj_w_sub"]) < 1e-4
    assert rel_l2(blk.mlp.c_fc.weight.grad[::8, ::8], d["grad_blk0_c_fc_w_sub"]) < 1e-4
    ids = torch.from_numpy(d["token_ids"])
    assert rel_l2(te.token_embedding.weight.grad[ids], d["grad_token_rows"]) < 1e-4
    np.testing.assert_allclose(float(te.token_embedding.weight.grad.norm()), float(d["grad_token_norm"]), rtol=1e-4)
