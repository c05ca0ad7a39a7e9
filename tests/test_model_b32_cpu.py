"""Host-side checks of the clip_vit_b_32 surface of get_model (no GPU): construction at the three reductions,
state-dict keys / shapes against the reference's own list (F10 fixture), the prompt init bound, and the patch
argument of the synthetic weight generators."""
import math

import numpy as np
import pytest
import torch

from conftest import ANCHORS_NWPU, BINS, golden
from ebc_amd import synthetic as syn


def _b32(reduction, layers=2, **kw):
    from ebc_amd.model import get_model
    kw.setdefault("text_layers", 1)
    return get_model("clip_vit_b_32", 224, reduction, BINS, ANCHORS_NWPU, prompt_type="word", num_vpt=32, deep_vpt=True,
                     vpt_drop=0.0, vit_layers=layers, **kw)


@pytest.mark.parametrize("reduction", [8, 16, 32])
def test_b32_constructs_at_every_reduction(reduction):
    m = _b32(reduction)
    assert m.encoder_reduction == 32 and m.reduction == reduction
    assert m.image_encoder.conv1.weight.shape == (768, 3, 32, 32)
    assert m.image_encoder.positional_embedding.shape == (7 * 7 + 1, 768)
    assert m.image_encoder.patch_size == (32, 32)
    assert m.channels == 768 and m.clip_embed_dim == 512
    assert all(not p.requires_grad for p in m.image_encoder.parameters())


def test_b32_rejects_other_reductions_and_b16_rule_is_unchanged():
    from ebc_amd.model import get_model
    with pytest.raises(NotImplementedError):
        _b32(4)
    kw = dict(prompt_type="word", num_vpt=32, deep_vpt=True, vpt_drop=0.0, vit_layers=1, text_layers=1)
    for r in (16, 8):
        assert get_model("clip_vit_b_16", 224, r, BINS, ANCHORS_NWPU, **kw).encoder_reduction == 16
    for r in (32, 4):
        with pytest.raises(NotImplementedError):
            get_model("clip_vit_b_16", 224, r, BINS, ANCHORS_NWPU, **kw)


@pytest.mark.parametrize("fixture", ["f10_b32_l2.npz", "f10_b32_l12.npz"])
def test_b32_state_dict_equals_the_reference_list(fixture):
    d = golden(fixture)
    m = _b32(8, layers=int(d["layers"]), text_layers=12)
    sd = m.state_dict()
    want = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(d["state_keys"], d["state_shapes"])}
    assert sorted(sd.keys()) == sorted(want.keys())
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    assert want["image_encoder.conv1.weight"] == (768, 3, 32, 32)
    assert want["image_encoder.positional_embedding"] == (50, 768)


def test_b32_vpt_init_bound():
    """models/clip/model.py:70-71: U(+-sqrt(6 / (3 * patch + 768))), patch 32."""
    bound = math.sqrt(6.0 / (3 * 32 + 768))
    torch.manual_seed(3)
    m = _b32(8, layers=3)
    for i in range(3):
        v = getattr(m, f"vpt_{i}").detach()
        assert v.shape == (32, 768)
        assert float(v.abs().max()) <= bound
        assert float(v.abs().max()) > 0.98 * bound          # 24576 draws: the largest is within 2 % of the bound
    # the synthetic prompts follow the same law; those of patch 16 keep the wider B/16 bound
    s32 = syn.trainable_state(0, layers=1, patch=32)["vpt_0"]
    s16 = syn.trainable_state(0, layers=1)["vpt_0"]
    assert float(np.abs(s32).max()) <= bound < float(np.abs(s16).max()) <= math.sqrt(6.0 / (3 * 16 + 768))


def test_b32_synthetic_weights_load():
    m = _b32(8, weights_seed=0)
    sd = syn.full_state(0, layers=2, text_layers=1, patch=32)
    assert sd["image_encoder.conv1.weight"].shape == (768, 3, 32, 32)
    assert sd["image_encoder.positional_embedding"].shape == (50, 768)
    np.testing.assert_array_equal(m.image_encoder.conv1.weight.numpy(), sd["image_encoder.conv1.weight"])
    np.testing.assert_array_equal(m.vpt_1.detach().numpy(), sd["vpt_1"])


def test_synthetic_patch_16_is_the_default_bit_for_bit():
    for a, b in ((syn.vit_state(0, 2, 224, patch=16), syn.vit_state(0, 2, 224)),
                 (syn.trainable_state(0, 2, patch=16), syn.trainable_state(0, 2)),
                 (syn.full_state(0, 2, 1, patch=16), syn.full_state(0, 2, 1))):
        assert list(a.keys()) == list(b.keys())
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    # tensors whose shape the patch size does not touch are the same arrays at patch 32
    a, b = syn.vit_state(0, 1, patch=32), syn.vit_state(0, 1)
    for k in a:
        if k.endswith("conv1.weight") or k.endswith("positional_embedding"):
            assert a[k].shape != b[k].shape
        else:
            assert np.array_equal(a[k], b[k]), k


def test_vit_l_14_is_still_refused_with_what_is_missing():
    from ebc_amd.model import get_model
    with pytest.raises(NotImplementedError, match=r"width 1024.*patch 14.*x1\.75"):
        get_model("clip_vit_l_14", 224, 7, BINS, ANCHORS_NWPU, prompt_type="word", num_vpt=32, deep_vpt=True,
                  vpt_drop=0.0)


def test_b32_workspace_export_is_host_arithmetic():
    """ebc_vit_workspace_bytes_p: patch 16 equals the unchanged export; patch 32 has 4x fewer patch tokens; other
    patch sizes answer 0."""
    from ebc_amd import _lib
    L = _lib.load()
    for dt in (0, 1, 2):
        for tr in (0, 1):
            assert L.ebc_vit_workspace_bytes_p(16, 224, 224, 16, 12, 32, dt, tr) == \
                L.ebc_vit_workspace_bytes(16, 224, 224, 12, 32, dt, tr)
    b16 = L.ebc_vit_workspace_bytes_p(16, 224, 224, 16, 12, 32, 1, 1)
    b32 = L.ebc_vit_workspace_bytes_p(16, 224, 224, 32, 12, 32, 1, 1)
    assert 12 * 16 * 82 * 768 * 4 < b32 < b16 / 2              # 82 token rows a crop against 229
    assert L.ebc_vit_workspace_bytes_p(16, 224, 224, 14, 12, 32, 1, 1) == 0
