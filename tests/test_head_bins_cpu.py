"""Host-side checks of the similarity head's bin-count bound (EBC_HEAD_MAX_BINS = 32): what the library refuses before
any device work, the wide text-gradient entry point's argument checks and workspace arithmetic, and the model's
construction with the reference's 20-bin reduction-32 table (tests/golden/f13_b32_r32_bins20.npz, written by
tests/golden/make_golden_bins20.py) and with one bin too many."""
import numpy as np
import pytest
import torch

from conftest import golden

EBC_E_ARG, EBC_E_UNSUPPORTED = -1, -3
_X = 0x1000          # a non-NULL pointer value; every call below is rejected before anything dereferences it


def _table():
    d = golden("f13_b32_r32_bins20.npz")
    return d, [(float(lo), float(hi)) for lo, hi in d["bins"]], [float(a) for a in d["anchors"]]


def test_header_states_the_cap():
    import os
    from conftest import REPO
    with open(os.path.join(REPO, "include", "ebc_hip.h")) as f:
        assert "#define EBC_HEAD_MAX_BINS 32" in f.read()
    from ebc_amd import model
    assert model.HEAD_MAX_BINS == 32


@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("NB", [0, 33])
def test_head_fwd_and_bwd_refuse_bin_counts_outside_1_to_32(NB, embed):
    from ebc_amd import _lib
    lib = _lib.load()
    assert lib.ebc_head_fwd(0, _X, _X, _X, _X, _X, _X, 8, 4, NB, embed, None) == EBC_E_UNSUPPORTED
    assert lib.ebc_head_bwd(0, 0, _X, _X, _X, _X, _X, _X, None, _X, None, None, 8, 4, NB, embed, None, 0,
                            None) == EBC_E_UNSUPPORTED


def _text_bwd_wide(lib, Z=_X, text=_X, ls=_X, anchors=_X, dl=_X, de=_X, dtext=_X, P=8, HW=4, NB=20, embed=512, dtype=0,
                   ws=_X, wsb=1 << 30):
    return lib.ebc_head_bwd_text_wide(dtype, Z, text, ls, anchors, dl, de, None, dtext, P, HW, NB, embed, ws, wsb, None)


@pytest.mark.parametrize("kw,rc", [
    (dict(Z=None), EBC_E_ARG), (dict(text=None), EBC_E_ARG), (dict(ls=None), EBC_E_ARG), (dict(anchors=None), EBC_E_ARG),
    (dict(dl=None), EBC_E_ARG), (dict(de=None), EBC_E_ARG), (dict(dtext=None), EBC_E_ARG), (dict(P=0), EBC_E_ARG),
    (dict(HW=0), EBC_E_ARG), (dict(P=8, HW=3), EBC_E_ARG), (dict(dtype=3), EBC_E_ARG), (dict(ws=None), EBC_E_ARG),
    (dict(wsb=(20 * 512 + 32) * 4 - 1), EBC_E_ARG), (dict(NB=33), EBC_E_UNSUPPORTED), (dict(NB=0), EBC_E_UNSUPPORTED),
    (dict(embed=768), EBC_E_UNSUPPORTED)])
def test_head_bwd_text_wide_rejects_without_device(kw, rc):
    from ebc_amd import _lib
    lib = _lib.load()
    assert _text_bwd_wide(lib, **kw) == rc


def test_head_bwd_text_wide_workspace_is_host_arithmetic():
    """ceil(P / 64) workgroup partials of NB * embed sums and 32 dot slots, in floats (include/ebc_hip.h)."""
    from ebc_amd import _lib
    lib = _lib.load()
    assert lib.ebc_head_bwd_text_wide_workspace_bytes(65, 20, 1024) == 2 * (20 * 1024 + 32) * 4
    assert lib.ebc_head_bwd_text_wide_workspace_bytes(16 * 49, 32, 512) == 13 * (32 * 512 + 32) * 4
    assert lib.ebc_head_bwd_text_wide_workspace_bytes(64, 1, 512) == (512 + 32) * 4
    for bad in ((0, 20, 512), (64, 33, 512), (64, 20, 768), (64, 0, 512)):
        assert lib.ebc_head_bwd_text_wide_workspace_bytes(*bad) == 0


def test_33_bins_is_an_error_at_construction():
    from ebc_amd.model import get_model
    bins = [(float(k), float(k)) for k in range(32)] + [(32.0, float("inf"))]
    anchors = [float(k) for k in range(32)] + [40.0]
    with pytest.raises(NotImplementedError, match="32"):
        get_model("clip_vit_b_32", 224, 32, bins, anchors, vit_layers=2, text_layers=2)
    get_model("clip_vit_b_32", 224, 32, bins[:31] + [(31.0, float("inf"))], anchors[:32], vit_layers=2, text_layers=2)


def test_the_references_20_bin_table_builds():
    from ebc_amd.model import get_model
    d, bins, anchors = _table()
    assert len(bins) == 20 and bins[0] == (0.0, 0.0) and bins[18] == (18.0, 18.0) and bins[19] == (19.0, float("inf"))
    m = get_model("clip_vit_b_32", 224, 32, bins, anchors, prompt_type="word", vit_layers=2, text_layers=2, weights_seed=0)
    assert m.text_features.shape == (20, 512) and bool(torch.isfinite(m.text_features).all())
    assert float(m.text_features.abs().max()) > 0
    ids = m._prompt_ids(torch.device("cpu")).numpy()
    assert ids.shape == d["prompt_tokens"].shape == (20, 77) and np.array_equal(ids, d["prompt_tokens"])
