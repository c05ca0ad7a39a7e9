"""Host-side checks of the HIP text tower (text_tower="hip", include/ebc_hip.h ebc_text_*): every argument rule of the
new exports answers before any device work, the workspace size is host arithmetic, the prompt index (Lt, the inverted
index of the embedding gather) agrees with a numpy restatement, and the keyword's CPU behaviour."""
import numpy as np
import pytest
import torch

import _text_refs as TR
from conftest import ANCHORS_NWPU, BINS

KW = dict(prompt_type="word", num_vpt=32, deep_vpt=True, vpt_drop=0.0, vit_layers=2, text_layers=2)
EBC_E_ARG, EBC_E_UNSUPPORTED = -1, -3
_X = 0x1000          # a non-NULL pointer value; every call below is rejected before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    from ebc_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ kernels
def _ca_fwd(lib, qkv=_X, out=_X, lse=_X, B=2, L=14, H=8, dtype=1):
    return lib.ebc_attention_causal_fwd(dtype, qkv, out, lse, B, L, H, None)


def _ca_bwd(lib, qkv=_X, dout=_X, out=_X, lse=_X, dqkv=_X, B=2, L=14, H=8, dtype=1):
    return lib.ebc_attention_causal_bwd(dtype, qkv, dout, out, lse, None, dqkv, B, L, H, None)


@pytest.mark.parametrize("kw,rc", [(dict(qkv=None), EBC_E_ARG), (dict(out=None), EBC_E_ARG), (dict(B=0), EBC_E_ARG),
                                   (dict(H=0), EBC_E_ARG), (dict(L=0), EBC_E_ARG), (dict(dtype=3), EBC_E_ARG),
                                   (dict(L=78), EBC_E_UNSUPPORTED), (dict(L=229), EBC_E_UNSUPPORTED)])
def test_causal_attention_fwd_rejects_without_device(lib, kw, rc):
    assert _ca_fwd(lib, **kw) == rc


@pytest.mark.parametrize("kw,rc", [(dict(qkv=None), EBC_E_ARG), (dict(dout=None), EBC_E_ARG), (dict(out=None), EBC_E_ARG),
                                   (dict(lse=None), EBC_E_ARG), (dict(dqkv=None), EBC_E_ARG), (dict(B=0), EBC_E_ARG),
                                   (dict(L=-1), EBC_E_ARG), (dict(dtype=-1), EBC_E_ARG), (dict(L=78), EBC_E_UNSUPPORTED)])
def test_causal_attention_bwd_rejects_without_device(lib, kw, rc):
    assert _ca_bwd(lib, **kw) == rc


@pytest.mark.parametrize("D,rc", [(512, None), (768, None), (256, EBC_E_UNSUPPORTED), (1024, EBC_E_UNSUPPORTED),
                                  (0, EBC_E_UNSUPPORTED)])
def test_layernorm_widths(lib, D, rc):
    """D in {512, 768} passes the width rule (the NULL x then answers EBC_E_ARG); anything else is EBC_E_UNSUPPORTED, in
    the forward, the backward and the parameter gradient."""
    want = EBC_E_UNSUPPORTED if rc else EBC_E_ARG
    if rc:
        assert lib.ebc_layernorm_fwd(1, _X, 0, 0, 0, _X, _X, _X, None, _X, _X, 8, D, None) == rc
        assert lib.ebc_layernorm_bwd(1, 0, _X, _X, 0, 0, 0, _X, _X, _X, None, _X, None, 8, D, None) == rc
        assert lib.ebc_layernorm_param_grad(1, 0, _X, _X, _X, _X, _X, _X, 8, D, None) == rc
    else:
        assert lib.ebc_layernorm_fwd(1, None, 0, 0, 0, _X, _X, _X, None, _X, _X, 8, D, None) == want
        assert lib.ebc_layernorm_bwd(1, 0, None, _X, 0, 0, 0, _X, _X, _X, None, _X, None, 8, D, None) == want
        assert lib.ebc_layernorm_param_grad(1, 0, None, _X, _X, _X, _X, _X, 8, D, None) == want


def test_row_sums_reject_without_device(lib):
    for bad in range(6):                                  # dy, x, mean, rstd, dgamma, dbeta
        a = [_X] * 6
        a[bad] = None
        assert lib.ebc_layernorm_param_grad(1, 0, *a, 8, 512, None) == EBC_E_ARG
    assert lib.ebc_layernorm_param_grad(1, 0, *([_X] * 6), 0, 512, None) == EBC_E_ARG
    assert lib.ebc_layernorm_param_grad(3, 0, *([_X] * 6), 8, 512, None) == EBC_E_ARG
    assert lib.ebc_colsum(1, 0, None, _X, 8, 512, None) == EBC_E_ARG
    assert lib.ebc_colsum(1, 0, _X, None, 8, 512, None) == EBC_E_ARG
    assert lib.ebc_colsum(1, 0, _X, _X, 0, 512, None) == EBC_E_ARG
    assert lib.ebc_colsum(1, 0, _X, _X, 8, 0, None) == EBC_E_ARG
    assert lib.ebc_colsum(3, 0, _X, _X, 8, 512, None) == EBC_E_ARG


def _emb_fwd(lib, tok=_X, pos=_X, ids=_X, x=_X, NB=5, Lt=9, width=512, vocab=49408):
    return lib.ebc_text_embed_fwd(tok, pos, ids, x, NB, Lt, width, vocab, None)


def _emb_bwd(lib, dx=_X, uniq=_X, offs=_X, rows=_X, nu=12, dtok=_X, dpos=_X, NB=5, Lt=9, ctx=77, width=512, vocab=49408):
    return lib.ebc_text_embed_bwd(dx, uniq, offs, rows, nu, dtok, dpos, NB, Lt, ctx, width, vocab, None)


@pytest.mark.parametrize("kw,rc", [(dict(tok=None), EBC_E_ARG), (dict(pos=None), EBC_E_ARG), (dict(ids=None), EBC_E_ARG),
                                   (dict(x=None), EBC_E_ARG), (dict(vocab=0), EBC_E_ARG), (dict(NB=0), EBC_E_UNSUPPORTED),
                                   (dict(NB=17), EBC_E_UNSUPPORTED), (dict(Lt=0), EBC_E_UNSUPPORTED),
                                   (dict(Lt=78), EBC_E_UNSUPPORTED), (dict(width=768), EBC_E_UNSUPPORTED)])
def test_embed_fwd_rejects_without_device(lib, kw, rc):
    assert _emb_fwd(lib, **kw) == rc


@pytest.mark.parametrize("kw,rc", [(dict(dx=None), EBC_E_ARG), (dict(uniq=None), EBC_E_ARG), (dict(offs=None), EBC_E_ARG),
                                   (dict(rows=None), EBC_E_ARG), (dict(dtok=None), EBC_E_ARG), (dict(dpos=None), EBC_E_ARG),
                                   (dict(vocab=-1), EBC_E_ARG), (dict(nu=0), EBC_E_ARG), (dict(nu=46), EBC_E_ARG),
                                   (dict(ctx=8), EBC_E_ARG), (dict(ctx=78), EBC_E_ARG), (dict(NB=17), EBC_E_UNSUPPORTED),
                                   (dict(Lt=78), EBC_E_UNSUPPORTED), (dict(width=256), EBC_E_UNSUPPORTED)])
def test_embed_bwd_rejects_without_device(lib, kw, rc):
    assert _emb_bwd(lib, **kw) == rc


# ------------------------------------------------------------------------------------------------ the tower
def _structs(layers=2, embed=512, width=512, heads=8, vocab=49408, context=77, hole=None, grads=False):
    """Weight / gradient structs whose every pointer is _X, except the field named by `hole` ("top:<name>" or
    "layer:<name>", NULL)."""
    from ebc_amd import _lib
    arr = (_lib.EbcTextLayer * layers)()
    for l in range(layers):
        for f in _lib._TEXT_LAYER_FIELDS:
            setattr(arr[l], f, None if hole == f"layer:{f}" and l == layers - 1 else _X)
    top = {n: (None if hole == f"top:{n}" else _X) for n in ("token_embedding", "positional_embedding", "ln_final_g",
                                                            "ln_final_b", "text_projection")}
    if grads:
        return _lib.EbcTextGrads(layer=None if hole == "layers" else arr, **top), arr
    return _lib.EbcTextWeights(layers=layers, width=width, heads=heads, embed=embed, vocab=vocab, context=context,
                               layer=None if hole == "layers" else arr, **top), arr


def _fwd(lib, w, ids=_X, eot=_X, NB=5, Lt=9, dtype=1, training=1, ws=_X, wsb=1 << 40, feat=_X):
    import ctypes
    return lib.ebc_text_forward(ctypes.byref(w) if w is not None else None, ids, eot, NB, Lt, dtype, training, ws, wsb, feat,
                                None)


def _bwd(lib, w, g, ids=_X, eot=_X, uniq=_X, offs=_X, rows=_X, nu=12, NB=5, Lt=9, dtype=1, ws=_X, wsb=1 << 40, df=_X):
    import ctypes
    return lib.ebc_text_backward(ctypes.byref(w) if w is not None else None, ctypes.byref(g) if g is not None else None,
                                 ids, eot, uniq, offs, rows, nu, NB, Lt, dtype, ws, wsb, df, None)


HOLES = ["layers"] + [f"top:{n}" for n in ("token_embedding", "positional_embedding", "ln_final_g", "ln_final_b",
                                           "text_projection")] + \
        [f"layer:{n}" for n in ("w_qkv", "b_qkv", "w_out", "b_out", "w_fc", "b_fc", "w_proj", "b_proj", "ln1_g", "ln1_b",
                                "ln2_g", "ln2_b")]


@pytest.mark.parametrize("hole", HOLES)
def test_text_tower_rejects_null_fields_without_device(lib, hole):
    w, k1 = _structs()
    g, k2 = _structs(grads=True)
    wb, k3 = _structs(hole=hole)
    gb, k4 = _structs(hole=hole, grads=True)
    assert _fwd(lib, wb) == EBC_E_ARG
    assert _bwd(lib, wb, g) == EBC_E_ARG
    assert _bwd(lib, w, gb) == EBC_E_ARG


@pytest.mark.parametrize("kw,rc", [(dict(ids=None), EBC_E_ARG), (dict(eot=None), EBC_E_ARG), (dict(ws=None), EBC_E_ARG),
                                   (dict(feat=None), EBC_E_ARG), (dict(dtype=3), EBC_E_ARG), (dict(wsb="short"), EBC_E_ARG),
                                   (dict(NB=0), EBC_E_UNSUPPORTED), (dict(NB=17), EBC_E_UNSUPPORTED),
                                   (dict(Lt=0), EBC_E_UNSUPPORTED), (dict(Lt=78), EBC_E_UNSUPPORTED)])
def test_text_forward_rejects_without_device(lib, kw, rc):
    w, keep = _structs()
    if kw.get("wsb") == "short":
        kw = dict(wsb=lib.ebc_text_workspace_bytes(5, 9, 2, 512, 1, 1) - 1)
    assert _fwd(lib, w, **kw) == rc
    assert _fwd(lib, None) == EBC_E_ARG


@pytest.mark.parametrize("kw,rc", [(dict(ids=None), EBC_E_ARG), (dict(eot=None), EBC_E_ARG), (dict(uniq=None), EBC_E_ARG),
                                   (dict(offs=None), EBC_E_ARG), (dict(rows=None), EBC_E_ARG), (dict(ws=None), EBC_E_ARG),
                                   (dict(df=None), EBC_E_ARG), (dict(nu=0), EBC_E_ARG), (dict(nu=46), EBC_E_ARG),
                                   (dict(dtype=-1), EBC_E_ARG), (dict(wsb="short"), EBC_E_ARG),
                                   (dict(NB=17), EBC_E_UNSUPPORTED), (dict(Lt=78), EBC_E_UNSUPPORTED)])
def test_text_backward_rejects_without_device(lib, kw, rc):
    w, k1 = _structs()
    g, k2 = _structs(grads=True)
    if kw.get("wsb") == "short":
        kw = dict(wsb=lib.ebc_text_workspace_bytes(5, 9, 2, 512, 1, 1) - 1)
    assert _bwd(lib, w, g, **kw) == rc
    assert _bwd(lib, w, None) == EBC_E_ARG and _bwd(lib, None, g) == EBC_E_ARG


@pytest.mark.parametrize("kw,rc", [(dict(embed=768), EBC_E_UNSUPPORTED), (dict(embed=0), EBC_E_UNSUPPORTED),
                                   (dict(width=768), EBC_E_UNSUPPORTED), (dict(heads=12), EBC_E_ARG),
                                   (dict(layers=0), EBC_E_ARG), (dict(vocab=0), EBC_E_ARG), (dict(context=8), EBC_E_ARG),
                                   (dict(context=78), EBC_E_ARG)])
def test_text_tower_rejects_bad_dimensions_without_device(lib, kw, rc):
    w, k1 = _structs(**kw)
    g, k2 = _structs(grads=True)
    assert _fwd(lib, w) == rc and _bwd(lib, w, g) == rc


def test_text_workspace_is_host_arithmetic(lib):
    f = lib.ebc_text_workspace_bytes
    base = f(5, 9, 2, 512, 1, 1)
    assert base > 0
    assert f(6, 9, 2, 512, 1, 1) > base and f(16, 9, 2, 512, 1, 1) > f(6, 9, 2, 512, 1, 1)         # monotone in NB
    assert f(5, 10, 2, 512, 1, 1) > base and f(5, 77, 2, 512, 1, 1) > f(5, 10, 2, 512, 1, 1)         # ... in Lt
    assert f(5, 9, 3, 512, 1, 1) > base and f(5, 9, 12, 512, 1, 1) > f(5, 9, 3, 512, 1, 1)           # ... in layers
    assert f(5, 9, 2, 1024, 1, 1) > base and f(5, 9, 2, 512, 0, 1) > base                            # embed, f32
    assert 0 < f(5, 9, 12, 512, 1, 0) < f(5, 9, 12, 512, 1, 1) / 4                                   # eval keeps one layer
    for bad in ((0, 9, 2, 512, 1, 1), (17, 9, 2, 512, 1, 1), (5, 0, 2, 512, 1, 1), (5, 78, 2, 512, 1, 1),
                (5, 9, 0, 512, 1, 1), (5, 9, 2, 768, 1, 1), (5, 9, 2, 512, 3, 1)):
        assert f(*bad) == 0


# ------------------------------------------------------------------------------------------------ the prompt index
def _check_index(tokens, full=False):
    from ebc_amd.text import prompt_index
    got = prompt_index(tokens, full)
    t = np.asarray(tokens)
    want = TR.prompt_index(t)
    if full:
        want.update(Lt=t.shape[1], ids=t.astype(np.int32), **TR.inverted_index(t))
    assert got["Lt"] == want["Lt"]
    for k in ("eot", "ids", "uniq", "offs", "rows"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    # the index inverts the gather: list u holds exactly the positions of uniq[u], ascending, and the lists tile rows
    flat = got["ids"].reshape(-1)
    assert np.array_equal(np.sort(got["rows"]), np.arange(flat.size)) and np.all(np.diff(got["uniq"]) > 0)
    for u, (a, b) in enumerate(zip(got["offs"][:-1], got["offs"][1:])):
        r = got["rows"][a:b]
        assert b > a and np.all(flat[r] == got["uniq"][u]) and np.all(np.diff(r) > 0)
    return got


def test_prompt_index_of_the_count_prompts():
    """The bin prompts repeat ids (SOT, "there", "are", "people", "."): Lt = max EOT + 1, far below 77."""
    from ebc_amd.text import format_count, prompt_tokens
    for ptype in ("word", "number"):
        bins = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 5), (6, 8), (9, float("inf"))]
        toks = prompt_tokens([format_count(b[0] if b[0] == b[1] else b, ptype) for b in bins])
        ix = _check_index(toks.numpy())
        assert 7 <= ix["Lt"] <= 14 and len(ix["uniq"]) < ix["ids"].size
        assert np.array_equal(ix["eot"], toks.argmax(-1).numpy())
        _check_index(toks.numpy(), full=True)


def test_prompt_index_of_a_full_context_prompt():
    """One prompt whose EOT sits at token 76: Lt = 77."""
    toks = np.zeros((3, 77), np.int64)
    toks[:, 0] = 49406
    toks[0, 1:76] = np.arange(1000, 1075)
    toks[0, 76] = 49407
    toks[1, 1:4], toks[1, 4] = [320, 533, 320], 49407
    toks[2, 1], toks[2, 2] = 320, 49407
    ix = _check_index(toks)
    assert ix["Lt"] == 77 and list(ix["eot"]) == [76, 4, 2]


# ------------------------------------------------------------------------------------------------ the keyword
def test_unknown_text_tower_is_an_error():
    from ebc_amd.model import get_model
    from ebc_amd.text import CLIPTextEncoder
    with pytest.raises(ValueError, match="text_tower"):
        get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, text_tower="bogus", **KW)
    with pytest.raises(ValueError, match="text_tower"):
        get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, freeze_text_encoder=False, text_tower="bogus", **KW)
    with pytest.raises(ValueError, match="impl"):
        CLIPTextEncoder(layers=1, impl="bogus")


def test_hip_tower_on_cpu_parameters_is_the_torch_tower():
    """text_tower="hip" with the parameters on the CPU runs the torch restatement: features bit-identical, the same
    trainable names and state-dict keys; the default is "torch", and a frozen model ignores the choice."""
    from ebc_amd.model import get_model
    mk = lambda **kw: get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, weights_seed=0, **KW, **kw)
    a, b = mk(freeze_text_encoder=False), mk(freeze_text_encoder=False, text_tower="hip")
    assert a.text_tower == "torch" and a.text_encoder.impl == "torch" and b.text_encoder.impl == "hip"
    assert mk(text_tower="hip").text_encoder.impl == "torch"
    ids = a._prompt_ids(torch.device("cpu"))
    fa, fb = a.text_encoder(ids), b.text_encoder(ids)
    assert torch.equal(fa, fb) and torch.equal(a.text_features, b.text_features) and fb.requires_grad
    assert list(a.state_dict()) == list(b.state_dict())
    assert [n for n, p in a.named_parameters() if p.requires_grad] == [n for n, p in b.named_parameters() if p.requires_grad]
