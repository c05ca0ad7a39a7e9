"""The HIP text tower (CLIPTextEncoder(impl="hip"): ebc_text_forward / ebc_text_backward) against the torch restatement
the fixtures F6 / F11 pin, run in float64 on the CPU with autograd: the features and every parameter gradient.

The bars are relative to PyTorch's own error on the same device: per tensor, the HIP tower's rel-L2 distance to the
float64 run is at most 4x (fp32; MFMA chains and split-K sums accumulate in other orders) or 2x (fp16 / bf16 under
torch.autocast, the project's precedent for clip_resnet50) the torch tower's distance to that run.  Both are measured
here and printed as "RATIO <tensor> <hip error / (factor x torch error)>".  A tensor, or rows of one, whose float64
gradient is identically zero must be exactly zero."""
import functools

import numpy as np
import pytest
import torch

from ebc_amd import synthetic as syn
from ebc_amd.text import CLIPTextEncoder

pytestmark = pytest.mark.gpu
F64 = torch.float64
LAYERS = 2
SOT, EOT = 49406, 49407


def _tokens(eots, seed):
    """Prompts with the EOT (the largest id) at the given positions; SOT first, a shared second token, repeated ids."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(len(eots), 77, dtype=torch.int32)
    for k, e in enumerate(eots):
        t[k, 0] = SOT
        t[k, 1:e] = torch.randint(300, 40000, (e - 1,), generator=g).to(torch.int32)
        if e > 2:
            t[k, 1] = 997
        if e > 5:
            t[k, 4] = t[k, 2]
        t[k, e] = EOT
    return t


SETS = {"lt14": (6, 9, 13), "lt77": (6, 76, 9, 13, 7)}


def _encoder(embed, impl, device, dtype=torch.float32):
    enc = CLIPTextEncoder(embed, 77, 49408, 512, 8, LAYERS, impl=impl)
    sd = {k[len("text_encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in syn.text_state(0, LAYERS, embed).items()}
    enc.load_state_dict(sd)
    return enc.to(device=device, dtype=dtype)


def _dfeat(nb, embed):
    return torch.randn(nb, embed, generator=torch.Generator().manual_seed(7), dtype=F64)


def _run(enc, tokens, dfeat, autocast=None):
    """features and every parameter gradient (CPU tensors) of one forward + backward."""
    dev = enc.positional_embedding.device
    enc.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        f = enc(tokens.to(dev))
    f.backward(dfeat.to(device=dev, dtype=f.dtype))
    out = {"features": f.detach().cpu()}
    out.update({n: p.grad.detach().cpu() for n, p in enc.named_parameters()})
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, embed):
    """The float64 CPU run (computed once per prompt set and width, never modified)."""
    tokens = _tokens(SETS[name], 3)
    return _run(_encoder(embed, "torch", "cpu", F64), tokens, _dfeat(len(SETS[name]), embed))


@functools.lru_cache(maxsize=None)
def _torch_gpu(name, embed, autocast):
    tokens = _tokens(SETS[name], 3)
    return _run(_encoder(embed, "torch", "cuda"), tokens, _dfeat(len(SETS[name]), embed), autocast)


def _err(a, ref):
    a, ref = a.to(F64), ref.to(F64)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def _compare(tag, hip, tor, ref, factor):
    bad = []
    for n in ref:
        e_hip, e_tor = _err(hip[n], ref[n]), _err(tor[n], ref[n])
        ratio = e_hip / (factor * e_tor) if e_tor > 0 else (0.0 if e_hip == 0 else float("inf"))
        print(f"RATIO {tag}.{n} {ratio:.4f}   (hip {e_hip:.3e}, torch {e_tor:.3e})")
        if not ratio <= 1.0:
            bad.append((n, e_hip, e_tor))
    assert not bad, bad


def _assert_exact_zeros(res, ref, Lt):
    """Rows whose float64 gradient is identically zero: positional rows >= Lt and unused token rows."""
    pos, tok = ref["positional_embedding"], ref["token_embedding.weight"]
    assert bool((pos[Lt:] == 0).all()) and bool((pos[:Lt].abs().amax(1) > 0).all())
    assert bool((res["positional_embedding"][Lt:] == 0).all())
    unused = tok.abs().amax(1) == 0
    assert 49408 - 77 * 5 < int(unused.sum()) < 49408
    assert bool((res["token_embedding.weight"][unused] == 0).all())
    for n, g in res.items():
        assert bool(torch.isfinite(g).all()), n


@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("name", ["lt14", "lt77"])
def test_fp32_parity_with_the_float64_tower(name, embed):
    tokens = _tokens(SETS[name], 3)
    Lt = max(SETS[name]) + 1
    ref, tor = _reference(name, embed), _torch_gpu(name, embed, None)
    enc = _encoder(embed, "hip", "cuda")
    hip = _run(enc, tokens, _dfeat(len(SETS[name]), embed))
    assert enc._hip_index[2]["ids"].shape == (len(SETS[name]), Lt)
    assert all(g.dtype == torch.float32 for g in hip.values())
    _compare(f"text_fp32[{name},{embed}]", hip, tor, ref, 4.0)
    _assert_exact_zeros(hip, ref, Lt)
    again = _run(enc, tokens, _dfeat(len(SETS[name]), embed))          # no atomics anywhere: bit-identical
    assert all(torch.equal(hip[n], again[n]) for n in hip)


@pytest.mark.parametrize("autocast", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name,embed", [("lt14", 512), ("lt77", 512), ("lt14", 1024)])
def test_autocast_parity_with_the_torch_tower(name, embed, autocast):
    tokens = _tokens(SETS[name], 3)
    ref, tor = _reference(name, embed), _torch_gpu(name, embed, autocast)
    hip = _run(_encoder(embed, "hip", "cuda"), tokens, _dfeat(len(SETS[name]), embed), autocast)
    assert all(g.dtype == torch.float32 for n, g in hip.items() if n != "features")
    _compare(f"text_{str(autocast)[6:]}[{name},{embed}]", hip, tor, ref, 2.0)
    _assert_exact_zeros(hip, ref, max(SETS[name]) + 1)


def test_truncation_to_lt_is_exact():
    """The Lt = 14 set run over all 77 tokens: features and every gradient inside the fp32 bar, rows 14 .. 76 of the
    positional gradient exact zeros in both."""
    name, embed = "lt14", 512
    tokens = _tokens(SETS[name], 3)
    ref, tor = _reference(name, embed), _torch_gpu(name, embed, None)
    enc = _encoder(embed, "hip", "cuda")
    short = _run(enc, tokens, _dfeat(3, embed))
    enc.hip_full_context = True
    full = _run(enc, tokens, _dfeat(3, embed))
    assert enc._hip_index[2]["ids"].shape == (3, 77)
    _compare("text_full_context", full, tor, ref, 4.0)
    for res in (short, full):
        _assert_exact_zeros(res, ref, 14)


@pytest.mark.parametrize("autocast", [None, torch.float16], ids=["f32", "f16"])
def test_eval_features_equal_the_training_forward(autocast):
    tokens = _tokens(SETS["lt14"], 3).cuda()
    enc = _encoder(512, "hip", "cuda")
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        f_train = enc(tokens)
        assert f_train.requires_grad and f_train.dtype == torch.float32
        with torch.no_grad():
            f_nograd = enc(tokens)
        enc.eval()
        with torch.no_grad():
            f_eval = enc(tokens)
    assert not f_nograd.requires_grad and torch.equal(f_train.detach(), f_nograd) and torch.equal(f_nograd, f_eval)
    seen = []
    h = enc.register_forward_hook(lambda mod, inp, out: seen.append(out.shape))     # forward dispatches: hooks fire
    enc(tokens)
    h.remove()
    assert seen == [torch.Size([3, 512])]
