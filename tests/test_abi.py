"""CPU checks of the C-ABI boundary: libebc_hip.so loads, exports every symbol include/ebc_hip.h
declares, the ctypes signature table covers them, and host-only entry points answer (no device work)."""
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "ebc_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ebc_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from ebc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "clip-ebc_amd")])
    return _lib.load()


def test_header_declares_the_hot_path():
    fns = declared_functions()
    for f in ("ebc_dace_loss", "ebc_gemm", "ebc_vit_forward", "ebc_vit_backward", "ebc_attention_fwd",
              "ebc_attention_bwd", "ebc_head_fwd", "ebc_head_bwd", "ebc_layernorm_fwd", "ebc_layernorm_bwd"):
        assert f in fns


def test_library_exports_every_declared_symbol(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(REPO, "clip-ebc_amd", "lib", "libebc_hip.so")]).decode()
    exported = set(re.findall(r"\bT (ebc_[a-z0-9_]+)", out))
    missing = [f for f in declared_functions() if f not in exported]
    assert not missing, missing
    for f in declared_functions():
        getattr(lib, f)


def test_ctypes_table_matches_header(lib):
    from ebc_amd import _lib
    assert set(_lib.SIGNATURES) == set(declared_functions())


def test_host_only_entry_points(lib):
    assert lib.ebc_version() >= 1
    # workspace sizing is pure host arithmetic
    assert lib.ebc_dace_workspace_bytes(16, 600, 224, 8) >= 4 * 58 * 600
    b_train = lib.ebc_vit_workspace_bytes(16, 224, 224, 12, 32, 1, 1)
    b_eval = lib.ebc_vit_workspace_bytes(16, 224, 224, 12, 32, 1, 0)
    assert b_train > 12 * 16 * 229 * 768 * 4 and b_eval < b_train / 4


def test_argument_validation_without_device(lib):
    # rejected before any device work
    assert lib.ebc_gemm(1, 0, 0, None, None, None, None, None, None, 16, 64, 64, None) == -1
    assert lib.ebc_dace_loss(None, None, None, 0, None, None, None, None, None, 0, 5, 224, 8, 0, 0, 1.0, 0.1,
                             0.01, 10.0, 100, 1e-9, 10, *([None] * 7), 0, None) == -1


EBC_E_ARG = -1
_X = 0x1000          # a non-NULL pointer value; every call below is rejected before anything dereferences it
F32, F16 = 0, 1


def _ln_fwd(lib, x=_X, rpg=0, gs=0, go=0, gamma=_X, beta=_X, out=_X, outf=None, mean=_X, rstd=_X, M=8):
    return lib.ebc_layernorm_fwd(F16, x, rpg, gs, go, gamma, beta, out, outf, mean, rstd, M, 768, None)


def _ln_bwd(lib, dy=_X, x=_X, rpg=0, gs=0, go=0, mean=_X, rstd=_X, gamma=_X, dx_in=None, dx_out=_X, dxt=None, M=8):
    return lib.ebc_layernorm_bwd(F16, 0, dy, x, rpg, gs, go, mean, rstd, gamma, dx_in, dx_out, dxt, M, 768, None)


@pytest.mark.parametrize("kw", [dict(x=None), dict(gamma=None), dict(beta=None), dict(out=None, outf=None),
                                dict(rstd=None), dict(rpg=4, gs=7, go=-1), dict(rpg=4, gs=7, go=4),
                                dict(rpg=196, gs=229, go=34), dict(rpg=1, gs=0, go=0)])
def test_layernorm_fwd_rejects_without_device(lib, kw):
    """NULL x / gamma / beta, no output at all, mean without rstd, a row map that leaves its group."""
    assert _ln_fwd(lib, **kw) == EBC_E_ARG


@pytest.mark.parametrize("kw", [dict(dy=None), dict(x=None), dict(mean=None), dict(rstd=None), dict(gamma=None),
                                dict(dx_out=None), dict(rpg=4, gs=7, go=-1), dict(rpg=49, gs=82, go=34)])
def test_layernorm_bwd_rejects_without_device(lib, kw):
    assert _ln_bwd(lib, **kw) == EBC_E_ARG


def test_attention_rejects_without_device(lib):
    """NULL operands on every path; delta_ws == NULL on the paths that use it: f32 at any L (the dQ kernel publishes
    delta for the dK/dV kernel) and every dtype at L > 256 (the streamed pair)."""
    for dt in (0, 1, 2):
        for L in (5, 229, 300):
            assert lib.ebc_attention_fwd(dt, None, _X, _X, 1, L, 2, None) == EBC_E_ARG
            assert lib.ebc_attention_fwd(dt, _X, None, _X, 1, L, 2, None) == EBC_E_ARG
            for bad in range(5):             # qkv, dout, out, lse, dqkv
                a = [_X] * 6
                a[bad if bad < 4 else 5] = None
                assert lib.ebc_attention_bwd(dt, *a, 1, L, 2, None) == EBC_E_ARG, (dt, L, bad)
    for dt, L in ((0, 5), (0, 200), (0, 300), (1, 300), (2, 257)):
        assert lib.ebc_attention_bwd(dt, _X, _X, _X, _X, None, _X, 1, L, 2, None) == EBC_E_ARG, (dt, L)


def _head_fwd(lib, Z=_X, text=_X, ls=_X, anchors=_X, logits=_X, expo=_X, P=8, HW=4):
    return lib.ebc_head_fwd(F32, Z, text, ls, anchors, logits, expo, P, HW, 5, 512, None)


def _head_bwd(lib, Z=_X, text=_X, ls=_X, anchors=_X, dl=_X, de=_X, dZ=_X, P=8, HW=4):
    return lib.ebc_head_bwd(F32, F32, Z, text, ls, anchors, dl, de, None, dZ, None, None, P, HW, 5, 512, None, 0, None)


@pytest.mark.parametrize("kw", [dict(P=0), dict(P=-4), dict(HW=0), dict(HW=-1), dict(P=8, HW=3), dict(Z=None),
                                dict(text=None), dict(ls=None), dict(anchors=None)])
def test_head_rejects_without_device(lib, kw):
    """P <= 0, HW <= 0 (p / HW on the device), P not a whole number of images, NULL operands."""
    assert _head_fwd(lib, **kw) == EBC_E_ARG
    assert _head_bwd(lib, **kw) == EBC_E_ARG


def test_head_outputs_and_cast_reject_without_device(lib):
    assert _head_fwd(lib, logits=None) == EBC_E_ARG and _head_fwd(lib, expo=None) == EBC_E_ARG
    assert _head_bwd(lib, dl=None) == EBC_E_ARG and _head_bwd(lib, de=None) == EBC_E_ARG
    assert _head_bwd(lib, dZ=None) == EBC_E_ARG
    # d bias / d logit_scale asked for without a workspace (already rejected before this change)
    assert lib.ebc_head_bwd(F32, F32, _X, _X, _X, _X, _X, _X, None, _X, _X, None, 8, 4, 5, 512, None, 0, None) == EBC_E_ARG
    assert lib.ebc_cast_f32(F16, None, _X, 8, None) == EBC_E_ARG
    assert lib.ebc_cast_f32(F16, _X, None, 8, None) == EBC_E_ARG


def test_product_has_no_cpu_fallback():
    """The product path refuses to run without a HIP device rather than falling back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ebc_amd import _lib
    with pytest.raises(RuntimeError):
        _lib.lib()
