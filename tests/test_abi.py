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


def _ln_fwd(lib, x=_X, rpg=0, gs=0, go=0, gamma=_X, beta=_X, out=_X, outf=None, mean=_X, rstd=_X, M=8, dtype=F16):
    return lib.ebc_layernorm_fwd(dtype, x, rpg, gs, go, gamma, beta, out, outf, mean, rstd, M, 768, None)


def _ln_bwd(lib, dy=_X, x=_X, rpg=0, gs=0, go=0, mean=_X, rstd=_X, gamma=_X, dx_in=None, dx_out=_X, dxt=None, M=8,
            dtype=F16):
    return lib.ebc_layernorm_bwd(dtype, 0, dy, x, rpg, gs, go, mean, rstd, gamma, dx_in, dx_out, dxt, M, 768, None)


@pytest.mark.parametrize("kw", [dict(x=None), dict(gamma=None), dict(beta=None), dict(out=None, outf=None),
                                dict(rstd=None), dict(rpg=4, gs=7, go=-1), dict(rpg=4, gs=7, go=4),
                                dict(rpg=196, gs=229, go=34), dict(rpg=1, gs=0, go=0), dict(dtype=3)])
def test_layernorm_fwd_rejects_without_device(lib, kw):
    """NULL x / gamma / beta, no output at all, mean without rstd, a row map that leaves its group, a dtype that is
    none of the three."""
    assert _ln_fwd(lib, **kw) == EBC_E_ARG


@pytest.mark.parametrize("kw", [dict(dy=None), dict(x=None), dict(mean=None), dict(rstd=None), dict(gamma=None),
                                dict(dx_out=None), dict(rpg=4, gs=7, go=-1), dict(rpg=49, gs=82, go=34), dict(dtype=3)])
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
    for L in (5, 229, 300):                  # a dtype that is none of the three, on the resident and the streamed path
        assert lib.ebc_attention_fwd(3, _X, _X, _X, 1, L, 2, None) == EBC_E_ARG
        assert lib.ebc_attention_bwd(3, _X, _X, _X, _X, _X, _X, 1, L, 2, None) == EBC_E_ARG


def _head_fwd(lib, Z=_X, text=_X, ls=_X, anchors=_X, logits=_X, expo=_X, P=8, HW=4, dtype=F32):
    return lib.ebc_head_fwd(dtype, Z, text, ls, anchors, logits, expo, P, HW, 5, 512, None)


def _head_bwd(lib, Z=_X, text=_X, ls=_X, anchors=_X, dl=_X, de=_X, dZ=_X, P=8, HW=4, dtype=F32, dtype_dz=F32):
    return lib.ebc_head_bwd(dtype, dtype_dz, Z, text, ls, anchors, dl, de, None, dZ, None, None, P, HW, 5, 512, None, 0, None)


@pytest.mark.parametrize("kw", [dict(P=0), dict(P=-4), dict(HW=0), dict(HW=-1), dict(P=8, HW=3), dict(Z=None),
                                dict(text=None), dict(ls=None), dict(anchors=None), dict(dtype=3)])
def test_head_rejects_without_device(lib, kw):
    """P <= 0, HW <= 0 (p / HW on the device), P not a whole number of images, NULL operands, a dtype of Z that is none
    of the three."""
    assert _head_fwd(lib, **kw) == EBC_E_ARG
    assert _head_bwd(lib, **kw) == EBC_E_ARG


def test_head_outputs_and_cast_reject_without_device(lib):
    assert _head_fwd(lib, logits=None) == EBC_E_ARG and _head_fwd(lib, expo=None) == EBC_E_ARG
    assert _head_bwd(lib, dl=None) == EBC_E_ARG and _head_bwd(lib, de=None) == EBC_E_ARG
    assert _head_bwd(lib, dZ=None) == EBC_E_ARG
    assert _head_bwd(lib, dtype_dz=3) == EBC_E_ARG and _head_bwd(lib, dtype=F16, dtype_dz=3) == EBC_E_ARG
    # d bias / d logit_scale asked for without a workspace (already rejected before this change)
    assert lib.ebc_head_bwd(F32, F32, _X, _X, _X, _X, _X, _X, None, _X, _X, None, 8, 4, 5, 512, None, 0, None) == EBC_E_ARG
    assert lib.ebc_cast_f32(F16, None, _X, 8, None) == EBC_E_ARG
    assert lib.ebc_cast_f32(F16, _X, None, 8, None) == EBC_E_ARG
    assert lib.ebc_cast_f32(3, _X, _X, 8, None) == EBC_E_ARG


EBC_E_UNSUPPORTED = -3
BF16 = 2
STORE, GELU, RESID, GELU_BWD = 0, 1, 2, 3

# The single-kernel entry points' answers to calls they refuse on the host: every NULL in turn, P % HW, the bin and
# width ranges, a short workspace, a dtype that is none of the three, a row map that leaves its group, and pairs of
# faults that pin the order of the tests (a NULL operand is EBC_E_ARG before a bin count out of range is
# EBC_E_UNSUPPORTED).  The codes are part of the ABI: callers tell a bad call from a shape the library does not run.
# Every pointer is bogus, so a call that launched would not return.
_A, _U, _BIG = EBC_E_ARG, EBC_E_UNSUPPORTED, 1 << 30
_CALLS = {   # entry point -> (argument names in order, a call that is accepted)
    "ebc_head_fwd": ("dtype Z text ls anchors logits expo P HW NB embed stream",
                     dict(dtype=F32, Z=_X, text=_X, ls=_X, anchors=_X, logits=_X, expo=_X, P=8, HW=4, NB=5, embed=512)),
    "ebc_head_bwd": ("dtype dtype_dz Z text ls anchors dl de gscale dZ dbias dscale P HW NB embed ws wsb stream",
                     dict(dtype=F32, dtype_dz=F32, Z=_X, text=_X, ls=_X, anchors=_X, dl=_X, de=_X, dZ=_X, P=8, HW=4, NB=5,
                          embed=512, wsb=0)),
    "ebc_head_bwd_text": ("dtype Z text ls anchors dl de gscale dtext P HW NB embed ws wsb stream",
                          dict(dtype=F32, Z=_X, text=_X, ls=_X, anchors=_X, dl=_X, de=_X, dtext=_X, P=8, HW=4, NB=5,
                               embed=512, ws=_X, wsb=_BIG)),
    "ebc_layernorm_fwd": ("dtype x rpg gs go gamma beta out outf mean rstd M D stream",
                          dict(dtype=F16, x=_X, rpg=0, gs=0, go=0, gamma=_X, beta=_X, out=_X, mean=_X, rstd=_X, M=8, D=768)),
    "ebc_layernorm_bwd": ("dtype dy_f32 dy x rpg gs go mean rstd gamma dx_in dx_out dxt M D stream",
                          dict(dtype=F16, dy_f32=0, dy=_X, x=_X, rpg=0, gs=0, go=0, mean=_X, rstd=_X, gamma=_X, dx_out=_X,
                               M=8, D=768)),
    "ebc_attention_fwd": ("dtype qkv out lse B L H stream", dict(dtype=F16, qkv=_X, out=_X, lse=_X, B=1, L=5, H=2)),
    "ebc_attention_bwd": ("dtype qkv dout out lse delta dqkv B L H stream",
                          dict(dtype=F16, qkv=_X, dout=_X, out=_X, lse=_X, delta=_X, dqkv=_X, B=1, L=5, H=2)),
    "ebc_im2col": ("dtype x out B H W patch stream", dict(dtype=F16, x=_X, out=_X, B=2, H=32, W=32, patch=16)),
    "ebc_cast_f32": ("dtype src out n stream", dict(dtype=F16, src=_X, out=_X, n=8)),
}
_CALLS["ebc_head_bwd_text_wide"] = _CALLS["ebc_head_bwd_text"]
_HEAD_NULLS = [(dict([(k, None)]), _A) for k in ("Z", "text", "ls", "anchors", "dl", "de")]
_HEAD_SHAPE = [(dict(P=8, HW=3), _A), (dict(P=0), _A), (dict(NB=0), _U), (dict(NB=33), _U), (dict(embed=768), _U),
               (dict(dtype=3), _A), (dict(NB=40, Z=None), _A), (dict(NB=33, HW=3), _A), (dict(NB=33, dtype=3), _U),
               (dict(embed=768, dtype=3), _U)]
_TEXT = _HEAD_NULLS + [(dict(dtext=None), _A)] + _HEAD_SHAPE + [
    (dict(ws=None), _A), (dict(wsb=0), _A), (dict(dtype=3, ws=None), _A), (dict(embed=768, ws=None), _U),
    (dict(NB=0, wsb=0), _U)]
_REJECTED = {
    "ebc_head_fwd": _HEAD_NULLS[:4] + [(dict(logits=None), _A), (dict(expo=None), _A)] + _HEAD_SHAPE,
    "ebc_head_bwd": _HEAD_NULLS + [(dict(dZ=None), _A)] + _HEAD_SHAPE + [
        (dict(dtype_dz=3), _A), (dict(dbias=_X), _A), (dict(dscale=_X), _A),
        (dict(dbias=_X, ws=_X, wsb=(512 + 1) * 4 - 1), _A), (dict(dbias=_X, P=64, HW=64, ws=_X, wsb=(512 + 1) * 4), _A),
        (dict(dbias=_X, NB=33), _U), (dict(dscale=_X, embed=768, ws=_X, wsb=8), _U), (dict(dbias=_X, dtype=3), _A)],
    # the narrow text gradient stops at 16 bins; its workspace holds ceil(P / 64) * (NB * embed + 16) floats
    "ebc_head_bwd_text": _TEXT + [(dict(NB=17), _U), (dict(NB=17, dtype=3), _U), (dict(NB=17, text=None), _A),
                                  (dict(wsb=(5 * 512 + 16) * 4 - 1), _A)],
    "ebc_head_bwd_text_wide": _TEXT + [(dict(wsb=(5 * 512 + 32) * 4 - 1), _A), (dict(wsb=(5 * 512 + 16) * 4), _A)],
    "ebc_layernorm_fwd": [(dict(x=None), _A), (dict(gamma=None), _A), (dict(beta=None), _A), (dict(out=None), _A),
                          (dict(rstd=None), _A), (dict(rpg=4, gs=7, go=4), _A), (dict(rpg=4, gs=7, go=-1), _A),
                          (dict(D=700), _U), (dict(D=1024), _U), (dict(M=0), _U), (dict(dtype=3), _A),
                          (dict(dtype=3, D=512), _A), (dict(x=None, D=700), _A), (dict(rpg=4, gs=7, go=4, M=0), _A),
                          (dict(D=700, dtype=3), _U)],
    "ebc_layernorm_bwd": [(dict([(k, None)]), _A) for k in ("dy", "x", "mean", "rstd", "gamma", "dx_out")] + [
        (dict(rpg=4, gs=7, go=4), _A), (dict(D=700), _U), (dict(M=0), _U), (dict(dtype=3), _A), (dict(dtype=3, D=512), _A),
        (dict(gamma=None, M=0), _A), (dict(rpg=49, gs=82, go=34, D=700), _A), (dict(M=-1, dtype=3), _U)],
    "ebc_attention_fwd": [(dict(qkv=None), _A), (dict(out=None), _A), (dict(L=0), _U), (dict(L=20000), _U), (dict(B=0), _U),
                          (dict(H=0), _U), (dict(dtype=3), _A), (dict(dtype=3, L=300), _A), (dict(qkv=None, L=0), _A),
                          (dict(L=0, dtype=3), _U)],
    "ebc_attention_bwd": [(dict([(k, None)]), _A) for k in ("qkv", "dout", "out", "lse", "dqkv")] + [
        (dict(L=0), _U), (dict(L=20000), _U), (dict(B=0), _U), (dict(dtype=F32, delta=None), _A),
        (dict(L=300, delta=None), _A), (dict(dtype=3), _A), (dict(lse=None, B=0), _A), (dict(L=20000, delta=None), _U),
        (dict(dtype=3, L=300, delta=None), _A)],
    "ebc_im2col": [(dict(x=None), _A), (dict(out=None), _A), (dict(B=0), _A), (dict(patch=0), _A), (dict(H=8), _A),
                   (dict(H=40), _A), (dict(H=36, W=36, patch=6), _A), (dict(H=64, W=64, patch=64), _A), (dict(dtype=3), _A),
                   (dict(x=None, H=40), _A)],
    "ebc_cast_f32": [(dict(src=None), _A), (dict(out=None), _A), (dict(n=6), _A), (dict(dtype=3), _A), (dict(n=6, dtype=3), _A)],
}


@pytest.mark.parametrize("fn,kw,rc", [(fn, kw, rc) for fn, cases in _REJECTED.items() for kw, rc in cases],
                         ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_moved_entry_points_keep_their_return_codes(lib, fn, kw, rc):
    names, valid = _CALLS[fn]
    args = {**valid, **kw}
    assert getattr(lib, fn)(*[args.get(n) for n in names.split()]) == rc


@pytest.mark.parametrize("fn,args,nbytes", [
    ("ebc_head_bwd_workspace_bytes", (0, 512), 0), ("ebc_head_bwd_workspace_bytes", (-5, 512), 0),
    ("ebc_head_bwd_workspace_bytes", (8, 512), 513 * 4), ("ebc_head_bwd_workspace_bytes", (3136, 1024), 98 * 1025 * 4),
    ("ebc_head_bwd_workspace_bytes", (33, 768), 2 * 769 * 4),
    ("ebc_head_bwd_text_workspace_bytes", (8, 5, 512), (5 * 512 + 16) * 4),
    ("ebc_head_bwd_text_workspace_bytes", (3136, 16, 1024), 49 * (16 * 1024 + 16) * 4),
    ("ebc_head_bwd_text_workspace_bytes", (8, 17, 512), 0), ("ebc_head_bwd_text_workspace_bytes", (8, 5, 768), 0),
    ("ebc_head_bwd_text_workspace_bytes", (0, 5, 512), 0), ("ebc_head_bwd_text_workspace_bytes", (8, 0, 512), 0),
    ("ebc_head_bwd_text_workspace_bytes", (8, 5, 0), 0),
    ("ebc_head_bwd_text_wide_workspace_bytes", (8, 17, 512), (17 * 512 + 32) * 4),
    ("ebc_head_bwd_text_wide_workspace_bytes", (6272, 20, 1024), 98 * (20 * 1024 + 32) * 4),
    ("ebc_head_bwd_text_wide_workspace_bytes", (65, 32, 1024), 2 * (32 * 1024 + 32) * 4),
    ("ebc_head_bwd_text_wide_workspace_bytes", (8, 33, 512), 0), ("ebc_head_bwd_text_wide_workspace_bytes", (8, 5, 768), 0),
    ("ebc_head_bwd_text_wide_workspace_bytes", (0, 5, 512), 0), ("ebc_head_bwd_text_wide_workspace_bytes", (8, 0, 512), 0)])
def test_head_workspace_sizes(lib, fn, args, nbytes):
    assert getattr(lib, fn)(*args) == nbytes


def _gemm(lib, dtype=F16, epi=STORE, out_f32=0, A=_X, B=_X, C=_X, bias=None, resid=None, aux=None, M=16, N=64, K=64):
    return lib.ebc_gemm(dtype, epi, out_f32, A, B, C, bias, resid, aux, M, N, K, None)


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("epi", [-1, 4, 5, 6, 7, 8, 9, 1 << 20])
def test_gemm_rejects_internal_epilogue_ids_without_device(lib, dtype, epi):
    """Only EBC_EPI_STORE .. EBC_EPI_GELU_BWD are public: the LayerNorm-fold ids 6, 7 and 8 used to reach a kernel whose
    fold operands were all NULL.  Every operand is a bogus pointer here, so a call that launched would not return."""
    assert _gemm(lib, dtype=dtype, epi=epi, resid=_X, aux=_X, bias=_X) == EBC_E_ARG
    assert _gemm(lib, dtype=dtype, epi=epi, out_f32=1, resid=_X, aux=_X, bias=_X) == EBC_E_ARG


@pytest.mark.parametrize("kw", [dict(A=None), dict(B=None), dict(C=None), dict(K=48), dict(K=96), dict(K=0), dict(N=96),
                                dict(N=32), dict(N=0), dict(M=0), dict(M=-3), dict(dtype=F32, K=48), dict(dtype=F32, K=16),
                                dict(epi=RESID), dict(epi=RESID, out_f32=1), dict(epi=GELU_BWD),
                                dict(dtype=F32, epi=RESID), dict(dtype=F32, epi=GELU_BWD), dict(dtype=3), dict(dtype=-1),
                                dict(dtype=7, epi=RESID, resid=_X)])
def test_gemm_rejects_without_device(lib, kw):
    """NULL A / B / C, K % 64 (16-bit) and K % 32 (f32), N % 64, empty shapes, RESID without resid, GELU' without aux,
    a dtype that is none of the three."""
    assert _gemm(lib, **kw) == EBC_E_ARG
    assert _gemm(lib, **{"dtype": BF16, **kw}) == EBC_E_ARG


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("epi", [GELU, GELU_BWD])
def test_gemm_gelu_to_f32_is_unsupported_without_device(lib, dtype, epi):
    assert _gemm(lib, dtype=dtype, epi=epi, out_f32=1, aux=_X) == EBC_E_UNSUPPORTED


def _rows(lib, dtype=F16, out_f32=0, A=_X, B=_X, C=_X, bias=None, M=15, N=768, K=768, rpg=5, gs=23, go=1):
    return lib.ebc_gemm_rows(dtype, out_f32, A, B, C, bias, M, N, K, rpg, gs, go, None)


@pytest.mark.parametrize("kw", [dict(A=None), dict(B=None), dict(C=None), dict(K=800), dict(dtype=F32, K=48), dict(N=800),
                                dict(M=0), dict(dtype=5), dict(dtype=3), dict(rpg=-1), dict(go=-1), dict(go=19), dict(rpg=24),
                                dict(rpg=1, gs=0, go=0), dict(rpg=196, gs=229, go=34)])
def test_gemm_rows_rejects_without_device(lib, kw):
    """ebc_gemm's checks, and a row map that leaves its group."""
    assert _rows(lib, **kw) == EBC_E_ARG


def _wgrad(lib, dtype=F16, A=_X, B=_X, C=_X, M=128, N=64, K=64, ws=None, wsb=0):
    return lib.ebc_gemm_wgrad(dtype, A, B, C, M, N, K, ws, wsb, None)


@pytest.mark.parametrize("kw", [dict(A=None), dict(B=None), dict(C=None), dict(K=96), dict(dtype=F32, K=48), dict(N=96),
                                dict(M=0), dict(N=0), dict(K=0), dict(dtype=3), dict(dtype=-2)])
def test_gemm_wgrad_rejects_without_device(lib, kw):
    assert _wgrad(lib, **kw) == EBC_E_ARG


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("M,N,K", [(100, 192, 1024), (100, 192, 4096), (300, 1024, 25088)])
def test_gemm_wgrad_rejects_a_split_plan_without_its_workspace(lib, dtype, M, N, K):
    """A shape whose plan splits K (two pieces, or partials and a reduce launch): NULL workspace, one that is a byte
    short, NULL with a size."""
    import ctypes
    out = (ctypes.c_int * 3)()
    assert lib.ebc_gemm_wgrad_tile_config(dtype, M, N, K, out) > 0
    need = lib.ebc_gemm_wgrad_workspace_bytes(dtype, M, N, K)
    if abs(out[2]) == 1:
        assert need == 0                                     # (the f32 plan of a shape need not split)
        return
    assert need > 16 * 1024
    assert _wgrad(lib, dtype=dtype, M=M, N=N, K=K, ws=None, wsb=0) == EBC_E_ARG
    assert _wgrad(lib, dtype=dtype, M=M, N=N, K=K, ws=None, wsb=need) == EBC_E_ARG
    assert _wgrad(lib, dtype=dtype, M=M, N=N, K=K, ws=_X, wsb=need - 1) == EBC_E_ARG
    assert _wgrad(lib, dtype=dtype, M=M, N=N, K=K, ws=_X, wsb=0) == EBC_E_ARG


def test_gemm_wgrad_tile_config_is_host_only(lib):
    import ctypes
    out = (ctypes.c_int * 3)()
    assert lib.ebc_gemm_wgrad_tile_config(F16, 128, 64, 64, out) == 2 and tuple(out) == (128, 64, 1)
    assert lib.ebc_gemm_wgrad_tile_config(F32, 128, 64, 64, None) == 2
    for bad in (dict(dtype=3), dict(M=0), dict(N=-1), dict(K=0)):
        a = {"dtype": F16, "M": 128, "N": 64, "K": 64, **bad}
        assert lib.ebc_gemm_wgrad_tile_config(a["dtype"], a["M"], a["N"], a["K"], out) == EBC_E_ARG
    # a split plan's workspace is the counter block plus what the plan's pieces need
    for dt in (F32, F16, BF16):
        for M, N, K in ((100, 192, 1024), (100, 192, 4096), (300, 384, 8192), (300, 1024, 25088)):
            cfg = lib.ebc_gemm_wgrad_tile_config(dt, M, N, K, out)
            bm, bn, sp = tuple(out)
            tiles = -(-M // bm) * (N // bn)
            want = 0 if abs(sp) == 1 else 16384 + (-sp * M * N * 4 if sp < 0 else sp * tiles * bm * bn * 4)
            assert cfg in (1, 2, 3, 7) and N % bn == 0 and lib.ebc_gemm_wgrad_workspace_bytes(dt, M, N, K) == want


def test_gpu_gemm_case_lists_reach_every_tile_and_plan_class(lib):
    """The shapes of tests/test_gpu_gemm_kernels.py against the host-only dispatch calls, so a dispatch change that moves
    a case onto another kernel shows without a GPU: every tile id ebc_gemm can return and every (tile, split class) of
    ebc_gemm_wgrad has a case, except the classes the planner never picks."""
    import ctypes
    import test_gpu_gemm_kernels as T
    out = (ctypes.c_int * 3)()
    for dt, cases in ((F32, T.CASES32), (F16, T.CASES16), (BF16, T.CASES16)):
        for tile, M, N, K in cases:
            assert lib.ebc_gemm_tile_config(dt, M, N, K, out) == tile and tuple(out) == (*T.TILES[tile][:2], 1), (dt, M, N, K)
    assert {c[0] for c in T.CASES16} == set(T.TILES) == {1, 2, 3, 4, 5, 7, 15, 16} and {c[0] for c in T.CASES32} == {2}
    reachable = set()
    for M in (1, 129, 1000, 3664, 4097, 7328, 8065, 12544, 24321, 32060, 50176):
        for N in range(64, 4097, 64):
            for K in (64, 512, 768, 1024, 2304, 3072, 4096, 8192):
                reachable.add(lib.ebc_gemm_tile_config(F16, M, N, K, None))
    assert reachable == set(T.TILES)

    def split_class(s):
        return min(abs(s), 3)                       # 1: no split, 2: last arriver, 3: partials and a reduce launch

    for dt, plans in ((F32, T.WGRAD32), (F16, T.WGRAD16), (BF16, T.WGRAD16)):
        for (M, N, K), plan in plans:
            assert (lib.ebc_gemm_wgrad_tile_config(dt, M, N, K, out), out[2]) == plan, (dt, M, N, K)
            assert (out[2] < 0) == (abs(out[2]) > 2)
    assert {(p[0], split_class(p[1])) for _, p in T.WGRAD16} == {(t, c) for t in (1, 2, 3, 7) for c in (1, 2, 3)}
    assert {(p[0], split_class(p[1])) for _, p in T.WGRAD32} == {(2, 1), (2, 2), (2, 3)}


def _transpose(lib, dtype=F16, src=_X, out=_X, R=9, C=72, ld=16):
    return lib.ebc_transpose(dtype, src, out, R, C, ld, None)


@pytest.mark.parametrize("kw", [dict(src=None), dict(out=None), dict(R=0), dict(C=0), dict(C=-8), dict(C=68), dict(C=4),
                                dict(ld=8), dict(R=17), dict(ld=20), dict(ld=12), dict(dtype=3), dict(dtype=-1)])
def test_transpose_rejects_without_device(lib, kw):
    """NULL in / out, empty shapes, C % 8, ld_out < R, ld_out % 8, a bad dtype."""
    assert _transpose(lib, **kw) == EBC_E_ARG


def test_product_has_no_cpu_fallback():
    """The product path refuses to run without a HIP device rather than falling back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ebc_amd import _lib
    with pytest.raises(RuntimeError):
        _lib.lib()


# ------------------------------------------------------------------------------------------- fused DACE loss: plan
# ebc_dace_plan per LDS grid at reduction 8: (size, G, lds_cap_s, lds_cap_c, lds_cap, 16 lanes offered)
DACE_PLAN = [(64, 8, 1840, 1840, 1471, True), (128, 16, 1034, 1310, 826, True), (192, 24, 691, 1245, 553, True),
             (224, 28, 582, 1202, 468, True), (256, 32, 494, 1154, 392, True), (320, 40, 361, 1036, 287, False),
             (384, 48, 262, 892, 217, False), (448, 56, 183, 722, 157, False), (512, 64, 117, 526, 87, False)]


def _plan(lib, size, red, n):
    import ctypes
    out = (ctypes.c_int * 6)()
    return lib.ebc_dace_plan(size, red, n, out), list(out)


@pytest.mark.parametrize("size,G,cap_s,cap_c,cap,w16", DACE_PLAN)
def test_dace_plan_table(lib, size, G, cap_s, cap_c, cap, w16):
    """The capacities are the recorded ones (a capacity one point too high would put a crop's last factor row past the
    LDS allocation), and the paths switch exactly at them."""
    for n in (0, 1, 17, 256, 257, cap, cap + 1, cap_s, cap_s + 1, cap_c, cap_c + 1, 5000):
        g, out = _plan(lib, size, 8, n)
        assert g == G and out[3:] == [cap_s, cap_c, cap], (n, g, out)
        first = 0 if n <= cap_s else 1 if n <= cap_c else (2 if n <= cap else 3)
        assert out[0] == first and out[2] == (2 if n <= cap else 3), (n, out)
        assert out[1] == (0 if first >= 2 else 16 if (w16 and n >= 257) else 8), (n, out)
    assert cap <= cap_s <= cap_c
    for pad in range(size - 8, max(size - 32, 0), -8):          # a padded density grid runs on the same LDS grid
        if all(pad // 8 > t[1] for t in DACE_PLAN if t[1] < G):
            assert _plan(lib, pad, 8, 1)[0] == G, pad


def test_dace_plan_geometry(lib):
    assert lib.ebc_dace_plan(8, 8, 1, None) == 8 and lib.ebc_dace_plan(24, 8, 1, None) == 8
    assert lib.ebc_dace_plan(320, 16, 1, None) == 24 and lib.ebc_dace_plan(640, 16, 1, None) == 40
    assert lib.ebc_dace_plan(768, 32, 1, None) == 24 and lib.ebc_dace_plan(512, 16, 1, None) == 32
    for bad in ((520, 8, 1), (224, 0, 1), (224, -8, 1), (225, 8, 1), (0, 8, 1), (224, 8, -1)):
        assert lib.ebc_dace_plan(*bad, None) == 0, bad


def _dace_h(lib, offsets, size, ws, ws_bytes, red=8):
    """ebc_dace_loss_h with every argument valid but, possibly, the offsets and the workspace; no pointer is read
    before the checks under test."""
    import ctypes
    B = len(offsets) - 1
    o = (ctypes.c_int * (B + 1))(*offsets)
    return lib.ebc_dace_loss_h(_X, _X, _X, 0, _X, o, None, _X, _X, B, 5, size, red, 0, 0, 1.0, 0.1, 0.01, 10.0, 100, 1e-9,
                               10, _X, _X, _X, _X, None, None, ws, ws_bytes, None)


@pytest.mark.parametrize("size,G,cap_s,cap_c,cap,w16", DACE_PLAN)
def test_dace_loss_h_refuses_a_missing_or_short_workspace(lib, size, G, cap_s, cap_c, cap, w16):
    """Return codes only, all before any launch: a crop that can reach the workspace path (more than lds_cap points:
    directly, or as the dense fallback of the bucketed path) needs the whole workspace."""
    for offsets in ([0, 3, 3 + cap + 1], [0, cap_c + 1], [0, 0, cap_s + 1, cap_s + 2]):
        need = lib.ebc_dace_workspace_bytes(len(offsets) - 1, offsets[-1], size, 8)
        assert _dace_h(lib, offsets, size, None, need) == EBC_E_ARG
        assert _dace_h(lib, offsets, size, None, 0) == EBC_E_ARG
        for short in (0, 8, 255, 256, need - 1):
            assert _dace_h(lib, offsets, size, _X, short) == EBC_E_ARG, (offsets, short)
    assert _dace_h(lib, [0, 5, 3], size, _X, 1 << 24) == EBC_E_ARG          # offsets that decrease


# ------------------------------------------------------------------------------------------- Sinkhorn, Adam: host side
def test_sinkhorn_workspace_bytes_is_host_only(lib):
    """0 for a non-positive size, 0 while K fits LDS beside u, v and K^T u (199 x 199), the whole of K from 200 x 200."""
    for na, nb in ((0, 5), (5, 0), (-1, 5), (5, -7), (0, 0)):
        assert lib.ebc_sinkhorn_workspace_bytes(na, nb) == 0
    assert lib.ebc_sinkhorn_workspace_bytes(199, 199) == 0
    assert lib.ebc_sinkhorn_workspace_bytes(200, 200) == 4 * 200 * 200


def _sinkhorn(lib, a=_X, b=_X, C=_X, na=8, nb=8, reg=0.5, max_iter=1, thr=1e-9, eval_freq=10, info=_X, ws=None, wsb=0):
    return lib.ebc_sinkhorn(a, b, C, na, nb, reg, max_iter, thr, eval_freq, 1, _X, _X, _X, _X, _X, _X, info, ws, wsb, None)


@pytest.mark.parametrize("kw", [dict(reg=0.0), dict(reg=-1.0), dict(reg=float("nan")), dict(eval_freq=0), dict(eval_freq=-3),
                                dict(info=None), dict(a=None), dict(b=None), dict(C=None), dict(na=0), dict(nb=-2),
                                dict(na=200, nb=200), dict(na=200, nb=200, ws=_X, wsb=4 * 200 * 200 - 1)])
def test_sinkhorn_rejects_without_device(lib, kw):
    """reg <= 0, eval_freq <= 0, a NULL info or operand, an empty shape, a workspace shape without its workspace."""
    assert _sinkhorn(lib, **kw) == EBC_E_ARG


def test_sinkhorn_oversize_is_unsupported_without_device(lib):
    """u, v and K^T u must stay in LDS: nb = 13632 at na = 1 is the first size that does not fit."""
    assert _sinkhorn(lib, na=1, nb=13632, ws=_X, wsb=1 << 30) == EBC_E_UNSUPPORTED
    assert _sinkhorn(lib, na=1, nb=13633, ws=_X, wsb=1 << 30) == EBC_E_UNSUPPORTED
    assert _sinkhorn(lib, na=20000, nb=20000, ws=_X, wsb=1 << 40) == EBC_E_UNSUPPORTED


def _adam(lib, fn, tensors=_X, n=1, step=_X, spar=0, scaler=_X, cpar=0, interval=2000):
    if fn == "check":
        return lib.ebc_amp_check(tensors, n, scaler, cpar, None)
    f = lib.ebc_adam_step if fn == "step" else lib.ebc_adam_update
    return f(tensors, n, step, spar, scaler, cpar, 1e-3, 0.9, 0.999, 1e-8, 0.0, 2.0, 0.5, interval, 1, None)


_ADAM_BAD = [dict(n=0), dict(n=-1), dict(tensors=None), dict(cpar=2), dict(cpar=-1)]
_ADAM_BAD_UPDATE = [dict(spar=2), dict(spar=-1), dict(step=None), dict(interval=0), dict(interval=-5)]


@pytest.mark.parametrize("fn,kw", [(fn, kw) for fn in ("step", "update") for kw in _ADAM_BAD + _ADAM_BAD_UPDATE] +
                         [("check", kw) for kw in _ADAM_BAD + [dict(scaler=None)]])
def test_adam_rejects_without_device(lib, fn, kw):
    """n <= 0, NULL tensors, a parity that is neither 0 nor 1, growth_interval <= 0, a NULL step count; the check alone
    also refuses a NULL scaler (the two update calls take it as "no scaler")."""
    assert _adam(lib, fn, **kw) == EBC_E_ARG
