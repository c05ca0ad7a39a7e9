"""The encoder as ebc_vit_forward / ebc_vit_backward execute it, one stage at a time, per element against the float64
stage references of tests/_vit_refs.py (pinned on the CPU in tests/test_vit_refs_cpu.py).

The calls go straight over ctypes with the synthetic loader's weights in an _EncoderCache (the model's own preparation of
the folded operands); the workspace is exactly ebc_vit_workspace_bytes_p bytes inside a sentinel frame, and after the
call every stage's output is read back through the workspace mirror and held to the reference computed from the operands
that stage received (also read back).  This is what reaches gemm_nt_ln's five epilogues (RESID with the 16-bit copy and
row partials, with and without the deep-VPT row replacement; LN; LN_GELU; GELU_BWD with the backward partials; LN_BWD),
the launchers without a C entry point (embed_tokens, layernorm_fwd_vpt, layernorm_bwd_fill / _rows / _vpt, vpt_sum,
attention_bwd with rows > 0) and vit.hip's own carve, fold / fold_b choice, trimmed layer-0 backward and prompt-gradient
modes.  Every case first asserts the tiles its products run on (ebc_gemm_tile_config), so a retuned dispatch table fails
the case list and not the coverage.  Every check prints "RATIO <name> <largest error / bound>" before it asserts.
"""
import ctypes

import pytest
import torch

import _enc_refs as ER
import _vit_refs as V
from _kernel_checks import _Framed, _report
from ebc_amd import _lib
import test_gpu_encoder_kernels as E
from test_gpu_encoder_kernels import _check_attn_bwd, _check_attn_fwd

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
F64 = torch.float64
WS_FILL = 0x47             # 16-bit 7.28 / 5.1e4 (bf16), f32 5.1e4: an unwritten output misses every bound
VP = ctypes.c_void_p


def _setup(name, dname, mode, per_crop, fold, stats="benign", layers=None):
    from ebc_amd.model import _EncoderCache
    dt = DT[dname]
    patch, H, W, NV, B, nl, G, L, M = V.case_dims(name)
    nl = layers or nl
    lib = _lib.lib()
    code = _lib.dtype_code(dt)
    # the tiles this case is in the list for
    assert V.case_tiles(lib, code, name) == (V.TILES16[name] if dname != "f32" else (2,) * 5), name
    enc = V.make_encoder(name, stats, nl)
    cache = _EncoderCache(enc, NV, dt, torch.device("cuda"), ln_fold=fold)
    P = V.params_from_cache(cache, H // patch, W // patch)
    image, vpts, bstride = V.make_inputs(name, mode, per_crop, nl, stats=stats)
    s = dict(name=name, dname=dname, dt=dt, code=code, lib=lib, cache=cache, P=P, image=image.cuda(), bstride=bstride,
             vpts=[v.cuda() if v is not None else None for v in vpts], nl=nl, fold=fold and dname != "f32",
             w=cache.weights(H // patch, W // patch), dims=(patch, H, W, NV, B, nl, G, L, M),
             parts=V.part_counts(lib, code, M), tag=f"{name}[{dname},{mode},{'crop' if per_crop else 'shared'},"
                                                    f"{'fold' if fold and dname != 'f32' else 'nofold'},{stats}]")
    if s["fold"]:
        assert max(s["parts"][:2]) <= V.LN_PMAX and P["layers"][0]["w_qkv_ln"] is not None
    return s


def _forward(s, training):
    """ebc_vit_forward into a framed workspace of exactly the library's size, and a framed feat."""
    patch, H, W, NV, B, nl, G, L, M = s["dims"]
    lib = s["lib"]
    nbytes = lib.ebc_vit_workspace_bytes_p(B, H, W, patch, nl, NV, s["code"], training)
    frame = _Framed(nbytes // 256, 256, torch.uint8, fill=WS_FILL)
    ws = V.Workspace(frame.mid.view(-1), B, L, G, 3 * patch * patch, nl, s["dt"], training, s["parts"])
    assert ws.total == nbytes == frame.mid.numel()
    feat = _Framed(B * G, V.WIDTH, torch.float32)
    arr = (VP * nl)(*[v.data_ptr() if v is not None else None for v in s["vpts"]])
    rc = lib.ebc_vit_forward(ctypes.byref(s["w"]), _lib.ptr(s["image"]), B, H, W, arr, s["bstride"], s["code"], training,
                             _lib.ptr(frame.mid), nbytes, _lib.ptr(feat.mid), _lib.stream())
    _lib.check(rc, "ebc_vit_forward")
    torch.cuda.synchronize()
    assert frame.ok() and feat.ok()
    s.update(frame=frame, ws=ws, featf=feat, feat=feat.mid.view(B, G, V.WIDTH))
    return s


class _binade_aware:
    """The attention reference and bounds are test_gpu_encoder_kernels' own (_check_attn_fwd / _check_attn_bwd), with
    one derived term added to the 16-bit outputs' final rounding.  Those bounds have the form d + ulp_T(ref) / 2; the
    kernel rounds its computed value x~, |x~ - ref| <= d, within ulp_T(x~) / 2, and where ref lies within d below a power
    of two x~ may lie above it, where T's spacing is twice ulp_T(ref).  At L = 8 (every term of dK = dS^T Q / 8 can line
    up: 8 terms) and 1e6 elements a case that measures 0.90 .. 0.95 everywhere else passed the unamended bound on exactly
    one such element in three cases, the only ratios above 1 of this module's first run (bf16, dK, keys 0 / 1 of the
    trimmed backward):
        fold_b_low   flags 0   ref  3.124604852e-02  stored  3.149414062e-02   (2^-5 = 3.125e-02)   ratio 1.0334
        fold_b_low   flags 2   ref -3.121321233e-02  stored -3.149414062e-02                        ratio 1.0268
        many_tiles   flags 0   ref  1.249551507e-01  stored  1.259765625e-01   (2^-3 = 1.25e-01)    ratio 1.1138
    with ulp_T(stored) = 2 ulp_T(ref) in all three and in no other element near its bound: the kernel is right, the
    final-rounding term was short.  V.binade_aware replaces ulp_T(ref) / 2 by ulp_T(|ref| + d) / 2, which differs only
    for those elements.  While active, test_gpu_encoder_kernels' checks report through it."""

    def __init__(self, refs, dt):
        self.refs, self.dt = refs, dt

    def __enter__(self):
        self.old = E._report
        E._report = self.report

    def __exit__(self, *exc):
        E._report = self.old

    def report(self, name, err, bound):
        ref = self.refs.get(name.rsplit(".", 1)[1])
        if ref is not None and self.dt != torch.float32:
            bound = V.binade_aware(ref, bound, self.dt)
        _report(name, err, bound)


def _attn_fwd_check(s):
    B, L, dname = s["dims"][4], s["dims"][7], s["dname"]

    def check(tag, QKV, O, lse):
        q, k, v = ER.split_qkv(QKV.cpu(), B, L, V.HEADS)
        with _binade_aware({"out": ER.attention_fwd(q, k, v)["o"]}, s["dt"]):
            _check_attn_fwd(tag, dname, q, k, v, ER.heads(O.cpu(), B, L, V.HEADS), lse.cpu().to(F64))
    return check


def _attn_bwd_check(s):
    B, L, dname = s["dims"][4], s["dims"][7], s["dname"]

    def check(tag, QKV, dO, O, lse, dQKV, delta, lim):
        """Rows >= lim of every crop are not promised by the trimmed launch: the reference stands in for them."""
        q, k, v = ER.split_qkv(QKV.cpu(), B, L, V.HEADS)
        do, o, lse64 = ER.heads(dO.cpu(), B, L, V.HEADS), ER.heads(O.cpu(), B, L, V.HEADS), lse.cpu().to(F64)
        got = [t.clone() for t in ER.split_qkv(dQKV.cpu(), B, L, V.HEADS)]
        r = ER.attention_bwd(q, k, v, do, o, lse64)
        if lim < L:
            for t, key in zip(got, ("dq", "dk", "dv")):
                t[:, :, lim:] = r[key][:, :, lim:]
        with _binade_aware({key: r[key] for key in ("dq", "dk", "dv")}, s["dt"]):
            _check_attn_bwd(tag, dname, q, k, v, do, o, lse64, (*got, delta.cpu().to(F64)))
    return check


def _check_forward(s, training=True):
    lib, code, M = s["lib"], s["code"], s["dims"][-1]
    bn_out = V.tile_of(lib, code, M, V.WIDTH, V.WIDTH)[2]
    bn_proj = V.tile_of(lib, code, M, V.WIDTH, V.MLP)[2]
    V.walk_forward(V.Walk("check", _report, s["tag"] + ("" if training else ".eval")), s["ws"], s["P"], s["image"],
                   s["vpts"], s["bstride"], s["feat"], s["fold"], training, bn_out, bn_proj, _attn_fwd_check(s))


# (case, mode, per crop, fold, stats) of the 16-bit types
FWD16 = [("tiny", "deep", True, True, "benign"), ("tiny", "deep", False, True, "benign"),
         ("tiny", "shallow", False, True, "benign"), ("tiny", "deep", True, False, "benign"),
         ("tiny", "deep", True, True, "outlier"), ("tiny", "deep", True, True, "offset"),
         ("ragged135", "deep", False, True, "offset"), ("tiny_nv0", "none", False, True, "benign"),
         ("tiny_nv0", "none", False, False, "benign"), ("ragged135", "deep", True, True, "benign"),
         ("ragged261", "deep", True, True, "benign"), ("ragged261", "deep", False, False, "outlier"),
         ("fold_b_low", "deep", False, True, "benign"), ("fold_b_high", "deep", True, True, "benign"),
         ("many_tiles", "deep", True, True, "benign"),
         ("patch16", "deep", False, True, "benign"), ("L229", "deep", False, True, "benign")]
FWD32 = [("tiny", "deep", True, False, "benign"), ("tiny", "shallow", False, False, "benign"),
         ("tiny_nv0", "none", False, False, "benign"), ("patch16", "deep", False, False, "outlier")]


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


@pytest.mark.parametrize("name,mode,per_crop,fold,stats", FWD16, ids=_ids(FWD16))
@pytest.mark.parametrize("dname", ["f16", "bf16"])
def test_forward_stages_16bit(dname, name, mode, per_crop, fold, stats):
    """training = 1 saves every layer: patch_t / patch_f / X_0; per layer the statistics, QKV, the prompt rows bit for
    bit, attention, X1, A (and G, H of the last layer), X_l+1; feat with mpost / rpost."""
    _check_forward(_forward(_setup(name, dname, mode, per_crop, fold, stats), 1))


@pytest.mark.parametrize("name,mode,per_crop,fold,stats", FWD32, ids=_ids(FWD32))
def test_forward_stages_f32(name, mode, per_crop, fold, stats):
    """f32 has no fold; its launchers without a C entry point (embed_tokens, layernorm_fwd_vpt) are the same code."""
    _check_forward(_forward(_setup(name, "f32", mode, per_crop, fold, stats), 1))


@pytest.mark.parametrize("dname,fold", [("f16", True), ("f16", False), ("bf16", True), ("bf16", False), ("f32", False)])
def test_eval_forward_is_the_training_forward(dname, fold):
    """training = 0, three layers: X ping-pongs between two buffers and every layer shares LayerSave 0; the workspace is
    exactly the eval size inside its frame.  The kernels take the same arithmetic path in both modes (eval only passes
    no pre-activation buffer to the c_fc product, whose epilogue skips that store), so feat is the training forward's
    bit for bit, and held to the same reference and bound from the X_3 / mpost / rpost left in the eval workspace."""
    tr =_forward(_setup("tiny", dname, "deep", True, fold), 1)
    feat_tr = tr["feat"].clone()
    ev = _forward(_setup("tiny", dname, "deep", True, fold), 0)
    assert ev["ws"].total < tr["ws"].total
    _check_forward(ev, training=False)
    assert torch.equal(ev["feat"], feat_tr), int((ev["feat"] != feat_tr).sum())


# ------------------------------------------------------------------------------------------------ backward
def _backward(s, flags, want_dvpt=True):
    patch, H, W, NV, B, nl, G, L, M = s["dims"]
    assert nl == 1
    lib = s["lib"]
    s["dfeat"] = V.make_dfeat(s["name"]).cuda()
    frames = [None]
    if NV and want_dvpt:
        nb = B if s["bstride"] else 1
        frames = [_Framed(nb * NV, V.WIDTH, torch.float32)]
    s["dvpt"] = [f.mid.view(-1, NV, V.WIDTH) if s["bstride"] else f.mid for f in frames] if frames[0] is not None else [None]
    arr = (VP * nl)(*[f.mid.data_ptr() if f is not None else None for f in frames])
    nbytes = s["frame"].mid.numel()
    rc = lib.ebc_vit_backward(ctypes.byref(s["w"]), B, H, W, s["code"], _lib.ptr(s["frame"].mid), nbytes,
                              _lib.ptr(s["dfeat"]), arr, s["bstride"], flags, _lib.stream())
    _lib.check(rc, "ebc_vit_backward")
    torch.cuda.synchronize()
    assert s["frame"].ok() and all(f is None or f.ok() for f in frames)
    fold_b = s["fold"] and V.fold_b_taken(lib, s["code"], M, flags)
    bn_gelu = V.tile_of(lib, s["code"], M, V.MLP, V.WIDTH)[2]
    V.walk_backward(V.Walk("check", _report, f"{s['tag']}.bwd[flags={flags},fold_b={int(fold_b)}]"), s["ws"], s["P"],
                    s["dfeat"], s["dvpt"], s["bstride"], flags, fold_b, bn_gelu, _attn_bwd_check(s))
    if NV and want_dvpt and not s["bstride"]:
        # vpt_sum has no entry point to feed dyadic rows through, but its inputs can be read back: the shared gradient
        # is the crop-order f32 sum of the stored per-crop rows bit for bit (another order, a missing or a doubled crop
        # changes the bits of most of the NV * 768 sums)
        rows = s["ws"].get("vpt_rows")[0]
        acc = rows[0].clone()
        for b in range(1, B):
            acc += rows[b]
        assert torch.equal(s["dvpt"][0], acc), int((s["dvpt"][0] != acc).sum())
    return fold_b


# (case, per crop, flags, fold_b expected)
BWD16 = [("tiny", True, 0, False), ("tiny", False, 0, False), ("tiny", True, 1, False), ("tiny", False, 1, False),
         ("tiny_nv0", False, 0, False), ("ragged135", False, 0, False),
         ("fold_b_low", False, 0, True), ("fold_b_low", True, 1, True), ("fold_b_low", False, 2, False),
         ("fold_b_high", True, 0, True), ("many_tiles", False, 0, False), ("L229", False, 0, False)]


@pytest.mark.parametrize("name,per_crop,flags,fold_b", BWD16, ids=_ids(BWD16))
@pytest.mark.parametrize("dname", ["f16", "bf16"])
def test_backward_stages_16bit(dname, name, per_crop, flags, fold_b):
    """One layer, so the transients hold its values after the call.  flags 0: layer 0's trimmed path (dX_L, dA and its
    partials, dX1 by EPI_LN_BWD or by the product + LayerNorm launch, dO, the attention backward's promised rows, dH on
    the row-mapped prompt rows, the prompt gradient per crop or summed); EBC_VIT_BWD_FULL_LAYER0 (1): the path the
    deeper layers take (full attention backward, layernorm_bwd_vpt: exact zeros in the prompt rows of dX / dXt);
    EBC_VIT_BWD_NO_LN_FOLD (2): the unfolded MLP half at a shape that folds."""
    nv = V.case_dims(name)[3]
    s = _forward(_setup(name, dname, "deep" if nv else "none", per_crop, True, layers=1), 1)
    assert _backward(s, flags) == fold_b


@pytest.mark.parametrize("per_crop,flags", [(True, 0), (False, 0), (False, 1)])
def test_backward_stages_f32(per_crop, flags):
    """f32: no fold; layernorm_bwd_fill / _rows / _vpt, vpt_sum and the attention backward's delta are the same code."""
    s = _forward(_setup("tiny", "f32", "deep", per_crop, False, layers=1), 1)
    assert _backward(s, flags) is False
