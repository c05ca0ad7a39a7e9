"""The similarity head at 17 .. 32 bins (head.hip: the 32-slot instances of head_fwd_kernel / head_bwd_kernel, and
head_text_wide_bwd_kernel behind ebc_head_bwd_text_wide), per element against float64.

No new tolerance: the forward and backward cases ARE tests/test_gpu_encoder_kernels.py's test_head_fwd / test_head_bwd,
called with the new bin counts and pixel counts (their error models take NB and embed as arguments); the text gradient
is checked against tests/test_gpu_head_text_kernel.py's text_grad_ref / text_grad_bound (the wide kernel forms dl, the
per-wave sums and the fixed-order combine as head_text_bwd_kernel does; its logits pass through LDS unrounded).  The one
variation written out here, the backward without gscale and with an all-zero text row, restates test_head_bwd's bound.

Bin counts: 17 (the first past the 16-slot instances; one row in the second LDS group of the wide text kernel at 1024
channels), 20 (the reference's reduction-32 table), 31 and 32 (a partial last group, and the cap)."""
import pytest
import torch

import _bn_refs as BR
import _enc_refs as R
import test_gpu_encoder_kernels as E
import test_gpu_head_text_kernel as T
from _kernel_checks import _Hold, _guard_ok, _guarded, _report
from ebc_amd import _lib

pytestmark = pytest.mark.gpu
F64, U, DT, WS_GUARD = E.F64, E.U, E.DT, E.WS_GUARD
NBS = [17, 20, 31, 32]
FWD_P = [1, 5, 131]            # 4 pixels a workgroup: one pixel; a full workgroup and one pixel; 33 workgroups, ragged
BWD_P = [1, 33, 2049]          # 32 a workgroup: nblk 1, 2 and 65 (the finalize kernel's 64-row round plus its tail)
TXT_P = [1, 65, 4097]          # 64 a workgroup: nblk 1, 2 and 65

hold = _Hold()


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    hold.clear()
    E.hold.clear()
    T.hold.clear()


def test_cases_reach_every_finalize_path():
    assert [-(-P // 32) for P in BWD_P] == [1, 2, 65] and [-(-P // T.PPB) for P in TXT_P] == [1, 2, 65]
    assert [-(-P // 4) for P in FWD_P] == [1, 2, 33]


@pytest.mark.parametrize("P", FWD_P)
@pytest.mark.parametrize("NB", NBS)
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname", E.DNAMES)
def test_head_fwd_wide(zname, embed, NB, P):
    E.test_head_fwd(zname, embed, P, NB)


@pytest.mark.parametrize("P", BWD_P)
@pytest.mark.parametrize("NB", NBS)
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname,dzname", E.HEAD_DTYPES)
def test_head_bwd_wide(zname, dzname, embed, NB, P):
    """gscale = 0.625, every (dbias, dscale) NULL combination, two runs bit-equal, guarded workspace; a zero pixel row
    and one of norm 1e-3 where there are three pixels."""
    E.test_head_bwd(zname, dzname, embed, P, NB, P >= 3)


@pytest.mark.parametrize("NB", NBS)
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname,dzname", [("f32", "f32"), ("f16", "f16"), ("bf16", "bf16")])
def test_head_bwd_wide_no_gscale_zero_text_row(zname, dzname, embed, NB):
    """gscale NULL and text row NB - 1 all zero (the text clamp: tn = 0, its logit exactly 0).  The bound is
    test_head_bwd's, term by term (see its docstring), at gs = 1."""
    zdt, dzdt = DT[zname], DT[dzname]
    Lb = _lib.lib()
    P, B = 66, 2
    HW, nblk = P // B, -(-P // 32)
    Z, text, ls, anchors = E._head_inputs(P, NB, embed, zdt, True)
    text[NB - 1] = 0
    dl_up = E._randn((B, NB, HW), 7).to(torch.float32).to(F64)
    de_up = E._randn((B, HW), 8).to(torch.float32).to(F64)
    r = R.head_bwd(Z, text, ls, anchors, dl_up, de_up, 1.0, B, HW)
    assert bool((r["tn"][NB - 1] == 0).all()) and bool((r["lg"][:, NB - 1] == 0).all())
    hb = E._head_fwd_bounds(r, embed, NB)
    NV, rho_n, rho_s = hb["NV"], hb["rho_n"], hb["rho_s"]
    pa = r["pr"] * anchors.abs()
    dee = (pa * (hb["rho_q"] + (NB + 1) * U)).sum(1, keepdim=True)
    T1 = r["dlg"].abs()
    ame = (anchors - r["e"][:, None]).abs()
    T2 = (r["de"] * r["pr"]).abs() * ame
    ddl = U * T1 + T2 * (hb["rho_q"] + 3 * U) + (r["de"] * r["pr"]).abs() * (dee + U * ame) + U * (T1 + T2)
    tna = r["tn"].abs()
    ddzn = r["s"] * (ddl @ tna) + r["s"] * (r["dl"].abs() @ tna) * (rho_s + rho_n + (NB + 3) * U)
    zna = r["zn"].abs()
    ddot = (zna * ddzn + (r["zn"] * r["dzn"]).abs() * (rho_n + (NV + 8) * U)).sum(1, keepdim=True)
    inv = 1.0 / r["den"][:, None]
    zd = zna * r["dot"].abs()[:, None]
    ddz = inv * (ddzn + zna * ddot + zd * (rho_n + 2 * U) + U * (r["dzn"].abs() + zd)) + r["dz"].abs() * (rho_n + U)
    depth = -(-nblk // 64)
    dbias_b = ddz.sum(0) + (21 + depth) * U * r["dz"].abs().sum(0) + 0.5 * BR.ulp(r["dbias"], torch.float32)
    dllg = (r["dl"] * r["lg"]).abs()
    dsc_b = float((ddl * r["lg"].abs() + r["dl"].abs() * hb["dlg"] + U * dllg).sum() + (8 * NB + 13 + depth) * U * dllg.sum()
                  + 0.5 * BR.ulp(r["dscale"], torch.float32))
    need = Lb.ebc_head_bwd_workspace_bytes(P, embed)
    ptrs = (hold(Z.to(zdt)), hold(text, True), hold(ls, True), hold(anchors, True), hold(dl_up, True), hold(de_up, True))
    ws = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dZ = _guarded(P, embed, dzdt)
    dbias, dsc = E._vec(embed), E._vec(1)
    _lib.check(Lb.ebc_head_bwd(_lib.dtype_code(zdt), _lib.dtype_code(dzdt), *ptrs, None, _lib.ptr(dZ), _lib.ptr(dbias),
                               _lib.ptr(dsc), P, HW, NB, embed, _lib.ptr(ws), need, _lib.stream()), "head_bwd")
    assert _guard_ok(dZ, P) and _guard_ok(dbias, embed) and _guard_ok(dsc, 1) and bool((ws[need:] == 0xA5).all())
    fits = r["dz"].abs() < float(torch.finfo(dzdt).max) * (1 - 2.0 ** -8)
    assert torch.equal(dZ[:P].cpu()[~fits], r["dz"].to(dzdt)[~fits])
    err = torch.where(fits, (E._cpu64(dZ[:P]) - r["dz"]).abs(), torch.zeros_like(ddz))
    tag = f"head_bwd_wide[{zname},{embed},NB={NB},no gscale]"
    _report(f"{tag}.dz", err, ddz + 0.5 * BR.ulp(r["dz"], dzdt))
    _report(f"{tag}.dbias", (E._cpu64(dbias[:embed]) - r["dbias"]).abs(), dbias_b)
    _report(f"{tag}.dscale", (E._cpu64(dsc[:1]) - r["dscale"]).abs(), torch.tensor([dsc_b], dtype=F64))


# ------------------------------------------------------------------------------------------------ wide text gradient
def _launch_text(Lb, wide, zdt, ptrs, pgs, P, HW, NB, embed):
    """One launch with guard words round dtext (a sentinel frame before and after) and past the workspace."""
    fn = Lb.ebc_head_bwd_text_wide if wide else Lb.ebc_head_bwd_text
    need = (Lb.ebc_head_bwd_text_wide_workspace_bytes if wide else Lb.ebc_head_bwd_text_workspace_bytes)(P, NB, embed)
    assert need == -(-P // T.PPB) * (NB * embed + (32 if wide else 16)) * 4
    ws = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws[:need].view(torch.float32).fill_(float("nan"))
    from _kernel_checks import _Framed
    dtext = _Framed(NB, embed, torch.float32)
    _lib.check(fn(_lib.dtype_code(zdt), *ptrs, pgs, _lib.ptr(dtext.mid), P, HW, NB, embed, _lib.ptr(ws), need, _lib.stream()),
               "head_bwd_text_wide" if wide else "head_bwd_text")
    assert dtext.ok() and bool((ws[need:] == 0xA5).all())
    return dtext.mid


def _run_text(zname, embed, P, NB, B, special=False, gs=None, also_old=False):
    zdt = DT[zname]
    Lb = _lib.lib()
    HW, nblk = P // B, -(-P // T.PPB)
    Z, text, ls, anchors, dl_up, de_up, r = T._inputs(P, NB, embed, zdt, B, special, gs)
    hb = E._head_fwd_bounds(r, embed, NB)
    t = T.text_grad_ref(r, text)
    if special:
        k0 = NB // 2
        assert float(r["nrm"][1]) == 0 and float(t["tnrm"][k0]) == 0 and torch.equal(t["dt"][k0], t["g"][k0] / 1e-12)
    bound = T.text_grad_bound(r, t, hb, anchors, NB, nblk)
    ptrs = (hold(Z.to(zdt)), hold(text, True), hold(ls, True), hold(anchors, True), hold(dl_up, True), hold(de_up, True))
    pgs = None if gs is None else hold(torch.tensor([gs]), True)
    a = _launch_text(Lb, True, zdt, ptrs, pgs, P, HW, NB, embed)
    b = _launch_text(Lb, True, zdt, ptrs, pgs, P, HW, NB, embed)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))            # two launches, bit-identical
    _report(f"head_bwd_text_wide[{zname},{embed},P={P},NB={NB},nblk={nblk}]", (a.to(F64).cpu() - t["dt"]).abs(), bound)
    if also_old:
        o = _launch_text(Lb, False, zdt, ptrs, pgs, P, HW, NB, embed)
        _report(f"head_bwd_text[{zname},{embed},P={P},NB={NB}]", (o.to(F64).cpu() - t["dt"]).abs(), bound)


@pytest.mark.parametrize("P", TXT_P)
@pytest.mark.parametrize("NB", NBS)
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname", E.DNAMES)
def test_head_bwd_text_wide(zname, embed, NB, P):
    _run_text(zname, embed, P, NB, B=1)


@pytest.mark.parametrize("NB", NBS)
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname", E.DNAMES)
def test_head_bwd_text_wide_clamps_and_images_across_workgroups(zname, embed, NB):
    """An all-zero pixel row and an all-zero text row; B = 2 images of 49 pixels, so a workgroup's 64 pixels (and one
    wave's) come from both images."""
    _run_text(zname, embed, 98, NB, B=2, special=True)


@pytest.mark.parametrize("NB", [17, 32])
@pytest.mark.parametrize("embed", [512, 1024])
def test_head_bwd_text_wide_gscale(embed, NB):
    _run_text("f32", embed, 98, NB, B=2, gs=0.625)


@pytest.mark.parametrize("NB", [1, 16])
@pytest.mark.parametrize("embed", [512, 1024])
def test_wide_and_old_entry_points_meet_the_same_bound_up_to_16_bins(embed, NB):
    _run_text("f32", embed, 98, NB, B=2, also_old=True)
