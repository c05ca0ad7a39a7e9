"""ebc_head_bwd_text (head.hip head_text_bwd_kernel + head_text_finalize_kernel): the similarity head's gradient
with respect to the raw text rows, per element against a float64 restatement written here on top of tests/_enc_refs.py.

Conventions of tests/test_gpu_encoder_kernels.py: guarded outputs, the workspace sized exactly plus guard bytes, every
check prints "RATIO <name> <largest error / bound>" before it asserts, bounds first order in u = 2^-24 read off the
kernel's rounding points; the forward's errors (_head_fwd_bounds) and the error of dl are that module's."""
import pytest
import torch

import _bn_refs as BR
import _enc_refs as R
import test_gpu_encoder_kernels as E
from _kernel_checks import _Hold, _guard_ok, _guarded, _report
from ebc_amd import _lib

pytestmark = pytest.mark.gpu
F64, U, TRANS, DT, WS_GUARD = E.F64, E.U, E.TRANS, E.DT, E.WS_GUARD
PPB = 64                                  # pixels a workgroup (head.hip HEAD_TXT_PPB), 16 a wave

hold = _Hold()


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    hold.clear()


def text_grad_ref(r, text):
    """From _enc_refs.head_bwd's terms: g_k = s sum_p dl[p][k] zn_p, dt_k = (g_k - tn_k <tn_k, g_k>) / max(||t_k||, 1e-12),
    g_k / 1e-12 where the norm is clamped (F.normalize backward, as head_bwd does for the pixel rows)."""
    text = text.to(F64)
    tnrm = torch.sqrt((text * text).sum(1))
    tden = torch.clamp(tnrm, min=1e-12)
    g = r["s"] * (r["dl"].t() @ r["zn"])                                   # [NB][embed]
    tdot = torch.where(tnrm <= 1e-12, torch.zeros_like(tnrm), (r["tn"] * g).sum(1))
    return {"g": g, "tdot": tdot, "tden": tden, "tnrm": tnrm, "dt": (g - r["tn"] * tdot[:, None]) / tden[:, None]}


def _ddl(r, hb, anchors, NB):
    """The error of dl[p][k], as test_gpu_encoder_kernels.test_head_bwd charges it (the kernel forms dl the same way)."""
    pa = r["pr"] * anchors.abs()
    dee = (pa * (hb["rho_q"] + (NB + 1) * U)).sum(1, keepdim=True)
    T1 = r["dlg"].abs()
    ame = (anchors - r["e"][:, None]).abs()
    T2 = (r["de"] * r["pr"]).abs() * ame
    return U * T1 + T2 * (hb["rho_q"] + 3 * U) + (r["de"] * r["pr"]).abs() * (dee + U * ame) + U * (T1 + T2)


def text_grad_bound(r, t, hb, anchors, NB, nblk):
    """The error model test_head_bwd applies to its sums over the pixels (d bias, d scale), term by term in float64:
      raw      sum_p dl zn, zn = z inv [rho_n + u], one fma a pixel: ddl |zn| + |dl zn| (rho_n + 2 u), and the chain:
               16 pixels a wave, 3 over the waves, then the fixed-order combine, ceil(nblk / 64) a chain and 3 + 8 over
               chains and waves: depth 30 + ceil(nblk / 64)
      g        s raw: s draw + |g| (rho_s + u)
      dot      sum_p dl lg (one chain a bin): ddl |lg| + |dl| dlg + u |dl lg|, depth 16 + 2 + 11 + ceil(nblk / 64)
      dt       (g - tn dot) inv, tn = t inv [rho_n + u]: inv (dg + |tn| ddot + |tn dot| (rho_n + 2 u) + u (|g| + |tn dot|))
               + |dt| (rho_n + u) + ulp / 2; a clamped row takes g / 1e-12"""
    rho_n, rho_s = hb["rho_n"], hb["rho_s"]
    ddl = _ddl(r, hb, anchors, NB)
    zna, dla = r["zn"].abs(), r["dl"].abs()
    A = dla.t() @ zna
    blocks = -(-nblk // 64)
    draw = ddl.t() @ zna + A * (rho_n + 2 * U) + (30 + blocks) * U * A
    dg = r["s"] * draw + t["g"].abs() * (rho_s + U)
    dllg = (r["dl"] * r["lg"]).abs()
    ddot = (ddl * r["lg"].abs() + dla * hb["dlg"] + U * dllg).sum(0) + (29 + blocks) * U * dllg.sum(0)
    inv = 1.0 / t["tden"][:, None]
    td = r["tn"].abs() * t["tdot"].abs()[:, None]
    return (inv * (dg + r["tn"].abs() * ddot[:, None] + td * (rho_n + 2 * U) + U * (t["g"].abs() + td))
            + t["dt"].abs() * (rho_n + U) + 0.5 * BR.ulp(t["dt"], torch.float32))


def _inputs(P, NB, embed, zdt, B, special=False, gs=None):
    HW = P // B
    Z, text, ls, anchors = E._head_inputs(P, NB, embed, zdt, special=False)
    if special:                                        # both clamps: an all-zero pixel row and an all-zero text row
        Z[1] = 0
        text[NB // 2] = 0
    dl_up = E._randn((B, NB, HW), 7).to(torch.float32).to(F64)
    de_up = E._randn((B, HW), 8).to(torch.float32).to(F64)
    r = R.head_bwd(Z, text, ls, anchors, dl_up, de_up, 1.0 if gs is None else gs, B, HW)
    return Z, text, ls, anchors, dl_up, de_up, r


def _launch(Lb, zdt, ptrs, pgs, P, HW, NB, embed, need):
    ws = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws[:need].view(torch.float32).fill_(float("nan"))
    dtext = _guarded(NB, embed, torch.float32)
    _lib.check(Lb.ebc_head_bwd_text(_lib.dtype_code(zdt), *ptrs, pgs, _lib.ptr(dtext), P, HW, NB, embed, _lib.ptr(ws), need,
                                    _lib.stream()), "head_bwd_text")
    assert _guard_ok(dtext, NB) and bool((ws[need:] == 0xA5).all())
    return dtext


def _run_case(zname, embed, P, NB, B, special=False, gs=None):
    zdt = DT[zname]
    Lb = _lib.lib()
    HW = P // B
    nblk = -(-P // PPB)
    Z, text, ls, anchors, dl_up, de_up, r = _inputs(P, NB, embed, zdt, B, special, gs)
    hb = E._head_fwd_bounds(r, embed, NB)
    t = text_grad_ref(r, text)
    if special:
        k0 = NB // 2
        assert float(r["nrm"][1]) == 0 and float(t["tnrm"][k0]) == 0 and torch.equal(t["dt"][k0], t["g"][k0] / 1e-12)
    bound = text_grad_bound(r, t, hb, anchors, NB, nblk)
    need = Lb.ebc_head_bwd_text_workspace_bytes(P, NB, embed)
    assert need == nblk * (NB * embed + 16) * 4
    ptrs = (hold(Z.to(zdt)), hold(text, True), hold(ls, True), hold(anchors, True), hold(dl_up, True), hold(de_up, True))
    pgs = None if gs is None else hold(torch.tensor([gs]), True)
    a = _launch(Lb, zdt, ptrs, pgs, P, HW, NB, embed, need)
    b = _launch(Lb, zdt, ptrs, pgs, P, HW, NB, embed, need)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))            # two launches, bit-identical
    _report(f"head_bwd_text[{zname},{embed},P={P},NB={NB},nblk={nblk}]", (a[:NB].to(F64).cpu() - t["dt"]).abs(), bound)


# P = 1: one pixel, one workgroup; 65: one workgroup and one pixel (a ragged last workgroup); 64 * 64 + 1: 65 workgroups,
# the smallest count at which wave 0 of head_text_finalize_kernel runs its eight-chain main loop (0 + 56 < nblk) AND its
# tail (block 64) -- nblk = 65 of test_head_bwd_cases_reach_every_finalize_path, at this kernel's 64 pixels a workgroup
P_CASES = [1, 65, 64 * 64 + 1]


def test_cases_reach_both_finalize_loops():
    nblk = [-(-P // PPB) for P in P_CASES]
    assert nblk == [1, 2, 65] and nblk[2] == [-(-P // 32) for P, _, _ in E.HEAD_BWD][6]
    assert 0 + 56 < nblk[2] and nblk[2] > 64 and all(0 + 56 >= n for n in range(1, 57))


@pytest.mark.parametrize("P", P_CASES)
@pytest.mark.parametrize("NB", [1, 7, 16])
@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname", E.DNAMES)
def test_head_bwd_text(zname, embed, NB, P):
    _run_case(zname, embed, P, NB, B=1)


@pytest.mark.parametrize("embed", [512, 1024])
@pytest.mark.parametrize("zname", E.DNAMES)
def test_head_bwd_text_clamps_and_images_across_workgroups(zname, embed):
    """An all-zero pixel row and an all-zero text row (both F.normalize clamps); B = 2 images of HW = 49 pixels: 64 is no
    multiple of 49, so a workgroup's pixels (and one wave's) come from both images."""
    _run_case(zname, embed, 98, 5, B=2, special=True)


@pytest.mark.parametrize("embed", [512, 1024])
def test_head_bwd_text_gscale(embed):
    _run_case("f32", embed, 98, 7, B=2, gs=0.625)


@pytest.mark.parametrize("embed", [512, 1024])
def test_head_bwd_is_bit_identical_around_a_text_launch(embed):
    """The frozen path: ebc_head_bwd's dZ / d bias / d scale alone, and between two text-gradient launches on the same
    stream (which share nothing with it but the inputs)."""
    Lb = _lib.lib()
    P, NB, B = 270, 12, 2
    HW = P // B
    Z, text, ls, anchors, dl_up, de_up, _ = _inputs(P, NB, embed, torch.float32, B)
    ptrs = (hold(Z.to(torch.float32)), hold(text, True), hold(ls, True), hold(anchors, True), hold(dl_up, True),
            hold(de_up, True))
    need = Lb.ebc_head_bwd_workspace_bytes(P, embed)
    need_t = Lb.ebc_head_bwd_text_workspace_bytes(P, NB, embed)

    def bwd():
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        dZ, dbias, dsc = _guarded(P, embed, torch.float16), E._vec(embed), E._vec(1)
        _lib.check(Lb.ebc_head_bwd(_lib.EBC_F32, _lib.EBC_F16, *ptrs, None, _lib.ptr(dZ), _lib.ptr(dbias), _lib.ptr(dsc), P, HW,
                                   NB, embed, _lib.ptr(ws), need, _lib.stream()), "head_bwd")
        return dZ, dbias, dsc

    alone = bwd()
    _launch(Lb, torch.float32, ptrs, None, P, HW, NB, embed, need_t)
    between = bwd()
    _launch(Lb, torch.float32, ptrs, None, P, HW, NB, embed, need_t)
    torch.cuda.synchronize()
    for x, y in zip(alone, between):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
