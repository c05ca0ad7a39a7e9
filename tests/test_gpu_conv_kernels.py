"""The implicit-GEMM 3x3 convolutions (conv_gemm MODE 1 / MODE 2 of csrc/gemm.hip, splitk_reduce_kernel, the stream-K path
and the EPI_STATS / EPI_ADD_RELU_GRAD epilogues) per element against the float64 references of tests/_conv_refs.py,
through ebc_conv3x3_fwd, ebc_conv3x3_fwd_bn and ebc_conv3x3_wgrad.

Every case first pins the plan it means to run (ebc_conv_tile_config: tile id, tile rows and columns, and 1 = one
launch, 2 = the last-arriver split, s > 2 = s f32 partials + splitk_reduce_kernel, -G = stream-K on G workgroups), then
runs it
  * on dyadic operands (multiples of 1/8 in [-2, 2]: every product is a multiple of 1/64 and every partial sum stays
    below 2^24 / 64, exact in f32 in any order and however K is cut), where the outputs and the column sums must equal
    the reference bit for bit (rounded once to a 16-bit T); the sums of squares are bit-exact wherever every tile
    row's sum stays below 2^24 times their spacing 2^-12 and are held to the bound elsewhere;
  * on Gaussian operands, every element held to the bound _conv_refs counts from the kernel's rounding points
    (RATIO lines: largest error / bound).
Every output sits in a sentinel frame; the workspace is exactly ebc_dec_workspace_bytes long with a guard behind it and
its 16 KiB counter block must be zero again after every call; every call runs twice and must repeat bit for bit; the
reference product and the bounds are computed on the device in float64.

MODE 1 images carry a non-zero frame (the reference reads the image as given, so a tap that lands on the wrong cell at
a border moves the element) and NaN in the alignment columns xp >= W + 2.  The kernel's A address of row (b, y, x) and
tap (ky, kx) is cell (y + ky, x + kx) with x + kx <= W + 1, rows past M are clamped to row M - 1: no slack cell is ever
read, so every output must be what a zero slack gives, bit for bit.

MODE 2: column b * HWp + r of dzT meets position b * Pimg + ky * W + r of xT3's row, which for r >= H * W is the image's
next rows (real data for ky < 2): dzT's padding columns inside Kq must be zero, and xT3 is whatever
ebc_dec_transpose3 writes (include/ebc_hip.h states this).  The test zeroes dzT's padding and overwrites the positions
of xT3 that belong to no image row (past (H + 2) * W of every image, past the last image), which only padding columns
of dzT ever meet, and dzT's never-read columns >= Kq, with a finite sentinel.

Plans reachable over B in 1..31, H in 7..56, C, N in 64..768 (ebc_conv_tile_config), all covered here:
  MODE 1 16-bit: tile 2, 13, 17 plain; tile 3 and 7 plain and stream-K;   f32: tile 2 plain
  MODE 2 16-bit: tile 2, 13, 3: plain, 2-split, partials; tile 3 stream-K (even and aligned shares); tile 7 partials
  MODE 2 f32: tile 2 plain, 2-split, partials
(tile 7 never runs a MODE 2 plan other than partials there, tile 17 is MODE 1 only.)
Largest error / bound measured on an MI355X, Gaussian runs: 0.886 behind a bf16 store and 0.508 behind an f16 store (the
store's own half ulp; exactly 1.0 at the dyadic runs' ties), 0.004 for f32 outputs, 1e-4 / 3e-4 for the column sums /
sums of squares (0.118 for the dyadic sums of squares, whose bound has no accumulator term), 0.013 for the weight
gradients: the 2 units per K step are far above what the MFMA accumulation loses, so the f32-side outputs are pinned
mostly by the dyadic runs' bit-exactness."""
import ctypes

import pytest
import torch

import _conv_refs as R
from _kernel_checks import F64, GUARD_ROWS, SENT, _Framed, _exact, _report
from ebc_amd import _lib

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CNT_BYTES = 16 * 1024
TILES = {2: (128, 64), 3: (256, 192), 7: (256, 256), 13: (128, 96), 17: (224, 192)}
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
MOM = float(torch.tensor(0.1, dtype=torch.float32))


def _pin(dt, mode, M, N, K, tile, splits):
    out = (ctypes.c_int * 3)()
    got = _lib.lib().ebc_conv_tile_config(_lib.dtype_code(dt), mode, M, N, K, out)
    assert (got, out[0], out[1], out[2]) == (tile, *TILES[tile], splits), (mode, M, N, K, got, tuple(out))


def _workspace(dt, B, H, W, C, N):
    need = _lib.lib().ebc_dec_workspace_bytes(_lib.dtype_code(dt), B, H, W, C, N)
    ws = torch.zeros(need + 4096, dtype=torch.uint8, device="cuda")          # exactly `need` bytes, then a guard
    ws[need:] = 0xA5
    return ws, need


def _ws_ok(ws, need):
    return int(ws[:CNT_BYTES].count_nonzero()) == 0 and bool((ws[need:] == 0xA5).all())


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _eighths(g, *shape):
    """Multiples of 1/8 in [-2, 2]."""
    return torch.randint(-16, 17, shape, device="cuda", generator=g).to(torch.float32) / 8


def _held(name, out, ref, bound):
    _report(name, (out.to(F64) - ref).abs(), bound.clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ MODE 1
# (B, H, W, C, N) -> (tile, ebc_conv_tile_config's out[2]); every M = B * H * W ends inside a tile row
FWD16 = [((1, 7, 7, 64, 64), (2, 1)), ((3, 6, 10, 64, 128), (2, 1)),                 # one tile; 2 x 2 tiles, ragged
         ((1, 5, 30, 64, 64), (2, 1)), ((1, 4, 31, 64, 64), (2, 1)),                 # Wp 32 at W = 30, 40 at W = 31
         ((1, 7, 7, 64, 192), (13, 1)), ((2, 14, 14, 64, 192), (13, 1)),
         ((13, 28, 28, 64, 768), (17, 1)),
         ((21, 56, 56, 64, 192), (3, 1)), ((21, 56, 56, 64, 256), (7, 1)),           # more tiles than CUs, one launch
         ((21, 56, 56, 512, 192), (3, -8)), ((21, 56, 56, 512, 256), (7, -8)),       # 2 tail tiles, 4 whole pieces each
         ((31, 28, 28, 256, 768), (3, -256)), ((31, 56, 56, 256, 256), (7, -256))]   # shares cross tile edges
FWD32 = [((2, 7, 7, 64, 64), (2, 1)), ((3, 6, 10, 64, 128), (2, 1)), ((1, 4, 31, 64, 64), (2, 1))]


class _FwdOps:
    """One MODE 1 shape's operands as the kernel receives them, and their float64 product."""

    def __init__(self, dt, shape, dyadic, seed):
        B, H, W, C, N = shape
        self.dyadic = dyadic
        g, geo = _gen(seed), R.geometry(B, H, W)
        draw = (lambda *s: _eighths(g, *s)) if dyadic else (lambda *s: torch.randn(*s, device="cuda", generator=g))
        x, frame = draw(B, H, W, C).to(dt), draw(B, geo["Hp"], geo["Wp"], C).to(dt)
        if dyadic:
            frame[frame == 0] = 0.125                                         # the frame cells are non-zero
        self.wk = (draw(N, 3, 3, C) if dyadic else draw(N, 3, 3, C) / (9 * C) ** 0.5).to(dt).contiguous()
        self.xnan = R.pad_image(x, geo, pad_fill=frame, slack_fill=float("nan")).contiguous()
        self.xzero = R.pad_image(x, geo, pad_fill=frame, slack_fill=0.0).contiguous()
        assert bool(self.xnan[:, :, W + 2:].isnan().all()) and not bool(self.xzero.isnan().any())
        M = B * H * W
        self.gy = draw(M, N).to(dt)
        # the ReLU output the mask reads: negative values, -0.0, +0.0 and positive values
        y = draw(M, N)
        sel = torch.randint(0, 4, (M, N), device="cuda", generator=g)
        y = torch.where(sel == 0, torch.zeros_like(y), torch.where(sel == 1, -torch.zeros_like(y), y)).to(dt)
        assert bool((y < 0).any()) and bool((y > 0).any()) and bool(((y == 0) & y.signbit()).any())
        assert bool(((y == 0) & ~y.signbit()).any())
        self.y = y
        self.P, self.Sp = R.conv_fwd(self.xzero, self.wk, geo, with_abs=not dyadic)
        if dyadic:
            self.Sp = torch.zeros_like(self.P)                                 # exact accumulators: no f32-side error


def _fwd_call(dt, shape, ops, xpad, epi, ws, need):
    """One ebc_conv3x3_fwd call: (out frame, colsum frame or None)."""
    B, H, W, C, N = shape
    L, M = _lib.lib(), B * H * W
    out = _Framed(M, N, dt)
    cs = _Framed(2, N, F64) if epi == 4 else None
    gy, y = (ops.gy, ops.y) if epi == 5 else (None, None)
    rc = L.ebc_conv3x3_fwd(_lib.dtype_code(dt), _lib.ptr(xpad), _lib.ptr(ops.wk), _lib.ptr(out.mid),
                           _lib.ptr(cs.mid) if cs else None, _lib.ptr(gy), _lib.ptr(y), _lib.ptr(ws) if ws is not None else None,
                           need if ws is not None else 0, B, H, W, C, N, _lib.stream())
    _lib.check(rc, "ebc_conv3x3_fwd")
    torch.cuda.synchronize()
    assert out.ok() and (cs is None or cs.ok())
    assert ws is None or _ws_ok(ws, need)
    return out, cs


def _check_fwd(tag, dt, shape, ops, epi, bm, pieces, out, cs):
    C = shape[3]
    K = 9 * C
    if epi == 5:
        ref = R.add_relu_grad(ops.P, ops.gy, ops.y)
        d = R.add_relu_grad_bound(ops.Sp, ops.gy, K, pieces, dt) if not ops.dyadic else torch.zeros_like(ref)
    else:
        ref, d = ops.P, R.acc_bound(ops.Sp, K, pieces, dt)
    _held(tag + ".out", out.mid, ref, R.held(ref, d, dt))
    if ops.dyadic:
        _exact(out.mid, ref, dt)
    if cs is not None:
        s, q = R.stats(ops.P)
        bs, bq = R.stats_bound(ops.P, R.acc_bound(ops.Sp, K, pieces, dt), bm)
        _held(tag + ".col_s", cs.mid[0], s, bs)
        _held(tag + ".col_q", cs.mid[1], q, bq)
        if ops.dyadic:
            assert bool(R.stats_exact_in_f32(ops.P, bm, 2.0 ** -6).all()), "not a dyadic case: a tile row's sum leaves f32"
            assert torch.equal(cs.mid[0], s), int((cs.mid[0] != s).sum())
            sq = R.stats_exact_in_f32(ops.P * ops.P, bm, 2.0 ** -12)
            assert torch.equal(cs.mid[1][sq], q[sq]), int((cs.mid[1][sq] != q[sq]).sum())


def _run_fwd(dname, shape, plan):
    dt = DT[dname]
    B, H, W, C, N = shape
    tile, splits = plan
    M, bm = B * H * W, TILES[tile][0]
    _pin(dt, 1, M, N, 9 * C, tile, splits)
    assert M % bm != 0
    streamk = splits < 0
    pieces = 4 if streamk else 1
    ws, need = _workspace(dt, B, H, W, C, N)
    for dyadic in (True, False):
        ops = _FwdOps(dt, shape, dyadic, seed=M * 31 + N + C + (1 if dyadic else 0))
        tag = f"fwd.{dname}.t{tile}.s{splits}.{B}x{H}x{W}x{C}x{N}.{'dyadic' if dyadic else 'random'}"
        for epi in (0, 4, 5):
            a, acs = _fwd_call(dt, shape, ops, ops.xnan, epi, ws, need)
            _check_fwd(f"{tag}.epi{epi}", dt, shape, ops, epi, bm, pieces, a, acs)
            b, bcs = _fwd_call(dt, shape, ops, ops.xnan, epi, ws, need)               # again: re-armed counters
            z, zcs = _fwd_call(dt, shape, ops, ops.xzero, epi, ws, need)              # zero slack: the same bits
            assert torch.equal(a.mid, b.mid) and torch.equal(a.mid, z.mid), tag
            if acs is not None:
                assert torch.equal(acs.mid, bcs.mid) and torch.equal(acs.mid, zcs.mid), tag
            if streamk and epi != 4:
                # no workspace, no colsum: the plain launch of the same tile, held to the same bound
                p, _ = _fwd_call(dt, shape, ops, ops.xnan, epi, None, 0)
                _check_fwd(f"{tag}.epi{epi}.plain", dt, shape, ops, epi, bm, 1, p, None)


def _fid(v):
    return "x".join(map(str, v)).replace("-", "sk")


@pytest.mark.parametrize("dname", ["f16", "bf16"])
@pytest.mark.parametrize("shape,plan", FWD16, ids=_fid)
def test_conv_fwd_16bit_every_plan_and_epilogue(dname, shape, plan):
    _run_fwd(dname, shape, plan)


@pytest.mark.parametrize("shape,plan", FWD32, ids=_fid)
def test_conv_fwd_f32_every_epilogue(shape, plan):
    _run_fwd("f32", shape, plan)


@pytest.mark.parametrize("dname", ["bf16", "f32"])
def test_conv_fwd_bn_equals_unfused(dname):
    """ebc_conv3x3_fwd_bn = ebc_conv3x3_fwd(colsum) + ebc_bn_finalize bit for bit in every output (f16:
    test_gpu_bn_kernels.py), at 3 x 6 x 10: two tile rows, the last one ragged."""
    dt, L = DT[dname], _lib.lib()
    shape = B, H, W, C, N = 3, 6, 10, 64, 128
    code, M = _lib.dtype_code(dt), B * H * W
    ops = _FwdOps(dt, shape, False, seed=77)
    g = _gen(78)
    gamma, beta = torch.rand(N, device="cuda", generator=g) + 0.5, torch.randn(N, device="cuda", generator=g)
    rm0, rv0 = torch.randn(N, device="cuda", generator=g), torch.rand(N, device="cuda", generator=g) + 0.5
    res = []
    for fused in (False, True):
        ws, need = _workspace(dt, B, H, W, C, N)
        out, cs = _Framed(M, N, dt), _Framed(2, N, F64)
        outs = [torch.full((N + GUARD_ROWS,), SENT, device="cuda") for _ in range(4)]
        rm, rv, nbt = rm0.clone(), rv0.clone(), torch.tensor([5], dtype=torch.int64, device="cuda")
        if fused:
            _lib.check(L.ebc_conv3x3_fwd_bn(code, _lib.ptr(ops.xnan), _lib.ptr(ops.wk), _lib.ptr(out.mid), _lib.ptr(ws), need, B,
                                            H, W, C, N, EPS, MOM, _lib.ptr(gamma), _lib.ptr(beta),
                                            *[_lib.ptr(o) for o in outs], _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt),
                                            _lib.ptr(cs.mid), _lib.stream()), "conv_bn")
        else:
            _lib.check(L.ebc_conv3x3_fwd(code, _lib.ptr(ops.xnan), _lib.ptr(ops.wk), _lib.ptr(out.mid), _lib.ptr(cs.mid), None,
                                         None, _lib.ptr(ws), need, B, H, W, C, N, _lib.stream()), "conv")
            _lib.check(L.ebc_bn_finalize(_lib.ptr(cs.mid), float(M), EPS, MOM, _lib.ptr(gamma), _lib.ptr(beta),
                                         *[_lib.ptr(o) for o in outs], _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt), N,
                                         _lib.stream()), "finalize")
        assert out.ok() and cs.ok() and _ws_ok(ws, need) and all(bool((o[N:] == SENT).all()) for o in outs)
        res.append([out.mid, cs.mid] + outs + [rm, rv, nbt])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert int(res[0][-1]) == 6 and not bool(res[0][0].isnan().any())


# ------------------------------------------------------------------------------------------------ MODE 2
WG_SENT = 3.0                # finite, non-zero, dyadic: a padding cell of xT3 that met a non-zero dzT column would show
# (B, H, W, C, N) -> (tile, out[2]): 1 no split, 2 the last arriver adds the other piece, s > 2 f32 partials and a
# reduce launch, -G stream-K
WG16 = [((1, 7, 7, 64, 64), (2, 1)), ((3, 10, 10, 64, 128), (2, 1)),             # one k-tile; 312 columns in Kq = 320
        ((3, 6, 10, 64, 128), (2, 1)),                                           # H != W
        ((5, 14, 14, 64, 64), (2, 2)), ((24, 10, 10, 64, 64), (2, 3)),           # (5 x 200 = 1000 columns in 1024)
        ((8, 7, 7, 512, 512), (13, 1)), ((5, 14, 14, 512, 192), (13, 2)), ((16, 14, 14, 384, 64), (13, 5)),
        ((8, 7, 7, 768, 768), (3, 1)), ((5, 14, 14, 512, 768), (3, 2)), ((6, 56, 56, 256, 64), (3, 21)),
        ((12, 14, 14, 768, 768), (3, -256)),                                     # stream-K, even shares
        ((16, 28, 28, 768, 768), (3, -252)),                                     # stream-K, shares of 84 k-tiles
        ((4, 56, 56, 512, 64), (7, 14))]
WG32 = [((3, 10, 10, 64, 128), (2, 1)), ((3, 6, 10, 64, 128), (2, 1)), ((4, 28, 28, 256, 256), (2, 2)),
        ((8, 28, 28, 256, 256), (2, 7))]


def _run_wgrad(dname, shape, plan):
    dt, L = DT[dname], _lib.lib()
    B, H, W, C, N = shape
    tile, splits = plan
    code, geo = _lib.dtype_code(dt), R.geometry(B, H, W)
    Kq, Qs = geo["Kq"], geo["Qs"]
    _pin(dt, 2, N, 9 * C, Kq, tile, splits)
    if splits == -252:
        assert Kq // 64 == 196 and 108 * 196 == 252 * 84           # the aligned shares of 84 k-tiles; -256: even shares
    pieces = 4 if splits < 0 else splits
    ws, need = _workspace(dt, B, H, W, C, N)
    pad = R.xT3_padding_mask(geo, device="cuda")
    for dyadic in (True, False):
        g = _gen(B * 1009 + H * W + C + N + (1 if dyadic else 0))
        if dyadic:
            x, dz = _eighths(g, B, H, W, C).to(dt), _eighths(g, B, H, W, N).to(dt)
        else:
            x = torch.randn(B, H, W, C, device="cuda", generator=g).to(dt)
            dz = (torch.randn(B, H, W, N, device="cuda", generator=g) / (B * H * W) ** 0.5).to(dt)
        xpad = R.pad_image(x, geo, pad_fill=0.0, slack_fill=float("nan")).contiguous()
        xT3 = torch.full((3, C, Qs), SENT, dtype=dt, device="cuda")
        _lib.check(L.ebc_dec_transpose3(code, _lib.ptr(xpad), _lib.ptr(xT3), B, H, W, C, _lib.stream()), "transpose3")
        assert not bool(xT3.isnan().any()) and int(xT3[:, :, pad].count_nonzero()) == 0
        xT3[:, :, pad] = WG_SENT
        dzT = R.dz_transposed(dz, geo, fill=0.0, tail_fill=WG_SENT).contiguous()
        ref, Sp = R.conv_wgrad(dz, x, with_abs=not dyadic)
        ref = ref.reshape(N, 9 * C)
        bound = R.acc_bound(Sp.reshape(N, 9 * C), Kq, pieces, dt) if not dyadic else torch.zeros_like(ref)
        tag = f"wgrad.{dname}.t{tile}.s{splits}.{B}x{H}x{W}x{C}x{N}.{'dyadic' if dyadic else 'random'}"
        outs = []
        for _ in range(2):
            dw = _Framed(N, 9 * C, torch.float32)
            _lib.check(L.ebc_conv3x3_wgrad(code, _lib.ptr(dzT), _lib.ptr(xT3), _lib.ptr(dw.mid), _lib.ptr(ws), need, B, H, W, C,
                                           N, _lib.stream()), "ebc_conv3x3_wgrad")
            torch.cuda.synchronize()
            assert dw.ok() and _ws_ok(ws, need), tag
            _held(tag, dw.mid, ref, bound)
            if dyadic:
                _exact(dw.mid, ref, torch.float32)
            outs.append(dw.mid)
        assert torch.equal(outs[0], outs[1]), tag


def _kind(s):
    return "plain" if s == 1 else "split2" if s == 2 else "partials" if s > 2 else "stream-K"


def test_every_reachable_plan_is_covered():
    """The (operand width, mode, tile, split kind) combinations ebc_conv_tile_config hands out over a grid of decoder
    shapes are exactly the ones the case lists above run: a planner change that opens a new path, or closes a listed
    one, fails here."""
    L, out = _lib.lib(), (ctypes.c_int * 3)()
    found = set()
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        bits = 32 if dt == torch.float32 else 16
        for B in (1, 2, 3, 5, 8, 12, 13, 16, 21, 24, 31):
            for H in (7, 10, 14, 28, 56):
                for C in (64, 256, 384, 512, 768):
                    for N in (64, 128, 192, 256, 512, 768):
                        for mode, (m, n, k) in ((1, (B * H * H, N, 9 * C)), (2, (N, 9 * C, R.geometry(B, H, H)["Kq"]))):
                            tile = L.ebc_conv_tile_config(_lib.dtype_code(dt), mode, m, n, k, out)
                            found.add((bits, mode, tile, _kind(out[2])))
    covered = {(16, 1, t, _kind(s)) for _, (t, s) in FWD16} | {(32, 1, t, _kind(s)) for _, (t, s) in FWD32}
    covered |= {(16, 2, t, _kind(s)) for _, (t, s) in WG16} | {(32, 2, t, _kind(s)) for _, (t, s) in WG32}
    assert found == covered, (sorted(found - covered), sorted(covered - found))


@pytest.mark.parametrize("dname", ["f16", "bf16"])
@pytest.mark.parametrize("shape,plan", WG16, ids=_fid)
def test_conv_wgrad_16bit_every_plan(dname, shape, plan):
    _run_wgrad(dname, shape, plan)


@pytest.mark.parametrize("shape,plan", WG32, ids=_fid)
def test_conv_wgrad_f32_every_plan(shape, plan):
    _run_wgrad("f32", shape, plan)
