"""gemm_nt_kernel, splitk_reduce_kernel and transpose_kernel (csrc/gemm.hip) per element against the float64 references
of tests/_gemm_refs.py, through ebc_gemm, ebc_gemm_rows, ebc_gemm_wgrad and ebc_transpose.

Every case first pins the kernel instance it runs (ebc_gemm_tile_config / ebc_gemm_wgrad_tile_config), then runs it
  * on dyadic operands (A integers in [-4, 4], B in {-1, -1/2, 0, 1/2, 1}, integer bias, resid multiples of 1/2): every
    partial sum is a multiple of 1/2 below 2^23, exact in f32 in any order, so STORE / RESID outputs and GELU's aux must
    equal the reference bit for bit (rounded once to a 16-bit T);
  * on random operands (A ~ N(0, 1), B ~ N(0, 1/K), bias, resid ~ N(0, 1)), every element held to the bound
    _gemm_refs.epilogue derives from the kernel's rounding points (RATIO lines: largest error / bound).
The reference product and the bounds are computed on the device in float64.  Every output sits in a sentinel frame with
guard rows before and after it.

What the kernel's own constants make of the shape list: the two-half epilogue operand load (PH = 2) exists on tiles 3 and
7 only (tile 4's waves own 3 row fragments, an odd count); the 96-wide tiles' narrowest product has N = 192 (N = 96 is
no ebc_gemm shape: N % 64); 1100 rows of 12 tile columns make three even groups of tile rows, 1153 a last group of one.
Largest error / bound measured on an MI355X: 0.994 behind a bf16 store and 0.961 behind an f16 store (the store's own
half ulp), 0.022 for the f32 outputs of 16-bit products, 0.095 for f32 products, 0.026 for ebc_gemm_wgrad."""
import ctypes

import pytest
import torch

import _gemm_refs as R
from _kernel_checks import F64, SENT, _Framed, _Hold, _exact, _report
from ebc_amd import _lib

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# tile id -> (rows BM, columns BN, wave rows WGM); a wave owns WM = BM / WGM rows of its tile
TILES = {1: (128, 128, 2), 2: (128, 64, 2), 3: (256, 192, 4), 4: (192, 192, 4), 5: (128, 96, 2), 7: (256, 256, 4),
         15: (128, 96, 2), 16: (128, 96, 2)}
SMALL_M = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129]


def _edge_m(tile, m0):
    """m0 is the smallest M that reaches the tile (its last tile holds one row): the last tile ending inside the first
    16-row fragment, inside a wave's rows, past a wave-row boundary, and full."""
    bm, _, wgm = TILES[tile]
    assert (m0 - 1) % bm == 0
    return [m0, m0 + 15, m0 + bm // wgm - 1, m0 + bm // wgm + 1, m0 - 1 + bm]


def _cases16():
    c = [(2, M, N, K) for M in SMALL_M for N, K in ((64, 64), (128, 128), (64, 192), (128, 832))]
    # 12 tile columns: grouped tile order, group_m 3 over 9 tile rows (even groups) and over 10 (a last group of one)
    c += [(2, 1100, 768, 64), (2, 1153, 768, 64)]
    # (N = 96 itself is no ebc_gemm shape, N % 64: the narrowest products of the 96-wide tiles have N = 192)
    c += [(15, M, N, K) for M in SMALL_M for N in (192, 768) for K in (768, 832, 896)]          # 3-stage ring
    c += [(16, M, N, K) for M in SMALL_M for N in (192, 768) for K in (2304, 2368, 2432, 2496)]  # 4-stage ring
    c += [(5, M, 768, 768) for M in _edge_m(5, 4097)] + [(5, 4097, 768, 832)]                   # (needs K >= 768)
    for tile, m0, N in ((1, 8065, 512), (4, 1921, 2304), (3, 2305, 3072), (7, 7937, 3072)):
        c += [(tile, M, N, 64) for M in _edge_m(tile, m0)]
        c += [(tile, m0, N, K) for K in (128, 192, 832, 768)]
    c += [(4, M, 960, 64) for M in _edge_m(4, 4801)]            # 5 tile columns: not grouped
    c += [(7, M, 1024, 64) for M in _edge_m(7, 24321)]          # 4 tile columns: not grouped
    return c


def _cases32():
    c = [(2, M, N, K) for M in SMALL_M for N, K in ((64, 32), (128, 64), (64, 96), (128, 800))]
    return c + [(2, 300, 768, 32), (2, 300, 768, 96)]           # group_m 2 over 3 tile rows: a last group of one


CASES16, CASES32 = _cases16(), _cases32()
# (name, epilogue, out_f32, keeps aux, in place)
VARIANTS = [("store_T", R.STORE, 0, False, False), ("store_f32", R.STORE, 1, False, False),
            ("gelu_aux", R.GELU, 0, True, False), ("gelu_noaux", R.GELU, 0, False, False),
            ("resid_f32_inplace", R.RESID, 1, False, True), ("resid_f32", R.RESID, 1, False, False),
            ("resid_T", R.RESID, 0, False, False), ("gelu_bwd", R.GELU_BWD, 0, False, False)]
# f32 operands have one output type: the two f32-output variants would repeat the others
VARIANTS32 = [v for v in VARIANTS if v[0] not in ("store_f32", "resid_T")]


def _pin(dt, M, N, K, tile):
    out = (ctypes.c_int * 3)()
    got = _lib.lib().ebc_gemm_tile_config(_lib.dtype_code(dt), M, N, K, out)
    assert (got, out[0], out[1], out[2]) == (tile, TILES[tile][0], TILES[tile][1], 1), (M, N, K)


class _Ops:
    """One shape's operands, as the kernel receives them, the float64 product and |A|.|B|^T (shared by its variants)."""

    def __init__(self, dt, M, N, K, dyadic, seed, a_rows=None):
        g = torch.Generator(device="cuda").manual_seed(seed)
        ar = a_rows or M

        def ints(lo, hi, *shape):
            return torch.randint(lo, hi + 1, shape, device="cuda", generator=g).to(torch.float32)

        def normal(*shape):
            return torch.randn(*shape, device="cuda", generator=g)

        if dyadic:
            self.A, self.B = ints(-4, 4, ar, K).to(dt), (ints(-2, 2, N, K) / 2).to(dt)
            self.bias, self.resid = ints(-8, 8, N), ints(-16, 16, M, N) / 2
        else:
            self.A, self.B = normal(ar, K).to(dt), (normal(N, K) / K ** 0.5).to(dt)
            self.bias, self.resid = normal(N), normal(M, N)
        self.aux = normal(M, N).to(dt)              # GELU': the stored pre-activation, as given
        self.dyadic = dyadic


def _held(name, out, ref, bound):
    _report(name, (out.to(F64) - ref).abs(), bound.clamp_min(1e-300))


def _run_variant(dt, M, N, K, ops, P, Sp, var, use_bias, tag):
    name, epi, of32, keep_aux, inplace = var
    L, h = _lib.lib(), _Hold()
    out_dt = torch.float32 if (of32 or dt == torch.float32) else dt
    C = _Framed(M, N, out_dt)
    bias = ops.bias if use_bias else None
    resid = aux = auxf = None
    if epi == R.RESID:
        resid = ops.resid
        if inplace:
            C.mid.copy_(ops.resid)
            resid = C.mid
    if epi == R.GELU and keep_aux:
        auxf = _Framed(M, N, dt)
        aux = auxf.mid
    if epi == R.GELU_BWD:
        aux = ops.aux
    rc = L.ebc_gemm(_lib.dtype_code(dt), epi, of32, h(ops.A), h(ops.B), _lib.ptr(C.mid), _lib.ptr(bias), _lib.ptr(resid),
                    _lib.ptr(aux), M, N, K, _lib.stream())
    _lib.check(rc, "ebc_gemm")
    refs = R.epilogue(epi, P, Sp, K, dt, out_dt, bias=bias, resid=ops.resid, aux=ops.aux)
    tag = f"{tag}.{name}{'+bias' if use_bias else ''}"
    _held(tag + ".C", C.mid, *refs["C"])
    if auxf is not None:
        _held(tag + ".aux", auxf.mid, *refs["aux"])
        assert auxf.ok(), tag
    assert C.ok(), tag
    if ops.dyadic:
        if epi in (R.STORE, R.RESID):
            _exact(C.mid, refs["C"][0], out_dt)
        if auxf is not None:
            _exact(auxf.mid, refs["aux"][0], dt)


def _run_shape(dname, tile, M, N, K, variants):
    dt = DT[dname]
    _pin(dt, M, N, K, tile)
    for dyadic in (True, False):
        ops = _Ops(dt, M, N, K, dyadic, seed=M * 7919 + N * 31 + K + (1 if dyadic else 0))
        P, Sp = R.product(ops.A, ops.B)
        tag = f"{dname}.t{tile}.{M}x{N}x{K}.{'dyadic' if dyadic else 'random'}"
        for var in variants:
            for use_bias in ((False,) if var[1] == R.GELU_BWD else (True, False)):       # GELU' takes no bias
                _run_variant(dt, M, N, K, ops, P, Sp, var, use_bias, tag)


def _id(c):
    return "t%d-%dx%dx%d" % c


@pytest.mark.parametrize("dname", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASES16, ids=_id)
def test_gemm_16bit_every_tile_and_epilogue(dname, case):
    _run_shape(dname, *case, VARIANTS)


@pytest.mark.parametrize("case", CASES32, ids=_id)
def test_gemm_f32_every_epilogue(case):
    _run_shape("f32", *case, VARIANTS32)


# ------------------------------------------------------------------------------------------------ ebc_gemm_rows
ROWS_POISON = 512.0          # exact in every type; a row of it read by mistake moves an output by hundreds


@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("M", [15, 13])
@pytest.mark.parametrize("K", [768, 2304])
def test_gemm_rows_prompt_rows(dname, M, K):
    """Layer 0's prompt rows at their smallest: groups of 5 rows starting at row 1 of every 23; M = 13 ends inside a
    group.  The A rows outside the groups hold ROWS_POISON."""
    dt, N, rpg, gs, go = DT[dname], 768, 5, 23, 1
    _pin(dt, M, N, K, 2 if dname == "f32" else (15 if K < 2304 else 16))
    L = _lib.lib()
    rows = R.row_map(M, rpg, gs, go, device="cuda")
    a_rows = -(-M // rpg) * gs
    for dyadic in (True, False):
        ops = _Ops(dt, M, N, K, dyadic, seed=M + K + (1 if dyadic else 0), a_rows=a_rows)
        keep = torch.zeros(a_rows, dtype=torch.bool, device="cuda")
        keep[rows] = True
        ops.A[~keep] = ROWS_POISON
        assert int(keep.sum()) == M and not bool(keep[0]) and not bool(keep[go + rpg])
        P, Sp = R.product(ops.A[rows], ops.B)
        for of32 in ((1,) if dname == "f32" else (0, 1)):
            for bias in (ops.bias, None):
                h = _Hold()
                out_dt = torch.float32 if (of32 or dname == "f32") else dt
                C = _Framed(M, N, out_dt)
                _lib.check(L.ebc_gemm_rows(_lib.dtype_code(dt), of32, h(ops.A), h(ops.B), _lib.ptr(C.mid), _lib.ptr(bias), M, N,
                                           K, rpg, gs, go, _lib.stream()), "ebc_gemm_rows")
                ref, bound = R.epilogue(R.STORE, P, Sp, K, dt, out_dt, bias=bias)["C"]
                _held(f"rows.{dname}.{M}x{K}.{'dyadic' if dyadic else 'random'}.f32={of32}.bias={bias is not None}", C.mid,
                      ref, bound)
                assert C.ok()
                if dyadic:
                    _exact(C.mid, ref, out_dt)


# ------------------------------------------------------------------------------------------------ ebc_gemm_wgrad
CNT_BYTES = 16 * 1024
# (M, N, K) -> (tile, splits): 1 no split, 2 the last arriver adds the other piece, negative: f32 partials and a reduce
# launch.  Found with ebc_gemm_wgrad_tile_config; M is never a multiple of the tile's rows.
WGRAD16 = [((100, 64, 64), (2, 1)), ((100, 192, 1024), (2, 2)), ((100, 192, 4096), (2, -8)),
           ((700, 3072, 512), (1, 1)), ((700, 2048, 1024), (1, 2)), ((300, 384, 8192), (1, -16)),
           ((1500, 3072, 512), (3, 1)), ((1500, 3072, 1024), (3, 2)), ((300, 192, 32768), (3, -64)),
           ((1600, 5120, 512), (7, 1)), ((2100, 2048, 1024), (7, 2)), ((300, 1024, 25088), (7, -28))]
WGRAD32 = [((100, 64, 64), (2, 1)), ((100, 192, 1024), (2, 2)), ((100, 192, 4096), (2, -16))]     # f32: tile 2 only


def _run_wgrad(dname, shape, plan):
    dt, (M, N, K), L = DT[dname], shape, _lib.lib()
    out = (ctypes.c_int * 3)()
    tile = L.ebc_gemm_wgrad_tile_config(_lib.dtype_code(dt), M, N, K, out)
    assert (tile, out[2]) == plan and (out[0], out[1]) == TILES[tile][:2] and M % out[0] != 0, (tile, tuple(out))
    splits = abs(out[2])
    need = L.ebc_gemm_wgrad_workspace_bytes(_lib.dtype_code(dt), M, N, K)
    assert (need == 0) == (splits == 1)
    ws = torch.zeros(need + 4096, dtype=torch.uint8, device="cuda")          # exactly `need` bytes, then a sentinel
    ws[need:] = 0xA5
    for dyadic in (True, False):
        ops = _Ops(dt, M, N, K, dyadic, seed=M * 13 + K + (1 if dyadic else 0))
        P, Sp = R.product(ops.A, ops.B)
        ref, bound = R.epilogue(R.STORE, P, Sp, K, dt, torch.float32, splits=splits)["C"]
        outs = []
        for _ in range(2):
            h = _Hold()
            C = _Framed(M, N, torch.float32)
            _lib.check(L.ebc_gemm_wgrad(_lib.dtype_code(dt), h(ops.A), h(ops.B), _lib.ptr(C.mid), M, N, K,
                                        _lib.ptr(ws) if need else None, need, _lib.stream()), "ebc_gemm_wgrad")
            _held(f"wgrad.{dname}.t{tile}.s{out[2]}.{M}x{N}x{K}.{'dyadic' if dyadic else 'random'}", C.mid, ref, bound)
            assert C.ok()
            assert int(ws[:min(need, CNT_BYTES)].count_nonzero()) == 0         # the counter block is re-armed
            assert bool((ws[need:] == 0xA5).all())
            if dyadic:
                _exact(C.mid, ref, torch.float32)
            outs.append(C.mid.clone())
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dname", ["f16", "bf16"])
@pytest.mark.parametrize("shape,plan", WGRAD16, ids=lambda v: "x".join(map(str, v)))
def test_gemm_wgrad_16bit_every_plan_class(dname, shape, plan):
    _run_wgrad(dname, shape, plan)


@pytest.mark.parametrize("shape,plan", WGRAD32, ids=lambda v: "x".join(map(str, v)))
def test_gemm_wgrad_f32_every_plan_class(shape, plan):
    _run_wgrad("f32", shape, plan)


# ------------------------------------------------------------------------------------------------ ebc_transpose
@pytest.mark.parametrize("dname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("Rr", [1, 7, 9, 63, 65, 100])
def test_transpose_ragged_rows_and_columns(dname, Rr):
    """R % 8 != 0 takes the kernel's ragged tail, C % 64 != 0 its partial column tile; the padding columns r >= R and the
    guard rows keep the sentinel."""
    dt, L = DT[dname], _lib.lib()
    for Cc in (8, 72, 200):
        for ld in ((Rr + 7) // 8 * 8, (Rr + 7) // 8 * 8 + 8):
            g = torch.Generator(device="cuda").manual_seed(Rr * 1000 + Cc + ld)
            x = torch.randn(Rr, Cc, device="cuda", generator=g).to(dt)
            out = _Framed(Cc, ld, dt)
            _lib.check(L.ebc_transpose(_lib.dtype_code(dt), _lib.ptr(x), _lib.ptr(out.mid), Rr, Cc, ld, _lib.stream()),
                       "ebc_transpose")
            assert torch.equal(out.mid, R.transpose_padded(x, ld, SENT)), (Rr, Cc, ld)
            assert out.ok(), (Rr, Cc, ld)
