"""Records the host-side dispatch decisions of the GEMM / conv / workspace planners into gemm_dispatch.json.

Every entry point called here is host arithmetic (no device work), so this runs without a GPU.  The fixture pins the
decisions of the library it was recorded from: to check a refactor, record it from a build of the commit BEFORE the
change (EBC_LIB_PATH=<that build's libebc_hip.so> python tests/golden/make_gemm_dispatch.py) and let
tests/test_gemm_dispatch_cpu.py compare the current library against it.  Re-record only when a decision is meant to
change.  Each record carries its own arguments, so the test needs nothing but the file.
"""
import ctypes
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "clip-ebc_amd"))
from ebc_amd import _lib  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_dispatch.json")
DTYPES = (_lib.EBC_F32, _lib.EBC_F16, _lib.EBC_BF16)

GEMM_M = (37, 458, 777, 1000, 3136, 3664, 7328, 12544, 24000, 32060, 50176)
GEMM_N = (64, 128, 192, 512, 768, 1024, 2048, 2304, 3072)
GEMM_K = (64, 512, 768, 2304, 3072)
# tests/test_gpu_gemm.py test_gemm_wgrad's shapes, the 32-crop projection dW and a ResNet-50 one
WGRAD = ((512, 768, 12544), (512, 768, 1600), (128, 64, 64), (300, 192, 2048), (512, 768, 25088), (1024, 2048, 50176))
DEC_B, DEC_HW, DEC_C = (1, 2, 16, 30, 32), (14, 28, 56), (64, 256, 768, 2048)
VIT = dict(B=(1, 16, 32), size=(224, 448), patch=(16, 32), layers=(2, 12), num_vpt=(0, 32), training=(0, 1))


def gemm_tile_config(L, dt, M, N, K):
    out = (ctypes.c_int * 3)()
    return [L.ebc_gemm_tile_config(dt, M, N, K, out), *out]


def conv_tile_config(L, dt, mode, M, N, K):
    out = (ctypes.c_int * 3)()
    return [L.ebc_conv_tile_config(dt, mode, M, N, K, out), *out]


def decoder(L, dt, B, HW, C):
    """[geometry rc, geometry[6], mode-1 tile config[4], mode-2 tile config[4], decoder workspace bytes] at C = N."""
    geo = (ctypes.c_long * 6)()
    rc = L.ebc_dec_geometry(dt, B, HW, HW, C, geo)
    kq = geo[3]
    return [rc, list(geo), conv_tile_config(L, dt, 1, B * HW * HW, C, 9 * C), conv_tile_config(L, dt, 2, C, 9 * C, kq),
            L.ebc_dec_workspace_bytes(dt, B, HW, HW, C, C)]


def record(L):
    """{entry: [[args, result], ...]} over the grids above."""
    rec = {"gemm_tile_config": [], "gemm_wgrad_workspace_bytes": [], "decoder": [], "vit_workspace_bytes_p": []}
    for dt in DTYPES:
        for M, N, K in itertools.product(GEMM_M, GEMM_N, GEMM_K):
            rec["gemm_tile_config"].append([[dt, M, N, K], gemm_tile_config(L, dt, M, N, K)])
        for M, N, K in WGRAD:
            rec["gemm_wgrad_workspace_bytes"].append([[dt, M, N, K], L.ebc_gemm_wgrad_workspace_bytes(dt, M, N, K)])
        for B, HW, C in itertools.product(DEC_B, DEC_HW, DEC_C):
            rec["decoder"].append([[dt, B, HW, C], decoder(L, dt, B, HW, C)])
        for B, size, patch, layers, nv, tr in itertools.product(*VIT.values()):
            rec["vit_workspace_bytes_p"].append(
                [[B, size, size, patch, layers, nv, dt, tr], L.ebc_vit_workspace_bytes_p(B, size, size, patch, layers, nv, dt, tr)])
    return rec


def main():
    rec = record(_lib.load())
    with open(OUT, "w") as f:          # one record a line: small and diffable
        f.write("{\n")
        f.write(",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r, separators=(",", ":")) for r in v))
                           for k, v in rec.items()))
        f.write("\n}\n")
    print(OUT, os.path.getsize(OUT), "bytes", {k: len(v) for k, v in rec.items()})


if __name__ == "__main__":
    main()
