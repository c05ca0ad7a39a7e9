"""Helpers shared by the per-kernel GPU modules (test_gpu_bn_kernels.py, test_gpu_encoder_kernels.py,
test_gpu_gemm_kernels.py, test_gpu_conv_kernels.py, test_gpu_vit_stages.py): sentinel-guarded
output buffers, operand lifetime, and the per-element checks that print "RATIO <name> <largest error / bound>" before
they assert."""
import torch

import _bn_refs as R
from ebc_amd import _lib

F64 = torch.float64
U = R.U32
SENT = 7.0
GUARD_ROWS = 64


def _f32(t):
    return t.to(torch.float32).cuda().contiguous()


class _Hold(list):
    """Device copies of a call's operands, kept alive until the test has read the results."""

    def __call__(self, t, f32=False):
        d = _f32(t) if f32 else t.cuda()
        self.append(d)
        return _lib.ptr(d)


def _guarded(rows, cols, dt, fill=SENT):
    """[rows + GUARD_ROWS][cols] device tensor full of the sentinel; the kernel may only write the first `rows`."""
    return torch.full((rows + GUARD_ROWS, cols), fill, dtype=dt, device="cuda")


def _guard_ok(t, rows, fill=SENT):
    return bool((t[rows:] == fill).all())


class _Framed:
    """[GUARD_ROWS + rows + GUARD_ROWS][cols] device tensor full of the sentinel; `mid` (what the kernel is given) is
    the `rows` in the middle, so a write before the first row or past the last lands on a guard."""

    def __init__(self, rows, cols, dt, fill=SENT):
        self.rows, self.fill = rows, fill
        self.full = torch.full((rows + 2 * GUARD_ROWS, cols), fill, dtype=dt, device="cuda")
        self.mid = self.full[GUARD_ROWS:GUARD_ROWS + rows]

    def ok(self):
        lo, hi = self.full[:GUARD_ROWS], self.full[GUARD_ROWS + self.rows:]
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


def _report(name, err, bound):
    ratio = float((err / bound).max())
    print(f"RATIO {name} {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio, int((err / bound).argmax()))     # NaN fails too


def _elem(name, out, ref, A, k, dt, extra=None):
    """|out - ref| <= ulp_T(ref)/2 + k * 2^-24 * A per element."""
    out = out.detach().to(F64).cpu().reshape(ref.shape)
    bound = 0.5 * R.ulp(ref, dt) + k * U * A
    if extra is not None:
        bound = bound + extra
    _report(name, (out - ref).abs(), bound)


def _exact(out, ref, dt):
    """Dyadic inputs: the reference is exact in f32, the stored value is it rounded once to T."""
    assert torch.equal(ref.to(torch.float32).to(F64), ref), "the reference is not exact in f32: not a dyadic case"
    want = ref.to(torch.float32).to(dt)
    got = out.detach().to(want.device).reshape(want.shape)       # (a reference kept on the device is compared there)
    assert torch.equal(got, want), int((got != want).sum())
