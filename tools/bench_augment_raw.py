"""Crops/s and ms per batch of the training input path when the images start on the CPU as uint8, on the
`bench.py --augment` workload (16 images of 1536x2048, 2 crops each -> 224x224, trainer defaults; the images are uint8
[3,H,W], the reference's .npy layout), in one process:

  (a) float   : the only route before raw sources: per batch, `float() / 255` of every whole image on the CPU, the
                upload of the f32 tensors (12 bytes a pixel), `CropAugment.__call__`;
  (b) windows : `RawCropLoader(resident=False, prefetch=False)`: the crop windows packed and uploaded as bytes;
  (c) prefetch: as (b) with prefetch=True (batch k+1 packed and copied on a side stream before batch k is handed out);
  (d) resident: `RawCropLoader(resident=True)`: the split in HBM as bytes, windows read in place.

Every mode is timed twice: alone, and with a stand-in for the training step (a chain of matmuls of about
`--step-ms`, launched on the main stream for every batch), where what a mode adds to the bare step is its exposed
cost.  A pass is `--batches` batches and ends in a device synchronise; the figure is the median over `--reps` passes
after `--warmup`, the spread (min..max) is printed beside it.  Last line: the device-only time of `apply` for resident
uint8 against resident float32 sources on the same plans (events around 10 calls, as bench.py --augment --full).
One JSON line per mode.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "clip-ebc_amd"))
import torch  # noqa: E402

from ebc_amd.loader import RawCropLoader  # noqa: E402
from ebc_amd.transforms import CropAugment  # noqa: E402

H, W, NI, NC = 1536, 2048, 16, 2


def make_step(ms, dev):
    """A chain of 4096^3 fp16 matmuls on the current stream that lasts about `ms`."""
    a = torch.randn(4096, 4096, device=dev, dtype=torch.float16)
    b = torch.randn(4096, 4096, device=dev, dtype=torch.float16) * 0.01
    for _ in range(3):
        a @ b
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        a @ b
    e1.record()
    torch.cuda.synchronize()
    n = max(1, round(ms / (e0.elapsed_time(e1) / 20)))

    def step():
        for _ in range(n):
            a @ b
    return step, n


def timed(make_iter, batches, step, reps, warmup):
    out = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in make_iter():
            if step is not None:
                step()
        torch.cuda.synchronize()
        if rep >= warmup:
            out.append((time.perf_counter() - t0) / batches * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, default=12,
                    help="batches a pass: a pass starts on an idle device, so its first batch's host work is exposed")
    ap.add_argument("--step-ms", type=float, default=8.4, help="32 crops at the training step's ~3800 crops/s")
    ap.add_argument("--modes", default="float,windows,prefetch,resident")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_raw.py needs a HIP device")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    images = [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for _ in range(NI)]   # the .npy layout
    labels = [torch.rand(200, 2, generator=g) * torch.tensor([W, H], dtype=torch.float32) for _ in range(NI)]
    aug = CropAugment()                                        # trainer.py:40-52 defaults
    step, n_mm = make_step(args.step_ms, dev)
    bare = timed(lambda: range(args.batches), args.batches, step, args.reps, args.warmup)
    split_i, split_l = images * args.batches, labels * args.batches      # `batches` batches an epoch, the same 16 images

    def float_route():
        for _ in range(args.batches):
            up = [im.float().div_(255.).to(dev) for im in images]
            yield aug(up, labels, NC)

    def loader(**kw):
        ld = RawCropLoader(split_i, split_l, aug, NI, NC, shuffle=False, device=dev, **kw)
        return lambda: iter(ld)

    # upload bytes a batch: (a) 12 H W an image; (b, c) the packed windows (drawn plans, 16-byte aligned); (d) none
    torch.manual_seed(1)
    win = []
    for _ in range(20):
        plans = [aug.plan_crop(i, H, W, labels[i].clone())[0] for i in range(NI) for _ in range(NC)]
        win.append(sum((3 * p.crop_h * p.crop_w + 15) & ~15 for p in plans))
    modes = {"float": (float_route, 12 * H * W * NI), "windows": (loader(resident=False, prefetch=False), int(statistics.mean(win))),
             "prefetch": (loader(resident=False, prefetch=True), int(statistics.mean(win))),
             "resident": (loader(resident=True), 0)}
    crops = NI * NC
    for name in args.modes.split(","):
        fn, nbytes = modes[name]
        torch.manual_seed(0)
        alone = timed(fn, args.batches, None, args.reps, args.warmup)
        with_step = timed(fn, args.batches, step, args.reps, args.warmup)
        med, med_s, med_b = statistics.median(alone), statistics.median(with_step), statistics.median(bare)
        print(json.dumps({
            "metric": f"train input path from CPU uint8, {NI} images of {H}x{W} x {NC} crops -> 224, trainer defaults",
            "mode": name, "crops_per_s": round(crops / med * 1e3, 1), "ms_per_batch": round(med, 3),
            "ms_per_batch_spread": [round(min(alone), 3), round(max(alone), 3)],
            "ms_per_batch_with_step": round(med_s, 3),
            "ms_per_batch_with_step_spread": [round(min(with_step), 3), round(max(with_step), 3)],
            "bare_step_ms": round(med_b, 3), "exposed_ms_beside_step": round(med_s - med_b, 3),
            "upload_bytes_per_batch": nbytes, "step_matmuls": n_mm, "batches_per_pass": args.batches,
            "reps": args.reps, "warmup": args.warmup, "cpu_threads": torch.get_num_threads()}), flush=True)

    # device-only: apply on resident uint8 against resident float32, the same plans
    torch.manual_seed(2)
    plans = [aug.plan_crop(i, H, W, labels[i].clone())[0] for i in range(NI) for _ in range(NC)]
    srcs = {"u8_hwc": [im.permute(1, 2, 0).contiguous().to(dev) for im in images], "u8_chw": [im.to(dev) for im in images],
            "f32": [im.float().div_(255.).to(dev) for im in images]}
    dev_ms = {k: [] for k in srcs}
    for rep in range(args.warmup + args.reps):
        for k, s in srcs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                aug.apply(s, plans)
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                dev_ms[k].append(e0.elapsed_time(e1) / 10)
    print(json.dumps({"metric": "device-only ms per apply of 32 crops, resident sources, same plans",
                      **{f"{k}_ms": round(statistics.median(v), 4) for k, v in dev_ms.items()},
                      **{f"{k}_spread": [round(min(v), 4), round(max(v), 4)] for k, v in dev_ms.items()},
                      "reps": args.reps, "warmup": args.warmup}), flush=True)


if __name__ == "__main__":
    main()
