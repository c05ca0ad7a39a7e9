"""End-to-end images/s of a val split that starts from raw uint8 images, two ways, in one process, alternating:

  (a) host  : per image, on the CPU threads torch is bound to, the reference's preparation (`/255.`, right/bottom zero
              padding to the window grid, Normalize; datasets/crowd.py:141-162, datasets/transforms.py:123-135), then
              the H2D copy of the f32 tensor, then `sliding_window_predict` and the count (the D2H map + CPU sum);
  (b) device: `evaluate_raw` (one packed u8 H2D a call, tiles normalised from the bytes on the device, tile batches
              across images, one batched assembly, one D2H of the counts).

Workloads: 64 synthetic u8 [768,1024,3] images and 8 of [2048,3072,3]; window = stride = 224, fit = "zero_pad"; the full
clip_vit_b_16 under fp16 autocast.  Each pass ends in a device synchronise (both paths read their counts back); the
figure of a path is the median over the timed passes, the spread is printed beside it, and the counts of the two
paths are compared.  One JSON line per workload.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "clip-ebc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ebc_amd.eval_utils import evaluate_raw, fit_size, sliding_window_counts, sliding_window_predict  # noqa: E402
from ebc_amd.model import get_model  # noqa: E402
from ebc_amd.transforms import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402

BINS = [(0.0, 0.0), (1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (4.0, float("inf"))]
ANCHORS_NWPU = [0.0, 1.0, 2.0, 3.0, 4.21931]
WIN = 224


def host_path(model, images, dev):
    mean = torch.tensor(IMAGENET_MEAN)[:, None, None]
    std = torch.tensor(IMAGENET_STD)[:, None, None]
    counts = []
    for u8 in images:
        x = u8.permute(2, 0, 1).float() / 255.
        Hf, Wf = fit_size(x.shape[1], x.shape[2], WIN, WIN, "zero_pad")
        x = torch.nn.functional.pad(x, (0, Wf - x.shape[2], 0, Hf - x.shape[1]), value=0.)
        x = x.sub_(mean).div_(std)
        counts.append(float(sliding_window_predict(model, x[None].to(dev), WIN, WIN).sum()))
    return np.asarray(counts)


def device_path(model, images, per_call):
    out = []
    for k in range(0, len(images), per_call):
        out.append(sliding_window_counts(model, images[k:k + per_call], WIN, WIN, fit="zero_pad").numpy())
    return np.concatenate(out).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images-per-call", type=int, default=32)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--sets", default="64x768x1024,8x2048x3072")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_raw.py needs a HIP device")
    dev = torch.device("cuda:0")
    model = get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, prompt_type="word", num_vpt=32, vpt_drop=0.0,
                      deep_vpt=True, weights_seed=0, vit_layers=args.layers).to(dev).eval()
    for spec in args.sets.split(","):
        n, H, W = (int(v) for v in spec.split("x"))
        g = np.random.Generator(np.random.PCG64(n))
        images = [torch.from_numpy(g.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(n)]
        Hf, Wf = fit_size(H, W, WIN, WIN, "zero_pad")
        tiles = n * (Hf // WIN) * (Wf // WIN)
        times = {"host": [], "device": []}
        counts = {}
        with torch.autocast("cuda", dtype=torch.float16):
            for rep in range(args.warmup + args.reps):
                for name, fn in (("host", lambda: host_path(model, images, dev)),
                                 ("device", lambda: device_path(model, images, args.images_per_call))):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    counts[name] = fn()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        times[name].append(time.perf_counter() - t0)
            # evaluate_raw is device_path plus the error metrics: one pass, to show the public entry point runs
            errs = evaluate_raw(model, ((im, np.zeros((0, 2))) for im in images), WIN, WIN, fit="zero_pad",
                                images_per_call=args.images_per_call)
        med = {k: statistics.median(v) for k, v in times.items()}
        rel = float(np.max(np.abs(counts["device"] - counts["host"]) / np.maximum(np.abs(counts["host"]), 1e-30)))
        print(json.dumps({
            "metric": f"val-split images/s from raw u8, {n} images of {H}x{W} (fitted {Hf}x{Wf}, {tiles} tiles), "
                      f"clip_vit_b_16 {args.layers} layers fp16 autocast",
            "host_images_per_s": round(n / med["host"], 2), "device_images_per_s": round(n / med["device"], 2),
            "ratio": round(med["host"] / med["device"], 3),
            "host_s": [round(t, 4) for t in times["host"]], "device_s": [round(t, 4) for t in times["device"]],
            "device_tiles_per_s": round(tiles / med["device"], 1), "cpu_threads": torch.get_num_threads(),
            "images_per_call": args.images_per_call, "reps": args.reps, "warmup": args.warmup,
            "counts_max_rel_diff": rel, "evaluate_raw_mae": float(errs["mae"])}), flush=True)


if __name__ == "__main__":
    main()
