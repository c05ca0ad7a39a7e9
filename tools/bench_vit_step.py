"""Train-step throughput of a CLIP ViT backbone on one MI355X, for backbones bench.py does not time (clip_vit_b_32):

    python tools/bench_vit_step.py [--model clip_vit_b_32] [--crops 16] [--steps 60] [--warmup 15] [--dtype fp16]

The step is bench.py's (model forward under autocast, DACE/DMCount loss, backward, the HIP Adam + GradScaler step) on
bench.py's synthetic crops; each timed step sits between two device events and the median over the timed steps is
reported (crops/s = crops / median), with the spread, as one JSON line.  No GPU: an error, not a CPU time."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "clip-ebc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BINS = [(0.0, 0.0), (1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (4.0, float("inf"))]
ANCHORS_NWPU = [0.0, 1.0, 2.0, 3.0, 4.21931]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="clip_vit_b_32", choices=["clip_vit_b_32", "clip_vit_b_16"])
    ap.add_argument("--crops", type=int, default=16)
    ap.add_argument("--reduction", type=int, default=8)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vit_step.py needs a HIP device")
    from ebc_amd import optim as eo
    from ebc_amd import synthetic as syn
    from ebc_amd.losses import DACELoss
    from ebc_amd.model import get_model
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    model = get_model(args.model, 224, args.reduction, BINS, ANCHORS_NWPU, prompt_type="word", num_vpt=32,
                      vpt_drop=0.0, deep_vpt=True, weights_seed=0).to(dev).train()
    loss_fn = DACELoss(BINS, args.reduction, weight_count_loss=1.0, count_loss="dmcount", input_size=224).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    amp = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": None}[args.dtype]
    opt = eo.Adam(params, lr=1e-4, weight_decay=1e-4)
    scaler = eo.GradScaler(enabled=args.dtype == "fp16")
    pool = []
    for s in range(min(8, args.warmup + args.steps)):
        img, pts, dens = syn.synthetic_crops(args.crops, 224, seed=1000 + s)
        pool.append((torch.from_numpy(img).to(dev), [torch.from_numpy(p).to(dev) for p in pts],
                     torch.from_numpy(dens).to(dev)))

    def step(i):
        img, pts, dens = pool[i % len(pool)]
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            logits, exp = model(img)
            loss, _ = loss_fn(logits, exp, dens, pts)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return loss

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        loss = step(args.warmup + i)
        b.record()
    torch.cuda.synchronize()
    ms = np.asarray([a.elapsed_time(b) for a, b in ev])
    assert bool(torch.isfinite(loss)), "the last step's loss is not finite"
    med = float(np.median(ms))
    wall = ev[0][0].elapsed_time(ev[-1][1]) / args.steps          # first start to last end: includes the gaps between steps
    print(json.dumps({"metric": f"train crops/s {args.model} 224px reduction {args.reduction}, {args.crops} crops, "
                                f"{args.dtype} autocast, full step (fwd + DACE/DMCount + bwd + Adam)",
                      "value": round(args.crops / med * 1e3, 1), "unit": "crops/s", "step_ms_median": round(med, 3),
                      "step_ms_window_mean": round(wall, 3),
                      "step_ms_p10": round(float(np.percentile(ms, 10)), 3),
                      "step_ms_p90": round(float(np.percentile(ms, 90)), 3), "steps": args.steps,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
