"""Train-step throughput of a CLIP ViT backbone on one MI355X, for backbones bench.py does not time (clip_vit_b_32):

    python tools/bench_vit_step.py [--model clip_vit_b_32] [--crops 16] [--steps 60] [--warmup 15] [--dtype fp16]
                                   [--train-text [--text-tower {torch,hip}]]

The step is bench.py's (model forward under autocast, DACE/DMCount loss, backward, the HIP Adam + GradScaler step) on
bench.py's synthetic crops; each timed step sits between two device events and the median over the timed steps is
reported (crops/s = crops / median), with the spread, as one JSON line.  No GPU: an error, not a CPU time.

--train-text builds the model with freeze_text_encoder=False (the text tower runs in every forward and takes gradients
through ebc_head_bwd_text) and adds to the line: the launch's in-step time from one probed step (ebc_probe_begin / _end),
its isolated time at the step's shape, its partial-buffer bytes, and the text tower's own forward + backward under the
same autocast (events around it, median).  --text-tower hip runs that tower in the library (text_tower="hip":
ebc_text_forward / ebc_text_backward) instead of PyTorch-ROCm; the line then also carries the tower's host enqueue time
(the same forward + backward timed on the host clock without a device wait, median) beside its device time."""
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


def _median_ms(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def _text_cost(model, step, args, amp, dev):
    """What --train-text adds to a step, split into the new launch and the PyTorch text tower."""
    import ctypes
    from ebc_amd import _lib
    L = _lib.lib()
    cap = 4096
    _lib.check(L.ebc_probe_begin(cap), "ebc_probe_begin")
    step(0)
    recs = (_lib.EbcProbeRecord * cap)()
    n = L.ebc_probe_end(ctypes.cast(recs, ctypes.c_void_p), cap)
    in_step = [r.ms for r in recs[:min(n, cap)] if _lib.PROBE_KINDS.get(r.kind) == "head_bwd_text"]
    g = (224 // args.reduction) ** 2
    P, NB, E = args.crops * g, len(BINS), model.clip_embed_dim
    gen = torch.Generator(device=dev).manual_seed(1)
    Z = torch.randn(P, E, device=dev, generator=gen)
    text = torch.randn(NB, E, device=dev, generator=gen)
    dl = torch.randn(args.crops, NB, g, device=dev, generator=gen)
    de = torch.randn(args.crops, g, device=dev, generator=gen)
    ls, anchors = torch.full((1,), 2.659, device=dev), torch.tensor(ANCHORS_NWPU, device=dev)
    need = L.ebc_head_bwd_text_workspace_bytes(P, NB, E)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    dtext = torch.empty(NB, E, device=dev)
    p, st = _lib.ptr, _lib.stream(dev)
    iso = _median_ms(lambda: _lib.check(L.ebc_head_bwd_text(_lib.EBC_F32, p(Z), p(text), p(ls), p(anchors), p(dl), p(de),
                                                            None, p(dtext), P, g, NB, E, p(ws), need, st), "head_bwd_text"))
    ids = model._prompt_ids(dev)
    gt = torch.randn(NB, E, device=dev, generator=gen)

    def tower():
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            tf = model.text_encoder(ids).float()
        tf.backward(gt)
    tower_ms = _median_ms(tower)
    import time
    host = []
    for _ in range(20):                      # enqueue cost alone: the device runs behind, the queue is drained between calls
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tower()
        host.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)
    return {"text_tower": args.text_tower, "text_tower_host_enqueue_ms": round(float(np.median(host)), 3),
            "head_bwd_text_ms_in_step": [round(v, 4) for v in in_step], "head_bwd_text_ms_isolated": round(iso, 4),
            "head_bwd_text_partial_bytes": int(need), "text_tower_fwd_bwd_ms": round(tower_ms, 3),
            "trainable_params": int(sum(q.numel() for q in model.parameters() if q.requires_grad))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="clip_vit_b_32", choices=["clip_vit_b_32", "clip_vit_b_16"])
    ap.add_argument("--crops", type=int, default=16)
    ap.add_argument("--reduction", type=int, default=8)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--train-text", action="store_true", help="freeze_text_encoder=False")
    ap.add_argument("--text-tower", default="torch", choices=["torch", "hip"],
                    help="with --train-text: the text tower on PyTorch-ROCm or in the library (text_tower=)")
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
                      vpt_drop=0.0, deep_vpt=True, weights_seed=0,
                      freeze_text_encoder=not args.train_text, text_tower=args.text_tower).to(dev).train()
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
    extra = _text_cost(model, step, args, amp, dev) if args.train_text else {}
    print(json.dumps({"metric": f"train crops/s {args.model} 224px reduction {args.reduction}, {args.crops} crops, "
                                f"{args.dtype} autocast, full step (fwd + DACE/DMCount + bwd + Adam)"
                                + (f", trainable text tower ({args.text_tower})" if args.train_text else ""),
                      "value": round(args.crops / med * 1e3, 1), "unit": "crops/s", "step_ms_median": round(med, 3),
                      "step_ms_window_mean": round(wall, 3),
                      "step_ms_p10": round(float(np.percentile(ms, 10)), 3),
                      "step_ms_p90": round(float(np.percentile(ms, 90)), 3), "steps": args.steps,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(0), **extra}))


if __name__ == "__main__":
    main()
