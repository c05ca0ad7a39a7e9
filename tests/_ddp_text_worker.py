"""Rank body of the world-2 DDP test with a trainable text tower (tests/test_gpu_text_train.py).

As tests/_ddp_worker.py (whose batch, split and bins it uses): a fresh process forked from the session's forkserver,
both ranks on cuda:0 over gloo, SyncBatchNorm + DistributedDataParallel through ebc_amd.distributed.wrap_ddp.  The model
is built with freeze_text_encoder=False, so DDP's buckets carry the text tower's gradients too."""
from __future__ import annotations

import os

import _ddp_worker as W

TEXT_LAYERS = 2


def build(device):
    from ebc_amd.model import get_model
    return get_model("clip_vit_b_16", 224, 8, W.BINS, W.ANCHORS, prompt_type="word", vit_layers=W.LAYERS,
                     text_layers=TEXT_LAYERS, freeze_text_encoder=False, weights_seed=0).to(device).train()


def rank_main(rank: int, world: int, port: int, out_dir: str) -> None:
    import torch
    import torch.distributed as dist
    from ebc_amd.distributed import wrap_ddp
    from ebc_amd.losses import DACELoss
    from ebc_amd.model import DecoderMaskTap
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    model = wrap_ddp(build(dev), 0)
    img, pts, dens = W.batch()
    b0 = sum(W.SPLIT[:rank])
    sl = slice(b0, b0 + W.SPLIT[rank])
    DecoderMaskTap.capture = []                # this rank's decoder ReLU decisions (the parent replays them)
    logits, exp = model(torch.from_numpy(img[sl]).to(dev))
    (m1, m2, _, _), = DecoderMaskTap.capture
    DecoderMaskTap.capture = None
    loss, _ = DACELoss(W.BINS, 8, count_loss="dmcount", input_size=224)(
        logits, exp, torch.from_numpy(dens[sl]).to(dev), [torch.from_numpy(p).to(dev) for p in pts[sl]])
    loss.backward()
    torch.cuda.synchronize()
    m = model.module
    res = {}
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        g = p.grad.detach()
        if k == "text_encoder.token_embedding.weight":         # 49408 x 512: its norm and the rows with a gradient
            rows = g.abs().amax(1).nonzero().flatten()
            res["tok_rows"], res["tok_grad"], res["tok_norm"] = rows.cpu(), g[rows].cpu(), g.norm().cpu()
        else:
            res[k] = g.cpu()
    res["mask1"], res["mask2"] = m1.cpu(), m2.cpu()
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
