"""Rank body of the world-2 DDP test with the HIP text tower (tests/test_gpu_text_tower_train.py): tests/_ddp_text_worker.py's
rank_main with its model built with text_tower="hip", replaced inside the child process."""
from __future__ import annotations

import _ddp_text_worker as TW
import _ddp_worker as W

TEXT_LAYERS = TW.TEXT_LAYERS


def build(device):
    from ebc_amd.model import get_model
    return get_model("clip_vit_b_16", 224, 8, W.BINS, W.ANCHORS, prompt_type="word", vit_layers=W.LAYERS,
                     text_layers=TEXT_LAYERS, freeze_text_encoder=False, weights_seed=0,
                     text_tower="hip").to(device).train()


def rank_main(rank: int, world: int, port: int, out_dir: str) -> None:
    TW.build = build                     # this process only: a fresh child of the forkserver
    TW.rank_main(rank, world, port, out_dir)
