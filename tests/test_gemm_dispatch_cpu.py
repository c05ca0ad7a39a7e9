"""CPU pin of the host-side dispatch decisions: tile configurations, split / stream-K factors, decoder geometry and
workspace sizes over the grid of tests/golden/make_gemm_dispatch.py must equal the recorded fixture (recorded from
the commit before the dispatch refactor).  Host arithmetic only: no device work, no `gpu` marker."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_gemm_dispatch as mk  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from ebc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "clip-ebc_amd")])
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "gemm_dispatch.json")) as f:
        return json.load(f)


def _mismatches(records, fn):
    return [(args, want, got) for args, want in records for got in [fn(*args)] if got != want][:10]


def test_fixture_covers_the_grid(recorded):
    assert {k: len(v) for k, v in recorded.items()} == {
        "gemm_tile_config": 3 * len(mk.GEMM_M) * len(mk.GEMM_N) * len(mk.GEMM_K),
        "gemm_wgrad_workspace_bytes": 3 * len(mk.WGRAD),
        "decoder": 3 * len(mk.DEC_B) * len(mk.DEC_HW) * len(mk.DEC_C),
        "vit_workspace_bytes_p": 3 * 3 * 2 ** 5}


def test_gemm_tile_config(lib, recorded):
    assert not _mismatches(recorded["gemm_tile_config"], lambda *a: mk.gemm_tile_config(lib, *a))


def test_gemm_wgrad_workspace_bytes(lib, recorded):
    assert not _mismatches(recorded["gemm_wgrad_workspace_bytes"], lib.ebc_gemm_wgrad_workspace_bytes)


def test_decoder_geometry_conv_tiles_and_workspace(lib, recorded):
    assert not _mismatches(recorded["decoder"], lambda *a: mk.decoder(lib, *a))


def test_vit_workspace_bytes(lib, recorded):
    assert not _mismatches(recorded["vit_workspace_bytes_p"], lib.ebc_vit_workspace_bytes_p)
