"""The tile-first binner at its own list-length edges (scenes: tests/tile_lists.py, DESIGN.md "List-length edges").

Every branch of k_tile_sort, k_tf_scatter, the second tile-id pass and the projector's histogram is decided by an exact list
length, pair count or splat count.  The scenes put those counts on the edges; every frame here is held to the oracle's
counts, offsets and index lists exactly AND to zero order faults, zero misranked frames and no overflow (check_frames): a
misranked list heals itself — the frame is rendered again with ballot ranking — and only those counters tell.
Each scene's purpose is asserted from the oracle before the GPU is asked anything.
"""
import os
import subprocess
import sys

import pytest

import splat_renderer_amd as sr
from tests import tile_lists as TL
from tests.tile_first_child import check_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCREENS = {"one_class": TL.ONE_CLASS_SCREEN, "two_classes": TL.TWO_CLASS_SCREEN}


def _scene(name, screen):
    w, h = SCREENS[screen]
    tiles = -(-w // 16) * -(-h // 16)
    assert tiles <= 4200 if screen == "one_class" else 4200 < tiles < 6144  # <_, 24, true> alone | short class 8 + long class
    sc = TL.build(name, w, h)
    TL.check_scene(sc)
    return sc


@pytest.mark.parametrize("screen", ["one_class", "two_classes"])
@pytest.mark.parametrize("name", ["by_length", "by_passes"])
def test_edge_lists_default_ranking(device, name, screen):
    """by_length on the two-class screen also compares the float image with the sortFirst frame's, bit for bit."""
    sc = _scene(name, screen)
    check_frames(sr, device, sc, "default ranking", image=(name == "by_length" and screen == "two_classes"))


@pytest.mark.parametrize("screen", ["one_class", "two_classes"])
@pytest.mark.parametrize("name", ["by_length", "by_passes"])
def test_edge_lists_ballot_ranking(monkeypatch, name, screen):
    sc = _scene(name, screen)
    monkeypatch.setenv("SPLAT_RANK", "ballot")
    dev = sr.Device(0)  # (the ranking is resolved once per context)
    try:
        assert dev.rankStatus()["policy"] == "ballot"
        check_frames(sr, dev, sc, "ballot ranking")
    finally:
        dev.destroy()


@pytest.mark.parametrize("rank", ["checked", "ballot"])
@pytest.mark.parametrize("short", [8, 12, 16])
def test_each_short_class(short, rank):
    """k_tile_sort<_, 8 | 12 | 16, false> followed by <_, 24, true> beyond its cap, on both scenes: n == cap and cap + 1 of
    every class are in by_length.  The class is read once per process: a child per value, on the shipped library."""
    w, h = SCREENS["two_classes"]
    env = dict(os.environ, SPLAT_TILE_SORT_SHORT=str(short))
    env.pop("SPLAT_LIB_PATH", None)
    env.pop("SPLAT_RANK", None)
    if rank == "ballot":
        env["SPLAT_RANK"] = "ballot"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tile_first_child.py"), str(w), str(h), "by_length", "by_passes"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    line = f"tile_first_child ok: short={short} rank={rank} cases=by_length@{w}x{h},by_passes@{w}x{h}"
    assert p.returncode == 0 and line in p.stdout.splitlines(), p.stdout[-2000:] + p.stderr[-3000:]


@pytest.mark.parametrize("r", [1, 2, 3])
def test_large_blocks_with_a_ragged_tail(device, r):
    """2^20 + r splats: 1024-splat blocks, four splats per thread from one 16-byte load, in k_tf_scatter and in the
    projector's histogram — and a last thread that must load r splats one by one (`i0 + 3 < n`)."""
    sc = TL.ragged_tail(r)
    TL.check_ragged_tail(sc, r)
    n = sc["props"].shape[0]
    assert n > 2 ** 20 and n % 4 == r  # (a change of TF_SMALL_FRAME_SPLATS must not silently move the case off the path)
    check_frames(sr, device, sc, f"2^20 + {r} splats")


@pytest.mark.parametrize("kind", ["block", "giant"])
def test_blocks_that_expand_in_several_rounds(device, kind):
    """k_tf_scatter stages TF_STAGE = 4096 pairs per round: 256-splat blocks of ~10 000 pairs with rectangles across the
    round boundaries, and one splat whose own rectangle (65 x 64 tiles) is more than a round."""
    sc = TL.multi_round(kind)
    TL.check_multi_round(sc, kind)
    check_frames(sr, device, sc, "rounds of the scatter", image=True)
