#!/usr/bin/env python3
"""Frames of the tests/tile_lists.py scenes on the SHIPPED library, in a process of their own: SPLAT_TILE_SORT_SHORT (the
per-tile sort's short class: 8, 12 or 16 pairs per thread) is read once per process, so tests/test_gpu_tile_first_edges.py
starts one child per value and ranking policy.  check_frames() is what that file's in-process tests call too.

    SPLAT_TILE_SORT_SHORT=12 [SPLAT_RANK=ballot] python tests/tile_first_child.py 1136 960 by_length by_passes
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.helpers import assert_same  # noqa: E402


def check_frames(sr, dev, sc, what, image=False):
    """Renders the scene tile-first, twice (the first frame is host-synchronised, the second sync-free), and holds each frame
    to the oracle: pair total, counts, offsets, index lists — and NO recovery: a misranked list is rendered again with ballot
    ranking and an overflowed frame again with room, after which the lists match; only the three counters tell.
    image: the float image is, bit for bit, the sortFirst frame's."""
    props, normals, u, w, h, ref = sc["props"], sc["normals"], sc["u"], sc["w"], sc["h"], sc["ref"]
    n, want_total = props.shape[0], int(ref["indices"].shape[0])
    made = [dev.createBufferFrom(props), dev.createBufferFrom(normals)]
    try:
        pbuf, nbuf = made
        r = sr.Renderer(dev, None, "rgba8unorm", n, frameOrder="tileFirst")
        made.append(r)
        for rep in ("first frame", "sync-free frame"):
            tag = (what, sc["name"], w, h, rep)
            r.render(u, pbuf, nbuf, None, w, h, wantFloat=image)
            total = r.finish()
            b = r.binner
            assert_same(b.getTileCountsBuffer().read(np.uint32), ref["counts"], tag + ("counts",))
            assert_same(b.getTileOffsetsBuffer().read(np.uint32), ref["offsets"], tag + ("offsets",))
            assert_same(b.getTileIndicesBuffer().read(np.uint32, want_total), ref["indices"], tag + ("lists",), offsets=ref["offsets"],
                        keys=ref["keys"])
            assert total == want_total, tag + (total, want_total)
            assert not r.previousFrameOverflowed, tag
            assert r.framesMisranked == 0, tag
            assert dev.rankStatus()["orderFaults"] == 0, tag + (dev.rankStatus(),)
        if image:
            got = r.readPixelsFloat().copy()
            r2 = sr.Renderer(dev, None, "rgba8unorm", n, frameOrder="sortFirst")
            made.append(r2)
            r2.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
            assert_same(got.view(np.uint32), r2.readPixelsFloat().view(np.uint32), (what, sc["name"], w, h, "image"))
    finally:
        for o in reversed(made):
            o.destroy()


def main(argv):
    import splat_renderer_amd as sr
    from splat_renderer_amd import _lib
    from tests import tile_lists as TL
    w, h, names = int(argv[1]), int(argv[2]), argv[3:]
    short, rank = os.environ.get("SPLAT_TILE_SORT_SHORT", ""), os.environ.get("SPLAT_RANK", "")
    assert short in ("8", "12", "16"), f"SPLAT_TILE_SORT_SHORT={short!r}: this child is for a forced short class"
    assert not getattr(_lib.load(), "has_hooks", False), f"{_lib.LIB_PATH}: the short classes are held to the oracle on the shipped library"
    tiles = -(-w // 16) * -(-h // 16)
    assert tiles > 4200, tiles  # (at most 4200 tiles: one launch sorts every tile and no short class runs)
    scenes = [TL.build(name, w, h) for name in names]
    for sc in scenes:
        TL.check_scene(sc)
    dev = sr.Device(0)
    try:
        st = dev.rankStatus()
        assert st["policy"] == (rank or "checked") and st["orderFaults"] == 0, st
        for sc in scenes:
            check_frames(sr, dev, sc, f"short class {short}, {st['policy']}")
        assert dev.rankStatus()["orderFaults"] == 0
    finally:
        dev.destroy()
    print(f"tile_first_child ok: short={short} rank={st['policy']} cases=" + ",".join(f"{n}@{w}x{h}" for n in names))


if __name__ == "__main__":
    main(sys.argv)
