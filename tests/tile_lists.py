"""Scenes for the tile-first binner in which chosen tiles hold chosen numbers of pairs (CPU only: oracle + tests.helpers).

Almost every branch of k_tile_sort, k_tf_scatter and the second tile-id pass is decided by an exact list length, pair count
or splat count; a random scene never puts one of those on an edge.  Here a sparse scene is thinned to ANCHORS (splats whose
rectangle is one tile that holds nothing else) and L - 1 further small splats are placed on an anchor's view ray, so that
the anchor's tile holds exactly L pairs.  How far they are spread along the ray sets the tile's key range, i.e. the number
of radix passes its sort takes; about a quarter of every list are exact positional duplicates of other entries (equal depth
keys, resolved by splat index).  Nothing about a scene is taken on trust: check_scene() asserts its purpose from the oracle's
lists alone, in tests/test_tile_first_edges_cpu.py and again at the top of every GPU test that renders it.
"""
import functools

import numpy as np

from oracle import oracle as O
from tests.helpers import make_case, oracle_pipeline

TILE = 16
# every list length at which the per-tile sort or the order check takes another path ("List-length edges")
BY_LENGTH = [1, 2, 63, 64, 65, 127, 255, 256, 257, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096,
             4097, 5887, 5888, 5889, 6143, 6144, 6145, 8191, 8192, 8193, 12288, 12289]
BY_PASSES_LENGTHS = [256, 2048, 2049, 4096, 4097, 5888, 5889, 8193]
BY_PASSES = [(length, passes) for length in BY_PASSES_LENGTHS for passes in range(5)]
# 70 x 60 = 4200 tiles: the largest screen one launch sorts; 71 x 60 = 4260: two classes, and below the 6144 tiles from
# which the frame's mean list length picks the short class (so the class is 8 unless SPLAT_TILE_SORT_SHORT forces one)
ONE_CLASS_SCREEN = (1120, 960)
TWO_CLASS_SCREEN = (1136, 960)
ALIGNED_LENGTHS = (4096, 4097)  # one whole partition of the second tile-id pass, and one partition plus one pair
SPARSE_SPLATS = 3000            # the thinned scene leaves ~300 anchors: the piles' tiles, and single-entry filler tiles


def tile_id_low_bits(tiles):
    """The low digit of the two-pass tile-id sort (csrc/common.h: tile_id_low_bits)."""
    bits = 1
    while (1 << bits) < tiles:
        bits += 1
    return bits if bits <= 8 else min(bits // 2, 8)


def tile_rects(proj, w, h, tile=TILE):
    """Per splat (tx0, tx1, ty0, ty1, hits) of TileBinner.binSorted's rectangle (oracle.c: bin_range), in float64 as there."""
    ntx, nty = -(-w // tile), -(-h // tile)
    r = proj[:, :4].astype(np.float64)
    min_x, min_y = np.maximum(r[:, 0], 0.0), np.maximum(r[:, 1], 0.0)
    max_x, max_y = np.minimum(r[:, 2], float(w)), np.minimum(r[:, 3], float(h))
    a, b = np.floor(min_x / tile), np.minimum(np.floor(max_x / tile), ntx - 1.0)
    c, d = np.floor(min_y / tile), np.minimum(np.floor(max_y / tile), nty - 1.0)
    ok = ~np.isnan(r).any(axis=1) & (min_x < max_x) & (min_y < max_y) & (a <= b) & (c <= d)
    a, b, c, d = (np.where(ok, v, 0).astype(np.int64) for v in (a, b, c, d))
    hits = np.where(ok, (b - a + 1) * (d - c + 1), 0)
    return a, b, c, d, hits


def list_passes(ref, tile):
    """Radix passes of the tile's sort: ceil(bits(kmax - kmin) / 8), from the oracle's keys."""
    lst = ref["indices"][ref["offsets"][tile]:ref["offsets"][tile] + ref["counts"][tile]]
    k = ref["keys"][lst].astype(np.int64)
    return (int(k.max() - k.min()).bit_length() + 7) // 8


def _pile(rng, anchor_row, anchor_depth, px_per_radius, eye, length, passes):
    """length - 1 rows (x, y, z, radius) on the view ray of the anchor.  passes: None (natural spread: a few hundred
    thousand key steps), or 0..4."""
    extra = length - 1
    if extra == 0:
        return np.zeros((0, 4), np.float32)
    p = anchor_row[:3].astype(np.float64)
    ulp = float(np.spacing(np.float32(anchor_depth)))  # one key step (the anchors lie at depths in [2.2, 3.7): one binade)
    dups = extra if passes == 0 else length // 4
    fresh = extra - dups
    if passes is None:
        delta = rng.uniform(0.001, 0.05, fresh)
    else:
        steps = {0: 0, 1: 200, 2: 1 << 14, 3: 1 << 20, 4: 1 << 20}[passes]
        delta = rng.integers(0, steps + 1, fresh).astype(np.float64) * ulp
        if fresh:
            delta[0] = steps * ulp  # (the range itself, not left to the draw)
    scale = 1.0 + delta / anchor_depth
    if passes == 4:  # a few entries a tenth of the way from the eye: three binades nearer, keys 2^24 and more apart
        scale[:min(8, fresh)] = rng.uniform(0.09, 0.11, min(8, fresh))
    rows = np.empty((extra, 4), np.float64)
    rows[:fresh, :3] = eye + (p - eye) * scale[:, None]
    # a projected radius of a quarter pixel wherever the splat sits on the ray (the anchor's own radius gives the ratio)
    rows[:fresh, 3] = 0.25 / px_per_radius * scale
    members = np.vstack([anchor_row[None, :4].astype(np.float64), rows[:fresh]])
    rows[fresh:] = members[rng.integers(0, members.shape[0], dups)]  # exact duplicates: equal keys, resolved by index
    return rows.astype(np.float32)


@functools.lru_cache(maxsize=None)
def build(name, w, h):
    """name: "by_length" (one tile per length of BY_LENGTH, natural key range) or "by_passes" (one tile per (length, passes)
    of BY_PASSES).  Returns a dict: props, normals, u, w, h, ref (the oracle pipeline's result), table ((tile, length,
    passes) per piled tile, int64), requested ([(length, passes or None)]).  Shared between tests: treat it as read-only."""
    requested = {"by_length": [(length, None) for length in BY_LENGTH], "by_passes": list(BY_PASSES)}[name]
    rng = np.random.default_rng({"by_length": 11, "by_passes": 12}[name])
    base, _, u = make_case(SPARSE_SPLATS, w, h, 97, 1.0)
    base[:, 3] = np.float32(6e-4)  # ~0.25 px
    eye = np.asarray(u[16:19], np.float64)
    ntx, nty = -(-w // TILE), -(-h // TILE)
    ref0 = oracle_pipeline(base, None, u, w, h)
    proj = ref0["proj"]
    tx0, _, ty0, _, hits = tile_rects(proj, w, h)
    tile_of = ty0 * ntx + tx0
    cx, cy = (proj[:, 0] + proj[:, 2]) * 0.5, (proj[:, 1] + proj[:, 3]) * 0.5
    inside = (np.abs(cx % TILE - 8.0) <= 5.0) & (np.abs(cy % TILE - 8.0) <= 5.0)  # (room for the pile's rounding)
    depth = proj[:, 4]
    anchors = np.nonzero((hits == 1) & (ref0["counts"][tile_of] == 1) & inside & (depth >= 2.2) & (depth < 3.7))[0]
    anchors = anchors[rng.permutation(anchors.size)]
    lo_mask = (1 << tile_id_low_bits(ntx * nty)) - 1
    digit = tile_of[anchors] & lo_mask
    # the aligned lengths first: each takes a low tile-id digit that no other occupied tile shares
    taken, exclusive, chosen = np.zeros(anchors.size, bool), set(), {}
    for j, (length, _) in enumerate(requested):
        if length in ALIGNED_LENGTHS:
            k = next(k for k in range(anchors.size) if not taken[k] and int(digit[k]) not in exclusive)
            taken[k] = True
            exclusive.add(int(digit[k]))
            chosen[j] = k
    shared = np.isin(digit, list(exclusive))
    for j, (length, _) in enumerate(requested):
        if j not in chosen:
            k = next(k for k in range(anchors.size) if not taken[k] and not shared[k])
            taken[k] = True
            chosen[j] = k
    keep = taken | ~shared  # filler: every other anchor outside the exclusive digits, one pair each
    rows, piles = [base[anchors[keep], :4]], []
    for j, (length, passes) in enumerate(requested):
        a = anchors[chosen[j]]
        piles.append(int(tile_of[a]))
        rows.append(_pile(rng, base[a], float(depth[a]), float(proj[a, 5]) / float(base[a, 3]), eye, length, passes))
    pos_radius = np.vstack(rows)
    n = pos_radius.shape[0]
    order = rng.permutation(n)  # a list's members lie all over the index range: across the scatter's blocks
    props = np.empty((n, 8), np.float32)
    props[:, :4] = pos_radius[order]
    props[:, 4:7] = rng.uniform(0.0, 1.0, (n, 3))
    props[:, 7] = rng.uniform(0.01, 0.05, n)  # (thin: the composite walks deep into the long lists)
    normals = np.empty((n, 4), np.float32)
    nrm = rng.standard_normal((n, 3))
    normals[:, :3] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    normals[:, 3] = 1.0
    ref = oracle_pipeline(props, normals, u, w, h)
    table = np.array([(t, length, list_passes(ref, t) if ref["counts"][t] else -1) for t, (length, _) in zip(piles, requested)], np.int64)
    return dict(name=name, props=props, normals=normals, u=u, w=w, h=h, ref=ref, table=table, requested=requested)


def check_scene(sc):
    """The scene's purpose, from the oracle's lists alone: every requested (length, passes) is there exactly, no other
    tile is longer than 1, the pair total is what the table sums to, and the aligned lengths' first-pass runs hold nothing
    else."""
    ref, table, w, h = sc["ref"], sc["table"], sc["w"], sc["h"]
    counts = ref["counts"].astype(np.int64)
    tiles = counts.size
    assert tiles == -(-w // TILE) * -(-h // TILE)
    assert np.unique(table[:, 0]).size == table.shape[0] == len(sc["requested"])
    got = []
    for t, length, passes in table:
        assert counts[t] == length, (int(t), int(counts[t]), int(length))
        assert passes == list_passes(ref, t)
        got.append((int(length), int(passes)))
    for (length, passes), (want_length, want_passes) in zip(got, sc["requested"]):
        assert length == want_length
        if want_passes is not None:
            assert passes == want_passes, (length, passes, want_passes)
        else:  # the natural key range
            assert passes == 0 if length == 1 else passes in (2, 3), (length, passes)
    if sc["name"] == "by_length":
        assert [g[0] for g in got] == BY_LENGTH
    else:
        assert got == BY_PASSES
    others = counts.copy()
    others[table[:, 0]] = 0
    assert others.max() <= 1, int(others.max())
    total = int(table[:, 1].sum() + others.sum())
    assert ref["indices"].shape[0] == total == sc["props"].shape[0]  # (every splat is exactly one pair)
    assert 100_000 < total < 400_000
    # a quarter of every list ties with another entry of it
    for t, length, passes in table:
        lst = ref["indices"][ref["offsets"][t]:ref["offsets"][t] + length]
        k = ref["keys"][lst]
        tied = length - np.unique(k).size
        assert tied >= (length // 4 if passes else length - 1), (int(length), int(tied))
    if tiles > 256:
        lo_mask = (1 << tile_id_low_bits(tiles)) - 1
        occupied = np.nonzero(counts)[0]
        for t, length, _ in table:
            if length in ALIGNED_LENGTHS:
                assert np.count_nonzero((occupied & lo_mask) == (t & lo_mask)) == 1, (int(t), int(length))
    return total


# ---- 1024-splat blocks with ragged tails ------------------------------------------------------------------------------
RAGGED_SCREEN = (320, 208)  # 20 x 13 = 260 tiles: the second tile-id pass runs


@functools.lru_cache(maxsize=None)
def _ragged_base():
    w, h = RAGGED_SCREEN
    props, normals, u = make_case((1 << 20) + 3, w, h, 131, 0.25)
    return props, normals, u, O.project(u, props)


@functools.lru_cache(maxsize=None)
def ragged_tail(r):
    """2^20 + r splats of about one pair each: the smallest frames that take 1024-splat blocks (four splats per thread,
    one 16-byte load) outside a band, with a tail of r splats behind the last whole load."""
    w, h = RAGGED_SCREEN
    props, normals, u, proj = _ragged_base()
    n = (1 << 20) + r
    props, normals, proj = props[:n], normals[:n], proj[:n]
    keys, pay = O.extract_keys(proj)
    _, order = O.sort_pairs(keys, pay)
    counts, offsets, idx = O.bin_sorted(proj, order, w, h, TILE)
    ref = dict(proj=proj, keys=keys, order=order, counts=counts, offsets=offsets, indices=idx)
    return dict(name=f"ragged_tail_{r}", props=props, normals=normals, u=u, w=w, h=h, ref=ref)


def check_ragged_tail(sc, r):
    n, w, h = sc["props"].shape[0], sc["w"], sc["h"]
    assert n == (1 << 20) + r and n > 2 ** 20 and n % 4 == r  # (beyond TF_SMALL_FRAME_SPLATS, r splats past a whole load)
    assert sc["ref"]["counts"].size > 256
    hits = tile_rects(sc["ref"]["proj"], w, h)[4]
    total = int(sc["ref"]["indices"].shape[0])
    assert hits.sum() == total and 0.5 * n < total < 2.0 * n, (n, total)
    assert hits[n - r:].min() >= 1  # the tail's splats are on the screen: a dropped one is a missing pair
    return total


# ---- blocks that expand in several rounds -----------------------------------------------------------------------------
TF_STAGE = 4096  # pairs a block of the scatter stages per round (csrc/tile_first.hip)


@functools.lru_cache(maxsize=None)
def multi_round(kind):
    """kind "block": 700 splats of ~40 tiles each — every 256-splat block expands in several rounds of TF_STAGE pairs;
    "giant": one splat whose own rectangle is the whole screen of 65 x 64 tiles, among small ones."""
    if kind == "block":
        w, h, n = 640, 480, 700
        props, normals, u = make_case(n, w, h, 141, 1.0)
        props[:, 3] = np.float32(0.16) * props[:, 3] / props[:, 3].mean()
    else:
        w, h, n = 1040, 1024, 300
        props, normals, u = make_case(n, w, h, 142, 0.02)
        props[100, :4] = (0.0, 0.0, 0.0, 1.0)
    ref = oracle_pipeline(props, normals, u, w, h)
    return dict(name=f"multi_round_{kind}", props=props, normals=normals, u=u, w=w, h=h, ref=ref)


def check_multi_round(sc, kind):
    w, h = sc["w"], sc["h"]
    hits = tile_rects(sc["ref"]["proj"], w, h)[4]
    assert hits.sum() == sc["ref"]["indices"].shape[0]
    assert sc["props"].shape[0] <= 2 ** 20  # (256-splat blocks)
    straddles = 0
    sums = []
    for b0 in range(0, hits.size, 256):
        hb = hits[b0:b0 + 256]
        off = np.cumsum(hb) - hb
        sums.append(int(hb.sum()))
        for edge in range(TF_STAGE, sums[-1], TF_STAGE):
            straddles += int(np.any((off < edge) & (off + hb > edge)))
    if kind == "block":
        assert max(sums) > 2 * TF_STAGE and min(sums[:-1]) > TF_STAGE, sums  # a wide margin: three rounds and more
        assert straddles >= 2, straddles
    else:
        assert -(-w // TILE) >= 65 and -(-h // TILE) >= 64
        assert hits[100] == (-(-w // TILE)) * (-(-h // TILE)) > TF_STAGE, int(hits[100])
        assert straddles >= 1
    return int(hits.sum())
