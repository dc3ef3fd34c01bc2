#!/usr/bin/env python3
"""Generates tests/golden/ref_binsorted_*.npz and ref_scan.npz — OUTPUTS OF THE REFERENCE'S OWN CODE.

Almost all of the reference's hot path needs a WebGPU device, but two pieces are plain
CPU loops: the count / exclusive-scan / fill loops of `TileBinner.binSorted` (the definition of the
tile lists, parity contract 2) and the loop of `PrefixSumScanner.scanCPU`.  This script, run in the
build container (the reference is not present anywhere else), reads those statements from
/root/reference as text, strips TypeScript-only syntax IN MEMORY (there is none in these ranges beyond
non-null assertions, but the stripper is applied anyway), and executes them under the container's
Node 12 — the program goes to `node -` on stdin, nothing of it is written to disk — on the inputs of
the committed fixtures plus an edge-case set (off-screen, straddling, NaN, padding indices), all at tile size 16,
and cases at other tile sizes: bounds on and one f32 ulp either side of tile edges at T = 1, 10, 24 and 4096, and
records-only scenes of more than 2^17 and 2^18 tiles (tile ids wider than 17 bits).  Only the
resulting arrays are stored.  tests/ then hold BOTH the oracle and the HIP path to these arrays, so the
integer half of the parity contract (tile counts, offsets, lists; the scan) is pinned to an execution
of the reference itself.  Still unpinned: every float stage (projector, composite) and gl-matrix.

Run from the repo root:  python tests/golden/make_ref_fixtures.py
"""
import json
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src"
TILE = 16  # the scene fixtures' and `edges`' tile size


def strip_types(js):
    """Erasable TypeScript syntax -> JavaScript, for statement bodies (no declarations with generics in here)."""
    js = re.sub(r"(\b(?:let|const|var)\s+\w+)\s*:\s*[\w<>\[\]| ]+(?=\s*=)", r"\1", js)  # let x: T = ...
    js = re.sub(r"(\w|\))!(?=[.\[,;)\s])", r"\1", js)                                   # non-null assertion x!
    js = re.sub(r"\s+as\s+\w+(\[\])?", "", js)                                          # casts
    return js


def between(text, first, last, include_last=False):
    a = text.index(first)
    b = text.index(last, a)
    return text[a:b + (len(last) if include_last else 0)]


def reference_statements():
    tb = open(os.path.join(REF, "TileBinner.ts")).read()
    body = between(tb, "async binSorted(", "async bin(")
    # src/TileBinner.ts:426-495: from the count pass to the end of the fill pass
    loops = between(body, "this.tileCounts = new Uint32Array(this.numTiles);", "readbackBuffer.unmap();")
    ps = open(os.path.join(REF, "PrefixSumScanner.ts")).read()
    scan_body = between(ps, "private async scanCPU(", "cleanupTempBuffers(): void")
    # src/PrefixSumScanner.ts:150-155
    scan = between(scan_body, "const outputData = new Uint32Array(numElements);", "readbackBuffer.unmap();")
    return strip_types(loops), strip_types(scan)


PROGRAM = """
const input = JSON.parse(require('fs').readFileSync(0, 'utf8'));
const GPUBufferUsage = { STORAGE: 0, COPY_DST: 0, MAP_READ: 0 };
function binSorted(sortedIndices, projectedData, screenWidth, screenHeight) {
  %(LOOPS)s
  return { counts: Array.from(this.tileCounts), offsets: Array.from(this.tileOffsets), indices: Array.from(indices),
           total: this.totalSplatCount };
}
function scanCPU(inputData, numElements) {
  %(SCAN)s
  return Array.from(outputData);
}
const out = {};
for (const name of Object.keys(input.bins)) {
  const c = input.bins[name];
  const ntx = Math.ceil(c.width / c.tile), nty = Math.ceil(c.height / c.tile);   // TileBinner.ts ensureBuffers
  const self = { numTiles: ntx * nty, numTilesX: ntx, numTilesY: nty, tileSize: c.tile, splatIndicesBuffer: null,
                 device: { createBuffer: () => ({ destroy() {} }) } };
  const projected = new Float32Array(new Uint32Array(c.projected_bits).buffer);
  out[name] = binSorted.call(self, new Uint32Array(c.sorted), projected, c.width, c.height);
}
out.scans = input.scans.map(a => scanCPU(new Uint32Array(a), a.length));
process.stdout.write(JSON.stringify(out));
"""


def edge_case():
    """Bounds chosen by hand: off-screen on every side, straddling corners, exactly on tile edges, degenerate,
    NaN in every position, and padding indices (0xFFFFFFFF) in the sorted order."""
    w, h = 70, 52  # ragged: 5 x 4 tiles
    nan = np.nan
    b = [[-50, 10, -20, 30], [10, 70, 30, 90], [-5, -5, 5, 5], [60, 40, 100, 100], [16, 16, 32, 32], [nan, 0, 10, 10],
         [0, nan, 10, 10], [0, 0, nan, 10], [0, 0, 10, nan], [20, 20, 20, 40], [20, 20, 40, 20], [30, 30, 10, 10],
         [0, 0, 70, 52], [69.5, 51.5, 69.9, 51.9], [-1e9, -1e9, 1e9, 1e9], [70, 0, 80, 10], [0, 52, 10, 60],
         [15.999, 15.999, 16.0, 16.0], [31.5, 0.25, 48.0, 15.75], [np.inf, 0, np.inf, 10], [-np.inf, 0, np.inf, 10]]
    rec = np.zeros((len(b), 8), np.float32)
    rec[:, :4] = np.array(b, np.float32)
    order = np.array([3, 0xFFFFFFFF, 4, 2, 1, 0, 5, 0xFFFFFFFF, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6], np.uint32)
    return rec, order, w, h


def tile_edge_case(tile, w, h, n=240, seed=5):
    """Bounds on multiples of `tile` and one f32 ulp either side of them (and of the screen's width and height), in
    every coordinate, so that floor(x / tile) lands on both sides of every tile edge.  A non-power-of-two tile takes
    the f64 branch of the binner's tile range, a power of two the f32 one: both must equal the JS-number division."""
    rng = np.random.default_rng(seed)

    def edge_values(limit):
        v = np.arange(0, limit + tile, tile, dtype=np.float32)
        v = np.concatenate([v, np.float32([limit, -1.0, limit + 1.0])])
        return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]).astype(np.float32)

    xs, ys = edge_values(w), edge_values(h)
    rec = np.zeros((n, 8), np.float32)
    a, b = rng.choice(xs, (2, n)), rng.choice(ys, (2, n))
    rec[:, 0], rec[:, 2] = np.minimum(a[0], a[1]), np.maximum(a[0], a[1])
    rec[:, 1], rec[:, 3] = np.minimum(b[0], b[1]), np.maximum(b[0], b[1])
    rec[::17, 2] = rec[::17, 0]  # some empty in x, some reversed in y
    rec[5::19, 1], rec[5::19, 3] = rec[5::19, 3], rec[5::19, 1]
    rec[:, 4:] = rng.random((n, 4), np.float32)
    order = rng.permutation(n).astype(np.uint32)
    order = np.insert(order, [3, n // 2], 0xFFFFFFFF)
    return rec, order


def records_only_case(n, w, h, size, seed):
    """A records-only scene: n random boxes of up to `size` pixels a side over a w x h screen (some hanging off it) in a
    random sorted order."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 8), np.float32)
    x0 = rng.uniform(-size, w, n).astype(np.float32)
    y0 = rng.uniform(-size, h, n).astype(np.float32)
    rec[:, 0], rec[:, 1] = x0, y0
    rec[:, 2] = x0 + rng.uniform(0, size, n).astype(np.float32)
    rec[:, 3] = y0 + rng.uniform(0, size, n).astype(np.float32)
    rec[:, 4:] = rng.random((n, 4), np.float32)
    return rec, rng.permutation(n).astype(np.uint32)


# (name, tile, width, height) of the edge cases at other tile sizes; the screens are not multiples of the tile, and at 4096
# the one tile is larger than the screen
TILE_EDGE_CASES = [("edges_t1", 1, 13, 9), ("edges_t10", 10, 73, 47), ("edges_t24", 24, 101, 77), ("edges_t4096", 4096, 70, 52)]
# (name, tile, width, height, boxes, box size, seed): 140 000 tiles (18-bit ids) and 265 200 tiles (19-bit ids)
RECORDS_ONLY_CASES = [("boxes_t2_800x700", 2, 800, 700, 3000, 24.0, 7), ("boxes_t1_520x510", 1, 520, 510, 400, 12.0, 8)]


def main():
    loops, scan = reference_statements()
    program = PROGRAM % {"LOOPS": loops, "SCAN": scan}
    bins, inputs = {}, {}
    for name in ("tiny7", "small300", "ragged1000"):
        g = np.load(os.path.join(HERE, name + ".npz"))
        n, w, h, _ = (int(x) for x in g["dims"])
        inputs[name] = (g["projected"], g["order"][:n].copy(), w, h, TILE)
    rec, order, w, h = edge_case()
    inputs["edges"] = (rec, order, w, h, TILE)
    for name, tile, w, h in TILE_EDGE_CASES:
        inputs[name] = tile_edge_case(tile, w, h) + (w, h, tile)
    for name, tile, w, h, n, size, seed in RECORDS_ONLY_CASES:
        inputs[name] = records_only_case(n, w, h, size, seed) + (w, h, tile)
    for name, (proj, order, w, h, tile) in inputs.items():
        bins[name] = {"width": w, "height": h, "tile": tile, "sorted": [int(x) for x in order],
                      "projected_bits": [int(x) for x in np.ascontiguousarray(proj, np.float32).view(np.uint32).reshape(-1)]}
    rng = np.random.default_rng(11)
    scans = [[1, 2, 3, 4, 5], [0] * 9, [7], [int(x) for x in rng.integers(0, 5000, 8160)], [int(x) for x in rng.integers(0, 3, 1024)]]
    # the program is handed to node as an argument, the data on stdin: nothing of either is written to disk
    r = subprocess.run(["node", "-e", program], input=json.dumps({"bins": bins, "scans": scans}), capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("node failed:\n" + r.stderr)
    out = json.loads(r.stdout)
    for name, (proj, order, w, h, tile) in inputs.items():
        o = out[name]
        assert o["total"] == len(o["indices"])
        np.savez_compressed(os.path.join(HERE, f"ref_binsorted_{name}.npz"), projected=np.ascontiguousarray(proj, np.float32),
                            sorted=order, dims=np.array([w, h, tile], np.int64), counts=np.array(o["counts"], np.uint32),
                            offsets=np.array(o["offsets"], np.uint32), indices=np.array(o["indices"], np.uint32))
        print(f"ref_binsorted_{name}.npz: {len(o['counts'])} tiles, {o['total']} pairs")
    np.savez_compressed(os.path.join(HERE, "ref_scan.npz"), **{f"in{i}": np.array(a, np.uint32) for i, a in enumerate(scans)},
                        **{f"out{i}": np.array(a, np.uint32) for i, a in enumerate(out["scans"])})
    print(f"ref_scan.npz: {len(scans)} cases; node {subprocess.run(['node', '--version'], capture_output=True, text=True).stdout.strip()}")


if __name__ == "__main__":
    main()
