"""CPU tests of the point-cloud initialisation: the NumPy restatement of splat_knn_mean_sq's contract (tests/knn_ref.py) against
a binary64 brute force and on the contract's special cases, the header, the build, and load_point_ply.

The 2 ulp of the first test.  On arbitrary floats a d(i, j) carries the roundings of a difference, a square and two sums (up to
about 5 x 2^-24 relative, all terms being non-negative) and the mean two sums and a division: 4 ulp at worst, so 2 ulp is no
bound there.  The test's cloud is a jittered grid whose coordinates are multiples of 2^-7 in [0, 8): differences (11 bits),
squares (20 bits) and their sums (22 bits) are then exact in binary32, binary32 and binary64 see the same distances and pick the
same neighbours whatever the ties, and what is left is two sums and a division, half an ulp each: 1.5 ulp, under the 2 asserted.
What the test holds is the rule itself: the operation order, j != i, the three smallest, the chunking and the row lists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from splat_renderer_amd import SplatError, load_point_ply
from tests import knn_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def ulp32(x):
    x = np.abs(np.asarray(x, F))
    return (np.nextafter(x, F(np.inf)) - x).astype(np.float64)


def test_restatement_agrees_with_float64():
    rng = np.random.default_rng(21)
    g = np.arange(9, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * 0.875 + 0.5 + rng.uniform(-0.3, 0.3, (729, 3))
    p = (np.round(p * 128.0) / 128.0).astype(F)
    assert p.min() >= 0 and p.max() < 8 and np.array_equal(p * F(128), np.round(p * F(128)))
    want, b = KR.mean_sq_f64(p)
    d64 = ((p[:, None, :].astype(np.float64) - p[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(d64.astype(F).astype(np.float64), d64), "the distances are not exact in binary32"
    assert len(np.unique(p, axis=0)) == 729 and b[:, 0].min() > 0
    got = KR.mean_sq(p)
    err = float((np.abs(got.astype(np.float64) - want) / ulp32(want)).max())
    print(f"729 points: max |binary32 - binary64| = {err:.3f} ulp; nearest pair {np.sqrt(b[:, 0].min()):.3g} apart")
    assert err <= 2.0
    assert np.array_equal(KR.mean_sq(p, rows=[5, 700, 31]), got[[5, 700, 31]])
    assert np.array_equal(KR.mean_sq(p, chunk=7), got)
    wide = np.concatenate([p, np.full((729, 1), np.nan, F)], axis=1)
    assert np.array_equal(KR.mean_sq(wide), got), "the fourth column was read"


def test_duplicates_give_exact_zeros():
    base = KR.uniform(50, 22)
    p = np.concatenate([base, base[:10], base[:10], base[:10], base[20:30], base[20:30]])
    got = KR.mean_sq(p)
    four = np.r_[0:10, 50:80]      # a point and three copies: three neighbours at distance 0
    three = np.r_[20:30, 80:100]   # a point and two copies: b0 = b1 = 0, the third is a real neighbour
    print(f"rows with three copies: max {got[four].max()}; rows with two copies: min {got[three].min():.3g}")
    assert (got[four].view(np.uint32) == 0).all(), "three copies must give +0.0 exactly"
    assert (got[three] > 0).all()
    for i in three:  # (0 + 0) + b2 is exact: the row is the third smallest binary32 distance over 3
        dx, dy, dz = (p[i, a] - np.delete(p[:, a], i) for a in range(3))
        assert got[i] == np.sort((dx * dx + dy * dy) + dz * dz)[2] / F(3.0)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fewer_than_four_points(n):
    got = KR.mean_sq(KR.uniform(n, 23))
    print(n, got)
    assert got.shape == (n,) and np.isposinf(got).all()
    assert np.isfinite(KR.mean_sq(KR.uniform(4, 23))).all()


def test_non_finite_points():
    p = KR.uniform(40, 24)
    clean = KR.mean_sq(p)
    q = np.concatenate([p, p[:3]])
    q[40, 0], q[41, 2], q[42, 1] = np.nan, np.inf, -np.inf
    got = KR.mean_sq(q)
    print(f"rows of the non-finite points: {got[40:]}")
    assert np.isposinf(got[40:]).all(), "a point with a NaN or infinite coordinate gets +inf"
    assert np.array_equal(got[:40], clean), "a non-finite point changed its neighbours' rows"
    far = np.concatenate([p, np.array([[3e38, 0, 0]], F)])  # finite, but every square overflows
    got = KR.mean_sq(far)
    assert np.isposinf(got[40]) and np.array_equal(got[:40], clean)


def test_morton_order_on_known_cells():
    """KR.morton_order on a cloud whose cells can be read off: the box is [0, 8]^3, a coordinate c falls in cell
    floor(c / 8 * 2^21) (the maximum in the last cell), bit k of axis a's cell sits at bit 3 k + a, a non-finite point gets the
    largest code, and equal codes keep their index order."""
    p = np.array([[0, 0, 0], [8, 8, 8], [4, 0, 0], [0, 4, 0], [0, 0, 4], [np.nan, 1, 1], [4, 0, 0], [1, 2, np.inf], [8, 0, 0],
                  [2.0 ** -18, 0, 0], [0, 2.0 ** -18, 0]], F)
    order, codes = KR.morton_order(p)
    top, full = 1 << 20, (1 << 21) - 1
    spread = lambda v: sum(((v >> k) & 1) << (3 * k) for k in range(21))  # noqa: E731
    want = [0, spread(full) * 7, spread(top), spread(top) << 1, spread(top) << 2, 2 ** 63 - 1, spread(top), 2 ** 63 - 1, spread(full), 1, 2]
    assert codes.dtype == np.uint64 and codes.tolist() == want
    assert order.tolist() == [0, 9, 10, 2, 6, 8, 3, 4, 1, 5, 7], order
    assert KR.block_of(np.arange(130)[::-1]).tolist() == [2, 2] + [1] * 64 + [0] * 64
    # a degenerate axis (no extent) is cell 0, and a cloud with no finite point is all the largest code, in index order
    flat = KR.uniform(50, 27)
    flat[:, 1] = 0.5
    assert not (KR.morton_order(flat)[1] & np.uint64(0x2492492492492492)).any()
    order, codes = KR.morton_order(np.full((5, 3), np.nan, F))
    assert (codes == np.uint64(2 ** 63 - 1)).all() and order.tolist() == [0, 1, 2, 3, 4]
    # the rows only the second trip over the groups serves: a neighbour more than 64 blocks away and in a group from 64 on
    block = np.array([0, 4095, 4096, 4160, 4161, 4700])
    assert KR.second_far_trip(block, [0, 2, 3, 4, 5], [[0, 1, 1], [1, 3, 3], [2, 2, 2], [2, 3, 4], [1, 1, 2]]).tolist() == \
        [False, False, False, True, True]


def test_clouds_past_64_groups_reach_the_second_trip():
    """What tests/test_gpu_knn.py's clouds above 262 144 points are there for, counted without a GPU (the neighbours from scipy's
    cKDTree in float64: an approximation of the binary32 rule that is good enough for counts this far from their bounds).
    uniform(300 000, 21): at least 1000 queries have a neighbour that only k_knn_search's second far trip reaches (measured:
    3345; 467 at n = 270 336; 0 at 262 145 and at 262 144, where there is no such trip or one group of one block)."""
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree

    def second_trip_queries(p):
        order, codes = KR.morton_order(p)
        fin = np.flatnonzero(np.isfinite(p).all(axis=1))
        q = p[fin].astype(np.float64)
        nb = fin[cKDTree(q).query(q, k=4)[1][:, 1:]]
        return int(KR.second_far_trip(KR.block_of(order), fin, nb).sum()), order, codes

    counts = {n: second_trip_queries(KR.uniform(n, 21))[0] for n in (KR.FAR_HEAD, KR.FAR_HEAD + 1, KR.FAR_N)}
    print(f"queries served by the second far trip: {counts}")
    assert counts[KR.FAR_HEAD] == 0 and counts[KR.FAR_HEAD + 1] == 0 and counts[KR.FAR_N] >= 1000
    # the non-finite tail: 6000 rows, one coordinate each, of the three kinds; a whole group of the second trip holds nobody
    p, rows = KR.nonfinite_tail()
    assert rows.size == 6000 and np.array_equal(np.flatnonzero(~np.isfinite(p).all(axis=1)), rows)
    assert ((~np.isfinite(p)).sum(axis=1)[rows] == 1).all()
    assert all(k.sum() >= 1000 for k in (np.isnan(p).any(axis=1), np.isposinf(p).any(axis=1), np.isneginf(p).any(axis=1)))
    count, order, codes = second_trip_queries(p)
    assert (codes[rows] == np.uint64(2 ** 63 - 1)).all() and np.array_equal(np.sort(order[-6000:]), rows)
    fin = np.isfinite(p).all(axis=1)
    held = np.bincount(KR.block_of(order)[fin] // KR.GROUP, minlength=74)
    print(f"non-finite tail: {count} second-trip queries; finite points per group from 64 on: {held[64:]}")
    assert held.size == 74 and count >= 1000 and held[72] == 0 and held[:71].min() == KR.BLOCK * KR.GROUP
    # the shifted tail: all codes distinct (what the evaluation counts' equality under a row reversal rests on)
    p = KR.shifted_tail()
    count, order, codes = second_trip_queries(p)
    print(f"shifted tail: {count} second-trip queries")
    assert np.unique(codes).size == KR.FAR_N and count >= 1000
    assert p[:KR.FAR_HEAD, 0].max() < 1 and p[KR.FAR_HEAD:, 0].min() >= 9 and np.abs(p[:, 1:]).max() <= 1


def test_header_declares_the_section():
    text = open(os.path.join(ROOT, "include", "splat.h")).read()
    assert "Initialisation from a point cloud" in text
    assert re.search(r"#define SPLAT_ABI_VERSION 3\b", text)
    assert re.search(r"uint64_t\s+splat_knn_workspace_bytes\s*\(\s*uint32_t n\s*\)\s*;", text)
    m = re.search(r"int\s+splat_knn_mean_sq\s*\(([^;]*)\)\s*;", text)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "ctx", "sorter", "points", "stride_floats", "n", "workspace", "workspace_bytes", "mean_sq", "evaluations"]


def test_library_exports_the_symbols():
    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "splat_knn_workspace_bytes") and hasattr(lib, "splat_knn_mean_sq")
    assert "splat_knn_workspace_bytes" in _lib.SIGNATURES and "splat_knn_mean_sq" in _lib.SIGNATURES
    f = lib.splat_knn_workspace_bytes
    f.restype, f.argtypes = C.c_uint64, [C.c_uint32]
    sizes = [int(f(n)) for n in (0, 1, 64, 65, 100000)]
    print("workspace bytes for n = 0, 1, 64, 65, 100000:", sizes)
    assert sizes == sorted(sizes) and sizes[4] >= 100000 * 20 and all(s % 16 == 0 for s in sizes)


def test_knn_object_is_built_without_contraction():
    """The search's bounds are lower bounds only while they round as the distance does: knn.o is an EXACT object."""
    csrc = os.path.join(ROOT, "splat_renderer_amd", "csrc")
    out = subprocess.run(["make", "-n", "-B", "-C", csrc, "_obj/knn.o"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "knn.hip" in ln and "-c" in ln]
    print(lines)
    assert len(lines) == 1 and "-ffp-contract=off" in lines[0] and "-ffp-contract=on" not in lines[0] and "-ffast-math" not in lines[0]
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "$(BUILD)/knn.o" in mk.split("OBJS =")[1].split("\n\n")[0], "knn.o is not linked into the library"


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("normals", [False, True])
def test_load_point_ply(tmp_path, double, normals):
    rng = np.random.default_rng(25)
    xyz = rng.normal(0, 3, (257, 3))
    xyz = xyz if double else xyz.astype(F)
    rgb8 = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    rgb8[0], rgb8[1] = 0, 255
    path = str(tmp_path / "points3D.ply")
    KR.write_point_ply(path, xyz, rgb8, double=double, normals=normals)
    got_xyz, got_rgb = load_point_ply(path)
    assert got_xyz.dtype == F and got_xyz.shape == (257, 3) and got_rgb.dtype == F and got_rgb.shape == (257, 3)
    assert got_xyz.flags.c_contiguous and got_rgb.flags.c_contiguous
    assert np.array_equal(got_xyz, xyz.astype(F))
    assert np.array_equal(got_rgb, rgb8.astype(F) / F(255.0))
    assert got_rgb.min() == 0.0 and got_rgb.max() == 1.0


def test_load_point_ply_rejections(tmp_path):
    xyz = KR.uniform(5, 26)
    path = str(tmp_path / "no_colours.ply")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        f.write(xyz.tobytes())
    with pytest.raises(SplatError) as ei:
        load_point_ply(path)
    print(ei.value)
    assert ei.value.code == -1 and "red" in str(ei.value) and "no_colours.ply" in str(ei.value)
    ok = str(tmp_path / "ok.ply")
    KR.write_point_ply(ok, xyz, np.zeros((5, 3), np.uint8))
    raw = open(ok, "rb").read()
    for name, data, why in (("short.ply", raw[:-4], "ends after"), ("ascii.ply", raw.replace(b"binary_little_endian", b"ascii"), "format"),
                            ("magic.ply", b"plx" + raw[3:], "magic"), ("int.ply", raw.replace(b"property float x", b"property int x"), "float or double")):
        bad = str(tmp_path / name)
        open(bad, "wb").write(data)
        with pytest.raises(SplatError) as ei:
            load_point_ply(bad)
        assert why in str(ei.value), (name, str(ei.value))
