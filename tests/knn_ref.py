"""NumPy restatement of splat_knn_mean_sq's contract (include/splat.h, "Initialisation from a point cloud"): brute force in
binary32, every operator one rounding, in the header's operation order.

    d(i, j)    = ((dx dx + dy dy) + dz dz)            dx = x_i - x_j, ...
    candidates = the j != i with d(i, j) finite       (a duplicate is a candidate, at distance 0)
    b0 <= b1 <= b2 = the three smallest, padded with +inf
    mean_sq[i] = ((b0 + b1) + b2) / 3.0f

NumPy's float32 array operations round once each and never contract, so this is the contract and not an approximation of it.
Also the scenes the CPU and GPU tests share, and a writer for the point PLYs that load_point_ply reads.
"""
import numpy as np

F = np.float32


def mean_sq(points, rows=None, chunk=256):
    """points (n, >= 3) float32 (columns past the third are not read) -> mean_sq of every point, or of the points in `rows`;
    chunked over the queries: chunk x n distances at a time."""
    p = np.ascontiguousarray(np.asarray(points, F)[:, :3])
    n = p.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    out = np.empty(rows.shape[0], F)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    with np.errstate(all="ignore"):
        for s in range(0, rows.shape[0], chunk):
            r = rows[s:s + chunk]
            dx, dy, dz = x[r, None] - x[None, :], y[r, None] - y[None, :], z[r, None] - z[None, :]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == F
            d[~np.isfinite(d)] = np.inf
            d[np.arange(r.shape[0]), r] = np.inf  # j != i
            if n < 3:
                d = np.concatenate([d, np.full((r.shape[0], 3 - n), np.inf, F)], axis=1)
            b = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
            out[s:s + chunk] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / F(3.0)
    return out


def mean_sq_f64(points):
    """The same rule in binary64 (for the restatement's own error): (mean_sq float64 (n,), b (n, 3) the three distances)."""
    p = np.asarray(points, F)[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    d[~np.isfinite(d)] = np.inf
    np.fill_diagonal(d, np.inf)
    b = np.sort(d, axis=1)[:, :3]
    return b.sum(axis=1) / 3.0, b


AXIS_BITS, BLOCK, GROUP, NEAR = 21, 64, 64, 64  # knn.hip's KNN_AXIS_BITS, KB, KG, KNN_NEAR


def morton_order(points):
    """(order, codes): k_knn_codes and the two stable sorts restated in float64.  codes[i] is point i's 63-bit code, the box of
    the finite points cut into 2^21 cells per axis, bit k of axis a's cell at bit 3 k + a, 2^63 - 1 for a point with a non-finite
    coordinate; order[pos] is the point at sorted position pos, ties by index.  The search's results do not depend on the order:
    the tests use it to prove that a cloud reaches the blocks and groups it is there for, and for nothing else."""
    p = np.asarray(points, F)[:, :3]
    n = p.shape[0]
    fin = np.isfinite(p).all(axis=1)
    codes = np.full(n, 0x7fffffffffffffff, np.uint64)
    if fin.any():
        q = p[fin].astype(np.float64)
        lo, ext = q.min(axis=0), q.max(axis=0) - q.min(axis=0)
        cells = float(1 << AXIS_BITS)
        code = np.zeros(q.shape[0], np.uint64)
        for a in range(3):
            t = (q[:, a] - lo[a]) / ext[a] * cells if ext[a] > 0.0 else np.zeros(q.shape[0])
            cell = np.clip(t, 0.0, cells - 1.0).astype(np.uint64)  # (truncation, as the kernel's cast)
            for k in range(AXIS_BITS):
                code |= ((cell >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k + a)
        codes[fin] = code
    return np.argsort(codes, kind="stable"), codes


def block_of(order):
    """block[i]: the 64-point block of the sorted array that point i lies in."""
    block = np.empty(order.shape[0], np.int64)
    block[order] = np.arange(order.shape[0]) // BLOCK
    return block


def second_far_trip(block, rows, neighbours):
    """Which of the queries `rows`, with neighbour indices `neighbours` (len(rows), 3), have a neighbour that only the search's
    second trip over the groups can find: one in a block more than NEAR blocks from the query's own (so not met in the near
    rounds) and in a group of index 64 or higher (so not in the first trip's 64 groups).  `block` is block_of(order)."""
    nb, qb = block[np.asarray(neighbours, np.int64)], block[np.asarray(rows, np.int64)][:, None]
    return ((np.abs(nb - qb) > NEAR) & (nb // GROUP >= 64)).any(axis=1)


# ---- scenes (seeds fixed here) -------------------------------------------------------------------------------------------------

def uniform(n, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F)


def scene(name):
    """The exact-bits scenes of tests/test_gpu_knn.py, by name."""
    rng = np.random.default_rng({"uniform": 11, "grid": 12, "clusters": 13, "duplicates": 14, "line": 15, "identical": 16, "outlier": 17,
                                 "nonfinite": 18}[name])
    if name == "uniform":
        return rng.uniform(-1, 1, (2000, 3)).astype(F)
    if name == "grid":  # all ties
        g = np.arange(10, dtype=F)
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        return np.ascontiguousarray(p[rng.permutation(p.shape[0])])
    if name == "clusters":  # sigma 1e-4, 3 and 200 at 0, 50 and -1000
        parts = [rng.normal(c, s, (k, 3)) for c, s, k in ((0.0, 1e-4, 600), (50.0, 3.0, 700), (-1000.0, 200.0, 500))]
        p = np.concatenate(parts).astype(F)
        return np.ascontiguousarray(p[rng.permutation(p.shape[0])])
    if name == "duplicates":  # 400 points, 200 of them duplicated once and 50 duplicated three times (exact zeros)
        base = rng.uniform(-1, 1, (400, 3)).astype(F)
        p = np.concatenate([base, base[:200], base[350:], base[350:], base[350:]])
        return np.ascontiguousarray(p[rng.permutation(p.shape[0])])
    if name == "line":
        t = rng.uniform(-5, 5, 700)
        return np.stack([0.3 * t + 1.0, -0.7 * t, 2.0 * t - 3.0], axis=1).astype(F)
    if name == "identical":
        return np.tile(np.array([[0.25, -1.5, 3.0]], F), (130, 1))
    if name == "outlier":
        p = rng.uniform(-1, 1, (1500, 3)).astype(F)
        p[777] = (1e6, -1e6, 3e5)
        return p
    if name == "nonfinite":
        p = rng.uniform(-1, 1, (300, 3)).astype(F)
        p[41, 1] = np.nan
        p[200, 0] = np.inf
        return p
    raise KeyError(name)


SCENES = ("uniform", "grid", "clusters", "duplicates", "line", "identical", "outlier", "nonfinite")


def pruning_scene(name, n=32768):
    """The three clouds of the pruning test, from default_rng(3): the uniform cube; the same cloud with rows 0-7 replaced by
    uniform points in [-1000, 1000)^3 (the generator's next draws); the unit sphere's surface (a fresh default_rng(3))."""
    rng = np.random.default_rng(3)
    if name == "sphere":
        v = rng.normal(size=(n, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    p = rng.uniform(-1, 1, (n, 3)).astype(F)
    if name == "outliers":
        p[:8] = rng.uniform(-1000, 1000, (8, 3)).astype(F)
    elif name != "cube":
        raise KeyError(name)
    return p


FAR_N, FAR_HEAD = 300000, 262144  # 4688 blocks in 74 groups; 64 groups of 64 blocks of 64 points, the first trip's reach


def nonfinite_tail():
    """(points, rows): uniform(FAR_N, 21) with 6000 rows (default_rng(22)) given a NaN, a +inf or a -inf in one coordinate.  They
    sort to the end: the last 94 blocks, among them all of group 72, hold no finite point."""
    p = uniform(FAR_N, 21)
    rng = np.random.default_rng(22)
    rows = np.sort(rng.choice(FAR_N, 6000, replace=False))
    p[rows, rng.integers(0, 3, rows.size)] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(rows.size) % 3]
    return p, rows


def shifted_tail():
    """Rows below FAR_HEAD uniform in [-1, 1)^3, the rows from there on uniform in [9, 11) x [-1, 1)^2 (default_rng(23)): the
    first trip of k_knn_bbox's 1024 workgroups sees x below 1 only."""
    rng = np.random.default_rng(23)
    p = rng.uniform(-1, 1, (FAR_N, 3)).astype(F)
    p[FAR_HEAD:, 0] = rng.uniform(9, 11, FAR_N - FAR_HEAD).astype(F)
    return p


def write_point_ply(path, xyz, rgb8, double=False, normals=False):
    """A binary_little_endian point PLY as structure from motion writes it: x y z (float or double), optionally nx ny nz, red
    green blue (uchar)."""
    n = xyz.shape[0]
    ft = "<f8" if double else "<f4"
    fields = [("x", ft), ("y", ft), ("z", ft)] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if normals else [])
    fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.zeros(n, np.dtype(fields))
    for a, k in enumerate("xyz"):
        v[k] = xyz[:, a]
    for a, k in enumerate(("red", "green", "blue")):
        v[k] = rgb8[:, a]
    if normals:
        v["nx"], v["ny"], v["nz"] = 0.0, 0.0, 1.0
    kinds = {"<f8": "double", "<f4": "float", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\ncomment a test cloud\n" + f"element vertex {n}\n" + \
        "".join(f"property {kinds[t]} {k}\n" for k, t in fields) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
