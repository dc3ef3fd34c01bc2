"""GPU tests of the point-cloud initialisation (include/splat.h, "Initialisation from a point cloud"; GaussianFit.from_points)
against the restatement of tests/knn_ref.py, with the sentinel-tail buffers of tests/test_gpu_density.py.

Bounds (none taken from the code under test):
  mean_sq      EXACT: the bits of the restatement, on every scene, size and stride.  The contract is a function of the input
               alone, every operator one rounding, and a skipped block provably cannot lower a third distance: there is nothing
               to tolerate.  Past 262 144 points (the far loop's and the box's second trip) the reference over every row is a
               brute force in torch on the device, itself held to the restatement's bits on 1024 rows or more of each cloud.
  evaluations  <= n / 4 per query: a condition that tells a search that prunes from one that does not (brute force performs
               n - 1 per query; a prototype with 10-bit Morton codes 27 207 on the cloud with eight outliers), not a measurement.
  from_points  log_scales within 1e-6 relative of 0.5 log(max(ref, 1e-7)) in float64: the binary32 sqrt and log each round to
               about 6e-8 of a value whose logarithm is of order 1 or more; everything else it sets is exact.
Every test prints the figures it asserts on.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import autograd as AG
from tests import ellipsoid_ref as ER
from tests import knn_ref as KR
from tests import test_gpu_density as TD

pytestmark = pytest.mark.gpu

_dev, _ptr, _host, SENT = TD._dev, TD._ptr, TD._host, TD.SENT
F = np.float32
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
EV_SENT = 0xDEADBEEF


def _cx(n):
    cx = AG._context(torch.empty(4, device="cuda"))
    cx.ensure_sorter(max(n, 1))
    return cx


def knn_gpu(points, stride=3, evaluations=True):
    """splat_knn_mean_sq on the device: (mean_sq (n,), evaluations or None).  stride 4: the fourth word of every point is a NaN
    sentinel.  The input and the sentinel tails are checked to be untouched."""
    p = np.ascontiguousarray(points, F)
    n = p.shape[0]
    if stride == 4:
        p = np.concatenate([p, np.full((n, 1), SENT, np.uint32).view(F)], axis=1)
    cx = _cx(n)
    P = _dev(p)
    out = _dev(np.full(max(n, 1), SENT, np.uint32))
    ev = _dev(np.full(2, EV_SENT, np.uint32))
    nbytes = int(cx.lib.splat_knn_workspace_bytes(n))
    ws = torch.empty(max(nbytes // 4, 4), device="cuda", dtype=torch.int32)
    rc = cx.lib.splat_knn_mean_sq(cx.ctx, cx.sorter, _ptr(P), stride, n, ws.data_ptr(), nbytes, _ptr(out), _ptr(ev) if evaluations else None)
    assert rc == 0, cx.lib.splat_last_error(cx.ctx)
    torch.cuda.synchronize()
    assert np.array_equal(_host(*P, np.uint32, p.shape), bits(p)), "the points were written"
    got = _host(*out, np.uint32, (max(n, 1),))
    assert (got[n:] == SENT).all()
    e = _host(*ev, np.uint32, (2,))
    if not evaluations or n == 0:
        assert (e == EV_SENT).all(), "evaluations was written"
        return got[:n].view(F), None
    return got[:n].view(F), int(e.view(np.uint64)[0])


def assert_exact(got, want, label):
    same = bits(got) == bits(want)
    bad = np.flatnonzero(~same)
    print(f"{label}: {got.shape[0]} rows, {bad.size} differ" + (f"; first {bad[:4]}: {got[bad[:4]]} != {want[bad[:4]]}" if bad.size else "") +
          f"; {int(np.isposinf(want).sum())} +inf rows, {int((want == 0).sum())} zero rows")
    assert bad.size == 0, f"{label}: {bad.size} rows differ from the restatement"


_REFS = {}


def scene_ref(name):
    if name not in _REFS:
        p = KR.scene(name)
        p.setflags(write=False)
        want = KR.mean_sq(p)
        want.setflags(write=False)
        _REFS[name] = (p, want)
    return _REFS[name]


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("name", KR.SCENES)
def test_exact_bits(device, name, stride):
    p, want = scene_ref(name)
    got, ev = knn_gpu(p, stride)
    n = p.shape[0]
    print(f"{name}: {ev / n:.1f} evaluations per query (brute force {n - 1})")
    assert_exact(got, want, f"{name} stride {stride}")
    if name == "duplicates":
        assert int((want.view(np.uint32) == 0).sum()) == 200, "the scene has 50 points in four copies: 200 exact zeros"
    if name == "identical":
        assert (want.view(np.uint32) == 0).all()
    if name == "nonfinite":
        assert np.isposinf(got[[41, 200]]).all() and np.isfinite(np.delete(got, [41, 200])).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025, 3840, 3841, 20011])
def test_sizes(device, n):
    p = KR.uniform(n, 1000 + n)
    want = KR.mean_sq(p)
    got, ev = knn_gpu(p, 3)
    print(f"n={n}: {ev} evaluations, {ev / n:.1f} per query")
    assert_exact(got, want, f"n={n}")
    if n < 4:
        assert np.isposinf(got).all()
    assert 0 < ev <= n * n, "a lane meets a candidate at most once (its own slot included)"


@pytest.mark.parametrize("name", ["cube", "outliers", "sphere"])
def test_pruning(device, name):
    n = 32768
    p = KR.pruning_scene(name, n)
    got, ev = knn_gpu(p, 3)
    rows = np.sort(np.random.default_rng(4).choice(n, 512, replace=False))
    if name == "outliers":
        rows[:8] = np.arange(8)  # (the outliers themselves among them)
        rows = np.unique(rows)
    want = KR.mean_sq(p, rows=rows)
    per_query = ev / n
    print(f"{name}: {per_query:.1f} evaluations per query; the cap is n / 4 = {n // 4}, brute force {n - 1}")
    assert_exact(got[rows], want, f"{name}, {rows.size} rows")
    assert np.isfinite(got).all()
    assert per_query <= n / 4


# ---- past 64 groups: the far loop's and the box's second trip ---------------------------------------------------------------------
# k_knn_search's far loop takes 64 groups (of 64 blocks of 64 points) per trip and k_knn_bbox's grid is capped at 1024 workgroups of
# 256: both make a second trip only above n = 262 144.  KR.mean_sq cannot serve every row there (about 6 s per 1024 rows on a CPU), so
# the reference over ALL rows is a brute force in torch on the device, which is itself held to KR.mean_sq's bits on PIN_ROWS rows of
# every cloud.  It shares nothing with the kernel: no sort, no boxes, no pruning.

PIN_ROWS = 1024
BRUTE_CHUNK = 512  # query rows per pass: three (512, n) float32 temporaries and topk's, under 2 GB at n = 300 000


def brute_force(points, dev="cuda"):
    """(distances (n, 3) float32 ascending, neighbours (n, 3) int64): the three nearest candidates of every row by the header's
    rule, each operator one eager float32 op (one rounding, no contraction): dx dx, dy dy, their sum, dz dz, the final sum;
    non-finite distances +inf, the query's own index out."""
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(points, F)[:, :3])).to(dev)
    n = p.shape[0]
    need = 5 * BRUTE_CHUNK * n * 4 + (64 << 20)
    free = torch.cuda.mem_get_info()[0] if dev == "cuda" else need
    if free < need:
        pytest.skip(f"the brute-force reference needs {need >> 20} MB of device memory, {free >> 20} MB are free")
    x, y, z = (p[:, a].contiguous() for a in range(3))
    dist = torch.empty((n, 3), device=dev, dtype=torch.float32)
    nbr = torch.empty((n, 3), device=dev, dtype=torch.int64)
    for s in range(0, n, BRUTE_CHUNK):
        e = min(s + BRUTE_CHUNK, n)
        dx, dy, dz = x[s:e, None] - x[None, :], y[s:e, None] - y[None, :], z[s:e, None] - z[None, :]
        dx.mul_(dx)   # dx dx
        dy.mul_(dy)   # dy dy
        dx.add_(dy)   # dx dx + dy dy
        dz.mul_(dz)   # dz dz
        dx.add_(dz)   # (dx dx + dy dy) + dz dz
        assert dx.dtype == torch.float32
        d = dx.nan_to_num_(nan=float("inf"), posinf=float("inf"), neginf=float("inf"))
        r = torch.arange(s, e, device=dev)
        d[r - s, r] = float("inf")  # j != i
        b, j = torch.topk(d, 3, dim=1, largest=False)
        b, o = torch.sort(b, dim=1)
        dist[s:e], nbr[s:e] = b, torch.gather(j, 1, o)
    return dist.cpu().numpy(), nbr.cpu().numpy()


def brute_mean_sq(dist):
    """The mean in NumPy, as KR.mean_sq forms it: the division never goes through a device kernel."""
    return ((dist[:, 0] + dist[:, 1]) + dist[:, 2]) / F(3.0)


def far_reference(points, label, regime_rows=()):
    """(mean_sq of every row, neighbours, order, codes, second-trip queries) of a cloud past 64 groups: the device brute force,
    pinned to KR.mean_sq on the rows a case is there for (every query that only the second far trip serves, and `regime_rows`),
    topped up with seeded random rows: at least 256 of those, and PIN_ROWS rows in all."""
    n = points.shape[0]
    dist, nbr = brute_force(points)
    want = brute_mean_sq(dist)
    order, codes = KR.morton_order(points)
    fin = np.flatnonzero(np.isfinite(want))
    second = fin[KR.second_far_trip(KR.block_of(order), fin, nbr[fin])]
    regime = np.unique(np.concatenate([second, np.asarray(regime_rows, np.int64)]))
    others = np.random.default_rng(41).choice(np.setdiff1d(np.arange(n), regime), max(PIN_ROWS - regime.size, 256), replace=False)
    rows = np.sort(np.concatenate([regime, others]))
    pin = KR.mean_sq(points, rows=rows, chunk=4)
    bad = np.flatnonzero(bits(want[rows]) != bits(pin))
    print(f"{label}: the device brute force against KR.mean_sq on {rows.size} rows ({regime.size} regime rows and {others.size} random ones): "
          f"{bad.size} differ; {second.size} queries served by the second far trip")
    assert np.unique(rows).size == rows.size >= PIN_ROWS and bad.size == 0, \
        f"{label}: the REFERENCE (torch brute force) differs from KR.mean_sq on {bad.size} rows, first {rows[bad[:4]]}: not the kernel"
    return want, nbr, order, codes, second


@pytest.mark.parametrize("n", [KR.FAR_HEAD, KR.FAR_HEAD + 1, KR.FAR_N])
def test_far_groups_uniform(device, n):
    """262 144 points are 64 groups and 1024 workgroups of k_knn_bbox: the last size with one trip of either loop.  262 145 is
    the boundary.  At 300 000 (4688 blocks, 74 groups) at least 1000 queries have a neighbour that only the second far trip
    can reach (KR.second_far_trip, from the reference's neighbours and the restated order): a far loop that stopped after 64
    groups would leave those rows too large.  Every row is compared."""
    p = KR.uniform(n, 21)
    want, _, order, _, second = far_reference(p, f"cube n={n}")
    groups = -(-(-(-n // KR.BLOCK)) // KR.GROUP)
    got, ev = knn_gpu(p, 3)
    print(f"cube n={n}: {groups} groups, {ev / n:.1f} evaluations per query (cap n / 4 = {n // 4})")
    assert groups == {KR.FAR_HEAD: 64, KR.FAR_HEAD + 1: 65, KR.FAR_N: 74}[n]
    if n == KR.FAR_N:
        assert second.size >= 1000, f"only {second.size} queries need the second far trip"
    assert_exact(got, want, f"cube n={n}")
    assert np.isfinite(got).all() and ev / n <= n / 4


def test_far_groups_non_finite_tail(device):
    """6000 points with a NaN, +inf or -inf coordinate sort to the end: the last blocks hold nobody, and a whole group of the
    second trip (index 64 or higher) is empty boxes.  Their rows are +inf, every other row is the reference's bits."""
    p, rows = KR.nonfinite_tail()
    want, _, order, _, _ = far_reference(p, "non-finite tail", regime_rows=rows[:256])
    block = KR.block_of(order)
    blocks = -(-p.shape[0] // KR.BLOCK)
    fin = np.isfinite(p).all(axis=1)
    assert np.array_equal(np.flatnonzero(~fin), rows)
    held = np.bincount(block[fin] // KR.GROUP, minlength=-(-blocks // KR.GROUP))
    empty = np.flatnonzero(held == 0)
    print(f"non-finite tail: the finite points end in block {int(block[fin].max())} of {blocks}; groups without a finite point: {empty}")
    assert empty.size >= 1 and empty.min() >= 64
    got, ev = knn_gpu(p, 3)
    print(f"non-finite tail: {ev / p.shape[0]:.1f} evaluations per query")
    assert np.isposinf(got[rows]).all() and np.isfinite(got[fin]).all()
    assert_exact(got, want, "non-finite tail")


def test_far_box_shifted_tail(device):
    """The rows from 262 144 on lie at x in [9, 11): the first trip of k_knn_bbox's grid-stride loop sees x < 1 only, the second
    brings the cloud's true extent.  The box feeds the codes, and the codes only order the visits: a wrong box cannot change
    mean_sq, it changes `evaluations`.  So the check is metamorphic: the same cloud with its rows reversed puts the shifted rows
    into the first trip.  With all codes distinct (asserted) the sorted array, the blocks and every wave's work are the same
    in both, and the counter is an integer sum: the two counts must be equal, and mean_sq equal under the permutation."""
    p = KR.shifted_tail()
    n = p.shape[0]
    want, _, _, codes, _ = far_reference(p, "shifted tail", regime_rows=np.arange(KR.FAR_HEAD, KR.FAR_HEAD + 256))
    assert np.unique(codes).size == n, "two points share a Morton code: the reversed cloud may sort its ties differently"
    assert p[:KR.FAR_HEAD, 0].max() < 1 and p[KR.FAR_HEAD:, 0].min() >= 9
    fwd, ev_fwd = knn_gpu(p, 3)
    rev, ev_rev = knn_gpu(np.ascontiguousarray(p[::-1]), 3)
    print(f"shifted tail: {ev_fwd / n:.1f} evaluations per query forward, {ev_rev / n:.1f} reversed (cap n / 4 = {n // 4})")
    assert_exact(fwd, want, "shifted tail, forward")
    assert_exact(rev[::-1], want, "shifted tail, reversed")
    assert np.array_equal(bits(rev[::-1]), bits(fwd))
    assert ev_fwd == ev_rev, f"evaluations {ev_fwd} forward and {ev_rev} reversed: the two clouds were not ordered alike"
    assert ev_fwd / n <= n / 4


def test_two_calls_give_the_same_bits(device):
    p = KR.scene("clusters")
    a, ea = knn_gpu(p, 3)
    b, eb = knn_gpu(p, 3)
    c, ec = knn_gpu(p, 4)
    print(f"evaluations {ea}, {eb}, {ec}")
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)) and ea == eb == ec
    d, none = knn_gpu(p, 3, evaluations=False)
    assert none is None and np.array_equal(bits(a), bits(d))


def test_rejections(device):
    n = 500
    p = KR.uniform(n, 31)
    cx = _cx(n)
    lib, ctx = cx.lib, cx.ctx
    P, out, ev = _dev(p), _dev(np.full(n, SENT, np.uint32)), _dev(np.full(2, EV_SENT, np.uint32))
    nbytes = int(lib.splat_knn_workspace_bytes(n))
    ws = torch.empty(nbytes // 4 + 8, device="cuda", dtype=torch.int32)
    good = dict(sorter=cx.sorter, points=_ptr(P), stride=3, n=n, ws=ws.data_ptr(), nbytes=nbytes, out=_ptr(out), ev=_ptr(ev))

    def call(**kw):
        a = dict(good, **kw)
        return lib.splat_knn_mean_sq(ctx, a["sorter"], a["points"], a["stride"], a["n"], a["ws"], a["nbytes"], a["out"], a["ev"])
    invalid = dict(null_points=dict(points=None), null_out=dict(out=None), null_workspace=dict(ws=None), null_sorter=dict(sorter=None),
                   misaligned_points=dict(points=_ptr(P) + 2), misaligned_out=dict(out=_ptr(out) + 2), misaligned_evaluations=dict(ev=_ptr(ev) + 4),
                   stride_2=dict(stride=2), stride_0=dict(stride=0), n_2_30=dict(n=1 << 30), small_workspace=dict(nbytes=nbytes - 1),
                   misaligned_workspace=dict(ws=ws.data_ptr() + 8))
    for label, kw in invalid.items():
        rc = call(**kw)
        print(f"{label}: {rc} {lib.splat_last_error(ctx).decode()[:90]!r}")
        assert rc == -1, label
    small = C.c_void_p()
    assert lib.splat_sort_create(ctx, 100, C.byref(small)) == 0
    cap = int(lib.splat_sort_capacity(small))
    big = KR.uniform(cap + 1, 32)
    B, bout = _dev(big), _dev(np.full(cap + 1, SENT, np.uint32))
    bbytes = int(lib.splat_knn_workspace_bytes(cap + 1))
    bws = torch.empty(bbytes // 4, device="cuda", dtype=torch.int32)
    rc = lib.splat_knn_mean_sq(ctx, small, _ptr(B), 3, cap + 1, bws.data_ptr(), bbytes, _ptr(bout), None)
    print(f"a sorter of capacity {cap} and n = {cap + 1}: {rc}")
    assert rc == -4
    assert lib.splat_knn_mean_sq(ctx, small, _ptr(B), 3, cap, bws.data_ptr(), bbytes, _ptr(bout), None) == 0  # (it fits)
    torch.cuda.synchronize()
    assert_exact(_host(*bout, np.uint32, (cap + 1,))[:cap].view(F), KR.mean_sq(big[:cap]), f"n = {cap} on the small sorter")
    lib.splat_sort_destroy(small)
    # n = 0: success, and nothing is written, with or without pointers
    assert call(n=0) == 0 and call(n=0, points=None, out=None, ws=None, nbytes=0, sorter=None) == 0
    torch.cuda.synchronize()
    assert (_host(*out, np.uint32, (n,)) == SENT).all() and (_host(*ev, np.uint32, (2,)) == EV_SENT).all(), "a refused or empty call wrote"
    got, _ = knn_gpu(np.zeros((0, 3), F))
    assert got.shape == (0,)
    # the Python entry point refuses what is not a CUDA float32 (n, 3) or (n, 4) tensor
    for bad in (torch.zeros(5, 3), torch.zeros(5, 2, device="cuda"), torch.zeros(5, 3, device="cuda", dtype=torch.float64), np.zeros((5, 3), F)):
        with pytest.raises(sr.SplatError):
            sr.knn_mean_sq_distance(bad)
    assert sr.knn_mean_sq_distance(torch.zeros(0, 3, device="cuda")).shape == (0,)


def test_python_entry_point(device):
    p, want = scene_ref("uniform")
    t = torch.from_numpy(np.array(p)).cuda()
    assert_exact(sr.knn_mean_sq_distance(t).cpu().numpy(), want, "knn_mean_sq_distance (n, 3)")
    t4 = torch.cat([t, torch.full((t.shape[0], 1), float("nan"), device="cuda")], dim=1)
    got, ev = sr.knn_mean_sq_distance(t4, return_evaluations=True)
    assert_exact(got.cpu().numpy(), want, "knn_mean_sq_distance (n, 4)")
    assert 0 < int(ev) <= p.shape[0] * (p.shape[0] - 1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (torch's current stream: another context and sorter)
        other = sr.knn_mean_sq_distance(t)
    side.synchronize()
    assert_exact(other.cpu().numpy(), want, "on a side stream")


def test_from_points(device, tmp_path):
    """A fit started from a point PLY: 2 000 points of test_fitting_converges' target cloud, jittered, with colours."""
    n, w, h = 2000, 256, 256
    u = TD.camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, 31, 1.0, 0.04, degenerate=False)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, F), device="cuda")  # noqa: E731
    with torch.no_grad():
        target, _ = AG.render_gaussians(u, t(pos[:, :3]), t(scl[:, :3]), t(rot), t(col[:, 3]).clamp(0.05, 0.95), colors=t(col[:, :3]).clamp(0.05, 0.95),
                                        width=w, height=h)
        target = target.clone()
    rng = np.random.default_rng(6)
    xyz = (pos[:, :3] + rng.normal(0, 0.01, (n, 3))).astype(F)
    rgb8 = np.round(np.clip(col[:, :3], 0.05, 0.95) * 255).astype(np.uint8)
    path = str(tmp_path / "points3D.ply")
    KR.write_point_ply(path, xyz, rgb8, normals=True)
    lxyz, lrgb = sr.load_point_ply(path)
    assert np.array_equal(lxyz, xyz)
    fit = sr.GaussianFit.from_points(lxyz, lrgb)
    ref = KR.mean_sq(xyz).astype(np.float64)
    want = 0.5 * np.log(np.maximum(ref, 1e-7))
    ls = fit.log_scales.detach().cpu().numpy().astype(np.float64)
    rel = float((np.abs(ls - want[:, None]) / np.abs(want[:, None])).max())
    print(f"log_scales: max relative error {rel:.3g} (bound 1e-6); |log scale| from {np.abs(want).min():.3g} to {np.abs(want).max():.3g}")
    assert fit.n == n and fit.degree == 3 and rel <= 1e-6
    sh = fit.sh.detach().cpu().numpy().reshape(n, 16, 3)
    dc = (lrgb.astype(np.float64) - 0.5) / 0.28209479177387814  # (formed in float64 and rounded once: at most the one ulp of a double rounding)
    print(f"SH DC: max |fit - formula| {np.abs(sh[:, 0] - dc).max():.3g}")
    assert (np.abs(sh[:, 0] - dc) <= TD.ulp32(dc)).all() and not sh[:, 1:].any()
    assert np.array_equal(fit.rotations.detach().cpu().numpy(), np.tile(np.array([1, 0, 0, 0], F), (n, 1)))
    op = torch.sigmoid(fit.opacity_logits.detach().double()).cpu().numpy()
    assert np.abs(op - 0.1).max() <= 1e-7, "the opacity is 0.1"
    assert np.array_equal(fit.means.detach().cpu().numpy(), xyz)
    losses = []
    for step in range(100):
        rgb, _ = fit.render(u, w, h)
        if step == 0:
            assert bool(torch.isfinite(rgb).all()), "the first frame is not finite"
        loss = AG.photometric_loss(rgb, target)
        loss.backward()
        fit.step()
        losses.append(float(loss.detach()))
    print(f"from_points fit: loss {losses[0]:.4g} -> {losses[-1]:.4g} after 100 steps (ratio {losses[0] / losses[-1]:.2f})")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert all(bool(torch.isfinite(q).all()) for q in fit.parameters())


def test_from_points_floor_and_refusals(device):
    p = KR.uniform(200, 33)
    p[1:4] = p[0] + np.array([[5e-5, 0, 0], [0, 5e-5, 0], [0, 0, 5e-5]], F)  # four points within 1e-4: mean_sq ~ 5e-9 < 1e-7
    p[11] = p[10] + F(1e-4)  # two points closer than sqrt(1e-7), whose other neighbours are far: no floor
    ref = KR.mean_sq(p).astype(np.float64)
    assert (ref[:4] < 1e-7).all() and ref[10] > 1e-7 and np.sqrt(((p[10] - p[11]).astype(np.float64) ** 2).sum()) < np.sqrt(1e-7)
    rgb = np.random.default_rng(34).uniform(0, 1, (200, 3)).astype(F)
    fit = sr.GaussianFit.from_points(p, rgb, degree=0)
    ls = fit.log_scales.detach().cpu().numpy().astype(np.float64)
    want = 0.5 * np.log(np.maximum(ref, 1e-7))
    rel = float((np.abs(ls - want[:, None]) / np.abs(want[:, None])).max())
    print(f"floored rows: log scale {ls[:4, 0]} (0.5 log 1e-7 = {0.5 * np.log(1e-7):.7g}); max relative error {rel:.3g}")
    assert rel <= 1e-6 and np.abs(ls[:4] - 0.5 * np.log(1e-7)).max() <= 1e-6 * 8.06 and (ls[4:] > 0.5 * np.log(1e-7)).all()
    assert fit.degree == 0 and fit.sh.shape == (200, 3)
    other = sr.GaussianFit.from_points(p, rgb, degree=0, min_sq_distance=1e-3, opacity=0.3)
    assert float(other.log_scales.detach().min()) >= 0.5 * np.log(1e-3) - 1e-5
    for bad, why in ((p[:3], "three points"), (np.concatenate([p[:50], np.array([[np.nan, 0, 0]], F)]), "a NaN coordinate")):
        with pytest.raises(sr.SplatError) as ei:
            sr.GaussianFit.from_points(bad, rgb[:bad.shape[0]], degree=0)
        print(f"{why}: {ei.value}")
