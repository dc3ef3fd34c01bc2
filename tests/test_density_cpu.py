"""The restatement of density control (tests/density_ref.py) held to the rules of include/splat.h, "Density control and
optimiser", on the CPU: Philox's known answers, the plan's invariants on seeded clouds (the restatement asserts of its own
inputs that every class is populated), the distribution of split children, save_gaussian_ply as the inverse of
load_gaussian_ply, and the new entry points in the header, the binding and the addon."""
import os
import re

import numpy as np
import pytest

from tests import density_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("splat_adam_step", "splat_density_accumulate", "splat_densify_plan_workspace_bytes", "splat_densify_plan",
                    "splat_densify_geometry", "splat_densify_rows")


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
], ids=["zeros", "ones", "pi_digits"])
def test_philox_known_answers(counter, key, want):
    got = DR.philox4x32_10(np.array(counter, np.uint32), np.array(key, np.uint32))
    assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]


def plan_inputs(n, seed):
    """A seeded cloud's plan inputs whose four classes (under THRESHOLDS) each hold at least 5 % of n."""
    rng = np.random.default_rng(seed)
    log_scales = rng.normal(np.log(0.03), 0.7, (n, 3)).astype(np.float32)
    logits = rng.normal(0.0, 3.0, n).astype(np.float32)
    denom = rng.integers(0, 5, n).astype(np.float32)
    grad_accum = (denom * np.exp(rng.normal(np.log(2e-4), 1.0, n))).astype(np.float32)
    max_radius = np.exp(rng.normal(np.log(8.0), 0.8, n)).astype(np.float32)
    return log_scales, logits, grad_accum, denom, max_radius


THRESHOLDS = dict(grad_threshold=2e-4, scale_threshold=0.06, min_opacity=0.1)


@pytest.mark.parametrize("n, seed", [(1000, 1), (5000, 2), (20011, 3)])
def test_plan_invariants(n, seed):
    inp = plan_inputs(n, seed)
    rows, counts, refused = DR.plan(*inp, **THRESHOLDS)
    for k in ("pruned", "kept", "cloned", "split"):
        assert counts[k] >= 0.05 * n, (k, counts)
    assert sum(counts.values()) == n and refused.size == 0
    assert rows.shape[0] == counts["kept"] + 2 * counts["cloned"] + 2 * counts["split"]
    parent, kind = (rows & DR.PARENT_MASK).astype(np.int64), rows >> 30
    assert (np.diff(parent) >= 0).all(), "rows are in parent order"
    g, s, o = DR.plan_quantities(*inp[:4])
    dead = ~(o >= THRESHOLDS["min_opacity"])
    assert not dead[parent].any(), "a dead splat has rows"
    assert set(np.unique(parent)) == set(np.nonzero(~dead)[0])
    # the kinds of a parent: {0}, (0, 1) in that order, (2, 3) in that order
    first = np.r_[True, np.diff(parent) != 0]
    starts = np.nonzero(first)[0]
    for a, b in zip(starts, np.r_[starts[1:], parent.size]):
        assert tuple(int(k) for k in kind[a:b]) in ((0,), (0, 1), (2, 3)), (int(parent[a]), kind[a:b])
    split_parents = parent[kind == 2]
    assert (s[split_parents] > THRESHOLDS["scale_threshold"]).all() and (g[split_parents] >= THRESHOLDS["grad_threshold"]).all()
    clone_parents = parent[kind == 1]
    assert (s[clone_parents] <= THRESHOLDS["scale_threshold"]).all() and (g[clone_parents] >= THRESHOLDS["grad_threshold"]).all()

    survivors = n - counts["pruned"]
    wanted = counts["cloned"] + counts["split"]
    order = np.sort(np.r_[split_parents, clone_parents])  # the splats that wanted more, in index order
    for cap in (survivors + wanted + 10, survivors + wanted, survivors + wanted // 2, survivors + 1, survivors, survivors - 7, 1):
        rows_c, counts_c, refused_c = DR.plan(*inp, **THRESHOLDS, max_splats=cap)
        total = rows_c.shape[0]
        assert total == counts_c["kept"] + 2 * counts_c["cloned"] + 2 * counts_c["split"]
        assert counts_c["pruned"] == counts["pruned"]
        if survivors <= cap:
            assert total <= cap and total == min(cap, survivors + wanted)
        else:
            assert total == survivors
        assert np.array_equal(refused_c, order[order.size - refused_c.size:]), "refusals are a suffix of the splats that wanted more"
        assert refused_c.size == wanted - (counts_c["cloned"] + counts_c["split"])
        assert not dead[(rows_c & DR.PARENT_MASK).astype(np.int64)].any()


def test_plan_nan_falls_on_the_safe_side():
    n = 64
    ls, lo, ga, dn, mr = plan_inputs(n, 7)
    lo[:] = 2.0
    ls[:] = np.log(0.01)
    dn[:] = 1
    ga[:] = 1.0                        # everyone alive, small, and wants more: clones
    lo[3] = np.nan                     # NaN opacity: dead
    ls[5, 1] = np.nan                  # NaN scale: not split; dead only where max_world_scale is on
    ga[7] = np.nan                     # NaN statistic: kept, never densified
    rows, counts, _ = DR.plan(ls, lo, ga, dn, mr, **THRESHOLDS)
    kinds = {int(p): sorted(int(k) for k in (rows >> 30)[(rows & DR.PARENT_MASK) == p]) for p in (3, 5, 7, 9)}
    assert kinds == {3: [], 5: [0, 1], 7: [0], 9: [0, 1]}, kinds
    assert counts == dict(pruned=1, kept=1, cloned=n - 2, split=0)
    rows, counts, _ = DR.plan(ls, lo, ga, dn, mr, **THRESHOLDS, max_world_scale=1.0)
    assert not ((rows & DR.PARENT_MASK) == 5).any() and counts["pruned"] == 2
    dn[11] = 0                         # never seen: g = 0, whatever grad_accum holds
    ga[11] = np.inf
    rows, _, _ = DR.plan(ls, lo, ga, dn, mr, **THRESHOLDS)
    assert ((rows & DR.PARENT_MASK) == 11).sum() == 1


def test_split_children_are_standard_normal_when_whitened():
    n = 100_000                        # two children each: 200 000
    rng = np.random.default_rng(11)
    means = rng.normal(size=(n, 3))
    log_scales = rng.normal(np.log(0.05), 0.5, (n, 3))
    rot = rng.normal(size=(n, 4))
    parents = np.arange(n, dtype=np.uint32)
    rows = np.stack([parents | np.uint32(2 << 30), parents | np.uint32(3 << 30)], axis=1).reshape(-1)
    mu, ls = DR.apply_geometry(rows, means, log_scales, rot, seed=0x1234_5678_9ABC)
    assert np.allclose(ls, np.repeat(log_scales, 2, axis=0) - np.log(1.6), rtol=0, atol=1e-15)
    R = DR.rotation_matrices(np.repeat(rot, 2, axis=0))
    white = np.einsum("nji,nj->ni", R, mu - np.repeat(means, 2, axis=0)) / np.exp(np.repeat(log_scales, 2, axis=0))
    N = white.shape[0]
    assert N >= 200_000
    mean, var = white.mean(axis=0), white.var(axis=0)
    print(f"whitened children: mean {mean}, variance {var} over {N}")
    assert (np.abs(mean) <= 5.0 / np.sqrt(N)).all(), mean
    assert (np.abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / N)).all(), var
    assert np.abs(white).max() < 6.8
    # the two children of a parent differ; the same seed repeats; another seed does not
    assert not np.allclose(mu[0::2], mu[1::2])
    assert np.array_equal(DR.apply_geometry(rows[:100], means, log_scales, rot, seed=0x1234_5678_9ABC)[0], mu[:100])
    assert not np.allclose(DR.apply_geometry(rows[:100], means, log_scales, rot, seed=5)[0], mu[:100])


def test_apply_rows():
    rows = np.array([0, 2, 2 | (1 << 30), 5 | (2 << 30), 5 | (3 << 30)], np.uint32)
    plane = np.arange(24, dtype=np.float32).reshape(6, 4) + 1
    assert np.array_equal(DR.apply_rows(rows, plane), plane[[0, 2, 2, 5, 5]])
    z = DR.apply_rows(rows, plane, zero_new=True)
    assert np.array_equal(z[:2], plane[[0, 2]]) and not z[2:].any()


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_save_ply_round_trips(tmp_path, degree):
    from splat_renderer_amd.ply import load_gaussian_ply, save_gaussian_ply
    rng = np.random.default_rng(20 + degree)
    n, K = 300, (degree + 1) ** 2
    pos = rng.normal(size=(n, 3)).astype(np.float32)
    scl = np.exp(rng.normal(-3, 1.5, (n, 3))).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    op = rng.uniform(0.001, 0.999, n).astype(np.float32)
    sh = rng.normal(size=(n, K, 3)).astype(np.float32)
    path = str(tmp_path / "cloud.ply")
    save_gaussian_ply(path, pos, scl, rot, op, sh)
    g = load_gaussian_ply(path)
    assert g["degree"] == degree
    for key, a in (("positions", pos), ("rotations", rot), ("sh", sh)):
        assert np.array_equal(g[key].view(np.uint32), a.view(np.uint32)), key
    # the stored value is the float32 nearest the float64 log / logit; what comes back is within 1 ulp of its exp / sigmoid
    stored_ls = np.log(scl.astype(np.float64)).astype(np.float32)
    o64 = op.astype(np.float64)
    stored_lo = (np.log(o64) - np.log1p(-o64)).astype(np.float32)
    want_s, want_o = np.exp(stored_ls.astype(np.float64)), 1.0 / (1.0 + np.exp(-stored_lo.astype(np.float64)))
    assert (np.abs(g["scales"] - want_s) <= ulp32(want_s)).all()
    assert (np.abs(g["opacity"] - want_o) <= ulp32(want_o)).all()
    # 3DGS's property order, zero normals, channel-major f_rest
    header = open(path, "rb").read().split(b"end_header\n")[0].decode()
    names = re.findall(r"property float (\S+)", header)
    assert names == (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{j}" for j in range(3 * (K - 1))]
                     + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    raw = np.frombuffer(open(path, "rb").read().split(b"end_header\n", 1)[1], "<f4").reshape(n, len(names))
    assert not raw[:, 3:6].any()
    if K > 1:
        assert np.array_equal(raw[:, 9], sh[:, 1, 0]) and np.array_equal(raw[:, 9 + (K - 1)], sh[:, 1, 1])
    # raw parameters are stored as they are
    save_gaussian_ply(path, pos, None, rot, None, sh.reshape(n, -1), log_scales=stored_ls, opacity_logits=stored_lo)
    raw2 = np.frombuffer(open(path, "rb").read().split(b"end_header\n", 1)[1], "<f4").reshape(n, len(names))
    assert np.array_equal(raw2.view(np.uint32), raw.view(np.uint32))


def test_new_entry_points_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "splat.h")).read()
    assert re.search(r"#define SPLAT_ABI_VERSION 3\b", header), "the ABI version stays 3: entry points were only added"
    from splat_renderer_amd import _lib
    napi = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert "EXPORT(%s)" % name[len("splat_"):] in napi, name
    lib = _lib.load()
    assert lib.splat_abi_version() == 3
    import splat_renderer_amd as sr
    assert hasattr(sr, "GaussianFit") and hasattr(sr, "save_gaussian_ply")
