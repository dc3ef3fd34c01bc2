"""MCMC relocation without a GPU: the restatement of tests/mcmc_ref.py against 60-digit arithmetic and against the law of its
draws, and the new entry points' place in the header, the library, the Python binding and the N-API shim."""
import ctypes as C
import decimal
import os
import re

import numpy as np
import pytest

from tests import mcmc_ref as MR
from tests.test_abi_cpu import ROOT, declared_functions

ENTRIES = ["splat_mcmc_apply", "splat_mcmc_noise", "splat_mcmc_sample", "splat_mcmc_sample_workspace_bytes"]


def test_one_copy_is_the_identity():
    for o in (0.005, 0.1, 0.5, 0.9, 1 - 1e-7):
        on, D = MR.relocation(o, 1)
        assert D == on and abs(on - o) <= 1e-12 * o, (o, on, D)  # (1 - (1 - o) is o to a rounding of 1 - o; the sum is its one term)
        if o > MR.OPACITY_MAX:  # (the new logit is the clamp's)
            continue
        logit = np.float32(np.log(o) - np.log1p(-o))
        nl, lr = MR.new_values(logit, 0, 0.0)
        assert abs(nl - float(logit)) <= 1e-9 * max(1.0, abs(float(logit))) and abs(lr) <= 1e-12  # the coefficient o / D is 1


def relocation_decimal(o, N):
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        o = D(o)
        on = 1 - ((1 - o).ln() / N).exp()
        total = D(0)
        for a in range(1, N + 1):
            for k in range(a):
                total += D(MR.BINOM[a - 1][k]) * (-1) ** k * on ** (k + 1) / D(k + 1).sqrt()
        return on, total


def test_relocation_against_sixty_digits():
    worst = 0.0
    for o in (0.005, 0.01, 0.1, 0.5, 0.9, 0.99, 0.999, 1 - 1e-7):
        for N in (1, 2, 3, 5, 10, 20, 35, 51):
            on, D = MR.relocation(o, N)
            ron, rD = relocation_decimal(o, N)  # (of the same binary64 o)
            e = max(abs(float((decimal.Decimal(on) - ron) / ron)), abs(float((decimal.Decimal(D) - rD) / rD)))
            worst = max(worst, e)
            assert e <= 1e-11, f"o={o} N={N}: relative {e:.3g}"
    print(f"relocation against 60 digits: worst relative {worst:.3g}")


def test_draw_frequencies():
    """200 000 draws over 64 weights: every source's frequency within 5 standard deviations of q_i / T."""
    rng = np.random.default_rng(5)
    logits = rng.normal(-1.0, 2.5, 64).astype(np.float32)
    draws = 200_000
    targets, sources, counts, words = MR.sample(logits, MR.ADD, draws, 0x1234_5678_9ABC_DEF0, 0.005)
    _, dead, w = MR.weights(logits, 0.005)
    assert dead.any() and not dead.all() and words == (int(dead.sum()), int((~dead).sum()), draws)
    assert np.array_equal(targets, 64 + np.arange(draws)) and int(counts.sum()) == draws
    assert np.array_equal(counts, np.bincount(sources, minlength=64))
    p = w / w.sum()
    sd = np.sqrt(draws * p * (1 - p))
    z = np.abs(counts - draws * p) / np.where(sd > 0, sd, 1)
    print(f"draw frequencies: worst deviation {z.max():.2f} standard deviations")
    assert (z <= 5).all() and not counts[dead].any()


def test_sample_edges():
    logits = np.array([np.nan, -np.inf, np.inf, 0.0, -20.0], np.float32)
    q, dead, w = MR.weights(logits, 0.005)
    assert q.tolist() == [0, 0, 2 ** 24, 2 ** 23, 0] and dead.tolist() == [True, True, False, False, True]
    targets, sources, counts, words = MR.sample(logits, MR.RELOCATE, 0, 3, 0.005)
    assert targets.tolist() == [0, 1, 4] and words == (3, 2, 3) and set(sources.tolist()) <= {2, 3}
    _, _, counts, words = MR.sample(np.full(7, -30.0, np.float32), MR.RELOCATE, 0, 3, 0.005)  # nobody alive
    assert words == (7, 0, 0) and not counts.any()


@pytest.mark.parametrize("name", MR.FAR_CASES)
def test_clouds_past_256_block_sums_reach_their_trips(name):
    """What tests/test_gpu_mcmc.py's clouds above 524 288 splats are there for, from the restatement alone: the trip counts of the
    block sums' scan, a first trip that sums past 2^32, at least 1000 of 5000 added draws with a source past the first trip (from
    n = 1 229 577 on), zero totals where a case wants them, every source in the alive range, and every input's 2^24 o at least 1e-6
    from an integer (MR.off_integers moved the few that were not)."""
    logits, alive = MR.far_case(name)
    n = len(logits)
    x = MR.scaled_opacity(logits)
    assert float(np.abs(x - np.round(x)).min()) >= 1e-6
    if name.startswith("n="):
        raw = MR.normal_logits(n, 100 + n)
        moved = np.flatnonzero(raw != logits)
        print(f"{name}: {moved.size} logits moved off an integer: rows {moved}")
        assert moved.size <= 8 and np.array_equal(logits[moved], np.nextafter(raw[moved], np.float32(np.inf)))
    targets, sources, counts, words = MR.sample(logits, MR.ADD, 5000, 0xC0FFEE_0000_0002, 0.005)
    first, total, past = MR.far_case_regime(name, logits, alive, sources, 0.005)
    print(f"{name}: n = {n}; weight up to the end of the first trip {first}, total {total}; {past} of 5000 draws past the first trip")
    assert words[2] == 5000 and int(counts.sum()) == 5000 and np.array_equal(targets, n + np.arange(5000))


def test_header_declares_the_entries_and_keeps_the_abi():
    names = declared_functions()
    assert all(n in names for n in ENTRIES)
    text = open(os.path.join(ROOT, "include", "splat.h")).read()
    assert re.search(r"#define SPLAT_ABI_VERSION 3\b", text)
    assert text.index("Density control and optimiser") < text.index("MCMC relocation")


def test_library_exports_the_entries():
    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    probe = C.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    if probe is None or not all(hasattr(probe, n) for n in ENTRIES):
        g.build()
        probe = C.CDLL(_lib.LIB_PATH)
    assert [n for n in ENTRIES if not hasattr(probe, n)] == []
    lib = _lib.load()
    assert lib.splat_abi_version() == 3
    for n in (0, 1, 2049, 5_000_000):  # three uint32 planes, the uint64 scan, its block sums
        assert lib.splat_mcmc_sample_workspace_bytes(n) >= 3 * 4 * n + 8 * n + 8 * ((n + 2047) // 2048)


def test_binding_and_addon_cover_the_entries():
    from splat_renderer_amd import _lib
    assert all(n in _lib.SIGNATURES for n in ENTRIES)
    assert (_lib.MCMC_RELOCATE, _lib.MCMC_ADD) == (MR.RELOCATE, MR.ADD)
    assert C.sizeof(_lib.McmcPlanes) == 15 * 8 + 8
    src = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    exported = set(re.findall(r"EXPORT\(([a-z0-9_]+)\)", src.split("napi_property_descriptor d[]")[1]))
    assert {n[len("splat_"):] for n in ENTRIES} <= exported
    from splat_renderer_amd.fit import GaussianFit
    for name in ("relocate", "add_new", "inject_noise", "regularizer"):
        assert callable(getattr(GaussianFit, name))
