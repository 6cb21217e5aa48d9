"""Host tests of the MAP-Elites oracle (fiber_amd/es/map_elites_oracle.py), of
the shared cases of tests/map_elites_cases.py and of the validation that
MapElitesConfig and the ops wrappers do before any launch.  No GPU."""

import numpy as np
import pytest

import map_elites_cases as C
from fiber_amd import ops
from fiber_amd.es import MapElitesConfig, MapElitesEngine
from fiber_amd.es import ga_oracle as go
from fiber_amd.es import map_elites_oracle as mo
from fiber_amd.es import philox_ref

SMALL_CASES = [c for c in C.insert_cases() if mo.n_cells(c["bins"]) <= 64]


# ---- cells_exact ---------------------------------------------------------------

@pytest.mark.parametrize("case", C.insert_cases(),
                         ids=[c["name"] for c in C.insert_cases()])
def test_cells_exact_against_the_scalar_loop(case):
    bins, lo, hi = case["bins"], case["lo"], case["hi"]
    inv = mo.grid_inv(bins, lo, hi)
    assert inv.dtype == np.float32
    got = mo.cells_exact(case["bc"], lo, inv, bins, case["fitness"])
    want = C.cells_brute(case["bc"], lo, inv, bins, case["fitness"])
    assert got.dtype == np.int32
    assert np.array_equal(got, want)
    assert got.max() < mo.n_cells(bins) and got.min() >= -1


@pytest.mark.parametrize("bins", [(4, 4, 1, 1), (3, 5, 2, 2)])
def test_the_bc_inputs_hold_what_they_name(bins):
    bc = C.insert_bc(1000, bins)
    lo, hi = C.grid_bounds(bins)
    inv = mo.grid_inv(bins, lo, hi)
    for d in range(4):
        col = bc[:, d]
        for e in C.edge_values(bins, d):
            assert (col == e).any()
            assert (col == np.nextafter(e, np.float32(-np.inf))).any()
            assert (col == np.nextafter(e, np.float32(np.inf))).any()
        assert (col == np.inf).any() and (col == -np.inf).any()
        assert ((col == 0) & np.signbit(col)).any()          # -0.0
        assert (col < lo[d]).any() and (col > hi[d]).any()
        assert np.isnan(col).any()
    assert (np.isnan(bc).sum(axis=1) <= 1).all()
    # on the exact dimensions an edge gives an integer t: the bin above it
    edges = C.edge_values(bins, 0)
    t = (edges - np.float32(lo[0])) * inv[0]
    assert np.array_equal(t, np.arange(1, bins[0], dtype=np.float32))
    rows = np.zeros((edges.size, 4), dtype=np.float32)
    rows[:, 0] = edges
    rows[:, 1:] = np.float32([lo[1], lo[2], lo[3]])
    stride = bins[1] * bins[2] * bins[3]
    cells = mo.cells_exact(rows, lo, inv, bins)
    assert np.array_equal(cells // stride, np.arange(1, bins[0]))
    # the float32 below an edge may round back onto it in bc - lo (an ulp
    # of bc can be half an ulp of the difference): either bin, never a third
    rows[:, 0] = np.nextafter(edges, np.float32(-np.inf))
    off = mo.cells_exact(rows, lo, inv, bins) // stride - np.arange(
        1, bins[0])
    assert ((off == 0) | (off == -1)).all() and (off == -1).any()


def test_cells_exact_clamps_and_refuses_nans():
    bins, lo, hi = (4, 4, 1, 1), (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)
    inv = mo.grid_inv(bins, lo, hi)
    bc = np.float32([[-5, 0.5, 0, 0], [5, 0.5, 0, 0], [np.inf, -np.inf, 9, 9],
                     [0.5, np.nan, 0, 0], [-0.0, 0.99999, 0, 0]])
    f = np.float32([1, 1, 1, 1, 1])
    assert mo.cells_exact(bc, lo, inv, bins, f).tolist() == [2, 14, 12, -1, 3]
    f = np.float32([1, np.nan, 1, 1, 1])
    assert mo.cells_exact(bc, lo, inv, bins, f).tolist() == [2, -1, 12, -1, 3]


# ---- insert_exact ------------------------------------------------------------------

@pytest.mark.parametrize("case", SMALL_CASES,
                         ids=[c["name"] for c in SMALL_CASES])
def test_insert_exact_against_the_double_loop(case):
    want = C.insert_expected(case)
    brute = C.insert_brute(case["arch_fitness"], case["arch_filled"],
                           case["fitness"], want["cell"])
    assert np.array_equal(want["winner"], brute)
    won = want["winner"] >= 0
    # a filled cell never empties, its fitness never falls
    assert (want["arch_filled"] >= (case["arch_filled"] != 0)).all()
    was = case["arch_filled"] != 0
    assert (want["arch_fitness"][was] >= case["arch_fitness"][was]).all()
    assert np.array_equal(want["arch_filled"] != 0, was | won)
    assert (want["order"][:-1][~won]
            == case["fitness"].size + np.flatnonzero(~won)).all()


def test_the_named_insert_cases_do_what_they_name():
    cases = {c["name"]: c for c in C.insert_cases()}
    equal = C.insert_expected(cases["occupant-equal"])
    assert (equal["winner"] == -1).all()
    zero = C.insert_expected(cases["occupant-other-zero"])
    assert (zero["winner"] == -1).all()
    assert np.signbit(zero["arch_fitness"][zero["arch_fitness"] == 0]).all()
    below = C.insert_expected(cases["occupant-one-ulp-below"])
    assert (below["winner"] >= 0).all()
    # the best child appears twice: the lower index wins
    assert 3 in below["winner"].tolist() or 17 in below["winner"].tolist()
    f = cases["occupant-one-ulp-below"]["fitness"]
    for c, m in enumerate(below["winner"]):
        same = np.flatnonzero((below["cell"] == below["cell"][m])
                              & (f == f[m]))
        assert m == same.min()
    ties = C.insert_expected(cases["ties1000-2x2-empty"])
    assert (ties["winner"] >= 0).all()
    assert np.bincount(ties["cell"][ties["cell"] >= 0]).min() > 100
    special = C.insert_expected(cases["special-1x1x1x1-empty"])
    assert special["winner"].tolist() == [2]          # the first +inf


# ---- compact_exact --------------------------------------------------------------------

@pytest.mark.parametrize("pattern", C.COMPACT_PATTERNS)
def test_compact_exact(pattern):
    for size in C.COMPACT_SIZES[:-1]:
        flags = C.compact_flags(size, pattern)
        idx, n = mo.compact_exact(flags)
        want = [c for c in range(size) if flags[c]]
        assert n == len(want) and idx[:n].tolist() == want
        assert (idx[n:] == -1).all() and idx.shape == (size,)
    assert mo.compact_exact(C.compact_flags(65, "random"))[1] not in (0, 65)


# ---- parents_exact ---------------------------------------------------------------------

@pytest.mark.parametrize("pop,n", C.PARENT_CASES)
def test_parents_exact_against_a_scalar_philox_loop(pop, n):
    idx, _padded = C.parent_filled(n)
    root = 3 * n + 5
    pidx, slot = mo.parents_exact(C.PARENT_SEED, C.PARENT_GEN, pop, idx, root)
    assert pidx.dtype == slot.dtype == np.int32
    assert slot.tolist() == list(range(pop))
    for m in range(0, pop, max(1, pop // 50)):
        if n == 0:
            assert pidx[m] == root
            continue
        u = int(philox_ref.philox4x32_10(
            np.uint32(C.PARENT_SEED), np.uint32(C.PARENT_GEN), np.uint32(m),
            np.uint32(0), np.uint32(0x45530005), np.uint32(0))[0])
        assert pidx[m] == idx[(u * n) >> 32]
    if n > 1:
        assert np.unique(pidx).size > 1
    # another tag than the GA's parent draw
    if n == 1000:
        ga, _ = go.parents_exact(C.PARENT_SEED, C.PARENT_GEN, pop, 0, n)
        assert not np.array_equal(idx[ga], pidx)


# ---- config and wrapper validation -----------------------------------------------------------

def test_config_validation():
    cfg = MapElitesConfig(pop=16, bins=[4, 4, 1, 1])
    assert cfg.bins == (4, 4, 1, 1) and cfg.cells == 16
    assert cfg.bc_lo is None and cfg.bc_hi is None
    for bad in (dict(pop=0), dict(pop=65537), dict(bins=(4, 4, 1)),
                dict(bins=(4, 0, 1, 1)), dict(bins=(4, 2.5, 1, 1)),
                dict(bins=(256, 256, 1, 1)), dict(bins=(65535, 1, 1, 1)),
                dict(bc_lo=(0, 0, 0, 0)), dict(bc_hi=(1, 1, 1, 1)),
                dict(bc_lo=(0, 0, 0, 0), bc_hi=(1, 1, 0, 1)),
                dict(bc_lo=(0, 0, 0, 0), bc_hi=(1, 1, 1)),
                dict(bc_lo=(0, 0, 0, 0), bc_hi=(1, 1, float("inf"), 1)),
                dict(bc_lo=(0, float("nan"), 0, 0), bc_hi=(1, 1, 1, 1)),
                dict(horizon=0), dict(sigma=-0.1), dict(sigma=float("nan")),
                dict(sigma=float("inf"))):
        with pytest.raises(ValueError):
            MapElitesConfig(**bad)
    assert MapElitesConfig(bins=(65534, 1, 1, 1)).cells == ops.ME_CELLS_MAX
    with pytest.raises(NotImplementedError):
        MapElitesEngine(MapElitesConfig(), ctx=object())


def test_me_grid_rounds_the_scale_once_from_double():
    bins, lo32, inv32, cells = ops.me_grid((3, 5, 2, 2), *C.grid_bounds(
        (3, 5, 2, 2)))
    assert cells == 60 and bins == (3, 5, 2, 2)
    lo, hi = C.grid_bounds((3, 5, 2, 2))
    assert np.array_equal(np.float32(inv32), mo.grid_inv(bins, lo, hi))
    assert np.array_equal(np.float32(lo32), np.float32(lo))
    assert ops.ME_CELLS_MAX == ops.GA_ROWS_MAX - 1 == 65534
    for bad in (((4, 4, 1), (0,) * 4, (1,) * 4),
                ((4, 0, 1, 1), (0,) * 4, (1,) * 4),
                ((256, 256, 1, 1), (0,) * 4, (1,) * 4),
                ((4, 4, 1, 1), (0,) * 4, (1, 0, 1, 1)),
                ((4, 4, 1, 1), (0,) * 4, (1, float("inf"), 1, 1)),
                ((4, 4, 1, 1), (0,) * 3, (1,) * 4),
                ((4, 4, 1, 1), (0,) * 4, (1e-46, 1, 1, 1)),
                ((4, 4, 1, 1), (-1e39, 0, 0, 0), (1,) * 4)):
        with pytest.raises(ValueError):
            ops.me_grid(*bad)


# ---- auto bounds -----------------------------------------------------------------------------

def test_auto_bounds_rule_and_the_engines_copy_of_it():
    from fiber_amd.es.map_elites import bounds_from_bc

    rng = np.random.default_rng(3)
    bc = rng.standard_normal((50, 4)).astype(np.float32)
    bc[:, 2] = 0.75                          # no range: widened by 1
    bc[4, 1] = np.nan
    bc[9, 0] = np.inf                        # the whole row is left out
    lo, hi = mo.auto_bounds(bc)
    ok = np.isfinite(bc).all(axis=1)
    a, b = bc[ok, 0].astype(float).min(), bc[ok, 0].astype(float).max()
    assert lo[0] == a - (b - a) / 2 and hi[0] == b + (b - a) / 2
    assert (lo[2], hi[2]) == (-0.25, 1.75)
    assert bounds_from_bc(bc) == (lo, hi)
    nothing = np.full((3, 4), np.nan, dtype=np.float32)
    assert mo.auto_bounds(nothing) == bounds_from_bc(nothing) \
        == ((-1.0,) * 4, (1.0,) * 4)


# ---- ArchiveMirror ---------------------------------------------------------------------------

@pytest.mark.parametrize("bounds", ["given", "auto"])
def test_archive_mirror_invariants_on_random_inputs(bounds):
    bins, pop, gens = (3, 3, 2, 1), 24, 12
    rng = np.random.default_rng(42)
    lo, hi = ((-1.0,) * 4, (1.0,) * 4) if bounds == "given" else (None, None)
    mirror = mo.ArchiveMirror(7, pop, bins, lo, hi)
    Cn = mirror.C
    assert Cn == 18 and mirror.parents()[0].tolist() == [Cn] * pop
    alias = 0
    for g in range(gens):
        fit = rng.standard_normal(pop).astype(np.float32)
        fit[rng.random(pop) < 0.1] = np.nan
        fit[rng.random(pop) < 0.2] = np.float32(0.5)
        bc = (0.6 * rng.standard_normal((pop, 4))).astype(np.float32)
        bc[rng.random(pop) < 0.05, 1] = np.nan
        before_fit = mirror.arch_fitness.copy()
        before_filled = mirror.arch_filled.copy()
        before_bc = mirror.arch_bc.copy()
        before_idx = mirror.filled_idx[: mirror.n_filled].copy()
        out = mirror.step(fit, bc)
        assert mirror.generation == g + 1
        # parents come from the cells that were filled before the step
        if before_idx.size:
            assert set(out["parent_idx"].tolist()) <= set(before_idx.tolist())
        else:
            assert (out["parent_idx"] == Cn).all()
        was = before_filled != 0
        assert (mirror.arch_filled[was] != 0).all()
        assert (mirror.arch_fitness[was] >= before_fit[was]).all()
        won = out["winner"] >= 0
        assert np.array_equal(mirror.arch_filled != 0, was | won)
        assert np.array_equal(mirror.arch_fitness[won],
                              fit[out["winner"][won]])
        assert np.array_equal(mirror.arch_bc[won], bc[out["winner"][won]])
        assert np.array_equal(mirror.arch_bc[~won], before_bc[~won])
        assert (out["cell"][out["winner"][won]] == np.flatnonzero(won)).all()
        assert not np.isnan(mirror.arch_fitness[mirror.arch_filled != 0]
                            ).any()
        n = mirror.n_filled
        assert mirror.filled_idx[:n].tolist() == np.flatnonzero(
            mirror.arch_filled).tolist()
        alias += len(C.aliasing_cells(out["winner"], out["parent_idx"], Cn))
        # every chain's last applied mutation is the generation it was born
        rows = mirror.lineage()
        assert rows.shape == (Cn + 1, g + 1) and (rows[Cn] == -1).all()
        for c in range(Cn):
            applied = np.flatnonzero(rows[c] >= 0)
            if mirror.arch_filled[c]:
                assert applied[-1] == mirror.arch_born[c]
                m = rows[c, applied[-1]]
                assert 0 <= m < pop
            else:
                assert applied.size == 0 and mirror.arch_born[c] == -1
    assert mirror.n_filled > 1
    if bounds == "given":
        assert alias > 0                      # the aliasing hazard occurred
    assert mirror.lo is not None and len(mirror.lo) == 4
