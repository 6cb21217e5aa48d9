"""Case lists and inputs shared by tests/test_map_elites.py (CPU) and
tests/gpu/test_map_elites_gpu.py.  Everything here runs without a GPU, is
computed once per process and is never modified by a test."""

import functools

import numpy as np

import ga_cases as GC
from fiber_amd.es import map_elites_oracle as mo

BC_DIM = 4

# ---- ga_rollout_mlp_bc against its siblings ----------------------------------
SIBLING_HORIZONS = (1, 8)
SIBLING_SIGMA = 0.05

# ---- me_insert -------------------------------------------------------------------
# 64 is the wave, 256 the block of me_assign; (254, 258, 1, 1) has 65532
# cells, two under the most the archive takes.
INSERT_POPS = (1, 63, 64, 65, 257, 1000)
INSERT_BINS = ((4, 4, 1, 1), (3, 5, 2, 2), (1, 1, 1, 1), (254, 258, 1, 1))
# Dimensions 0 and 2: bin width 0.25 from -1, so every edge and the scale
# are exact in fp32 and a BC on an edge gives an integer t.  Dimensions 1
# and 3: [-0.3, 0.7), where neither is.


def grid_bounds(bins):
    lo = (-1.0, -0.3, -1.0, -0.3)
    hi = (-1.0 + 0.25 * bins[0], 0.7, -1.0 + 0.25 * bins[2], 0.7)
    return lo, hi


def edge_values(bins, d):
    """The interior bin edges of dimension d as float32 (exact for d = 0,
    2)."""
    lo, hi = grid_bounds(bins)
    k = np.arange(1, bins[d], dtype=np.float64)
    return (lo[d] + k * (hi[d] - lo[d]) / bins[d]).astype(np.float32)


def _pool(bins, d, rng):
    """Values for component d: every interior edge, its two float32
    neighbours, the bounds, points outside them, both infinities, -0.0 and
    a few interior points."""
    lo, hi = grid_bounds(bins)
    edges = edge_values(bins, d)
    inf32 = np.float32(np.inf)
    parts = [edges, np.nextafter(edges, -inf32), np.nextafter(edges, inf32),
             np.float32([lo[d], hi[d], lo[d] - 1.0, hi[d] + 1.0, np.inf,
                         -np.inf, -0.0, 0.0]),
             rng.uniform(lo[d], hi[d], 8).astype(np.float32)]
    return np.concatenate(parts).astype(np.float32)


@functools.lru_cache(maxsize=None)
def insert_bc(pop, bins):
    """bc[pop][4]: component d of member m walks the pool of dimension d
    with its own stride, so the four do not move together; every 17th
    member has a NaN in one component."""
    rng = np.random.default_rng(500 + pop + 7 * sum(bins))
    bc = np.empty((pop, BC_DIM), dtype=np.float32)
    m = np.arange(pop)
    for d, stride in enumerate((1, 3, 5, 7)):
        pool = _pool(bins, d, rng)
        bc[:, d] = pool[(m * stride + d) % pool.size]
    nan_at = m[m % 17 == 5]
    bc[nan_at, (nan_at // 17) % BC_DIM] = np.nan
    bc.setflags(write=False)
    return bc


TIE_VALUES = np.float32([-1.5, 0.0, -0.0, 0.25, 3.0])


@functools.lru_cache(maxsize=None)
def insert_fitness(pop):
    """A third of the members share one of a few values (both zeros among
    them), a few are NaN or infinite, the rest are distinct."""
    rng = np.random.default_rng(900 + pop)
    f = rng.standard_normal(pop).astype(np.float32)
    tied = rng.random(pop) < 0.33
    f[tied] = rng.choice(TIE_VALUES, int(tied.sum()))
    f[rng.random(pop) < 0.04] = np.nan
    f[rng.random(pop) < 0.02] = np.inf
    f[rng.random(pop) < 0.02] = -np.inf
    f.setflags(write=False)
    return f


def archive(C, kind, seed=0):
    """(arch_fitness[C], arch_bc[C][4], arch_filled[C]) before the insert:
    'empty', 'full' or 'half' (a random half filled).  The fitness of a
    filled cell comes from the values the members tie on, or is random."""
    rng = np.random.default_rng(70 + seed + C)
    if kind == "empty":
        filled = np.zeros(C, dtype=np.int32)
    elif kind == "full":
        filled = np.ones(C, dtype=np.int32)
    else:
        assert kind == "half"
        filled = (rng.random(C) < 0.5).astype(np.int32)
    fit = rng.standard_normal(C).astype(np.float32)
    tied = rng.random(C) < 0.5
    fit[tied] = rng.choice(TIE_VALUES, int(tied.sum()))
    bc = rng.standard_normal((C, BC_DIM)).astype(np.float32)
    # what an empty cell holds is never read; make a stale read show
    fit[filled == 0] = np.float32(1e30)
    return fit, bc, filled


def _case(name, bins, bc, fitness, arch):
    lo, hi = grid_bounds(bins)
    for a in (bc, fitness) + tuple(arch):
        a.setflags(write=False)
    return dict(name=name, bins=tuple(bins), lo=lo, hi=hi, bc=bc,
                fitness=fitness, arch_fitness=arch[0], arch_bc=arch[1],
                arch_filled=arch[2])


def _spread_bc(n, bins, seed):
    """n finite interior BCs, uniformly over the grid."""
    rng = np.random.default_rng(seed)
    lo, hi = grid_bounds(bins)
    return rng.uniform(lo, hi, (n, BC_DIM)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def insert_cases():
    cases = []
    for pop in INSERT_POPS:
        for bins in INSERT_BINS:
            cases.append(_case(
                "pop%d-%s-half" % (pop, "x".join(map(str, bins))), bins,
                insert_bc(pop, bins).copy(), insert_fitness(pop).copy(),
                archive(mo.n_cells(bins), "half", pop)))
    # 1000 members, 40 % of them tied, 5 % NaN, into 4 cells: hundreds of
    # contenders per cell
    bins = (2, 2, 1, 1)
    ties = GC.fitness_ties(1000).copy()
    for kind in ("empty", "full", "half"):
        cases.append(_case("ties1000-2x2-" + kind, bins,
                           _spread_bc(1000, bins, 11), ties.copy(),
                           archive(4, kind, 1)))
    # the special values: one cell, and 2 x 2
    special = GC.fitness_special().copy()
    for bins in ((1, 1, 1, 1), (2, 2, 1, 1)):
        for kind in ("empty", "full"):
            cases.append(_case(
                "special-%s-%s" % ("x".join(map(str, bins)), kind), bins,
                _spread_bc(special.size, bins, 12), special.copy(),
                archive(mo.n_cells(bins), kind, 2)))
    # the occupant against the best child: equal (it stays, also as the
    # other zero) and one ulp below (the child wins)
    bins = (2, 2, 1, 1)
    bc = _spread_bc(40, bins, 13)
    f = np.random.default_rng(14).standard_normal(40).astype(np.float32)
    f[3] = f[17] = f.max()                   # the best child twice
    lo, hi = grid_bounds(bins)
    cell = mo.cells_exact(bc, lo, mo.grid_inv(bins, lo, hi), bins)
    best = np.array([f[cell == c].max() for c in range(4)], dtype=np.float32)
    assert np.isfinite(best).all()           # every cell has a child
    arch_bc = _spread_bc(4, bins, 15)
    full = np.ones(4, dtype=np.int32)
    cases.append(_case("occupant-equal", bins, bc.copy(), f.copy(),
                       (best.copy(), arch_bc.copy(), full.copy())))
    below = np.nextafter(best, np.float32(-np.inf)).astype(np.float32)
    cases.append(_case("occupant-one-ulp-below", bins, bc.copy(), f.copy(),
                       (below, arch_bc.copy(), full.copy())))
    fz = f.copy()
    fz[fz == fz.max()] = np.float32(0.0)
    fz[fz > 0] = -fz[fz > 0]                 # +0 is the best of every cell
    bestz = np.array([fz[cell == c].max() for c in range(4)],
                     dtype=np.float32)
    occ = np.where(bestz == 0, np.float32(-0.0), bestz).astype(np.float32)
    cases.append(_case("occupant-other-zero", bins, bc.copy(), fz,
                       (occ, arch_bc.copy(), full.copy())))
    return tuple(cases)


def insert_expected(case):
    """What me_insert must leave: cell, winner, order and the archive."""
    bins, lo, hi = case["bins"], case["lo"], case["hi"]
    pop = case["fitness"].size
    C = mo.n_cells(bins)
    cell = mo.cells_exact(case["bc"], lo, mo.grid_inv(bins, lo, hi), bins,
                          case["fitness"])
    winner, fit, filled = mo.insert_exact(
        case["arch_fitness"], case["arch_filled"], case["fitness"], cell)
    arch_bc = case["arch_bc"].copy()
    won = winner >= 0
    arch_bc[won] = case["bc"][winner[won]]
    order = np.append(np.where(won, winner, pop + np.arange(C)),
                      pop + C).astype(np.int32)
    return dict(cell=cell, winner=winner, order=order, arch_fitness=fit,
                arch_bc=arch_bc, arch_filled=filled)


def insert_brute(arch_fitness, arch_filled, fitness, cell):
    """The winner rule as a double loop over Python floats."""
    C = len(arch_fitness)
    winner = [-1] * C
    for c in range(C):
        best = None
        for m in range(len(fitness)):
            if int(cell[m]) != c:
                continue
            fm = float(fitness[m])
            if best is None or fm > float(fitness[best]):
                best = m                      # a later equal does not win
        if best is None:
            continue
        if arch_filled[c] and not float(fitness[best]) > float(
                arch_fitness[c]):
            continue
        winner[c] = best
    return np.array(winner, dtype=np.int32)


def cells_brute(bc, lo, inv, bins, fitness):
    """The cell rule member by member, every float32 rounding spelled
    out."""
    out = []
    for m, row in enumerate(bc):
        if any(x != x for x in row) or fitness[m] != fitness[m]:
            out.append(-1)
            continue
        c = 0
        for d in range(BC_DIM):
            with np.errstate(over="ignore", invalid="ignore"):
                diff = np.float32(np.float32(row[d]) - np.float32(lo[d]))
                t = float(np.float32(diff * np.float32(inv[d])))
            if t == float("inf"):
                b = bins[d] - 1
            elif t == float("-inf"):
                b = 0
            else:
                b = min(max(int(np.floor(t)), 0), bins[d] - 1)
            c = c * bins[d] + b
        out.append(c)
    return np.array(out, dtype=np.int32)


# ---- me_compact --------------------------------------------------------------------
# 64 is the wave, 1024 the workgroup and the chunk; 65534 the most cells.
COMPACT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65534)
COMPACT_PATTERNS = ("none", "all", "first", "last", "random")


def compact_flags(C, pattern):
    f = np.zeros(C, dtype=np.int32)
    if pattern == "all":
        f[:] = 1
    elif pattern == "first":
        f[0] = 1
    elif pattern == "last":
        f[-1] = 1
    elif pattern == "random":
        f[:] = np.random.default_rng(C).random(C) < 0.5
        f[f != 0] = np.random.default_rng(C + 1).integers(
            1, 5, int((f != 0).sum()))       # any non-zero value counts
    else:
        assert pattern == "none"
    return f


# ---- me_parents -----------------------------------------------------------------------
PARENT_CASES = ((7, 0), (7, 1), (256, 3), (1000, 1000))
PARENT_SEED, PARENT_GEN = 1234, 5


def parent_filled(n):
    """n filled cells that are not 0..n-1, and the padded device list."""
    idx = (np.arange(n) * 3 + 2).astype(np.int32)
    padded = np.full(3 * n + 5, -1, dtype=np.int32)
    padded[:n] = idx
    return idx, padded


# ---- engine -------------------------------------------------------------------------------
# The seed is chosen so that in at least one of the 5 generations a cell's
# new elite descends from another cell that is itself replaced in that
# generation: materialising the weights in place would then read a row that
# has already been overwritten.  Found by running seeds 1..24 on an MI355X:
# 13 of them show it at least once, seed 2 in three of the five generations
# (1, 2 and 1 such cells in generations 2, 3 and 4).  The GPU test asserts
# the property, so a stale entry fails.
ENGINE_SEED = 2
ENGINE = dict(pop=16, bins=(4, 4, 1, 1), horizon=4, seed=ENGINE_SEED)
ENGINE_GENERATIONS = 5
ILLUMINATE = dict(pop=256, bins=(8, 8, 1, 1), horizon=32)
ILLUMINATE_GENERATIONS = 30


def aliasing_cells(winner, parent_idx, C):
    """The cells c whose new elite (member winner[c]) has a parent cell p !=
    c that is itself replaced in this generation."""
    out = []
    for c in range(C):
        m = int(winner[c])
        if m < 0:
            continue
        p = int(parent_idx[m])
        if p < C and p != c and winner[p] >= 0:
            out.append(c)
    return out
