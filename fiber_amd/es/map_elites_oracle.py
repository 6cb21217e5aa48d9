"""Numpy oracle of the MAP-Elites kernels (fiber_amd/csrc/ops/me_kernels.hip)
and of MapElitesEngine's bookkeeping.  Runs anywhere; nothing here comes from
a GPU run.  Derivations: profiles/map_elites.md.  Each function is written
without reference to the kernel's method (sorts and dictionaries where the
device takes an atomic maximum, a cumulative count where it ballots).

  grid_inv        the fp32 bin scale of a grid, from double precision
  cells_exact     me_insert's cell of every member, in fp32 numpy
  insert_exact    me_insert's winners and the archive's new fitness / filled
  compact_exact   me_compact
  parents_exact   me_parents, integer for integer
  auto_bounds     the bounds MapElitesEngine fixes after generation 0
  ArchiveMirror   the engine's whole bookkeeping, one generation at a time
  member_rollout  one member of ga_rollout_mlp_bc: ga_oracle's
"""

import numpy as np

from . import philox_ref
from .ga_oracle import member_rollout  # noqa: F401

TAG_ME_PARENT = np.uint32(0x45530005)
BC_DIM = 4


def n_cells(bins):
    bins = tuple(int(b) for b in bins)
    assert len(bins) == BC_DIM and min(bins) >= 1, bins
    return bins[0] * bins[1] * bins[2] * bins[3]


def grid_inv(bins, lo, hi):
    """float32 [4]: ``bins[d] / (hi[d] - lo[d])`` in float64, rounded once
    to float32."""
    bins = np.asarray(bins, dtype=np.float64)
    span = np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
    return (bins / span).astype(np.float32)


def cells_exact(bc, lo, inv, bins, fitness=None):
    """int32 cell[pop] of the rows ``bc[pop][4]``: per dimension ``t = (bc -
    lo) * inv`` with float32 operands and one float32 rounding per
    operation, ``b = floor(t)`` clamped to ``[0, bins - 1]`` (an infinite t
    clamps too), the four bin numbers folded row-major.  -1 for a row with
    a NaN component, or with a NaN ``fitness`` if that is given."""
    bc = np.asarray(bc, dtype=np.float32).reshape(-1, BC_DIM)
    lo = np.asarray(lo, dtype=np.float32)
    inv = np.asarray(inv, dtype=np.float32)
    bins = np.asarray([int(b) for b in bins], dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = bc - lo                       # float32 - float32 -> float32
        t = diff * inv
    assert diff.dtype == np.float32 and t.dtype == np.float32
    dead = np.isnan(bc).any(axis=1)
    if fitness is not None:
        dead |= np.isnan(np.asarray(fitness, dtype=np.float32))
    whole = np.floor(np.where(np.isnan(t), np.float32(0), t))
    b = np.clip(whole.astype(np.float64), 0.0,
                (bins - 1).astype(np.float64)).astype(np.int64)
    cell = ((b[:, 0] * bins[1] + b[:, 1]) * bins[2] + b[:, 2]) * bins[3] \
        + b[:, 3]
    cell[dead] = -1
    return cell.astype(np.int32)


def insert_exact(arch_fitness, arch_filled, fitness, cell):
    """(winner[C], new_fitness[C], new_filled[C]).  Per cell the candidates
    are the members with that ``cell`` and, if the cell is filled, the
    occupant.  The best child is the greatest fitness, the lower index among
    equals (-0 equals +0); it wins only if the cell is empty or it is
    strictly greater than the occupant.  ``winner`` is the member or -1.

    A stable sort over (cell, descending fitness, index); the first entry
    of every run of equal cells is the best child."""
    arch_fitness = np.asarray(arch_fitness, dtype=np.float32)
    arch_filled = np.asarray(arch_filled)
    fitness = np.asarray(fitness, dtype=np.float32)
    cell = np.asarray(cell)
    C = arch_fitness.size
    winner = np.full(C, -1, dtype=np.int32)
    new_fitness = arch_fitness.copy()
    new_filled = (arch_filled != 0).astype(np.int32)
    live = np.flatnonzero(cell >= 0)
    assert not np.isnan(fitness[live]).any()
    # ascending negation = descending value; -(+0) and -(-0) compare equal
    neg = -fitness[live].astype(np.float64)
    by = np.lexsort((live, neg, cell[live]))
    ranked = live[by]
    first = np.ones(ranked.size, dtype=bool)
    first[1:] = cell[ranked[1:]] != cell[ranked[:-1]]
    for m in ranked[first]:
        c = int(cell[m])
        occupied = bool(arch_filled[c])
        # an occupant that is NaN (never stored by the engine) loses
        if occupied and not np.isnan(arch_fitness[c]) \
                and not float(fitness[m]) > float(arch_fitness[c]):
            continue
        winner[c] = m
        new_fitness[c] = fitness[m]
        new_filled[c] = 1
    return winner, new_fitness, new_filled


def compact_exact(arch_filled):
    """(filled_idx[C], n): the indices of the non-zero entries in ascending
    order, -1 behind them, and their number."""
    arch_filled = np.asarray(arch_filled)
    on = arch_filled != 0
    place = np.cumsum(on) - 1
    out = np.full(arch_filled.size, -1, dtype=np.int32)
    for c in range(arch_filled.size):
        if on[c]:
            out[place[c]] = c
    return out, int(on.sum())


def parents_exact(seed, gen, pop, filled_idx, root_row):
    """int32 (parent_idx[pop], slot[pop]) of generation ``gen``: member m
    mutates the elite of cell ``filled_idx[(u_m * n) >> 32]`` with the draw
    of slot m, ``n = len(filled_idx)`` and ``u_m`` the first word of
    philox4x32_10 keyed (seed, gen) at counter (m, 0, TAG_ME_PARENT, 0).
    With no filled cell every parent is ``root_row``."""
    pop = int(pop)
    filled_idx = np.asarray(filled_idx, dtype=np.int64).reshape(-1)
    n = filled_idx.size
    m = np.arange(pop, dtype=np.uint32)
    slot = m.astype(np.int32)
    if n == 0:
        return np.full(pop, int(root_row), dtype=np.int32), slot
    u = philox_ref.philox4x32_10(
        np.uint32(int(seed) & 0xFFFFFFFF), np.uint32(int(gen) & 0xFFFFFFFF),
        m, np.uint32(0), TAG_ME_PARENT, np.uint32(0))[0]
    pick = (u.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)
    return filled_idx[pick.astype(np.int64)].astype(np.int32), slot


def auto_bounds(bc):
    """(lo[4], hi[4]) as Python floats: per dimension the minimum and the
    maximum over the rows of ``bc`` that are finite throughout, widened by
    half the range on each side, or by 1 where the range is 0.  With no
    finite row: (-1, 1)."""
    rows = [[float(x) for x in row] for row in np.asarray(bc).reshape(-1, 4)]
    rows = [r for r in rows if all(np.isfinite(x) for x in r)]
    lo, hi = [], []
    for d in range(BC_DIM):
        col = [r[d] for r in rows] or [0.0]
        a, b = min(col), max(col)
        pad = (b - a) / 2 if b > a else 1.0
        lo.append(a - pad)
        hi.append(b + pad)
    return tuple(lo), tuple(hi)


class ArchiveMirror:
    """MapElitesEngine's bookkeeping on the host.  ``step(fitness, bc)``
    takes one generation's results and performs parents, cells, winners,
    the archive's fitness / BC / filled / born and the seed chains; what the
    generation chose is returned and the state is left in the attributes.
    Chains are Python lists, one per cell and one for the root (all -1)."""

    def __init__(self, seed, pop, bins, lo=None, hi=None):
        self.seed, self.pop = int(seed), int(pop)
        self.bins = tuple(int(b) for b in bins)
        self.C = n_cells(self.bins)
        self.lo = None if lo is None else tuple(float(x) for x in lo)
        self.hi = None if hi is None else tuple(float(x) for x in hi)
        C = self.C
        self.arch_fitness = np.zeros(C, dtype=np.float32)
        self.arch_bc = np.zeros((C, BC_DIM), dtype=np.float32)
        self.arch_filled = np.zeros(C, dtype=np.int32)
        self.arch_born = np.full(C, -1, dtype=np.int32)
        self.chains = [[] for _ in range(C + 1)]
        self.filled_idx = np.full(C, -1, dtype=np.int32)
        self.n_filled = 0
        self.generation = 0

    def parents(self):
        """(parent_idx, slot) of the generation about to run."""
        return parents_exact(self.seed, self.generation, self.pop,
                             self.filled_idx[: self.n_filled], self.C)

    def step(self, fitness, bc):
        g = self.generation
        fitness = np.asarray(fitness, dtype=np.float32)
        bc = np.asarray(bc, dtype=np.float32).reshape(self.pop, BC_DIM)
        parent_idx, slot = self.parents()
        if self.lo is None:
            self.lo, self.hi = auto_bounds(bc)
        inv = grid_inv(self.bins, self.lo, self.hi)
        cell = cells_exact(bc, self.lo, inv, self.bins, fitness)
        winner, new_fitness, new_filled = insert_exact(
            self.arch_fitness, self.arch_filled, fitness, cell)
        chains = []
        for c in range(self.C):
            m = int(winner[c])
            if m >= 0:
                self.arch_bc[c] = bc[m]
                self.arch_born[c] = g
                chains.append(self.chains[int(parent_idx[m])] + [int(slot[m])])
            else:
                chains.append(self.chains[c] + [-1])
        chains.append(self.chains[self.C] + [-1])
        self.chains = chains
        self.arch_fitness, self.arch_filled = new_fitness, new_filled
        self.filled_idx, self.n_filled = compact_exact(new_filled)
        self.generation = g + 1
        return {"parent_idx": parent_idx, "slot": slot, "cell": cell,
                "winner": winner}

    def lineage(self):
        """int32 [C + 1][generation]: the chains as MapElitesEngine keeps
        them, the root row last."""
        out = np.full((self.C + 1, self.generation), -1, dtype=np.int32)
        for c, chain in enumerate(self.chains):
            out[c, :] = chain
        return out
