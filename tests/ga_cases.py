"""Case lists and inputs shared by tests/test_ga.py (CPU) and
tests/gpu/test_ga_gpu.py.  Everything here runs without a GPU, is computed
once per process and is never modified by a test."""

import functools

import numpy as np

import rollout_oracle_cases as RC
from fiber_amd.es import ga_oracle

NPARAMS = 4610
ITER = RC.ITER

# ---- ga_rollout_mlp against its siblings ---------------------------------
SIBLING_SIGMAS = (0.05, 4.0)
SIBLING_HORIZONS = (1, 8)
SIBLING_POP = 8
SIBLING_SEED = RC.SEED
UNMUTATED_PARENT_IDX = (2, 0, 1, 1, 2, 0, 0, 2)


@functools.lru_cache(maxsize=None)
def parent_rows(T=3):
    """T distinct parent rows: row 0 is the policy of RC.member_args(), the
    others are built the same way from other salts."""
    rows = [np.asarray(RC.member_args()[0], dtype=np.float32)]
    rows += [RC.bits._theta(20 + t).numpy() for t in range(1, T)]
    out = np.stack(rows).astype(np.float32)
    out.setflags(write=False)
    return out


# ---- mixed launch: elites and mutated members of distinct parents --------
# Member m is row MIXED_PARENT_IDX[m], unmutated where MIXED_SLOT[m] < 0 and
# otherwise mutated with the draw of slot 3m + 1, which is never the member
# index: a kernel that keys the draw by m, or reads parent m, is off by
# whole perturbations.  The elites sit at the front, as ga_parents puts
# them, and in the middle, and their parents are not their own index.
MIXED_POP = 8
MIXED_SIGMA = 0.05
MIXED_PARENT_IDX = (1, 2, 1, 1, 2, 0, 0, 2)
MIXED_SLOT = (-1, -1, 7, 10, 13, -1, 19, 22)
MIXED_H_MAX = 3
# (seed, generation, h): all MIXED_POP * 64 episodes are decided through h
# steps.  Found on the CPU by find_mixed_launches over seeds 100..299 at
# generations (ITER, 0, 3); the property is asserted by the tests, so a
# stale entry fails instead of comparing undecided episodes.
MIXED_LAUNCHES = ((100, 7, 3), (138, 3, 3), (103, 7, 2), (112, 0, 2),
                  (100, 0, 1))


def mixed_member_rollout(seed, gen, m, horizon=MIXED_H_MAX):
    _theta, mu, nu, A, B = RC.member_args()
    return ga_oracle.member_rollout(
        parent_rows()[MIXED_PARENT_IDX[m]], MIXED_SIGMA, seed, gen,
        MIXED_SLOT[m], horizon, mu, nu, A, B)


@functools.lru_cache(maxsize=None)
def mixed_launch(seed, gen):
    """Oracle rollouts, MIXED_H_MAX steps, of the MIXED_POP members.
    Horizon h < MIXED_H_MAX is a prefix of it."""
    return tuple(mixed_member_rollout(seed, gen, m)
                 for m in range(MIXED_POP))


def find_mixed_launches(seeds, gens, horizons=(3, 2, 1)):
    """CPU search behind MIXED_LAUNCHES: (seed, gen, h) with h the longest
    of ``horizons`` through which every episode of every member is
    decided."""
    found = []
    for seed in seeds:
        for gen in gens:
            through = MIXED_H_MAX
            for m in range(MIXED_POP):
                ro = mixed_member_rollout(seed, gen, m)
                # decided[:, t] is cumulative, so the count is the horizon
                through = min(through, int(ro.decided.all(axis=0).sum()))
                if through < min(horizons):
                    break
            for h in horizons:
                if through >= h:
                    found.append((seed, gen, h))
                    break
    return found


# ---- ga_truncate --------------------------------------------------------------
# 2048 is the kernel's LDS tile: one size on each side of it and the tile
# itself, and the largest population the kernel takes.
TRUNCATE_SIZES = (2, 3, 255, 256, 257, 1000, 2047, 2048, 2049)
TRUNCATE_MAX = 65536


def truncate_ts(n):
    return tuple(sorted({1, max(1, n // 2), n}))


@functools.lru_cache(maxsize=None)
def fitness_random(n):
    """n distinct-ish finite values, both signs."""
    rng = np.random.default_rng(1000 + n)
    f = rng.standard_normal(n).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def fitness_ties(n=1000):
    """40 % of the members share one of 5 values, 5 % are NaN (both signs
    of NaN, two payloads), the rest are distinct."""
    rng = np.random.default_rng(77)
    f = rng.standard_normal(n).astype(np.float32)
    who = rng.permutation(n)
    tied, nans = who[: (2 * n) // 5], who[(2 * n) // 5 : (2 * n) // 5 + n // 20]
    f[tied] = rng.choice(np.float32([-1.5, 0.0, 0.25, 0.25, 3.0]), tied.size)
    bits = f.view(np.uint32)
    bits[nans[0::2]] = 0x7FC00000
    bits[nans[1::2]] = 0xFFC00001
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def fitness_special():
    """Signed zeros, infinities, denormals, the extremes and NaNs, each more
    than once and interleaved, so that every tie is broken by index."""
    tiny = np.float32(1e-45)                       # the smallest denormal
    big = np.finfo(np.float32).max
    vals = [0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.nan, 1.0, -0.0, 0.0,
            -np.inf, np.inf, -tiny, tiny, big, -big, np.nan, 1.0, 2e-39,
            -2e-39, 0.0, np.nan, big, -big]
    f = np.array(vals, dtype=np.float32)
    f.setflags(write=False)
    return f


def truncate_brute(f, T):
    """The order rule as a double loop over Python floats."""
    n = len(f)

    def beats(j, i):
        fj, fi = float(f[j]), float(f[i])
        if fi != fi:                                # f[i] is NaN
            return fj == fj or j < i
        return fj > fi or (fj == fi and j < i)

    order = [None] * n
    for i in range(n):
        order[sum(beats(j, i) for j in range(n) if j != i)] = i
    assert None not in order
    return np.array(order[:T], dtype=np.int32)


# ---- ga_parents ------------------------------------------------------------------
PARENT_CASES = ((7, 1, 1), (256, 3, 3), (1000, 4, 1000))
PARENT_SEED, PARENT_GEN = 1234, 5

# ---- engine ----------------------------------------------------------------------
ENGINE = dict(pop=16, truncation=4, n_elite=1, horizon=4)
ENGINE_GENERATIONS = 5
LEARN = dict(pop=256, truncation=16, horizon=32)
LEARN_GENERATIONS = 30
