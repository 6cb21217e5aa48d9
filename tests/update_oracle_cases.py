"""Case lists and inputs shared by tests/test_update_oracle.py (CPU) and
tests/gpu/test_update_oracle_gpu.py.  Everything here runs without a GPU, is
computed once per process and is never modified by a test."""

import functools

import numpy as np

from fiber_amd.es import update_oracle as oracle

NP_MLP = 4610
NP_CONV = 677686

# (seed, iteration, pair) of the draw vectors that are compared one by one
TRIPLES = ((1234, 3, 5), (7, 1, 0), (5, 2, 40))


def hot_range(pair):
    """A range of 4 pairs holding ``pair`` that does not start at 0, which
    only pair 0 itself cannot have."""
    begin = max(pair - 2, 0)
    return begin, begin + 4


@functools.lru_cache(maxsize=None)
def draws(seed, iteration, pair, nparams=NP_CONV):
    z = oracle.noise_fp64(seed, iteration, pair, nparams)
    z.setflags(write=False)
    return z


# ---- es_grad ----------------------------------------------------------------
GRAD_SEED, GRAD_ITER = 5, 2
# (pair_begin, pair_end) at nparams = 4610: one pair; 63, the largest single
# chunk; 64 = 32 chunks of 2; 65 = 22 chunks of 3 and 10 empty ones; 70; and
# 70 from pair 6 on, with its two shards.
MLP_RANGES = ((0, 1), (0, 63), (0, 64), (0, 65), (0, 70), (6, 76))
SHARDS = ((6, 38), (38, 76))
WHOLE = (6, 76)
# at nparams = NP_CONV: one chunk; 4 x 16; 17, 17, 17, 15
CONV_RANGES = ((2, 6), (2, 66), (2, 68))


def weights(begin, end):
    """float32 pair weights for [begin, end), indexed by pair like the
    kernel's wpair and 5 entries longer than the range: NaN everywhere
    outside it, so a read outside poisons the output, and a +0.0 and a -0.0
    inside when the range has room."""
    rng = np.random.default_rng(100 * begin + end)
    w = np.full(end + 5, np.nan, dtype=np.float32)
    w[begin:end] = (rng.random(end - begin) - 0.5).astype(np.float32)
    if end - begin >= 8:
        w[begin + 1] = 0.0
        w[begin + 4] = -0.0
        w[end - 1] = 0.0       # the last pair of the last used chunk
    return w


@functools.lru_cache(maxsize=None)
def conv_blocks():
    """Parameter blocks compared at NP_CONV: the first 512, the last 512
    (the ragged tail among them) and every 37th in between."""
    nblocks = (NP_CONV + 3) // 4
    jb = np.concatenate([np.arange(512), np.arange(512, nblocks - 512, 37),
                         np.arange(nblocks - 512, nblocks)])
    jb.setflags(write=False)
    return jb


@functools.lru_cache(maxsize=None)
def grad_reference(begin, end, nparams):
    """(g, abs_sum, tolerance, parameter indices) of es_grad over [begin,
    end) with ``weights(begin, end)``; at NP_CONV on conv_blocks() only."""
    jb = conv_blocks() if nparams == NP_CONV else None
    g, abs_sum = oracle.grad_fp64(weights(begin, end), begin, end, GRAD_SEED,
                                  GRAD_ITER, nparams, jb)
    pairs = end - begin
    tol = oracle.grad_tol(abs_sum, pairs, oracle.grad_chunks(pairs, nparams))
    return g, abs_sum, tol, oracle.param_index(nparams, jb)


# ---- centered_rank ----------------------------------------------------------
RANK_SIZES = (2, 3, 255, 256, 257, 4096, 16384, 16385)

_SPECIALS = np.array(
    [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1e-45, -1e-45, 0.0, -0.0,
     np.inf, -np.inf, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38],
    dtype=np.float32)


@functools.lru_cache(maxsize=None)
def rank_input(n, salt=0):
    """float32 [n]: values of both signs with fractional parts, a third of
    them quantised to halves (heavy ties), and +-0, +-inf and denormals
    spread over the whole index range.  n = 2 and 3 take what fits."""
    if n == 2:
        f = np.array([1.25, -np.inf], dtype=np.float32)
    elif n == 3:
        f = np.array([-0.0, 2.5, 0.0], dtype=np.float32)
    else:
        rng = np.random.default_rng(7000 + 13 * n + salt)
        f = (rng.standard_normal(n) * 3.0).astype(np.float32)
        tie = rng.random(n) < 1.0 / 3.0
        f[tie] = np.round(f[tie] * 2.0) / 2.0
        small = rng.random(n) < 0.05
        f[small] *= np.float32(1e-3)
        pos = np.linspace(0, n - 1, _SPECIALS.size).astype(np.int64)
        f[pos] = np.roll(_SPECIALS, salt)
    f.setflags(write=False)
    return f


def rank_equal_input(n):
    return np.full(n, -2.75, dtype=np.float32)


# ---- whole step ---------------------------------------------------------------
STEP_ITERATIONS = (5, 6, 7)
MLP_STEP_POPS = (128, 130)     # 64 pairs: 32 chunks; 65 pairs: empty chunks
STEP_HORIZON = 2
CONV_STEP_POP = 8
POPULATION_SEEDS = (1234, 77)
POPULATION_POP = 128


# ---- the variance floor taken by a real step ------------------------------------
# A running normaliser with a long history (2^23 observations; the count
# stays exact in fp32 after the step's 128 * 64 * 2 more) whose dims 0 and 1
# have the variance 1e-3: the step adds states of variance near 0.1, which
# moves it to about 1.2e-3, far under the 1e-2 floor of ESEngine.step, while
# dims 2 and 3 stay near 1.  The means differ per dim and in sign so that
# the floored dims reach the +-5 clamp of the normalised obs on both sides.
FLOOR_POP = 128
FLOOR_COUNT = 2.0 ** 23
FLOOR_MEAN = (0.3, -0.2, 0.1, -0.4)
FLOOR_VAR = (1e-3, 1e-3, 1.0, 1.0)
FLOOR_SEED = 1234               # ESConfig's default seed


def floor_obs_state():
    """obs_sum, obs_sumsq, obs_count (float32) to load into the engine."""
    mean = np.array(FLOOR_MEAN, dtype=np.float64)
    var = np.array(FLOOR_VAR, dtype=np.float64)
    return {
        "obs_sum": (FLOOR_COUNT * mean).astype(np.float32),
        "obs_sumsq": (FLOOR_COUNT * (var + mean * mean)).astype(np.float32),
        "obs_count": np.array([FLOOR_COUNT], dtype=np.float32),
    }


def floor_standin_obs_stat(asign, iteration):
    """A stand-in for the obs_stat[9] of the step's rollout, without a
    GPU: horizon STEP_HORIZON = 2 accumulates s_0, which is the same env
    draw for every member, and s_1 = 0.97 s_0 + 0.08 tanh(A s_0) + asign *
    0.05 B, here with every action of every member equal to ``asign``, the
    two extremes of what the policy can do."""
    from fiber_amd.es import philox_ref
    from fiber_amd.es.engine import make_env_params

    assert STEP_HORIZON == 2
    env_A, env_B = (t.double().numpy()
                    for t in make_env_params(FLOOR_SEED, "cpu"))
    s0 = philox_ref.env_init_state(FLOOR_SEED, iteration, 64).astype(
        np.float64)
    s1 = 0.97 * s0 + 0.08 * np.tanh(s0 @ env_A.T) + asign * 0.05 * env_B
    s = np.concatenate([s0, s1])
    return np.concatenate([FLOOR_POP * s.sum(0), FLOOR_POP * (s * s).sum(0),
                           [FLOOR_POP * 64.0 * STEP_HORIZON]]).astype(
                               np.float32)
