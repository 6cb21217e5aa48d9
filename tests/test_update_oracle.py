"""CPU checks of the fp64 oracle of the ES update half
(fiber_amd/es/update_oracle.py): numpy's draws against it, the coverage the
GPU draw test relies on, agreement with the existing numpy / torch
references, and mutation checks of every tolerance.  Derivations:
profiles/update_oracle.md."""

import dataclasses

import numpy as np
import pytest
import torch

import update_oracle_cases as C
from fiber_amd import ops
from fiber_amd.es import philox_ref
from fiber_amd.es import rollout_oracle
from fiber_amd.es import update_oracle as oracle

U, ULP, Z_SIDE_ULPS = oracle.U, oracle.ULP, oracle.Z_SIDE_ULPS

# A mutation must miss the tolerance by at least this factor somewhere.
MUTATION_FACTOR = 10.0


def test_constants_are_the_rollout_oracles():
    assert oracle.U is rollout_oracle.U and oracle.ULP is rollout_oracle.ULP
    assert oracle.Z_SIDE_ULPS is rollout_oracle.Z_SIDE_ULPS
    assert oracle.RANK_TOL == 2.0 * U


# ---- draws ------------------------------------------------------------------

@pytest.mark.parametrize("seed,iteration,pair", C.TRIPLES)
def test_numpy_draws_against_fp64(seed, iteration, pair):
    want = C.draws(seed, iteration, pair)
    got = philox_ref.noise_for_pair(seed, iteration, pair, C.NP_CONV)
    assert got.dtype == np.float32 and got.shape == want.shape
    worst = float(oracle.rel_err(got, want).max())
    print("numpy normal4 vs fp64 at", (seed, iteration, pair),
          "max relative error / ULP =", worst / ULP)
    assert worst <= Z_SIDE_ULPS * ULP


@pytest.mark.parametrize("seed,iteration,pair", C.TRIPLES)
def test_draw_vectors_cover_the_hard_arguments(seed, iteration, pair):
    """The tail of the log, draws near zero and every zero of cos and sin
    occur in each compared vector."""
    jb = np.arange((C.NP_CONV + 3) // 4, dtype=np.uint32)
    u0, u2, a0, a1 = oracle.draw_arguments(
        np.uint32(seed), np.uint32(iteration),
        np.uint32(pair) * np.ones_like(jb), jb, philox_ref.TAG_NOISE)
    z = C.draws(seed, iteration, pair)
    # the last block is ragged: its z2, z3 are not parameters, so leave the
    # whole block out of the conditions
    u = np.concatenate([u0[:-1], u2[:-1]])
    ang = np.concatenate([a0[:-1], a1[:-1]]).astype(np.float64)
    z = np.abs(z[:4 * (jb.size - 1)])
    assert u.min() <= 2.0 ** -18
    assert z.max() >= 4.5
    assert z.min() <= 1e-5
    for k in range(5):
        assert np.abs(ang - k * np.pi / 2.0).min() <= 3e-5, k
    assert u.max() <= 1.0 and u.min() > 0.0


def test_noise_blocks_and_tail():
    full = C.draws(*C.TRIPLES[0])
    nblocks = (C.NP_CONV + 3) // 4
    jb = np.array([0, 3, nblocks - 2, nblocks - 1])
    idx = oracle.param_index(C.NP_CONV, jb)
    assert idx.size == 14 and idx[-1] == C.NP_CONV - 1   # NP_CONV % 4 == 2
    got = oracle.noise_fp64(*C.TRIPLES[0], C.NP_CONV, jb)
    assert np.array_equal(got, full[idx])
    assert oracle.noise_fp64(1234, 3, 5, C.NP_MLP).shape == (C.NP_MLP,)


# ---- agreement with the existing references ------------------------------------

def test_grad_chunks_restates_the_launcher():
    g = oracle.grad_chunks
    assert [g(p, C.NP_MLP) for p in (1, 63, 64, 65, 70)] == [1, 1, 32, 32, 32]
    assert [g(p, C.NP_CONV) for p in (4, 63, 64, 66)] == [1, 1, 4, 4]
    assert oracle.grad_per_chunk(64, C.NP_MLP) == 2
    assert oracle.grad_per_chunk(65, C.NP_MLP) == 3   # 22 chunks used
    assert -(-65 // 3) == 22
    assert oracle.grad_per_chunk(64, C.NP_CONV) == 16
    assert oracle.grad_per_chunk(66, C.NP_CONV) == 17  # 17, 17, 17, 15
    # bx = 32 is where the conv branch starts
    assert g(64, 4 * 256 * 31) == 32 and g(64, 4 * 256 * 31 + 1) == 4


def test_grad_fp64_matches_numpy_noise_sums():
    """The same sum from philox_ref's float32 draws, accumulated in float64,
    differs by numpy's draw error alone."""
    for begin, end in ((0, 1), (6, 76)):
        g, abs_sum, _tol, _j = C.grad_reference(begin, end, C.NP_MLP)
        w = C.weights(begin, end).astype(np.float64)
        ref = np.zeros(C.NP_MLP)
        for k in range(begin, end):
            ref += w[k] * philox_ref.noise_for_pair(
                C.GRAD_SEED, C.GRAD_ITER, k, C.NP_MLP).astype(np.float64)
        assert np.isfinite(g).all()       # no NaN weight was read
        ratio = np.abs(ref - g) / (Z_SIDE_ULPS * ULP * abs_sum)
        print("grad_fp64 vs numpy sums", (begin, end), "err/tol",
              ratio.max())
        assert ratio.max() <= 1.0
        assert (abs_sum >= np.abs(g)).all()


def test_grad_fp64_on_conv_blocks_is_the_full_vector_there():
    begin, end = C.CONV_RANGES[0]
    g, _a, _t, idx = C.grad_reference(begin, end, C.NP_CONV)
    full, _a2 = oracle.grad_fp64(C.weights(begin, end), begin, end,
                                 C.GRAD_SEED, C.GRAD_ITER, C.NP_CONV)
    assert full.shape == (C.NP_CONV,)
    assert np.array_equal(g, full[idx])
    assert idx[0] == 0 and idx[-1] == C.NP_CONV - 1
    assert idx.size == 4 * C.conv_blocks().size - 2      # the ragged tail
    assert 1024 < C.conv_blocks().size < 8192


@pytest.mark.parametrize("n", C.RANK_SIZES[:-2] + (70,))
def test_centered_rank_exact_matches_torch_reference(n):
    for f in (C.rank_input(n), C.rank_equal_input(n)):
        want = oracle.centered_rank_exact(f)
        got = ops.centered_rank_ref(torch.from_numpy(f.copy())).numpy()
        assert got.dtype == np.float32
        assert np.array_equal(oracle.ranks_from_centered(got, n),
                              oracle.ranks_exact(f))
        # the torch reference may divide by reciprocal and multiply: one
        # rounding more than the kernels' 2*U
        assert np.abs(got - want).max() <= 3.0 * U
    assert np.array_equal(np.sort(oracle.ranks_exact(C.rank_input(n))),
                          np.arange(n))


def test_centered_rank_exact_ties_zeros_and_infinities():
    f = np.array([0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, np.inf, 0.0],
                 dtype=np.float32)
    assert list(oracle.ranks_exact(f)) == [2, 3, 5, 1, 6, 0, 7, 4]
    assert list(oracle.centered_rank_exact(
        np.float32([3.0, 3.0, 3.0]))) == [-0.5, 0.0, 0.5]
    with pytest.raises(ValueError):
        oracle.centered_rank_exact(np.float32([1.0]))


# ---- mutations of the gradient -----------------------------------------------

def _report(name, ratio):
    print("mutation %-34s misses the tolerance by %.3g x" % (name, ratio))
    assert ratio >= MUTATION_FACTOR, name


def test_grad_mutations_stand_out():
    begin, end = C.WHOLE
    g, _abs, tol, _j = C.grad_reference(begin, end, C.NP_MLP)
    w = C.weights(begin, end).astype(np.float64)
    k = begin + 2                       # the last pair of chunk 0
    assert w[k] != 0.0
    term = w[k] * oracle.noise_fp64(C.GRAD_SEED, C.GRAD_ITER, k, C.NP_MLP)
    _report("pair dropped from a chunk",
            (np.abs((g - term) - g) / tol).max())
    _report("pair counted twice", (np.abs((g + term) - g) / tol).max())

    nblocks = (C.NP_MLP + 3) // 4
    jb = np.arange(nblocks - 2)
    here, abs_here = oracle.grad_fp64(C.weights(begin, end), begin, end,
                                      C.GRAD_SEED, C.GRAD_ITER, C.NP_MLP, jb)
    there, _a = oracle.grad_fp64(C.weights(begin, end), begin, end,
                                 C.GRAD_SEED, C.GRAD_ITER, C.NP_MLP, jb + 1)
    tol_here = oracle.grad_tol(abs_here, end - begin, 32)
    _report("counter jb+1 instead of jb",
            (np.abs(there - here) / tol_here).max())
    # ... and the mutation is wrong everywhere, not at one coordinate
    assert (np.abs(there - here) > tol_here).mean() > 0.99


def test_tail_from_the_neighbouring_block_stands_out():
    """NP_CONV % 4 == 2: the last block holds two parameters.  A kernel
    that takes them from the block before must not pass."""
    begin, end = C.CONV_RANGES[0]
    nblocks = (C.NP_CONV + 3) // 4
    w = C.weights(begin, end)
    tail, abs_tail = oracle.grad_fp64(w, begin, end, C.GRAD_SEED,
                                      C.GRAD_ITER, C.NP_CONV,
                                      np.array([nblocks - 1]))
    prev, _a = oracle.grad_fp64(w, begin, end, C.GRAD_SEED, C.GRAD_ITER,
                                C.NP_CONV, np.array([nblocks - 2]))
    assert tail.shape == (2,) and prev.shape == (4,)
    tol = oracle.grad_tol(abs_tail, end - begin, 1)
    for name, mut in (("tail from block-1, same lanes", prev[:2]),
                      ("tail from block-1, next lanes", prev[2:])):
        _report(name, (np.abs(mut - tail) / tol).min())


# ---- mutations of the step ----------------------------------------------------

@dataclasses.dataclass
class Cfg:
    sigma: float = 0.05
    lr: float = 0.02
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8


STEP_SEED, STEP_ITER, STEP_POP = 1234, 6, 128


def _step_inputs():
    rng = np.random.default_rng(42)
    n = C.NP_MLP
    state = {
        "theta": (rng.standard_normal(n) * 0.2).astype(np.float32),
        "adam_m": (rng.standard_normal(n) * 0.05).astype(np.float32),
        "adam_v": (rng.random(n) * 0.01 + 1e-4).astype(np.float32),
        "t_step": 4,
        "obs_sum": (rng.standard_normal(4) * 500.0).astype(np.float32),
        "obs_sumsq": (rng.random(4) * 4000.0 + 3000.0).astype(np.float32),
        "obs_count": np.float32([4 * 16384.0]),
    }
    fitness = (rng.standard_normal(STEP_POP) * 0.3 + 1.0).astype(np.float32)
    assert np.unique(fitness).size == STEP_POP          # no ties
    obs_stat = np.concatenate([
        rng.standard_normal(4) * 200.0, rng.random(4) * 1500.0 + 500.0,
        [16384.0]]).astype(np.float32)
    return state, fitness, obs_stat


def _step(state, fitness, obs_stat, cfg=Cfg()):
    return oracle.step_fp64(state, fitness, obs_stat, cfg, STEP_SEED,
                            STEP_ITER, C.NP_MLP)


def _worst(base, tol, mut, fields=None):
    worst = 0.0
    for name in fields or tol:
        t = tol[name]
        ok = np.isfinite(t) & (t > 0.0)
        worst = max(worst, float(
            (np.abs(mut[name] - base[name])[ok] / t[ok]).max()))
    return worst


def test_step_fp64_formulas():
    """The chain against a direct float64 transcription on one coordinate
    and the obs fields, and the shape of what it returns."""
    state, fitness, obs_stat = _step_inputs()
    new, tol, flags = _step(state, fitness, obs_stat)
    assert new["t_step"] == 5
    assert set(tol) == set(new) - {"t_step"}
    cfg = Cfg()
    r = oracle.centered_rank_exact(fitness)
    w = (r[0::2] - r[1::2]).astype(np.float32)   # exact: multiples of 1/127
    g, _a = oracle.grad_fp64(r[0::2] - r[1::2], 0, 64, STEP_SEED, STEP_ITER,
                             C.NP_MLP)
    assert np.abs(w - (r[0::2] - r[1::2])).max() <= U
    g = g / (128 * 0.05)
    m = 0.9 * state["adam_m"].astype(np.float64) + (1 - 0.9) * g
    v = 0.999 * state["adam_v"].astype(np.float64) + (1 - 0.999) * g * g
    th = state["theta"].astype(np.float64) + cfg.lr * (m / (1 - 0.9 ** 5)) / (
        np.sqrt(v / (1 - 0.999 ** 5)) + 1e-8)
    assert np.allclose(new["adam_m"], m, rtol=1e-13, atol=0)
    assert np.allclose(new["adam_v"], v, rtol=1e-13, atol=0)
    assert np.allclose(new["theta"], th, rtol=1e-12, atol=0)
    cnt = 5 * 16384.0
    osum = state["obs_sum"].astype(np.float64) + obs_stat[:4]
    osq = state["obs_sumsq"].astype(np.float64) + obs_stat[4:8]
    assert new["obs_count"] == cnt
    assert np.array_equal(new["obs_sum"], osum)
    assert np.allclose(new["obs_mu"], osum / cnt, rtol=1e-15)
    assert np.allclose(new["obs_nu"], np.maximum(
        osq / cnt - (osum / cnt) ** 2, oracle.C1EM2), rtol=1e-13)
    assert not flags["obs_nu_clamp"].any()
    # the tolerances say something: nearly every coordinate of theta is
    # held far more tightly than the size of an Adam step
    share = float((tol["theta"] < 1e-3 * cfg.lr).mean())
    print("share of theta held within 1e-3 * lr:", share,
          " median tol / lr:", float(np.median(tol["theta"])) / cfg.lr)
    assert share > 0.99
    for name in ("adam_m", "adam_v"):
        assert np.isfinite(tol[name]).all() and (tol[name] > 0).all()


def test_obs_nu_clamp_is_flagged_and_exact_below():
    state, fitness, obs_stat = _step_inputs()
    state = dict(state)
    cnt = float(state["obs_count"][0]) + float(obs_stat[8])
    # dim 0: variance far below the clamp; dim 1: on it
    state["obs_sum"] = state["obs_sum"].copy()
    state["obs_sumsq"] = state["obs_sumsq"].copy()
    state["obs_sum"][:2] = 0.0
    obs_stat = obs_stat.copy()
    obs_stat[:2] = 0.0
    state["obs_sumsq"][:2] = 0.0
    obs_stat[4] = 1e-3 * cnt
    obs_stat[5] = np.float32(oracle.C1EM2 * cnt)
    new, tol, flags = _step(state, fitness, obs_stat)
    assert list(flags["obs_nu_clamp"]) == [False, True, False, False]
    assert new["obs_nu"][0] == oracle.C1EM2 and tol["obs_nu"][0] == 0.0


def test_floor_state_puts_dims_0_and_1_under_the_floor():
    """The state that tests/gpu/test_update_oracle_gpu.py loads for its
    variance-floor case, chosen here from step_fp64 with stand-in
    statistics (every action +1, every action -1): after the step the
    variance of dims 0 and 1 is below 1e-2 by more than its tolerance, so
    obs_nu is the floor itself with tolerance 0, and dims 2 and 3 are
    above it by more than theirs."""
    state, fitness, _stat = _step_inputs()
    state = dict(state)
    state.update(C.floor_obs_state())
    assert float(state["obs_count"][0]) + C.FLOOR_POP * 64 * 2 < 2.0 ** 24
    for asign in (1.0, -1.0):
        obs_stat = C.floor_standin_obs_stat(asign, STEP_ITER)
        new, tol, flags = oracle.step_fp64(state, fitness, obs_stat, Cfg(),
                                           C.FLOOR_SEED, STEP_ITER, C.NP_MLP)
        cnt = new["obs_count"][0]
        var = new["obs_sumsq"] / cnt - new["obs_mu"] ** 2
        print("actions %+d: variance after the step %s" % (asign, var))
        assert not flags["obs_nu_clamp"].any()
        assert (var[:2] < 0.2 * oracle.C1EM2).all() and (var[2:] > 0.5).all()
        assert (new["obs_nu"][:2] == oracle.C1EM2).all()
        assert (tol["obs_nu"][:2] == 0.0).all()
        assert (new["obs_nu"][2:] > oracle.C1EM2).all()
        assert (tol["obs_nu"][2:] > 0.0).all()
        # rstd = 9.95: a state 0.51 from the mean is clamped
        assert abs(1.0 / np.sqrt(oracle.C1EM2 + 1e-4) - 9.95) < 0.01


def test_step_mutations_stand_out():
    state, fitness, obs_stat = _step_inputs()
    base, tol, _flags = _step(state, fitness, obs_stat)

    mut, _t, _f = _step(dict(state, t_step=state["t_step"] - 1), fitness,
                        obs_stat)
    assert mut["t_step"] == base["t_step"] - 1
    _report("bias correction with t-1", _worst(base, tol, mut, ("theta",)))

    cfg = Cfg()
    mut, _t, _f = _step(state, fitness, obs_stat, dataclasses.replace(
        cfg, adam_beta1=cfg.adam_beta2, adam_beta2=cfg.adam_beta1))
    _report("beta1 and beta2 swapped",
            min(_worst(base, tol, mut, (name,))
                for name in ("theta", "adam_m", "adam_v")))

    # float(pop) * sigma with pop halved is the same number as with sigma
    # halved: both are exact scalings by 2
    mut, _t, _f = _step(state, fitness, obs_stat,
                        dataclasses.replace(cfg, sigma=cfg.sigma / 2.0))
    _report("pop_total replaced by the pairs",
            min(_worst(base, tol, mut, (name,))
                for name in ("theta", "adam_m", "adam_v")))

    swapped = np.concatenate([obs_stat[4:8], obs_stat[:4], obs_stat[8:]])
    mut, _t, _f = _step(state, fitness, swapped)
    _report("obs_sum and obs_sumsq slots swapped",
            min(_worst(base, tol, mut, (name,))
                for name in ("obs_sum", "obs_sumsq", "obs_mu", "obs_nu")))

    flipped = fitness.reshape(-1, 2)[:, ::-1].reshape(-1).copy()
    mut, _t, _f = _step(state, flipped, obs_stat)
    # the gradient changes sign: adam_v, which squares it, cannot see that
    assert _worst(base, tol, mut, ("adam_v",)) <= 1.0
    _report("wpair from ranks[1::2] - ranks[0::2]",
            min(_worst(base, tol, mut, (name,))
                for name in ("theta", "adam_m")))


def test_step_fp64_shard_and_conv_state():
    """A shard's pair_range restricts the gradient; a state without obs
    fields (the conv engine) returns none."""
    state, fitness, _obs = _step_inputs()
    conv_state = {k: state[k] for k in ("theta", "adam_m", "adam_v",
                                        "t_step")}
    cfg = Cfg()
    whole, tol, flags = oracle.step_fp64(conv_state, fitness, None, cfg,
                                         STEP_SEED, STEP_ITER, C.NP_MLP)
    assert set(whole) == {"theta", "adam_m", "adam_v", "t_step"}
    assert flags == {}
    lo, _t, _f = oracle.step_fp64(conv_state, fitness, None, cfg, STEP_SEED,
                                  STEP_ITER, C.NP_MLP, pair_range=(0, 40))
    hi, _t, _f = oracle.step_fp64(conv_state, fitness, None, cfg, STEP_SEED,
                                  STEP_ITER, C.NP_MLP, pair_range=(40, 64))
    m0 = 0.9 * conv_state["adam_m"].astype(np.float64)
    # adam_m is linear in the gradient: the shards' parts add up
    assert np.allclose((lo["adam_m"] - m0) + (hi["adam_m"] - m0),
                       whole["adam_m"] - m0, rtol=0, atol=1e-15)
