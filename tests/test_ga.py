"""Host tests of the Deep GA oracle (fiber_amd/es/ga_oracle.py), of the shared
cases of tests/ga_cases.py and of the validation that the ops wrappers and
GAEngine do before any launch.  No GPU."""

import numpy as np
import pytest
import torch

import ga_cases as C
import rollout_oracle_cases as RC
from fiber_amd import ops
from fiber_amd.es import ga_oracle as go
from fiber_amd.es import philox_ref
from fiber_amd.es import rollout_oracle


# ---- truncate_exact --------------------------------------------------------

@pytest.mark.parametrize("f", [C.fitness_special(), C.fitness_ties(200),
                               C.fitness_random(2), C.fitness_random(3),
                               C.fitness_random(257)],
                         ids=["special", "ties", "n2", "n3", "n257"])
def test_truncate_exact_is_the_order_rule(f):
    n = f.size
    full = C.truncate_brute(f, n)
    assert sorted(full.tolist()) == list(range(n))
    for T in C.truncate_ts(n):
        got = go.truncate_exact(f, T)
        assert got.dtype == np.int32 and got.shape == (T,)
        assert np.array_equal(got, full[:T]), T


def test_truncate_exact_on_the_special_values():
    f = C.fitness_special()
    order = go.truncate_exact(f, f.size)
    vals = f[order]
    # +inf first, by index; NaNs last, by index, whatever their sign
    assert order[:2].tolist() == [2, 11]
    nan_at = np.flatnonzero(np.isnan(f))
    assert order[-nan_at.size:].tolist() == nan_at.tolist()
    assert not np.isnan(vals[: -nan_at.size]).any()
    # -inf is a number: it ranks above the NaNs, below everything else
    assert order[-nan_at.size - 2: -nan_at.size].tolist() == [3, 10]
    # the two zeros tie: all five in index order, between the denormals
    zeros = np.flatnonzero(f == 0)
    at = [order.tolist().index(i) for i in zeros]
    assert at == list(range(at[0], at[0] + zeros.size))
    assert vals[at[0] - 1] == np.float32(1e-45)
    assert vals[at[-1] + 1] == -np.float32(1e-45)
    # non-increasing over the numbers
    nums = vals[: -nan_at.size].astype(np.float64)
    assert (nums[1:] <= nums[:-1]).all()


def test_ties_case_has_the_shares_it_names():
    f = C.fitness_ties()
    n = f.size
    assert np.isnan(f).sum() == n // 20
    _vals, counts = np.unique(f[~np.isnan(f)], return_counts=True)
    assert counts[counts > 1].sum() >= (2 * n) // 5
    assert np.signbit(f[np.isnan(f)]).any()
    assert not np.signbit(f[np.isnan(f)]).all()


def test_truncate_exact_refuses_bad_sizes():
    for f, T in ((np.zeros(1, np.float32), 1), (np.zeros(4, np.float32), 0),
                 (np.zeros(4, np.float32), 5),
                 (np.zeros((2, 2), np.float32), 1)):
        with pytest.raises(ValueError):
            go.truncate_exact(f, T)


# ---- parents_exact ----------------------------------------------------------

@pytest.mark.parametrize("pop,n_elite,T_cur", C.PARENT_CASES)
def test_parents_exact_ranges_and_elites_first(pop, n_elite, T_cur):
    pidx, slot = go.parents_exact(C.PARENT_SEED, C.PARENT_GEN, pop, n_elite,
                                  T_cur)
    assert pidx.dtype == slot.dtype == np.int32
    assert pidx.shape == slot.shape == (pop,)
    assert (pidx >= 0).all() and (pidx < T_cur).all()
    assert np.array_equal(pidx[:n_elite], np.arange(n_elite))
    assert (slot[:n_elite] == -1).all()
    assert np.array_equal(slot[n_elite:], np.arange(n_elite, pop))
    # the draw, written out for one member
    m = pop - 1
    u = philox_ref.philox4x32_10(
        np.uint32(C.PARENT_SEED), np.uint32(C.PARENT_GEN),
        np.array([m], np.uint32), np.uint32(0), np.uint32(0x45530004),
        np.uint32(0))[0]
    assert pidx[m] == (int(u[0]) * T_cur) >> 32
    if T_cur >= 3 and pop >= 256:
        # every survivor gets offspring, and not in a fixed pattern
        assert len(set(pidx[n_elite:].tolist())) >= min(T_cur, 3)
        other, _ = go.parents_exact(C.PARENT_SEED, C.PARENT_GEN + 1, pop,
                                    n_elite, T_cur)
        assert not np.array_equal(other, pidx)


def test_parents_exact_refuses_more_elites_than_parents():
    with pytest.raises(ValueError):
        go.parents_exact(1, 0, 8, 2, 1)
    with pytest.raises(ValueError):
        go.parents_exact(1, 0, 8, -1, 4)


# ---- lineage_step / decode_fp64 -----------------------------------------------

def test_lineage_step_gathers_the_parents_chain():
    lineage = np.array([[5, -1], [7, 9], [-1, -1]], dtype=np.int32)
    pidx = np.array([0, 1, 2, 1, 0, 2], dtype=np.int32)
    slot = np.array([-1, -1, 2, 3, 4, 5], dtype=np.int32)
    order = np.array([3, 0, 5], dtype=np.int32)
    new = go.lineage_step(lineage, pidx, slot, order, 2)
    assert new.dtype == np.int32
    assert new.tolist() == [[7, 9, 3], [5, -1, -1], [-1, -1, 5]]
    # generation 0: nothing to inherit, wider storage is ignored
    first = go.lineage_step(np.full((1, 8), -1, np.int32),
                            np.zeros(4, np.int32),
                            np.array([-1, 1, 2, 3], np.int32),
                            np.array([2, 0], np.int32), 0)
    assert first.tolist() == [[2], [-1]]


def test_decode_of_an_elite_only_chain_is_theta0_exactly():
    theta0 = np.asarray(RC.member_args()[0], dtype=np.float32)
    rows = np.array([[-1, -1, -1], [-1, 4, -1]], dtype=np.int32)
    value, tol = go.decode_fp64(theta0, rows, 0.05, 11)
    assert value.shape == tol.shape == (2, C.NPARAMS)
    assert np.array_equal(value[0], theta0.astype(np.float64))
    assert (tol[0] == 0).all()
    # one mutation: theta0 + sigma z of (seed, generation 1, slot 4)
    z = philox_ref.noise_for_pair(11, 1, 4, C.NPARAMS).astype(np.float64)
    sig = float(np.float32(0.05))
    assert np.array_equal(value[1], theta0.astype(np.float64) + sig * z)
    want = np.abs(sig * z) * (go.Z_REL + go.U) + go.U * np.abs(value[1])
    assert np.array_equal(tol[1], want) and (tol[1] > 0).all()
    # no columns at all
    value, tol = go.decode_fp64(theta0, np.zeros((1, 0), np.int32), 0.05, 11)
    assert np.array_equal(value[0], theta0.astype(np.float64))
    assert (tol == 0).all()


def test_decode_tolerance_grows_with_every_applied_generation():
    theta0 = np.asarray(RC.member_args()[0], dtype=np.float32)
    rows = np.array([[3, -1, -1], [3, -1, 8], [3, 6, 8]], dtype=np.int32)
    _value, tol = go.decode_fp64(theta0, rows, 0.05, 11)
    assert (tol[1] > tol[0]).all() and (tol[2] > tol[1]).all()
    # still a rounding-sized bound: far under one perturbation
    assert tol.max() < 1e-6


# ---- member_rollout and the pinned mixed launches -----------------------------

def test_member_rollout_is_the_rollout_oracles_member():
    """A mutated member of slot s at generation g is es_rollout_mlp's member
    2s at iteration g; an unmutated one is the eval cell of its row."""
    theta, mu, nu, A, B = RC.member_args()
    got = go.member_rollout(theta, 0.05, 125, RC.ITER, 1, 2, mu, nu, A, B)
    want = rollout_oracle.member_rollout(theta, 0.05, 125, RC.ITER, 2, 2, mu,
                                         nu, A, B)
    assert np.array_equal(got.returns, want.returns)
    assert np.array_equal(got.return_tol, want.return_tol)
    got = go.member_rollout(theta, 0.05, 125, RC.ITER, -1, 2, mu, nu, A, B)
    want = rollout_oracle.eval_cell(theta, mu, nu, A, B, 125, RC.ITER, 2)
    assert np.array_equal(got.returns, want.returns)
    assert not got.policy.w2_flag.any()


def test_mixed_launch_definition():
    rows = C.parent_rows()
    assert rows.shape == (3, C.NPARAMS) and rows.dtype == np.float32
    assert len({r.tobytes() for r in rows}) == 3
    assert len(C.MIXED_PARENT_IDX) == len(C.MIXED_SLOT) == C.MIXED_POP
    assert set(C.MIXED_PARENT_IDX) == {0, 1, 2}
    elites = [m for m, s in enumerate(C.MIXED_SLOT) if s < 0]
    assert 0 in elites and any(m > 1 for m in elites)
    assert any(C.MIXED_PARENT_IDX[m] != m for m in elites)
    assert all(s != m for m, s in enumerate(C.MIXED_SLOT))
    assert len(C.MIXED_LAUNCHES) >= 2
    assert max(h for _s, _g, h in C.MIXED_LAUNCHES) >= 2


@pytest.mark.parametrize("seed,gen,h", C.MIXED_LAUNCHES[:1])
def test_pinned_mixed_launch_is_decided_for_every_member(seed, gen, h):
    ros = C.mixed_launch(seed, gen)
    assert len(ros) == C.MIXED_POP
    assert all(ro.decided[:, h - 1].all() for ro in ros)
    # the members differ: parents and draws are really distinct
    fits = [rollout_oracle.fitness_of(ro, h)[0] for ro in ros]
    assert len(set(fits)) >= C.MIXED_POP - 2


# ---- GAConfig / GAEngine validation ----------------------------------------------

def test_config_defaults_and_validation():
    from fiber_amd.es import GAConfig

    cfg = GAConfig()
    assert (cfg.pop, cfg.truncation, cfg.n_elite, cfg.sigma, cfg.horizon,
            cfg.seed) == (1024, 32, 1, 0.02, 200, 1234)
    GAConfig(pop=2, truncation=2, n_elite=2, sigma=0.0, horizon=1)
    for bad in (dict(n_elite=0), dict(n_elite=33), dict(truncation=2048),
                dict(pop=1, truncation=1), dict(pop=65537),
                dict(sigma=-0.1), dict(sigma=float("nan")),
                dict(sigma=float("inf")), dict(horizon=0)):
        with pytest.raises(ValueError):
            GAConfig(**bad)
    # a config changed after construction is checked again by the engine
    from fiber_amd.es import GAEngine

    cfg = GAConfig(pop=8, truncation=4)
    cfg.n_elite = 5
    with pytest.raises(ValueError):
        GAEngine(cfg, device=torch.device("cpu"))


def test_engine_refuses_a_ring_context():
    from fiber_amd.es import GAConfig, GAEngine

    with pytest.raises(NotImplementedError, match="data-parallel"):
        GAEngine(GAConfig(pop=8, truncation=2, horizon=2), ctx=object())


def test_ops_validate_before_touching_the_device():
    """CPU tensors and bad shapes are refused by the wrappers' own checks:
    TypeError for dtype / device / contiguity first, then ValueError."""
    assert ops.ops_available()
    f = torch.zeros(8)
    with pytest.raises(TypeError):
        ops.ga_truncate(f, 2)                      # not on the GPU
    with pytest.raises(TypeError):
        ops.ga_truncate([0.0, 1.0], 1)
    with pytest.raises(TypeError):
        ops.ga_parents(1, 0, 8, 1, 1, torch.device("cpu"))
    for bad in (dict(pop=0), dict(n_elite=2), dict(T_cur=0),
                dict(n_elite=-1)):
        args = dict(pop=8, n_elite=1, T_cur=1)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.ga_parents(1, 0, args["pop"], args["n_elite"], args["T_cur"],
                           torch.device("cuda", 0))
    theta = torch.zeros(ops.NPARAMS)
    with pytest.raises(TypeError):
        ops.ga_decode(theta, torch.zeros(1, 2, dtype=torch.int32), 0.05, 1)
    with pytest.raises(TypeError):
        ops.ga_rollout_mlp(theta.view(1, -1), torch.zeros(2), torch.zeros(2),
                           0.05, 1, 0, 4, torch.zeros(4), torch.ones(4),
                           torch.zeros(4, 4), torch.zeros(4))
