"""Deep GA on the device: the kernels of fiber_amd/csrc/ops/ga_kernels.hip and
GAEngine (fiber_amd/es/ga.py) against their siblings, bit for bit where the
two must agree, and against the numpy oracle (fiber_amd/es/ga_oracle.py,
rollout_oracle; derivations in profiles/ga.md) where they do not.

  ga_rollout_mlp   mutated members: es_rollout_mlp's even members, bits;
                   unmutated ones: es_eval_matrix's cells, bits; a mixed
                   launch: rollout_oracle.fitness_of / obs_stats_tol on
                   launches whose every episode the oracle calls decided
  ga_truncate      truncate_exact, exactly
  ga_parents       parents_exact, exactly
  ga_survivors     es_eval_matrix of the rows returns fitness[order], bits
  ga_decode        the materialised parents, bits, and decode_fp64's
                   per-element tolerance
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import ga_cases as C  # noqa: E402
import rollout_oracle_cases as RC  # noqa: E402
from fiber_amd.es import ga_oracle as go  # noqa: E402
from fiber_amd.es import rollout_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


def _dev():
    return torch.device("cuda", 0)


def _to_dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(_dev()).contiguous()


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=_dev())


def _f64(t):
    return t.detach().cpu().double().numpy()


def _device_member_args():
    return [_to_dev(a) for a in RC.member_args()]


def _eval_rows(rows, mu, nu, A, B, seed, gen, h):
    """es_eval_matrix of rows[K] on the one environment, every policy with
    the same normaliser: scores[K]."""
    from fiber_amd import ops

    K = rows.shape[0]
    return ops.es_eval_matrix(
        rows, mu.expand(K, 4).contiguous(), nu.expand(K, 4).contiguous(),
        A.unsqueeze(0), B.unsqueeze(0), seed, gen, h)[:, 0]


# ---- 1. mutated members keep es_rollout_mlp's bits ---------------------------

@requires_gpu
@pytest.mark.parametrize("sigma", C.SIBLING_SIGMAS)
@pytest.mark.parametrize("horizon", C.SIBLING_HORIZONS)
def test_mutated_members_carry_the_es_kernels_bits(horizon, sigma):
    from fiber_amd import ops

    theta, mu, nu, A, B = _device_member_args()
    pop = C.SIBLING_POP
    fit, stat = ops.ga_rollout_mlp(
        theta.unsqueeze(0), _i32([0] * pop), _i32(range(pop)), sigma,
        C.SIBLING_SEED, C.ITER, horizon, mu, nu, A, B)
    want, _stat = ops.es_rollout_mlp(theta, sigma, C.SIBLING_SEED, C.ITER,
                                     horizon, 0, 2 * pop, mu, nu, A, B)
    assert fit.shape == (pop,) and stat.shape == (9,)
    assert torch.isfinite(fit).all()
    assert torch.equal(fit, want[0::2])
    assert float(stat[8]) == pop * 64 * horizon
    assert fit.unique().numel() > 1


# ---- 2. unmutated members keep es_eval_matrix's bits -------------------------

@requires_gpu
@pytest.mark.parametrize("horizon", C.SIBLING_HORIZONS)
def test_unmutated_members_carry_the_eval_matrix_bits(horizon):
    from fiber_amd import ops

    _theta, mu, nu, A, B = _device_member_args()
    parents = _to_dev(C.parent_rows())
    pidx = C.UNMUTATED_PARENT_IDX
    fit, stat = ops.ga_rollout_mlp(
        parents, _i32(pidx), _i32([-1] * len(pidx)), 0.05, C.SIBLING_SEED,
        C.ITER, horizon, mu, nu, A, B)
    scores = _eval_rows(parents, mu, nu, A, B, C.SIBLING_SEED, C.ITER,
                        horizon)
    assert scores.unique().numel() == 3           # the rows really differ
    assert torch.equal(fit, scores[torch.tensor(pidx, device=_dev())])
    assert float(stat[8]) == len(pidx) * 64 * horizon


# ---- 3. a mixed launch against the fp64 rollout oracle -----------------------

@requires_gpu
@pytest.mark.parametrize("seed,gen,h", C.MIXED_LAUNCHES)
def test_mixed_launch_against_the_rollout_oracle(seed, gen, h):
    """Every one of the MIXED_POP * 64 episodes is decided through h steps
    (the oracle says so from its own numbers), so every member's fitness and
    the obs statistics are compared in full."""
    from fiber_amd import ops

    ros = C.mixed_launch(seed, gen)
    assert len(ros) == C.MIXED_POP
    assert all(ro.decided[:, h - 1].all() for ro in ros)
    _theta, mu, nu, A, B = _device_member_args()
    fit, stat = ops.ga_rollout_mlp(
        _to_dev(C.parent_rows()), _i32(C.MIXED_PARENT_IDX),
        _i32(C.MIXED_SLOT), C.MIXED_SIGMA, seed, gen, h, mu, nu, A, B)
    fit, stat = _f64(fit), _f64(stat)
    for m, ro in enumerate(ros):
        want, tol = rollout_oracle.fitness_of(ro, h)
        print("seed %d gen %d h %d member %d: fitness err %.3e tol %.3e"
              % (seed, gen, h, m, abs(fit[m] - want), tol))
        assert abs(fit[m] - want) <= tol, (m, fit[m], want, tol)
    st = rollout_oracle.obs_stats(ros, h)
    want = np.concatenate([st.sum, st.sumsq])
    tol = rollout_oracle.obs_stats_tol(st)
    print("   stats max err/tol %.3f" % (np.abs(stat[:8] - want) / tol).max())
    assert (np.abs(stat[:8] - want) <= tol).all(), (stat, want, tol)
    assert stat[8] == C.MIXED_POP * 64 * h


# ---- 4. ga_truncate ------------------------------------------------------------

def _check_truncate(f):
    from fiber_amd import ops

    n = f.size
    full = go.truncate_exact(f, n)
    fd = _to_dev(f)
    for T in C.truncate_ts(n):
        got = ops.ga_truncate(fd, T)
        assert got.dtype == torch.int32 and got.shape == (T,)
        assert np.array_equal(got.cpu().numpy(), full[:T]), (n, T)


@requires_gpu
@pytest.mark.parametrize("n", C.TRUNCATE_SIZES)
def test_truncate_matches_the_order_rule(n):
    _check_truncate(C.fitness_random(n))


@requires_gpu
def test_truncate_with_ties_nans_and_special_values():
    _check_truncate(C.fitness_ties())
    _check_truncate(C.fitness_special())
    # all equal: the order is the index order; all NaN likewise
    for value in (1.0, float("nan")):
        _check_truncate(np.full(300, value, dtype=np.float32))


@requires_gpu
def test_truncate_at_the_largest_population():
    from fiber_amd import ops

    n = C.TRUNCATE_MAX
    f = C.fitness_random(n).copy()
    f[::7] = f[3]                                  # ties across every tile
    f[5::1001] = np.nan
    got = ops.ga_truncate(_to_dev(f), n // 2)
    assert np.array_equal(got.cpu().numpy(), go.truncate_exact(f, n // 2))


# ---- 5. ga_parents ---------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("pop,n_elite,T_cur", C.PARENT_CASES)
def test_parents_match_the_numpy_mirror(pop, n_elite, T_cur):
    from fiber_amd import ops

    pidx, slot = ops.ga_parents(C.PARENT_SEED, C.PARENT_GEN, pop, n_elite,
                                T_cur, _dev())
    want_pidx, want_slot = go.parents_exact(C.PARENT_SEED, C.PARENT_GEN, pop,
                                            n_elite, T_cur)
    assert pidx.dtype == slot.dtype == torch.int32
    assert np.array_equal(pidx.cpu().numpy(), want_pidx)
    assert np.array_equal(slot.cpu().numpy(), want_slot)


# ---- 6. ga_survivors ---------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("T,horizon", [(4, 8), (C.MIXED_POP, 1)])
def test_survivors_are_the_weights_the_members_were_scored_with(T, horizon):
    from fiber_amd import ops

    seed, gen = C.MIXED_LAUNCHES[0][:2]
    _theta, mu, nu, A, B = _device_member_args()
    parents = _to_dev(C.parent_rows())
    pidx, slot = _i32(C.MIXED_PARENT_IDX), _i32(C.MIXED_SLOT)
    fit, _stat = ops.ga_rollout_mlp(parents, pidx, slot, C.MIXED_SIGMA, seed,
                                    gen, horizon, mu, nu, A, B)
    order = ops.ga_truncate(fit, T)
    # NPARAMS = 4 * 1152 + 2: the last parameter block has two live lanes,
    # and the row after the last one must stay as it is
    buf = torch.full((T + 1, ops.NPARAMS), float("nan"), device=_dev())
    new = ops.ga_survivors(parents, pidx, slot, order, C.MIXED_SIGMA, seed,
                           gen, out=buf[:T])
    assert new.data_ptr() == buf.data_ptr()
    assert torch.isnan(buf[T]).all()
    assert torch.isfinite(buf[:T]).all()
    scores = _eval_rows(new, mu, nu, A, B, seed, gen, horizon)
    assert torch.equal(scores, fit[order.long()])
    before = parents.clone()
    for t, m in enumerate(order.tolist()):
        row = parents[C.MIXED_PARENT_IDX[m]]
        if C.MIXED_SLOT[m] < 0:
            assert torch.equal(new[t], row)
        else:
            assert int((new[t] != row).sum()) > ops.NPARAMS // 2
    assert torch.equal(parents, before)           # out of place
    if T == C.MIXED_POP:
        assert sorted(order.tolist()) == list(range(T))


# ---- 7-9. the engine ---------------------------------------------------------------

@pytest.fixture(scope="module")
def engine_run():
    """GAEngine, pop 16, truncation 4, 5 generations: the engine and what
    every generation launched, chose and left behind."""
    from fiber_amd.es import GAConfig, GAEngine

    eng = GAEngine(GAConfig(**C.ENGINE), device=_dev())
    history = []
    for _ in range(C.ENGINE_GENERATIONS):
        before = eng.lineage.cpu().numpy().copy()
        t_cur = eng.parents.shape[0]
        stats = eng.step()
        history.append({
            "lineage_before": before, "T_cur": t_cur, "stats": stats,
            "fitness": eng.last["fitness"].cpu().numpy().copy(),
            "parent_idx": eng.last["parent_idx"].cpu().numpy().copy(),
            "slot": eng.last["slot"].cpu().numpy().copy(),
            "order": eng.last["order"].cpu().numpy().copy(),
            "lineage": eng.lineage.cpu().numpy().copy(),
            "parents": eng.parents.clone()})
    return eng, history


@requires_gpu
def test_decode_rebuilds_the_parents_bit_for_bit(engine_run):
    from fiber_amd import ops

    eng, history = engine_run
    cfg, G, T = eng.cfg, C.ENGINE_GENERATIONS, C.ENGINE["truncation"]
    assert eng.generation == G and eng.parents.shape == (T, ops.NPARAMS)
    chains = eng.lineage[:, :G].contiguous()
    rows = chains.cpu().numpy()
    print("seed chains after %d generations:\n%s" % (G, rows))
    assert any((r < 0).any() for r in rows), "no chain passed an elite step"
    assert any((r >= 0).all() for r in rows), "no chain is mutated throughout"
    assert np.array_equal(np.stack([eng.genome(t).numpy() for t in range(T)]),
                          rows)
    # the guard row after the last one stays as it is
    buf = torch.full((T + 1, ops.NPARAMS), float("nan"), device=_dev())
    got = ops.ga_decode(eng.theta0, chains, cfg.sigma, cfg.seed, out=buf[:T])
    assert torch.isnan(buf[T]).all()
    assert torch.equal(got, eng.parents)
    assert torch.equal(eng.decode(chains), eng.parents)
    assert torch.equal(eng.decode(rows[1].tolist())[0], eng.parents[1])
    assert torch.equal(eng.theta, eng.parents[0])
    # every earlier generation too: the fold is the same, column by column
    for g, h in enumerate(history):
        assert torch.equal(eng.decode(h["lineage"][:, : g + 1]),
                           h["parents"]), g
    value, tol = go.decode_fp64(eng.theta0.cpu().numpy(), rows, cfg.sigma,
                                cfg.seed)
    diff = np.abs(_f64(got) - value)
    print("ga_decode max err %.3e, max tol %.3e" % (diff.max(), tol.max()))
    assert (diff <= tol).all()
    assert tol.max() < 1e-6                        # rounding-sized


@requires_gpu
def test_engine_bookkeeping_matches_the_oracle(engine_run):
    eng, history = engine_run
    cfg = eng.cfg
    for g, h in enumerate(history):
        t_cur = h["T_cur"]
        assert t_cur == (1 if g == 0 else cfg.truncation)
        pidx, slot = go.parents_exact(cfg.seed, g, cfg.pop,
                                      min(cfg.n_elite, t_cur), t_cur)
        assert np.array_equal(h["parent_idx"], pidx), g
        assert np.array_equal(h["slot"], slot), g
        order = go.truncate_exact(h["fitness"], cfg.truncation)
        assert np.array_equal(h["order"], order), g
        want = go.lineage_step(h["lineage_before"], pidx, slot, order, g)
        assert np.array_equal(h["lineage"][:, : g + 1], want), g
        assert (h["lineage"][:, g + 1:] == -1).all()
        stats = h["stats"]
        assert stats["generation"] == g + 1
        assert stats["fitness_max"] == float(h["fitness"].max())
        assert stats["elite_fitness"] == float(h["fitness"][0])
        assert stats["rollouts"] == cfg.pop * 64
        assert stats["env_steps"] == cfg.pop * 64 * cfg.horizon
    assert np.isfinite(history[-1]["fitness"]).all()


@requires_gpu
def test_checkpoint_stores_chains_and_resumes_bit_for_bit(tmp_path):
    from fiber_amd import ops
    from fiber_amd.es import GAConfig, GAEngine

    cfg = GAConfig(**C.ENGINE)
    run = GAEngine(cfg, device=_dev())
    for _ in range(3):
        run.step()
    path = str(tmp_path / "ga.pt")
    run.save(path)
    state = torch.load(path, weights_only=False)
    assert "parents" not in state
    assert state["lineage"].shape == (cfg.truncation, 3)
    assert state["lineage"].dtype == torch.int32
    assert state["theta0"].shape == (ops.NPARAMS,)

    resumed = GAEngine(GAConfig(**C.ENGINE), device=_dev())
    resumed.load(path)
    assert resumed.generation == 3
    assert torch.equal(resumed.parents, run.parents)
    assert torch.equal(resumed.lineage[:, :3], run.lineage[:, :3])
    for name in ("obs_sum", "obs_sumsq", "obs_count", "obs_mu", "obs_nu"):
        assert torch.equal(getattr(resumed, name), getattr(run, name)), name
    run.step()
    resumed.step()
    assert torch.equal(resumed.last["fitness"], run.last["fitness"])
    assert torch.equal(resumed.parents, run.parents)
    assert torch.equal(resumed.lineage, run.lineage)

    # chains drawn with another sigma or seed are refused, not misread
    other = GAEngine(GAConfig(sigma=0.03, **C.ENGINE), device=_dev())
    with pytest.raises(ValueError):
        other.load(path)
    from fiber_amd.es import ESConfig, ESEngine

    plain = ESEngine(ESConfig(pop_per_gpu=8, horizon=2), device=_dev())
    with pytest.raises(ValueError):
        resumed.load_state_dict(plain.state_dict())


@requires_gpu
def test_checkpoint_with_another_truncation_breeds_from_the_saved_rows():
    """load_state_dict compares sigma and seed only.  A checkpoint with 4
    chains loaded into an engine of truncation 3 gives 4 parents; the next
    step breeds from those 4 and leaves 3."""
    from fiber_amd.es import GAConfig, GAEngine

    run = GAEngine(GAConfig(**C.ENGINE), device=_dev())
    run.step()
    run.step()
    other = GAEngine(GAConfig(pop=12, truncation=3, n_elite=2, horizon=2),
                     device=_dev())
    other.load_state_dict(run.state_dict())
    assert other.generation == 2
    assert torch.equal(other.parents, run.parents)
    other.step()
    cfg = other.cfg
    pidx, slot = go.parents_exact(cfg.seed, 2, cfg.pop, cfg.n_elite, 4)
    assert np.array_equal(other.last["parent_idx"].cpu().numpy(), pidx)
    assert np.array_equal(other.last["slot"].cpu().numpy(), slot)
    assert other.parents.shape[0] == other.lineage.shape[0] == 3
    assert torch.equal(other.decode(other.lineage[:, :3]), other.parents)


@requires_gpu
def test_lineage_capacity_doubles_when_full():
    from fiber_amd.es import GAConfig, GAEngine

    eng = GAEngine(GAConfig(pop=4, truncation=2, horizon=1), device=_dev())
    assert eng.lineage.shape == (1, 8)
    for _ in range(9):
        eng.step()
    assert eng.lineage.shape == (2, 16) and eng.generation == 9
    assert torch.equal(eng.decode(eng.lineage[:, :9]), eng.parents)


# ---- 10. it learns -------------------------------------------------------------------

@requires_gpu
def test_thirty_generations_improve_on_theta0():
    """Defaults but pop 256, truncation 16, horizon 32.  Deterministic with
    the fixed seeds.  On an MI355X (profiles/ga.md): evaluate(iteration=0)
    22.974325 for theta0, 31.241808 for theta after 30 generations, and
    23.980198 for theta0 under the normaliser learned over the run."""
    from fiber_amd.es import GAConfig, GAEngine

    eng = GAEngine(GAConfig(**C.LEARN), device=_dev())
    start = float(eng.evaluate(iteration=0))
    assert torch.equal(eng.theta, eng.theta0)
    for _ in range(C.LEARN_GENERATIONS):
        stats = eng.step()
    final = float(eng.evaluate(iteration=0))
    # start and final differ in the normaliser too (initial against learned).
    # theta0 under the learned one separates selection from that drift: the
    # same normaliser, environment and start states on both sides.
    from fiber_amd import ops

    drift = float(ops.es_eval_matrix(
        eng.theta0.unsqueeze(0), eng.obs_mu.unsqueeze(0),
        eng.obs_nu.unsqueeze(0), eng.env_A.unsqueeze(0),
        eng.env_B.unsqueeze(0), eng.cfg.seed, 0, eng.cfg.horizon))
    print("GA pop 256 T 16 h 32, 30 generations: evaluate(iteration=0) "
          "theta0 %.6f -> theta %.6f (last fitness_max %.6f); theta0 under "
          "the learned normaliser %.6f"
          % (start, final, stats["fitness_max"], drift))
    assert final > start
    assert final > drift


# ---- validation ------------------------------------------------------------------------

@requires_gpu
def test_ops_validate_before_launching():
    from fiber_amd import ops

    dev = _dev()
    theta, mu, nu, A, B = _device_member_args()
    parents = _to_dev(C.parent_rows())
    pidx, slot = _i32([0, 1, 2, 0]), _i32([-1, 1, 2, 3])

    def rollout(parents=parents, pidx=pidx, slot=slot, sigma=0.05, horizon=2,
                mu=mu, A=A):
        return ops.ga_rollout_mlp(parents, pidx, slot, sigma, 1, 0, horizon,
                                  mu, nu, A, B)

    fit, _stat = rollout()
    for bad in (dict(parents=parents.double()), dict(parents=parents.cpu()),
                dict(pidx=pidx.long()), dict(slot=slot.float()),
                dict(slot=slot.cpu()), dict(parents=parents[:, ::2]),
                dict(mu=mu.cpu()), dict(A=A.t())):
        with pytest.raises(TypeError):
            rollout(**bad)
    for bad in (dict(parents=parents[:, :-1].contiguous()),
                dict(parents=parents[0]), dict(slot=slot[:3].contiguous()),
                dict(pidx=pidx.view(2, 2)), dict(horizon=0),
                dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(mu=mu[:3].contiguous())):
        with pytest.raises(ValueError):
            rollout(**bad)

    for bad_t in (0, 5):
        with pytest.raises(ValueError):
            ops.ga_truncate(fit, bad_t)
    with pytest.raises(ValueError):
        ops.ga_truncate(fit[:1].contiguous(), 1)
    with pytest.raises(ValueError):
        ops.ga_truncate(torch.zeros(65537, device=dev), 1)
    with pytest.raises(ValueError):
        ops.ga_truncate(fit.view(2, 2), 1)
    with pytest.raises(TypeError):
        ops.ga_truncate(fit.double(), 1)

    with pytest.raises(ValueError):
        ops.ga_parents(1, 0, 8, 2, 1, dev)         # n_elite > T_cur
    with pytest.raises(ValueError):
        ops.ga_parents(1, 0, 0, 0, 1, dev)

    order = ops.ga_truncate(fit, 2)
    with pytest.raises(ValueError):                # in place
        ops.ga_survivors(parents, pidx, slot, order, 0.05, 1, 0,
                         out=parents[:2])
    with pytest.raises(ValueError):
        ops.ga_survivors(parents, pidx, slot, order, 0.05, 1, 0,
                         out=torch.empty(3, ops.NPARAMS, device=dev))
    with pytest.raises(TypeError):
        ops.ga_survivors(parents, pidx, slot, order.long(), 0.05, 1, 0)
    with pytest.raises(ValueError):                # more survivors than pop
        ops.ga_survivors(parents, pidx, slot, _i32([0, 1, 2, 3, 0]), 0.05, 1,
                         0)

    chains = torch.zeros(2, 3, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.ga_decode(theta[:-1].contiguous(), chains, 0.05, 1)
    with pytest.raises(ValueError):
        ops.ga_decode(theta, chains[0], 0.05, 1)
    with pytest.raises(TypeError):
        ops.ga_decode(theta, chains.long(), 0.05, 1)
    with pytest.raises(ValueError):
        ops.ga_decode(theta, chains, float("inf"), 1)
    # no generations: copies of theta0
    none = ops.ga_decode(theta, chains[:, :0].contiguous(), 0.05, 1)
    assert torch.equal(none, theta.expand(2, -1))
