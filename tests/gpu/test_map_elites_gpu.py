"""MAP-Elites on the device: the kernels of fiber_amd/csrc/ops/me_kernels.hip
and MapElitesEngine (fiber_amd/es/map_elites.py) against their siblings, bit
for bit where the two must agree, and against the numpy oracle
(fiber_amd/es/map_elites_oracle.py; derivations in profiles/map_elites.md),
exactly.

  ga_rollout_mlp_bc  fitness / obs_stat: ga_rollout_mlp's bits; BC of mutated
                     members: es_rollout_mlp_bc's even members, bits; of
                     unmutated ones: es_eval_bc's cells, bits
  me_insert          cells_exact / insert_exact, integers and bit patterns
  me_compact         compact_exact
  me_parents         parents_exact
  engine             es_eval_bc of the stored rows returns the stored fitness
                     and BC; ArchiveMirror generation by generation;
                     ga_decode of the chains; checkpoints; illumination
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import ga_cases as GC  # noqa: E402
import map_elites_cases as C  # noqa: E402
import rollout_oracle_cases as RC  # noqa: E402
from fiber_amd.es import ga_oracle as go  # noqa: E402
from fiber_amd.es import map_elites_oracle as mo  # noqa: E402

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


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    if torch.is_tensor(a):
        a = _np(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device_member_args():
    return [_to_dev(a) for a in RC.member_args()]


# ---- 1. ga_rollout_mlp_bc against its siblings -------------------------------

@requires_gpu
@pytest.mark.parametrize("horizon", C.SIBLING_HORIZONS)
def test_rollout_bc_carries_its_siblings_bits(horizon):
    from fiber_amd import ops

    seed, gen = GC.SIBLING_SEED, GC.ITER
    theta, mu, nu, A, B = _device_member_args()
    parents = _to_dev(GC.parent_rows())
    pop = GC.MIXED_POP
    assert pop == 8

    # the mixed launch: fitness and obs_stat are ga_rollout_mlp's
    pidx, slot = _i32(GC.MIXED_PARENT_IDX), _i32(GC.MIXED_SLOT)
    fit, stat, bc, final = ops.ga_rollout_mlp_bc(
        parents, pidx, slot, GC.MIXED_SIGMA, seed, gen, horizon, mu, nu, A,
        B, return_final_states=True)
    want_fit, want_stat = ops.ga_rollout_mlp(
        parents, pidx, slot, GC.MIXED_SIGMA, seed, gen, horizon, mu, nu, A, B)
    assert fit.shape == (pop,) and stat.shape == (9,) and bc.shape == (pop, 4)
    assert final.shape == (pop, 64, 4)
    assert torch.equal(fit, want_fit) and torch.equal(stat, want_stat)
    assert torch.isfinite(bc).all() and bc.unique().numel() > pop
    # the BC is the mean of the final states (64 addends: 1e-5 is loose)
    assert torch.allclose(bc, final.mean(dim=1), rtol=0, atol=1e-5)
    again = ops.ga_rollout_mlp_bc(parents, pidx, slot, GC.MIXED_SIGMA, seed,
                                  gen, horizon, mu, nu, A, B)
    assert len(again) == 3 and torch.equal(again[2], bc)

    # mutated members of one parent row: es_rollout_mlp_bc's even members
    fit, stat, bc = ops.ga_rollout_mlp_bc(
        theta.unsqueeze(0), _i32([0] * pop), _i32(range(pop)),
        C.SIBLING_SIGMA, seed, gen, horizon, mu, nu, A, B)
    es_fit, _stat, es_bc = ops.es_rollout_mlp_bc(
        theta, C.SIBLING_SIGMA, seed, gen, horizon, 0, 2 * pop, mu, nu, A, B)
    assert torch.equal(bc, es_bc[0::2]) and torch.equal(fit, es_fit[0::2])
    assert bc.unique(dim=0).shape[0] == pop

    # unmutated members: es_eval_bc's cells
    upidx = GC.UNMUTATED_PARENT_IDX
    fit, stat, bc = ops.ga_rollout_mlp_bc(
        parents, _i32(upidx), _i32([-1] * len(upidx)), C.SIBLING_SIGMA, seed,
        gen, horizon, mu, nu, A, B)
    K = parents.shape[0]
    scores, ev_bc = ops.es_eval_bc(
        parents, mu.expand(K, 4).contiguous(), nu.expand(K, 4).contiguous(),
        A.unsqueeze(0), B.unsqueeze(0), seed, gen, horizon)
    rows = torch.tensor(upidx, device=_dev())
    assert torch.equal(bc, ev_bc[:, 0][rows])
    assert torch.equal(fit, scores[:, 0][rows])
    assert ev_bc[:, 0].unique(dim=0).shape[0] == K


# ---- 2. me_insert ------------------------------------------------------------------

def _run_insert(case):
    from fiber_amd import ops

    arch_fit = _to_dev(case["arch_fitness"])
    arch_bc = _to_dev(case["arch_bc"])
    arch_filled = _to_dev(case["arch_filled"])
    cell, winner, order = ops.me_insert(
        _to_dev(case["fitness"]), _to_dev(case["bc"]), case["bins"],
        case["lo"], case["hi"], arch_fit, arch_bc, arch_filled)
    assert cell.dtype == winner.dtype == order.dtype == torch.int32
    return dict(cell=_np(cell), winner=_np(winner), order=_np(order),
                arch_fitness=_np(arch_fit), arch_bc=_np(arch_bc),
                arch_filled=_np(arch_filled))


def _assert_insert_equal(got, want):
    for key in ("cell", "winner", "order", "arch_filled"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("arch_fitness", "arch_bc"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key


@requires_gpu
@pytest.mark.parametrize("case", C.insert_cases(),
                         ids=[c["name"] for c in C.insert_cases()])
def test_insert_equals_the_oracle(case):
    _assert_insert_equal(_run_insert(case), C.insert_expected(case))


@requires_gpu
def test_insert_does_not_depend_on_scheduling():
    cases = {c["name"]: c for c in C.insert_cases()}
    for name in ("ties1000-2x2-empty", "ties1000-2x2-half",
                 "pop1000-4x4x1x1-half"):
        first, second = _run_insert(cases[name]), _run_insert(cases[name])
        _assert_insert_equal(first, second)


# ---- 3. me_compact -------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("size", C.COMPACT_SIZES)
def test_compact_equals_the_oracle(size):
    from fiber_amd import ops

    for pattern in C.COMPACT_PATTERNS:
        flags = C.compact_flags(size, pattern)
        want_idx, want_n = mo.compact_exact(flags)
        # a guard element behind the list stays as it is
        buf = torch.full((size + 1,), 77, dtype=torch.int32, device=_dev())
        idx, n = ops.me_compact(_to_dev(flags), out_filled_idx=buf[:size])
        assert idx.data_ptr() == buf.data_ptr() and int(buf[size]) == 77
        assert n.dtype == torch.int32 and n.shape == (1,)
        assert int(n) == want_n, pattern
        assert np.array_equal(_np(idx), want_idx), pattern


# ---- 4. me_parents ----------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("pop,n", C.PARENT_CASES)
def test_parents_equal_the_oracle(pop, n):
    from fiber_amd import ops

    idx, padded = C.parent_filled(n)
    root = padded.size
    pidx, slot = ops.me_parents(C.PARENT_SEED, C.PARENT_GEN, pop,
                                _to_dev(padded), _i32([n]), root)
    want_pidx, want_slot = mo.parents_exact(C.PARENT_SEED, C.PARENT_GEN, pop,
                                            idx, root)
    assert pidx.dtype == slot.dtype == torch.int32
    assert np.array_equal(_np(pidx), want_pidx)
    assert np.array_equal(_np(slot), want_slot)
    if n == 0:
        assert (_np(pidx) == root).all()


# ---- 5-6. the engine --------------------------------------------------------------------

def _state(eng):
    g = eng.generation
    return {
        "arch_theta": eng.arch_theta.clone(),
        "arch_fitness": _np(eng.arch_fitness).copy(),
        "arch_bc": _np(eng.arch_bc).copy(),
        "arch_filled": _np(eng.arch_filled).copy(),
        "arch_born": _np(eng.arch_born).copy(),
        "lineage": _np(eng.lineage[:, :g]).copy(),
        "filled_idx": _np(eng.filled_idx).copy(),
        "n_filled": int(eng.n_filled),
    }


@pytest.fixture(scope="module")
def engine_run():
    """MapElitesEngine, pop 16, 4 x 4 cells, 5 generations: the engine and
    what every generation launched, chose and left behind."""
    from fiber_amd.es import MapElitesConfig, MapElitesEngine

    eng = MapElitesEngine(MapElitesConfig(**C.ENGINE), device=_dev())
    history = []
    for _ in range(C.ENGINE_GENERATIONS):
        mu, nu = eng.obs_mu.clone(), eng.obs_nu.clone()
        stats = eng.step()
        h = _state(eng)
        h.update(stats=stats, obs_mu=mu, obs_nu=nu,
                 **{k: _np(v).copy() for k, v in eng.last.items()})
        history.append(h)
    return eng, history


@requires_gpu
def test_the_stored_elite_is_what_was_scored(engine_run):
    """After generation 0 (the initial normaliser) es_eval_bc of the filled
    rows at (seed, 0, horizon) returns the stored fitness and BC: the
    winner, its BC and the materialised weights belong together."""
    from fiber_amd import ops

    eng, history = engine_run
    cfg, h = eng.cfg, history[0]
    assert torch.equal(h["obs_mu"], torch.zeros(4, device=_dev()))
    assert torch.equal(h["obs_nu"], torch.ones(4, device=_dev()))
    cells = np.flatnonzero(h["arch_filled"])
    assert cells.size == h["n_filled"] >= 1
    rows = h["arch_theta"][torch.from_numpy(cells).to(_dev())].contiguous()
    K = rows.shape[0]
    scores, bc = ops.es_eval_bc(
        rows, h["obs_mu"].expand(K, 4).contiguous(),
        h["obs_nu"].expand(K, 4).contiguous(), eng.env_A.unsqueeze(0),
        eng.env_B.unsqueeze(0), cfg.seed, 0, cfg.horizon)
    assert np.array_equal(_bits(scores[:, 0]), _bits(h["arch_fitness"][cells]))
    assert np.array_equal(_bits(bc[:, 0]), _bits(h["arch_bc"][cells]))
    # the root row and the rows of empty cells are theta0
    empty = np.flatnonzero(h["arch_filled"] == 0).tolist() + [eng.cells]
    for c in empty:
        assert torch.equal(h["arch_theta"][c], eng.theta0)
    if K > 1:
        assert rows.unique(dim=0).shape[0] == K


@requires_gpu
def test_engine_bookkeeping_matches_the_mirror(engine_run):
    eng, history = engine_run
    cfg, Cn = eng.cfg, eng.cells
    mirror = mo.ArchiveMirror(cfg.seed, cfg.pop, cfg.bins)
    aliasing = []
    for g, h in enumerate(history):
        out = mirror.step(h["fitness"], h["bc"])
        if g == 0:
            assert mirror.lo == eng.bc_lo and mirror.hi == eng.bc_hi
        for key in ("parent_idx", "slot", "cell", "winner"):
            assert np.array_equal(h[key], out[key]), (g, key)
        assert np.array_equal(h["arch_filled"], mirror.arch_filled), g
        assert np.array_equal(h["arch_born"], mirror.arch_born), g
        on = mirror.arch_filled != 0
        assert np.array_equal(_bits(h["arch_fitness"][on]),
                              _bits(mirror.arch_fitness[on])), g
        assert np.array_equal(_bits(h["arch_bc"][on]),
                              _bits(mirror.arch_bc[on])), g
        assert np.array_equal(h["filled_idx"], mirror.filled_idx), g
        assert h["n_filled"] == mirror.n_filled, g
        assert np.array_equal(h["lineage"], mirror.lineage()), g
        aliasing.append(C.aliasing_cells(h["winner"], h["parent_idx"], Cn))
        stats = h["stats"]
        assert stats["generation"] == g + 1
        assert stats["coverage"] == mirror.n_filled / Cn
        assert stats["inserted"] == int((out["winner"] >= 0).sum())
        assert stats["fitness_max"] == float(mirror.arch_fitness[on].max())
        assert stats["rollouts"] == cfg.pop * 64
        assert stats["env_steps"] == cfg.pop * 64 * cfg.horizon
        qd = float(mirror.arch_fitness[on].astype(np.float64).sum())
        assert abs(stats["qd_score"] - qd) <= 1e-5 * max(1.0, abs(qd))
    print("cells whose new elite descends from a cell replaced in the same "
          "generation, by generation:", aliasing)
    assert any(aliasing), "the aliasing hazard did not occur: pick a seed"

    # the chains rebuild the weights bit for bit, every generation
    for g, h in enumerate(history):
        assert torch.equal(eng.decode(h["lineage"]), h["arch_theta"]), g
    G = C.ENGINE_GENERATIONS
    cells = np.flatnonzero(history[-1]["arch_filled"])
    chains = np.stack([_np(eng.genome(c)) for c in cells])
    assert np.array_equal(chains, history[-1]["lineage"][cells])
    got = eng.decode(chains)
    assert torch.equal(got, eng.arch_theta[torch.from_numpy(cells).to(_dev())])
    value, tol = go.decode_fp64(_np(eng.theta0), chains, cfg.sigma, cfg.seed)
    diff = np.abs(_np(got).astype(np.float64) - value)
    print("ga_decode of the elites: max err %.3e, max tol %.3e"
          % (diff.max(), tol.max()))
    assert (diff <= tol).all()
    assert tol.max() < 1e-6                        # rounding-sized
    assert chains.shape[1] == G

    # the public accessors
    best = eng.best_cell()
    on = history[-1]["arch_filled"] != 0
    assert history[-1]["arch_fitness"][best] == \
        history[-1]["arch_fitness"][on].max()
    assert torch.equal(eng.theta, eng.arch_theta[best])
    theta, fitness, bc, genome = eng.elite(best)
    assert torch.equal(theta, eng.arch_theta[best])
    assert fitness == float(history[-1]["arch_fitness"][best])
    assert np.array_equal(_bits(bc), _bits(history[-1]["arch_bc"][best]))
    assert torch.equal(genome, eng.genome(best))
    assert torch.isfinite(eng.evaluate()).all()
    empty = np.flatnonzero(~on)
    if empty.size:
        with pytest.raises(KeyError):
            eng.elite(int(empty[0]))
    with pytest.raises(IndexError):
        eng.genome(Cn)


# ---- 7. checkpoint ----------------------------------------------------------------------

def _assert_same_state(a, b):
    sa, sb = _state(a), _state(b)
    assert a.generation == b.generation
    assert a.bc_lo == b.bc_lo and a.bc_hi == b.bc_hi
    for key in sa:
        if key == "arch_theta":
            assert torch.equal(sa[key], sb[key]), key
        elif key in ("arch_fitness", "arch_bc"):
            on = sa["arch_filled"] != 0
            assert np.array_equal(_bits(sa[key][on]), _bits(sb[key][on])), key
        else:
            assert np.array_equal(sa[key], sb[key]), key
    for name in ("obs_sum", "obs_sumsq", "obs_count", "obs_mu", "obs_nu"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@requires_gpu
def test_checkpoint_stores_chains_and_resumes_bit_for_bit(tmp_path):
    from fiber_amd.es import ESConfig, ESEngine
    from fiber_amd.es import MapElitesConfig, MapElitesEngine

    run = MapElitesEngine(MapElitesConfig(**C.ENGINE), device=_dev())
    for _ in range(3):
        run.step()
    path = str(tmp_path / "me.pt")
    run.save(path)
    state = torch.load(path, weights_only=False)
    assert "arch_theta" not in state
    assert state["me_lineage"].shape == (run.cells + 1, 3)
    assert state["me_lineage"].dtype == torch.int32
    assert state["bc_lo"] == run.bc_lo and state["bc_hi"] == run.bc_hi

    resumed = MapElitesEngine(MapElitesConfig(**C.ENGINE), device=_dev())
    resumed.load(path)
    _assert_same_state(resumed, run)
    for _ in range(2):
        run.step()
        resumed.step()
        assert torch.equal(resumed.last["fitness"], run.last["fitness"])
        assert torch.equal(resumed.last["bc"], run.last["bc"])
    _assert_same_state(resumed, run)
    assert run.generation == 5

    # an archive drawn with another sigma or seed, or on another grid, is
    # refused, not misread
    for other in (dict(C.ENGINE, sigma=0.03),
                  dict(C.ENGINE, seed=C.ENGINE_SEED + 1),
                  dict(C.ENGINE, bins=(4, 2, 2, 1))):
        eng = MapElitesEngine(MapElitesConfig(**other), device=_dev())
        with pytest.raises(ValueError):
            eng.load(path)
    plain = ESEngine(ESConfig(pop_per_gpu=8, horizon=2), device=_dev())
    with pytest.raises(ValueError):
        resumed.load_state_dict(plain.state_dict())


@requires_gpu
def test_lineage_capacity_doubles_when_full():
    from fiber_amd.es import MapElitesConfig, MapElitesEngine

    eng = MapElitesEngine(
        MapElitesConfig(pop=4, bins=(2, 2, 1, 1), horizon=1), device=_dev())
    assert eng.lineage.shape == (5, 8)
    for _ in range(9):
        eng.step()
    assert eng.lineage.shape == (5, 16) and eng.generation == 9
    assert torch.equal(eng.decode(eng.lineage[:, :9]), eng.arch_theta)


# ---- 8. illumination ---------------------------------------------------------------------

@requires_gpu
def test_thirty_generations_illuminate_the_grid():
    """Pop 256, 8 x 8 cells, horizon 32, bounds from generation 0.
    Deterministic with the fixed seeds.  Figures of an MI355X run:
    profiles/map_elites.md."""
    from fiber_amd.es import MapElitesConfig, MapElitesEngine

    eng = MapElitesEngine(MapElitesConfig(**C.ILLUMINATE), device=_dev())
    assert torch.equal(eng.theta, eng.theta0)
    trace = []
    fit = np.full(eng.cells, -np.inf)
    for g in range(C.ILLUMINATE_GENERATIONS):
        stats = eng.step()
        filled = _np(eng.arch_filled) != 0
        now = np.where(filled, _np(eng.arch_fitness).astype(np.float64),
                       -np.inf)
        assert (now >= fit).all(), g               # no cell's fitness falls
        fit = now
        trace.append(stats)
        if g:
            assert stats["coverage"] >= trace[-2]["coverage"], g
            assert stats["fitness_max"] >= trace[-2]["fitness_max"], g
    first, last = trace[0], trace[-1]
    print("MAP-Elites pop 256, 8 x 8, h 32: coverage %.4f -> %.4f, qd-score "
          "%.3f -> %.3f, best %.6f -> %.6f, bounds lo %s hi %s"
          % (first["coverage"], last["coverage"], first["qd_score"],
             last["qd_score"], first["fitness_max"], last["fitness_max"],
             eng.bc_lo, eng.bc_hi))
    assert last["coverage"] > first["coverage"]


# ---- 9. validation -------------------------------------------------------------------------

@requires_gpu
def test_ops_validate_before_launching():
    from fiber_amd import ops

    dev = _dev()
    theta, mu, nu, A, B = _device_member_args()
    parents = _to_dev(GC.parent_rows())
    pidx, slot = _i32([0, 1, 2, 0]), _i32([-1, 1, 2, 3])

    def rollout(parents=parents, pidx=pidx, slot=slot, sigma=0.05, horizon=2,
                mu=mu, A=A):
        return ops.ga_rollout_mlp_bc(parents, pidx, slot, sigma, 1, 0,
                                     horizon, mu, nu, A, B)

    fit, _stat, bc = rollout()
    for bad in (dict(parents=parents.double()), dict(parents=parents.cpu()),
                dict(pidx=pidx.long()), dict(slot=slot.cpu()),
                dict(parents=parents[:, ::2]), dict(A=A.t())):
        with pytest.raises(TypeError):
            rollout(**bad)
    for bad in (dict(parents=parents[0]), dict(slot=slot[:3].contiguous()),
                dict(horizon=0), dict(sigma=-1.0),
                dict(sigma=float("nan")), dict(sigma=float("inf")),
                dict(mu=mu[:3].contiguous())):
        with pytest.raises(ValueError):
            rollout(**bad)

    bins, lo, hi = (2, 2, 1, 1), (-1.0,) * 4, (1.0,) * 4
    af = torch.zeros(4, device=dev)
    ab = torch.zeros(4, 4, device=dev)
    afl = torch.zeros(4, dtype=torch.int32, device=dev)

    def insert(fit=fit, bc=bc, bins=bins, lo=lo, hi=hi, af=af, ab=ab,
               afl=afl):
        return ops.me_insert(fit, bc, bins, lo, hi, af, ab, afl)

    cell, winner, order = insert()
    assert cell.shape == (4,) and winner.shape == (4,) and order.shape == (5,)
    for bad in (dict(fit=fit.double()), dict(bc=bc.cpu()),
                dict(afl=afl.long()), dict(afl=afl.bool()),
                dict(ab=ab.t()), dict(af=af.cpu())):
        with pytest.raises(TypeError):
            insert(**bad)
    for bad in (dict(bins=(2, 0, 1, 1)), dict(bins=(2, 2, 1)),
                dict(bins=(256, 256, 1, 1)), dict(bins=(4, 2, 1, 1)),
                dict(hi=(1.0, -1.0, 1.0, 1.0)), dict(hi=(1.0, -2.0, 1.0, 1.0)),
                dict(hi=(1.0, float("inf"), 1.0, 1.0)),
                dict(lo=(float("nan"), -1.0, -1.0, -1.0)),
                dict(bc=bc[:3].contiguous()), dict(fit=fit.view(2, 2)),
                dict(af=torch.zeros(5, device=dev)),
                dict(ab=torch.zeros(4, 3, device=dev))):
        with pytest.raises(ValueError):
            insert(**bad)

    with pytest.raises(TypeError):
        ops.me_compact(afl.long())
    with pytest.raises(TypeError):
        ops.me_compact(afl.cpu())
    with pytest.raises(ValueError):
        ops.me_compact(afl.view(2, 2))
    with pytest.raises(ValueError):
        ops.me_compact(torch.zeros(0, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.me_compact(torch.zeros(65535, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.me_compact(afl, out_filled_idx=torch.zeros(
            3, dtype=torch.int32, device=dev))

    fidx, n = ops.me_compact(afl)
    with pytest.raises(ValueError):
        ops.me_parents(1, 0, 0, fidx, n, 4)
    with pytest.raises(ValueError):
        ops.me_parents(1, 0, 65537, fidx, n, 4)
    with pytest.raises(ValueError):
        ops.me_parents(1, 0, 8, fidx, n, -1)
    with pytest.raises(ValueError):
        ops.me_parents(1, 0, 8, fidx, torch.zeros(2, dtype=torch.int32,
                                                  device=dev), 4)
    with pytest.raises(TypeError):
        ops.me_parents(1, 0, 8, fidx.long(), n, 4)
    with pytest.raises(TypeError):
        ops.me_parents(1, 0, 8, fidx, n.cpu(), 4)
    with pytest.raises(ValueError):
        ops.me_parents(1, 0, 8, fidx, n, 4, out_slot=torch.zeros(
            7, dtype=torch.int32, device=dev))
