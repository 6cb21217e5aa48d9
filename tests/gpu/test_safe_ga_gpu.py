"""Safe mutations on the device: the kernels of
fiber_amd/csrc/ops/sm_kernels.hip and SafeGAEngine (fiber_amd/es/safe_ga.py).

  sm_steps           the fp64 oracle (fiber_amd/es/sm_oracle.py) within its
                     own tolerance on every case of tests/sm_cases.py; row
                     independence, guard rows and repeatability in bits; the
                     cases with an exact answer, in bits
  ga_rollout_mlp_sm  with every step equal to sigma: ga_rollout_mlp, bits
  ga_survivors_sm    likewise ga_survivors, bits; with real step rows,
                     es_eval_matrix of its rows returns fitness[order], bits
  SafeGAEngine       decode, checkpoint, repeatability, the probe
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import ga_cases as GC  # noqa: E402
import rollout_oracle_cases as RC  # noqa: E402
import sm_cases as C  # noqa: E402

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


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _device_member_args():
    return [_to_dev(a) for a in RC.member_args()]


def _eval_rows(rows, mu, nu, A, B, seed, gen, h):
    from fiber_amd import ops

    K = rows.shape[0]
    return ops.es_eval_matrix(
        rows, mu.expand(K, 4).contiguous(), nu.expand(K, 4).contiguous(),
        A.unsqueeze(0), B.unsqueeze(0), seed, gen, h)[:, 0]


# ---- 1. sm_steps against the oracle -------------------------------------------

@requires_gpu
@pytest.mark.parametrize("probe", list(C.probes()))
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("s_min", C.S_MINS)
def test_steps_match_the_oracle_on_every_case(s_min, mode, probe):
    """All thetas of the case list as the rows of one launch."""
    from fiber_amd import ops

    names = list(C.thetas())
    rows = _to_dev(np.stack([C.thetas()[n] for n in names]))
    steps, sens = ops.sm_steps(rows, _to_dev(C.probes()[probe]), C.SIGMA,
                               s_min, mode, return_sens=True)
    assert steps.shape == sens.shape == (len(names), ops.NPARAMS)
    steps, sens = _f64(steps), _f64(sens)
    for t, name in enumerate(names):
        ratio = C.worst_ratio(steps[t], sens[t],
                              C.reference(name, probe, mode, s_min))
        print("%s / %s / %s / s_min %g: worst err / tol %.3f"
              % (name, probe, mode, s_min, ratio))
        assert ratio <= 1.0, name


@requires_gpu
@pytest.mark.parametrize("mode", C.MODES)
def test_rows_are_independent_and_repeatable(mode):
    from fiber_amd import ops

    probe = _to_dev(C.probes()["special"])
    three = _to_dev(np.stack([C.thetas()[n]
                              for n in ("asymA", "init1234", "asymB")]))
    T = 3
    assert T in C.ROW_COUNTS and 1 in C.ROW_COUNTS
    # guard rows on both sides of out keep their bits
    buf = torch.full((T + 2, ops.NPARAMS), float("nan"), device=_dev())
    got, sens = ops.sm_steps(three, probe, C.SIGMA, 0.01, mode,
                             out=buf[1:T + 1], return_sens=True)
    assert got.data_ptr() == buf[1].data_ptr()
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[T + 1]).all()
    assert torch.isfinite(got).all() and torch.isfinite(sens).all()
    # a second launch: identical bits
    again, sens2 = ops.sm_steps(three, probe, C.SIGMA, 0.01, mode,
                                return_sens=True)
    assert torch.equal(_bits(again), _bits(got))
    assert torch.equal(_bits(sens2), _bits(sens))
    # row t alone, first of 3 and last of 3
    for t in range(T):
        alone = ops.sm_steps(three[t:t + 1].contiguous(), probe, C.SIGMA,
                             0.01, mode)
        first = ops.sm_steps(three[[t, (t + 1) % 3, (t + 2) % 3]]
                             .contiguous(), probe, C.SIGMA, 0.01, mode)
        last = ops.sm_steps(three[[(t + 1) % 3, (t + 2) % 3, t]]
                            .contiguous(), probe, C.SIGMA, 0.01, mode)
        assert torch.equal(_bits(alone[0]), _bits(got[t])), t
        assert torch.equal(_bits(first[0]), _bits(got[t])), t
        assert torch.equal(_bits(last[2]), _bits(got[t])), t
    assert not torch.equal(got[0], got[1])
    # a NaN row changes no other row
    poisoned = three.clone()
    poisoned[1] = float("nan")
    bad = ops.sm_steps(poisoned, probe, C.SIGMA, 0.01, mode)
    assert torch.equal(_bits(bad[0]), _bits(got[0]))
    assert torch.equal(_bits(bad[2]), _bits(got[2]))
    # no rows: empty results, nothing launched
    none, none_sens = ops.sm_steps(three[:0].contiguous(), probe, C.SIGMA,
                                   0.01, mode, return_sens=True)
    assert none.shape == none_sens.shape == (0, ops.NPARAMS)


# ---- 2. the cases with an exact answer ----------------------------------------

@requires_gpu
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("s_min", C.S_MINS)
def test_exact_cases(s_min, mode):
    from fiber_amd import ops

    names = ("zero", "saturating", "asymA")
    rows = _to_dev(np.stack([C.thetas()[n] for n in names]))
    steps, sens = ops.sm_steps(rows, _to_dev(C.probes()["default"]), C.SIGMA,
                               s_min, mode, return_sens=True)
    steps, sens = steps.cpu().numpy(), sens.cpu().numpy()
    sigma = np.float32(C.SIGMA)
    floor = sigma / np.float32(s_min)              # IEEE fp32 division
    # b3: sensitivity exactly 1, step exactly sigma, every row
    assert (sens[:, C.OFF_B3:] == 1.0).all()
    assert (steps[:, C.OFF_B3:].view(np.uint32)
            == sigma.view(np.uint32)).all()
    # zero theta: nothing else is felt at all
    assert (sens[0, :C.OFF_B3] == 0.0).all()
    assert (steps[0, :C.OFF_B3].view(np.uint32)
            == floor.view(np.uint32)).all()
    # saturating theta: h1 = +-1 exactly, nothing reaches W1 and b1
    assert (sens[1, :C.OFF_W2] == 0.0).all()
    assert (steps[1, :C.OFF_W2].view(np.uint32)
            == floor.view(np.uint32)).all()
    assert (sens[1, C.OFF_W3:C.OFF_B3] > 0).any()
    if mode == "sum":
        # both W3 rows see the same sum of h2
        for t in range(len(names)):
            assert np.array_equal(
                sens[t, C.OFF_W3:C.OFF_W3 + C.HID].view(np.uint32),
                sens[t, C.OFF_W3 + C.HID:C.OFF_B3].view(np.uint32)), t
        assert (sens[2, C.OFF_W3:C.OFF_B3] > 0).all()


# ---- 3. constant steps: the plain GA kernels, bits -----------------------------

def _launches():
    """(parents, parent_idx, slot, sigma, seed, gen, horizon): ga_cases'
    sibling launches and its mixed launch."""
    theta = RC.member_args()[0]
    pop = GC.SIBLING_POP
    out = []
    for horizon in GC.SIBLING_HORIZONS:
        out.append((np.asarray(theta, np.float32)[None, :], [0] * pop,
                    list(range(pop)), GC.SIBLING_SIGMAS[0], GC.SIBLING_SEED,
                    GC.ITER, horizon))
    seed, gen, _h = GC.MIXED_LAUNCHES[0]
    out.append((GC.parent_rows(), GC.MIXED_PARENT_IDX, GC.MIXED_SLOT,
                GC.MIXED_SIGMA, seed, gen, GC.MIXED_H_MAX))
    return out


@requires_gpu
@pytest.mark.parametrize("launch", range(3))
def test_constant_steps_carry_the_plain_kernels_bits(launch):
    from fiber_amd import ops

    parents, pidx, slot, sigma, seed, gen, horizon = _launches()[launch]
    _theta, mu, nu, A, B = _device_member_args()
    parents, pidx, slot = _to_dev(parents), _i32(pidx), _i32(slot)
    steps = torch.full_like(parents, sigma)
    fit, stat = ops.ga_rollout_mlp_sm(parents, steps, pidx, slot, seed, gen,
                                      horizon, mu, nu, A, B)
    want_fit, want_stat = ops.ga_rollout_mlp(parents, pidx, slot, sigma,
                                             seed, gen, horizon, mu, nu, A,
                                             B)
    assert torch.equal(_bits(fit), _bits(want_fit))
    assert torch.equal(_bits(stat), _bits(want_stat))
    assert fit.unique().numel() > 1
    T = min(4, pidx.numel())
    order = ops.ga_truncate(fit, T)
    buf = torch.full((T + 1, ops.NPARAMS), float("nan"), device=_dev())
    new = ops.ga_survivors_sm(parents, steps, pidx, slot, order, seed, gen,
                              out=buf[:T])
    want = ops.ga_survivors(parents, pidx, slot, order, sigma, seed, gen)
    assert new.data_ptr() == buf.data_ptr()
    assert torch.isnan(buf[T]).all()
    assert torch.equal(_bits(new), _bits(want))


# ---- 4. real step rows: the survivors are what was scored ---------------------

@requires_gpu
@pytest.mark.parametrize("mode", C.MODES)
def test_survivors_are_the_weights_the_members_were_scored_with(mode):
    from fiber_amd import ops

    seed, gen, _h = GC.MIXED_LAUNCHES[0]
    horizon = GC.MIXED_H_MAX
    _theta, mu, nu, A, B = _device_member_args()
    parents = _to_dev(GC.parent_rows())
    assert parents.shape[0] == 3
    pidx, slot = _i32(GC.MIXED_PARENT_IDX), _i32(GC.MIXED_SLOT)
    steps = ops.sm_steps(parents, _to_dev(C.probes()["default"]), 0.004,
                         0.01, mode)
    assert steps.unique().numel() > 1000           # really per parameter
    assert not torch.equal(steps[0], steps[1])     # and per parent
    fit, _stat = ops.ga_rollout_mlp_sm(parents, steps, pidx, slot, seed, gen,
                                       horizon, mu, nu, A, B)
    T = GC.MIXED_POP
    order = ops.ga_truncate(fit, T)
    new = ops.ga_survivors_sm(parents, steps, pidx, slot, order, seed, gen)
    scores = _eval_rows(new, mu, nu, A, B, seed, gen, horizon)
    assert torch.equal(_bits(scores), _bits(fit[order.long()]))
    before = parents.clone()
    for t, m in enumerate(order.tolist()):
        row = parents[GC.MIXED_PARENT_IDX[m]]
        if GC.MIXED_SLOT[m] < 0:
            assert torch.equal(new[t], row)
        else:
            assert int((new[t] != row).sum()) > ops.NPARAMS // 2
    assert torch.equal(parents, before)            # out of place
    # the move of a mutated member is its parent's step row times the draw
    plain = ops.ga_survivors(parents, pidx, slot, order, 1.0, seed, gen)
    for t, m in enumerate(order.tolist()):
        if GC.MIXED_SLOT[m] >= 0:
            p = GC.MIXED_PARENT_IDX[m]
            z = _f64(plain[t]) - _f64(parents[p])  # sigma = 1: the draw
            move = _f64(new[t]) - _f64(parents[p])
            assert np.allclose(move, _f64(steps[p]) * z, rtol=1e-4,
                               atol=1e-6), m


@requires_gpu
def test_ops_validate_before_launching():
    from fiber_amd import ops

    dev = _dev()
    _theta, mu, nu, A, B = _device_member_args()
    parents = _to_dev(GC.parent_rows())
    probe = _to_dev(C.probes()["default"])
    steps = ops.sm_steps(parents, probe, 0.004)
    pidx, slot = _i32([0, 1, 2, 0]), _i32([-1, 1, 2, 3])
    for bad in (dict(thetas=parents[:, :-1].contiguous()),
                dict(thetas=parents[0]), dict(probe=probe[:63].contiguous()),
                dict(probe=probe.view(4, 64)), dict(mode="so"),
                dict(s_min=0.0), dict(sigma=-1.0),
                dict(out=torch.empty(2, ops.NPARAMS, device=dev)),
                dict(out=parents)):
        args = dict(thetas=parents, probe=probe, sigma=0.004)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.sm_steps(**args)
    for bad in (dict(thetas=parents.double()), dict(probe=probe.cpu()),
                dict(thetas=parents[:, ::2]), dict(probe=probe.t())):
        args = dict(thetas=parents, probe=probe, sigma=0.004)
        args.update(bad)
        with pytest.raises(TypeError):
            ops.sm_steps(**args)
    with pytest.raises(ValueError):                # steps of another shape
        ops.ga_rollout_mlp_sm(parents, steps[:2].contiguous(), pidx, slot, 1,
                              0, 2, mu, nu, A, B)
    with pytest.raises(TypeError):
        ops.ga_rollout_mlp_sm(parents, steps.double(), pidx, slot, 1, 0, 2,
                              mu, nu, A, B)
    with pytest.raises(ValueError):
        ops.ga_rollout_mlp_sm(parents, steps, pidx, slot, 1, 0, 0, mu, nu, A,
                              B)
    order = _i32([1, 0])
    with pytest.raises(ValueError):                # in place, either input
        ops.ga_survivors_sm(parents, steps, pidx, slot, order, 1, 0,
                            out=parents[:2])
    with pytest.raises(ValueError):
        ops.ga_survivors_sm(parents, steps, pidx, slot, order, 1, 0,
                            out=steps[1:])
    with pytest.raises(ValueError):
        ops.ga_survivors_sm(parents, steps[:1].contiguous(), pidx, slot,
                            order, 1, 0)
    with pytest.raises(TypeError):
        ops.ga_survivors_sm(parents, steps, pidx, slot, order.long(), 1, 0)


# ---- 5. the engine ------------------------------------------------------------------

def _engine(mode, probe=None, **over):
    from fiber_amd.es import SafeGAConfig, SafeGAEngine

    cfg = dict(GC.ENGINE, mode=mode)
    cfg.update(over)
    return SafeGAEngine(SafeGAConfig(**cfg), device=_dev(), probe=probe)


@requires_gpu
@pytest.mark.parametrize("mode", C.MODES)
def test_engine_decodes_resumes_and_repeats_bit_for_bit(mode, tmp_path):
    from fiber_amd import ops

    G, T = GC.ENGINE_GENERATIONS, GC.ENGINE["truncation"]
    eng, twin = _engine(mode), _engine(mode)
    assert torch.equal(eng.probe.cpu(),
                       torch.from_numpy(C.probes()["default"]))
    history = []
    for g in range(G):
        if g == 3:
            path = str(tmp_path / "safe_ga.pt")
            eng.save(path)
        eng.step()
        twin.step()
        history.append((eng.lineage[:, : g + 1].clone(), eng.parents.clone(),
                        eng.last["fitness"].clone()))
        # two engines with the same config are identical
        assert torch.equal(_bits(twin.last["fitness"]),
                           _bits(eng.last["fitness"])), g
        assert torch.equal(_bits(twin.parents), _bits(eng.parents)), g
    assert eng.generation == G and eng.parents.shape == (T, ops.NPARAMS)
    assert eng.last["steps"].shape == (T, ops.NPARAMS)
    assert eng.last["steps"].unique().numel() > 1000
    rows = eng.lineage[:, :G].cpu().numpy()
    print("seed chains after %d generations:\n%s" % (G, rows))
    assert (rows >= 0).any()
    # decode(genome(t)) is parents[t], for every t, and every generation
    for t in range(T):
        got = eng.decode(eng.genome(t))
        assert got.shape == (1, ops.NPARAMS)
        assert torch.equal(_bits(got[0]), _bits(eng.parents[t])), t
    for g, (chains, parents, _fit) in enumerate(history):
        assert torch.equal(_bits(eng.decode(chains)), _bits(parents)), g
    # the plain fold of the same chains is something else
    plain = ops.ga_decode(eng.theta0, eng.lineage[:, :G].contiguous(),
                          eng.cfg.sigma, eng.cfg.seed)
    assert not torch.equal(plain, eng.parents)

    # save after 3 generations, load, run on: the same parents and fitness
    state = torch.load(path, weights_only=False)
    assert "parents" not in state
    assert state["lineage"].shape == (T, 3)
    assert state["probe"].shape == (64, 4)
    assert state["config"]["mode"] == mode
    resumed = _engine(mode)
    resumed.load(path)
    assert resumed.generation == 3
    assert torch.equal(_bits(resumed.parents), _bits(history[2][1]))
    resumed.step()
    assert torch.equal(_bits(resumed.last["fitness"]), _bits(history[3][2]))
    assert torch.equal(_bits(resumed.parents), _bits(history[3][1]))
    for other in (dict(sigma=0.004), dict(s_min=0.02), dict(seed=7)):
        with pytest.raises(ValueError):
            _engine(mode, **other).load(path)
    with pytest.raises(ValueError):
        _engine("sum" if mode == "abs" else "abs").load(path)

    # a different probe gives different parents
    other = _engine(mode, probe=torch.from_numpy(
        C.probes()["special"].copy()))
    for _ in range(2):
        other.step()
    assert not torch.equal(other.parents, history[1][1])
    with pytest.raises(ValueError, match="probe"):
        other.load(path)
