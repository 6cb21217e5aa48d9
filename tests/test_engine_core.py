"""fiber_amd/es/_core.py: every shared helper against the sequence the
engines used to carry, written out longhand here, bit for bit
(``torch.equal``); whole-engine trajectories on the CPU with the ``ops``
entry points replaced by deterministic torch fakes; and the checkpoint keys
of every engine."""

import dataclasses
import types

import pytest
import torch

import engine_core_cases as C
from fiber_amd import ops
from fiber_amd.es import (ESConfig, ESEngine, LSTMESEngine,
                          RecurrentESEngine, SNESConfig, SNESEngine,
                          WideESEngine, _core)
from fiber_amd.es.engine import init_theta, make_env_params
from fiber_amd.es.lstm import init_theta_lstm
from fiber_amd.es.recurrent import init_theta_gru
from fiber_amd.es.wide import init_theta_wide

CPU = torch.device("cpu")
N = ops.NPARAMS


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- Adam ascent -----------------------------------------------------------
def _adam_state(shape, seed):
    """theta, m, v with non-trivial moments (v >= 0)."""
    return (_randn(*shape, seed=seed), 0.1 * _randn(*shape, seed=seed + 1),
            0.01 * _randn(*shape, seed=seed + 2) ** 2)


@pytest.mark.parametrize("shape", [(N,), (2, N)])
def test_adam_three_steps(shape):
    cfg = ESConfig()
    got = _adam_state(shape, 10)
    want = [t.clone() for t in got]
    for t_step in (4, 5, 6):
        grad = _randn(*shape, seed=20 + t_step)
        _core.adam_ascent(*got, grad, t_step, cfg)
        C.longhand_adam(*want, grad, t_step, cfg)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    assert not torch.equal(got[0], _adam_state(shape, 10)[0])


def test_adam_on_a_row_view():
    cfg = ESConfig()
    got = _adam_state((3, N), 30)
    before = [t.clone() for t in got]
    want = [t[1].clone() for t in got]
    for t_step in (1, 2, 3):
        grad = _randn(N, seed=40 + t_step)
        _core.adam_ascent(got[0][1], got[1][1], got[2][1], grad, t_step, cfg)
        C.longhand_adam(*want, grad, t_step, cfg)
    for g, w, b in zip(got, want, before):
        assert torch.equal(g[1], w)            # the parent tensor moved
        assert not torch.equal(g[1], b[1])
        assert torch.equal(g[0], b[0]) and torch.equal(g[2], b[2])


# ---- normaliser ------------------------------------------------------------
class _Holder(_core.ObsNormaliser):
    def __init__(self, *lead):
        self.cfg, self.device = ESConfig(), CPU
        self._init_normaliser(*lead)


def _fields(s):
    return [getattr(s, f) for f in
            ("obs_sum", "obs_sumsq", "obs_count", "obs_mu", "obs_nu")]


def _obs_stat(lead, seed, count=512.0, spread=1.0):
    """A plausible obs_stat[..., 9]: count * mean, count * (mean^2 + var)."""
    mean = _randn(*lead, 4, seed=seed)
    var = spread * _randn(*lead, 4, seed=seed + 1) ** 2
    cnt = torch.full((*lead, 1), count)
    return torch.cat([cnt * mean, cnt * (mean ** 2 + var), cnt], dim=-1)


def test_normaliser_allocation():
    for lead in ((), (3,)):
        s = _Holder(*lead)
        assert [tuple(t.shape) for t in _fields(s)] == [
            lead + (4,), lead + (4,), lead + (1,), lead + (4,), lead + (4,)]
        assert all(t.dtype == torch.float32 for t in _fields(s))
        assert not any(t.any() for t in _fields(s)[:4])
        assert torch.equal(s.obs_nu, torch.ones(*lead, 4))


@pytest.mark.parametrize("lead, longhand", [((), C.longhand_merge_1d),
                                            ((3,), C.longhand_merge_2d)])
def test_merge_and_refresh(lead, longhand):
    got, want = _Holder(*lead), _Holder(*lead)
    for k in range(3):
        stat = _obs_stat(lead, 50 + 2 * k)
        got._merge_obs_stat(stat)
        longhand(want, stat)
        for g, w in zip(_fields(got), _fields(want)):
            assert torch.equal(g, w)
        assert got.obs_mu.is_contiguous() and got.obs_nu.is_contiguous()
    assert float(got.obs_count.reshape(-1)[0]) == 3 * 512.0


@pytest.mark.parametrize("lead", [(), (3,)])
def test_refresh_edges(lead):
    s = _Holder(*lead)
    # count == 0: the divisor is clamp_min(1.0), not 0
    s.obs_sum += 3.0
    s.obs_sumsq += 11.0
    s._refresh_normaliser()
    assert torch.equal(s.obs_mu, torch.full(lead + (4,), 3.0))
    assert torch.equal(s.obs_nu, torch.full(lead + (4,), 2.0))
    # dims 0, 1: variance under the floor (the floor exactly); dim 2: a
    # negative computed variance; dim 3: above the floor, kept
    s = _Holder(*lead)
    s.obs_count += 4.0
    s.obs_sum += torch.tensor([4.0, 8.0, 8.0, 4.0])
    s.obs_sumsq += torch.tensor([4.0, 16.02, 15.0, 6.0])
    s._refresh_normaliser()
    mu, nu = C.longhand_refresh(s.obs_sum, s.obs_sumsq, s.obs_count)
    assert torch.equal(s.obs_mu, mu) and torch.equal(s.obs_nu, nu)
    floor = torch.tensor(1e-2)
    assert (s.obs_sumsq / 4.0 - s.obs_mu ** 2)[..., 2].max() < 0
    assert torch.equal(s.obs_nu[..., :3], floor.expand(lead + (3,)))
    assert torch.equal(s.obs_nu[..., 3], torch.full(lead, 0.5))


def test_obs_state_round_trip():
    src, dst = _Holder(), _Holder()
    src._merge_obs_stat(_obs_stat((), 60))
    state = src._obs_state()
    assert list(state) == ["obs_sum", "obs_sumsq", "obs_count"]
    dst._load_obs_state(state)
    for g, w in zip(_fields(dst), _fields(src)):
        assert torch.equal(g, w)


# ---- env resolution --------------------------------------------------------
def test_env_default_is_make_env_params():
    cfg = ESConfig(seed=77)
    got = _core.resolve_env(cfg, CPU, None)
    want = make_env_params(77, CPU)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert _core.make_env_params is make_env_params


def test_env_supplied_is_copied_as_fp32():
    env_A = _randn(4, 4, seed=1).double()
    env_B = _randn(4, seed=2).double()
    got_A, got_B = _core.resolve_env(ESConfig(), CPU, (env_A, env_B))
    assert got_A.dtype == got_B.dtype == torch.float32
    assert got_A.is_contiguous() and got_B.is_contiguous()
    assert torch.equal(got_A, env_A.float())
    assert torch.equal(got_B, env_B.float())
    keep_A, keep_B = got_A.clone(), got_B.clone()
    env_A += 1.0
    env_B += 1.0
    assert torch.equal(got_A, keep_A) and torch.equal(got_B, keep_B)
    # fp32 input is copied too
    a32, b32 = _randn(4, 4, seed=3), _randn(4, seed=4)
    got_A, got_B = _core.resolve_env(ESConfig(), CPU, (a32, b32))
    a32 += 1.0
    b32 += 1.0
    assert not torch.equal(got_A, a32) and not torch.equal(got_B, b32)


@pytest.mark.parametrize("shape_A, shape_B", [((4, 3), (4,)), ((4, 4), (3,)),
                                              ((16,), (4,)),
                                              ((4, 4), (4, 1))])
def test_env_wrong_shape(shape_A, shape_B):
    with pytest.raises(ValueError) as exc:
        _core.resolve_env(ESConfig(), CPU,
                          (torch.zeros(shape_A), torch.zeros(shape_B)))
    assert str(exc.value) == "env_params must be (env_A[4][4], env_B[4])"


# ---- act() input -----------------------------------------------------------
def _act_engine():
    return types.SimpleNamespace(
        cfg=ESConfig(), theta=torch.zeros(3),
        obs_mu=_randn(4, seed=5), obs_nu=_randn(4, seed=6) ** 2 + 1e-2)


def test_act_input_checks():
    eng = _act_engine()
    with pytest.raises(TypeError) as exc:
        _core.act_input(eng, [[0.0] * 4])
    assert str(exc.value) == "obs must be a tensor, got list"
    for bad in (torch.zeros(4), torch.zeros(2, 3)):
        with pytest.raises(ValueError) as exc:
            _core.act_input(eng, bad)
        assert str(exc.value) == ("obs must be [n, 4], got %s"
                                  % (tuple(bad.shape),))
    with pytest.raises(TypeError) as exc:
        _core.act_input(eng, torch.zeros(2, 4, dtype=torch.float64))
    assert str(exc.value) == "obs must be torch.float32, got torch.float64"
    with pytest.raises(TypeError) as exc:
        _core.act_input(eng, torch.zeros(2, 4, device="meta"))
    assert str(exc.value) == "obs is on meta, the engine on cpu"


def test_act_input_values():
    eng = _act_engine()
    obs = 4.0 * _randn(33, 4, seed=7)     # far enough out to hit the clamp
    keep = obs.clone()
    rstd = torch.rsqrt(eng.obs_nu + 1e-4)
    want = ((obs - eng.obs_mu) * rstd).clamp_(-5.0, 5.0).contiguous()
    assert want.abs().max() == 5.0
    got = _core.act_input(eng, obs)
    assert torch.equal(got, want) and got.is_contiguous()
    # the recurrent engines' form, obs_mask = 0b0101: dims 0 and 2 visible
    x = ((obs - eng.obs_mu) * rstd).clamp_(-5.0, 5.0)
    visible = torch.tensor([(0b0101 >> d) & 1 for d in range(4)],
                           dtype=torch.float32, device=obs.device)
    want = (x * visible).contiguous()
    got = _core.act_input(eng, obs, 0b0101)
    assert torch.equal(got, want) and got.is_contiguous()
    assert not got[:, 1].any() and not got[:, 3].any() and got[:, 0].any()
    assert torch.equal(obs, keep)


# ---- whole-engine trajectories on the CPU ----------------------------------
CFG, STEPS = C.CFG, C.STEPS


def fake_rollout(theta, iteration, pop, obs_mu, obs_nu, salt):
    """fitness[pop], obs_stat[9]: a seeded function of (theta, iteration)
    that also feels the normaliser, as a rollout does."""
    gen = torch.Generator().manual_seed(7919 * salt + int(iteration))
    fitness = (torch.randn(pop, generator=gen) + theta[:pop]
               + (obs_mu.sum() + obs_nu.sum()) * torch.arange(pop) / pop)
    mean = torch.tensor([0.5, -1.0, 2.0, 0.0]) + 1e-3 * theta[:4]
    # dims 0 and 1 under the normaliser's floor, 2 and 3 above it
    var = torch.tensor([1e-3, 4e-3, 0.5, 2.0]) * (
        1.0 + 0.1 * torch.rand(4, generator=gen))
    cnt = torch.full((1,), float(pop * 64 * CFG.horizon))
    return fitness.contiguous(), torch.cat(
        [cnt * mean, cnt * (mean ** 2 + var), cnt])


def fake_noise(npairs, iteration, nparams):
    gen = torch.Generator().manual_seed(104729 + int(iteration))
    return torch.randn(npairs, nparams, generator=gen)


def fake_grad(wpair, iteration, nparams):
    return wpair @ fake_noise(wpair.numel(), iteration, nparams)


def fake_grad_sigma(wdiff, wsum, iteration):
    z = fake_noise(wdiff.numel(), iteration, N)
    return wdiff @ z, wsum @ (z * z - 1.0)


@pytest.fixture
def fake_ops(monkeypatch):
    """The ``ops`` entry points the five engines call, replaced by the
    fakes above; each records that it ran."""
    ran = set()

    def rollout(salt):
        def fake(theta, sigma, seed, iteration, horizon, member_offset, pop,
                 obs_mu, obs_nu, env_A, env_B, obs_mask=None):
            ran.add(salt)
            assert seed == CFG.seed and member_offset == 0
            assert salt not in (3, 4) or obs_mask == 0b0101
            return fake_rollout(theta, iteration, pop, obs_mu, obs_nu, salt)
        return fake

    def rollout_wide(theta, hidden, *rest):
        assert hidden == 128
        return rollout(5)(theta, *rest)

    def es_grad(wpair, pair_begin, pair_end, seed, iteration, device,
                nparams=None):
        assert (pair_begin, pair_end) == (0, wpair.numel())
        return fake_grad(wpair, iteration, N if nparams is None else nparams)

    def es_grad_sigma(wdiff, wsum, pair_begin, pair_end, seed, iteration,
                      device):
        return fake_grad_sigma(wdiff, wsum, iteration)

    monkeypatch.setattr(ops, "es_rollout_mlp", rollout(1))
    monkeypatch.setattr(ops, "es_rollout_mlp_sigma", rollout(2))
    monkeypatch.setattr(ops, "es_rollout_gru", rollout(3))
    monkeypatch.setattr(ops, "es_rollout_lstm", rollout(4))
    monkeypatch.setattr(ops, "es_rollout_mlp_wide", rollout_wide)
    monkeypatch.setattr(ops, "centered_rank", ops.centered_rank_ref)
    monkeypatch.setattr(ops, "es_grad", es_grad)
    monkeypatch.setattr(ops, "es_grad_sigma", es_grad_sigma)
    return ran


def longhand_run(theta, salt, snes=None):
    """STEPS iterations of the update as every engine used to spell it,
    driven by the fakes.  Returns the state_dict fields."""
    cfg = CFG
    pop = cfg.pop_per_gpu
    theta = theta.clone()
    adam_m, adam_v = torch.zeros_like(theta), torch.zeros_like(theta)
    t_step = 0
    s = types.SimpleNamespace(
        obs_sum=torch.zeros(4), obs_sumsq=torch.zeros(4),
        obs_count=torch.zeros(1), obs_mu=torch.zeros(4),
        obs_nu=torch.ones(4))
    sigma = None
    if snes is not None:
        sigma = torch.full((N,), float(cfg.sigma))
    for _ in range(STEPS):
        iteration = t_step
        fitness, obs_stat = fake_rollout(theta, iteration, pop, s.obs_mu,
                                         s.obs_nu, salt)
        ranks = ops.centered_rank_ref(fitness)
        wpair = (ranks[0::2] - ranks[1::2]).contiguous()
        if snes is None:
            grad = fake_grad(wpair, iteration, theta.numel())
        else:
            wsum = (ranks[0::2] + ranks[1::2]).contiguous()
            grad, g_sig = fake_grad_sigma(wpair, wsum, iteration)
        grad /= float(pop) * cfg.sigma
        t_step += 1
        C.longhand_adam(theta, adam_m, adam_v, grad, t_step, cfg)
        if snes is not None:
            sigma.mul_(torch.exp(g_sig * (0.5 * snes.lr_sigma / pop))
                       ).clamp_(snes.sigma_min, snes.sigma_max)
        C.longhand_merge_1d(s, obs_stat)
    want = {"theta": theta, "adam_m": adam_m, "adam_v": adam_v,
            "t_step": t_step, "obs_sum": s.obs_sum,
            "obs_sumsq": s.obs_sumsq, "obs_count": s.obs_count,
            "config": dataclasses.asdict(cfg)}
    if snes is not None:
        want["sigma"] = sigma
    return want, s


def _engine_cases():
    seed = CFG.seed
    snes = SNESConfig().resolved(CFG)
    return [
        ("es", 1, lambda: ESEngine(CFG, ctx=None, device=CPU),
         init_theta(seed, CPU), None, {}),
        ("snes", 2, lambda: SNESEngine(CFG, device=CPU),
         init_theta(seed, CPU), snes,
         {"snes_config": dataclasses.asdict(snes)}),
        ("gru", 3, lambda: RecurrentESEngine(CFG, device=CPU,
                                             obs_mask=0b0101),
         init_theta_gru(seed, CPU), None, {"obs_mask": 0b0101}),
        ("lstm", 4, lambda: LSTMESEngine(CFG, device=CPU, obs_mask=0b0101),
         init_theta_lstm(seed, CPU), None, {"obs_mask": 0b0101}),
        ("wide", 5, lambda: WideESEngine(CFG, 128, device=CPU),
         init_theta_wide(seed, 128, CPU), None, {"hidden": 128}),
    ]


@pytest.mark.parametrize("case", _engine_cases(), ids=lambda c: c[0])
def test_engine_trajectory(fake_ops, case):
    _name, salt, make, theta0, snes, extra = case
    eng = make()
    assert torch.equal(eng.theta, theta0)
    stats = [eng.step() for _ in range(STEPS)]
    assert fake_ops == {salt}
    want, s = longhand_run(theta0, salt, snes)
    want.update(extra)
    got = eng.state_dict()
    assert list(got) == list(C.CHECKPOINT_KEYS[type(eng).__name__])
    assert set(got) == set(want)
    for key, value in want.items():
        if torch.is_tensor(value):
            assert got[key].dtype == value.dtype, key
            assert torch.equal(got[key], value), key
        else:
            assert got[key] == value and type(got[key]) is type(value), key
    assert torch.equal(eng.obs_mu, s.obs_mu)
    assert torch.equal(eng.obs_nu, s.obs_nu)
    assert (eng.obs_nu[:2] == 1e-2).all() and (eng.obs_nu[2:] > 0.1).all()
    base = ["fitness_mean", "fitness_max", "grad_norm", "rollouts",
            "env_steps"]
    if snes is not None:
        base += ["sigma_mean", "sigma_min", "sigma_max"]
    for st in stats:
        assert list(st) == base
        assert [type(st[k]) for k in base[:5]] == [float] * 3 + [int] * 2
        assert st["rollouts"] == 8 * 64 and st["env_steps"] == 8 * 64 * 4
    # evaluate(): the rollout at sigma = 0, two members, nothing changes
    if salt >= 3:
        val = eng.evaluate()
        ref, _ = fake_rollout(eng.theta, eng.t_step, 2, eng.obs_mu,
                              eng.obs_nu, salt)
        assert val.dim() == 0 and torch.equal(val, ref[0])
        assert torch.equal(eng.state_dict()["theta"], want["theta"])


# ---- checkpoint compatibility ----------------------------------------------
def _parent_checkpoint(name, nparams):
    """A state_dict with exactly the earlier commit's keys for engine class
    ``name``, every tensor filled so that a load is visible."""
    obs_stat = _obs_stat((), 90)
    state = {
        "theta": _randn(nparams, seed=91),
        "adam_m": _randn(nparams, seed=92),
        "adam_v": _randn(nparams, seed=93) ** 2,
        "t_step": 7,
        "obs_sum": obs_stat[:4].clone(),
        "obs_sumsq": obs_stat[4:8].clone(),
        "obs_count": obs_stat[8:].clone(),
        "obs_mask": 0b0011,
        "hidden": 128,
        "config": dataclasses.asdict(CFG),
        "sigma": torch.full((N,), 0.07),
        "snes_config": dataclasses.asdict(SNESConfig().resolved(CFG)),
    }
    return {k: state[k] for k in C.CHECKPOINT_KEYS[name]}


@pytest.mark.parametrize("case", _engine_cases(), ids=lambda c: c[0])
def test_parent_checkpoint_loads(case, tmp_path):
    eng = case[2]()
    name = type(eng).__name__
    state = _parent_checkpoint(name, eng.theta.numel())
    assert tuple(state) == C.CHECKPOINT_KEYS[name]
    eng.load_state_dict(state)
    got = eng.state_dict()
    assert tuple(got) == C.CHECKPOINT_KEYS[name]
    for key in C._ES_KEYS:
        assert torch.equal(torch.as_tensor(got[key]),
                           torch.as_tensor(state[key])), key
    mu, nu = C.longhand_refresh(state["obs_sum"], state["obs_sumsq"],
                              state["obs_count"])
    assert torch.equal(eng.obs_mu, mu) and torch.equal(eng.obs_nu, nu)
    if "obs_mask" in state:
        assert eng.obs_mask == 0b0011
    if "sigma" in state:
        assert torch.equal(eng.sigma, state["sigma"])
    # and through a file, where the engine has save / load
    if hasattr(eng, "save"):
        path = str(tmp_path / "ckpt.pt")
        torch.save(state, path)
        other = case[2]()
        other.load(path)
        other.save(path)
        again = torch.load(path, weights_only=False)
        assert tuple(again) == C.CHECKPOINT_KEYS[name]
        assert torch.equal(again["theta"], state["theta"])
        assert torch.equal(other.obs_nu, nu)
