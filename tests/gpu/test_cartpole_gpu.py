"""The CartPole kernels against fiber_amd.es.cartpole_oracle (fp64), and the
engine against a hand composition of the ops.  The inputs are
tests/cartpole_cases.py's; tests/test_cartpole_oracle.py states what they
cover.  Every oracle test prints its worst error / bound ratio."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cartpole_cases as K  # noqa: E402
from fiber_amd import ops  # noqa: E402
from fiber_amd.es import CartPoleESEngine, ESConfig, _core, init_theta  # noqa: E402
from fiber_amd.es import cartpole_oracle as C  # noqa: E402
from fiber_amd.es import philox_ref, rollout_oracle as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _dev(a):
    return torch.tensor(a, device=DEV)


# ---- 1. cartpole_step against the oracle -----------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("cart", list(K.CARTS))
def test_step_matches_oracle(n, cart):
    cart = K.CARTS[cart]
    rng = np.random.default_rng(n)
    s = rng.uniform(-1.0, 1.0, (n, 4)) * [cart[6], 2.0, cart[7], 2.0]
    # rows that land within 1e-3 of a threshold, on either side of it
    near = np.array([sx * (thr + d) for thr in (cart[6], cart[7])
                     for sx in (1.0, -1.0) for d in (-7e-4, 2e-4)])
    k = min(n, 8)
    s[:k, 1] = s[:k, 3] = 0.01
    s[np.arange(k), np.where(np.arange(k) < 4, 0, 2)] = near[:k]
    s = s.astype(np.float32)
    a = rng.random(n) < 0.5
    nxt, done = ops.cartpole_step(_dev(s), _dev(a.astype(np.int32)),
                                  _dev(cart))
    want, bound, want_done, decided = C.step(s, a, cart)
    ratio = (np.abs(nxt.cpu().numpy() - want) / bound).max()
    print("cartpole_step n=%d: %.3f, %d undecided" % (n, ratio,
                                                       (~decided).sum()))
    assert ratio <= 1.0
    assert decided.mean() >= 0.9
    assert (done.cpu().numpy().astype(bool) == want_done)[decided].all()


# ---- 2. one rollout step, restarted from the kernel's own state -----------

def _launch(sigma, horizon, cart, offset=K.OFFSET, pop=K.POP, it=K.ITER):
    out = ops.es_rollout_mlp_cartpole(
        _dev(K.theta()), sigma, K.SEED, it, horizon, offset, pop, _dev(K.MU),
        _dev(K.NU), _dev(K.CARTS[cart]), return_lengths=True,
        return_final=True)
    return [t.cpu().numpy() for t in out]


def _alive(lengths, state, h, cart):
    """The kernel's alive bits after h steps, from what it returns."""
    inside = ((np.abs(state[..., 0]) <= cart[6])
              & (np.abs(state[..., 2]) <= cart[7]))
    return (lengths == h) & (inside | (h == 0))


@pytest.mark.parametrize("h", list(range(16)) + [40, 199])
@pytest.mark.parametrize("sigma", K.SIGMAS)
@pytest.mark.parametrize("cart", list(K.CARTS))
def test_rollout_step_matches_oracle(h, sigma, cart):
    cv = K.CARTS[cart]
    _f0, _st0, len0, s0 = _launch(sigma, h, cart)
    _f1, _st1, len1, s1 = _launch(sigma, h + 1, cart)
    if h == 0:
        init, init_err = C.init_states(K.SEED, K.ITER)
        assert (np.abs(s0 - init) <= init_err).all() and not len0.any()
    alive0, alive1 = _alive(len0, s0, h, cv), _alive(len1, s1, h + 1, cv)
    theta, worst, undecided = K.theta(), 0.0, 0
    for m in range(K.POP):
        member = K.OFFSET + m
        z = philox_ref.noise_for_pair(K.SEED, K.ITER, member // 2, R.NPARAMS)
        pol = C.make_policy(theta, -sigma if member % 2 else sigma, z)
        act, act_ok = C.policy_step(pol, s0[m], K.MU, K.NU)
        want, bound, done, done_ok = C.step(s0[m], act, cv)
        live = alive0[m]
        sure = live & act_ok & done_ok
        undecided += int((live & ~sure).sum())
        if sure.any():
            worst = max(worst, float(
                (np.abs(s1[m] - want) / bound)[sure].max()))
        assert (alive1[m] == ~done)[sure].all()
        assert (len1[m] == len0[m] + live).all()
        # finished environments are frozen, bit for bit
        assert s1[m][~live].tobytes() == s0[m][~live].tobytes()
    print("rollout_step %s h=%d sigma=%g: %.3f, nlive %s, %d undecided"
          % (cart, h, sigma, worst, alive0.sum(1).tolist(), undecided))
    assert worst <= 1.0
    assert undecided <= 0.05 * K.POP * 64


# ---- 3. bookkeeping --------------------------------------------------------

def test_fitness_and_count_are_exact_and_early_exit_changes_nothing():
    f2, st2, len2, s2 = _launch(0.05, 200, "default")
    f4, st4, len4, s4 = _launch(0.05, 400, "default")
    for f, st, ln in ((f2, st2, len2), (f4, st4, len4)):
        assert f.tobytes() == (ln.sum(1).astype(np.float32)
                               / np.float32(64)).tobytes()
        assert st[8] == ln.sum()
    ended = (len2 < 200).all(1)   # out of the loop before step 200
    assert ended.any()
    assert f4[ended].tobytes() == f2[ended].tobytes()
    assert len4[ended].tobytes() == len2[ended].tobytes()
    assert s4[ended].tobytes() == s2[ended].tobytes()
    assert (len4[~ended] >= len2[~ended]).all()


@pytest.mark.parametrize("cart", list(K.STAT_ITERS))
def test_obs_stat_sums_the_presented_states(cart):
    it = K.STAT_ITERS[cart]
    _f, st, lengths, _s = _launch(0.05, K.STAT_H, cart, pop=2, it=it)
    ros = K.members(0.05, cart, K.STAT_H, it, 2)
    assert (lengths == np.stack([ro.lengths for ro in ros])).all()
    want = C.obs_stats(ros)
    ratio = (np.abs(st[:8] - np.concatenate([want.sum, want.sumsq]))
             / R.obs_stats_tol(want)).max()
    print("obs_stat %s: %.3f" % (cart, ratio))
    assert ratio <= 1.0 and st[8] == lengths.sum()


def test_last_members_are_the_last_pair():
    _f, _st, lengths, _s = _launch(0.05, 8, "small", offset=32766, pop=2)
    for m in range(2):
        ro = C.member_rollout(K.theta(), 0.05, K.SEED, K.ITER, 8, 32766 + m,
                              K.MU, K.NU, K.CARTS["small"])
        sure = ro.decided[:, -1]
        assert sure.mean() > 0.8
        assert (lengths[m] == ro.lengths)[sure].all()
    assert (lengths[0] != lengths[1]).any()


# ---- 4. engine ---------------------------------------------------------------

def _engine_bits(e):
    return [t.cpu().numpy().tobytes() for t in (
        e.theta, e.adam_m, e.adam_v, e.obs_sum, e.obs_sumsq, e.obs_count,
        e.obs_mu, e.obs_nu)]


def test_engine_is_the_hand_composition(tmp_path):
    cfg = ESConfig(pop_per_gpu=32, horizon=30, seed=99)
    eng = CartPoleESEngine(cfg, device=DEV)
    twin = CartPoleESEngine(cfg, device=DEV)   # stepped by hand
    assert torch.equal(eng.theta, init_theta(99, DEV))
    assert torch.equal(eng.cart, ops.cartpole_params(device=DEV))
    for it in range(3):
        fit, stat = ops.es_rollout_mlp_cartpole(
            twin.theta, cfg.sigma, cfg.seed, it, cfg.horizon, 0, 32,
            twin.obs_mu, twin.obs_nu, twin.cart)
        ranks = ops.centered_rank(fit)
        grad = ops.es_grad((ranks[0::2] - ranks[1::2]).contiguous(), 0, 16,
                           cfg.seed, it, DEV, nparams=ops.NPARAMS)
        grad /= 32.0 * cfg.sigma
        twin.t_step += 1
        _core.adam_ascent(twin.theta, twin.adam_m, twin.adam_v, grad,
                          twin.t_step, cfg)
        twin._merge_obs_stat(stat)
        stats = eng.step()
        assert _engine_bits(eng) == _engine_bits(twin)
        assert stats["env_steps"] == int(stat[8]) < 32 * 64 * cfg.horizon
        assert stats["fitness_mean"] == float(fit.mean())
    eng.save(tmp_path / "cartpole.pt")
    fresh = CartPoleESEngine(cfg, device=DEV)
    fresh.load(tmp_path / "cartpole.pt")
    assert _engine_bits(fresh) == _engine_bits(eng) and fresh.t_step == 3
    assert "cart" not in eng.state_dict()
    fit0 = ops.es_rollout_mlp_cartpole(eng.theta, 0.0, cfg.seed, 3,
                                       cfg.horizon, 0, 2, eng.obs_mu,
                                       eng.obs_nu, eng.cart)[0]
    assert eng.evaluate() == fit0[0] == fit0[1]
    obs = torch.randn(70, 4, device=DEV) * 0.1
    x = ((obs - eng.obs_mu) * torch.rsqrt(eng.obs_nu + 1e-4)).clamp(-5, 5)
    logits = ops.mlp_policy_forward(eng.theta, x.contiguous())
    assert torch.equal(eng.act(obs), (logits[:, 1] > logits[:, 0]).long())
    with pytest.raises(NotImplementedError):
        CartPoleESEngine(cfg, ctx=object(), device=DEV)
    with pytest.raises(ValueError):
        ops.cartpole_params(theta_threshold=0.6)
