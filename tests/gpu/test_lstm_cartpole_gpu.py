"""es_rollout_lstm_cartpole against fp64, one step at a time from the kernel's
own state (lstm_oracle's cell, cartpole_oracle's physics), against the
serving step and the stand-alone physics bit for bit, and
LSTMCartPoleESEngine against a hand composition of the ops.  The inputs are
tests/cartpole_cases.py's; tests/test_lstm_cartpole.py conditions them on
the CPU.  The tolerances are the oracles' own."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cartpole_cases as K  # noqa: E402
from fiber_amd import ops  # noqa: E402
from fiber_amd.es import (ESConfig, LSTMCartPoleESEngine, _core,  # noqa: E402
                          init_theta_lstm)
from fiber_amd.es import cartpole_oracle as C  # noqa: E402
from fiber_amd.es import lstm_cartpole_oracle as LC  # noqa: E402
from fiber_amd.es import lstm_oracle as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MASKS = (0b0101, 0b1111)
HS = list(range(26)) + [40]
THETA = init_theta_lstm(K.SEED, "cpu")
OUTPUTS = ("fitness", "obs_stat", "lengths", "final_state", "final_hidden",
           "final_cell")


def _dev(a):
    return torch.as_tensor(a).to(DEV)


def _launch(sigma, horizon, cart, mask, pop=K.POP, mu=K.MU, lengths=True,
            final=True):
    """(fitness, obs_stat, lengths, final_state, final_hidden, final_cell)"""
    out = ops.es_rollout_lstm_cartpole(
        _dev(THETA), sigma, K.SEED, K.ITER, horizon, K.OFFSET, pop, _dev(mu),
        _dev(K.NU), _dev(K.CARTS[cart]), mask, return_lengths=lengths,
        return_final=final)
    return [t.cpu().numpy() for t in out]


def _alive(lengths, state, h, cart):
    """The kernel's alive bits after h steps, from what it returns."""
    inside = ((np.abs(state[..., 0]) <= cart[6])
              & (np.abs(state[..., 2]) <= cart[7]))
    return (lengths == h) & (inside | (h == 0))


# ---- 1. one step against fp64, restarted from the kernel's own state -------

@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("sigma", K.SIGMAS)
@pytest.mark.parametrize("cart", list(K.CARTS))
def test_rollout_step_matches_oracles(cart, sigma, mask):
    cv = K.CARTS[cart]
    runs = {h: _launch(sigma, h, cart, mask)
            for h in sorted(set(HS) | {h + 1 for h in HS})}
    pols = [LC.member_policy(THETA.numpy(), sigma, K.SEED, K.ITER,
                             K.OFFSET + m) for m in range(K.POP)]
    _f, _st, len0, s0, hid0, cel0 = runs[0]
    init, init_err = C.init_states(K.SEED, K.ITER)
    assert (np.abs(s0 - init) <= init_err).all()
    assert not len0.any() and not hid0.any() and not cel0.any()
    worst = {"h": 0.0, "c": 0.0, "state": 0.0}
    undecided = live_steps = 0
    for h in HS:
        _f, _st, len0, s0, hid0, cel0 = runs[h]
        _f, _st, len1, s1, hid1, cel1 = runs[h + 1]
        alive0, alive1 = _alive(len0, s0, h, cv), _alive(len1, s1, h + 1, cv)
        for m in range(K.POP):
            live, on = alive0[m], alive1[m]
            st = LC.step(pols[m], s0[m], hid0[m], cel0[m], K.MU, K.NU, mask,
                         cv)
            sure = live & st.action_decided & st.done_decided
            live_steps += int(live.sum())
            undecided += int((live & ~sure).sum())
            assert not (on & ~live).any()
            # the rows of an environment that is still alive at h + 1
            for key, got, want, tol in (("h", hid1[m], st.h, st.tol_h),
                                        ("c", cel1[m], st.c, st.tol_c)):
                if on.any():
                    worst[key] = max(worst[key], float(
                        (np.abs(got - want) / tol)[on].max()))
            if sure.any():
                worst["state"] = max(worst["state"], float(
                    (np.abs(s1[m] - st.state) / st.bound)[sure].max()))
            assert (on == ~st.done)[sure].all()
            assert (len1[m] == len0[m] + live).all()
            # ended: frozen bit for bit, zero hidden and cell rows
            assert s1[m][~live].tobytes() == s0[m][~live].tobytes()
            assert not hid0[m][~live].any() and not cel0[m][~live].any()
            assert not hid1[m][~on].any() and not cel1[m][~on].any()
        print("%s sigma %g mask %s h=%d: live per member %s"
              % (cart, sigma, format(mask, "04b"), h,
                 alive0.sum(1).tolist()))
    print("%s sigma %g mask %s: worst error / tolerance %s, %d of %d live "
          "environment-steps undecided"
          % (cart, sigma, format(mask, "04b"),
             {k: round(v, 4) for k, v in worst.items()}, undecided,
             live_steps))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert undecided <= 0.05 * live_steps


# ---- 2. the serving step and the stand-alone physics, bit for bit ----------

@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("h", [3, 12, 20])
def test_rollout_step_is_serving_step_and_cartpole_step(h, mask):
    cv = K.CARTS["default"]
    _f, _st, len0, s0, hid0, cel0 = _launch(0.0, h, "default", mask, pop=2)
    _f, _st, len1, s1, hid1, cel1 = _launch(0.0, h + 1, "default", mask,
                                            pop=2)
    alive0, alive1 = _alive(len0, s0, h, cv), _alive(len1, s1, h + 1, cv)
    for m in range(2):
        x, slack = L.observe(s0[m], K.MU, K.NU, mask)
        live = alive0[m] & ~slack.any(-1)
        on = alive1[m] & live
        assert on.sum() >= 4
        logits, hnew, cnew = ops.lstm_policy_step(
            _dev(THETA), _dev(x.astype(np.float32)), _dev(hid0[m]),
            _dev(cel0[m]))
        action = (logits[:, 1] > logits[:, 0]).to(torch.int32)
        nxt, done = ops.cartpole_step(_dev(s0[m]), action, _dev(cv))
        nxt, done = nxt.cpu().numpy(), done.cpu().numpy().astype(bool)
        assert hnew.cpu().numpy()[on].tobytes() == hid1[m][on].tobytes()
        assert cnew.cpu().numpy()[on].tobytes() == cel1[m][on].tobytes()
        assert nxt[live].tobytes() == s1[m][live].tobytes()
        assert (alive1[m] == ~done)[live].all()


# ---- 3. early exit and tile skipping change nothing ------------------------

def test_early_exit_changes_nothing_and_counts_are_exact():
    run2 = _launch(0.05, 200, "small", 0b0101)
    run4 = _launch(0.05, 400, "small", 0b0101)
    for f, st, ln in (run2[:3], run4[:3]):
        assert f.tobytes() == (ln.sum(1).astype(np.float32)
                               / np.float32(64)).tobytes()
        assert st[8] == ln.sum()
    # every member has left the loop before step 200
    assert (run2[2] < 200).all()
    for a, b, what in zip(run2, run4, OUTPUTS):
        assert a.tobytes() == b.tobytes(), what
    for lengths, final in ((False, False), (True, False), (False, True)):
        part = _launch(0.05, 200, "small", 0b0101, lengths=lengths,
                       final=final)
        names = OUTPUTS[:2] + OUTPUTS[2:3] * lengths + OUTPUTS[3:] * final
        assert len(part) == len(names)
        for got, what in zip(part, names):
            assert got.tobytes() == run2[OUTPUTS.index(what)].tobytes(), what


# ---- 4. the mask -----------------------------------------------------------

def test_mask_zero_hides_the_normaliser_and_masks_differ():
    other = np.array([-0.4, 0.3, 0.2, -0.1], dtype=np.float32)
    for a, b, what in zip(_launch(0.05, 30, "default", 0),
                          _launch(0.05, 30, "default", 0, mu=other), OUTPUTS):
        assert a.tobytes() == b.tobytes(), what
    assert not np.array_equal(_launch(0.05, 30, "default", 0b0101)[2],
                              _launch(0.05, 30, "default", 0b1111)[2])


# ---- 5. engine -------------------------------------------------------------

def _engine_bits(e):
    return [t.cpu().numpy().tobytes() for t in (
        e.theta, e.adam_m, e.adam_v, e.obs_sum, e.obs_sumsq, e.obs_count,
        e.obs_mu, e.obs_nu)]


def test_engine_is_the_hand_composition(tmp_path):
    cfg = ESConfig(pop_per_gpu=32, horizon=30, seed=99)
    eng = LSTMCartPoleESEngine(cfg, device=DEV)
    twin = LSTMCartPoleESEngine(cfg, device=DEV)   # stepped by hand
    assert torch.equal(eng.theta, init_theta_lstm(99, DEV))
    assert torch.equal(eng.cart, ops.cartpole_params(device=DEV))
    assert eng.obs_mask == 0b0101
    for it in range(3):
        fit, stat = ops.es_rollout_lstm_cartpole(
            twin.theta, cfg.sigma, cfg.seed, it, cfg.horizon, 0, 32,
            twin.obs_mu, twin.obs_nu, twin.cart, 0b0101)
        ranks = ops.centered_rank(fit)
        grad = ops.es_grad((ranks[0::2] - ranks[1::2]).contiguous(), 0, 16,
                           cfg.seed, it, DEV, nparams=ops.LSTM_NPARAMS)
        grad /= 32.0 * cfg.sigma
        twin.t_step += 1
        _core.adam_ascent(twin.theta, twin.adam_m, twin.adam_v, grad,
                          twin.t_step, cfg)
        twin._merge_obs_stat(stat)
        stats = eng.step()
        assert _engine_bits(eng) == _engine_bits(twin)
        assert stats["env_steps"] == int(stat[8]) < 32 * 64 * cfg.horizon
        assert stats["fitness_mean"] == float(fit.mean())
    eng.save(tmp_path / "lstm_cartpole.pt")
    fresh = LSTMCartPoleESEngine(cfg, device=DEV, obs_mask=0b1111)
    fresh.load(tmp_path / "lstm_cartpole.pt")
    assert _engine_bits(fresh) == _engine_bits(eng) and fresh.t_step == 3
    assert fresh.obs_mask == 0b0101 and "cart" not in eng.state_dict()
    fit0 = ops.es_rollout_lstm_cartpole(
        eng.theta, 0.0, cfg.seed, 3, cfg.horizon, 0, 2, eng.obs_mu,
        eng.obs_nu, eng.cart, 0b0101)[0]
    assert eng.evaluate() == fit0[0] == fit0[1]
    obs = torch.randn(70, 4, device=DEV) * 0.1
    x = ((obs - eng.obs_mu) * torch.rsqrt(eng.obs_nu + 1e-4)).clamp(-5, 5)
    x = (x * torch.tensor([1.0, 0.0, 1.0, 0.0], device=DEV)).contiguous()
    zeros = torch.zeros(70, 64, device=DEV)
    logits, hnew, cnew = ops.lstm_policy_step(eng.theta, x, zeros, zeros)
    actions, (h1, c1) = eng.act(obs)
    assert torch.equal(actions, (logits[:, 1] > logits[:, 0]).long())
    assert torch.equal(h1, hnew) and torch.equal(c1, cnew)
    again, _ = eng.act(obs, (h1, c1))
    l2 = ops.lstm_policy_step(eng.theta, x, hnew, cnew)[0]
    assert torch.equal(again, (l2[:, 1] > l2[:, 0]).long())
    with pytest.raises(NotImplementedError):
        LSTMCartPoleESEngine(cfg, ctx=object(), device=DEV)
    with pytest.raises(ValueError):
        LSTMCartPoleESEngine(cfg, device=DEV, obs_mask=16)


def test_wrapper_refuses_bad_arguments():
    args = dict(theta=_dev(THETA), sigma=0.05, seed=1, iteration=0, horizon=4,
                member_offset=0, pop_shard=2, obs_mu=_dev(K.MU),
                obs_nu=_dev(K.NU), cart=_dev(K.CARTS["default"]))
    wide = np.array(K.CARTS["default"])
    wide[7] = 0.6     # past the sin / cos polynomials' range
    for bad, err in ((dict(theta=_dev(THETA)[:-1]), ValueError),
                     (dict(theta=_dev(torch.zeros(THETA.numel() + 1))[1:]),
                      ValueError),                       # not 16-byte aligned
                     (dict(theta=THETA), TypeError),     # not on the GPU
                     (dict(obs_mu=_dev(K.MU)[:3]), ValueError),
                     (dict(cart=_dev(wide)), ValueError),
                     (dict(cart=_dev(K.CARTS["default"])[::2]), TypeError),
                     (dict(pop_shard=3), ValueError),
                     (dict(member_offset=1), ValueError),
                     (dict(horizon=ops.CART_HORIZON_MAX), ValueError),
                     (dict(obs_mask=16), ValueError),
                     (dict(obs_mask=-1), ValueError)):
        with pytest.raises(err):
            ops.es_rollout_lstm_cartpole(**{**args, **bad})
