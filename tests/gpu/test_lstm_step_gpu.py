"""es_rollout_lstm one step at a time at depth, under saturation, under the
clamp and for every mask, and against lstm_policy_step bit for bit.

Every comparison is lstm_step_cases.compare_pair: launches at horizons h and
h + 1, ONE step of lstm_oracle from the kernel's own fp32 (state, hidden,
cell) at h, compared with the kernel at h + 1 for every member, env and
hidden unit.  The tolerances are lstm_oracle's and the two derivations of
tests/gpu/test_lstm_gpu.py; the conditions the inputs meet are asserted on
the CPU in tests/test_lstm_step.py.  Every test prints its worst error /
tolerance per quantity (profiles/lstm.md records them)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import lstm_step_cases as S  # noqa: E402
from fiber_amd import ops  # noqa: E402
from fiber_amd.es import lstm_oracle as L  # noqa: E402
from fiber_amd.es import philox_ref  # noqa: E402
from fiber_amd.es.rollout_oracle import C1EM4  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_TENSORS = {}
OUTPUTS = ("fitness", "obs_stat", "final_state", "final_hidden",
           "final_cell")


def _launch(c, horizon, offset=S.OFFSET, pop=S.POP, mask=0b1111, mu=None,
            final=True):
    """One launch: a run, as numpy arrays (with ``final=False`` only fitness
    and obs_stat)."""
    if c.name not in _TENSORS:
        _TENSORS[c.name] = [torch.from_numpy(np.array(a)).to(DEV)
                            for a in (c.theta, c.mu, c.nu, c.A, c.B)]
    theta, obs_mu, nu, A, B = _TENSORS[c.name]
    if mu is not None:
        obs_mu = torch.from_numpy(mu).to(DEV)
    out = ops.es_rollout_lstm(theta, c.sigma, c.seed, S.ITER, horizon, offset,
                              pop, obs_mu, nu, A, B, mask, return_final=final)
    return tuple(t.cpu().numpy() for t in out)


def _check(label, c, h, run0, run1, offset=S.OFFSET, mask=0b1111):
    v = S.compare_pair(c, offset, mask, h, run0, run1)
    print("%s h=%d: %s least decided share %.3f"
          % (label, h, {k: round(r, 4) for k, r in v.worst.items()},
             min(v.shares)))
    assert v.count_ok, label
    assert min(v.shares) >= S.CAP, (label, h, v.shares)
    assert all(r <= 1.0 for r in v.worst.values()), (label, h, v.worst)
    return v


# ---- deep steps -------------------------------------------------------------------

@pytest.mark.parametrize("name,h", [(n, h) for n in S.SETS
                                    for h in S.case(n).horizons])
def test_deep_step_matches_oracle(name, h):
    c = S.case(name)
    run0, run1 = _launch(c, h), _launch(c, h + 1)
    print("%s h=%d: max |c| %.2f" % (name, h, np.abs(run0[4]).max()))
    _check(name, c, h, run0, run1)


def test_step_under_the_normaliser_an_engine_floored():
    """The normaliser of a real LSTMESEngine.step() whose variance the
    engine floors in dims 0 and 1, and that engine's theta and env."""
    import update_oracle_cases as C
    from fiber_amd.es import ESConfig, LSTMESEngine

    cfg = ESConfig(pop_per_gpu=C.FLOOR_POP, horizon=C.STEP_HORIZON)
    assert cfg.seed == C.FLOOR_SEED
    eng = LSTMESEngine(cfg, device=DEV)
    state = eng.state_dict()
    state.update({k: torch.from_numpy(v)
                  for k, v in C.floor_obs_state().items()})
    eng.load_state_dict(state)
    eng.step(C.STEP_ITERATIONS[0])
    nu = eng.obs_nu.cpu().numpy()
    assert (nu[:2].view(np.uint32)
            == np.float32(1e-2).view(np.uint32)).all(), nu
    assert (nu[2:] > 0.5).all(), nu
    c = S.Case("engine", eng.theta.cpu().numpy(), eng.obs_mu.cpu().numpy(),
               nu, eng.env_A.cpu().numpy(), eng.env_B.cpu().numpy(),
               cfg.sigma, cfg.seed, (S.H_CLAMP[-1],))
    h = c.horizons[0]
    try:
        run0, run1 = _launch(c, h), _launch(c, h + 1)
    finally:
        _TENSORS.pop("engine", None)
    _check("engine-floored", c, h, run0, run1)
    raw = (run0[2].astype(np.float64) - c.mu) / np.sqrt(
        nu.astype(np.float64) + C1EM4)
    hi, lo = (raw > 5.0).sum((0, 1)), (raw < -5.0).sum((0, 1))
    print("engine-floored: obs_nu %s, x above +5 per dim %s, below -5 %s"
          % (nu, hi, lo))
    assert hi[:2].sum() >= 1 and lo[:2].sum() >= 1


# ---- every step of one episode ------------------------------------------------------

def test_every_step_of_one_episode():
    c = S.case("base")
    runs = [_launch(c, hor) for hor in range(S.H_TOP + 1)]
    f, st, s, hid, cel = runs[0]
    init = philox_ref.env_init_state(c.seed, S.ITER, S.ENVS)
    assert (np.abs(s - init) <= (L.Z_REL + L.U) * np.abs(init)).all()
    assert not hid.any() and not cel.any()
    assert not f.any() and not st.any()
    worst, share = {}, 1.0
    for h in range(S.H_TOP):
        v = S.compare_pair(c, S.OFFSET, 0b1111, h, runs[h], runs[h + 1])
        assert S.passes(v), (h, v.worst, v.count_ok)
        for k, r in v.worst.items():
            worst[k] = S.worse(worst.get(k, 0.0), r)
        share = min(share, min(v.shares))
    print("every step 0..%d: %s least decided share %.3f"
          % (S.H_TOP - 1, {k: round(r, 4) for k, r in worst.items()}, share))
    assert share >= S.CAP


# ---- all 16 masks -------------------------------------------------------------------

@pytest.mark.parametrize("mask", S.MASKS)
def test_every_mask_matches_oracle(mask):
    c = S.case("base")
    hs = range(min(S.H_MASK), max(S.H_MASK) + 2)
    runs = {hor: _launch(c, hor, mask=mask) for hor in hs}
    for h in S.H_MASK:
        _check("mask %s" % format(mask, "04b"), c, h, runs[h], runs[h + 1],
               mask=mask)
    if mask == 0:
        # the policy cannot see the observation: another obs_mu changes no
        # bit of the hidden or the cell state, hence none of the actions,
        # states, fitness or statistics
        other = np.array([-0.4, 0.3, 0.2, -0.1], dtype=np.float32)
        assert not np.array_equal(other, c.mu)
        for hor in hs:
            again = _launch(c, hor, mask=0, mu=other)
            for a, b, what in zip(runs[hor], again, OUTPUTS):
                assert a.tobytes() == b.tobytes(), (hor, what)


# ---- the rollout kernel against the serving kernel -----------------------------------

@pytest.mark.parametrize("name,h", S.SERVING)
def test_rollout_step_is_the_serving_step_bit_for_bit(name, h):
    """Both kernels inline lstm_cell: from the rollout's own (state, hidden,
    cell) at h, lstm_policy_step returns the rollout's hidden and cell state
    at h + 1 bit for bit, and logits whose action is the one the rollout
    took.  At sigma 0, where the rollout's weights are theta's; on
    "saturated0" at h = 199 the cell state is near 199."""
    c = S.case(name)
    assert c.sigma == 0.0
    _f0, _st0, s0, hid0, cel0 = _launch(c, h, pop=2)
    _f1, _st1, s1, hid1, cel1 = _launch(c, h + 1, pop=2)
    theta = _TENSORS[c.name][0]
    for m in range(2):
        member = S.OFFSET + m
        x, slack = L.observe(s0[m], c.mu, c.nu)
        keep = ~slack.any(-1)
        assert keep.mean() > 0.90
        logits, hnew, cnew = ops.lstm_policy_step(
            theta, torch.from_numpy(x.astype(np.float32)).to(DEV),
            torch.from_numpy(hid0[m]).to(DEV),
            torch.from_numpy(cel0[m]).to(DEV))
        logits, hnew, cnew = (t.cpu().numpy() for t in (logits, hnew, cnew))
        rh, rc, rl = S.policy_step_ratios(c.theta, x, hid0[m], cel0[m],
                                          logits, hnew, cnew)
        dh = int((hnew[keep].view(np.uint32)
                  != hid1[m][keep].view(np.uint32)).sum())
        dc = int((cnew[keep].view(np.uint32)
                  != cel1[m][keep].view(np.uint32)).sum())
        print("serving %s h=%d member %d: %d of %d envs kept, %d hidden and "
              "%d cell values differ in bits, max |c| %.2f; policy step h' "
              "%.3f c' %.3f logits %.3f"
              % (name, h, member, keep.sum(), keep.size, dh, dc,
                 np.abs(cel0[m]).max(), rh, rc, rl))
        assert rh <= 1.0 and rc <= 1.0 and rl <= 1.0
        assert dh == 0 and dc == 0
        # the action the rollout took, read off its state at h + 1
        _wh, _wc, want_l, _th, _tc, tol_l = L.cell(
            L.make_policy(c.theta), x, hid0[m], cel0[m])
        decided = np.abs(want_l[:, 1] - want_l[:, 0]) > tol_l.sum(-1)
        up, tol_s = L.env_step(s0[m], np.ones(S.ENVS, bool), c.A, c.B)
        down, _ = L.env_step(s0[m], np.zeros(S.ENVS, bool), c.A, c.B)
        is_up = (np.abs(s1[m] - up) <= tol_s).all(-1)
        is_down = (np.abs(s1[m] - down) <= tol_s).all(-1)
        assert (is_up ^ is_down).all()
        served = logits[:, 1] > logits[:, 0]
        sel = keep & decided
        assert decided.mean() >= S.CAP
        assert np.array_equal(served[sel], is_up[sel])
        assert np.array_equal(served[sel], (want_l[:, 1] > want_l[:, 0])[sel])


# ---- a launch far from pair 0 -------------------------------------------------------

def test_two_members_at_a_large_offset():
    c = S.case("base")
    h = S.FAR_H
    run0 = _launch(c, h, S.FAR_OFFSET, S.FAR_POP)
    run1 = _launch(c, h + 1, S.FAR_OFFSET, S.FAR_POP)
    _check("offset %d" % S.FAR_OFFSET, c, h, run0, run1, S.FAR_OFFSET)
    # and they are not the members at the small offset
    near = _launch(c, h + 1, S.OFFSET, S.FAR_POP)
    assert not np.array_equal(near[3], run1[3])
    assert not np.array_equal(near[4], run1[4])


# ---- the optional outputs at depth ---------------------------------------------------

@pytest.mark.parametrize("horizon", [199, 200])
def test_return_final_changes_no_bits_at_depth(horizon):
    for name in ("base", "saturated"):
        c = S.case(name)
        with_final = _launch(c, horizon)
        plain = _launch(c, horizon, final=False)
        assert len(plain) == 2 and len(with_final) == 5
        for a, b, what in zip(with_final, plain, OUTPUTS):
            assert a.tobytes() == b.tobytes(), (name, horizon, what)
