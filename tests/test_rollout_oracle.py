"""CPU checks of the per-episode fp64 rollout oracle
(fiber_amd/es/rollout_oracle.py): its constants, its agreement with the
fp32 references on the episodes it calls decided, the coverage conditions
of the GPU test, and mutation checks of the classifier.  Derivations:
profiles/rollout_oracle.md."""

import os

import numpy as np
import torch

import rollout_oracle_cases as C
from fiber_amd.es import engine as es_engine
from fiber_amd.es import philox_ref
from fiber_amd.es import rollout_oracle as oracle
# the float64 Box-Muller, shared with the update oracle's tests
from fiber_amd.es.update_oracle import normals_fp64 as _normals_fp64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CELLS = [(k, m) for k in range(C.K) for m in range(C.M)]

# A mutation must stand out from the comparison tolerance by this factor.
MUTATION_FACTOR = 100.0


# ---- constants ---------------------------------------------------------

def test_tanh_emulation_error_is_the_documented_one():
    got = oracle.measure_tanh_emulation_error()
    print("fast_tanh fp32 emulation, max |err| =", got)
    assert got <= oracle.TANH_EMUL_ERR
    # the constant is the measured value rounded up, not a loose guess
    assert got >= 0.75 * oracle.TANH_EMUL_ERR
    assert oracle.EPS_TANH == 4.0 * (oracle.TANH_EMUL_ERR
                                     + 2.5 * oracle.ULP)
    src = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "fiber_amd",
                            "csrc", "ops", "es_kernels.hip")).read()
    assert "#define TWO_LOG2E 0x1.715476p+1f" in src
    assert "1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f)" in src


def test_numpy_draws_are_within_their_share_of_z_rel():
    """Z_REL allows Z_SIDE_ULPS ulp for numpy's float32 log/sin/cos and as
    much for the device's.  numpy's share is measured here against a
    float64 Box-Muller on the draws the tests use."""
    worst = 0.0
    for seed in (C.SEED, 125, 109):
        e = np.arange(64, dtype=np.uint32)
        want = _normals_fp64(seed, C.ITER, e, np.uint32(0),
                             philox_ref.TAG_ENV)
        got = philox_ref.normal4(seed, C.ITER, e, np.uint32(0),
                                 philox_ref.TAG_ENV, np.uint32(0))
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
        jb = np.arange((oracle.NPARAMS + 3) // 4, dtype=np.uint32)
        want = _normals_fp64(seed, C.ITER, np.uint32(3) * np.ones_like(jb),
                             jb, philox_ref.TAG_NOISE).reshape(-1)
        got = philox_ref.noise_for_pair(seed, C.ITER, 3, 4 * jb.size)
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
    print("numpy normal4 vs fp64, max relative error / ULP =",
          worst / oracle.ULP)
    assert worst <= oracle.Z_SIDE_ULPS * oracle.ULP
    assert oracle.Z_REL == 2.0 * oracle.Z_SIDE_ULPS * oracle.ULP


def test_bf16_round_matches_torch_and_finds_midpoints():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.standard_normal(20000) * 3.0,
                        rng.standard_normal(20000) * 1e-3,
                        [0.0, 1.0, -1.0, 5.0, -5.0, 0.5, 1.0 - 2.0 ** -9]])
    v = v.astype(np.float32)
    want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float64).numpy()
    r, dist, q = oracle.bf16_round(v.astype(np.float64))
    assert np.array_equal(r, want)
    # a value d above a midpoint: distance d, rounds up; below: down
    lo = np.array([0.25, 1.0, 3.0, 0.75]) + 0.0
    _r, _d, ql = oracle.bf16_round(lo)
    mid = lo + 0.5 * ql
    for d in (1e-9, -1e-9):
        rr, dd, qq = oracle.bf16_round(mid + d)
        assert np.allclose(dd, abs(d), rtol=1e-6)
        assert np.array_equal(rr, lo + ql if d > 0 else lo)
        other = oracle.bf16_other_neighbour(mid + d, rr, qq)
        assert np.array_equal(other, lo if d > 0 else lo + ql)
    # exact ties go to even, like the device conversion
    rr, dd, _q = oracle.bf16_round(mid)
    assert np.array_equal(
        rr, torch.from_numpy(mid).to(torch.bfloat16).double().numpy())
    assert (dd == 0).all()


# ---- agreement with the fp32 references ----------------------------------

def test_decided_episodes_match_eval_matrix_reference():
    """engine.eval_matrix_reference is an fp32 implementation of the same
    step with an accurate tanh, so the oracle's bound for any such
    implementation, return_tol, is its own rounding: on episodes decided
    through h the two must agree within it, episode by episode."""
    inp = C.inputs_torch("cpu")
    for h in C.HORIZONS:
        ref = es_engine.eval_matrix_reference(*inp, C.SEED, C.ITER,
                                              h).double().numpy()
        for k, m in CELLS:
            ro = C.cell(k, m)
            dec = ro.decided[:, h - 1]
            err = np.abs(ref[k, m] - ro.returns[:, h - 1])
            tol = ro.return_tol[:, h - 1]
            assert (err[dec] <= tol[dec]).all(), (h, k, m, err[dec].max())
            assert tol.max() < 2e-5 * h, "the tolerance is of order 1e-5"


def test_rollout_reference_members_and_committed_fixture():
    """Perturbed members against engine.rollout_reference's episodes, and
    through them the committed fixture: its mean is reproduced bit for bit
    by the reference episodes, which agree with the oracle on every
    decided episode, so the fixture's mean equals (oracle on the decided
    episodes + reference on the others) / 64 within the mean of the
    bounds."""
    theta = es_engine.init_theta(42, "cpu")
    env_A, env_B = es_engine.make_env_params(42, "cpu")
    mu, nu = torch.zeros(4), torch.ones(4)
    seed, it, h, sigma = 1234, 0, 8, 0.05
    want = np.load(os.path.join(GOLDEN, "rollout_reference_h8_m0to3.npy"))
    s0 = torch.from_numpy(philox_ref.env_init_state(seed, it, 64))
    compared = 0
    for member in range(4):
        eps = torch.from_numpy(philox_ref.noise_for_pair(
            seed, it, member // 2, oracle.NPARAMS))
        th = theta + (-sigma if member % 2 else sigma) * eps
        ref = es_engine._reference_episodes(th, s0, h, mu, nu, env_A, env_B)
        assert np.float32(ref.mean()) == want[member]
        ro = oracle.member_rollout(theta.numpy(), sigma, seed, it, h, member,
                                   mu.numpy(), nu.numpy(), env_A.numpy(),
                                   env_B.numpy())
        ref = ref.double().numpy()
        dec = ro.decided[:, h - 1]
        err = np.abs(ref - ro.returns[:, h - 1])
        assert (err[dec] <= ro.return_tol[dec, h - 1]).all(), (
            member, err[dec].max())
        mixed = np.where(dec, ro.returns[:, h - 1], ref).mean()
        bound = (ro.return_tol[dec, h - 1].sum() / 64.0
                 + 7.0 * oracle.U * np.abs(ref).mean())  # fp32 mean of 64
        assert abs(float(want[member]) - mixed) <= bound
        compared += int(dec.sum())
    assert compared >= 0.6 * 4 * 64


def test_recorded_eval_matrix_golden_matches_on_decided_episodes():
    """tests/golden/eval_matrix_bits_k2m2_h17.npy holds episode returns
    recorded from es_eval_matrix on an MI355X.  Every later build is held
    to those bits (tests/gpu/test_rollout_bits.py); this holds the
    recording itself to the oracle, on the episodes decided through all
    17 steps, and needs no GPU."""
    gold = np.load(os.path.join(GOLDEN, "eval_matrix_bits_k2m2_h17.npy"))
    h = C.bits.EVAL_H
    compared = 0
    for k, m in CELLS:
        ro = C.cell(k, m, None, 0, h)
        dec = ro.decided[:, h - 1]
        err = np.abs(gold[k, m, 1:].astype(np.float64)
                     - ro.returns[:, h - 1])
        print("golden cell", k, m, "compared", int(dec.sum()), "max err",
              err[dec].max(), "max err/tol",
              (err[dec] / ro.return_tol[dec, h - 1]).max())
        assert (err[dec] <= ro.return_tol[dec, h - 1]).all()
        assert dec.sum() >= 16
        compared += int(dec.sum())
        fit, tol = oracle.fitness_of(ro, h)
        if dec.all():
            assert abs(float(gold[k, m, 0]) - fit) <= tol
    assert compared >= 100


# ---- conditions the GPU test relies on, from the oracle alone --------------

def test_coverage_conditions():
    seen = {h: np.zeros(64, bool) for h in C.HORIZONS}
    for k, m in CELLS:
        ro = C.cell(k, m)
        for h in C.HORIZONS:
            share = ro.decided[:, h - 1].mean()
            if h <= C.CAP_SHORT_H:
                assert share >= C.CAP_SHORT, (k, m, h, share)
            if h <= C.CAP_LONG_H:
                assert share >= C.CAP_LONG, (k, m, h, share)
            seen[h] |= ro.decided[:, h - 1]
        # decided is cumulative
        assert (ro.decided[:, 1:] <= ro.decided[:, :-1]).all()
    for h in C.HORIZONS:
        assert seen[h].all(), (h, np.flatnonzero(~seen[h]))


def test_member_launches_are_fully_decided():
    for sigma in C.SIGMAS:
        offsets = set()
        for seed, off, h in C.LAUNCHES[sigma]:
            for ro in C.launch(sigma, seed, off):
                assert ro.decided[:, h - 1].all(), (sigma, seed, off)
            offsets.add(off)
            assert C.POP >= 4 and C.POP % 2 == 0  # both parities
        assert 0 in offsets and any(o > 0 for o in offsets)
        assert any(o % 2 for o in offsets)  # a launch that splits a pair
        for h in (2, 3):
            assert len(C.launches_decided_through(sigma, h)) >= 2
    for seed in C.PAIRS_SEEDS:
        assert (seed, 0) in C.launches_decided_through(C.PAIRS_SIGMA,
                                                       C.PAIRS_H)


def test_member_fitness_applies_offset_pair_and_sign():
    theta, mu, nu, A, B = C.member_args()
    seed, off, _h = C.LAUNCHES[0.05][1]
    ros = C.launch(0.05, seed, off)
    fit, tol, dec, ro = oracle.member_fitness(theta, 0.05, seed, C.ITER, 3,
                                              off, 1, mu, nu, A, B)
    assert dec and fit == oracle.fitness_of(ros[1], 3)[0] and tol > 0
    # members 2p and 2p+1 share the noise with opposite signs
    z = philox_ref.noise_for_pair(seed, C.ITER, (off + 1) // 2,
                                  oracle.NPARAMS).astype(np.float64)
    b1 = slice(oracle.OFF_B1, oracle.OFF_W2)
    sg = float(np.float32(0.05))
    assert np.array_equal(ros[0].policy.b1, theta[b1] + sg * z[b1])
    assert np.array_equal(ros[1].policy.b1, theta[b1] - sg * z[b1])
    assert not np.array_equal(ros[1].policy.w2, ros[2].policy.w2)


# ---- mutations ---------------------------------------------------------

def test_single_wrong_action_stands_out():
    """Flip the action of one decided step (all envs at once: they are
    independent).  The next state always moves by far more than its bound.
    The return moves by more than MUTATION_FACTOR tolerances at some
    compared horizon for nearly every flip; it cannot for all, because the
    reward change of a flip, -0.4 * sum_d c_d * 0.05 B_d, can cancel.  So:
    at the steps with a compared horizon right behind them (t < 4) at
    least 95% of the flips of a cell stand out, and for every env and
    every step the flip stands out in at least one cell."""
    stood_out = np.zeros((C.H_MAX, 64), bool)
    for k, m in CELLS:
        base = C.cell(k, m)
        for t in range(C.H_MAX):
            mut = C.cell(k, m, t)
            dec = base.decided[:, t]
            assert (mut.action[:, t] != base.action[:, t]).all()
            assert np.array_equal(mut.states[:, :t + 1],
                                  base.states[:, :t + 1])
            move = (np.abs(mut.states[:, t + 1] - base.states[:, t + 1])
                    / base.state_err[:, t + 1])
            assert (move[dec] > MUTATION_FACTOR).all()
            best = np.zeros(64)
            for h in C.HORIZONS:
                if h > t:
                    ratio = (np.abs(mut.returns[:, h - 1]
                                    - base.returns[:, h - 1])
                             / base.return_tol[:, h - 1])
                    best = np.maximum(
                        best, np.where(base.decided[:, h - 1], ratio, 0.0))
            hit = dec & (best > MUTATION_FACTOR)
            if t < 4:
                assert hit.sum() >= 0.95 * dec.sum(), (k, m, t)
            stood_out[t] |= hit
    assert stood_out.all()


def test_flagged_h1_cannot_turn_a_decided_action():
    """At every decided step, move the h1 values that sit near a bf16
    midpoint to their other neighbour, one bf16 ulp away, each alone and
    all together: the action must stay."""
    tried = 0
    runs = [C.cell(k, m) for k, m in CELLS]
    runs += [ro for sigma in C.SIGMAS
             for seed, off, _h in C.LAUNCHES[sigma][:2]
             for ro in C.launch(sigma, seed, off)]
    for ro in runs:
        for e, t in zip(*np.nonzero(ro.decided & ro.h1_flag.any(-1))):
            idx = np.flatnonzero(ro.h1_flag[e, t])
            variants = [idx] + ([[j] for j in idx] if idx.size > 1 else [])
            for js in variants:
                h1 = ro.h1[e, t].copy()
                h1[js] = ro.h1_alt[e, t][js]
                assert (np.abs(h1[js] - ro.h1[e, t][js]) > 0).all()
                l0, l1 = oracle.logits_from_h1(ro.policy, h1)
                assert (l1 > l0) == ro.action[e, t], (e, t, js)
                tried += 1
    assert tried > 100


def test_swapped_stat_slot_stands_out():
    """Any two of the eight obs_stat slots differ by more than
    MUTATION_FACTOR tolerances, so sum/sumsq or two dims exchanged cannot
    pass the GPU comparison."""
    for sigma in C.SIGMAS:
        for h in (1, 2, 3):
            for seed, off in C.launches_decided_through(sigma, h - 1):
                st = oracle.obs_stats(C.launch(sigma, seed, off), h)
                v = np.concatenate([st.sum, st.sumsq])
                tol = oracle.obs_stats_tol(st)
                gap = np.abs(v[:, None] - v[None, :])
                need = MUTATION_FACTOR * np.maximum(tol[:, None],
                                                    tol[None, :])
                off_diag = ~np.eye(8, dtype=bool)
                assert (gap[off_diag] > need[off_diag]).all(), (
                    sigma, h, seed, off, v, tol)


def test_obs_stats_counts_states_before_the_horizon():
    ros = C.launch(0.05, *C.LAUNCHES[0.05][0][:2])
    st1 = oracle.obs_stats(ros, 1)
    s0 = ros[0].states[:, 0]
    assert st1.n_terms == C.POP * 64
    assert np.allclose(st1.sum, C.POP * s0.sum(0), rtol=1e-12)
    assert np.allclose(st1.sumsq, C.POP * (s0 * s0).sum(0), rtol=1e-12)
    st3 = oracle.obs_stats(ros, 3)
    want = sum(ro.states[:, :3].sum((0, 1)) for ro in ros)
    assert np.allclose(st3.sum, want, rtol=1e-12)
    assert (st3.abs_sum >= np.abs(st3.sum)).all()
