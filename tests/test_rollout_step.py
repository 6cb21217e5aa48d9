"""CPU side of the one-step-at-a-time rollout checks
(tests/rollout_step_cases.py): the conditions the GPU tests rely on, from
the oracle alone, and mutation checks that feed the comparison a stand-in
kernel with one defect at a time.  Derivations: profiles/rollout_oracle.md,
"One step at a time"."""

import numpy as np

import rollout_oracle_cases as C
import rollout_step_cases as S
from fiber_amd.es import rollout_oracle as oracle


def _restart(name, k, m, h):
    tr = S.trajectory(name, k, m)
    return S.one_step(S.cell_args(name, k, m),
                      tr.states[:, h].astype(np.float32))


# ---- conditions, from the oracle alone -------------------------------------

def test_h_list_is_what_the_issue_asks():
    assert any(h % 2 for h in S.H_LIST) and any(not h % 2 for h in S.H_LIST)
    assert 199 in S.H_LIST and any(45 <= h <= 55 for h in S.H_LIST)
    assert oracle.ENVS == 64
    # the multi-step classifier compares nothing there: the reason for this
    for k, m in S.CELLS:
        assert not S.trajectory("base", k, m).decided[:, 49].any()


def test_decided_share_of_every_restart():
    """Restarting one step from the oracle's own state at h leaves at
    least CAP of the 64 envs of every cell decided, for every case."""
    for name, h in S.STEP_CASES:
        for k, m in S.CELLS:
            st = _restart(name, k, m, h)
            share = st.decided.mean()
            print("%s h=%d cell(%d,%d): decided %.3f, state bound %.2e"
                  % (name, h, k, m, share, st.main.state_err[:, 1].max()))
            assert share >= S.CAP, (name, h, k, m, share)
            # nothing accumulated: the bound is the one of a single step
            assert st.main.state_err[:, 1].max() < 1e-6


def test_member_seeds_meet_the_cap_and_rejected_ones_do_not():
    for sigma in C.SIGMAS:
        seed = S.MEMBER_SEEDS[sigma]
        shares = S.member_shares(sigma, seed)
        print("sigma %g seed %d: least decided share per h %s"
              % (sigma, seed, dict(zip(S.MEMBER_H, shares))))
        assert min(shares) >= S.CAP, (sigma, seed, shares)
        # the seed is the first from 100 on: every earlier one is listed
        rejected = S.MEMBER_SEEDS_REJECTED[sigma]
        assert tuple(s for s, _share in rejected) == tuple(range(100, seed))
        for bad, share in rejected:
            got = min(S.member_shares(sigma, bad))
            assert got < S.CAP and abs(got - share) < 1e-9, (sigma, bad, got)
    # the launch splits an antithetic pair at both ends
    assert S.MEMBER_OFFSET % 2 == 1 and C.POP == 4
    assert set(S.MEMBER_H) >= {50, 199}


def test_clamp_set_is_the_floor_and_fires_in_both_signs():
    th_b, mu_b, nu_b, A_b, B_b = S.inputs_numpy("base")
    th, mu, nu, A, B = S.inputs_numpy("clamp")
    for a, b in ((th, th_b), (A, A_b), (B, B_b), (mu[:, [0, 2, 3]],
                                                  mu_b[:, [0, 2, 3]]),
                 (nu[:, 2:], nu_b[:, 2:])):
        assert np.array_equal(a, b)
    assert (nu[:, :2].view(np.uint32) == np.float32(1e-2).view(
        np.uint32)).all()
    assert (mu[:, 1] == np.float32(0.45)).all()
    # the multi-step comparison at h = 1, 2, 3: the caps already in force
    for k, m in S.CELLS:
        ro = S.clamp_cell(k, m)
        for h in S.CLAMP_HORIZONS:
            assert h <= C.CAP_SHORT_H
            share = ro.decided[:, h - 1].mean()
            assert share >= C.CAP_SHORT, (k, m, h, share)
        rstd = 1.0 / np.sqrt(nu[k].astype(np.float64) + oracle.C1EM4)
        x = (ro.states[:, :max(S.CLAMP_HORIZONS)]
             - mu[k].astype(np.float64)) * rstd
        hi, lo, mixed, hi_share, lo_share = S.clamp_condition(x)
        print("clamp cell(%d,%d) h<=3: above +5 per dim %s, below -5 %s"
              % (k, m, np.round(hi_share, 3), np.round(lo_share, 3)))
        assert hi and lo and mixed, (k, m)
        # clamped and unclamped lanes meet in one MFMA operand
        assert hi_share[2:].max() == 0.0 and lo_share[2:].max() == 0.0
        # the one-step case
        st = _restart("clamp", k, m, S.CLAMP_STEP_H)
        hi, lo, mixed, hi_share, lo_share = S.clamp_condition(st.x_raw)
        print("clamp cell(%d,%d) h=%d: above +5 per dim %s, below -5 %s"
              % (k, m, S.CLAMP_STEP_H, np.round(hi_share, 3),
                 np.round(lo_share, 3)))
        assert hi and lo and mixed, (k, m)
    # the base set never reaches the clamp: the gap this set closes
    for k, m in S.CELLS:
        for h in S.H_LIST:
            assert np.abs(_restart("base", k, m, h).x_raw).max() < 5.0


def test_one_step_reward_tolerance_is_far_below_a_reward():
    """7 U P(h + 1) at h = 199 with the largest state of any cell."""
    s_max = max(np.abs(S.trajectory(n, k, m).states).max()
                for n in S.SETS for k, m in S.CELLS)
    worst = 7.0 * S.U * S.partial_bound(200, s_max)
    print("s_max %.3f, reward tolerance at h = 199: %.3e" % (s_max, worst))
    assert worst < 1e-3


# ---- mutations: a stand-in kernel with one defect at a time -----------------

def _standin_cells(name, h, defect):
    out = []
    for k, m in S.CELLS:
        dec, s_ok, r_ok = S.standin_check(
            S.cell_args(name, k, m), S.trajectory(name, k, m), h, defect)
        out.append(((k, m), dec, s_ok, r_ok))
    return out


def test_sound_standin_passes_every_case():
    """Without a defect the stand-in is within every bound, so a failure
    below is the defect's and not the stand-in's."""
    for name, h in S.STEP_CASES:
        for cell, _dec, s_ok, r_ok in _standin_cells(name, h, None):
            assert s_ok.all() and r_ok.all(), (name, h, cell)


def test_missing_or_wrong_clamp_fails_the_clamp_case():
    """The clamp reaches the env only through the action, so it shows only
    at decided steps whose action turns.  The cells of environment 0
    hardly ever turn one past h = 11 (profiles/rollout_oracle.md); the
    check of the input set fails through the two cells of environment 1,
    so each policy is caught."""
    for defect in ("no_clamp", "clamp_4"):
        caught = {}
        for cell, dec, s_ok, _r in _standin_cells("clamp", S.CLAMP_STEP_H,
                                                  defect):
            caught[cell] = int((~s_ok).sum())
            assert dec[~s_ok].all()  # only a decided env can fail
        print("%s at h = %d: envs out of bound per cell %s"
              % (defect, S.CLAMP_STEP_H, caught))
        for k in range(C.K):
            assert sum(n for (kk, _m), n in caught.items() if kk == k) >= 1
        assert sum(caught.values()) >= 10, (defect, caught)


def test_wrong_state_buffer_fails_every_case():
    """The drive read from the other half of the double buffer, s_(h-1):
    every env of every cell leaves its bound, at both parities of h."""
    for name, h in S.STEP_CASES:
        for cell, _dec, s_ok, _r in _standin_cells(name, h, "wrong_buffer"):
            assert not s_ok.any(), (name, h, cell, int(s_ok.sum()))


def test_dropped_last_reward_fails_every_case():
    for name, h in S.STEP_CASES:
        for cell, _dec, s_ok, r_ok in _standin_cells(name, h,
                                                     "reward_dropped"):
            assert s_ok.all()
            # a reward can be near 0 (1 = 0.1 |s|^2) in a few envs
            assert (~r_ok).mean() >= 0.9, (name, h, cell, int(r_ok.sum()))


def test_undecided_step_accepts_the_other_outcome_only():
    """The candidate set: at an undecided step the flipped outcome passes,
    at a decided one it does not, and a state between the two never."""
    seen = 0
    for name, h in S.STEP_CASES:
        for k, m in S.CELLS:
            st = _restart(name, k, m, h)
            flipped = st.alt.states[:, 1].astype(np.float32)
            sm = S.match_states(st, flipped)
            assert np.array_equal(sm.ok, ~st.decided), (name, h, k, m)
            assert np.array_equal(sm.took_alt, ~st.decided)
            mid = (0.5 * (st.alt.states[:, 1] + st.main.states[:, 1])
                   ).astype(np.float32)
            assert not S.match_states(st, mid).ok.any()
            seen += int((~st.decided).sum())
    assert seen >= 1


def test_stat_step_identity_and_what_its_tolerance_resolves():
    """obs_stat_{h+1} - obs_stat_h is the sum over members and envs of s_h
    (and of s_h^2): checked on the oracle trajectories of the sigma = 0.05
    launch.  The tolerance carries the rounding of two accumulations of
    51,000 terms each, so it is a few units against terms sums in the
    hundreds: a state dropped, doubled or put in another slot stands out
    (tolerance under 5% of the sum of |terms| in every slot), while s_h
    against its neighbours s_(h-1), s_(h+1), which have settled by h = 199,
    is resolved in some slots only; the ratios are printed.  The step
    itself is held by the state check, at 1e-6."""
    sigma = 0.05
    seed = S.MEMBER_SEEDS[sigma]
    trs = [S.member_trajectory(sigma, seed, S.MEMBER_OFFSET + i)
           for i in range(C.POP)]
    for h in S.STAT_H[:1]:
        stats = {}
        for hor in (h, h + 1):
            st = oracle.obs_stats(trs, hor)
            stats[hor] = np.concatenate([st.sum, st.sumsq])
        finals = np.stack([tr.states[:, h] for tr in trs])
        want, absw = S.stat_step_want(finals)
        tol = S.stat_step_tol(stats[h], stats[h + 1], absw, h,
                              C.POP * oracle.ENVS)
        # stat_step_want rounds the states to fp32, as the kernel holds them
        assert np.allclose(stats[h + 1] - stats[h], want, rtol=0,
                           atol=1e-3)
        for other in (h - 1, h + 1):
            w2, _a = S.stat_step_want(np.stack([tr.states[:, other]
                                                for tr in trs]))
            print("h=%d vs s_%d: |difference| / tol per slot %s"
                  % (h, other, np.round(np.abs(w2 - want) / tol, 2)))
        assert (tol < 0.05 * absw).all(), (tol, absw)
