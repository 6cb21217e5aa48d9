"""CPU side of the one-step-at-a-time LSTM rollout checks
(tests/lstm_step_cases.py): the conditions the GPU tests rely on, from
lstm_oracle alone; the tolerances stay sharp on every input set; and
stand-in kernels with one defect each fail the very comparison the GPU tests
use.  Figures: profiles/lstm.md, "One step at a time, at depth"."""

import numpy as np
import pytest

import lstm_step_cases as S
from fiber_amd.es import lstm_oracle as L

# max |c| over units and envs on "base": what h <= 8 stays under (6.17 at
# most) and h = 199 exceeds (23.6 at least); the bound is their geometric
# mean, rounded
C_DEPTH = 12.0
# bf16 has 8 bits: from |c| = 128 on its spacing is 1
C_BF16_COARSE = 128.0
# Share of i / f / o gate values in (0.05, 0.95).  "saturated" has 0.29 at
# h = 8 and 0.16 .. 0.21 deeper, "wide" 0.128 .. 0.167: what is met at every
# checked h is asserted.
MID_SATURATED, MID_DEEP = 0.25, 0.12
# Hoped for and not met: that sigma 4.0 drives every member of "wide" past
# both ends of fast_sigmoid's exp2, as it does in the GRU.  Measured: only
# member 4 goes below PRE_OVERFLOW (-102.9 at h = 49, -93.96 at h = 50); the
# least pre-activation of members 2, 3 and 5 is -66.98, -80.52 and -84.46.
# No member reaches PRE_UNDERFLOW: the largest pre-activation is 95.78
# (member 3, h = 199).  theta x 8 stays inside |pre| < 69.  So the overflow
# end is exercised by one member at two checked h, the underflow end of exp2
# by none; |pre| > 50 (sigmoid within 2e-22 of 0 or 1) is reached by every
# member of both sets.
WIDE_OVERFLOW = {4: (49, 50)}
PRE_FAR = 50.0
# |c| and |c'| beyond this with one sign: tanh of both is +-1 to the last
# bit of a double (1 - tanh 20 = 8e-18), so h' = o tanh(c) and o tanh(c')
# are the same number
TANH_FLAT = 20.0


# ---- rollout is the chain of the single steps ---------------------------------

def test_rollout_chains_observe_cell_env_step():
    c = S.case("base")
    ro = S.trajectory("base", S.OFFSET)
    assert ro.s.shape == (S.H_TOP + 1, 64, 4)
    assert ro.h.shape == ro.c.shape == (S.H_TOP + 1, 64, 64)
    assert ro.pre.shape == (S.H_TOP, 4, 64, 64)
    assert not ro.h[0].any() and not ro.c[0].any()
    assert ro.s.dtype == ro.h.dtype == ro.c.dtype == np.float32
    for t in (0, 1, 50, 199):
        x, slack = L.observe(ro.s[t], c.mu, c.nu)
        assert np.array_equal(x, ro.x[t])
        hn, cn, logits, _th, _tc, tol_l, pre = L.cell(
            S.policy_for(c, S.OFFSET), x, ro.h[t], ro.c[t], slack,
            with_pre=True)
        assert np.array_equal(hn.astype(np.float32), ro.h[t + 1])
        assert np.array_equal(cn.astype(np.float32), ro.c[t + 1])
        assert np.array_equal(tol_l, ro.tol_l[t])
        assert np.array_equal(np.stack(pre), ro.pre[t])
        s1 = L.env_step(ro.s[t], logits[:, 1] > logits[:, 0], c.A, c.B)[0]
        assert np.array_equal(s1.astype(np.float32), ro.s[t + 1])
    empty = L.rollout(S.policy_for(c, S.OFFSET), c.mu, c.nu, 15, c.A, c.B,
                      ro.s[0], 0)
    assert empty.s.shape == (1, 64, 4) and empty.x.size == 0
    assert empty.c.shape == (1, 64, 64) and not empty.c.any()


def test_slip_and_with_pre_leave_the_default_cell_alone():
    c = S.case("base")
    ro, pol = S.trajectory("base", S.OFFSET), S.policy_for(c, S.OFFSET)
    plain = L.cell(pol, ro.x[50], ro.h[50], ro.c[50])
    more = L.cell(pol, ro.x[50], ro.h[50], ro.c[50], with_pre=True)
    assert len(plain) == 6 and len(more) == 7 and len(more[6]) == 4
    for a, b in zip(plain, more):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(AssertionError):
        L.cell(pol, ro.x[50], ro.h[50], ro.c[50], slip="no_such_slip")


# ---- 2. conditions --------------------------------------------------------------

@pytest.mark.parametrize("name", S.SETS + ("saturated0",))
def test_seed_meets_the_decided_cap_and_rejected_ones_do_not(name):
    seed = S.SEEDS[name]
    for m in S.MEMBERS:
        share = S.decided(S.trajectory(name, m)).mean(-1)
        hs = list(S.case(name).horizons)
        print("%s member %d: decided share at h %s = %s"
              % (name, m, hs, np.round(share[hs], 3)))
        assert (share[hs] >= S.CAP).all(), (name, m, share[hs])
    rejected = S.SEEDS_REJECTED[name]
    assert tuple(s for s, _ in rejected) == tuple(range(S.WORLD_SEED, seed))
    for bad, share in rejected:
        got = S.least_share(name, bad)
        assert got < S.CAP and abs(got - share) < 1e-9, (name, bad, got)
    assert S.OFFSET % 2 == 0 and S.POP == 4


def test_decided_cap_of_every_step_masks_and_the_far_members():
    every = S.least_share("base", horizons=range(S.H_TOP))
    masks = min(float(S.decided(S.trajectory("base", m, mask, 4))
                      [list(S.H_MASK)].mean(-1).min())
                for m in S.MEMBERS for mask in S.MASKS)
    far = S.least_share("base", horizons=(S.FAR_H,), members=range(
        S.FAR_OFFSET, S.FAR_OFFSET + S.FAR_POP))
    serving = min(S.least_share(name, horizons=(h,), members=S.MEMBERS[:2])
                  for name, h in S.SERVING)
    print("least decided share: every h %.3f, masks %.3f, far %.3f, "
          "serving %.3f" % (every, masks, far, serving))
    assert min(every, masks, far, serving) >= S.CAP
    assert S.FAR_OFFSET % 2 == 0 and S.FAR_OFFSET >> 1 == 16383


def test_clamp_set_is_on_the_floor_and_fires_in_both_signs():
    base, c = S.case("base"), S.case("clamp")
    assert (c.nu[:2].view(np.uint32)
            == np.float32(1e-2).view(np.uint32)).all()
    assert np.array_equal(c.nu[2:], base.nu[2:])
    assert np.array_equal(c.mu[[0, 2, 3]], base.mu[[0, 2, 3]])
    assert c.mu[1] == np.float32(0.45)
    # Both signs fire at every checked h in the launch's four members, and
    # in every member over the three h.  Not in every member at every h: at
    # h = 50 member 3 has all 64 envs at +5 in dim 0 and none at -5.
    per_step = {h: np.zeros(2, int) for h in S.H_CLAMP}
    for m in S.MEMBERS:
        ro = S.trajectory("clamp", m)
        total = np.zeros(2, int)
        for h in S.H_CLAMP:
            above, below = ro.x_raw[h] > 5.0, ro.x_raw[h] < -5.0
            assert (ro.x[h][above] == 5.0).all()
            assert (ro.x[h][below] == -5.0).all()
            hi, lo = above.sum(0), below.sum(0)
            print("clamp member %d h=%d: x clamped to +5 per dim %s, to -5 %s"
                  % (m, h, hi, lo))
            assert hi[:2].sum() + lo[:2].sum() >= 1, (m, h)
            assert hi[2:].sum() == 0 and lo[2:].sum() == 0, (m, h)
            # clamped and unclamped values meet in one operand
            assert (np.abs(ro.x[h][:, :2]) < 5.0).any()
            total += (hi.sum(), lo.sum())
            per_step[h] += (hi.sum(), lo.sum())
        print("clamp member %d: %d values at +5, %d at -5 over h %s"
              % (m, total[0], total[1], S.H_CLAMP))
        assert total.min() >= 1, (m, total)
    for h, n in per_step.items():
        assert n.min() >= 1, (h, n)
    # the sets before this one never reach the clamp: the gap it closes
    for name in ("base0", "base", "wide", "saturated"):
        for m in S.MEMBERS:
            assert np.abs(S.trajectory(name, m).x_raw).max() < 5.0


def test_gates_saturate_and_keep_a_share_on_the_slope():
    for name in ("wide", "saturated"):
        for m in S.MEMBERS:
            sat = [S.saturation(S.trajectory(name, m), h) for h in S.H_DEEP]
            print("%s member %d: (min pre, max pre, share on the slope) per "
                  "h %s" % (name, m, [tuple(np.round(v, 3)) for v in sat]))
            for h, (lo, hi, mid) in zip(S.H_DEEP, sat):
                assert mid >= MID_DEEP, (name, m, h, mid)
                # what is met of the two ends of exp2 (WIDE_OVERFLOW)
                over = name == "wide" and h in WIDE_OVERFLOW.get(m, ())
                assert (lo < S.PRE_OVERFLOW) == over, (name, m, h, lo)
                assert hi < S.PRE_UNDERFLOW, (name, m, h, hi)
            if name == "saturated":
                # theta x 8 at h = 8: gates on the slope, c still small
                assert sat[0][2] >= MID_SATURATED
            assert min(lo for lo, _hi, _mid in sat) < -PRE_FAR
            assert max(hi for _lo, hi, _mid in sat) > PRE_FAR


def test_cell_state_at_depth_is_not_the_one_of_the_first_steps():
    for m in S.MEMBERS:
        ro = S.trajectory("saturated", m)
        top = float(np.abs(ro.c[S.H_TOP]).max())
        # max |c| of the (h, h + 1) pair at 199, per member
        print("saturated member %d: max |c| %.2f at h = 199, %.2f after step "
              "199" % (m, np.abs(ro.c[199]).max(), top))
        assert top >= C_BF16_COARSE
        assert np.abs(ro.c[199]).max() >= C_BF16_COARSE
        ro = S.trajectory("base", m)
        early = float(np.abs(ro.c[:9]).max())
        deep = float(np.abs(ro.c[199]).max())
        print("base member %d: max |c| %.3f at h <= 8, %.3f at h = 199"
              % (m, early, deep))
        assert early < C_DEPTH < deep


def test_serving_comparison_leaves_out_few_envs_and_reaches_large_c():
    for name, h in S.SERVING:
        c = S.case(name)
        assert c.sigma == 0.0
        for m in S.MEMBERS[:2]:
            ro = S.trajectory(name, m)
            _x, slack = L.observe(ro.s[h], c.mu, c.nu)
            assert slack.any(-1).mean() < 0.10, (name, m, h)
    sat, sat0 = S.case("saturated"), S.case("saturated0")
    assert np.array_equal(sat.theta, sat0.theta) and sat0.seed == sat.seed
    top = float(np.abs(S.trajectory("saturated0", S.OFFSET).c[199]).max())
    print("saturated0: max |c| %.2f at h = 199" % top)
    assert top >= C_BF16_COARSE


# ---- 3. the tolerances stay sharp ------------------------------------------------

# slip: (index of the output it acts on, index of that output's tolerance)
_SLIPS = {"c_rounded": (1, 4), "if_swapped": (1, 4), "tanh_c_old": (0, 3),
          "h_rounded": (2, 5)}


@pytest.mark.parametrize("slip", sorted(_SLIPS))
@pytest.mark.parametrize("name", S.SETS)
def test_tolerance_catches_slip_on_every_set(name, slip):
    """At every checked h of every set and for every member.  ``c_rounded``
    and ``if_swapped`` are held by tol_c, ``tanh_c_old`` by tol_h,
    ``h_rounded`` by tol_l.  ``tanh_c_old`` cannot show on a unit whose c and
    c' both lie beyond +-TANH_FLAT with one sign (up to 35 % of the units of
    "saturated" at h = 199): that it does not is asserted, and so is that it
    shows on other units of the same step."""
    c = S.case(name)
    out, tol = _SLIPS[slip]
    for h in c.horizons:
        worst = []
        for m in S.MEMBERS:
            ro, pol = S.trajectory(name, m), S.policy_for(c, m)
            want = L.cell(pol, ro.x[h], ro.h[h], ro.c[h])
            got = L.cell(pol, ro.x[h], ro.h[h], ro.c[h], slip=slip)
            moved = np.abs(got[out] - want[out]) / want[tol]
            if slip == "tanh_c_old":
                c0, c1 = ro.c[h].astype(np.float64), want[1]
                flat = (np.minimum(np.abs(c0), np.abs(c1)) > TANH_FLAT) \
                    & (np.sign(c0) == np.sign(c1))
                assert not moved[flat].any(), (name, h, m)
                if name == "saturated" and h >= 49:
                    assert flat.mean() > 0.10, (name, h, m, flat.mean())
                moved = moved[~flat]
            worst.append(float(moved.max()))
        print("%s h=%d %s: moves its output by %s tolerances per member"
              % (name, h, slip, ["%.3g" % w for w in worst]))
        assert min(worst) > 1.0, (name, h, slip, worst)
        if slip == "c_rounded" and name == "saturated" and h == 199:
            # |c| up to 199: the rounding moves c by up to 0.5, tol_c is
            # about |c| EPS_SIG = 2e-4
            print("c_rounded on saturated at h = 199: %.0f tol_c at least"
                  % min(worst))
            assert min(worst) > 1000.0


# ---- 4. stand-in kernels that must fail ---------------------------------------

def _failing(v):
    return sorted(k for k, r in v.worst.items() if not r <= 1.0)


@pytest.mark.parametrize("name", S.SETS)
def test_sound_standin_passes_every_case(name):
    for h in S.case(name).horizons:
        v = S.standin_verdict(name, 0b1111, None, h)
        print(name, h, {k: round(r, 4) for k, r in v.worst.items()})
        assert S.passes(v), (name, h, v.worst)
        assert min(v.shares) >= S.CAP


def test_sound_standin_passes_every_mask():
    for mask in S.MASKS:
        for h in S.H_MASK:
            v = S.standin_verdict("base", mask, None, h, top=4)
            assert S.passes(v) and min(v.shares) >= S.CAP, (mask, h, v.worst)


@pytest.mark.parametrize("defect", ["no_clamp", "clamp_4"])
def test_missing_or_wrong_clamp_fails(defect):
    for h in S.H_CLAMP:
        v = S.standin_verdict("clamp", 0b1111, defect, h)
        print(defect, h, v.worst)
        assert "h" in _failing(v) and "c" in _failing(v)
    # where the clamp never fires the defect is no defect
    assert S.passes(S.standin_verdict("base", 0b1111, defect, 8))


def test_ignored_or_reversed_mask_fails():
    for mask in S.MASKS:
        mirror = sum(((mask >> d) & 1) << (3 - d) for d in range(4))
        for h in S.H_MASK:
            ign = S.standin_verdict("base", mask, "mask_ignored", h, top=4)
            rev = S.standin_verdict("base", mask, "mask_reversed", h, top=4)
            assert ("c" in _failing(ign)) == (mask != 0b1111), (mask, h)
            # a palindrome (0, 6, 9, 15) reads the same in both orders
            assert ("c" in _failing(rev)) == (mask != mirror), (mask, h)


def test_hidden_dims_left_out_of_the_statistics_fails():
    for mask in (0b0011, 0b0000, 0b1110):
        for h in S.H_MASK:
            v = S.standin_verdict("base", mask, "stats_skip_hidden", h, top=4)
            assert _failing(v) == ["stat"], (mask, h, v.worst)


# defect: the quantities it must fail through
_STATE_DEFECTS = {
    "wrong_parity": ("c", "h"),
    "h_carried_bf16": ("h",),
    "c_carried_bf16": ("c",),
    "c_tiles_swapped": ("c",),
    "hfin_stale": ("h",),
    "cell_stale": ("c",),
    "gates_fo_swapped": ("c", "h"),
}


@pytest.mark.parametrize("name", S.SETS)
@pytest.mark.parametrize("defect", sorted(_STATE_DEFECTS))
def test_wrong_carried_state_fails_every_case(name, defect):
    for h in S.case(name).horizons:
        v = S.standin_verdict(name, 0b1111, defect, h)
        print(defect, name, h, v.worst)
        for k in _STATE_DEFECTS[defect]:
            assert k in _failing(v), (name, h, k, v.worst)


def test_final_hidden_not_zeroed_fails_at_horizon_0():
    """The hfin tile is written at the last step only: at horizon 0 it
    returns what it held.  The comparison restarts from it, the kernel
    started from zeros."""
    runs = S.standin_runs("base", 0b1111, "hfin_not_zeroed", 2)
    assert runs[0][3].any() and not runs[0][4].any()
    v = S.compare_pair(S.case("base"), S.OFFSET, 0b1111, 0, runs[0], runs[1])
    print("hfin_not_zeroed", v.worst)
    assert "h" in _failing(v)
    # one step later nothing is left of it
    assert S.passes(S.compare_pair(S.case("base"), S.OFFSET, 0b1111, 1,
                                   runs[1], runs[2]))
    sound = S.standin_runs("base", 0b1111, None, 2)
    assert not sound[0][3].any()
    assert S.passes(S.compare_pair(S.case("base"), S.OFFSET, 0b1111, 0,
                                   sound[0], sound[1]))


def test_restart_from_zeros_fails():
    """Guards the test itself: the oracle step must start from the kernel's
    own hidden and cell state, not from the start of the episode."""
    for name in S.SETS:
        h = S.case(name).horizons[-1]
        runs = S.standin_runs(name, 0b1111, None,
                              max(S.case(name).horizons) + 1,
                              S.standin_horizons(name))
        f, st, s, hid, cel = runs[h]
        v = S.compare_pair(S.case(name), S.OFFSET, 0b1111, h,
                           (f, st, s, np.zeros_like(hid), cel), runs[h + 1])
        assert "h" in _failing(v), (name, v.worst)
        v = S.compare_pair(S.case(name), S.OFFSET, 0b1111, h,
                           (f, st, s, hid, np.zeros_like(cel)), runs[h + 1])
        assert "c" in _failing(v), (name, v.worst)


def test_nan_fails():
    runs = S.standin_runs("base", 0b1111, None, max(S.H_DEEP) + 1,
                          S.standin_horizons("base"))
    for field in range(5):
        bad = [a.copy() for a in runs[9]]
        bad[field].reshape(-1)[-1] = np.nan
        assert not S.passes(S.compare_pair(S.case("base"), S.OFFSET, 0b1111,
                                           8, runs[8], tuple(bad))), field
    wrong_count = [a.copy() for a in runs[9]]
    wrong_count[1][8] += 1
    assert not S.passes(S.compare_pair(S.case("base"), S.OFFSET, 0b1111, 8,
                                       runs[8], tuple(wrong_count)))
    # a NaN in the first member is not covered up by the members after it
    nan = float("nan")
    assert S.worse(0.5, nan) != S.worse(0.5, nan)
    assert S.worse(nan, 0.5) != S.worse(nan, 0.5)
    assert S.worse(0.25, 0.5) == S.worse(0.5, 0.25) == 0.5
    bad = [a.copy() for a in runs[9]]
    bad[4][0, 0, 0] = np.nan
    v = S.compare_pair(S.case("base"), S.OFFSET, 0b1111, 8, runs[8],
                       tuple(bad))
    assert v.worst["c"] != v.worst["c"] and not S.passes(v)


@pytest.mark.parametrize("name", [n for n in S.SETS if n != "base0"])
def test_unflipped_sign_of_the_odd_members_fails(name):
    runs = S.standin_runs(name, 0b1111, "sign_not_flipped",
                          max(S.case(name).horizons) + 1,
                          S.standin_horizons(name))
    for h in S.case(name).horizons:
        v = S.standin_verdict(name, 0b1111, "sign_not_flipped", h)
        assert "h" in _failing(v) and "c" in _failing(v), (name, h, v.worst)
        # the even members alone would pass: the defect is in the odd ones
        for i, member in enumerate(S.MEMBERS):
            got, _share = S.compare_member(
                S.case(name), member, 0b1111, h, runs[h][2][i],
                runs[h][3][i], runs[h][4][i], runs[h + 1][2][i],
                runs[h + 1][3][i], runs[h + 1][4][i], runs[h][0][i],
                runs[h + 1][0][i])
            assert (got["c"] <= 1.0) == (member % 2 == 0), (name, h, member)
    # sigma 0: both signs are the same policy
    assert S.passes(S.standin_verdict("base0", 0b1111, "sign_not_flipped", 8))


@pytest.mark.parametrize("name", S.SETS)
def test_dropped_or_stale_reward_fails(name):
    """A dropped reward fails everywhere.  A reward taken from the old
    state fails at every h <= 50; at h = 199 the fitness tolerance, which
    grows with h, may no longer tell consecutive rewards apart: the ratio is
    printed and the verdict stated either way (profiles/lstm.md)."""
    for h in S.case(name).horizons:
        v = S.standin_verdict(name, 0b1111, "reward_dropped", h)
        assert _failing(v) == ["f"], (name, h, v.worst)
        v = S.standin_verdict(name, 0b1111, "reward_old_state", h)
        print("reward_old_state", name, h, "f ratio %.3g" % v.worst["f"])
        if h <= 50:
            assert _failing(v) == ["f"], (name, h, v.worst)
        else:
            assert _failing(v) in ([], ["f"])
