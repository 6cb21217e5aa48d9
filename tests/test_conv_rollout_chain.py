"""CPU tests of the teacher-forced rollout-step check
(tests/conv_rollout_cases.py): it accepts an fp32 emulation of
``ConvESEngine._rollout_body`` on every element, with either legal
evaluation of the observation, and rejects each chain slip the per-layer
tests cannot see, applied one at a time.  The GPU side is
tests/gpu/test_conv_rollout_chain_gpu.py.

Run with ``-s`` for the figures of profiles/conv_rollout_chain.md.
"""

import pytest
import torch

import conv_rollout_cases as C
from fiber_amd.es import conv_reference as cr

TWO = C.CASES["two_chunks"]


def _case_const(case):
    return C.EmuEngine(case, 0).const(0)


def check_case(case, bufs, steps=None, **kw):
    """check_step for every step of the case; returns {h: report}."""
    const = _case_const(case)
    members = C.chunk_corner_members(case["pop"], case["chunks"])
    kw.setdefault("perturb_members", members)
    return {h: C.check_step(bufs[h - 1], bufs[h], dict(const, t=h - 1), **kw)
            for h in (steps or case["horizons"])}


@pytest.fixture(scope="module")
def honest():
    return C.emulate_case(TWO)


# ---------------------------------------------------------------------------
# emulation
# ---------------------------------------------------------------------------


def test_checker_accepts_emulation_on_every_element(honest):
    """Two chunks, pop 8, rollout(0) then rollout(3), h = 1, 2, 3, under
    the conditions the GPU case asserts: no undecided env, every gap above
    4x the largest bound, >= 4 distinct actions."""
    reps = check_case(TWO, honest, max_undecided=0)
    actions = set()
    for h, rep in reps.items():
        print(C.format_report("two_chunks (emulation)", h, rep))
        assert rep["undecided"] == 0 and rep["decided"] == TWO["pop"] * C.E
        assert rep["min_gap_over_bound"] > 4.0
        assert rep["neighbour_miss"] > 0.99
        assert max(rep["margins"].values()) <= 1.0
        actions |= set(rep["actions"])
    assert len(actions) >= 4
    # the inputs are not vacuous: racc accumulates, state moves, chunks and
    # members differ
    assert float(honest[3]["racc"].min()) > 2.0
    assert not torch.equal(honest[2]["state"], honest[3]["state"])
    assert not torch.equal(honest[3]["act3"][:64], honest[3]["act3"][64:])


@pytest.mark.parametrize("name", ["eight_chunks", "single_eager",
                                  "second_shard"])
def test_case_seed_conditions(name):
    """The seeds recorded in CASES meet the search's conditions."""
    case = C.CASES[name]
    seed, ratio = C.search_seed(name, first=case["seed"], last=case["seed"])
    assert seed == case["seed"] and ratio > 4.0


def test_checker_accepts_second_shard_emulation():
    case = C.CASES["second_shard"]
    bufs = C.emulate_case(case)
    rep = check_case(case, bufs, max_undecided=0)[1]
    print(C.format_report("second_shard (emulation)", 1, rep))
    # pairs 2 and 3, not the rank-0 engine's 0 and 1
    rank0 = C.emulate_case(dict(case, rank=0, world=1), horizons=[1])[1]
    assert not torch.equal(rank0["wpert"], bufs[1]["wpert"])


def test_checker_accepts_fma_contracted_observation():
    """``noise + s * g`` rounded once (an fma) instead of twice moves a few
    e4m3 obs bytes; an emulation built on either evaluation passes."""
    bufs = C.emulate_case(TWO, horizons=[2, 3], fused=True)
    rep = check_case(TWO, bufs, steps=[3], max_undecided=0)[3]
    print(C.format_report("two_chunks (fma emulation)", 3, rep))
    # step 3 of this case has such pixels: the test is not vacuous
    assert rep["ambiguous_pixels"] > 0


# ---------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------

# mutation -> (case, stage that must flag it)
EXPECTED = {
    "chunk1_reads_chunk0_znoise": ("two_chunks", "layer1"),
    "chunk1_uses_chunk0_znoise": ("two_chunks", "noise"),
    "noise_t_plus_1": ("two_chunks", "noise"),
    "noise_at_capture_iteration": ("two_chunks", "noise"),
    "member_offset_drops_m0": ("two_chunks", "wpert"),
    "member_offset_drops_rank": ("second_shard", "wpert"),
    "racc_sliced_at_m0_times_E": ("two_chunks", "init"),
    "racc_assigned": ("two_chunks", "head"),
    "racc_not_reset": ("two_chunks", "init"),
    "state_reinitialised_each_step": ("two_chunks", "layer1"),
    "state_not_written_back": ("two_chunks", "head"),
    "antithetic_signs_swapped": ("two_chunks", "wpert"),
}


def test_every_mutation_is_listed():
    assert set(EXPECTED) == set(C.MUTATIONS)


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_checker_rejects_mutation(mutation):
    """Both engines (horizon h-1 and h) carry the same slip, as they would
    on the device.  The first step at which the check raises, and its
    stage, are recorded."""
    name, stage = EXPECTED[mutation]
    case = C.CASES[name]
    hmax = min(2, max(case["horizons"]))
    bufs = C.emulate_case(case, mutation, horizons=range(hmax + 1))
    flagged = None
    for h in range(1, hmax + 1):
        try:
            check_case(case, bufs, steps=[h], max_undecided=0)
        except C.StageError as exc:
            flagged = (h, exc.stage, str(exc).split("\n")[0][:200])
            break
    print("%-32s %s" % (mutation, flagged))
    assert flagged is not None, "the check accepted " + mutation
    assert flagged[1] == stage, flagged


def test_checker_rejects_stale_racc_without_the_init_stage(honest):
    """The init stage is this file's addition; the head stage alone also
    sees a racc that is not reset or not accumulated (h = 2)."""
    for mutation in ("racc_not_reset", "racc_sliced_at_m0_times_E"):
        bufs = C.emulate_case(TWO, mutation, horizons=[1, 2])
        with pytest.raises(C.StageError) as ei:
            check_case(TWO, bufs, steps=[2], max_undecided=0)
        assert ei.value.stage == "head", ei.value


def _plant_tie(honest, member, last_max):
    """Member ``member`` of the step-1 buffers gets W4 = 0 and b4 =
    [0, 0, 2, 0, 2, 0]: actions 2 and 4 tie exactly on the device."""
    prev, cur = honest[0], {k: v.clone() for k, v in honest[1].items()}
    cur["wpert"][member, cr.OFF_W4:cr.OFF_B4] = 0
    cur["wpert"][member, cr.OFF_B4:cr.NP_CONV] = torch.tensor(
        [0, 0, 2.0, 0, 2.0, 0]).to(torch.bfloat16)
    rows = slice(member * C.E, (member + 1) * C.E)
    const = _case_const(TWO)
    snew, rnew = C.emu_head(cur["act3"][rows], cur["wpert"][member:member + 1],
                            prev["state"][rows], prev["racc"][member],
                            const["env_A"], const["env_B"], last_max=last_max)
    cur["state"][rows] = snew
    cur["racc"][member] = rnew
    cur["fitness"] = cur["racc"].mean(dim=1)
    return prev, cur, dict(const, t=0)


def test_planted_exact_tie_first_maximum_wins(honest):
    prev, cur, const = _plant_tie(honest, 5, last_max=False)
    rep = C.check_step(prev, cur, const, max_undecided=None)
    assert rep["undecided"] == C.E
    assert rep["taken"][5 * C.E:6 * C.E].tolist() == [2] * C.E
    prev, cur, const = _plant_tie(honest, 5, last_max=True)
    with pytest.raises(C.StageError) as ei:
        C.check_step(prev, cur, const, max_undecided=None)
    assert ei.value.stage == "head" and "member 5 env 0" in str(ei.value)
    print("last maximum on a planted tie:", str(ei.value)[:160])


def test_undecided_precondition(honest):
    prev, cur, const = _plant_tie(honest, 5, last_max=False)
    with pytest.raises(C.StageError) as ei:
        C.check_step(prev, cur, const, max_undecided=2)
    assert ei.value.stage == "precondition"


# ---------------------------------------------------------------------------
# hand-worked undecided env
# ---------------------------------------------------------------------------


def test_hand_worked_undecided_rule():
    """One member.  Only hidden units 0 and 1 are used:

        action   W4[a][0]        W4[a][1]   b4
        0        0.25            0          0
        1        0.5             0          0
        3        0.5 - 2^-9      1          0       (others: all zero)

    env 0: h = (1, 2^-9 + 2^-16): logits (0.25, 0.5, 0, 0.5 + 2^-16, 0, 0).
      The top two are actions 3 and 1, gap 2^-16 = 1.526e-5; their bounds
      256 * 2^-23 * sum|w h| are 2^-15 * (0.5 + 2^-16) and 2^-15 * 0.5, sum
      3.05e-5 > gap: undecided, candidates {1, 3}.  Action 0 is 0.25 away.
    env 1: h = (1, 0): logits (0.25, 0.5, 0, 0.5 - 2^-9, 0, 0), gap 2^-9 =
      1.95e-3 against 3.05e-5: decided, action 1.
    envs 2..15: as env 1."""
    w4 = torch.zeros(1, 6, 256)
    w4[0, 0, 0], w4[0, 1, 0] = 0.25, 0.5
    w4[0, 3, 0], w4[0, 3, 1] = 0.5 - 2.0 ** -9, 1.0
    act3 = torch.zeros(C.E, 256)
    act3[:, 0] = 1.0
    act3[0, 1] = 2.0 ** -9 + 2.0 ** -16
    w4, act3 = w4.to(torch.bfloat16), act3.to(torch.bfloat16)
    assert float(w4[0, 3, 0]) == 0.5 - 2.0 ** -9   # bf16 holds them
    assert float(act3[0, 1]) == 2.0 ** -9 + 2.0 ** -16
    hd = C.head_decisions(act3, w4.reshape(1, -1),
                          torch.zeros(1, 6, dtype=torch.bfloat16))
    assert hd["logits"][0].tolist() == [0.25, 0.5, 0, 0.5 + 2.0 ** -16, 0, 0]
    assert hd["decided"].tolist() == [False] + [True] * 15
    assert hd["cand"][0].tolist() == [False, True, False, True, False,
                                      False]
    assert hd["cand"][1].tolist() == [False, True, False, False, False,
                                      False]
    gen = torch.Generator().manual_seed(1)
    state = torch.rand(C.E, 4, generator=gen) * 2 - 1
    racc = torch.full((C.E,), 1.5)
    env_A = torch.randn(4, 4, generator=gen) * 0.5
    env_B = torch.tensor([0.7, -1.1, 0.4, 0.9])

    def device(actions):
        s, r = cr.env_step_reference(state, torch.tensor(actions), env_A,
                                     env_B, racc)
        return s.float(), r.float()

    def run(actions):
        s, r = device(actions)
        return C.check_head(state, racc, s, r, hd, env_A, env_B, t=2)

    for a0 in (1, 3):  # either near-tied action of env 0
        rep = run([a0] + [1] * 15)
        assert rep["taken"].tolist() == [a0] + [1] * 15
    for a0 in (0, 2, 5):  # a third action is rejected
        with pytest.raises(C.StageError) as ei:
            run([a0] + [1] * 15)
        assert "member 0 env 0 (undecided" in str(ei.value)
    # the decided env 1 accepts its first maximum only
    with pytest.raises(C.StageError) as ei:
        run([1, 3] + [1] * 14)
    assert "member 0 env 1 (decided" in str(ei.value)
