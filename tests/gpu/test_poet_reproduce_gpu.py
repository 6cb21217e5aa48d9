"""GPU tests of the growable ESPopulation (add_pairs, remove_pairs) and of
poet.reproduce.  P = 3, pop = 8, horizon = 8.

A pair added to a population must be, bit for bit and field by field, the
ESEngine its documentation names: built with the new pair's seed and
environment and loaded with the donor's engine_state, moments zeroed.
Pairs that were not touched must not notice that the population grew or
shrank.  reproduce must admit the children that select_children names on
the numpy oracle's novelties, with the oracle's donors.
"""

import dataclasses

import numpy as np
import pytest
import torch

from fiber_amd.es import novelty_oracle as no

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

if torch.cuda.is_available():
    from fiber_amd import ops
    from fiber_amd.es import (ESConfig, ESEngine, ESPopulation,
                              propose_children, reproduce, select_children)
    from fiber_amd.es import engine as es_engine

SEEDS = [1234, 0x9E3779B9, (1 << 32) + 77]
NEW_SEEDS = [4321, 0xFFFFFFFF]
_ENGINE_FIELDS = ("theta", "adam_m", "adam_v", "obs_sum", "obs_sumsq",
                  "obs_count", "obs_mu", "obs_nu")
_ALL_FIELDS = _ENGINE_FIELDS + ("env_A", "env_B")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cfg():
    return ESConfig(pop_per_gpu=8, horizon=8)


def _envs(first, count):
    return [es_engine.make_env_params(first + i, "cpu") for i in range(count)]


def _population(steps=1):
    pop = ESPopulation(_cfg(), SEEDS, _envs(200, 3),
                       device=torch.device("cuda", 0))
    for _ in range(steps):
        pop.step()
    return pop


def _engine_for_new_pair(pop, donor, seed, env):
    """The engine add_pairs promises, from the pre-call state of pop."""
    eng = ESEngine(dataclasses.replace(pop.cfg, seed=seed), ctx=None,
                   device=pop.device, env_params=env)
    state = pop.engine_state(donor)
    state["adam_m"] = torch.zeros_like(state["adam_m"])
    state["adam_v"] = torch.zeros_like(state["adam_v"])
    eng.load_state_dict(state)
    return eng


def _assert_row_is_engine(pop, p, eng, what):
    for f in _ENGINE_FIELDS:
        assert _same_bits(getattr(pop, f)[p], getattr(eng, f)), (what, p, f)
    assert _same_bits(pop.env_A[p], eng.env_A), (what, p)
    assert _same_bits(pop.env_B[p], eng.env_B), (what, p)
    assert pop.t_step == eng.t_step


@requires_gpu
def test_added_pairs_are_their_engines_and_the_rest_is_untouched():
    pop, never_grew = _population(), _population()
    new_envs = _envs(300, 2)
    donors = [2, 0]
    engines = [_engine_for_new_pair(pop, donors[i], NEW_SEEDS[i],
                                    new_envs[i]) for i in range(2)]
    assert pop.adam_m[2].any()  # the donor's moments are not zero

    pop.add_pairs(NEW_SEEDS, new_envs, donors)
    assert pop.P == len(pop) == 5 and pop.seeds == SEEDS + NEW_SEEDS
    assert pop._seeds_dev.tolist() == ops.pair_seeds(SEEDS + NEW_SEEDS,
                                                     "cpu").tolist()
    for f in _ALL_FIELDS:
        assert getattr(pop, f).shape[0] == 5 and \
            getattr(pop, f).is_contiguous(), f
    for i in range(2):
        _assert_row_is_engine(pop, 3 + i, engines[i], "added")
        assert not pop.adam_m[3 + i].any() and not pop.adam_v[3 + i].any()
    assert _same_bits(pop.theta[3], pop.theta[2])
    assert _same_bits(pop.theta[4], pop.theta[0])

    for step in range(2):
        stats = pop.step()
        never_grew.step()
        for eng in engines:
            eng.step()
        for i in range(2):
            _assert_row_is_engine(pop, 3 + i, engines[i], "step %d" % step)
        for f in _ALL_FIELDS:
            assert _same_bits(getattr(pop, f)[:3], getattr(never_grew, f)), f
    assert stats["fitness_mean"].shape == (5,)
    # same policy, other seed and environment: the pairs have parted
    assert not torch.equal(pop.theta[3], pop.theta[2])
    assert pop.theta.unique(dim=0).shape[0] == 5

    # argument checks leave the population alone
    with pytest.raises(IndexError):
        pop.add_pairs([1], _envs(400, 1), [5])
    with pytest.raises(ValueError):
        pop.add_pairs([1, 2], _envs(400, 1), [0, 0])
    with pytest.raises(ValueError):
        pop.add_pairs([1], [(torch.zeros(3, 4), torch.zeros(4))], [0])
    pop.add_pairs([], [], [])
    assert pop.P == 5


@requires_gpu
def test_remove_pairs_leaves_the_survivors_on_their_course():
    pop, whole = _population(), _population()
    new_envs = _envs(300, 2)
    for p in (pop, whole):
        p.add_pairs(NEW_SEEDS, new_envs, [2, 0])
        p.step()
    env_A, env_B, seeds = pop.remove_pairs([3, 1])
    assert seeds == [SEEDS[1], NEW_SEEDS[0]]
    assert _same_bits(env_A, whole.env_A[[1, 3]])
    assert _same_bits(env_B, whole.env_B[[1, 3]])
    keep = [0, 2, 4]
    assert pop.P == 3 and pop.seeds == [whole.seeds[p] for p in keep]
    assert pop._seeds_dev.tolist() == whole._seeds_dev[keep].tolist()
    for step in range(2):
        for f in _ALL_FIELDS:
            got = getattr(pop, f)
            assert got.is_contiguous() and \
                _same_bits(got, getattr(whole, f)[keep]), (step, f)
        pop.step()
        whole.step()
    assert pop.t_step == whole.t_step

    with pytest.raises(ValueError):
        pop.remove_pairs([0, 1, 2])
    with pytest.raises(IndexError):
        pop.remove_pairs([3])
    with pytest.raises(IndexError):
        pop.remove_pairs([-1])
    assert pop.P == 3
    none = pop.remove_pairs([])
    assert none[0].shape == (0, 4, 4) and none[2] == [] and pop.P == 3


@requires_gpu
def test_state_dict_round_trips_after_growth():
    pop = _population()
    new_envs = _envs(300, 2)
    pop.add_pairs(NEW_SEEDS, new_envs, [2, 0])
    pop.step()
    state = pop.state_dict()
    assert state["seeds"] == SEEDS + NEW_SEEDS
    assert state["theta"].shape[0] == state["env_A"].shape[0] == 5
    twin = ESPopulation(pop.cfg, state["seeds"],
                        list(zip(state["env_A"], state["env_B"])),
                        device=pop.device)
    twin.load_state_dict(state)
    pop.step()
    twin.step()
    for f in _ALL_FIELDS:
        assert _same_bits(getattr(pop, f), getattr(twin, f)), f
    assert twin.t_step == pop.t_step == 3
    # a population that has not grown refuses the state
    with pytest.raises(ValueError):
        _population(0).load_state_dict(state)


def _reproduce_args(**over):
    args = dict(repro_threshold=-float("inf"), n_children=6,
                mutate_scale=0.3, mc_lo=-float("inf"), mc_hi=float("inf"),
                clip_lo=-100.0, clip_hi=100.0, knn=1, max_admit=2,
                max_pairs=4, child_seeds=[9000 + c for c in range(6)],
                horizon=8, seed=77, iteration=3)
    args.update(over)
    return args


@requires_gpu
def test_reproduce_admits_what_the_oracle_names():
    pop = _population(2)
    dev = pop.device
    P = 3
    archive = (torch.stack([e[0] for e in _envs(500, 2)]),
               torch.stack([e[1] for e in _envs(500, 2)]))
    scores = pop.transfer_matrix(8, 77, 3)

    # what reproduce will see, from the same seeded proposals
    base = _reproduce_args()
    child_A, child_B, parent_of = propose_children(
        pop.env_A, pop.env_B, [0, 1, 2], 6, base["mutate_scale"],
        torch.Generator().manual_seed(21))
    assert parent_of == [0, 1, 2, 0, 1, 2]
    all_A = torch.cat([pop.env_A, archive[0].to(dev), child_A.to(dev)])
    all_B = torch.cat([pop.env_B, archive[1].to(dev), child_B.to(dev)])
    all_scores = ops.es_eval_matrix(pop.theta, pop.obs_mu, pop.obs_nu,
                                    all_A.contiguous(), all_B.contiguous(),
                                    77, 3, 8).cpu().numpy()
    n_ref = P + 2
    child_scores = all_scores[:, n_ref:]
    assert np.isfinite(all_scores).all()
    # clip the middle half of the score range; the minimal criterion lets
    # the harder half of the children through
    lo_s, hi_s = float(all_scores.min()), float(all_scores.max())
    clip_lo = lo_s + 0.25 * (hi_s - lo_s)
    clip_hi = lo_s + 0.75 * (hi_s - lo_s)
    best = child_scores.max(axis=0)
    mc_hi = float(np.sort(best)[3])
    passed = best <= mc_hi
    assert 0 < passed.sum() < 6
    codes = no.codes_oracle(all_scores, clip_lo, clip_hi)
    # knn = 1: with 3 agents the distances are small integers, and one
    # square root orders them the same way in fp32 and fp64
    _d2, want_nov = no.knn_oracle(codes, n_ref, 1)
    want_admit = select_children(torch.from_numpy(want_nov),
                                 torch.from_numpy(passed), 2)
    assert len(want_admit) == 2
    want_donors = [int(np.argmax(child_scores[:, c])) for c in want_admit]

    before = {f: getattr(pop, f).clone() for f in _ALL_FIELDS}
    record = reproduce(pop, scores, archive=archive,
                       generator=torch.Generator().manual_seed(21),
                       **_reproduce_args(mc_hi=mc_hi, clip_lo=clip_lo,
                                         clip_hi=clip_hi))
    assert record["parents"] == [0, 1, 2]
    assert record["parent_of"] == parent_of
    assert torch.equal(record["child_A"], child_A)
    assert record["passed"].tolist() == passed.tolist()
    nov = record["novelty"].double().numpy()
    assert (np.abs(nov - want_nov) <= no.novelty_bound(want_nov, 1)).all()
    assert record["admitted"] == want_admit
    assert record["donors"] == want_donors

    # 3 + 2 pairs over max_pairs = 4: the oldest pair retires
    r_A, r_B, r_seeds = record["retired"]
    assert r_seeds == [SEEDS[0]]
    assert _same_bits(r_A, before["env_A"][:1])
    assert _same_bits(r_B, before["env_B"][:1])
    assert pop.P == 4
    assert pop.seeds == SEEDS[1:] + [9000 + c for c in want_admit]
    for f in _ALL_FIELDS:  # the survivors kept every bit
        assert _same_bits(getattr(pop, f)[:2], before[f][1:]), f
    for i, (c, d) in enumerate(zip(want_admit, want_donors)):
        row = 2 + i
        for f in ("theta", "obs_sum", "obs_sumsq", "obs_count", "obs_mu",
                  "obs_nu"):
            assert _same_bits(getattr(pop, f)[row], before[f][d]), (f, c)
        assert not pop.adam_m[row].any() and not pop.adam_v[row].any()
        assert _same_bits(pop.env_A[row], child_A[c].to(dev))
        assert _same_bits(pop.env_B[row], child_B[c].to(dev))
    pop.step()  # the grown population still steps
    assert torch.isfinite(pop.theta).all()


@requires_gpu
def test_reproduce_without_parents_or_passing_children_changes_nothing():
    pop = _population(1)
    scores = pop.transfer_matrix(8, 77, 3)
    before = pop.theta.clone()
    record = reproduce(pop, scores, generator=torch.Generator().manual_seed(1),
                       **_reproduce_args(repro_threshold=float("inf")))
    assert record["parents"] == [] and record["admitted"] == []
    assert record["retired"][2] == [] and pop.P == 3
    # parents, but no child passes the minimal criterion
    record = reproduce(pop, scores, generator=torch.Generator().manual_seed(1),
                       **_reproduce_args(mc_lo=1e9, mc_hi=2e9))
    assert record["parents"] == [0, 1, 2] and len(record["parent_of"]) == 6
    assert record["passed"].tolist() == [False] * 6
    assert record["admitted"] == [] and record["donors"] == []
    assert pop.P == 3 and pop.seeds == SEEDS
    assert _same_bits(pop.theta, before)
    # a subset of the parents: only the pair with the best own score
    diag = scores.diagonal().cpu()
    record = reproduce(pop, scores, generator=torch.Generator().manual_seed(1),
                       **_reproduce_args(repro_threshold=float(diag.max()),
                                         max_admit=0))
    assert record["parents"] == [int(diag.argmax())]
    assert set(record["parent_of"]) == {int(diag.argmax())}
    assert pop.P == 3
