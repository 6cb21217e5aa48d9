"""GPU tests of what ``ConvESEngine.rollout`` builds out of the conv
kernels: the per-chunk slices, the Philox pair of each member, the noise
step, the iteration read inside a captured graph, state / racc carried
from step to step and reset between rollouts.

Teacher-forced, one step at a time (tests/conv_rollout_cases.py): an engine
of horizon h-1 supplies what went into step h of an engine of horizon h,
and every layer of that step is checked against the fp64 references of
fiber_amd/es/conv_reference.py on the device's own inputs.  If the two
engines differed in their first h-1 steps, the observation built from
state_{h-1} would fail layer 1.  The CPU side
(tests/test_conv_rollout_chain.py) shows the check rejects each slicing,
pair-index, noise-step, reset and carry slip; the seeds were chosen there.

Run with ``-s`` for the figures of profiles/conv_rollout_chain.md.
"""

import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import conv_rollout_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

if torch.cuda.is_available():
    from fiber_amd.es.conv_policy import ConvESConfig, ConvESEngine

BUFFERS = ("racc", "state", "act1", "act2", "act3", "znoise", "wpert",
           "w1_fp8", "w3_fp8")


class StubCtx:
    """rollout() reads only .rank and .size."""

    def __init__(self, rank, size):
        self.rank, self.size = rank, size


def _engine(case, horizon, use_graph=True):
    cfg = ConvESConfig(pop_per_gpu=case["pop"], horizon=horizon,
                       sigma=C.SIGMA, seed=case["seed"])
    ctx = StubCtx(case["rank"], case["world"]) if case["world"] > 1 else None
    eng = ConvESEngine(cfg, ctx=ctx, device=torch.device("cuda"))
    if not use_graph:
        eng.use_graph = False
    return eng


def _run(case, horizon, use_graph=True):
    """The case's call sequence on a fresh engine of this horizon; returns
    (engine, CPU buffers)."""
    eng = _engine(case, horizon, use_graph)
    if case["capture"] is not None:
        eng.rollout(case["capture"])
    fit = eng.rollout(case["iteration"])
    torch.cuda.synchronize()
    assert len(eng._half_streams) == case["chunks"]
    if use_graph:
        assert eng._graph is not None, "graph capture did not engage"
    else:
        assert eng._graph is None
    bufs = {k: getattr(eng, k).cpu() for k in BUFFERS}
    bufs["fitness"] = fit.cpu()
    return eng, bufs


def _const(eng, case, t):
    return dict(seed=case["seed"], iteration=case["iteration"], t=t,
                chunks=case["chunks"], gtab_bf=eng.gtab_bf.cpu(),
                env_A=eng.env_A.cpu(), env_B=eng.env_B.cpu(),
                theta=eng.theta.cpu(), sigma=C.SIGMA, rank=case["rank"],
                world=case["world"], pop_per_gpu=case["pop"],
                capture=case["capture"])


def _check_case(name, use_graph=True, perturb_members=None):
    """Steps h of the case, each against the engine of horizon h-1.  At
    most 2 undecided envs per step (asserted by check_step before any
    comparison), >= 4 distinct decided actions over the case."""
    case = C.CASES[name]
    t0 = time.time()
    if perturb_members is None:
        perturb_members = C.chunk_corner_members(case["pop"], case["chunks"])
    hs = case["horizons"]
    runs = {h: _run(case, h, use_graph) for h in range(min(hs) - 1,
                                                       max(hs) + 1)}
    actions = set()
    for h in hs:
        eng, cur = runs[h]
        rep = C.check_step(runs[h - 1][1], cur, _const(eng, case, h - 1),
                           max_undecided=2, perturb_members=perturb_members)
        print(C.format_report(name, h, rep))
        assert rep["undecided"] <= 2
        actions |= set(rep["actions"])
    assert len(actions) >= 4, actions
    print("%s: %.1f s" % (name, time.time() - t0))
    return runs


@requires_gpu
def test_two_chunks_replay_at_another_iteration(monkeypatch):
    """pop 8 in 2 chunks; rollout(0) captures the graph, rollout(3) is
    checked, all members, h = 1, 2, 3: the iteration is not baked into the
    graph and racc is reset."""
    monkeypatch.setenv("FAM_CONV_STREAMS", "2")
    runs = _check_case("two_chunks")
    for eng, _ in runs.values():
        assert len(eng._half_streams) == 2 and eng._graph is not None


@requires_gpu
def test_default_eight_chunks(monkeypatch):
    """The 8-branch graph the conv benchmark measures, at the smallest
    population that keeps 8 chunks; all members, chunk by chunk."""
    monkeypatch.delenv("FAM_CONV_STREAMS", raising=False)
    runs = _check_case("eight_chunks")
    for eng, _ in runs.values():
        assert len(eng._half_streams) == 8 and eng._graph is not None


@requires_gpu
def test_single_chunk_eager(monkeypatch):
    monkeypatch.delenv("FAM_CONV_STREAMS", raising=False)
    runs = _check_case("single_eager", use_graph=False,
                       perturb_members=[0, 1])
    for eng, _ in runs.values():
        assert len(eng._half_streams) == 1 and eng._graph is None


@requires_gpu
def test_second_shard(monkeypatch):
    """rank 1 of 2, pop 4: wpert belongs to pairs 2 and 3 (check_step's
    wpert stage, all four members), and differs from a rank-0 engine's."""
    monkeypatch.delenv("FAM_CONV_STREAMS", raising=False)
    case = C.CASES["second_shard"]
    runs = _check_case("second_shard", perturb_members=[0, 1, 2, 3])
    assert runs[1][0].rank == 1 and runs[1][0].world == 2
    _, rank0 = _run(dict(case, rank=0, world=1), 0)
    for m in range(4):
        assert not torch.equal(rank0["wpert"][m], runs[1][1]["wpert"][m])


@requires_gpu
def test_graph_matches_eager_with_branches(monkeypatch):
    """2 chunks, pop 8, horizon 3, iteration 5 after a capture at
    iteration 1: every buffer of the graphed engine equals the eager
    engine's bit for bit."""
    monkeypatch.setenv("FAM_CONV_STREAMS", "2")
    case = dict(C.CASES["two_chunks"], capture=1, iteration=5)
    eager, be = _run(case, 3, use_graph=False)
    graphed, bg = _run(case, 3)
    assert len(eager._half_streams) == 2 and len(graphed._half_streams) == 2
    assert graphed._graph is not None and eager._graph is None
    for k in BUFFERS + ("fitness",):
        a, b = be[k], bg[k]
        if a.dtype in (torch.bfloat16, torch.float32):
            a = a.view(torch.int16 if a.dtype == torch.bfloat16
                       else torch.int32)
            b = b.view(a.dtype)
        if k == "wpert":  # the alignment pad is nobody's to write
            a, b = a[:, :C.cr.NP_CONV], b[:, :C.cr.NP_CONV]
        assert torch.equal(a, b), (k, int((a != b).sum()))
