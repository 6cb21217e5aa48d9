"""The ES update kernels against the fp64 oracle of
fiber_amd/es/update_oracle.py (derivations in profiles/update_oracle.md):
the device Box-Muller draw by draw, es_grad / es_grad_reduce at every
chunking edge and at the conv parameter count, es_perturb against es_grad,
centered_rank on both of its paths, and a whole step() of each engine
field by field.

Tolerances, with U = 2^-24 and ULP = 2^-23:

  draw          Z_SIDE_ULPS * ULP relative to the fp64 draw
  es_grad[j]    (Z_SIDE_ULPS * ULP + (per_chunk + chunks) * U)
                * sum_k |w_k z_k[j]|
  centered rank integer ranks equal, values within 2 * U
  step()        step_fp64's per-element tolerance of each field
"""

import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import update_oracle_cases as C  # noqa: E402
from fiber_amd.es import update_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

U, ULP, Z_SIDE_ULPS = oracle.U, oracle.ULP, oracle.Z_SIDE_ULPS


def _dev():
    return torch.device("cuda", 0)


def _f64(t):
    return t.detach().cpu().double().numpy()


def _one_hot_draws(ops, seed, iteration, pair, nparams):
    """The device's draws of one pair: es_grad with the weight 1.0 on it
    (0 + 1*z is z) inside a range of 4 pairs; every other entry of the
    weight vector is 0 inside the range and NaN outside."""
    begin, end = C.hot_range(pair)
    w = np.full(end + 3, np.nan, dtype=np.float32)
    w[begin:end] = 0.0
    w[pair] = 1.0
    return ops.es_grad(torch.from_numpy(w).to(_dev()), begin, end, seed,
                       iteration, _dev(), nparams=nparams)


# ---- device draws ---------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("nparams", (C.NP_CONV, C.NP_MLP))
@pytest.mark.parametrize("seed,iteration,pair", C.TRIPLES)
def test_device_draws_within_z_side_ulps(seed, iteration, pair, nparams):
    from fiber_amd import ops

    got = _one_hot_draws(ops, seed, iteration, pair, nparams)
    assert got.numel() == nparams
    # the counter holds the block index only: a shorter vector is a prefix
    want = C.draws(seed, iteration, pair)[:nparams]
    err = oracle.rel_err(_f64(got), want)
    worst = int(np.argmax(err))
    print("device draws", (seed, iteration, pair), "nparams", nparams,
          "max relative error / ULP = %.4f at j = %d (z = %.9g)"
          % (err[worst] / ULP, worst, want[worst]))
    assert err.max() <= Z_SIDE_ULPS * ULP


# ---- es_grad ----------------------------------------------------------------------

def _grad(ops, begin, end, nparams):
    w = torch.from_numpy(C.weights(begin, end).copy()).to(_dev())
    return ops.es_grad(w, begin, end, C.GRAD_SEED, C.GRAD_ITER, _dev(),
                       nparams=nparams)


@requires_gpu
def test_grad_chunks_matches_the_binding():
    from fiber_amd import ops

    o = ops._require_ops()
    for nparams in (C.NP_MLP, C.NP_CONV, 4 * 256 * 31, 4 * 256 * 31 + 1):
        for pairs in (1, 4, 63, 64, 65, 66, 70, 1024):
            assert o.es_grad_chunks(pairs, nparams) == oracle.grad_chunks(
                pairs, nparams), (pairs, nparams)


@requires_gpu
@pytest.mark.parametrize("begin,end", C.MLP_RANGES)
def test_es_grad_chunking_edges(begin, end):
    from fiber_amd import ops

    g, _abs, tol, _j = C.grad_reference(begin, end, C.NP_MLP)
    # The partial buffer is torch.empty: chunks with no pair must write
    # their zeros themselves.  Free NaN-filled blocks of the two sizes that
    # es_grad allocates, so the caching allocator most likely hands those
    # out (it may not: this sharpens the check, it is not the check).
    chunks = oracle.grad_chunks(end - begin, C.NP_MLP)
    poison = [torch.full((k * C.NP_MLP,), float("nan"), device=_dev())
              for k in (1, chunks)]
    torch.cuda.synchronize()
    del poison
    got = _f64(_grad(ops, begin, end, C.NP_MLP))
    assert got.shape == (C.NP_MLP,)
    assert np.isfinite(got).all(), "a weight outside the range was read"
    ratio = np.abs(got - g) / tol
    print("es_grad pairs [%d, %d) chunks %d: max err/tol = %.4f"
          % (begin, end, oracle.grad_chunks(end - begin, C.NP_MLP),
             ratio.max()))
    assert ratio.max() <= 1.0


@requires_gpu
def test_es_grad_shards_sum_to_the_whole_range():
    from fiber_amd import ops

    whole, _abs, _tol, _j = C.grad_reference(*C.WHOLE, C.NP_MLP)
    total = np.zeros(C.NP_MLP)
    tol = np.zeros(C.NP_MLP)
    w = torch.from_numpy(C.weights(*C.WHOLE).copy()).to(_dev())
    for begin, end in C.SHARDS:
        # the shards read the whole range's weight vector, as the ranks do
        total += _f64(ops.es_grad(w, begin, end, C.GRAD_SEED, C.GRAD_ITER,
                                  _dev()))
        _g, abs_sum = oracle.grad_fp64(C.weights(*C.WHOLE), begin, end,
                                       C.GRAD_SEED, C.GRAD_ITER, C.NP_MLP)
        pairs = end - begin
        tol += oracle.grad_tol(abs_sum, pairs,
                               oracle.grad_chunks(pairs, C.NP_MLP))
    ratio = np.abs(total - whole) / tol
    print("es_grad shards %s: max err/tol = %.4f" % (C.SHARDS, ratio.max()))
    assert ratio.max() <= 1.0


@requires_gpu
@pytest.mark.parametrize("begin,end", C.CONV_RANGES)
def test_es_grad_at_the_conv_parameter_count(begin, end):
    from fiber_amd import ops

    g, _abs, tol, idx = C.grad_reference(begin, end, C.NP_CONV)
    out = _grad(ops, begin, end, C.NP_CONV)
    assert out.numel() == C.NP_CONV
    got = _f64(out)
    assert np.isfinite(got).all()
    ratio = np.abs(got[idx] - g) / tol
    print("es_grad NP_CONV pairs [%d, %d) chunks %d x %d: max err/tol = %.4f"
          % (begin, end, oracle.grad_chunks(end - begin, C.NP_CONV),
             oracle.grad_per_chunk(end - begin, C.NP_CONV), ratio.max()))
    assert ratio.max() <= 1.0
    assert idx[-1] == C.NP_CONV - 1 and ratio[-2:].max() <= 1.0  # the tail


# ---- es_perturb and es_grad see the same eps --------------------------------------

@requires_gpu
def test_perturb_and_grad_regenerate_the_same_bits():
    """At theta = 0 and sigma = 1 es_perturb stores bf16(0 + z) and
    bf16(0 - z).  Both kernels inline fam_normal4, so with z the bits that
    es_grad returns the equality is exact."""
    from fiber_amd import ops

    o = ops._require_ops()
    dev = _dev()
    seed, iteration, first_pair = 4321, 9, 3
    pop = 4
    theta = torch.zeros(C.NP_CONV, device=dev)
    wpert = torch.full((pop, o.NP_CONV_PAD), 7.0, dtype=torch.bfloat16,
                       device=dev)
    iterp = torch.full((1,), iteration, dtype=torch.int32, device=dev)
    o.es_perturb(theta.data_ptr(), C.NP_CONV, o.NP_CONV_PAD, 1.0, seed,
                 iterp.data_ptr(), 2 * first_pair, pop, wpert.data_ptr(), 0,
                 0, torch.cuda.current_stream().cuda_stream)
    zero = torch.zeros(C.NP_CONV, device=dev)
    for k in range(pop // 2):
        z = _one_hot_draws(ops, seed, iteration, first_pair + k, C.NP_CONV)
        for member, want in ((2 * k, zero + z), (2 * k + 1, zero - z)):
            want = want.to(torch.bfloat16).view(torch.int16)
            got = wpert[member, :C.NP_CONV].view(torch.int16)
            differ = int((got != want).sum())
            assert differ == 0, (
                "member %d: %d of %d bf16 values differ from es_grad's eps"
                % (member, differ, C.NP_CONV))
        # the padding past NP_CONV is not written
        assert (wpert[2 * k:2 * k + 2, C.NP_CONV:] == 7.0).all()


# ---- centered_rank ----------------------------------------------------------------

def _assert_ranks(got, f, what):
    n = f.size
    got = _f64(got)
    want = oracle.centered_rank_exact(f)
    assert np.array_equal(oracle.ranks_from_centered(got, n),
                          oracle.ranks_exact(f)), what
    err = np.abs(got - want).max()
    assert err <= oracle.RANK_TOL, (what, err)
    return err / oracle.RANK_TOL


@requires_gpu
@pytest.mark.parametrize("n", C.RANK_SIZES)
def test_centered_rank_exact_ranks(n):
    from fiber_amd import ops

    o = ops._require_ops()
    worst = 0.0
    for f in (C.rank_input(n), C.rank_equal_input(n)):
        t = torch.from_numpy(f.copy()).to(_dev())
        worst = max(worst, _assert_ranks(ops.centered_rank(t), f, n))
        if n > 16384:
            # the O(n^2) kernel on the input that took the sort path
            raw = torch.empty_like(t)
            o.centered_rank(t.data_ptr(), n, raw.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
            worst = max(worst, _assert_ranks(raw, f, (n, "O(n^2)")))
    print("centered_rank n = %d: max err/tol = %.3f" % (n, worst))


@requires_gpu
def test_centered_rank_pairs_rows():
    from fiber_amd import ops

    rows = [C.rank_input(257, salt) for salt in (0, 1)]
    rows.append(C.rank_equal_input(257))
    t = torch.from_numpy(np.stack(rows)).to(_dev())
    got = ops.centered_rank_pairs(t)
    assert got.shape == (3, 257)
    for p, f in enumerate(rows):
        _assert_ranks(got[p], f, p)
        assert torch.equal(got[p], ops.centered_rank(t[p].contiguous()))


@requires_gpu
def test_centered_rank_rejects_a_single_member():
    """n = 1 used to return NaN (0/0)."""
    from fiber_amd import ops

    for n in (0, 1):
        with pytest.raises(ValueError):
            ops.centered_rank(torch.zeros(n, device=_dev()))
        with pytest.raises(ValueError):
            ops.centered_rank_pairs(torch.zeros(3, n, device=_dev()))


# ---- a whole step, field by field ---------------------------------------------------

MLP_FIELDS = ("theta", "adam_m", "adam_v", "obs_sum", "obs_sumsq",
              "obs_count", "obs_mu", "obs_nu")
CONV_FIELDS = ("theta", "adam_m", "adam_v")


def _snapshot(eng, fields, row=None):
    snap = {}
    for name in fields:
        t = getattr(eng, name)
        snap[name] = (t if row is None else t[row]).detach().cpu().numpy(
        ).copy()
    snap["t_step"] = eng.t_step
    return snap


def _compare_step(label, new, tol, flags, after, fields, worst):
    if "obs_nu_clamp" in flags:
        assert not flags["obs_nu_clamp"].any(), label
    for name in fields:
        got = after[name].astype(np.float64).reshape(-1)
        t = tol[name]
        assert np.isfinite(got).all(), (label, name)
        diff = np.abs(got - new[name].reshape(-1))
        assert (diff <= t).all(), (
            label, name, int(np.argmax(diff - t)),
            float((diff - t).max()))
        ok = t > 0.0
        if ok.any():
            worst[name] = max(worst.get(name, 0.0),
                              float((diff[ok] / t[ok]).max()))
    assert after["t_step"] == new["t_step"], label


@requires_gpu
@pytest.mark.parametrize("pop", C.MLP_STEP_POPS)
def test_es_engine_step_against_step_fp64(pop):
    from fiber_amd import ops
    from fiber_amd.es.engine import ESConfig, ESEngine

    cfg = ESConfig(pop_per_gpu=pop, horizon=C.STEP_HORIZON)
    eng = ESEngine(cfg, ctx=None, device=_dev())
    worst, share = {}, 1.0
    for it in C.STEP_ITERATIONS:
        before = _snapshot(eng, MLP_FIELDS)
        fitness, obs_stat = ops.es_rollout_mlp(
            eng.theta, cfg.sigma, cfg.seed, it, cfg.horizon, 0, pop,
            eng.obs_mu, eng.obs_nu, eng.env_A, eng.env_B)
        new, tol, flags = oracle.step_fp64(
            before, fitness.cpu().numpy(), obs_stat.cpu().numpy(), cfg,
            cfg.seed, it, C.NP_MLP)
        eng.step(it)
        _compare_step(("ESEngine", pop, it), new, tol, flags,
                      _snapshot(eng, MLP_FIELDS), MLP_FIELDS, worst)
        share = min(share, float((tol["theta"] < 1e-3 * cfg.lr).mean()))
    assert eng.t_step == len(C.STEP_ITERATIONS)
    print("ESEngine pop %d: max err/tol per field %s; least share of theta "
          "held within 1e-3*lr: %.4f"
          % (pop, {k: round(v, 4) for k, v in worst.items()}, share))


@requires_gpu
def test_conv_engine_step_against_step_fp64():
    from fiber_amd.es.conv_policy import ConvESConfig, ConvESEngine

    cfg = ConvESConfig(pop_per_gpu=C.CONV_STEP_POP, horizon=C.STEP_HORIZON)
    eng = ConvESEngine(cfg, ctx=None, device=_dev())
    worst = {}
    for it in C.STEP_ITERATIONS:
        before = _snapshot(eng, CONV_FIELDS)
        fitness = eng.rollout(it).cpu().numpy().copy()
        new, tol, flags = oracle.step_fp64(before, fitness, None, cfg,
                                           cfg.seed, it, C.NP_CONV)
        eng.step(it)
        _compare_step(("ConvESEngine", it), new, tol, flags,
                      _snapshot(eng, CONV_FIELDS), CONV_FIELDS, worst)
    print("ConvESEngine pop %d: max err/tol per field %s"
          % (C.CONV_STEP_POP, {k: round(v, 4) for k, v in worst.items()}))


@requires_gpu
def test_es_population_step_against_step_fp64():
    from fiber_amd import ops
    from fiber_amd.es.engine import ESConfig, make_env_params
    from fiber_amd.es.population import ESPopulation

    cfg = ESConfig(pop_per_gpu=C.POPULATION_POP, horizon=C.STEP_HORIZON)
    seeds = C.POPULATION_SEEDS
    envs = [make_env_params(s, "cpu") for s in seeds]
    pop = ESPopulation(cfg, seeds, envs, device=_dev())
    worst = {}
    for it in C.STEP_ITERATIONS:
        before = [_snapshot(pop, MLP_FIELDS, p) for p in range(len(seeds))]
        fitness, obs_stat = ops.es_rollout_mlp_pairs(
            pop.theta, cfg.sigma, pop._seeds_dev, it, cfg.horizon,
            cfg.pop_per_gpu, pop.obs_mu, pop.obs_nu, pop.env_A, pop.env_B)
        fitness, obs_stat = fitness.cpu().numpy(), obs_stat.cpu().numpy()
        pop.step(it)
        for p, seed in enumerate(seeds):
            new, tol, flags = oracle.step_fp64(
                before[p], fitness[p], obs_stat[p],
                dataclasses.replace(cfg, seed=seed), seed, it, C.NP_MLP)
            _compare_step(("ESPopulation", p, it), new, tol, flags,
                          _snapshot(pop, MLP_FIELDS, p), MLP_FIELDS, worst)
    print("ESPopulation P = %d: max err/tol per field %s"
          % (len(seeds), {k: round(v, 4) for k, v in worst.items()}))


@requires_gpu
def test_es_engine_step_takes_the_variance_floor():
    """One real step() on which the 1e-2 variance floor is the value taken
    (dims 0 and 1; the state is update_oracle_cases.floor_obs_state, chosen
    on the CPU), every field as above and obs_nu on the floor bit for bit.
    Then the +-5 clamp of the normalised obs under that engine's own
    normaliser: one more rollout pair of its theta, held one step at a
    time as in test_rollout_step_gpu.py."""
    import rollout_step_cases as S
    from fiber_amd import ops
    from fiber_amd.es import rollout_oracle
    from fiber_amd.es.engine import ESConfig, ESEngine

    cfg = ESConfig(pop_per_gpu=C.FLOOR_POP, horizon=C.STEP_HORIZON)
    assert cfg.seed == C.FLOOR_SEED
    eng = ESEngine(cfg, ctx=None, device=_dev())
    state = eng.state_dict()
    state.update({k: torch.from_numpy(v)
                  for k, v in C.floor_obs_state().items()})
    eng.load_state_dict(state)
    floor_bits = np.float32(1e-2).view(np.uint32)
    it = C.STEP_ITERATIONS[0]
    before = _snapshot(eng, MLP_FIELDS)
    fitness, obs_stat = ops.es_rollout_mlp(
        eng.theta, cfg.sigma, cfg.seed, it, cfg.horizon, 0, C.FLOOR_POP,
        eng.obs_mu, eng.obs_nu, eng.env_A, eng.env_B)
    new, tol, flags = oracle.step_fp64(
        before, fitness.cpu().numpy(), obs_stat.cpu().numpy(), cfg, cfg.seed,
        it, C.NP_MLP)
    eng.step(it)
    after = _snapshot(eng, MLP_FIELDS)
    # the reference variance is off the floor by more than its tolerance,
    # below it in dims 0 and 1, above it in dims 2 and 3
    assert not flags["obs_nu_clamp"].any()
    assert (new["obs_nu"][:2] == oracle.C1EM2).all()
    assert (tol["obs_nu"][:2] == 0.0).all()
    assert (new["obs_nu"][2:] > oracle.C1EM2).all()
    assert (after["obs_nu"][:2].view(np.uint32) == floor_bits).all(), (
        after["obs_nu"])
    worst = {}
    _compare_step(("ESEngine floor", it), new, tol, flags, after, MLP_FIELDS,
                  worst)
    print("ESEngine on the variance floor: obs_nu %s, max err/tol per field "
          "%s" % (after["obs_nu"], {k: round(v, 4) for k, v in worst.items()}))

    # the clamp, reached through the engine's normaliser
    h = S.CLAMP_STEP_H
    inp = [t.unsqueeze(0).contiguous() for t in (
        eng.theta, eng.obs_mu, eng.obs_nu, eng.env_A, eng.env_B)]
    runs = {}
    for hor in (h, h + 1):
        _scores, _bc, final, ep = ops.es_eval_bc(
            *inp, cfg.seed, it + 1, hor, return_final_states=True,
            return_episodes=True)
        runs[hor] = (final[0, 0].cpu().numpy(), ep[0, 0].cpu().numpy())
    args = (rollout_oracle.make_policy(after["theta"]), after["obs_mu"],
            after["obs_nu"], eng.env_A.cpu().numpy(),
            eng.env_B.cpu().numpy())
    st = S.one_step(args, runs[h][0])
    sm = S.match_states(st, runs[h + 1][0])
    s_max = max(float(np.abs(f).max()) for f, _e in runs.values())
    err, rtol = S.match_reward(st, sm, runs[h][1], runs[h + 1][1], h, s_max)
    hi, lo, mixed, hi_share, lo_share = S.clamp_condition(st.x_raw)
    print("one step from h=%d: decided %.3f, state max err/tol %.3f, reward "
          "max err/tol %.3f, x above +5 per dim %s, below -5 %s"
          % (h, st.decided.mean(), sm.ratio.max(), (err / rtol).max(),
             np.round(hi_share, 3), np.round(lo_share, 3)))
    assert st.decided.mean() >= S.CAP
    assert sm.ok.all(), np.flatnonzero(~sm.ok).tolist()
    assert (err <= rtol).all(), np.flatnonzero(err > rtol).tolist()
    # the clamp was reached in the floored dims, and lanes of the same
    # operand stayed inside it
    assert (np.abs(st.x_raw[:, :2]) > 5.0).any()
    assert mixed
