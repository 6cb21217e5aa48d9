"""Separable NES on the device: es_rollout_mlp_sigma and es_grad_sigma
(fiber_amd/csrc/ops/snes_kernels.hip) and SNESEngine (fiber_amd/es/snes.py)
against their scalar-sigma siblings, bit for bit where the two must agree,
and against the fp64 oracles (rollout_oracle, update_oracle, snes_oracle;
derivations in profiles/snes.md) where they do not.

Tolerances, with U = 2^-24 and ULP = 2^-23:

  fitness, obs_stat   rollout_oracle.fitness_of / obs_stats_tol, on launches
                      whose every episode the oracle calls decided
  g_sig[j]            (2 Z_SIDE_ULPS ULP + (1 + per_chunk + chunks) U)
                      * sum_k |wsum[k]| (z_k[j]^2 + 1)
  sigma after a step  sigma_step_fp64's per-element tolerance, off the
                      coordinates it flags as sitting on a clamp
  theta, Adam, obs    update_oracle.step_fp64's per-element tolerance
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import rollout_oracle_cases as RC  # noqa: E402
import snes_cases as C  # noqa: E402
from fiber_amd.es import rollout_oracle  # noqa: E402
from fiber_amd.es import snes_oracle as so  # noqa: E402
from fiber_amd.es import update_oracle as uo  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

ES_FIELDS = ("theta", "adam_m", "adam_v", "obs_sum", "obs_sumsq",
             "obs_count", "obs_mu", "obs_nu")


def _dev():
    return torch.device("cuda", 0)


def _f64(t):
    return t.detach().cpu().double().numpy()


def _to_dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(_dev()).contiguous()


def _device_member_args():
    return [_to_dev(a) for a in RC.member_args()]


# ---- 1. uniform sigma keeps the sibling's bits -----------------------------------

@requires_gpu
@pytest.mark.parametrize("s", C.UNIFORM_SIGMAS)
@pytest.mark.parametrize("horizon", C.UNIFORM_HORIZONS)
@pytest.mark.parametrize("offset", C.UNIFORM_OFFSETS)
def test_uniform_sigma_vector_gives_the_scalar_kernels_bits(offset, horizon,
                                                            s):
    from fiber_amd import ops

    theta, mu, nu, A, B = _device_member_args()
    sig = torch.full((ops.NPARAMS,), s, dtype=torch.float32, device=_dev())
    fit, stat = ops.es_rollout_mlp_sigma(
        theta, sig, C.UNIFORM_SEED, RC.ITER, horizon, offset, C.UNIFORM_POP,
        mu, nu, A, B)
    want_fit, want_stat = ops.es_rollout_mlp(
        theta, s, C.UNIFORM_SEED, RC.ITER, horizon, offset, C.UNIFORM_POP,
        mu, nu, A, B)
    assert fit.shape == (C.UNIFORM_POP,) and stat.shape == (9,)
    assert torch.isfinite(fit).all()
    assert torch.equal(fit, want_fit)
    assert torch.equal(stat, want_stat)
    # the members are not all alike: the launch says something
    assert fit.unique().numel() > 1


# ---- 2. non-uniform sigma against the fp64 rollout oracle --------------------------

@requires_gpu
@pytest.mark.parametrize("seed,offset,h", C.SIGMA_LAUNCHES)
def test_sigma_vector_members_against_the_rollout_oracle(seed, offset, h):
    """Every one of the POP * 64 episodes is decided through h steps (the
    oracle says so from its own numbers), so each member's fitness and the
    obs statistics are compared in full.  The oracle's policy is theta +-
    float32(sigma[j] z[j]) with sigma_vector(), whose five levels vary
    inside every layer: reading sigma at another j, or ignoring the vector,
    moves weights by multiples of their perturbation."""
    from fiber_amd import ops

    ros = C.sigma_launch(seed, offset)
    assert len(ros) == C.POP
    assert all(ro.decided[:, h - 1].all() for ro in ros)
    theta, mu, nu, A, B = _device_member_args()
    fit, stat = ops.es_rollout_mlp_sigma(
        theta, _to_dev(C.sigma_vector()), seed, RC.ITER, h, offset, C.POP,
        mu, nu, A, B)
    fit, stat = _f64(fit), _f64(stat)
    for i, ro in enumerate(ros):
        want, tol = rollout_oracle.fitness_of(ro, h)
        print("seed %d off %d h %d member %d: fitness err %.3e tol %.3e"
              % (seed, offset, h, offset + i, abs(fit[i] - want), tol))
        assert abs(fit[i] - want) <= tol, (i, fit[i], want, tol)
    st = rollout_oracle.obs_stats(ros, h)
    want = np.concatenate([st.sum, st.sumsq])
    tol = rollout_oracle.obs_stats_tol(st)
    print("   stats max err/tol %.3f" % (np.abs(stat[:8] - want) / tol).max())
    assert (np.abs(stat[:8] - want) <= tol).all(), (stat, want, tol)
    assert stat[8] == C.POP * 64 * h


# ---- 3. es_grad_sigma: the g_mu row -------------------------------------------------

def _grad_sigma(ops, begin, end, nparams, wbegin=None, wend=None):
    if wbegin is None:
        wbegin, wend = begin, end
    return ops.es_grad_sigma(
        _to_dev(C.wdiff_weights(wbegin, wend)),
        _to_dev(C.wsum_weights(wbegin, wend)), begin, end, C.GRAD_SEED,
        C.GRAD_ITER, _dev(), nparams=nparams)


@requires_gpu
@pytest.mark.parametrize("begin,end", C.MLP_RANGES)
def test_g_mu_row_carries_es_grads_bits(begin, end):
    from fiber_amd import ops

    g_mu, g_sig = _grad_sigma(ops, begin, end, C.NP_MLP)
    want = ops.es_grad(_to_dev(C.wdiff_weights(begin, end)), begin, end,
                       C.GRAD_SEED, C.GRAD_ITER, _dev())
    assert g_mu.shape == g_sig.shape == (C.NP_MLP,)
    assert torch.isfinite(g_mu).all()
    assert torch.equal(g_mu, want)


# ---- 4. es_grad_sigma: the g_sig row ------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("begin,end,nparams",
                         [r + (C.NP_MLP,) for r in C.MLP_RANGES]
                         + [C.CONV_RANGE + (C.NP_CONV,)])
def test_g_sig_row_against_the_fp64_oracle(begin, end, nparams):
    from fiber_amd import ops

    g, tol, idx = C.sigma_grad_reference(begin, end, nparams)
    chunks = uo.grad_chunks(end - begin, nparams)
    # chunks without a pair must write their own zeros: free NaN-filled
    # blocks of the partial buffer's size so the allocator likely hands
    # them out (it may not: this sharpens the check, it is not the check)
    poison = torch.full((chunks * 2 * nparams,), float("nan"), device=_dev())
    torch.cuda.synchronize()
    del poison
    g_mu, g_sig = _grad_sigma(ops, begin, end, nparams)
    assert g_sig.shape == (nparams,)
    got = _f64(g_sig)
    assert np.isfinite(got).all(), "a weight outside the range was read"
    assert np.isfinite(_f64(g_mu)).all()
    ratio = np.abs(got[idx] - g) / tol
    print("es_grad_sigma nparams %d pairs [%d, %d) chunks %d: g_sig max "
          "err/tol = %.4f" % (nparams, begin, end, chunks, ratio.max()))
    assert ratio.max() <= 1.0
    assert idx[-1] == nparams - 1                    # the ragged tail
    # two calls, the same bits, both rows
    again_mu, again_sig = _grad_sigma(ops, begin, end, nparams)
    assert torch.equal(again_mu, g_mu) and torch.equal(again_sig, g_sig)


@requires_gpu
def test_g_sig_shards_sum_to_the_whole_range():
    from fiber_amd import ops

    whole, _tol, _idx = C.sigma_grad_reference(*C.WHOLE, C.NP_MLP)
    total = np.zeros(C.NP_MLP)
    tol = np.zeros(C.NP_MLP)
    for begin, end in C.SHARDS:
        # the shards read the whole range's weight vectors, as ranks would
        _mu, g_sig = _grad_sigma(ops, begin, end, C.NP_MLP, *C.WHOLE)
        total += _f64(g_sig)
        _g, shard_tol, _idx = C.sigma_grad_reference(begin, end, C.NP_MLP,
                                                     *C.WHOLE)
        tol += shard_tol
    ratio = np.abs(total - whole) / tol
    print("es_grad_sigma shards %s: max err/tol = %.4f"
          % (C.SHARDS, ratio.max()))
    assert np.isfinite(total).all()
    assert ratio.max() <= 1.0


# ---- 5. engine with lr_sigma = 0 is ESEngine ---------------------------------------

@requires_gpu
@pytest.mark.parametrize("pop", C.STEP_POPS)
def test_engine_without_sigma_learning_is_es_engine_bit_for_bit(pop):
    from fiber_amd.es import ESConfig, ESEngine, SNESConfig, SNESEngine

    cfg = ESConfig(pop_per_gpu=pop, horizon=C.STEP_HORIZON)
    ref = ESEngine(cfg, ctx=None, device=_dev())
    eng = SNESEngine(cfg, SNESConfig(lr_sigma=0.0), device=_dev())
    for it in C.STEP_ITERATIONS:
        want = ref.step(it)
        got = eng.step(it)
        for name in ES_FIELDS:
            assert torch.equal(getattr(eng, name), getattr(ref, name)), (
                pop, it, name)
        assert eng.t_step == ref.t_step
        assert torch.equal(eng.sigma, torch.full_like(eng.sigma, cfg.sigma))
        for key, value in want.items():
            assert got[key] == value, (pop, it, key)
        assert got["sigma_mean"] == got["sigma_min"] == got["sigma_max"]
    assert float(ref.theta.abs().sum()) > 0 and ref.t_step == 3


# ---- 6. engine with lr_sigma = 0.5 against the oracles -----------------------------

def _snapshot(eng):
    snap = {name: getattr(eng, name).detach().cpu().numpy().copy()
            for name in ES_FIELDS + ("sigma",)}
    snap["t_step"] = eng.t_step
    return snap


def _oracle_step(eng, it):
    """(before, device fitness, step_fp64 triple, sigma_step_fp64 triple) of
    the step the engine is about to take: the rollout is the device's own,
    relaunched here with the engine's pre-step state."""
    from fiber_amd import ops

    cfg = eng.cfg
    before = _snapshot(eng)
    fitness, obs_stat = ops.es_rollout_mlp_sigma(
        eng.theta, eng.sigma, cfg.seed, it, cfg.horizon, 0, cfg.pop_per_gpu,
        eng.obs_mu, eng.obs_nu, eng.env_A, eng.env_B)
    fitness, obs_stat = fitness.cpu().numpy(), obs_stat.cpu().numpy()
    es = uo.step_fp64(before, fitness, obs_stat, cfg, cfg.seed, it, C.NP_MLP)
    sg = so.sigma_step_fp64(before["sigma"], fitness, cfg, eng.snes,
                            cfg.seed, it, C.NP_MLP)
    return before, es, sg


def _compare_sigma(label, after, sg):
    new, tol, flag = sg
    got = after["sigma"].astype(np.float64)
    assert np.isfinite(got).all(), label
    ok = ~flag
    diff = np.abs(got - new)
    assert (diff[ok] <= tol[ok]).all(), (
        label, int(np.argmax(np.where(ok, diff - tol, -np.inf))),
        float(np.where(ok, diff - tol, -np.inf).max()))
    loose = ok & (tol > 0)
    return (float((diff[loose] / tol[loose]).max()) if loose.any() else 0.0,
            int(flag.sum()))


@requires_gpu
def test_engine_sigma_and_theta_against_the_fp64_oracles():
    from fiber_amd.es import ESConfig, SNESConfig, SNESEngine

    cfg = ESConfig(pop_per_gpu=C.STEP_POP, horizon=C.STEP_HORIZON)
    eng = SNESEngine(cfg, SNESConfig(lr_sigma=C.STEP_LR_SIGMA),
                     device=_dev())
    worst = {}
    for it in C.STEP_ITERATIONS:
        before, (new, tol, flags), sg = _oracle_step(eng, it)
        stats = eng.step(it)
        after = _snapshot(eng)
        label = ("SNESEngine", it)
        assert not flags["obs_nu_clamp"].any(), label
        for name in ES_FIELDS:
            got = after[name].astype(np.float64).reshape(-1)
            assert np.isfinite(got).all(), (label, name)
            diff = np.abs(got - new[name].reshape(-1))
            assert (diff <= tol[name]).all(), (
                label, name, int(np.argmax(diff - tol[name])),
                float((diff - tol[name]).max()))
            ok = tol[name] > 0.0
            if ok.any():
                worst[name] = max(worst.get(name, 0.0),
                                  float((diff[ok] / tol[name][ok]).max()))
        assert after["t_step"] == new["t_step"]
        ratio, flagged = _compare_sigma(label, after, sg)
        worst["sigma"] = max(worst.get("sigma", 0.0), ratio)
        assert flagged == 0, "the default rails are far away"
        moved = int((after["sigma"] != before["sigma"]).sum())
        assert moved >= 1, label
        assert stats["sigma_min"] <= stats["sigma_mean"] <= stats["sigma_max"]
        assert stats["sigma_min"] == float(after["sigma"].min())
        assert stats["sigma_max"] == float(after["sigma"].max())
        print("SNESEngine it %d: %d of %d sigmas moved, range [%.6f, %.6f], "
              "sigma tol max %.3e" % (it, moved, C.NP_MLP,
                                      stats["sigma_min"],
                                      stats["sigma_max"], sg[1].max()))
    print("SNESEngine pop %d: max err/tol per field %s"
          % (C.STEP_POP, {k: round(v, 4) for k, v in worst.items()}))


@requires_gpu
def test_engine_keeps_sigma_inside_tight_rails():
    from fiber_amd.es import ESConfig, SNESConfig, SNESEngine

    cfg = ESConfig(pop_per_gpu=C.STEP_POP, horizon=C.STEP_HORIZON)
    snes = SNESConfig(lr_sigma=C.STEP_LR_SIGMA,
                      sigma_min=(1 - C.RAIL) * cfg.sigma,
                      sigma_max=(1 + C.RAIL) * cfg.sigma)
    eng = SNESEngine(cfg, snes, device=_dev())
    lo = float(np.float32(snes.sigma_min))
    hi = float(np.float32(snes.sigma_max))
    for it in C.STEP_ITERATIONS:
        _before, _es, sg = _oracle_step(eng, it)
        eng.step(it)
        after = _snapshot(eng)
        got = after["sigma"].astype(np.float64)
        assert (got >= lo).all() and (got <= hi).all(), it
        ratio, flagged = _compare_sigma(("rails", it), after, sg)
        print("rails it %d: %d at sigma_min, %d at sigma_max, %d flagged, "
              "max err/tol off the rails %.4f"
              % (it, int((got == lo).sum()), int((got == hi).sum()),
                 flagged, ratio))


# ---- 7. validation --------------------------------------------------------------------

@requires_gpu
def test_rollout_sigma_validates_before_launching():
    from fiber_amd import ops

    dev = _dev()
    theta, mu, nu, A, B = _device_member_args()
    sig = torch.full((ops.NPARAMS,), 0.05, device=dev)

    def call(theta=theta, sig=sig, horizon=4, offset=0, pop=2, mu=mu, nu=nu,
             A=A, B=B):
        return ops.es_rollout_mlp_sigma(theta, sig, 1, 0, horizon, offset,
                                        pop, mu, nu, A, B)

    call()                                            # the arguments are good
    strided = torch.full((2 * ops.NPARAMS,), 0.05, device=dev)[::2]
    assert strided.shape == sig.shape and not strided.is_contiguous()
    for bad in (dict(sig=sig.double()), dict(sig=sig.cpu()),
                dict(sig=strided), dict(sig=0.05), dict(theta=theta.half()),
                dict(theta=theta.cpu()), dict(mu=mu.cpu()),
                dict(A=A.t())):
        with pytest.raises(TypeError):
            call(**bad)
    for bad in (dict(sig=sig[:-1].contiguous()),
                dict(sig=torch.cat([sig, sig[:2]])),
                dict(sig=sig.view(2, -1)), dict(theta=theta[:-2].contiguous()),
                dict(mu=mu[:3].contiguous()), dict(A=A[:3].contiguous()),
                dict(horizon=0), dict(pop=0), dict(offset=-1),
                dict(offset=2 ** 31 - 2, pop=2)):
        with pytest.raises(ValueError):
            call(**bad)


@requires_gpu
def test_grad_sigma_validates_before_launching():
    from fiber_amd import ops

    dev = _dev()
    w = torch.zeros(10, device=dev)

    def call(wdiff=w, wsum=w, begin=0, end=8, device=dev, nparams=None):
        return ops.es_grad_sigma(wdiff, wsum, begin, end, 1, 0, device,
                                 nparams=nparams)

    g_mu, g_sig = call()
    assert g_mu.shape == g_sig.shape == (ops.NPARAMS,)
    assert not g_mu.any() and not g_sig.any()         # all weights are 0
    strided = torch.zeros(20, device=dev)[::2]
    for bad in (dict(wsum=w.double()), dict(wdiff=w.to(torch.int32)),
                dict(wsum=w.cpu()), dict(wdiff=w.cpu(), wsum=w.cpu()),
                dict(wsum=strided), dict(device=torch.device("cpu"))):
        with pytest.raises(TypeError):
            call(**bad)
    for bad in (dict(wsum=torch.zeros(9, device=dev)),    # mismatched
                dict(wdiff=torch.zeros(11, device=dev)),
                dict(end=11),                             # shorter than end
                dict(begin=-1), dict(begin=5, end=4), dict(nparams=0),
                dict(wdiff=w.view(2, 5), wsum=w.view(2, 5))):
        with pytest.raises(ValueError):
            call(**bad)
    # an empty range is no error: both rows are zero
    g_mu, g_sig = call(begin=3, end=3)
    assert not g_mu.any() and not g_sig.any()


@requires_gpu
def test_engine_refuses_a_ring_context():
    from fiber_amd.es import ESConfig, SNESEngine

    with pytest.raises(NotImplementedError, match="data-parallel"):
        SNESEngine(ESConfig(pop_per_gpu=8, horizon=2), ctx=object(),
                   device=_dev())


# ---- 8. checkpoint ----------------------------------------------------------------------

@requires_gpu
def test_checkpoint_resumes_bit_for_bit(tmp_path):
    from fiber_amd.es import ESConfig, SNESConfig, SNESEngine

    cfg = ESConfig(pop_per_gpu=C.STEP_POP, horizon=C.STEP_HORIZON)
    snes = SNESConfig(lr_sigma=C.STEP_LR_SIGMA, sigma_min=0.9 * cfg.sigma,
                      sigma_max=1.1 * cfg.sigma)
    run = SNESEngine(cfg, snes, device=_dev())
    run.step()
    run.step()
    path = str(tmp_path / "snes.pt")
    run.save(path)
    run.step()

    # a fresh engine with other SNES settings: load must bring the saved ones
    resumed = SNESEngine(cfg, SNESConfig(lr_sigma=0.01), device=_dev())
    resumed.load(path)
    assert resumed.snes == run.snes and resumed.t_step == 2
    state = torch.load(path, weights_only=False)
    assert state["sigma"].shape == (C.NP_MLP,)
    assert not torch.equal(state["sigma"],
                           torch.full((C.NP_MLP,), cfg.sigma))
    assert torch.equal(resumed.sigma.cpu(), state["sigma"])
    resumed.step()
    for name in ES_FIELDS + ("sigma",):
        assert torch.equal(getattr(resumed, name), getattr(run, name)), name
    assert resumed.t_step == run.t_step == 3

    # a plain ESEngine checkpoint is refused, not half loaded
    from fiber_amd.es import ESEngine

    plain = ESEngine(cfg, ctx=None, device=_dev()).state_dict()
    with pytest.raises(ValueError):
        resumed.load_state_dict(plain)
