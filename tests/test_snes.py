"""Host tests of the separable-NES oracle (fiber_amd/es/snes_oracle.py), of
the shared cases of tests/snes_cases.py and of the validation that the new
ops wrappers and the engine do before any launch.  No GPU."""

import types

import numpy as np
import pytest
import torch

import snes_cases as C
from fiber_amd import ops
from fiber_amd.es import snes_oracle as so
from fiber_amd.es import update_oracle as uo


# ---- sigma_grad_fp64 ---------------------------------------------------------

def test_sigma_grad_matches_the_per_member_sum():
    """Over the pairs [6, 76): sum_k wsum[k] (z_k^2 - 1) against the sum
    over the members, sum_i r_i (z_{i//2}^2 - 1), taken member by member in
    Python floats.  Held to 1e-12 relative to sum_k |wsum[k]| (z_k^2 + 1),
    the magnitude of the terms: relative to the result itself a coordinate
    that cancels to nearly 0 would have no bound at all."""
    begin, end = C.WHOLE
    rng = np.random.default_rng(31)
    r = rng.random(2 * end) - 0.5                   # member weights
    wsum = np.full(end + 3, np.nan)
    wsum[:end] = r[0::2] + r[1::2]
    g, abs_sum = so.sigma_grad_fp64(wsum, begin, end, C.GRAD_SEED,
                                    C.GRAD_ITER, C.NP_MLP)
    assert g.shape == abs_sum.shape == (C.NP_MLP,)
    want = np.zeros(C.NP_MLP)
    for i in range(2 * begin, 2 * end):
        z = uo.noise_fp64(C.GRAD_SEED, C.GRAD_ITER, i // 2, C.NP_MLP)
        want += r[i] * (z ** 2 - 1.0)
    assert np.isfinite(g).all()                      # no NaN from outside
    assert (np.abs(g - want) <= 1e-12 * abs_sum).all()
    assert (abs_sum >= np.abs(g)).all() and (abs_sum > 0).all()
    # the statistic is not degenerate: it has both signs and real size
    assert (g > 0.1).any() and (g < -0.1).any()


def test_sigma_grad_blocks_are_a_slice_of_the_whole():
    begin, end = 3, 9
    w = C.wsum_weights(begin, end)
    full, full_abs = so.sigma_grad_fp64(w, begin, end, 7, 1, C.NP_MLP)
    jb = np.array([0, 5, 700, (C.NP_MLP + 3) // 4 - 1])   # the ragged tail
    idx = uo.param_index(C.NP_MLP, jb)
    assert idx.size == 4 * 3 + 2 and idx[-1] == C.NP_MLP - 1
    g, abs_sum = so.sigma_grad_fp64(w, begin, end, 7, 1, C.NP_MLP, jb)
    assert np.array_equal(g, full[idx])
    assert np.array_equal(abs_sum, full_abs[idx])
    # the spread of the weights' own error rides the same slice
    w_err = np.full(w.size, 1e-7)
    _g, _a, spread = so.sigma_grad_fp64(w, begin, end, 7, 1, C.NP_MLP, jb,
                                        w_err=w_err)
    _g, _a, spread_full = so.sigma_grad_fp64(w, begin, end, 7, 1, C.NP_MLP,
                                             w_err=w_err)
    assert np.array_equal(spread, spread_full[idx]) and (spread > 0).all()


def test_sigma_grad_tol_counts_the_roundings():
    abs_sum = np.array([1.0, 8.0])
    # 64 pairs in 32 chunks of 2: 2 accumulates, 32 reduce adds, 1 for q
    want = (2 * so.Z_SIDE_ULPS * so.ULP + (1 + 2 + 32) * so.U) * abs_sum
    assert np.array_equal(so.sigma_grad_tol(abs_sum, 64, 32), want)
    # one chunk of 63
    want = (2 * so.Z_SIDE_ULPS * so.ULP + (1 + 63 + 1) * so.U) * abs_sum
    assert np.array_equal(so.sigma_grad_tol(abs_sum, 63, 1), want)


def test_wsum_weights_cover_every_zero_combination():
    for begin, end in C.MLP_RANGES + (C.CONV_RANGE,):
        wd, ws = C.wdiff_weights(begin, end), C.wsum_weights(begin, end)
        assert wd.shape == ws.shape and wd.dtype == ws.dtype == np.float32
        assert np.isnan(ws[:begin]).all() and np.isnan(ws[end:]).all()
        assert np.isfinite(ws[begin:end]).all()
        if end - begin >= 8:
            assert wd[begin + 1] == 0 and ws[begin + 1] != 0
            assert wd[begin + 2] != 0 and ws[begin + 2] == 0
            assert np.signbit(ws[begin + 2])
            assert wd[begin + 4] == 0 and ws[begin + 4] == 0
            assert wd[end - 1] == 0 and ws[end - 1] == 0
        assert not np.array_equal(wd[begin:end], ws[begin:end])


# ---- sigma_step_fp64 ---------------------------------------------------------

def _step_inputs(nparams=24, pop=8):
    rng = np.random.default_rng(5)
    fitness = rng.standard_normal(pop).astype(np.float32)
    sigma = np.full(nparams, 0.05, dtype=np.float32)
    cfg = types.SimpleNamespace(pop_per_gpu=pop, sigma=0.05)
    return sigma, fitness, cfg


def test_sigma_step_respects_both_clamps_and_flags_them():
    nparams = 24
    sigma, fitness, cfg = _step_inputs(nparams)
    wide = types.SimpleNamespace(lr_sigma=4.0, sigma_min=1e-6, sigma_max=1e3)
    free, tol, flag = so.sigma_step_fp64(sigma, fitness, cfg, wide, 11, 2,
                                         nparams)
    assert not flag.any() and (tol > 0).all()
    assert (free > 0.05).any() and (free < 0.05).any()
    # the formula itself, from the oracle's own gradient
    r = uo.centered_rank_exact(fitness)
    g, _abs = so.sigma_grad_fp64(r[0::2] + r[1::2], 0, 4, 11, 2, nparams)
    np.testing.assert_allclose(
        free, 0.05 * np.exp(0.5 * 4.0 / 8 * g) * (
            float(np.float32(0.05)) / 0.05), rtol=1e-14)

    order = np.argsort(free)
    lo_at, hi_at = order[3], order[-4]       # rails ON two reference values
    rails = types.SimpleNamespace(lr_sigma=4.0,
                                  sigma_min=float(np.float32(free[lo_at])),
                                  sigma_max=float(np.float32(free[hi_at])))
    new, tol2, flag2 = so.sigma_step_fp64(sigma, fitness, cfg, rails, 11, 2,
                                          nparams)
    lo, hi = rails.sigma_min, rails.sigma_max
    assert (new >= lo).all() and (new <= hi).all()
    assert flag2[lo_at] and flag2[hi_at] and flag2.sum() == 2
    below, above = order[:3], order[-3:]
    assert (new[below] == lo).all() and (new[above] == hi).all()
    assert (tol2[below] == 0).all() and (tol2[above] == 0).all()
    inside = order[4:-4]
    assert np.array_equal(new[inside], free[inside])
    assert np.array_equal(tol2[inside], tol[inside])


def test_sigma_step_with_lr_zero_leaves_sigma():
    sigma, fitness, cfg = _step_inputs()
    snes = types.SimpleNamespace(lr_sigma=0.0, sigma_min=5e-5, sigma_max=0.5)
    new, tol, flag = so.sigma_step_fp64(sigma, fitness, cfg, snes, 11, 2, 24)
    assert np.array_equal(new, sigma.astype(np.float64))
    assert not flag.any()
    # exp(0) within ULP, one product
    assert (tol <= 0.05 * (so.ULP + 2 * so.U)).all()


def test_sigma_step_refuses_unresolved_config_and_wrong_population():
    sigma, fitness, cfg = _step_inputs()
    with pytest.raises(ValueError):
        so.sigma_step_fp64(sigma, fitness, cfg, types.SimpleNamespace(
            lr_sigma=None, sigma_min=0.0, sigma_max=1.0), 11, 2, 24)
    with pytest.raises(ValueError):
        so.sigma_step_fp64(sigma, fitness[:6], cfg, types.SimpleNamespace(
            lr_sigma=0.1, sigma_min=0.0, sigma_max=1.0), 11, 2, 24)


# ---- the non-uniform sigma launches ------------------------------------------

def test_sigma_vector_is_five_powers_of_two_in_every_layer():
    s = C.sigma_vector()
    assert s.shape == (C.NP_MLP,) and s.dtype == np.float32
    levels = {2.0 ** -e for e in range(2, 7)}
    for lo, hi in ((0, 256), (256, 320), (320, 4416), (4416, 4480),
                   (4480, 4608)):
        assert set(s[lo:hi].tolist()) == levels
    assert s[4608] != s[4609]                       # b3
    # neighbours differ, and so do the rows of W2
    assert (s[1:] != s[:-1]).mean() > 0.9
    w2 = s[320:4416].reshape(64, 64)
    assert not np.array_equal(w2[0], w2[1])


def test_sigma_launches_are_decided_from_the_oracle_alone():
    for seed, off, h in C.SIGMA_LAUNCHES:
        ros = C.sigma_launch(seed, off)
        assert len(ros) == C.POP
        assert all(ro.decided[:, h - 1].all() for ro in ros), (seed, off, h)
    # the vector matters: the same members at the uniform mean sigma take
    # other actions somewhere
    seed, off, h = C.SIGMA_LAUNCHES[0]
    import rollout_oracle_cases as RC
    from fiber_amd.es import rollout_oracle

    theta, mu, nu, A, B = RC.member_args()
    differ = 0
    for i, ro in enumerate(C.sigma_launch(seed, off)):
        uni = rollout_oracle.member_rollout(
            theta, float(C.sigma_vector().mean()), seed, RC.ITER, h, off + i,
            mu, nu, A, B)
        differ += int((uni.action != ro.action[:, :h]).sum())
    assert differ > 0


# ---- wrapper and engine validation: refused before any launch ----------------

def test_extension_exports_the_snes_kernels():
    o = ops._require_ops()
    assert hasattr(o, "es_rollout_mlp_sigma") and hasattr(o, "es_grad_sigma")


def test_rollout_sigma_refuses_host_and_wrong_dtype_tensors():
    theta = torch.zeros(ops.NPARAMS)
    sig = torch.full((ops.NPARAMS,), 0.05)
    mu, nu = torch.zeros(4), torch.ones(4)
    A, B = torch.zeros(4, 4), torch.zeros(4)
    with pytest.raises(TypeError):
        ops.es_rollout_mlp_sigma(theta, sig, 1, 0, 4, 0, 2, mu, nu, A, B)
    with pytest.raises(TypeError):
        ops.es_rollout_mlp_sigma(theta, sig.double(), 1, 0, 4, 0, 2, mu, nu,
                                 A, B)
    with pytest.raises(TypeError):
        ops.es_rollout_mlp_sigma(theta, 0.05, 1, 0, 4, 0, 2, mu, nu, A, B)


def test_grad_sigma_refuses_host_and_wrong_dtype_tensors():
    w = torch.zeros(8)
    with pytest.raises(TypeError):
        ops.es_grad_sigma(w, w, 0, 8, 1, 0, torch.device("cuda", 0))
    with pytest.raises(TypeError):
        ops.es_grad_sigma(w.double(), w, 0, 8, 1, 0, torch.device("cuda", 0))
    with pytest.raises(TypeError):
        ops.es_grad_sigma(w, w, 0, 8, 1, 0, torch.device("cpu"))


def test_engine_refuses_a_ring_context_and_bad_configs():
    from fiber_amd.es import ESConfig, SNESConfig, SNESEngine

    cfg = ESConfig(pop_per_gpu=8, horizon=4)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        SNESEngine(cfg, SNESConfig(), ctx=object())
    cpu = torch.device("cpu")
    for bad in (SNESConfig(lr_sigma=-0.1), SNESConfig(lr_sigma=float("nan")),
                SNESConfig(sigma_min=-1.0),
                SNESConfig(sigma_min=0.2, sigma_max=0.1),
                SNESConfig(sigma_max=float("inf"))):
        with pytest.raises(ValueError):
            SNESEngine(cfg, bad, device=cpu)
    with pytest.raises(ValueError):
        SNESEngine(ESConfig(pop_per_gpu=7), SNESConfig(), device=cpu)


def test_snes_config_resolves_every_field_and_keeps_given_ones():
    from fiber_amd.es import ESConfig, SNESConfig

    got = SNESConfig().resolved(ESConfig(sigma=0.2))
    assert got.lr_sigma > 0 and 0 < got.sigma_min < 0.2 < got.sigma_max
    kept = SNESConfig(lr_sigma=0.0, sigma_min=0.1, sigma_max=0.3).resolved(
        ESConfig(sigma=0.2))
    assert (kept.lr_sigma, kept.sigma_min, kept.sigma_max) == (0.0, 0.1, 0.3)
