"""fiber_amd.es.wide_oracle on the CPU: the layout, the oracle against a plain
float64 MLP, and the close cap of the GPU step test from the oracle alone."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_cases as C  # noqa: E402
from fiber_amd import ops  # noqa: E402
from fiber_amd.es import init_theta_wide  # noqa: E402
from fiber_amd.es import wide_oracle as W  # noqa: E402


@pytest.mark.parametrize("hidden,n", [(128, 17410), (256, 67586)])
def test_layout(hidden, n):
    H = hidden
    assert ops.wide_nparams(H) == W.wide_nparams(H) == n == H * H + 8 * H + 2
    o = W.offsets(H)
    assert o == (4 * H, 5 * H, 5 * H + H * H, 6 * H + H * H, 8 * H + H * H, n)
    # what the kernel's fragments rely on: blocks start at multiples of 4,
    # W2 rows at multiples of 8
    assert all(v % 4 == 0 for v in o[:5]) and o[1] % 8 == 0 and H % 8 == 0
    theta = init_theta_wide(3, H, "cpu")
    assert tuple(theta.shape) == (n,)
    for lo, hi in ((o[0], o[1]), (o[2], o[3]), (o[4], n)):   # zero biases
        assert not theta[lo:hi].any()
    with pytest.raises(ValueError, match="es_rollout_mlp"):
        ops.wide_nparams(64)
    with pytest.raises(ValueError):
        ops.wide_nparams(192)


@pytest.mark.parametrize("hidden", C.HIDDEN)
@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_forward_matches_plain_mlp_to_the_bf16_bound(hidden, scale):
    H = hidden
    theta = (init_theta_wide(7, H, "cpu") * scale).numpy()
    # non-zero biases, so that a swapped bias block shows
    o = W.offsets(H)
    rng = np.random.default_rng(H)
    for lo, hi in ((o[0], o[1]), (o[2], o[3]), (o[4], o[5])):
        theta[lo:hi] = rng.normal(0.0, 0.1, hi - lo).astype(np.float32)
    x = torch.randn(96, 4, generator=torch.Generator().manual_seed(1))
    x = x.bfloat16().float().numpy().astype(np.float64)
    t = theta.astype(np.float64)
    h1 = np.tanh(x @ t[:o[0]].reshape(H, 4).T + t[o[0]:o[1]])
    h2 = np.tanh(h1 @ t[o[1]:o[2]].reshape(H, H).T + t[o[2]:o[3]])
    plain = h2 @ t[o[3]:o[4]].reshape(2, H).T + t[o[4]:]
    logits, tol = W.forward(W.make_policy(theta, H), x)
    bound = W.bf16_bound(W.make_policy(theta, H, bf16=False), x)
    ratio = float((np.abs(logits - plain) / bound).max())
    print("oracle vs plain H=%d x%g: %.3f of the bf16 bound (max %.3g); "
          "fp32 tol max %.3g" % (H, scale, ratio, bound.max(), tol.max()))
    assert ratio <= 1.0
    # the roundings are really there, and the fp32 tolerance is far finer
    assert np.abs(logits - plain).max() > 1e-5
    assert (tol < bound).all()


@pytest.mark.parametrize("hidden", C.HIDDEN)
@pytest.mark.parametrize("sigma", C.SIGMAS)
@pytest.mark.parametrize("h", C.HORIZONS)
def test_step_cases_stay_under_the_close_cap(hidden, sigma, h):
    theta, mu, nu, env_A, env_B = [
        t.numpy() for t in C.world(hidden, "cpu")]
    frac = np.mean([W.close_fraction(
        C.member_policy(theta, hidden, sigma, m), mu, nu, env_A, env_B,
        C.init_state(), h) for m in C.MEMBERS])
    print("close H=%d sigma=%g h=%d: %.4f" % (hidden, sigma, h, frac))
    assert frac <= C.CLOSE_CAP
