"""fiber_amd.es.cartpole_oracle against the Gym equations, and the conditions
of the inputs that tests/gpu/test_cartpole_gpu.py runs (cartpole_cases.py)."""

import numpy as np
import pytest

import cartpole_cases as K
from fiber_amd.es import cartpole_oracle as C


def _gym_step(s, a, cart):
    g, mc, mp, l, F, tau = [float(c) for c in cart[:6]]
    x, xd, th, thd = s.T
    force = np.where(a, F, -F)
    temp = (force + mp * l * thd ** 2 * np.sin(th)) / (mc + mp)
    th_acc = (g * np.sin(th) - np.cos(th) * temp) / (
        l * (4.0 / 3.0 - mp * np.cos(th) ** 2 / (mc + mp)))
    x_acc = temp - mp * l * th_acc * np.cos(th) / (mc + mp)
    return np.stack([x + tau * xd, xd + tau * x_acc, th + tau * thd,
                     thd + tau * th_acc], axis=-1)


@pytest.mark.parametrize("cart", list(K.CARTS))
def test_physics_is_gym_cartpole(cart):
    cart = K.CARTS[cart]
    assert cart is K.CARTS["default"] or (cart != K.CARTS["default"]).all()
    rng = np.random.default_rng(5)
    s = rng.uniform(-1.0, 1.0, (1000, 4)) * [cart[6], 3.0, cart[7], 3.0]
    a = rng.random(1000) < 0.5
    nxt, bound, done, _ = C.step(s, a, cart)
    want = _gym_step(s, a, cart)
    assert np.abs(nxt - want).max() <= 1e-9
    assert (done == ((np.abs(want[:, 0]) > cart[6])
                     | (np.abs(want[:, 2]) > cart[7]))).all()
    # a bound of a few fp32 roundings of the magnitudes involved
    assert (bound > 0).all() and bound.max() < 64 * C.U * 8.0


def test_gpu_inputs_cover_every_band_and_are_mostly_decided():
    bands = {(64, 64): 0, (49, 63): 0, (33, 48): 0, (17, 32): 0, (1, 16): 0,
             (0, 0): 0}
    for cart in K.CARTS:
        for sigma in K.SIGMAS:
            ros = K.members(sigma, cart, 200)
            for h in list(range(16)) + [40, 199]:
                undecided = sum(int((~ro.step_decided[:, h]).sum())
                                for ro in ros)
                assert undecided <= 0.05 * K.POP * 64, (cart, sigma, h)
                if h < 16:
                    for ro in ros:
                        n = int(ro.alive[:, h].sum())
                        bands[[b for b in bands if b[0] <= n <= b[1]][0]] += 1
            if cart == "small":
                assert any(ro.ended_by_x.any() for ro in ros)
                assert any(ro.ended_by_th.any() for ro in ros)
    assert all(bands.values()), bands
    # the statistics check sums whole launches: these are decided throughout
    for cart, it in K.STAT_ITERS.items():
        assert all(ro.decided[:, -1].all() and ro.lengths.sum() > 0
                   for ro in K.members(0.05, cart, K.STAT_H, it, 2))
