"""gru_oracle on the CPU: anchored on torch.nn.GRUCell, and sharp."""

import numpy as np
import pytest
import torch

from fiber_amd.es import gru_oracle as G


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(7)
    theta = (rng.standard_normal(G.GRU_NPARAMS) * 0.3).astype(np.float32)
    x = G.bf16_round(rng.standard_normal((16, 4)))[0]
    h = rng.uniform(-1.0, 1.0, (16, 64)).astype(np.float32)
    return theta, x, h


def test_cell_equals_torch_grucell_without_roundings(inputs):
    theta, x, h = inputs
    pol = G.make_policy(theta, bf16=False)
    hn = G.cell(pol, x, h, bf16=False)[0]
    ref = torch.nn.GRUCell(4, 64).double()
    zero = np.zeros(64)
    with torch.no_grad():
        ref.weight_ih.copy_(torch.from_numpy(pol.wi.reshape(192, 4)))
        ref.weight_hh.copy_(torch.from_numpy(pol.wh.reshape(192, 64)))
        ref.bias_ih.copy_(torch.from_numpy(np.concatenate(pol.b[:3])))
        ref.bias_hh.copy_(torch.from_numpy(
            np.concatenate([zero, zero, pol.b[3]])))
        want = ref(torch.from_numpy(x),
                   torch.from_numpy(h.astype(np.float64))).numpy()
    assert np.abs(hn - want).max() <= 1e-12


@pytest.mark.parametrize("slip", ["r_inside", "z_swapped", "h_rounded"])
def test_tolerance_catches_slip(inputs, slip):
    theta, x, h = inputs
    pol = G.make_policy(theta)
    hn, _l, tol_h, _tl = G.cell(pol, x, h)
    moved = np.abs(G.cell(pol, x, h, slip=slip)[0] - hn)
    assert (moved > tol_h).any(), (moved / tol_h).max()


def test_sigmoid_emulation_error_within_constant():
    assert G.measure_sigmoid_emulation_error() <= G.SIG_EMUL_ERR
