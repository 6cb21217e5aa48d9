"""fiber_amd.es.lstm_oracle on the CPU: its convention against
torch.nn.LSTMCell, and the condition on the inputs of
tests/gpu/test_lstm_gpu.py under which that test may accept either action."""

import numpy as np
import pytest
import torch

from fiber_amd.es import init_theta_lstm, philox_ref
from fiber_amd.es import lstm_oracle as L
from fiber_amd.es.engine import make_env_params

# the world of tests/gpu/test_lstm_gpu.py
SEED, ITER, OFFSET, POP = 4321, 3, 2, 6
MU = np.array([0.05, -0.1, 0.02, 0.0], np.float32)
NU = np.array([0.3, 0.5, 0.2, 0.4], np.float32)


def test_cell_equals_torch_lstmcell_without_roundings():
    theta = init_theta_lstm(5, "cpu")
    gen = torch.Generator().manual_seed(1)
    theta[17408:17664] = torch.randn(256, generator=gen) * 0.3   # biases
    theta[17792:] = torch.tensor([0.2, -0.1])
    x = torch.randn(9, 4, generator=gen, dtype=torch.float64)
    h = torch.rand(9, 64, generator=gen, dtype=torch.float64) * 2 - 1
    c = torch.randn(9, 64, generator=gen, dtype=torch.float64) * 1.5
    ref = torch.nn.LSTMCell(4, 64, dtype=torch.float64)
    th = theta.double()
    with torch.no_grad():
        ref.weight_ih.copy_(th[:1024].reshape(256, 4))
        ref.weight_hh.copy_(th[1024:17408].reshape(256, 64))
        ref.bias_ih.copy_(th[17408:17664])
        ref.bias_hh.zero_()
        want_h, want_c = ref(x, (h, c))
        want_l = want_h @ th[17664:17792].reshape(2, 64).T + th[17792:]
    got_h, got_c, got_l = L.cell(L.make_policy(theta.numpy(), bf16=False),
                                 x.numpy(), h.numpy(), c.numpy())[:3]
    for got, want in ((got_h, want_h), (got_c, want_c), (got_l, want_l)):
        assert np.abs(got - want.numpy()).max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("sigma,mask", [(0.0, 0b1111), (0.05, 0b1111),
                                        (0.05, 0b0011)])
def test_gpu_inputs_leave_few_actions_undecided(sigma, mask):
    theta = init_theta_lstm(SEED, "cpu").numpy()
    env_A, env_B = [t.numpy() for t in make_env_params(SEED, "cpu")]
    worst = 0
    for member in (OFFSET, OFFSET + 1, OFFSET + POP - 1):
        z = philox_ref.noise_for_pair(SEED, ITER, member // 2, L.LSTM_NPARAMS)
        pol = L.make_policy(theta, -sigma if member % 2 else sigma, z)
        s = philox_ref.env_init_state(SEED, ITER, 64)
        h = c = np.zeros((64, 64), np.float32)
        for _step in range(8):
            x, x_slack = L.observe(s, MU, NU, mask)
            hn, cn, logits, _th, _tc, tol_l = L.cell(pol, x, h, c, x_slack)
            close = np.abs(logits[:, 1] - logits[:, 0]) <= tol_l.sum(-1)
            worst = max(worst, int(close.sum()))
            s = L.env_step(s, logits[:, 1] > logits[:, 0], env_A,
                           env_B)[0].astype(np.float32)
            h, c = hn.astype(np.float32), cn.astype(np.float32)
    print("undecided envs per member and step, at most: %d of 64" % worst)
    assert worst <= 4
