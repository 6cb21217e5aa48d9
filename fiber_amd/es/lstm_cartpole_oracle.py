"""One step of ``es_rollout_lstm_cartpole`` in float64 (CPU only, numpy).

Nothing new is modelled here: a step is ``lstm_oracle.observe``, then
``lstm_oracle.cell``, then ``cartpole_oracle.step``, each with its own
tolerance.  ``step`` composes them for one member's 64 environments from
the fp32 ``(state, hidden, cell)`` the kernel itself returned, which is how
every rollout check of this package works; ``undecided_share`` chains it to
state a condition about test inputs on the CPU.
"""

import collections

import numpy as np

from . import cartpole_oracle as C
from . import lstm_oracle as L
from . import philox_ref

Step = collections.namedtuple("Step", [
    "x_slack",                        # [E][4]  observe's rounding slack
    "h", "c", "tol_h", "tol_c",       # [E][64] new hidden and cell state
    "action", "action_decided",       # [E]     l1 > l0, and by a safe margin
    "state", "bound",                 # [E][4]  new env state and its bound
    "done", "done_decided"])          # [E]     past a threshold, safely so


def member_policy(theta, sigma, seed, iteration, member):
    """Member ``member`` (member_offset already added) as the kernel stages
    it: ``lstm_oracle.make_policy`` of the pair's noise."""
    z = philox_ref.noise_for_pair(seed, iteration, member // 2,
                                  L.LSTM_NPARAMS)
    return L.make_policy(theta, -float(sigma) if member % 2 else float(sigma),
                         z)


def step(pol, state, hidden, cell, obs_mu, obs_nu, obs_mask, cart):
    """One step of every row, alive or not: the caller selects."""
    x, slack = L.observe(state, obs_mu, obs_nu, obs_mask)
    hn, cn, logits, tol_h, tol_c, tol_l = L.cell(pol, x, hidden, cell, slack)
    action = logits[:, 1] > logits[:, 0]
    decided = np.abs(logits[:, 1] - logits[:, 0]) > tol_l.sum(-1)
    nxt, bound, done, done_ok = C.step(state, action, cart)
    return Step(slack, hn, cn, tol_h, tol_c, action, decided, nxt, bound,
                done, done_ok)


def undecided_share(pol, obs_mu, obs_nu, obs_mask, cart, s0, steps):
    """``(undecided, live)`` environment-steps of the chained episode from
    ``s0`` and zero hidden and cell state, everything rounded to fp32
    between steps as the kernel holds it.  Only a statement about inputs:
    no comparison with the kernel goes through a chain."""
    s = np.asarray(s0, dtype=np.float32)
    h = np.zeros((s.shape[0], L.HID), dtype=np.float32)
    c = np.zeros_like(h)
    alive = np.ones(s.shape[0], bool)
    undecided = live = 0
    for _t in range(steps):
        if not alive.any():
            break
        st = step(pol, s, h, c, obs_mu, obs_nu, obs_mask, cart)
        live += int(alive.sum())
        undecided += int((alive & ~(st.action_decided
                                    & st.done_decided)).sum())
        s = np.where(alive[:, None], st.state, s).astype(np.float32)
        h, c = st.h.astype(np.float32), st.c.astype(np.float32)
        alive = alive & ~st.done
    return undecided, live
