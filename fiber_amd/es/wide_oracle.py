"""Float64 oracle of the wide MLP policy kernels (CPU only).

A plain reading of ``wide_load`` / ``wide_layer1`` / ``wide_layer2`` /
``wide_logit`` and of the env phase of ``wide_rollout`` in
fiber_amd/csrc/ops/wide_kernels.hip, for H = 128 and 256.  Everything is
float64 except the roundings the kernel makes to bf16, which are
reproduced exactly: W1, W2 and W3 when the policy is drawn, and ``h1``.
``h2`` stays unrounded, biases stay as given, and ``x`` is taken as the
caller gives it (bf16-valued; ``observe`` makes it from a state).

There is no bookkeeping across steps: every rollout check restarts from
the kernel's own fp32 state, so one ``forward`` and one ``env_step`` are
all a test needs.  ``forward`` returns a tolerance per logit, built term by
term from the magnitudes of that very step with the constants derived in
``rollout_oracle`` (profiles/wide_mlp.md); nothing here comes from a GPU
run.

The env phase is the 64-wide kernel's, expression for expression, and the
GRU kernel restates the same one: ``observe`` and ``env_step`` are
``gru_oracle``'s.
"""

import collections

import numpy as np

from .gru_oracle import env_step, observe  # noqa: F401
from .rollout_oracle import (  # noqa: F401  (C01, X_REL: for the tests)
    C01, EPS_TANH, SAFETY, U, X_REL, Z_REL, bf16_round, tanh_slope)

OBS, ACT = 4, 2
HIDDEN = (128, 256)

# |bf16(v) - v| <= UB |v|: 8 significant bits, so the spacing in the binade
# of v is at most 2^-7 |v| and the rounding moves v by at most half of it
UB = 2.0 ** -8


def offsets(hidden):
    """(B1, W2, B2, W3, B3, nparams) of the flat theta: ``W1[H][4], b1[H],
    W2[H][H], b2[H], W3[2][H], b3[2]``."""
    H = int(hidden)
    assert H in HIDDEN
    b1 = OBS * H
    w2 = b1 + H
    b2 = w2 + H * H
    w3 = b2 + H
    b3 = w3 + ACT * H
    return b1, w2, b2, w3, b3, b3 + ACT


def wide_nparams(hidden):
    return offsets(hidden)[5]


def accumulation_lengths(hidden):
    """fp32 terms that meet in one sum.  Layer 1: 4 products and the bias
    the accumulator starts from.  Layer 2: H products and the bias.  Logits:
    H fmas split over the lanes, the 2-level lane reduce, the 8 wave
    partials and b3 (H + 2, as N_LOGIT counts the 64-wide kernel), plus the
    depth of the reduce."""
    H = int(hidden)
    return OBS + 1, H + 1, H + 2 + 2


Policy = collections.namedtuple("Policy", [
    "hidden", "w1", "b1", "w2", "b2", "w3", "b3",   # [H][4] [H] [H][H] ...
    "w1_slack", "w2_slack", "w3_slack",   # bf16 spacing where flagged, else 0
    "b1_err", "b2_err", "b3_err"])        # fp32 uncertainty of the biases


def make_policy(theta, hidden, sgn_sigma=0.0, z=None, bf16=True):
    """The policy as the kernel draws it.  ``theta`` float32
    [wide_nparams(hidden)]; for a perturbed member ``z`` is the pair's
    float32 noise and ``sgn_sigma`` is +-sigma.  The kernel forms
    ``fmaf(sgn_sigma, z, theta)`` from its own z, so the exact float64 value
    here is known only to within ``|sgn z| * (Z_REL + U) + U*|w|``
    (rollout_oracle's rule): a weight closer than that to a bf16 midpoint is
    flagged and may round the other way.  ``bf16=False`` leaves the weights
    unrounded (the plain reference of the CPU test)."""
    H = int(hidden)
    o_b1, o_w2, o_b2, o_w3, o_b3, n = offsets(H)
    th = np.asarray(theta, dtype=np.float32).astype(np.float64)
    assert th.shape == (n,)
    if z is None:
        w, width = th, np.zeros_like(th)
    else:
        sz = float(np.float32(sgn_sigma)) * np.asarray(
            z, dtype=np.float32).astype(np.float64)
        w = th + sz
        width = np.abs(sz) * (Z_REL + U) + U * np.abs(w)

    def weights(lo, hi, shape):
        if not bf16:
            return w[lo:hi].reshape(shape), np.zeros(shape)
        r, dist, q = bf16_round(w[lo:hi])
        return r.reshape(shape), ((dist < width[lo:hi]) * q).reshape(shape)

    w1, w1_s = weights(0, o_b1, (H, OBS))
    w2, w2_s = weights(o_w2, o_b2, (H, H))
    w3, w3_s = weights(o_w3, o_b3, (ACT, H))
    return Policy(H, w1, w[o_b1:o_w2], w2, w[o_b2:o_w3], w3, w[o_b3:],
                  w1_s, w2_s, w3_s,
                  width[o_b1:o_w2], width[o_b2:o_w3], width[o_b3:])


def forward(pol, x, x_slack=None):
    """``(logits [E][2], tol_logits [E][2])`` for ``x`` [E][4].

    ``x_slack`` [E][4] is what the kernel's x may differ by (the bf16
    spacing where its rounding is ambiguous, from ``observe``).  The
    tolerance bounds |kernel's fp32 logits - these|."""
    n1, n2, n3 = accumulation_lengths(pol.hidden)
    x = np.asarray(x, dtype=np.float64)
    xs = np.zeros_like(x) if x_slack is None else np.asarray(x_slack)
    # ---- layer 1: accumulator starts from b1, 4 products (MFMA) ----------
    pre1 = x @ pol.w1.T + pol.b1
    mag1 = np.abs(x) @ np.abs(pol.w1).T + np.abs(pol.b1)
    e1 = (pol.b1_err + np.abs(x) @ pol.w1_slack.T + xs @ np.abs(pol.w1).T
          + SAFETY * (n1 - 1) * U * mag1)
    h1_raw = np.tanh(pre1)
    e_h1 = EPS_TANH + tanh_slope(pre1, e1) * e1
    # a value within its fp32 error of a rounding midpoint may land on the
    # other neighbour in the kernel: off by one spacing
    h1, dist, q = bf16_round(h1_raw)
    h1_slack = (dist < e_h1) * q
    # ---- layer 2: accumulator starts from b2, H products (MFMA) ----------
    pre2 = h1 @ pol.w2.T + pol.b2
    mag2 = np.abs(h1) @ np.abs(pol.w2).T + np.abs(pol.b2)
    e2 = (pol.b2_err + np.abs(h1) @ pol.w2_slack.T
          + h1_slack @ np.abs(pol.w2).T + SAFETY * (n2 - 1) * U * mag2)
    h2 = np.tanh(pre2)
    e_h2 = EPS_TANH + tanh_slope(pre2, e2) * e2
    # ---- logits: fp32 fmas on the fp32 h2, reduce, wave partials, b3 -----
    t = h2[:, None, :] * pol.w3[None, :, :]                  # [E][2][H]
    logits = t.sum(-1) + pol.b3
    tol = (e_h2 @ np.abs(pol.w3).T + np.abs(h2) @ pol.w3_slack.T
           + n3 * U * (np.abs(t).sum(-1) + np.abs(pol.b3)) + pol.b3_err)
    return logits, tol


def bf16_bound(plain, x):
    """Bound on |forward(policy) - the same MLP without any bf16 rounding|
    for bf16-valued ``x``, from the unrounded policy (``make_policy(...,
    bf16=False)``) and its own activations: each of the three weight
    roundings and the rounding of h1 moves its value by at most UB of it.
    tanh' is bounded over the interval the pre-activation can move in, and
    the 1.01 covers the products of two such terms (UB^2 against UB)."""
    x = np.asarray(x, dtype=np.float64)
    w1, w2, w3 = np.abs(plain.w1), np.abs(plain.w2), np.abs(plain.w3)
    pre1 = x @ plain.w1.T + plain.b1
    d_pre1 = UB * (np.abs(x) @ w1.T)
    h1 = np.tanh(pre1)
    d_h1 = tanh_slope(pre1, d_pre1) * d_pre1 + UB * np.abs(h1)
    pre2 = h1 @ plain.w2.T + plain.b2
    d_pre2 = 1.01 * (d_h1 @ w2.T + UB * (np.abs(h1) @ w2.T))
    h2 = np.tanh(pre2)
    d_h2 = tanh_slope(pre2, d_pre2) * d_pre2
    return 1.01 * (d_h2 @ w3.T + UB * (np.abs(h2) @ w3.T))


def close_fraction(pol, obs_mu, obs_nu, env_A, env_B, s0, steps):
    """Chain ``observe -> forward -> env_step`` for ``steps`` steps from
    ``s0`` [E][4] (the state rounded to fp32 between steps, as the kernel
    holds it) and return the share of envs that are *close* at the step
    after: ``|l1 - l0|`` within the summed logits tolerance, where the
    kernel may choose either action.  This only states a condition about
    test inputs on the CPU; no comparison with the kernel goes through it."""
    s = np.asarray(s0, dtype=np.float32)
    for _t in range(steps + 1):
        x, x_slack = observe(s, obs_mu, obs_nu)
        logits, tol = forward(pol, x, x_slack)
        close = np.abs(logits[:, 1] - logits[:, 0]) <= tol.sum(-1)
        s = env_step(s, logits[:, 1] > logits[:, 0], env_A,
                     env_B)[0].astype(np.float32)
    return float(close.mean())
