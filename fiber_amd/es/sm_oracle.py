"""Float64 oracle of the safe-mutation step kernel (CPU only).

A reading of ``sm_steps`` in fiber_amd/csrc/ops/sm_kernels.hip, written from
the kernel source.  The forward half is ``forward_oracle.forward`` (the
kernel's forward is ``mlp_policy_forward``'s); the policy staging and the
bf16 rounding are ``rollout_oracle``'s.

Everything is float64 except the roundings the kernel makes to bf16, which
are reproduced exactly: the staged weights, the probe, ``h1``, ``h2`` and,
in the backward, ``d2 = bf16(w3[k] * (1 - h2^2))`` and ``d1 = bf16(P * (1 -
h1^2))``.  Nothing else is rounded there: ``1 - h^2`` and the two products
stay fp32 in the kernel and float64 here.

The tolerance is carried element by element through the kernel's arithmetic
(derivation: profiles/safe_mutation.md):

* ``h1`` / ``h2`` that ``forward`` flags may be one bf16 spacing off in the
  kernel (``h1_off``, ``h2_off``, the widths of ``forward``); that moves
  ``1 - h^2`` by ``2 |h| off + off^2``, and EPS_TANH reaches the backward
  only through those flags, because the backward reads the rounded values;
* every fp32 operation adds U of its result; an MFMA sum of 64 products adds
  ``SAFETY * 64 * U * sum|terms|``, a 64-term VALU sum ``64 * U *
  sum|terms|``;
* ``d2`` and ``d1`` are mirrored.  A value closer to a bf16 rounding
  midpoint than the error it carries by then is flagged, as ``forward``
  flags ``h1``: it may be a spacing (or, where the error exceeds a spacing,
  that many spacings) off, and the flagged amount is carried on through
  ``|W2|``, ``|h1|``, ``|x|``;
* ``sens = sqrt(m0^2 + m1^2)`` moves by at most the 2-norm of what the two
  means move by, plus 3 U for its own three roundings; ``steps`` by what
  ``sigma / max(sens, s_min)`` spans over that interval, plus U.

``round_sens`` / ``round_steps`` bound something else: what the two bf16
roundings of the backward themselves change, half a spacing each, against
the same backward without them.  That is the distance to ``autograd`` taken
at the rounded forward point (tests/test_safe_ga.py).  Nothing here comes
from a GPU run.
"""

import collections

import numpy as np

from . import forward_oracle as fo
from .rollout_oracle import (EPS_TANH, HID, N_L1, N_L2, NPARAMS, OBS, OFF_B1,
                             OFF_B2, OFF_B3, OFF_W2, OFF_W3, SAFETY, U,
                             bf16_round, make_policy, tanh_slope)

BATCH = 64
MODES = ("abs", "sum")
N_SUM = 64                    # terms of every backward sum
SENS_ROUNDINGS = 3.0          # m0 * m0, the fma, the square root
SENS_UNDERFLOW = 2.0 ** -62   # m^2 under 2^-126 is lost: sqrt of that

ROUNDINGS = ("all", "forward", "none")

Forward = collections.namedtuple("SmForward", [
    "w1", "b1", "w2", "b2", "w3", "b3", "x",
    "h1", "h2", "h1_off", "h2_off"])

Steps = collections.namedtuple("SmSteps", [
    "sens", "steps",            # [NPARAMS] float64
    "tol_sens", "tol_steps",    # bound on |kernel - oracle|
    "round_sens", "round_steps",  # what the backward's bf16 roundings move
    "m", "tol_m",               # [2][NPARAMS] the two means and their bound
    "forward"])


def forward_rounded(theta, probe):
    """The kernel's forward: ``forward_oracle.forward`` and, from its
    widths, how far a flagged ``h1`` / ``h2`` can be off."""
    ref = fo.forward(theta, probe)
    pol = make_policy(theta)
    xb = fo.round_input(probe)
    t1 = xb[:, None, :] * pol.w1[None, :, :]
    e1 = SAFETY * N_L1 * U * (np.abs(t1).sum(-1) + np.abs(pol.b1))
    _r, _d, q1 = bf16_round(np.tanh(ref.pre1))
    w_h1 = EPS_TANH + e1 * tanh_slope(ref.pre1, e1)
    h1_off = ref.h1_flag * fo._spacings(w_h1, q1) * q1
    t2 = ref.h1[:, None, :] * pol.w2[None, :, :]
    e2 = SAFETY * N_L2 * U * (np.abs(t2).sum(-1) + np.abs(pol.b2))
    shift2 = h1_off @ pol.w2_abs.T
    slope2 = tanh_slope(ref.pre2, shift2 + e2)
    _r, _d, q2 = bf16_round(np.tanh(ref.pre2))
    w_h2 = EPS_TANH + (e2 + shift2) * slope2
    h2_off = ref.h2_flag * fo._spacings(w_h2, q2) * q2
    return Forward(pol.w1, pol.b1, pol.w2, pol.b2, pol.w3, pol.b3, xb,
                   ref.h1, ref.h2, h1_off, h2_off)


def forward_plain(theta, probe):
    """The fp64 MLP with nothing rounded."""
    th = np.asarray(theta, dtype=np.float32).astype(np.float64)
    assert th.shape == (NPARAMS,)
    w1 = th[:OFF_B1].reshape(HID, OBS)
    b1 = th[OFF_B1:OFF_W2]
    w2 = th[OFF_W2:OFF_B2].reshape(HID, HID)
    b2 = th[OFF_B2:OFF_W3]
    w3 = th[OFF_W3:OFF_B3].reshape(2, HID)
    b3 = th[OFF_B3:]
    x = np.asarray(probe, dtype=np.float32).astype(np.float64)
    h1 = np.tanh(x @ w1.T + b1)
    h2 = np.tanh(h1 @ w2.T + b2)
    zero = np.zeros_like(h1)
    return Forward(w1, b1, w2, b2, w3, b3, x, h1, h2, zero, zero)


def _round_bwd(raw, err, mirror):
    """bf16(raw) as the kernel forms it from a value within ``err`` of
    ``raw``: (value, bound on |kernel's - value|, half a spacing)."""
    if not mirror:
        return raw, np.zeros_like(raw), np.zeros_like(raw)
    r, dist, q = bf16_round(raw)
    flag = dist < err
    return r, flag * fo._spacings(err, q) * q, q / 2.0


def _flat(gw1, gb1, gw2, gb2, gw3, gb3):
    return np.concatenate([gw1.reshape(-1), gb1, gw2.reshape(-1), gb2,
                           gw3.reshape(-1), gb3])


def means(fw, mode, mirror, fp32):
    """``m[2][NPARAMS]`` of the forward ``fw`` with its kernel tolerance and
    the bound of the backward's own roundings.  ``mirror``: round ``d2`` /
    ``d1`` to bf16; ``fp32``: charge the fp32 operations."""
    assert mode in MODES, mode
    op = np.abs if mode == "abs" else (lambda v: v)
    u = U if fp32 else 0.0
    w2_abs, x_abs, h1_abs = np.abs(fw.w2), np.abs(fw.x), np.abs(fw.h1)
    s2 = 1.0 - fw.h2 ** 2
    e_s2 = 2.0 * np.abs(fw.h2) * fw.h2_off + fw.h2_off ** 2 + u * np.abs(s2)
    s1 = 1.0 - fw.h1 ** 2
    e_s1 = 2.0 * h1_abs * fw.h1_off + fw.h1_off ** 2 + u * np.abs(s1)
    m, tol, rnd = [], [], []
    for k in range(2):
        # d2[b][i] = bf16(w3[k][i] * s2[b][i])
        d2raw = fw.w3[k][None, :] * s2
        d2, e_d2, r_d2 = _round_bwd(
            d2raw, np.abs(fw.w3[k])[None, :] * e_s2 + u * np.abs(d2raw),
            mirror)
        # P[b][j] = sum_i d2[b][i] w2[i][j]   (MFMA)
        t = d2[:, :, None] * fw.w2[None, :, :]
        P = t.sum(1)
        e_P = e_d2 @ w2_abs + SAFETY * N_SUM * u * np.abs(t).sum(1)
        r_P = r_d2 @ w2_abs
        # d1[b][j] = bf16(P * s1)
        d1raw = P * s1
        d1, e_d1, r_d1 = _round_bwd(
            d1raw, e_P * np.abs(s1) + np.abs(P) * e_s1 + e_P * e_s1
            + u * np.abs(d1raw), mirror)
        r_d1 = r_d1 + r_P * np.abs(s1)
        d2_abs, d1_abs = np.abs(d2), np.abs(d1)
        # dW2[i][j] = sum_b op(d2[b][i]) op(h1[b][j])   (MFMA)
        tw2 = op(d2)[:, :, None] * op(fw.h1)[:, None, :]
        e_w2 = ((e_d2[:, :, None] * (h1_abs + fw.h1_off)[:, None, :]
                 + d2_abs[:, :, None] * fw.h1_off[:, None, :]).sum(0)
                + SAFETY * N_SUM * u * np.abs(tw2).sum(0))
        r_w2 = (r_d2[:, :, None] * h1_abs[:, None, :]).sum(0)
        # dW1[j][d] = sum_b op(d1[b][j]) op(x[b][d])    (MFMA)
        tw1 = op(d1)[:, :, None] * op(fw.x)[:, None, :]
        e_w1 = ((e_d1[:, :, None] * x_abs[:, None, :]).sum(0)
                + SAFETY * N_SUM * u * np.abs(tw1).sum(0))
        r_w1 = (r_d1[:, :, None] * x_abs[:, None, :]).sum(0)
        # the VALU sums: b = 0..63 in order, round to nearest
        e_b2 = e_d2.sum(0) + N_SUM * u * d2_abs.sum(0)
        e_b1 = e_d1.sum(0) + N_SUM * u * d1_abs.sum(0)
        gw3 = np.zeros((2, HID))
        e_w3 = np.zeros((2, HID))
        gw3[k] = op(fw.h2).sum(0)
        e_w3[k] = fw.h2_off.sum(0) + N_SUM * u * np.abs(fw.h2).sum(0)
        gb3 = np.zeros(2)
        gb3[k] = float(BATCH)
        zero2 = np.zeros(2)
        m.append(_flat(tw1.sum(0), op(d1).sum(0), tw2.sum(0), op(d2).sum(0),
                       gw3, gb3) / BATCH)
        tol.append(_flat(e_w1, e_b1, e_w2, e_b2, e_w3, zero2) / BATCH)
        rnd.append(_flat(r_w1, r_d1.sum(0), r_w2, r_d2.sum(0),
                         np.zeros((2, HID)), zero2) / BATCH)
    return np.stack(m), np.stack(tol), np.stack(rnd)


def _finish(m, e_m, sigma, s_min, own):
    """sens and steps from the two means, and what a move of ``e_m`` in the
    means does to them (plus, with ``own``, their own fp32 roundings)."""
    sens = np.sqrt(m[0] ** 2 + m[1] ** 2)
    e_sens = np.sqrt(e_m[0] ** 2 + e_m[1] ** 2)
    if own:
        e_sens = e_sens + SENS_ROUNDINGS * U * sens + SENS_UNDERFLOW
    steps = sigma / np.maximum(sens, s_min)
    lo = sigma / np.maximum(np.maximum(sens - e_sens, 0.0), s_min)
    hi = sigma / np.maximum(sens + e_sens, s_min)
    e_steps = np.maximum(lo - steps, steps - hi)
    if own:
        e_steps = e_steps + U * steps
    return sens, steps, e_sens, e_steps


def steps(theta, probe, sigma, s_min=0.01, mode="abs", rounding="all"):
    """``sm_steps`` of one row: ``theta`` float32 [4610], ``probe`` float32
    [64][4], finite.  ``rounding``: "all" is the kernel; "forward" keeps
    the forward's bf16 roundings and leaves the backward unrounded; "none"
    is the plain fp64 MLP.  Only "all" charges fp32 operations."""
    assert rounding in ROUNDINGS, rounding
    probe = np.asarray(probe, dtype=np.float32)
    assert probe.shape == (BATCH, OBS), probe.shape
    sigma = float(np.float32(sigma))
    s_min = float(np.float32(s_min))
    fw = (forward_plain(theta, probe) if rounding == "none"
          else forward_rounded(theta, probe))
    kernel = rounding == "all"
    if not kernel:
        zero = np.zeros_like(fw.h1)
        fw = fw._replace(h1_off=zero, h2_off=zero)
    m, e_m, r_m = means(fw, mode, mirror=kernel, fp32=kernel)
    sens, st, e_sens, e_steps = _finish(m, e_m, sigma, s_min, own=kernel)
    _s, _t, r_sens, r_steps = _finish(m, r_m, sigma, s_min, own=False)
    return Steps(sens, st, e_sens, e_steps, r_sens, r_steps, m, e_m, fw)
