"""Float64 oracle of the serving forward kernel and the MFMA probe (CPU
only).

A reading of ``mlp_policy_forward`` and ``mfma_gemm64_probe`` in
fiber_amd/csrc/ops/es_kernels.hip, written from the kernel source.  It
shares nothing with ``ops.mlp_policy_forward_ref``; the policy staging, the
bf16 rounding and every constant are those of ``rollout_oracle``.

Everything is float64 except the roundings the kernel makes to bf16, which
are reproduced exactly: W1, W2, W3 when the policy is staged, the input
``x``, ``h1`` and, unlike the rollout step loop, ``h2``.  Biases stay fp32.
The last layer is a sequential chain ``l = b3; l += w3[a][i] * h2[i]`` over
i = 0..63 in fp32.

``x``, the weights and the biases are given exactly, so their roundings are
the same on both sides.  ``h1`` and ``h2`` are roundings of values that the
kernel knows only to within its fp32 error: a value closer to a bf16
rounding midpoint than that error may round the other way in the kernel,
one bf16 spacing off.  The tolerance of a logit is therefore the sum of

* the fp32 bound: the accumulation error of each layer and EPS_TANH per
  activation, carried forward through ``tanh_slope`` and ``|W|`` as
  ``rollout_oracle.rollout`` carries them, and
* for every flagged ``h1[j]`` or ``h2[i]``, one bf16 spacing times its
  sensitivity: ``sum_i |w3[a][i]| slope2[i] |w2[i][j]|`` for h1[j],
  ``|w3[a][i]|`` for h2[i].

The width that flags ``h2[i]`` includes what the flagged ``h1`` can move
its pre-activation by (``shift2``): an h1 that goes the other way can carry
an h2 across a midpoint, which costs a whole spacing of h2 whatever the
slope.

That sum (``forward``) is an envelope: it holds whichever way each flagged
value went, and a single flagged h2 widens it by up to 3.9e-3 |w3|.  The
criterion proper (``resolve``) takes the kernel's output and asks whether
some permitted choice of roundings reproduces it within the fp32 bound
alone.  Derivation and measured figures: profiles/forward_oracle.md.
Nothing here comes from a GPU run.
"""

import collections

import numpy as np

from .rollout_oracle import (EPS_TANH, HID, N_L1, N_L2, OBS, SAFETY, U,
                             bf16_other_neighbour, bf16_round, make_policy,
                             tanh_slope)

# The two MFMA layers: (n-1) adds of n terms, each within U of a partial sum
# that never exceeds sum|terms|, taken as N * U * sum|terms| with the N of
# rollout_oracle (4 products + bias, 64 products + bias).  SAFETY covers
# MFMA adds that truncate instead of rounding to nearest, so it multiplies
# these two bounds and nothing else.
#
# The last layer runs in the VALU, round to nearest.  A product of two bf16
# values has 16 significant bits and is exact in fp32, so fused or not each
# of the 64 steps rounds once, by at most U of a partial sum that stays
# under |b3| + sum|terms|.
N_L3 = 64

# bf16 keeps the exponent range of fp32: below 2^-126 its spacing stops
# shrinking at 2^-133.
BF16_MIN_NORMAL = 2.0 ** -126
BF16_DENORM_Q = 2.0 ** -133

Forward = collections.namedtuple("Forward", [
    "logits",      # [B][2]   float64
    "tol",         # [B][2]   bound on |kernel - logits|
    "tol_fp32",    # [B][2]   its first term
    "tol_flip",    # [B][2]   its second term
    "h1", "h1_alt", "h1_flag",     # [B][64]
    "h2", "h2_alt", "h2_flag",     # [B][64]
    "pre1", "pre2"])               # [B][64]


def round_input(x):
    """fp32 ``x`` to bf16 as __float2bfloat16 does (nearest, ties to even),
    in float64.  x is given exactly, so there is nothing to flag.  Inputs
    under 2^-126 land on the bf16 denormal grid; whether the MFMA then
    reads them or flushes them moves a pre-activation by less than
    2^-126 * sum|w1|, far below U of anything here."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    r, _dist, _q = bf16_round(x)
    tiny = np.abs(x) < BF16_MIN_NORMAL
    return np.where(tiny, np.rint(x / BF16_DENORM_Q) * BF16_DENORM_Q, r)


def _spacings(width, q):
    """How many bf16 spacings a flagged value can be off: one, unless its
    width itself exceeds a spacing."""
    return np.maximum(1.0, np.ceil(width / q))


def forward(theta, x):
    """Logits of ``mlp_policy_forward(theta, x)`` and their tolerance, both
    [B][2], with the intermediate values.  ``theta`` float32 [4610], ``x``
    float32 [B][4], finite."""
    pol = make_policy(theta)
    xb = round_input(x)
    assert xb.ndim == 2 and xb.shape[1] == OBS
    # ---- layer 1: h1 = bf16(tanh(W1 x + b1)) ---------------------------
    t1 = xb[:, None, :] * pol.w1[None, :, :]              # [B][64][4]
    pre1 = t1.sum(-1) + pol.b1
    e1 = SAFETY * N_L1 * U * (np.abs(t1).sum(-1) + np.abs(pol.b1))
    h1_raw = np.tanh(pre1)
    h1, h1_dist, h1_q = bf16_round(h1_raw)
    w_h1 = EPS_TANH + e1 * tanh_slope(pre1, e1)
    h1_flag = h1_dist < w_h1
    h1_off = h1_flag * _spacings(w_h1, h1_q) * h1_q
    # ---- layer 2: h2 = bf16(tanh(W2 h1 + b2)) --------------------------
    t2 = h1[:, None, :] * pol.w2[None, :, :]              # [B][64][64]
    pre2 = t2.sum(-1) + pol.b2
    e2 = SAFETY * N_L2 * U * (np.abs(t2).sum(-1) + np.abs(pol.b2))
    shift2 = h1_off @ pol.w2_abs.T
    slope2 = tanh_slope(pre2, shift2 + e2)
    h2_raw = np.tanh(pre2)
    h2, h2_dist, h2_q = bf16_round(h2_raw)
    h2_err = EPS_TANH + e2 * slope2
    w_h2 = h2_err + shift2 * slope2
    h2_flag = h2_dist < w_h2
    h2_off = h2_flag * _spacings(w_h2, h2_q) * h2_q
    # ---- logits: b3 + sum_i w3[a][i] h2[i] ------------------------------
    w3_abs = np.abs(pol.w3)
    t3 = h2[:, None, :] * pol.w3[None, :, :]              # [B][2][64]
    logits = t3.sum(-1) + pol.b3
    tol_fp32 = (h2_err @ w3_abs.T
                + N_L3 * U * (np.abs(t3).sum(-1) + np.abs(pol.b3)))
    # sens1[b][a][j] = sum_i |w3[a][i]| slope2[b][i] |w2[i][j]|
    sens1 = np.einsum("ai,bi,ij->baj", w3_abs, slope2, pol.w2_abs)
    tol_flip = ((sens1 * h1_off[:, None, :]).sum(-1) + h2_off @ w3_abs.T)
    return Forward(
        logits, tol_fp32 + tol_flip, tol_fp32, tol_flip,
        h1, bf16_other_neighbour(h1_raw, h1, h1_q), h1_flag,
        h2, bf16_other_neighbour(h2_raw, h2, h2_q), h2_flag, pre1, pre2)


Resolved = collections.namedtuple("Resolved", [
    "logits",    # [B][2]  the oracle's logits under the chosen roundings
    "tol",       # [B][2]  the tolerance applied to them
    "ratio",     # [B]     max_a |got - logits| / tol
    "flipped"])  # [B]     flagged values taken the other way


_MASKS = {}


def _masks(k):
    if k not in _MASKS:
        _MASKS[k] = ((np.arange(1 << k)[:, None] >> np.arange(k)) & 1).astype(
            np.float64)
    return _MASKS[k]


def resolve(theta, x, got, max_h1=4, max_h2=14, ref=None):
    """The sharp form of the criterion.  ``forward`` charges every flagged
    value its whole spacing, whether or not the kernel took it the other
    way; that envelope runs to 1e-2 where the fp32 term is 5e-4.  Here the
    flagged roundings are resolved against ``got`` [B][2] instead: a row
    passes iff *some* permitted choice, each flagged h1 and h2 at its
    nearest value or at its other neighbour, gives logits within the fp32
    term of both of the row's ``got``.

    Per row: the nearest roundings are tried first.  If they miss, and the
    row lies inside the envelope (outside it no choice can fit), the
    subsets of the flagged h1 are enumerated, layer 2 recomputed for each,
    and for each the subsets of its flagged h2, whose moves add up
    linearly in the logits.  A flagged value whose width spans several
    spacings (only next to 0, where bf16 is finer than EPS_TANH) is not
    enumerated: a wide h1 widens the h2 widths by what it can shift the
    pre-activations, a wide h2 stays in the tolerance at its whole width.
    So do the cheapest flagged h2 past the ``max_h2`` dearest of a row,
    and a row with more than ``max_h1`` flagged h1 keeps the envelope."""
    if ref is None:
        ref = forward(theta, x)
    pol = make_policy(theta)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.logits.shape, (got.shape, ref.logits.shape)
    w3, w3_abs = pol.w3, np.abs(pol.w3)
    B = got.shape[0]
    out_l, out_t = ref.logits.copy(), ref.tol.copy()
    out_r, out_f = np.empty(B), np.zeros(B, int)
    xb = round_input(x)
    for b in range(B):
        env = (np.abs(got[b] - ref.logits[b]) / ref.tol[b]).max()
        # layer 1 of this row again, for the widths
        t1 = xb[b][None, :] * pol.w1
        pre1 = t1.sum(-1) + pol.b1
        e1 = SAFETY * N_L1 * U * (np.abs(t1).sum(-1) + np.abs(pol.b1))
        _r, _d, q1 = bf16_round(np.tanh(pre1))
        n1 = _spacings(EPS_TANH + e1 * tanh_slope(pre1, e1), q1)
        wide1 = ref.h1_flag[b] & (n1 > 1)
        narrow1 = np.flatnonzero(ref.h1_flag[b] & (n1 == 1))
        shiftw = (wide1 * n1 * q1) @ pol.w2_abs.T
        best = None
        subsets1 = range(1 << len(narrow1)) if len(narrow1) <= max_h1 else ()
        for s1 in subsets1:
            h1 = ref.h1[b].copy()
            take = narrow1[[(s1 >> i) & 1 == 1 for i in range(len(narrow1))]]
            h1[take] = ref.h1_alt[b][take]
            t2 = h1[None, :] * pol.w2
            pre2 = t2.sum(-1) + pol.b2
            e2 = SAFETY * N_L2 * U * (np.abs(t2).sum(-1) + np.abs(pol.b2))
            slope2 = tanh_slope(pre2, shiftw + e2)
            raw = np.tanh(pre2)
            h2, dist, q2 = bf16_round(raw)
            err = EPS_TANH + e2 * slope2
            w = err + shiftw * slope2
            n2 = _spacings(w, q2)
            flag = dist < w
            base = h2 @ w3.T + pol.b3
            tol = (w3_abs @ (err + flag * (n2 > 1) * n2 * q2)
                   + N_L3 * U * (np.abs(h2[None, :] * w3).sum(-1)
                                 + np.abs(pol.b3)))
            idx = np.flatnonzero(flag & (n2 == 1))
            move = ((bf16_other_neighbour(raw, h2, q2) - h2)[idx, None]
                    * w3.T[idx])                            # [k][2]
            if len(idx) > max_h2:
                order = np.argsort(-np.abs(move).max(-1))
                tol = tol + np.abs(move[order[max_h2:]]).sum(0)
                idx, move = idx[order[:max_h2]], move[order[:max_h2]]
            masks = _masks(len(idx))
            sums = masks @ move if len(idx) else np.zeros((1, 2))
            ratios = (np.abs(got[b] - base - sums) / tol).max(-1)
            pick = int(np.argmin(ratios))
            if best is None or ratios[pick] < best[0]:
                best = (ratios[pick], base + sums[pick], tol,
                        len(take) + int(masks[pick].sum()))
            if best[0] <= 1.0 or env > 1.0:
                # found a fit, or outside the envelope: nothing can fit
                break
        if best is None:
            out_r[b] = env
        else:
            out_r[b], out_l[b], out_t[b], out_f[b] = best
            if env > 1.0:
                out_r[b] = max(out_r[b], env)
    return Resolved(out_l, out_t, out_r, out_f)


def h2_rounding_margin(pol, h1):
    """What rounding ``h2`` to bf16 can move ``l1 - l0`` by, for bf16-valued
    ``h1[..., 64]`` of the policy ``pol``: ``sum_i |w3[1][i] - w3[0][i]| *
    spacing(h2_i) / 2``.  The rollout step loop keeps h2 in fp32, the
    serving kernel rounds it; a step whose margin clears the rollout
    oracle's threshold by more than SAFETY times this has the same action
    on both paths."""
    h2 = np.tanh(h1 @ pol.w2.T + pol.b2)
    _r, _dist, q = bf16_round(h2)
    return (pol.dw3 * q).sum(-1) / 2.0


Probe = collections.namedtuple("Probe", ["value", "alt", "flag", "lo", "hi"])


def probe_reference(a, b):
    """``mfma_gemm64_probe(a, b)`` for fp32 ``a``, ``b`` [64][64]: per
    element ``value = bf16(tanh(sum_k bf16(a[r][k]) bf16(b[k][c])))`` with
    the sum in float64, the other bf16 neighbour ``alt``, and the ``flag``
    that permits it: the tanh closer to a midpoint than its fp32 error
    ``w`` (EPS_TANH plus the slope times the bound of the 64-term MFMA
    sum).

    EPS_TANH is absolute, so near 0, where bf16 is finer than it, ``w``
    spans several spacings: ``lo`` and ``hi`` are the roundings of
    ``tanh -+ w``, the whole permitted range.  Where ``w`` is under a
    spacing, which is everywhere above about 1e-3, that range is ``value``
    alone, or ``value`` and ``alt`` if flagged."""
    ab, bb = round_input(a), round_input(b)
    assert ab.shape == (HID, HID) and bb.shape == (HID, HID)
    t = ab[:, :, None] * bb[None, :, :]                   # [r][k][c]
    pre = t.sum(1)
    e = SAFETY * N_L2 * U * np.abs(t).sum(1)
    raw = np.tanh(pre)
    r, dist, q = bf16_round(raw)
    w = EPS_TANH + e * tanh_slope(pre, e)
    return Probe(r, bf16_other_neighbour(raw, r, q), dist < w,
                 bf16_round(raw - w)[0], bf16_round(raw + w)[0])


def probe_mismatches(got, ref):
    """Elements [r][c] of ``got`` that are no permitted bf16 value."""
    got = np.asarray(got, dtype=np.float64)
    ok = (got >= ref.lo) & (got <= ref.hi) & (bf16_round(got)[0] == got)
    return np.argwhere(~ok)
