"""Float64 oracle of the LSTM policy kernels (CPU only).

A plain reading of ``lstm_cell`` in fiber_amd/csrc/ops/lstm_kernels.hip.
Everything is float64 except the roundings the kernel makes to bf16, which
are reproduced exactly: W_i, W_h and W_out when the policy is staged or
drawn, and the ``h`` the matmul reads.  The carried ``c``, ``c'`` and the
``h'`` the logits read stay unrounded, biases stay as given, and ``x`` is
taken as the caller gives it (bf16-valued).

The env phase of ``es_rollout_lstm`` is ``es_rollout_gru``'s, so ``observe``
and ``env_step`` are ``gru_oracle``'s.  As there, every rollout check
restarts from the kernel's own fp32 ``(state, hidden, cell)``: one ``cell``
and one ``env_step`` are all a test needs.  ``cell`` returns a tolerance per
output, built term by term from the kernel's arithmetic (profiles/lstm.md);
nothing here comes from a GPU run.
"""

import collections

import numpy as np

from .gru_oracle import (  # noqa: F401  (C01, X_REL, ...: for the tests)
    C01, C1EM4, EPS_SIG, EPS_TANH, N_LOGIT, SAFETY, U, X_REL, Z_REL,
    _sigmoid, _sigmoid_slope, bf16_round, env_step, observe, tanh_slope)

OBS, HID, ACT, GATES = 4, 64, 2, 4  # gates i, f, g, o: torch's order
OFF_WH, OFF_B, OFF_WO, OFF_BO, LSTM_NPARAMS = 1024, 17408, 17664, 17792, 17794

# fp32 terms that meet in one gate accumulator: 4 + 64 products and the bias
# it starts from.  Any order of n terms is within (n-1)*U*sum|terms|.
N_GATE = OBS + HID + 1

Policy = collections.namedtuple("Policy", [
    "wi", "wh", "b", "wo", "bo",        # [4][64][4] [4][64][64] [4][64] ...
    "wi_slack", "wh_slack", "wo_slack",  # bf16 spacing where flagged, else 0
    "b_err", "bo_err",                   # fp32 uncertainty of the biases
    "bf16"])                             # False: nothing is rounded


def make_policy(theta, sgn=0.0, z=None, bf16=True):
    """The policy as the kernel stages it.  ``theta`` float32
    [LSTM_NPARAMS]; for a perturbed member ``z`` is the pair's float32 noise
    and ``sgn`` is +-sigma.  The kernel forms ``fmaf(sgn, z, theta)`` from
    its own z, so the exact float64 value here is known only to within
    ``|sgn z| * (Z_REL + U) + U*|w|`` (rollout_oracle's rule): a weight
    closer than that to a bf16 midpoint is flagged and may round the other
    way.  ``bf16=False`` leaves the weights unrounded."""
    th = np.asarray(theta, dtype=np.float32).astype(np.float64)
    assert th.shape == (LSTM_NPARAMS,)
    if z is None:
        w, width = th, np.zeros_like(th)
    else:
        sz = float(np.float32(sgn)) * np.asarray(
            z, dtype=np.float32).astype(np.float64)
        w = th + sz
        width = np.abs(sz) * (Z_REL + U) + U * np.abs(w)

    def weights(lo, hi, shape):
        if not bf16:
            return w[lo:hi].reshape(shape), np.zeros(shape)
        r, dist, q = bf16_round(w[lo:hi])
        return r.reshape(shape), ((dist < width[lo:hi]) * q).reshape(shape)

    wi, wi_s = weights(0, OFF_WH, (GATES, HID, OBS))
    wh, wh_s = weights(OFF_WH, OFF_B, (GATES, HID, HID))
    wo, wo_s = weights(OFF_WO, OFF_BO, (ACT, HID))
    return Policy(wi, wh, w[OFF_B:OFF_WO].reshape(GATES, HID), wo,
                  w[OFF_BO:], wi_s, wh_s, wo_s,
                  width[OFF_B:OFF_WO].reshape(GATES, HID), width[OFF_BO:],
                  bf16)


def cell(pol, x, h, c, x_slack=None, slip=None, with_pre=False):
    """One step for ``x`` [E][4] and the carried ``h``, ``c`` [E][64]:
    ``(h', c', logits, tol_h, tol_c, tol_logits)``; ``with_pre`` appends the
    gate pre-activations ``(a_i, a_f, a_g, a_o)``, each [E][64].  ``x_slack``
    [E][4] is what the kernel's x may differ by (the bf16 spacing where its
    rounding is ambiguous).  With a ``bf16=False`` policy ``h`` is not
    rounded either: the plain float64 cell.

    ``slip`` names a deliberate mistake, for the tests that show the
    tolerances are sharp: ``"c_rounded"`` (the carried c rounded to bf16
    before ``f c``), ``"if_swapped"`` (``c' = i c + f g``), ``"tanh_c_old"``
    (``h' = o tanh(c)`` of the incoming c), ``"h_rounded"`` (the logits read
    ``bf16(h')``).  The tolerances returned with a slip are those of the
    slipped values and serve no comparison."""
    assert slip in (None, "c_rounded", "if_swapped", "tanh_c_old",
                    "h_rounded"), slip
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    hb = bf16_round(h)[0] if pol.bf16 else h
    xs = np.zeros_like(x) if x_slack is None else np.asarray(x_slack)

    def gate(g):
        """Pre-activation of gate g and its fp32 bound: the accumulator
        starts from the bias and takes the x and the h products."""
        a = pol.b[g][None, :] + x @ pol.wi[g].T + hb @ pol.wh[g].T
        mag = (np.abs(pol.b[g])[None, :] + np.abs(x) @ np.abs(pol.wi[g]).T
               + np.abs(hb) @ np.abs(pol.wh[g]).T)
        err = (pol.b_err[g][None, :] + np.abs(x) @ pol.wi_slack[g].T
               + xs @ np.abs(pol.wi[g]).T + np.abs(hb) @ pol.wh_slack[g].T)
        return a, err + SAFETY * (N_GATE - 1) * U * mag

    (a_i, e_i), (a_f, e_f), (a_g, e_g), (a_o, e_o) = (gate(g) for g in
                                                     range(GATES))
    ig, fg, og = _sigmoid(a_i), _sigmoid(a_f), _sigmoid(a_o)
    gg = np.tanh(a_g)
    err_i = EPS_SIG + _sigmoid_slope(a_i, e_i) * e_i
    err_f = EPS_SIG + _sigmoid_slope(a_f, e_f) * e_f
    err_o = EPS_SIG + _sigmoid_slope(a_o, e_o) * e_o
    err_g = EPS_TANH + tanh_slope(a_g, e_g) * e_g
    # the kernel: p = i * g (rounded), c' = fmaf(f, c, p) (rounded); c is the
    # caller's fp32 value, exact on both sides
    if slip == "c_rounded":
        c = bf16_round(c)[0]
    elif slip == "if_swapped":
        ig, fg = fg, ig
    p = ig * gg
    err_p = err_i * (np.abs(gg) + err_g) + ig * err_g
    err_p = err_p + U * (np.abs(p) + err_p)
    cn = fg * c + p
    tol_c = err_f * np.abs(c) + err_p
    tol_c = tol_c + U * (np.abs(cn) + tol_c)
    # h' = o * tanh(c') (rounded), tanh of the kernel's own c'
    tc = np.tanh(c if slip == "tanh_c_old" else cn)
    err_t = EPS_TANH + tanh_slope(cn, tol_c) * tol_c
    hn = og * tc
    tol_h = err_o * (np.abs(tc) + err_t) + og * err_t
    tol_h = tol_h + U * (np.abs(hn) + tol_h)
    # logits from the kernel's own fp32 h', which is within tol_h of hn
    hl = bf16_round(hn)[0] if slip == "h_rounded" else hn
    t = hl[:, None, :] * pol.wo[None, :, :]               # [E][2][64]
    logits = t.sum(-1) + pol.bo
    tol_l = (tol_h @ np.abs(pol.wo).T + np.abs(hn) @ pol.wo_slack.T
             + N_LOGIT * U * (np.abs(t).sum(-1) + np.abs(pol.bo))
             + pol.bo_err)
    if with_pre:
        return hn, cn, logits, tol_h, tol_c, tol_l, (a_i, a_f, a_g, a_o)
    return hn, cn, logits, tol_h, tol_c, tol_l


Rollout = collections.namedtuple("Rollout", [
    "s",        # [steps + 1][E][4]   env state, s[0] = s0
    "h",        # [steps + 1][E][64]  carried hidden state, h[0] = 0
    "c",        # [steps + 1][E][64]  carried cell state, c[0] = 0
    "x",        # [steps][E][4]       what the policy saw at step t
    "x_raw",    # [steps][E][4]       normalised obs before mask and clamp
    "pre",      # [steps][4][E][64]   gate pre-activations a_i, a_f, a_g, a_o
    "logits",   # [steps][E][2]
    "tol_l",    # [steps][E][2]       cell's logits tolerance at step t
    "action"])  # [steps][E]          l1 > l0


def rollout(pol, obs_mu, obs_nu, obs_mask, env_A, env_B, s0, steps):
    """``observe -> cell -> env_step`` chained for ``steps`` steps from the
    state ``s0`` [E][4] and zero hidden and cell states.  The state, the
    hidden and the cell state are rounded to fp32 between steps, as the
    kernel holds them.

    This serves only to choose test inputs and to state conditions about
    them on the CPU (how many steps are decided, where the clamp fires, how
    far the gates saturate, how large c grows).  Its tolerances are those of
    one step: nothing here bounds the kernel over several steps, and no
    comparison with the kernel goes through it."""
    mu = np.asarray(obs_mu, dtype=np.float32).astype(np.float64)
    nu = np.asarray(obs_nu, dtype=np.float32).astype(np.float64)
    s = np.asarray(s0, dtype=np.float32)
    h = np.zeros((s.shape[0], HID), dtype=np.float32)
    c = np.zeros((s.shape[0], HID), dtype=np.float32)
    out = {k: [] for k in Rollout._fields}
    out["s"].append(s)
    out["h"].append(h)
    out["c"].append(c)
    for _t in range(steps):
        x, x_slack = observe(s, mu, nu, obs_mask)
        hn, cn, logits, _tol_h, _tol_c, tol_l, pre = cell(
            pol, x, h, c, x_slack, with_pre=True)
        action = logits[:, 1] > logits[:, 0]
        s = env_step(s, action, env_A, env_B)[0].astype(np.float32)
        h, c = hn.astype(np.float32), cn.astype(np.float32)
        out["x"].append(x)
        out["x_raw"].append(
            (out["s"][-1].astype(np.float64) - mu) / np.sqrt(nu + C1EM4))
        out["pre"].append(np.stack(pre))
        out["logits"].append(logits)
        out["tol_l"].append(tol_l)
        out["action"].append(action)
        out["s"].append(s)
        out["h"].append(h)
        out["c"].append(c)
    return Rollout(*(np.stack(out[k]) if out[k] else np.zeros((0,))
                     for k in Rollout._fields))
