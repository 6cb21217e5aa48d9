"""Float64 oracle of the GRU policy kernels (CPU only).

A plain reading of ``gru_cell`` and of the env phase of ``es_rollout_gru``
in fiber_amd/csrc/ops/gru_kernels.hip.  Everything is float64 except the
roundings the kernel makes to bf16, which are reproduced exactly: W_i, W_h
and W_o when the policy is staged, and the ``h`` the matmul reads.  The
carried ``h`` and the ``h'`` the logits read stay unrounded, biases stay
as given, and ``x`` is taken as the caller gives it (bf16-valued).

There is no bookkeeping across steps: every rollout check restarts from
the kernel's own fp32 ``(state, hidden)``, so one ``cell`` and one
``env_step`` are all a test needs.  ``cell`` returns a tolerance per
output, built term by term from the kernel's arithmetic
(profiles/gru.md); nothing here comes from a GPU run.
"""

import collections

import numpy as np

from .rollout_oracle import (  # noqa: F401  (C01, X_REL: for the tests)
    C01, C005, C008, C097, C1EM4, EPS_TANH, N_LOGIT, SAFETY, U, ULP, X_REL,
    Z_REL, bf16_round, tanh_slope)

OBS, HID, ACT, GATES = 4, 64, 2, 3
OFF_WH, OFF_B, OFF_WO, OFF_BO, GRU_NPARAMS = 768, 13056, 13312, 13440, 13442

LOG2E = float.fromhex("0x1.715476p+0")

# ---- fast_sigmoid -----------------------------------------------------------
# rcp(1 + exp2(a * -log2e)).  Largest |fp32 emulation - fp64 sigmoid| with
# exp2 and rcp taken as correctly rounded: measure_sigmoid_emulation_error
# gives 9.16e-8 (tests/test_gru_oracle.py measures it again).
SIG_EMUL_ERR = 1.0e-7
# v_exp_f32 and v_rcp_f32 are documented to 1 ulp.  s = 1/(1+e): ds/de * e*ULP
# = e/(1+e)^2 * ULP <= ULP/4, and 1 ulp of the reciprocal s <= 1 is ULP.
SIG_HW_ERR = 0.25 * ULP + ULP
# the factor EPS_TANH carries over its measured + documented parts
EPS_SIG = 4.0 * (SIG_EMUL_ERR + SIG_HW_ERR)

# fp32 terms that meet in one gate accumulator: 4 + 64 products and the bias
# it starts from.  Any order of n terms is within (n-1)*U*sum|terms|.
N_GATE = OBS + HID + 1


def measure_sigmoid_emulation_error(dense=32.0, limit=1e4, n=2_000_001):
    """max |fp32 emulation of fast_sigmoid - fp64 sigmoid|, on the grid of
    ``rollout_oracle.measure_tanh_emulation_error``; each fp32 operation
    rounds once, exp2 and the reciprocal as correctly rounded."""
    x = np.concatenate([
        np.linspace(-dense, dense, n),
        np.geomspace(1e-9, limit, n // 4),
        -np.geomspace(1e-9, limit, n // 4),
    ]).astype(np.float32)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        m = x * np.float32(-LOG2E)                              # v_mul_f32
        e = np.exp2(m.astype(np.float64)).astype(np.float32)    # v_exp_f32
        ep1 = np.float32(1.0) + e                               # v_add_f32
        s = (1.0 / ep1.astype(np.float64)).astype(np.float32)   # v_rcp_f32
        ref = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    return float(np.max(np.abs(s.astype(np.float64) - ref)))


Policy = collections.namedtuple("Policy", [
    "wi", "wh", "b", "wo", "bo",        # [3][64][4] [3][64][64] [4][64] ...
    "wi_slack", "wh_slack", "wo_slack",  # bf16 spacing where flagged, else 0
    "b_err", "bo_err"])                  # fp32 uncertainty of the biases


def make_policy(theta, sgn=0.0, z=None, bf16=True):
    """The policy as the kernel stages it.  ``theta`` float32
    [GRU_NPARAMS]; for a perturbed member ``z`` is the pair's float32 noise
    and ``sgn`` is +-sigma.  The kernel forms ``fmaf(sgn, z, theta)`` from
    its own z, so the exact float64 value here is known only to within
    ``|sgn z| * (Z_REL + U) + U*|w|`` (rollout_oracle's rule): a weight
    closer than that to a bf16 midpoint is flagged and may round the other
    way.  ``bf16=False`` leaves the weights unrounded."""
    th = np.asarray(theta, dtype=np.float32).astype(np.float64)
    assert th.shape == (GRU_NPARAMS,)
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
    return Policy(wi, wh, w[OFF_B:OFF_WO].reshape(4, HID), wo, w[OFF_BO:],
                  wi_s, wh_s, wo_s, width[OFF_B:OFF_WO].reshape(4, HID),
                  width[OFF_BO:])


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def _sigmoid_slope(a, radius):
    """Upper bound of sigmoid' on [a - radius, a + radius]."""
    s = _sigmoid(np.maximum(np.abs(a) - radius, 0.0))
    return s * (1.0 - s)


def cell(pol, x, h, x_slack=None, bf16=True, slip=None, with_pre=False):
    """One step for ``x`` [E][4] and the carried ``h`` [E][64]:
    ``(h', logits, tol_h, tol_logits)``; ``with_pre`` appends the gate
    pre-activations ``(a_r, a_z, a_n)``, each [E][64].

    ``x_slack`` [E][4] is what the kernel's x may differ by (the bf16
    spacing where its rounding is ambiguous).  ``slip`` names a deliberate
    mistake, for the tests that show the tolerance is sharp: ``"r_inside"``
    (r multiplied into h before W_hn), ``"z_swapped"``, ``"h_rounded"`` (the
    carried h rounded to bf16)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    hb = bf16_round(h)[0] if bf16 else h
    xs = np.zeros_like(x) if x_slack is None else np.asarray(x_slack)

    def gate(g, bias_rows, use_x=True, use_h=True, hin=hb):
        """Pre-activation of accumulator (g, parts) and its fp32 bound."""
        a = sum(pol.b[r] for r in bias_rows)[None, :] + 0.0
        mag = sum(np.abs(pol.b[r]) for r in bias_rows)[None, :] + 0.0
        err = sum(pol.b_err[r] for r in bias_rows)[None, :] + 0.0
        if use_x:
            a = a + x @ pol.wi[g].T
            mag = mag + np.abs(x) @ np.abs(pol.wi[g]).T
            err = (err + np.abs(x) @ pol.wi_slack[g].T
                   + xs @ np.abs(pol.wi[g]).T)
        if use_h:
            a = a + hin @ pol.wh[g].T
            mag = mag + np.abs(hin) @ np.abs(pol.wh[g]).T
            err = err + np.abs(hin) @ pol.wh_slack[g].T
        return a, err + SAFETY * (N_GATE - 1) * U * mag

    a_r, e_r = gate(0, (0,))
    a_z, e_z = gate(1, (1,))
    r, z = _sigmoid(a_r), _sigmoid(a_z)
    err_r = EPS_SIG + _sigmoid_slope(a_r, e_r) * e_r
    err_z = EPS_SIG + _sigmoid_slope(a_z, e_z) * e_z
    a_nx, e_nx = gate(2, (2,), use_h=False)
    if slip == "r_inside":
        a_nh, e_nh = gate(2, (3,), use_x=False, hin=r * hb)
        pre = a_nx + a_nh
    else:
        a_nh, e_nh = gate(2, (3,), use_x=False)
        pre = a_nx + r * a_nh                        # one fmaf
    e_pre = (e_nx + r * e_nh + err_r * (np.abs(a_nh) + e_nh)
             + U * np.abs(pre))
    n = np.tanh(pre)
    err_n = EPS_TANH + tanh_slope(pre, e_pre) * e_pre
    hc = bf16_round(h)[0] if slip == "h_rounded" else h
    if slip == "z_swapped":
        z = 1.0 - z
    # the kernel: d = h - n (rounded), h' = fmaf(z, d, n) (rounded)
    hn = n + z * (hc - n)
    tol_h = ((1.0 - z) * err_n + err_z * (np.abs(hc - n) + err_n)
             + U * (np.abs(hc - n) * z + np.abs(hn)))
    # logits from the kernel's own fp32 h', which is within tol_h of hn
    t = hn[:, None, :] * pol.wo[None, :, :]               # [E][2][64]
    logits = t.sum(-1) + pol.bo
    tol_l = (tol_h @ np.abs(pol.wo).T + np.abs(hn) @ pol.wo_slack.T
             + N_LOGIT * U * (np.abs(t).sum(-1) + np.abs(pol.bo))
             + pol.bo_err)
    if with_pre:
        return hn, logits, tol_h, tol_l, (a_r, a_z, pre)
    return hn, logits, tol_h, tol_l


def observe(s, obs_mu, obs_nu, obs_mask=0b1111):
    """The kernel's x for the fp32 state ``s`` [E][4]: normalised, hidden
    dims zeroed, clamped to +-5, rounded to bf16.  Returns ``(x, x_slack)``;
    the slack is the bf16 spacing where x lies within the fp32 error of
    ``(s - mu) * rsqrtf(nu + 1e-4f)`` of a rounding midpoint."""
    s = np.asarray(s, dtype=np.float32).astype(np.float64)
    mu = np.asarray(obs_mu, dtype=np.float32).astype(np.float64)
    nu = np.asarray(obs_nu, dtype=np.float32).astype(np.float64)
    raw = (s - mu) / np.sqrt(nu + C1EM4)
    vis = np.array([(int(obs_mask) >> d) & 1 for d in range(OBS)], bool)
    x, dist, q = bf16_round(np.where(vis, np.clip(raw, -5.0, 5.0), 0.0))
    return x, np.where(vis & (dist < X_REL * np.abs(raw)), q, 0.0)


def env_step(s, action, env_A, env_B):
    """``(s', bound on |kernel's s' - it|)`` for the fp32 state ``s`` [E][4]
    and ``action`` [E] (bool, l1 > l0): ``0.97 s + 0.08 tanh(A s) + 0.05 B
    asign`` with the kernel's fp32 constants.  The bound is
    rollout_oracle's, with no incoming state error."""
    s = np.asarray(s, dtype=np.float32).astype(np.float64)
    A = np.asarray(env_A, dtype=np.float32).astype(np.float64)
    B = np.asarray(env_B, dtype=np.float32).astype(np.float64)
    asign = np.where(np.asarray(action, bool), 1.0, -1.0)
    ts = A[None, :, :] * s[:, None, :]
    drive_err = OBS * U * np.abs(ts).sum(-1)
    p97 = C097 * s
    inner = C008 * np.tanh(ts.sum(-1)) + p97
    c05b = C005 * B
    snew = inner + c05b * asign[:, None]
    tol = (C008 * (EPS_TANH + drive_err)
           + U * (np.abs(p97) + np.abs(inner) + np.abs(c05b) + np.abs(snew)))
    return snew, tol


Rollout = collections.namedtuple("Rollout", [
    "s",        # [steps + 1][E][4]   env state, s[0] = s0
    "h",        # [steps + 1][E][64]  carried hidden state, h[0] = 0
    "x",        # [steps][E][4]       what the policy saw at step t
    "x_raw",    # [steps][E][4]       normalised obs before mask and clamp
    "pre",      # [steps][3][E][64]   gate pre-activations a_r, a_z, a_n
    "logits",   # [steps][E][2]
    "tol_l",    # [steps][E][2]       cell's logits tolerance at step t
    "action"])  # [steps][E]          l1 > l0


def rollout(pol, obs_mu, obs_nu, obs_mask, env_A, env_B, s0, steps):
    """``observe -> cell -> env_step`` chained for ``steps`` steps from the
    state ``s0`` [E][4] and a zero hidden state.  The state and the hidden
    state are rounded to fp32 between steps, as the kernel holds them.

    This serves only to choose test inputs and to state conditions about
    them on the CPU (how many steps are decided, where the clamp fires,
    how far the gates saturate).  Its tolerances are those of one step:
    nothing here bounds the kernel over several steps, and no comparison
    with the kernel goes through it."""
    mu = np.asarray(obs_mu, dtype=np.float32).astype(np.float64)
    nu = np.asarray(obs_nu, dtype=np.float32).astype(np.float64)
    s = np.asarray(s0, dtype=np.float32)
    h = np.zeros((s.shape[0], HID), dtype=np.float32)
    out = {k: [] for k in Rollout._fields}
    out["s"].append(s)
    out["h"].append(h)
    for _t in range(steps):
        x, x_slack = observe(s, mu, nu, obs_mask)
        hn, logits, _tol_h, tol_l, pre = cell(pol, x, h, x_slack,
                                              with_pre=True)
        action = logits[:, 1] > logits[:, 0]
        s = env_step(s, action, env_A, env_B)[0].astype(np.float32)
        h = hn.astype(np.float32)
        out["x"].append(x)
        out["x_raw"].append(
            (out["s"][-1].astype(np.float64) - mu) / np.sqrt(nu + C1EM4))
        out["pre"].append(np.stack(pre))
        out["logits"].append(logits)
        out["tol_l"].append(tol_l)
        out["action"].append(action)
        out["s"].append(s)
        out["h"].append(h)
    return Rollout(*(np.stack(out[k]) if out[k] else np.zeros((0,))
                     for k in Rollout._fields))
