"""Thetas, probes, the case list and an fp32 emulation of ``sm_steps`` with
seeded slips, shared by tests/test_safe_ga.py (CPU) and
tests/gpu/test_safe_ga_gpu.py.  Everything here runs without a GPU, is
computed once per process and is never modified by a test."""

import functools
import itertools

import numpy as np

import forward_oracle_cases as FC
from fiber_amd.es import engine as es_engine
from fiber_amd.es import safe_ga
from fiber_amd.es import sm_oracle

NPARAMS, OBS, HID, ACT, BATCH = 4610, 4, 64, 2, 64
OFF_B1, OFF_W2, OFF_B2, OFF_W3, OFF_B3 = 256, 320, 4416, 4480, 4608

SEED = 1234
SIGMA = 0.002
MODES = ("abs", "sum")
S_MINS = (0.01, 1e-6)
ROW_COUNTS = (1, 3)

# pre-activations this far out round to +-1 in bf16 whatever the fp32 error
# of the kernel's tanh: 1 - tanh(6) = 1.2e-5 against half a spacing of 2e-3
SATURATED_PRE = 6.0


def _randn(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(
        np.float32)


def _layers(seed, s_w1, s_b1, s_w2, s_b2, s_w3, s_b3):
    """A random theta with its own scale per layer and nonzero biases:
    nothing in it is symmetric."""
    th = _randn(seed, NPARAMS)
    th[:OFF_B1] *= np.float32(s_w1)
    th[OFF_B1:OFF_W2] *= np.float32(s_b1)
    th[OFF_W2:OFF_B2] *= np.float32(s_w2)
    th[OFF_B2:OFF_W3] *= np.float32(s_b2)
    th[OFF_W3:OFF_B3] *= np.float32(s_w3)
    th[OFF_B3:] *= np.float32(s_b3)
    return th


@functools.lru_cache(maxsize=None)
def probes():
    """name -> float32 [64][4]."""
    default = safe_ga.default_probe(SEED)
    special = np.clip(_randn(51, BATCH, OBS) * np.float32(1.5), -5.0, 5.0)
    special[0] = 0.0
    special[1] = np.float32([5.0, -5.0, 5.0, -5.0])
    mid = FC._midpoints()
    mid = mid[np.abs(mid) <= 5.0]               # bf16 ties inside the clip
    for i, v in enumerate(mid):
        special[2 + i // OBS, i % OBS] = v
    out = {"default": default, "special": special.astype(np.float32)}
    for p in out.values():
        p.setflags(write=False)
    return out


def _saturating(base, probe):
    """``base`` with W1 x 100, every W1 row redrawn until all 64 layer-1
    pre-activations on ``probe`` lie beyond SATURATED_PRE, so that every
    h1 is exactly +-1 in bf16."""
    th = base.copy()
    xq = FC._bf(np.array(probe)).astype(np.float64)
    rng = np.random.default_rng(61)
    for j in range(HID):
        for _ in range(10000):
            w = (rng.standard_normal(OBS) * 50.0).astype(np.float32)
            pre = xq @ FC._bf(w).astype(np.float64) + float(th[OFF_B1 + j])
            if np.abs(pre).min() > SATURATED_PRE:
                break
        else:
            raise AssertionError("no saturating row for unit %d" % j)
        th[j * OBS:(j + 1) * OBS] = w
    return th


@functools.lru_cache(maxsize=None)
def thetas():
    """name -> float32 [NPARAMS], in a fixed order."""
    asym_a = _layers(71, 0.8, 0.3, 0.25, 0.2, 0.5, 0.4)
    out = {
        "init1234": es_engine.init_theta(SEED, "cpu").numpy().copy(),
        "asymA": asym_a,
        "asymB": _layers(72, 0.3, 0.6, 0.12, 0.4, 1.5, 0.1),
        "zero": np.zeros(NPARAMS, np.float32),
        "saturating": _saturating(asym_a, probes()["default"]),
        "asym0.2": FC.thetas()["asym0.2"].copy(),
    }
    for th in out.values():
        th.setflags(write=False)
    return out


def cases():
    """Every (theta, probe, mode, s_min)."""
    return list(itertools.product(thetas(), probes(), MODES, S_MINS))


@functools.lru_cache(maxsize=None)
def reference(theta_name, probe_name, mode, s_min):
    """The oracle of one case, computed once."""
    return sm_oracle.steps(thetas()[theta_name], probes()[probe_name], SIGMA,
                           s_min, mode)


def worst_ratio(got_steps, got_sens, ref):
    """Largest |got - oracle| / tol over the steps and the sensitivities of
    one row; inf for a non-finite value.  Accepted iff <= 1."""
    worst = 0.0
    for got, want, tol in ((got_steps, ref.steps, ref.tol_steps),
                           (got_sens, ref.sens, ref.tol_sens)):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape, (got.shape, want.shape)
        if not np.isfinite(got).all():
            return float("inf")
        worst = max(worst, float((np.abs(got - want) / tol).max()))
    return worst


# ---- fp32 emulation of the kernel ------------------------------------------

SLIPS = (
    "dW2_transposed",            # a transposed operand of the d2^T h1 GEMM
    "no_s2", "no_s1",            # a missing (1 - h^2)
    "abs_backprop",              # |d2| back-propagated instead of d2
    "abs_forgotten",             # abs mode reduces signed values
    "outputs_summed",            # |m0 + m1| instead of sqrt(m0^2 + m1^2)
    "sum_not_mean",
    "floor_after_division",
    "w3_row0_for_both",          # both outputs back-propagate W3 row 0
    "w3_transposed_layout",      # W3 read as [64][2]
)
# sens is symmetric in the two outputs, so exchanging the W3 rows as a whole
# exchanges m0 and m1 and changes nothing: no criterion on sens can see it
# (tests/test_safe_ga.py shows the equality).  The two W3 slips above are the
# ones that can be seen.
INVISIBLE_SLIPS = ("w3_rows_swapped",)


def _seq_sum(a):
    """Column sums of a[b][n] in fp32, b in order."""
    acc = np.zeros(a.shape[1], np.float32)
    for b in range(a.shape[0]):
        acc = acc + a[b]
    return acc


def _one_minus_sq(h):
    """fmaf(-h, h, 1) in fp32: one rounding."""
    return (1.0 - h.astype(np.float64) ** 2).astype(np.float32)


def emulate(theta, probe, sigma, s_min, mode, slip=None):
    """``sm_steps`` of one row in numpy float32: the kernel's roundings,
    fp32 adds in k order and fast_tanh.  Returns (steps, sens), float32
    [NPARAMS].  ``slip`` names one mistake."""
    assert slip is None or slip in SLIPS + INVISIBLE_SLIPS, slip
    theta = np.array(theta, dtype=np.float32)      # writable copies: the
    probe = np.array(probe, dtype=np.float32)      # cases are read-only
    w1 = theta[:OFF_B1].reshape(HID, OBS)
    b1 = theta[OFF_B1:OFF_W2]
    w2 = theta[OFF_W2:OFF_B2].reshape(HID, HID)
    b2 = theta[OFF_B2:OFF_W3]
    w3 = theta[OFF_W3:OFF_B3].reshape(ACT, HID)
    w1b, w2b, w3b = FC._bf(w1), FC._bf(w2), FC._bf(w3)
    if slip == "w3_rows_swapped":
        w3b = w3b[::-1]
    if slip == "w3_row0_for_both":
        w3b = np.stack([w3b[0], w3b[0]])
    if slip == "w3_transposed_layout":
        w3b = np.ascontiguousarray(w3b.reshape(HID, ACT).T)
    xq = FC._bf(probe)
    h1 = FC._bf(FC._fast_tanh(FC._matmul_f32(xq, w1b) + b1))
    h2 = FC._bf(FC._fast_tanh(FC._matmul_f32(h1, w2b) + b2))
    absolute = mode == "abs" and slip != "abs_forgotten"
    op = np.abs if absolute else (lambda v: v)
    s2, s1 = _one_minus_sq(h2), _one_minus_sq(h1)
    if slip == "no_s2":
        s2 = np.ones_like(s2)
    if slip == "no_s1":
        s1 = np.ones_like(s1)
    inv = np.float32(1.0 if slip == "sum_not_mean" else 1.0 / BATCH)
    m = []
    for k in range(ACT):
        d2 = FC._bf(w3b[k][None, :] * s2)
        back = np.abs(d2) if slip == "abs_backprop" else d2
        P = FC._matmul_f32(back, np.ascontiguousarray(w2b.T))
        d1 = FC._bf(P * s1)
        g_w2 = FC._matmul_f32(np.ascontiguousarray(op(d2).T),
                              np.ascontiguousarray(op(h1).T))
        if slip == "dW2_transposed":
            g_w2 = g_w2.T
        g_w1 = FC._matmul_f32(np.ascontiguousarray(op(d1).T),
                              np.ascontiguousarray(op(xq).T))
        g_w3 = np.zeros((ACT, HID), np.float32)
        g_w3[k] = _seq_sum(op(h2))
        g_b3 = np.zeros(ACT, np.float32)
        g_b3[k] = BATCH
        flat = np.concatenate([
            g_w1.reshape(-1), _seq_sum(op(d1)), g_w2.reshape(-1),
            _seq_sum(op(d2)), g_w3.reshape(-1), g_b3]).astype(np.float32)
        m.append(flat * inv)
    m0, m1 = m
    if slip == "outputs_summed":
        sens = np.abs(m0 + m1)
    else:
        sq = (m1.astype(np.float64) ** 2
              + (m0 * m0).astype(np.float64)).astype(np.float32)
        sens = np.sqrt(sq)
    sigma, s_min = np.float32(sigma), np.float32(s_min)
    with np.errstate(divide="ignore", over="ignore"):
        if slip == "floor_after_division":
            steps = np.maximum(sigma / sens, s_min)
        else:
            steps = sigma / np.maximum(sens, s_min)
    return steps.astype(np.float32), sens.astype(np.float32)
