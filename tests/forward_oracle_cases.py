"""Inputs, the criterion and the fp32 emulation shared by
tests/test_forward_oracle.py (CPU) and tests/gpu/test_forward_oracle_gpu.py.
Everything here runs without a GPU and is never modified by a test."""

import functools

import numpy as np
import torch

from fiber_amd.es import engine as es_engine
from fiber_amd.es import forward_oracle as fo
from fiber_amd.es import rollout_oracle as oracle

NPARAMS, OBS, HID, ACT, TILE = oracle.NPARAMS, 4, 64, 2, 64

BATCHES = (1, 63, 64, 65, 128, 129, 192)
N_ROWS = max(BATCHES)
GUARD_ROWS = TILE

# one parameter on each side of every boundary of the store_param index map
# (W1 | b1 | W2 | b2 | W3 | b3, and the rows inside W1, W2, W3)
BOUNDARY_J = (0, 3, 4, 255, 256, 319, 320, 383, 384, 4415, 4416, 4479, 4480,
              4543, 4544, 4607, 4608, 4609)


def _randn(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(
        np.float32)


@functools.lru_cache(maxsize=None)
def thetas():
    """name -> float32 [NPARAMS], in a fixed order."""
    out = {
        "init11": es_engine.init_theta(11, "cpu").numpy().copy(),
        "asym0.2": _randn(21, NPARAMS) * np.float32(0.2),
        "saturating4.0": _randn(22, NPARAMS) * np.float32(4.0),
    }
    base = _randn(23, NPARAMS) * np.float32(0.2)
    for j in BOUNDARY_J:
        th = base.copy()
        th[j] += np.float32(1.0)
        out["boundary%d" % j] = th
    return out


SATURATING = ("saturating4.0",)


def _midpoints():
    """fp32 values exactly half way between two neighbouring bf16 values:
    the ties of the input rounding, in several binades and both signs."""
    lo = np.array([1.0, 1.0 + 2.0 ** -7, 0.5, 0.75, 3.0, 0.0078125,
                   2.0 - 2.0 ** -7, 96.0], dtype=np.float64)
    _r, _d, q = oracle.bf16_round(lo)
    mid = (lo + q / 2.0).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), lo + q / 2.0)
    return np.concatenate([mid, -mid])


@functools.lru_cache(maxsize=None)
def pool():
    """float32 [N_ROWS][4]: randn rows with special rows (0, -0.0, fp32
    denormals, +-100, bf16 midpoints) spread so that every tile position
    class and every batch of ``rows_for`` meets some."""
    x = _randn(31, N_ROWS, OBS)
    mid = _midpoints()
    den = np.array([1e-40, -1e-40, 2.0 ** -149, -3e-39], dtype=np.float32)
    special = [
        np.zeros(4, np.float32),
        np.full(4, -0.0, np.float32),
        den,
        np.array([0.0, -0.0, 1e-40, 1.0], np.float32),
        np.array([100.0, -100.0, 100.0, -100.0], np.float32),
        np.array([-100.0, 0.5, 100.0, -0.25], np.float32),
    ] + [mid[i:i + 4] for i in range(0, mid.size, 4)]
    for i, row in enumerate(special):
        for start in (0, 60, 120, 180):
            x[(start + i) % N_ROWS] = row
    # a few single special entries inside ordinary rows
    x[20, 1], x[85, 3], x[150, 0], x[175, 2] = 0.0, mid[0], 100.0, den[0]
    return x


def rows_for(batch):
    """The pool rows that batch ``batch`` holds, in order: a different
    window for every batch, so a row meets several tile positions."""
    return (np.arange(batch) + 37 * batch) % N_ROWS


def x_for(batch):
    return np.ascontiguousarray(pool()[rows_for(batch)])


def cases():
    """Every (theta name, batch)."""
    return [(name, b) for name in thetas() for b in BATCHES]


# ---- the criterion ----------------------------------------------------------

def check_logits(got, theta, x):
    """Largest ``|got - oracle| / tol`` over the [batch][2] logits; the
    comparison passes iff it is at most 1.  A non-finite ``got`` gives
    inf.  The oracle's logits and tolerance are those of ``fo.resolve``:
    the flagged roundings are resolved against ``got`` and the tolerance is
    the fp32 term.  Output outside the envelope of ``fo.forward`` (the fp32
    term plus a whole spacing for every flagged value) fits no choice of
    roundings and is rejected at once, with its ratio to the envelope."""
    ref = fo.forward(theta, x)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.logits.shape, (got.shape, ref.logits.shape)
    if not np.isfinite(got).all():
        return float("inf")
    envelope = float((np.abs(got - ref.logits) / ref.tol).max())
    if envelope > 1.0:
        return envelope
    return float(fo.resolve(theta, x, got, ref=ref).ratio.max())


def guard_rows_untouched(out, batch):
    """``out`` [batch + GUARD_ROWS][2] as filled by ``emulate``: rows past
    ``batch`` still hold the not-written mark."""
    return bool(np.isnan(out[batch:]).all())


# ---- fp32 emulation of the kernel ------------------------------------------

def _bf(v):
    """fp32 -> bf16 -> fp32 by torch's conversion (nearest, ties to even),
    independent of the oracle's bf16_round."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def _fast_tanh(x):
    """fast_tanh in fp32, as measure_tanh_emulation_error emulates it: one
    rounding per operation, exp2 and the reciprocal correctly rounded."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        m = x * np.float32(oracle.TWO_LOG2E)
        e = np.exp2(m.astype(np.float64)).astype(np.float32)
        ep1 = e + np.float32(1.0)
        r = (1.0 / ep1.astype(np.float64)).astype(np.float32)
        return (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)


def _matmul_f32(act, w):
    """out[b][o] = sum_k act[b][k] * w[o][k], fp32 adds in k order.  The
    bf16 x bf16 products are exact in fp32."""
    acc = np.zeros((act.shape[0], w.shape[0]), np.float32)
    for k in range(act.shape[1]):
        acc = acc + act[:, k, None] * w[None, :, k]
    return acc


SLIPS = (
    "w1_transposed", "w2_transposed", "b1_shifted", "b2_shifted",
    "w3_rows_swapped", "b3_swapped", "biases_bf16", "x_not_rounded",
    "h1_not_rounded", "h2_not_rounded", "kslots_4to7_nonzero",
    "row_xor16", "tile1_reads_tile0", "tail_reads_row_batch",
)


def emulate(theta, x, slip=None):
    """``mlp_policy_forward`` in numpy float32: the kernel's roundings, fp32
    adds and fast_tanh, tile by tile.  Returns float32 ``[batch +
    GUARD_ROWS][2]``, the rows the kernel does not write holding NaN.

    ``slip`` names one mistake (SLIPS).  Two of them need a word:

    * ``kslots_4to7_nonzero``: both layer-1 operands carry 8 k-slots of
      which 4..7 are zero-filled.  A non-zero in those slots of ``x`` alone
      meets the zeros of W1 and changes nothing, so the slip drops both
      fills: the slots hold what a 4-float row stride leaves there, the
      next row's values.
    * ``tail_reads_row_batch``: the row guard compares ``<=``.  Rows past
      ``batch`` feed only their own outputs, so reading row ``batch`` shows
      in no logit of a valid row; what shows is that its logits are stored,
      in the first guard row.
    """
    assert slip is None or slip in SLIPS, slip
    theta = np.asarray(theta, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    batch = x.shape[0]
    w1 = theta[:256].reshape(HID, OBS)
    b1 = theta[256:320]
    w2 = theta[320:4416].reshape(HID, HID)
    b2 = theta[4416:4480]
    w3 = theta[4480:4608].reshape(ACT, HID)
    b3 = theta[4608:4610]
    if slip == "w1_transposed":
        w1 = theta[:256].reshape(OBS, HID).T
    if slip == "w2_transposed":
        w2 = w2.T
    if slip == "b1_shifted":
        b1 = np.roll(b1, 1)
    if slip == "b2_shifted":
        b2 = np.roll(b2, 1)
    if slip == "w3_rows_swapped":
        w3 = w3[::-1]
    if slip == "b3_swapped":
        b3 = b3[::-1]
    if slip == "biases_bf16":
        b1, b2, b3 = _bf(b1), _bf(b2), _bf(b3)
    w1p = np.zeros((HID, 8), np.float32)
    w1p[:, :OBS] = _bf(w1)
    if slip == "kslots_4to7_nonzero":
        w1p[:-1, OBS:] = w1p[1:, :OBS]
    w2b, w3b = _bf(w2), _bf(w3)

    # what lies behind x in memory, for the slips that read past a row
    x_mem = np.concatenate([x, np.ones((1, OBS), np.float32)])
    n_valid = batch + 1 if slip == "tail_reads_row_batch" else batch
    out = np.full((batch + GUARD_ROWS, ACT), np.nan, np.float32)
    for row0 in range(0, batch, TILE):
        rows = row0 + np.arange(TILE)
        src = rows.copy()
        if slip == "row_xor16":
            src = row0 + (np.arange(TILE) ^ 16)
        if slip == "tile1_reads_tile0" and row0 == TILE:
            src = rows - TILE
        xt = np.zeros((TILE, 8), np.float32)
        ok = src < n_valid
        xt[ok, :OBS] = x_mem[src[ok]]
        if slip == "kslots_4to7_nonzero":
            nxt = ok & (src + 1 < batch)
            xt[nxt, OBS:] = x_mem[src[nxt] + 1]
        if slip != "x_not_rounded":
            xt = _bf(xt)
        h1 = _fast_tanh(_matmul_f32(xt, w1p) + b1)
        if slip != "h1_not_rounded":
            h1 = _bf(h1)
        h2 = _fast_tanh(_matmul_f32(h1, w2b) + b2)
        if slip != "h2_not_rounded":
            h2 = _bf(h2)
        logit = np.broadcast_to(b3, (TILE, ACT)).astype(np.float32)
        for i in range(HID):
            # the product is exact in float64; one rounding, fused or not
            logit = (logit.astype(np.float64)
                     + h2[:, i, None].astype(np.float64)
                     * w3b[None, :, i].astype(np.float64)).astype(np.float32)
        stored = rows < n_valid
        out[rows[stored]] = logit[stored]
    return out


def accepts(out, theta, x):
    """The two things the GPU test asserts of the kernel's output buffer:
    the criterion on the leading rows, and untouched guard rows.  Returns
    (accepted, worst ratio)."""
    batch = np.asarray(x).shape[0]
    ratio = check_logits(out[:batch], theta, x)
    return ratio <= 1.0 and guard_rows_untouched(out, batch), ratio


# ---- the MFMA probe -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def probe_inputs():
    """name -> (a, b) float32 [64][64]: asymmetric random, and the
    identity."""
    return {
        "random": (_randn(41, HID, HID) * np.float32(0.3),
                   _randn(42, HID, HID) * np.float32(0.3)),
        "identity": (np.eye(HID, dtype=np.float32),
                     _randn(43, HID, HID) * np.float32(0.2)),
    }


def emulate_probe(a, b):
    """mfma_gemm64_probe in fp32: bf16(fast_tanh(bf16(a) @ bf16(b)))."""
    return _bf(_fast_tanh(_matmul_f32(_bf(a), _bf(b).T)))


# the transpositions tests/gpu/test_ops.py lists as diagnoses
PROBE_TRANSPOSITIONS = {
    "A.T@B": lambda a, b: emulate_probe(a.T, b),
    "A@B.T": lambda a, b: emulate_probe(a, b.T),
    "(A@B).T": lambda a, b: emulate_probe(a, b).T,
    "B@A": lambda a, b: emulate_probe(b, a),
}


# ---- serve what was trained ---------------------------------------------------

SERVE_SEED, SERVE_ITER, SERVE_H = 1234, 5, 8
SERVE_MU = np.array([0.05, -0.03, 0.02, -0.1], dtype=np.float32)
SERVE_NU = np.full(4, 0.5, dtype=np.float32)
SERVE_PAIRS = ((11, 100), (12, 101), (13, 102))   # (theta seed, env seed)
SERVE_MIN_SHARE = 0.80


@functools.lru_cache(maxsize=None)
def serve_case(i):
    """(theta float32, rollout, compared [64][8], band [64][8]) for pair i.
    ``compared``: steps at which the serving kernel must take the oracle's
    action; ``band``: steps the rollout oracle decides on their own but
    where rounding h2 may turn the action."""
    tseed, eseed = SERVE_PAIRS[i]
    theta = es_engine.init_theta(tseed, "cpu").numpy().copy()
    env_A, env_B = es_engine.make_env_params(eseed, "cpu")
    ro = oracle.eval_cell(theta, SERVE_MU, SERVE_NU, env_A.numpy(),
                          env_B.numpy(), SERVE_SEED, SERVE_ITER, SERVE_H)
    extra = oracle.SAFETY * fo.h2_rounding_margin(ro.policy, ro.h1)
    # per step, not cumulative: the states are given to the kernel
    own = ~ro.x_flag & (ro.margin > ro.threshold)
    compared = ~ro.x_flag & (ro.margin > ro.threshold + extra)
    return theta, ro, compared, own & ~compared
