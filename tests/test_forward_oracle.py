"""CPU checks of the fp64 oracle of the serving forward kernel and the MFMA
probe (fiber_amd/es/forward_oracle.py): the criterion accepts an fp32
emulation of the kernel on every case and rejects every listed slip, and
its tolerance stays tight.  Derivations: profiles/forward_oracle.md."""

import importlib.util
import os

import numpy as np
import pytest
import torch

import forward_oracle_cases as C
from fiber_amd.es import forward_oracle as fo
from fiber_amd.es import rollout_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emulated():
    """(theta name, batch) -> emulation output, slip-free."""
    th = C.thetas()
    return {(name, b): C.emulate(th[name], C.x_for(b))
            for name, b in C.cases()}


def test_oracle_reads_the_kernel_it_claims_to():
    """The rounding points the oracle reproduces are the kernel's."""
    src = open(os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                            "es_kernels.hip")).read()
    fwd = src[src.index("mlp_policy_forward(const float*"):
              src.index("mfma_gemm64_probe(const float*")]
    assert "xb[e][d] = __float2bfloat16(v);" in fwd
    assert "&h2[0][0], wave, lane);" in fwd           # h2 goes through bf16
    assert "float l = pol.b3[a];" in fwd
    assert "for (int h = 0; h < HID; ++h)" in fwd     # a sequential chain
    assert "pk.h[ri] = __float2bfloat16(th[ri]);" in src


def test_inputs_hold_the_edges():
    x = C.pool()
    assert x.shape == (C.N_ROWS, 4) and x.dtype == np.float32
    assert (x == 100.0).any() and (x == -100.0).any()
    assert np.signbit(x[x == 0.0]).any() and (~np.signbit(x[x == 0.0])).any()
    assert ((np.abs(x) < 2.0 ** -126) & (x != 0)).any()
    # exact bf16 ties: the distance to the midpoint is 0
    _r, dist, _q = oracle.bf16_round(x.astype(np.float64))
    assert (dist == 0).sum() >= 16
    # ... which the input rounding resolves to even, like torch
    assert np.array_equal(fo.round_input(x), C._bf(x).astype(np.float64))
    for b in C.BATCHES:
        assert len(set(C.rows_for(b).tolist())) == b
    assert len(C.thetas()) == 3 + len(C.BOUNDARY_J)
    sat = C.thetas()["saturating4.0"]
    assert np.abs(fo.forward(sat, C.x_for(64)).pre2).max() > 30.0


def test_criterion_accepts_the_emulation(emulated):
    th = C.thetas()
    worst = {}
    for (name, b), out in emulated.items():
        ok, ratio = C.accepts(out, th[name], C.x_for(b))
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert ok and ratio < 1.0, (name, b, ratio)
    for name, ratio in worst.items():
        print("emulation vs oracle, %-14s worst |err|/tol = %.3f"
              % (name, ratio))


@pytest.mark.parametrize("slip", C.SLIPS)
def test_criterion_rejects_the_slip(slip, emulated):
    """Every slip is rejected on at least one case; where it changes the
    output at all it is reported how many cases catch it."""
    th = C.thetas()
    rejected, changed, worst = 0, 0, 0.0
    for name, b in C.cases():
        out = C.emulate(th[name], C.x_for(b), slip)
        if np.array_equal(out, emulated[(name, b)], equal_nan=True):
            continue
        changed += 1
        ok, ratio = C.accepts(out, th[name], C.x_for(b))
        rejected += not ok
        worst = max(worst, ratio)
    print("slip %-22s changes %3d cases, rejected on %3d, worst ratio %.3g"
          % (slip, changed, rejected, worst))
    assert rejected >= 1, slip


def test_tolerance_stays_tight(emulated):
    """max(tol) under 1e-3 for every non-saturating theta, tol being the
    tolerance the criterion applies (fo.resolve): the fp32 term, plus the
    whole width of what it does not enumerate.  The envelope of fo.forward,
    which charges every flagged value a whole bf16 spacing, is printed
    beside it: one flagged h2 in [0.5, 1) costs 2^-8 |w3| = 3.9e-3 |w3|, so
    the envelope cannot stay under 1e-3 and is not what decides."""
    th = C.thetas()
    x = C.pool()
    for name, theta in th.items():
        ref = fo.forward(theta, x)
        got = C.emulate(theta, x)[:C.N_ROWS]
        res = fo.resolve(theta, x, got, ref=ref)
        flagged = (ref.h1_flag.sum(-1) + ref.h2_flag.sum(-1)).mean()
        print("%-14s max tol %.3e (envelope %.3e, its fp32 term %.3e), "
              "flagged h1/h2 per row %.1f, emulation worst ratio %.3f, "
              "rows resolved by a flip %d"
              % (name, res.tol.max(), ref.tol.max(), ref.tol_fp32.max(),
                 flagged, res.ratio.max(), int((res.flipped > 0).sum())))
        assert (res.tol > 0).all() and np.isfinite(res.tol).all()
        assert np.array_equal(ref.tol, ref.tol_fp32 + ref.tol_flip)
        assert (res.tol <= ref.tol * (1 + 1e-12)).all()
        assert res.ratio.max() <= 1.0
        if name not in C.SATURATING:
            assert res.tol.max() < 1e-3, (name, res.tol.max())
            assert ref.tol_fp32.max() < 1e-3


def test_resolve_finds_the_roundings_and_nothing_else():
    """Logits built from a known choice of other-way roundings are accepted
    with those roundings found; the same logits moved by 3 fp32 terms are
    rejected although they lie inside the envelope."""
    theta = C.thetas()["asym0.2"]
    x = C.pool()
    ref = fo.forward(theta, x)
    pol = oracle.make_policy(theta)
    rng = np.random.default_rng(3)
    take = ref.h2_flag & (rng.random(ref.h2_flag.shape) < 0.5)
    # only single-spacing flags are enumerated
    _r, _d, q = oracle.bf16_round(ref.h2)
    take &= np.abs(ref.h2_alt - ref.h2) <= q
    # in rows without a flagged h1: with h1 as it is, an h2 that only a
    # moved h1 could carry across its midpoint is rightly not permitted
    take &= ~ref.h1_flag.any(-1)[:, None]
    h2 = np.where(take, ref.h2_alt, ref.h2)
    got = h2 @ pol.w3.T + pol.b3
    res = fo.resolve(theta, x, got, ref=ref)
    assert take.any(-1).sum() > 30
    # exact but for the flagged values next to 0, finer than EPS_TANH, whose
    # move is not enumerated and stays, a few percent, in the tolerance
    assert res.ratio.max() < 0.1, res.ratio.max()
    assert np.median(res.ratio[take.any(-1)]) < 1e-9
    moved = (np.abs(got - ref.logits) > ref.tol_fp32).any(-1)
    assert moved.sum() >= 20 and (res.flipped[moved] > 0).all()
    # off by 3 fp32 terms in one logit
    off = got.copy()
    off[:, 0] += 3.0 * ref.tol_fp32[:, 0]
    inside = (np.abs(off - ref.logits) <= ref.tol).all(-1)
    res = fo.resolve(theta, x, off, ref=ref)
    print("rows inside the envelope %d, of which rejected %d"
          % (int(inside.sum()), int((res.ratio[inside] > 1).sum())))
    assert inside.sum() > 50
    # not all: among 2^8 subset sums some land 3 fp32 terms away
    assert (res.ratio[inside] > 1).mean() > 0.5


def test_flagged_values_sit_at_midpoints_and_alt_is_the_neighbour():
    ref = fo.forward(C.thetas()["asym0.2"], C.pool())
    for h, alt in ((ref.h1, ref.h1_alt), (ref.h2, ref.h2_alt)):
        _r, _d, q = oracle.bf16_round(h)
        gap = np.abs(alt - h)
        # one spacing of the binade of h, or of the one below it
        assert ((gap == q) | (gap == q / 2)).all()
        assert np.array_equal(oracle.bf16_round(alt)[0], alt)
    # moving the flagged h2 to their other neighbour stays inside tol
    pol = oracle.make_policy(C.thetas()["asym0.2"])
    h2 = np.where(ref.h2_flag, ref.h2_alt, ref.h2)
    moved = h2 @ pol.w3.T + pol.b3
    assert ref.h2_flag.any()
    assert (np.abs(moved - ref.logits) <= ref.tol).all()


def test_probe_reference_accepts_emulation_and_rejects_transpositions():
    for name, (a, b) in C.probe_inputs().items():
        ref = fo.probe_reference(a, b)
        bad = fo.probe_mismatches(C.emulate_probe(a, b), ref)
        print("probe %-8s flagged %d of 4096, emulation mismatches %d"
              % (name, int(ref.flag.sum()), len(bad)))
        assert len(bad) == 0, (name, bad[:8])
        # where the width is under a spacing the range is value (and alt)
        narrow = ~ref.flag
        assert np.array_equal(ref.lo[narrow], ref.value[narrow])
        assert np.array_equal(ref.hi[narrow], ref.value[narrow])
    a, b = C.probe_inputs()["random"]
    ref = fo.probe_reference(a, b)
    for name, variant in C.PROBE_TRANSPOSITIONS.items():
        bad = fo.probe_mismatches(variant(a, b), ref)
        print("probe transposition %-8s mismatches %d" % (name, len(bad)))
        assert len(bad) > 2048, name


def test_serve_cases_compare_enough_steps():
    """The coverage the GPU test asserts, from the oracle alone."""
    for i in range(len(C.SERVE_PAIRS)):
        _theta, ro, compared, band = C.serve_case(i)
        assert compared.shape == (64, C.SERVE_H)
        print("serve pair %d: compared %.1f%% of 512 steps, band %d steps, "
              "decided through 8 (cumulative) %.1f%%"
              % (i, 100.0 * compared.mean(), int(band.sum()),
                 100.0 * ro.decided.mean()))
        assert compared.mean() >= C.SERVE_MIN_SHARE
        assert not (compared & band).any()
        # both actions occur among the compared steps
        assert ro.action[compared].any() and (~ro.action[compared]).any()


def _load_serve_example():
    spec = importlib.util.spec_from_file_location(
        "_serve_policy_example", os.path.join(ROOT, "examples",
                                              "serve_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_serve_example_refuses_malformed_obs_without_fastapi():
    serve = _load_serve_example()
    good = serve.parse_obs([[0.1, -0.2, 0.05, 0.0], [1, 2, 3, 4]])
    assert good.dtype == torch.float32 and tuple(good.shape) == (2, 4)
    assert good.is_contiguous()
    assert tuple(serve.parse_obs([]).shape) == (0, 4)
    for bad in ([[1, 2, 3]], [1.0, 2.0, 3.0, 4.0], [[1, 2, 3, 4], [1, 2]],
                [[[1, 2, 3, 4]]], "abcd", [["a", "b", "c", "d"]], None, 3.5,
                [[1, 2, 3, 4, 5]], {"a": 1}, [[None, 1, 2, 3]]):
        with pytest.raises(ValueError):
            serve.parse_obs(bad)
    with pytest.raises(ValueError):
        serve.parse_obs([[0.0] * 4] * (serve.MAX_BATCH + 1))
