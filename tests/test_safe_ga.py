"""Host tests of the safe-mutation oracle (fiber_amd/es/sm_oracle.py), of the
shared cases of tests/sm_cases.py and of the validation that the ops wrappers
and SafeGAEngine do before any launch.  No GPU.

The oracle is anchored against ``torch.autograd`` in float64:

* with every bf16 rounding off it is the Jacobian of the plain fp64 MLP, to
  1e-10, in both modes;
* the forward's roundings are not an error of the backward, they fix the
  point at which the kernel takes its derivative: ``tanh'`` is ``1 - c^2``
  with ``c`` the *rounded* activation.  ``_act`` builds exactly that network
  (value ``c``, slope ``1 - c^2``), and the oracle with the forward's
  roundings alone is its Jacobian to 1e-10;
* with all roundings on, the oracle differs from that Jacobian only by the
  two bf16 roundings of the backward, and by no more than the bound it
  derives for them itself (``round_sens``, ``round_steps``).
"""

import numpy as np
import pytest
import torch

import sm_cases as C
from fiber_amd import ops
from fiber_amd.es import safe_ga
from fiber_amd.es import sm_oracle


# ---- the oracle against autograd -------------------------------------------

def _act(pre, c):
    """tanh, or the kernel's view of it at a rounded activation ``c``: the
    value ``c`` and the slope ``1 - c^2``."""
    if c is None:
        return torch.tanh(pre)
    return c + (1.0 - c * c) * (pre - pre.detach())


def _autograd_means(fw, mode, at_rounded_point):
    """m[2][NPARAMS] by 128 backward passes of the fp64 MLP with the
    weights and inputs of ``fw``."""
    params = [torch.tensor(np.asarray(a), dtype=torch.float64,
                           requires_grad=True)
              for a in (fw.w1, fw.b1, fw.w2, fw.b2, fw.w3, fw.b3)]
    w1, b1, w2, b2, w3, b3 = params
    x = torch.tensor(fw.x, dtype=torch.float64)
    c1 = torch.tensor(fw.h1) if at_rounded_point else None
    c2 = torch.tensor(fw.h2) if at_rounded_point else None
    m = torch.zeros(2, C.NPARAMS, dtype=torch.float64)
    for b in range(C.BATCH):
        h1 = _act(w1 @ x[b] + b1, None if c1 is None else c1[b])
        h2 = _act(w2 @ h1 + b2, None if c2 is None else c2[b])
        logits = w3 @ h2 + b3
        for k in range(2):
            g = torch.autograd.grad(logits[k], params, retain_graph=True)
            flat = torch.cat([t.reshape(-1) for t in g])
            m[k] += flat.abs() if mode == "abs" else flat
    return (m / C.BATCH).numpy()


ANCHOR = [(t, p, mode) for t in ("init1234", "asymA", "asymB")
          for p in C.probes() for mode in C.MODES]


@pytest.mark.parametrize("theta,probe,mode", ANCHOR)
def test_oracle_is_autograds_jacobian(theta, probe, mode):
    th, x = C.thetas()[theta], C.probes()[probe]
    s_min = 1e-6
    plain = sm_oracle.steps(th, x, C.SIGMA, s_min, mode, rounding="none")
    want = _autograd_means(plain.forward, mode, at_rounded_point=False)
    assert np.abs(plain.m - want).max() <= 1e-10
    assert np.abs(plain.sens - np.hypot(want[0], want[1])).max() <= 1e-10
    assert (plain.tol_sens == 0).all() and (plain.round_sens == 0).all()

    fwd = sm_oracle.steps(th, x, C.SIGMA, s_min, mode, rounding="forward")
    want = _autograd_means(fwd.forward, mode, at_rounded_point=True)
    assert np.abs(fwd.m - want).max() <= 1e-10
    want_sens = np.hypot(want[0], want[1])

    full = sm_oracle.steps(th, x, C.SIGMA, s_min, mode)
    diff = np.abs(full.sens - want_sens)
    assert diff.max() > 0                          # the roundings are there
    assert (diff <= full.round_sens + 1e-12).all()
    want_steps = full.steps * 0 + float(np.float32(C.SIGMA)) / np.maximum(
        want_sens, float(np.float32(s_min)))
    assert (np.abs(full.steps - want_steps)
            <= full.round_steps * (1 + 1e-9) + 1e-12).all()
    # the rounded model is the plain one to bf16 accuracy only, which is
    # why the plain Jacobian is not what the kernel is held to
    rel = np.abs(full.sens - plain.sens) / np.maximum(plain.sens, 1e-3)
    assert rel.max() > 1e-6


def test_b3_is_exactly_one_and_the_other_w3_row_gets_nothing():
    for mode in C.MODES:
        ref = C.reference("asymA", "default", mode, 0.01)
        assert (ref.sens[C.OFF_B3:] == 1.0).all()
        assert (ref.steps[C.OFF_B3:] == float(np.float32(C.SIGMA))).all()
        assert (ref.tol_m[:, C.OFF_B3:] == 0).all()
        assert (ref.m[0, C.OFF_W3 + C.HID:C.OFF_B3] == 0).all()
        assert (ref.m[1, C.OFF_W3:C.OFF_W3 + C.HID] == 0).all()
    ref = C.reference("asymA", "default", "sum", 0.01)
    assert np.array_equal(ref.sens[C.OFF_W3:C.OFF_W3 + C.HID],
                          ref.sens[C.OFF_W3 + C.HID:C.OFF_B3])


# ---- the shared cases ---------------------------------------------------------

def test_cases_are_what_they_say():
    thetas, probes = C.thetas(), C.probes()
    assert len(C.cases()) == len(thetas) * len(probes) * 4
    x = probes["default"]
    assert x.shape == (64, 4) and x.dtype == np.float32
    assert np.abs(x).max() <= 5.0 and np.isfinite(x).all()
    assert np.array_equal(x, safe_ga.default_probe(C.SEED))
    assert not np.array_equal(x, safe_ga.default_probe(C.SEED + 1))
    assert 0.7 < x.std() < 1.3 and abs(x.mean()) < 0.2
    sp = probes["special"]
    assert (sp[0] == 0).all() and (np.abs(sp[1]) == 5.0).all()
    mid = C.FC._midpoints()
    assert np.isin(sp[2:6].reshape(-1), mid).sum() >= 8
    # the saturating theta: every h1 is exactly +-1 on the default probe,
    # so nothing flows into W1 and b1
    ref = C.reference("saturating", "default", "abs", 0.01)
    assert (np.abs(ref.forward.h1) == 1.0).all()
    assert (ref.forward.h1_off == 0).all()
    assert (ref.sens[:C.OFF_W2] == 0).all()
    assert len(np.unique(ref.forward.h1, axis=0)) > 8   # the signs vary
    zero = C.reference("zero", "special", "abs", 0.01)
    assert (zero.sens[:C.OFF_B3] == 0).all()


@pytest.mark.parametrize("theta,probe,mode,s_min", C.cases())
def test_emulation_is_accepted(theta, probe, mode, s_min):
    """An fp32 reading of the kernel, independent of the oracle's code,
    lands inside the oracle's tolerance on every case."""
    ref = C.reference(theta, probe, mode, s_min)
    steps, sens = C.emulate(C.thetas()[theta], C.probes()[probe], C.SIGMA,
                            s_min, mode)
    assert C.worst_ratio(steps, sens, ref) <= 1.0


@pytest.mark.parametrize("slip", C.SLIPS)
def test_every_slip_is_rejected_on_some_case(slip):
    rejected = []
    for theta in ("asymA", "asymB", "init1234"):
        for probe in C.probes():
            for mode in C.MODES:
                ref = C.reference(theta, probe, mode, 0.01)
                steps, sens = C.emulate(C.thetas()[theta], C.probes()[probe],
                                        C.SIGMA, 0.01, mode, slip=slip)
                if C.worst_ratio(steps, sens, ref) > 1.0:
                    rejected.append((theta, probe, mode))
    print("%s rejected on %d of 12" % (slip, len(rejected)))
    assert rejected, slip


def test_a_swap_of_the_w3_rows_cannot_be_seen_in_sens():
    """The one slip of the list that no criterion on sens or steps can
    reject: exchanging the W3 rows exchanges m0 and m1, and sens is their
    2-norm.  The emulation with the swap lands inside the tolerance."""
    th, x = C.thetas()["asymA"], C.probes()["default"]
    for mode in C.MODES:
        ref = C.reference("asymA", "default", mode, 0.01)
        steps, sens = C.emulate(th, x, C.SIGMA, 0.01, mode,
                                slip="w3_rows_swapped")
        assert C.worst_ratio(steps, sens, ref) <= 1.0


def test_tolerance_is_rounding_sized():
    """Worst tol / sens over the elements above s_min, per mode, over the
    non-degenerate cases (recorded in profiles/safe_mutation.md)."""
    for mode in C.MODES:
        worst = 0.0
        for theta in ("init1234", "asymA", "asymB", "asym0.2"):
            for probe in C.probes():
                ref = C.reference(theta, probe, mode, 0.01)
                live = ref.sens > 0.01
                worst = max(worst, float((ref.tol_sens[live]
                                          / ref.sens[live]).max()))
        print("mode %s: worst tol / sens above s_min = %.3e" % (mode, worst))
        assert worst < (0.02 if mode == "abs" else 0.2)


# ---- config, wrappers, checkpoints ----------------------------------------------

def test_config_defaults_and_validation():
    from fiber_amd.es import GAConfig, SafeGAConfig

    cfg = SafeGAConfig()
    assert isinstance(cfg, GAConfig)
    assert (cfg.mode, cfg.s_min, cfg.pop, cfg.truncation) == ("abs", 0.01,
                                                              1024, 32)
    SafeGAConfig(mode="sum", s_min=1e-6, sigma=0.0)
    for bad in (dict(mode="so"), dict(mode=None), dict(s_min=0.0),
                dict(s_min=-1.0), dict(s_min=float("nan")),
                dict(s_min=float("inf")), dict(sigma=-0.1), dict(n_elite=0),
                dict(horizon=0)):
        with pytest.raises(ValueError):
            SafeGAConfig(**bad)


def test_engine_refuses_a_ring_context_and_a_bad_probe():
    from fiber_amd.es import SafeGAConfig, SafeGAEngine

    cfg = SafeGAConfig(pop=8, truncation=2, horizon=2)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        SafeGAEngine(cfg, ctx=object())
    cpu = torch.device("cpu")
    good = torch.from_numpy(C.probes()["special"].copy())
    eng = SafeGAEngine(cfg, device=cpu, probe=good)
    assert torch.equal(eng.probe, good)
    bad_nan = good.clone()
    bad_nan[3, 1] = float("nan")
    for bad in (good[:63], good.double(), good.t().contiguous(), bad_nan,
                good.reshape(-1)):
        with pytest.raises(ValueError):
            SafeGAEngine(cfg, device=cpu, probe=bad)


def test_ops_validate_before_touching_the_device():
    assert ops.ops_available()
    thetas = torch.zeros(2, ops.NPARAMS)
    probe = torch.zeros(64, 4)
    for bad in (dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(sigma=float("inf")), dict(s_min=0.0),
                dict(s_min=float("nan")), dict(s_min=float("inf")),
                dict(mode="max")):
        args = dict(sigma=0.01, s_min=0.01, mode="abs")
        args.update(bad)
        with pytest.raises(ValueError):
            ops.sm_steps(thetas, probe, **args)
    with pytest.raises(TypeError):
        ops.sm_steps(thetas, probe, 0.01)          # not on the GPU
    with pytest.raises(TypeError):
        ops.sm_steps(thetas.double(), probe, 0.01)
    with pytest.raises(TypeError):
        ops.sm_steps([0.0], probe, 0.01)
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.ga_rollout_mlp_sm(thetas, thetas.clone(), i32, i32, 1, 0, 4,
                              torch.zeros(4), torch.ones(4),
                              torch.zeros(4, 4), torch.zeros(4))
    with pytest.raises(TypeError):
        ops.ga_survivors_sm(thetas, thetas.clone(), i32, i32, i32, 1, 0)


def test_checkpoint_mismatches_are_refused():
    """sigma, seed, mode, s_min and the probe are compared before anything
    is decoded, so a CPU engine shows it."""
    from fiber_amd.es import GAConfig, GAEngine, SafeGAConfig, SafeGAEngine

    cpu = torch.device("cpu")
    base = dict(pop=8, truncation=2, horizon=2)
    state = SafeGAEngine(SafeGAConfig(**base), device=cpu).state_dict()
    assert "parents" not in state
    assert state["probe"].shape == (64, 4)
    assert state["config"]["mode"] == "abs"
    assert state["config"]["s_min"] == 0.01
    for other in (dict(sigma=0.004), dict(seed=7), dict(mode="sum"),
                  dict(s_min=0.02)):
        eng = SafeGAEngine(SafeGAConfig(**base, **other), device=cpu)
        with pytest.raises(ValueError):
            eng.load_state_dict(state)
    probe = torch.from_numpy(C.probes()["special"].copy())
    eng = SafeGAEngine(SafeGAConfig(**base), device=cpu, probe=probe)
    with pytest.raises(ValueError, match="probe"):
        eng.load_state_dict(state)
    # a plain GAEngine's checkpoint has no probe
    plain = GAEngine(GAConfig(sigma=SafeGAConfig().sigma, **base),
                     device=cpu).state_dict()
    eng = SafeGAEngine(SafeGAConfig(**base), device=cpu)
    with pytest.raises(ValueError):
        eng.load_state_dict(plain)
