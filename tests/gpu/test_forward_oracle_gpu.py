"""The serving forward kernel and the MFMA probe against the fp64 oracle
(fiber_amd/es/forward_oracle.py; derivations in profiles/forward_oracle.md),
with the structural properties of the kernel (guard rows, position
independence, row isolation), the serving path against the rollout oracle,
and the validation of ops.mlp_policy_forward."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import forward_oracle_cases as C  # noqa: E402
from fiber_amd.es import forward_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

SENTINEL = 0x7FC5A5A5  # int32 bits of a NaN payload that no kernel writes


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev()).contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _sentinel_buffer(rows):
    buf = torch.full((rows, 2), SENTINEL, dtype=torch.int32)
    return buf.view(torch.float32).to(_dev()).contiguous()


# ---- 1. the oracle ------------------------------------------------------------

@requires_gpu
def test_logits_against_the_oracle():
    from fiber_amd import ops

    worst = {}
    for name, theta in C.thetas().items():
        th = _t(theta)
        for b in C.BATCHES:
            x = C.x_for(b)
            got = ops.mlp_policy_forward(th, _t(x)).cpu().numpy()
            ratio = C.check_logits(got, theta, x)
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ratio <= 1.0, (name, b, ratio)
    for name, ratio in worst.items():
        print("kernel vs oracle, %-14s worst |err|/tol = %.4f"
              % (name, ratio))


@requires_gpu
def test_logits_error_against_the_fp32_term():
    """Not asserted: the kernel's error over the fp32 term of the tolerance
    alone, i.e. how much of the criterion the flagged roundings use."""
    from fiber_amd import ops

    for name in ("init11", "asym0.2", "saturating4.0"):
        theta = C.thetas()[name]
        x = C.pool()
        got = ops.mlp_policy_forward(_t(theta), _t(x)).cpu().numpy()
        ref = fo.forward(theta, x)
        err = np.abs(got.astype(np.float64) - ref.logits)
        print("%-14s max |err| %.3e, max err/tol_fp32 %.3f, rows beyond the "
              "fp32 term %d of %d"
              % (name, err.max(), (err / ref.tol_fp32).max(),
                 int((err > ref.tol_fp32).any(-1).sum()), x.shape[0]))
        assert (err <= ref.tol).all()


@requires_gpu
def test_probe_against_the_oracle():
    from fiber_amd import ops

    for name, (a, b) in C.probe_inputs().items():
        got = ops.mfma_gemm64_probe(_t(a), _t(b)).cpu().numpy()
        ref = fo.probe_reference(a, b)
        bad = fo.probe_mismatches(got, ref)
        took_alt = int((got != ref.value).sum())
        print("probe %-8s: %d of 4096 not the nearest rounding, %d not "
              "permitted" % (name, took_alt, len(bad)))
        assert len(bad) == 0, (name, bad[:8])


# ---- 2. guard rows ------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("batch", (1, 63, 65, 129))
def test_rows_past_batch_are_never_written(batch):
    from fiber_amd import ops

    theta = C.thetas()["asym0.2"]
    x = C.x_for(batch)
    buf = _sentinel_buffer(batch + C.GUARD_ROWS)
    out = ops.mlp_policy_forward(_t(theta), _t(x), out=buf[:batch])
    assert out.data_ptr() == buf.data_ptr()
    torch.cuda.synchronize()
    bits = _bits(buf)
    assert (bits[batch:] == SENTINEL).all()
    assert C.check_logits(buf[:batch].cpu().numpy(), theta, x) <= 1.0
    # the same bits as with storage of its own
    assert torch.equal(_bits(out), _bits(ops.mlp_policy_forward(
        _t(theta), _t(x))))


# ---- 3. position independence ---------------------------------------------------

@requires_gpu
def test_logits_do_not_depend_on_where_the_row_sits():
    from fiber_amd import ops

    theta = _t(C.thetas()["asym0.2"])
    rows = C.pool()[:40]                       # the fixed set of rows
    base = _bits(ops.mlp_policy_forward(theta, _t(rows)))
    rng = np.random.default_rng(7)
    filler = C.pool()[60:]
    # a permutation of x
    perm = rng.permutation(40)
    got = _bits(ops.mlp_policy_forward(theta, _t(rows[perm])))
    assert torch.equal(got, base[perm])
    # the rows reversed: row e sits where row 39 - e sat
    got = _bits(ops.mlp_policy_forward(theta, _t(rows[::-1])))
    assert torch.equal(got, base.flip(0))
    # in another tile, at other offsets inside it, at other batch sizes
    for lead, tail in ((64, 0), (64, 25), (77, 0), (128, 24), (3, 1)):
        x = np.concatenate([filler[:lead], rows, filler[lead:lead + tail]])
        got = _bits(ops.mlp_policy_forward(theta, _t(x)))
        assert torch.equal(got[lead:lead + 40], base), (lead, tail)
    # one at a time
    for e in (0, 17, 39):
        got = _bits(ops.mlp_policy_forward(theta, _t(rows[e:e + 1])))
        assert torch.equal(got[0], base[e])


# ---- 4. row isolation -----------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("batch", (65, 192))
def test_a_non_finite_row_stays_in_its_row(batch):
    from fiber_amd import ops

    theta = _t(C.thetas()["asym0.2"])
    x = C.x_for(batch).copy()
    clean = _bits(ops.mlp_policy_forward(theta, _t(x)))
    nan_row, inf_row = 5, batch - 1
    for nan_col, inf_col in ((0, 3), (2, 1)):
        bad = x.copy()
        bad[nan_row, nan_col] = np.nan
        bad[inf_row, inf_col] = np.inf
        got_f = ops.mlp_policy_forward(theta, _t(bad)).cpu()
        got = _bits(got_f)
        others = np.ones(batch, bool)
        others[[nan_row, inf_row]] = False
        others = torch.from_numpy(others)
        assert torch.equal(got[others], clean[others])
        assert torch.isnan(got_f[nan_row]).all()


# ---- 5. serve what was trained --------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("pair", range(len(C.SERVE_PAIRS)))
def test_engine_act_takes_the_trained_action(pair):
    """ESEngine.act on the rollout oracle's states s_t must return the
    oracle's action at every step whose margin clears the oracle's own
    threshold by SAFETY times what rounding h2 can move l1 - l0 by.  The
    steps between the two thresholds are counted, not asserted."""
    from fiber_amd.es import ESConfig, ESEngine

    theta, ro, compared, band = C.serve_case(pair)
    assert compared.mean() >= C.SERVE_MIN_SHARE, compared.mean()
    engine = ESEngine(ESConfig(pop_per_gpu=2, horizon=C.SERVE_H), ctx=None,
                      device=_dev())
    engine.theta.copy_(_t(theta))
    engine.obs_mu = _t(C.SERVE_MU)
    engine.obs_nu = _t(C.SERVE_NU)
    states = ro.states[:, :C.SERVE_H].reshape(-1, 4).astype(np.float32)
    actions, logits = engine.act(_t(states), return_logits=True)
    assert actions.dtype == torch.int64 and tuple(logits.shape) == (512, 2)
    act = actions.cpu().numpy().reshape(64, C.SERVE_H).astype(bool)
    assert np.array_equal(act, (logits[:, 1] > logits[:, 0]).cpu().numpy()
                          .reshape(64, C.SERVE_H))
    wrong = compared & (act != ro.action)
    band_off = band & (act != ro.action)
    print("serve pair %d: compared %d of 512 steps (%.1f%%), band %d steps "
          "of which %d differ from the rollout oracle"
          % (pair, int(compared.sum()), 100.0 * compared.mean(),
             int(band.sum()), int(band_off.sum())))
    assert not wrong.any(), np.argwhere(wrong)[:8]


@requires_gpu
def test_raw_observations_would_not_pass():
    """The normalisation is what the comparison rests on: the same states
    fed to the kernel as they are miss the oracle's action at compared
    steps (8, 11 and 1 of them in an fp32 emulation on the CPU)."""
    from fiber_amd import ops

    missed = 0
    for pair in range(len(C.SERVE_PAIRS)):
        theta, ro, compared, _band = C.serve_case(pair)
        states = ro.states[:, :C.SERVE_H].reshape(-1, 4).astype(np.float32)
        logits = ops.mlp_policy_forward(_t(theta), _t(states)).cpu().numpy()
        act = (logits[:, 1] > logits[:, 0]).reshape(64, C.SERVE_H)
        missed += int((compared & (act != ro.action)).sum())
    print("raw observations: %d compared steps miss the oracle's action"
          % missed)
    assert missed >= 10


# ---- 6. validation --------------------------------------------------------------

class _OtherDevice:
    """Stands in for a tensor on a second GPU, which a one-GPU machine
    cannot hold: everything _check and the shape tests read."""

    dtype = torch.float32
    is_cuda = True
    device = torch.device("cuda", 1)

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def is_contiguous(self):
        return True

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        raise AssertionError("a tensor on another device reached a launch")


@requires_gpu
def test_validation_raises_before_launch(monkeypatch):
    from fiber_amd import ops

    dev = _dev()
    theta = torch.zeros(ops.NPARAMS, device=dev)
    x = torch.zeros(5, 4, device=dev)
    launches = []

    class Recorder:
        def mlp_policy_forward(self, *args):
            launches.append(args)

    monkeypatch.setattr(ops, "_OPS", Recorder())
    fwd = ops.mlp_policy_forward

    # wrong dtype, CPU tensor, non-contiguous, another device
    for bad_theta, bad_x in (
            (theta.double(), x), (theta, x.half()), (theta, x.long()),
            (theta.cpu(), x), (theta, x.cpu()),
            (torch.zeros(2 * ops.NPARAMS, device=dev)[::2], x),
            (theta, torch.zeros(5, 8, device=dev)[:, ::2]),
            (theta, torch.zeros(4, 5, device=dev).T),
            (_OtherDevice(ops.NPARAMS), x), (theta, _OtherDevice(5, 4))):
        with pytest.raises(TypeError):
            fwd(bad_theta, bad_x)
    for bad_out in (torch.zeros(5, 2, device=dev).double(),
                    torch.zeros(5, 2), torch.zeros(5, 4, device=dev)[:, ::2],
                    _OtherDevice(5, 2)):
        with pytest.raises(TypeError):
            fwd(theta, x, out=bad_out)
    # shapes
    for bad_theta, bad_x in (
            (theta[:-1].contiguous(), x),
            (torch.zeros(ops.NPARAMS + 1, device=dev), x),
            (theta.view(1, -1), x), (theta.view(-1, 1), x),
            (theta, torch.zeros(1, 3, device=dev)),      # {"obs": [[1,2,3]]}
            (theta, torch.zeros(4, device=dev)),         # a 1-D x
            (theta, torch.zeros(5, 5, device=dev)),
            (theta, torch.zeros(2, 5, 4, device=dev)),
            (theta, torch.zeros(0, device=dev)),         # {"obs": []} as is
            (theta, torch.zeros((), device=dev))):
        with pytest.raises(ValueError):
            fwd(bad_theta, bad_x)
    for bad_out in (torch.zeros(4, 2, device=dev),
                    torch.zeros(6, 2, device=dev),
                    torch.zeros(10, device=dev),
                    torch.zeros(2, 5, device=dev),
                    torch.zeros(5, 2, 1, device=dev)):
        with pytest.raises(ValueError):
            fwd(theta, x, out=bad_out)
    # the 32-bit row index, without allocating
    assert ops._check_forward_batch(2 ** 29 - 1) == 2 ** 29 - 1
    for bad in (2 ** 29, 2 ** 29 + 1, 2 ** 31, -1):
        with pytest.raises(ValueError):
            ops._check_forward_batch(bad)
    assert launches == []
    # an empty batch: an empty result and no launch
    empty = fwd(theta, torch.zeros(0, 4, device=dev))
    assert tuple(empty.shape) == (0, 2) and empty.dtype == torch.float32
    assert empty.device == x.device
    keep = torch.zeros(0, 2, device=dev)
    assert fwd(theta, torch.zeros(0, 4, device=dev), out=keep) is keep
    assert launches == []
    # the recorder does see valid calls: the checks above are live
    out = torch.zeros(5, 2, device=dev)
    assert tuple(fwd(theta, x).shape) == (5, 2)
    assert fwd(theta, x, out=out) is out
    assert fwd(theta, x, out=torch.zeros(9, 2, device=dev)[:5]).shape[0] == 5
    assert len(launches) == 3
    assert launches[1][0] == theta.data_ptr() and launches[1][2] == 5
    assert launches[1][3] == out.data_ptr()


@requires_gpu
def test_engine_act_validates_and_breaks_ties_to_zero(monkeypatch):
    from fiber_amd import ops
    from fiber_amd.es import ESConfig, ESEngine

    engine = ESEngine(ESConfig(pop_per_gpu=2, horizon=2), ctx=None,
                      device=_dev())
    for bad in (torch.zeros(1, 3, device=_dev()), torch.zeros(4, device=_dev()),
                torch.zeros(2, 2, 4, device=_dev())):
        with pytest.raises(ValueError):
            engine.act(bad)
    for bad in (torch.zeros(1, 4, device=_dev()).double(), torch.zeros(1, 4),
                [[0.0, 0.0, 0.0, 0.0]]):
        with pytest.raises(TypeError):
            engine.act(bad)
    assert tuple(engine.act(torch.zeros(0, 4, device=_dev())).shape) == (0,)
    # zero weights and equal biases: l1 == l0, the action is 0
    engine.theta.zero_()
    a, l = engine.act(torch.randn(70, 4, device=_dev()), return_logits=True)
    assert (l[:, 0] == l[:, 1]).all() and (a == 0).all()
    # what reaches the kernel is the normalised, clamped observation
    engine.obs_mu = _t(C.SERVE_MU)
    engine.obs_nu = _t(C.SERVE_NU)
    seen = []
    real = ops.mlp_policy_forward
    monkeypatch.setattr(ops, "mlp_policy_forward",
                        lambda theta, x: seen.append(x.clone()) or real(
                            theta, x))
    obs = _t(np.array([[0.05, -0.03, 0.02, -0.1], [1.05, 0.97, -0.98, 0.9],
                       [100.0, -100.0, 3.0, 0.0]], dtype=np.float32))
    engine.act(obs)
    rstd = 1.0 / np.sqrt(np.float64(np.float32(0.5))
                         + np.float64(np.float32(1e-4)))
    want = np.clip((obs.cpu().double().numpy() - C.SERVE_MU.astype(
        np.float64)) * rstd, -5.0, 5.0)
    got = seen[0].cpu().double().numpy()
    assert seen[0].dtype == torch.float32 and seen[0].is_contiguous()
    # X_REL of the rollout oracle: 7 roundings of the fp32 formula
    from fiber_amd.es import rollout_oracle as oracle
    assert (np.abs(got - want) <= oracle.X_REL * np.abs(want)).all()
    assert got[0].tolist() == [0.0] * 4 and got[2, 0] == 5.0 \
        and got[2, 1] == -5.0
