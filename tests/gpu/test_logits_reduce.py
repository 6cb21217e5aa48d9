"""The rollout loop's cross-lane logits reduce, bit for bit.

The step loop sums each env's logits partials over the wave's four 16-lane
rows with v_permlane16_swap / v_permlane32_swap; it used to run a shfl_xor
tree through ds_bpermute.  The rollout outputs see the logits only through
`l1 > l0`, so the rollout goldens would miss most reduce errors.
ops.logits_reduce_probe runs both forms on the same per-lane partials
p0[4][64], p1[4][64] (4 column tiles x 64 lanes) and returns the
[64 env][2 logits] row each one writes; they must agree on the int32 view.

The tree, per tile ct and lane column l (env = ct*16 + l), is
(p[l] + p[l+16]) + (p[l+32] + p[l+48]) in fp32.  Integer-valued patterns
make every add exact, so a numpy model pins the tile / logit / env
addressing as well.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


def _probe(p0, p1):
    from fiber_amd import ops

    dev = torch.device("cuda", 0)
    shfl, swap = ops.logits_reduce_probe(
        torch.from_numpy(np.ascontiguousarray(p0, dtype=np.float32)).to(dev),
        torch.from_numpy(np.ascontiguousarray(p1, dtype=np.float32)).to(dev))
    return shfl.cpu().numpy(), swap.cpu().numpy()


def _tree(p0, p1):
    """numpy model: out[ct*16 + l][a] for a = 0 (p0), 1 (p1)."""
    out = np.empty((64, 2), dtype=np.float32)
    for a, p in enumerate((p0, p1)):
        r = p.astype(np.float32).reshape(4, 4, 16)  # [tile][kgrp][l]
        out[:, a] = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])).reshape(64)
    return out


def _assert_same_bits(shfl, swap, what):
    assert shfl.shape == swap.shape == (64, 2)
    bad = np.argwhere(shfl.view(np.int32) != swap.view(np.int32))
    assert bad.size == 0, (what, bad[:8], shfl[tuple(bad[0])],
                           swap[tuple(bad[0])])


def _random_cases():
    rng = np.random.default_rng(20250)
    cases = {}
    cases["normal"] = (rng.standard_normal((4, 64)),
                       rng.standard_normal((4, 64)))
    # magnitudes spread over ~20 binades: any other add order rounds
    # differently somewhere in 512 sums
    for i in range(3):
        e0 = rng.integers(-10, 11, (4, 64)).astype(np.float64)
        e1 = rng.integers(-10, 11, (4, 64)).astype(np.float64)
        cases["binades%d" % i] = (
            rng.standard_normal((4, 64)) * np.exp2(e0),
            rng.standard_normal((4, 64)) * np.exp2(e1))
    return cases


@requires_gpu
@pytest.mark.parametrize("name", ["normal", "binades0", "binades1",
                                  "binades2"])
def test_swap_equals_shfl_random(name):
    p0, p1 = _random_cases()[name]
    shfl, swap = _probe(p0, p1)
    assert np.isfinite(shfl).all()
    _assert_same_bits(shfl, swap, name)
    # the spread data is only a test if the order matters for it: the
    # other pairing of the same four values must round differently
    # somewhere
    r = p0.astype(np.float32).reshape(4, 4, 16)
    other = ((r[:, 0] + r[:, 2]) + (r[:, 1] + r[:, 3])).reshape(64)
    if name != "normal":
        assert (other.view(np.int32) != shfl[:, 0].view(np.int32)).any()


@requires_gpu
def test_swap_equals_shfl_zeros_and_infinities():
    rng = np.random.default_rng(7)
    # signed zeros: a sum is -0 only if all four terms are
    z0 = np.where(rng.integers(0, 2, (4, 64)) == 1, -0.0, 0.0)
    z1 = np.full((4, 64), -0.0)
    z1[:, ::5] = 0.0
    shfl, swap = _probe(z0, z1)
    _assert_same_bits(shfl, swap, "zeros")
    assert (shfl == 0).all()
    assert np.signbit(shfl).any() and not np.signbit(shfl).all()

    # infinities among finite values: +inf, -inf, and inf - inf = NaN
    f0 = rng.standard_normal((4, 64))
    f1 = rng.standard_normal((4, 64))
    f0[rng.integers(0, 8, (4, 64)) == 0] = np.inf
    f0[rng.integers(0, 8, (4, 64)) == 0] = -np.inf
    f1[rng.integers(0, 6, (4, 64)) == 0] = np.inf
    f1[:, 48:] = np.where(rng.integers(0, 3, (4, 16)) == 0, -np.inf,
                          f1[:, 48:])
    shfl, swap = _probe(f0, f1)
    _assert_same_bits(shfl, swap, "infinities")
    assert np.isnan(shfl).any() and np.isposinf(shfl).any() \
        and np.isneginf(shfl).any() and np.isfinite(shfl).any()


@requires_gpu
@pytest.mark.parametrize("square", [False, True], ids=["id", "id_squared"])
def test_lane_id_pattern_pins_addressing(square):
    # every (tile, lane) of p0 holds its own id 0..255, p1 the ids
    # 256..511; squared ids make sums of wrong lane sets collide less.
    # All values and sums are integers below 2**24: exact in fp32.
    ids = np.arange(256, dtype=np.float64).reshape(4, 64)
    p0, p1 = ids, ids + 256.0
    if square:
        p0, p1 = p0 * p0, p1 * p1
    shfl, swap = _probe(p0, p1)
    want = _tree(p0, p1)
    _assert_same_bits(shfl, swap, "lane id")
    assert np.array_equal(swap.view(np.int32), want.view(np.int32)), (
        swap, want)
    assert np.unique(want).size == 128
