"""The rollout kernels' tanh computes e^{2x} as exp2(x * 2*log2e) instead
of exp2((x + x) * log2e) (fiber_amd/csrc/ops/es_kernels.hip, TWO_LOG2E).
The two exp2 arguments must agree bitwise for every float32 x: x + x is
exact, and 2*log2e is the float32 log2e with its exponent bumped, so both
products round the same real number.  Checked here in numpy float32, which
rounds each multiply and add once (IEEE), like v_mul_f32 / v_add_f32."""

import re
import os

import numpy as np

LOG2E_BITS = 0x3FB8AA3B       # the constant __expf multiplies by
TWO_LOG2E_BITS = 0x4038AA3B   # the folded constant

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _both(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        old = (x + x) * _f32(LOG2E_BITS)
        new = x * _f32(TWO_LOG2E_BITS)
    assert old.dtype == np.float32 and new.dtype == np.float32
    return old.view(np.uint32), new.view(np.uint32)


def _assert_same_bits(x):
    old, new = _both(x)
    nan = np.isnan(x)
    # NaN in, NaN out on both sides (payloads are not part of the claim)
    assert np.isnan(old.view(np.float32)[nan]).all()
    assert np.isnan(new.view(np.float32)[nan]).all()
    bad = np.flatnonzero((old != new) & ~nan)
    assert bad.size == 0, [(hex(int(x.view(np.uint32)[i])), hex(int(old[i])),
                            hex(int(new[i]))) for i in bad[:8]]


def test_constants():
    assert _f32(TWO_LOG2E_BITS) == np.float32(2.0) * _f32(LOG2E_BITS)
    assert _f32(LOG2E_BITS) == np.float32(1.4426950408889634)
    # the kernel source spells the constant as a hex float literal
    src = open(os.path.join(REPO, "fiber_amd", "csrc", "ops",
                            "es_kernels.hip")).read()
    lit = re.search(r"#define TWO_LOG2E (0x[0-9a-f.]+p[+-]?\d+)f", src)
    assert lit, "TWO_LOG2E literal not found"
    assert np.float32(float.fromhex(lit.group(1))) == _f32(TWO_LOG2E_BITS)
    assert float.fromhex(lit.group(1)) == float(_f32(TWO_LOG2E_BITS))


def test_random_bit_patterns():
    rng = np.random.default_rng(20250)
    bits = rng.integers(0, 1 << 32, size=2_000_000, dtype=np.uint64)
    _assert_same_bits(bits.astype(np.uint32).view(np.float32))


def test_edge_values():
    fi = np.finfo(np.float32)
    edges = [0x00000000, 0x80000000,            # +-0
             0x00000001, 0x80000001,            # smallest denormals
             0x007FFFFF, 0x807FFFFF,            # largest denormals
             0x00400000, 0x00400001,            # x + x crosses into normals
             0x00800000, 0x80800000,            # smallest normals
             0x7F7FFFFF, 0xFF7FFFFF,            # +-FLT_MAX
             0x7EFFFFFF, 0x7F000000,            # x + x overflows
             0x7F800000, 0xFF800000]            # +-inf
    x = np.array(edges, dtype=np.uint32).view(np.float32)
    assert x[10] == fi.max and x[11] == -fi.max
    _assert_same_bits(x)
    # every denormal and the first normal binade, both signs: 2^25 values
    # is too many for a quick test, so a stride that hits both parities
    d = np.arange(0, 0x01000000, 37, dtype=np.uint32)
    _assert_same_bits(d.view(np.float32))
    _assert_same_bits((d | np.uint32(0x80000000)).view(np.float32))
    # the top two binades, where x + x and the product overflow
    t = np.arange(0x7E000000, 0x7F800000, 53, dtype=np.uint32)
    _assert_same_bits(t.view(np.float32))
