"""fp64 per-layer references for the ConvNet-policy kernels
(fiber_amd/csrc/ops/conv_kernels.hip) and the per-element checker the
layer tests use.  CPU-only, pure torch.

Each ``*_reference`` takes the bytes/bf16 values a kernel consumes (the
layouts of the header comment in conv_kernels.hip and ``OFF`` in
conv_policy.py) and returns ``(pre64, absdot)``: the exact fp64
pre-activation, bias included, and ``sum_k |a_k * b_k|``, which bounds
every partial sum of the dot product and so the error of any fp32
summation order.

``check_layer`` applies, to every output element,

    |got - tanh(p)| <= 1/2 ulp_fmt(|tanh(p)| + slack) + slack
    slack = TAU + K * 2^-23 * sum_k |a_k b_k| + 2^-23 |bias|

* the products fp8 x fp8 and bf16 x bf16 are exact in fp32, so the only
  error of the accumulation is the K-1 fp32 additions (plus the bias
  add), each at most 2^-24 of a partial sum that ``absdot`` bounds;
* TAU = 2^-18 bounds ``fast_tanh_c`` for |x| <= 4 (``__expf`` and
  ``rcpf`` are ~1 ulp each; 1 - 2r then has absolute error < ~1.5e-6);
* tanh is 1-Lipschitz, so a pre-activation error of ``slack`` is at
  most ``slack`` after it, and the single rounding to the output format
  adds half a unit of that format at the (slack-widened) magnitude.

Nothing here is fitted to what a kernel returns.
"""

import torch

CENV = 16
IMG = 84
TAU = 2.0 ** -18
K_LAYER1 = 256
K_LAYER2 = 256
K_FC = 2592
NP_CONV = 677686
NP_CONV_PAD = 677688
OFF_B1, OFF_W2, OFF_B2 = 4096, 4112, 12304
OFF_W3, OFF_B3, OFF_W4, OFF_B4 = 12336, 675888, 676144, 677680

_F8 = torch.float8_e4m3fn


# ---------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------


def e4m3_bytes(x):
    """RNE fp32 -> OCP e4m3 bytes (uint8)."""
    return x.to(torch.float32).to(_F8).view(torch.uint8)


def e4m3_val(u8):
    """e4m3 bytes -> fp64 values."""
    return u8.contiguous().view(_F8).to(torch.float32).to(torch.float64)


def to_f64(t):
    """Dequantise a kernel buffer: uint8 is read as e4m3, the rest cast."""
    if t.dtype == torch.uint8:
        return e4m3_val(t)
    return t.to(torch.float32).to(torch.float64) \
        if t.dtype == torch.bfloat16 else t.to(torch.float64)


def _ulp(x, mant_bits, min_exp):
    x = torch.as_tensor(x, dtype=torch.float64).abs()
    _, ex = torch.frexp(x)  # x = m * 2^ex, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(ex, min_exp), ex - 1)
    e = e.clamp(min=min_exp)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64),
                     (e - mant_bits).to(torch.float64))


def ulp_bf16(x):
    """Spacing of bf16 (7 mantissa bits) at |x|."""
    return _ulp(x, 7, -126)


def ulp_e4m3(x):
    """Spacing of e4m3 (3 mantissa bits, min normal 2^-6) at |x|; constant
    2^-9 in the subnormal range."""
    return _ulp(x, 3, -6)


_ULP = {"bf16": ulp_bf16, "e4m3": ulp_e4m3}


# ---------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------


def obs_reference(znoise_u8, state, gtab_bf16, fused=False):
    """obs[E][84][84][4] as conv_layer1 builds it in LDS:
    e4m3(e4m3val(znoise[be % 16]) + state[be][ic] * g) in fp32, RNE.
    Returned as the fp32 values of the e4m3 bytes.

    The kernel's source is ``noise + s * g``; the compiler may contract it
    to one fma.  ``fused=False`` rounds the product and the sum (two fp32
    roundings), ``fused=True`` rounds the exact sum once (the 32-bit
    product of an fp32 and a bf16 number, and its sum with a 4-bit e4m3
    number, are exact in fp64).  Both are legal fp32 evaluations; they give
    different e4m3 bytes only where an e4m3 midpoint lies within one fp32
    ulp of the sum (a few pixels per million off the 1/8 grid)."""
    state = state.to(torch.float32)
    nenv = state.shape[0]
    noise = e4m3_val(znoise_u8).to(torch.float32).reshape(
        CENV, IMG * IMG, 4)
    rows = torch.arange(nenv) % CENV
    g = gtab_bf16.to(torch.float32).reshape(1, IMG * IMG, 1)
    if fused:
        r = (noise[rows].double()
             + state[:, None, :].double() * g.double()).to(torch.float32)
    else:
        r = noise[rows] + state[:, None, :] * g
    return r.to(_F8).to(torch.float32).reshape(nenv, IMG, IMG, 4)


def _patches(x, k, stride):
    """x[E][H][W][C] -> [E][OH*OW][(ky*k+kx)*C+ic]"""
    p = x.unfold(1, k, stride).unfold(2, k, stride)  # [E,OH,OW,C,ky,kx]
    n, oh, ow = p.shape[:3]
    return p.permute(0, 1, 2, 4, 5, 3).reshape(n, oh * ow, -1)


def _dot(x, w, b):
    """x[E][P][K] (member-major envs), w[M][O][K], b[M][O] ->
    pre64, absdot [E][P][O]."""
    nenv, npos, k = x.shape
    m = w.shape[0]
    assert nenv == m * CENV, (nenv, m)
    xm = x.reshape(m, CENV, npos, k)
    pre = torch.einsum("mepk,mok->mepo", xm, w) + b[:, None, None, :]
    absdot = torch.einsum("mepk,mok->mepo", xm.abs(), w.abs())
    return pre.reshape(nenv, npos, -1), absdot.reshape(nenv, npos, -1)


def layer1_reference(obs, w1_fp8_u8, b1_bf16):
    """conv 16@8x8 stride 4 of obs[E][84][84][4] with W1 rows ordered
    (ky*8+kx)*4+ic; returns pre64, absdot [E][400][16]."""
    x = _patches(to_f64(obs).reshape(-1, IMG, IMG, 4), 8, 4)
    w = e4m3_val(w1_fp8_u8).reshape(-1, 16, 256)
    return _dot(x, w, to_f64(b1_bf16).reshape(-1, 16))


def layer2_reference(act1_bf16, w2_bf16, b2_bf16):
    """conv 32@4x4 stride 2 of act1[E][20*20][16] with W2 rows ordered
    (ky*4+kx)*16+ic; returns [E][81][32], flat index (y*9+x)*32+oc."""
    x = _patches(to_f64(act1_bf16).reshape(-1, 20, 20, 16), 4, 2)
    w = to_f64(w2_bf16).reshape(-1, 32, 256)
    return _dot(x, w, to_f64(b2_bf16).reshape(-1, 32))


def fc_reference(act2_u8, w3_fp8_u8, b3_bf16):
    """W3 @ act2_flat + b3; returns pre64, absdot [E][256]."""
    x = e4m3_val(act2_u8).reshape(-1, 1, K_FC)
    w = e4m3_val(w3_fp8_u8).reshape(-1, 256, K_FC)
    pre, absdot = _dot(x, w, to_f64(b3_bf16).reshape(-1, 256))
    return pre[:, 0], absdot[:, 0]


def env_step_reference(state, action, env_A, env_B, racc):
    """The env half of conv_head_env in fp64 for given actions:
    state[E][4], action[E], racc[E] -> (new_state, new_racc).  The
    kernel's fp32 constants are used at their fp32 values."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa
    force = (action.to(torch.float64) - 2.5) * f32(0.4)
    s = to_f64(state).reshape(-1, 4)
    drive = torch.tanh(s @ to_f64(env_A).reshape(4, 4).T)
    snew = (f32(0.97) * s + f32(0.08) * drive
            + f32(0.05) * to_f64(env_B).reshape(1, 4) * force[:, None])
    racc_new = to_f64(racc).reshape(-1) + 1.0 - f32(0.1) * (
        snew * snew).sum(dim=1)
    return snew, racc_new


def head_env_reference(act3_bf16, w4, b4, state, env_A, env_B, racc):
    """conv_head_env in fp64.  act3[E][256], w4[M][6][256], b4[M][6],
    state[E][4], racc[E].  Returns (logits, action, new_state, new_racc,
    bound): the action is the FIRST maximum (the kernel's strict ``>``),
    and bound[E][6] = 256 * 2^-23 * sum|w*h| + 2^-23 |b| is the
    worst-case fp32 error of a logit."""
    h = to_f64(act3_bf16).reshape(-1, 1, 256)
    w = to_f64(w4).reshape(-1, 6, 256)
    b = to_f64(b4).reshape(-1, 6)
    logits, absdot = _dot(h, w, b)
    logits, absdot = logits[:, 0], absdot[:, 0]
    bound = 256 * 2.0 ** -23 * absdot + 2.0 ** -23 * \
        b.abs().repeat_interleave(CENV, dim=0)
    action = torch.from_numpy(logits.numpy().argmax(axis=1))  # first max
    snew, racc_new = env_step_reference(state, action, env_A, env_B, racc)
    return logits, action, snew, racc_new, bound


# ---------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------


def layer_errors(got, pre64, absdot, K, fmt, bias=None):
    """(err, half_ulp, slack), each shaped like pre64.  ``absdot=None``
    is the exact-arithmetic case: slack = TAU."""
    got = to_f64(got).reshape(pre64.shape)
    want = torch.tanh(pre64)
    slack = torch.full_like(pre64, TAU)
    if absdot is not None:
        slack = slack + K * 2.0 ** -23 * absdot
    if bias is not None:
        slack = slack + 2.0 ** -23 * to_f64(bias).abs().expand_as(pre64)
    half_ulp = 0.5 * _ULP[fmt](want.abs() + slack)
    return (got - want).abs(), half_ulp, slack


def _decode(flat_index, shape):
    idx = []
    for n in reversed(shape):
        idx.append(flat_index % n)
        flat_index //= n
    idx = idx[::-1]
    be = idx[0]
    rest = idx[1:]
    pos = rest[0] if len(rest) == 2 else None
    return {"member": be // CENV, "env": be % CENV, "pos": pos,
            "channel": rest[-1]}


def check_layer(got, pre64, absdot, K, fmt, bias=None, raise_on_fail=True,
                what="layer"):
    """Apply the criterion to EVERY element.  Returns the boolean mask of
    passing elements; with ``raise_on_fail`` raises AssertionError naming
    the worst offenders as (member, env, pos, channel)."""
    err, half_ulp, slack = layer_errors(got, pre64, absdot, K, fmt, bias)
    ok = ~(err > half_ulp + slack)  # a NaN in got fails
    ok &= torch.isfinite(err)
    if raise_on_fail and not bool(ok.all()):
        excess = torch.where(ok, torch.zeros_like(err),
                             torch.nan_to_num(err - half_ulp - slack,
                                              nan=float("inf")))
        worst = torch.argsort(excess.reshape(-1), descending=True)[:8]
        gotf = to_f64(got).reshape(-1)
        lines = []
        for i in worst.tolist():
            if bool(ok.reshape(-1)[i]):
                continue
            d = _decode(i, list(pre64.shape))
            lines.append(
                "  member %(member)d env %(env)d pos %(pos)s ch %(channel)d"
                % d + ": got %.9g want tanh(%.9g)=%.9g err %.3g allowed %.3g"
                % (gotf[i], pre64.reshape(-1)[i],
                   torch.tanh(pre64.reshape(-1)[i]), err.reshape(-1)[i],
                   (half_ulp + slack).reshape(-1)[i]))
        raise AssertionError(
            "%s: %d of %d elements outside the criterion; worst:\n%s"
            % (what, int((~ok).sum()), ok.numel(), "\n".join(lines)))
    return ok


def worst_margin(got, pre64, absdot, K, fmt, bias=None):
    """max over elements of (|got - tanh p| - 1/2 ulp) / slack; <= 1 is a
    pass.  Reported in profiles/conv_layer_tests.md."""
    err, half_ulp, slack = layer_errors(got, pre64, absdot, K, fmt, bias)
    return float(((err - half_ulp) / slack).max())


# ---------------------------------------------------------------------------
# test data shared by the CPU (checker power) and GPU (kernel) tests
# ---------------------------------------------------------------------------


def distinct_biases(n, gen):
    """n distinct non-zero bf16 biases with 0.1 <= |b| <= 1, random sign
    and order."""
    half = (n + 1) // 2
    mag = torch.linspace(0.1, 1.0, half)
    b = torch.cat([mag, -mag])[:n]
    b = b[torch.randperm(n, generator=gen)].to(torch.bfloat16)
    assert len(set(b.float().tolist())) == n and bool((b != 0).all())
    return b


def random_policy(nmembers, seed):
    """Random asymmetric weights, distinct O(0.5) biases, state/gtab on
    the 1/8 grid (so noise + s*g is exact in fp32, with or without FMA),
    znoise = e4m3 bytes of values in +-0.52.  Scales keep |p| <= 4."""
    gen = torch.Generator().manual_seed(seed)
    m = nmembers
    th = torch.zeros(m, NP_CONV_PAD)

    def rnd(n, scale):
        return torch.randn(m, n, generator=gen) * scale

    w1 = rnd(4096, 0.04)
    th[:, OFF_W2:OFF_B2] = rnd(32 * 256, 0.05)
    w3 = rnd(256 * K_FC, 0.02)
    th[:, OFF_W4:OFF_B4] = rnd(6 * 256, 256 ** -0.5)
    th[:, :OFF_B1] = w1
    th[:, OFF_W3:OFF_B3] = w3
    for off, n in ((OFF_B1, 16), (OFF_B2, 32), (OFF_B3, 256), (OFF_B4, 6)):
        for i in range(m):
            th[i, off:off + n] = distinct_biases(n, gen).float()
    nenv = m * CENV
    state = torch.randint(-8, 9, (nenv, 4), generator=gen).float() / 8
    gtab = (torch.randint(-8, 9, (IMG * IMG,), generator=gen).float()
            / 8).to(torch.bfloat16)
    znoise = e4m3_bytes(
        (torch.rand(CENV, IMG * IMG * 4, generator=gen) * 2 - 1) * 0.52)
    return {
        "wpert": th.to(torch.bfloat16),
        "w1_fp8": e4m3_bytes(w1),
        "w3_fp8": e4m3_bytes(w3),
        "state": state,
        "gtab": gtab,
        "znoise": znoise,
    }


def policy_views(p):
    """Named views into a policy dict's wpert."""
    w = p["wpert"]
    return {
        "b1": w[:, OFF_B1:OFF_W2], "w2": w[:, OFF_W2:OFF_B2],
        "b2": w[:, OFF_B2:OFF_W3], "b3": w[:, OFF_B3:OFF_W4],
        "w4": w[:, OFF_W4:OFF_B4], "b4": w[:, OFF_B4:NP_CONV],
    }


def _pick(values, shape, gen, p_zero):
    """Draw from {0} u values; 0 with probability p_zero."""
    v = torch.tensor(values, dtype=torch.float32)
    x = v[torch.randint(0, len(values), shape, generator=gen)]
    return torch.where(torch.rand(shape, generator=gen) >= p_zero, x,
                       torch.zeros_like(x))


def _pow2(js):
    return [s * 2.0 ** -j for j in js for s in (1.0, -1.0)]


def _grid_biases(n, gen):
    """distinct non-zero multiples of 1/256 with |b| < 1: exact in bf16
    (8 significant bits) and exactly addable to the sums below."""
    k = torch.randperm(510, generator=gen)[:n]  # distinct
    k = torch.where(k < 255, k - 255, k - 254)  # -255..-1, 1..255
    return k.float() / 256


def exact_policy(nmembers, seed):
    """Inputs on power-of-two grids: every product and every partial sum,
    in any order, is exact in fp32, so the criterion runs with slack =
    TAU alone.  Per layer (q = grid of the products, B = bound of
    sum|a*b|, checked by the tests from ``absdot``; q * 2^24 > B + 1 is
    what makes fp32 exact, the +1 covering the bias on the 2^-8 grid):

      layer 1  noise in {0, +-2^-1..2^-4} (state = 0, so obs = noise),
               W1 in {0, +-2^-2..2^-4}: q = 2^-8, B <= 256 * 2^-3 = 32
      layer 2  act1 in {0, +-2^0..2^-3}, W2 in {0, +-2^-2..2^-5}:
               q = 2^-8, B <= 256 * 2^-2 = 64
      fc       act2 in {0, +-2^0..2^-3}, W3 in {0, +-2^-4..2^-6} (sparse):
               q = 2^-9, B < 16 asserted.  Twelve marked k positions (per
               27-tile chunk: one in a main tile and one in each of the
               tail tiles 24, 25, 26) carry act2 = 1 and the twelve
               weights +-{1,2,3,4,5,6}/8, which no other position has and
               which cancel in the sum: a skipped or doubled tile moves p
               by at least 2^-3.
    """
    gen = torch.Generator().manual_seed(seed)
    m = nmembers
    nenv = m * CENV
    th = torch.zeros(m, NP_CONV_PAD)
    w1 = _pick(_pow2([2, 3, 4]), (m, 4096), gen, 0.5)
    th[:, :OFF_B1] = w1
    th[:, OFF_W2:OFF_B2] = _pick(_pow2([2, 3, 4, 5]), (m, 32 * 256), gen,
                                 0.5)
    w3 = _pick(_pow2([4, 5, 6]), (m, 256, K_FC), gen, 0.9)
    act2 = _pick(_pow2([0, 1, 2, 3]), (nenv, K_FC), gen, 0.75)
    marked = []
    for chunk in range(3):
        for tile, within in ((5 + 7 * chunk, 3 + chunk), (24, 9), (25, 17),
                             (26, 30)):
            marked.append((chunk * 27 + tile) * 32 + within)
    special = torch.tensor([1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6]) / 8.0
    perm =torch.stack([torch.randperm(12, generator=gen)
                        for _ in range(m * 256)]).reshape(m, 256, 12)
    w3[:, :, marked] = special[perm]
    act2[:, marked] = 1.0
    th[:, OFF_W3:OFF_B3] = w3.reshape(m, -1)
    for off, n in ((OFF_B1, 16), (OFF_B2, 32), (OFF_B3, 256)):
        for i in range(m):
            th[i, off:off + n] = _grid_biases(n, gen)
    znoise = e4m3_bytes(_pick(_pow2([1, 2, 3, 4]),
                              (CENV, IMG * IMG * 4), gen, 0.25))
    act1 = _pick(_pow2([0, 1, 2, 3]), (nenv, 400 * 16), gen, 0.5)
    wpert = th.to(torch.bfloat16)
    assert torch.equal(wpert.float(), th)  # grids are bf16-exact
    w1b, w3b = e4m3_bytes(w1), e4m3_bytes(w3.reshape(m, -1))
    assert torch.equal(e4m3_val(w1b).float(), w1)
    assert torch.equal(e4m3_val(w3b).float(), w3.reshape(m, -1))
    return {
        "wpert": wpert, "w1_fp8": w1b, "w3_fp8": w3b,
        "state": torch.zeros(nenv, 4),
        "gtab": (torch.randint(-8, 9, (IMG * IMG,), generator=gen).float()
                 / 8).to(torch.bfloat16),
        "znoise": znoise,
        "act1": act1.to(torch.bfloat16),
        "act2": e4m3_bytes(act2),
        "fc_marked_k": marked,
    }
