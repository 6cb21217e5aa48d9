"""CPU tests of fiber_amd/es/conv_reference.py: the fp64 per-layer
references agree with torch's conv2d / matmul, and the per-element
criterion of ``check_layer`` accepts an honest fp32 emulation of each
layer on every element while rejecting each of the indexing / rounding
mistakes the MFMA kernels could make.  The GPU side of the same checks
is tests/gpu/test_conv_layers.py.

Run with ``-s`` to see the mutation table (mutation -> rejected element
count) and the constant-action fitness deltas.
"""

import pytest
import torch
import torch.nn.functional as F

from fiber_amd.es import conv_reference as cr

M = 3  # odd, so a member-stride error cannot alias
E = M * cr.CENV
_F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def pol():
    return cr.random_policy(M, 20241)


def fast_tanh32(x):
    assert x.dtype == torch.float32
    return 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0)


def conv_f(x, w, b, stride, dtype):
    """torch conv2d per member.  x[E][H][W][C], w[M][O][k][k][C], b[M][O]
    -> [E][OH*OW][O]; the permute(0,3,1,2) weight reorder is the one
    conv_rollout_reference uses."""
    outs = []
    for m in range(w.shape[0]):
        xm = x[m * cr.CENV:(m + 1) * cr.CENV].permute(0, 3, 1, 2).to(dtype)
        y = F.conv2d(xm, w[m].permute(0, 3, 1, 2).contiguous().to(dtype),
                     b[m].to(dtype), stride=stride)
        outs.append(y.permute(0, 2, 3, 1).reshape(cr.CENV, -1, w.shape[1]))
    return torch.cat(outs)


MUTATIONS = ["kykx_transposed", "k_tiles_swapped", "last_k_tile_dropped",
             "bias_shifted", "member0_weights_for_member1",
             "env_rows_rolled", "drow_rolled_by_4", "extra_bf16_rounding"]


def emulate(x, w, b, stride, fmt, mutation=None):
    """fp32 emulation of one layer: fp32 conv, the kernel's tanh formula
    in fp32, one rounding to the output format."""
    x, w, b = x.float().clone(), w.float().clone(), b.float().clone()
    m, o = w.shape[:2]
    if mutation == "kykx_transposed":
        w = w.transpose(2, 3).contiguous()
    elif mutation == "k_tiles_swapped":
        t = w.reshape(m, o, -1, 32).clone()
        t[:, :, [2, 5]] = t[:, :, [5, 2]]
        w = t.reshape(w.shape)
    elif mutation == "last_k_tile_dropped":
        t = w.reshape(m, o, -1, 32).clone()
        t[:, :, -1] = 0
        w = t.reshape(w.shape)
    elif mutation == "bias_shifted":
        b = torch.roll(b, 1, dims=1)
    elif mutation == "member0_weights_for_member1":
        w[1] = w[0]
    elif mutation == "env_rows_rolled":
        x = torch.roll(x, 1, dims=0)
    y = fast_tanh32(conv_f(x, w, b, stride, torch.float32))
    if mutation == "drow_rolled_by_4":
        y = torch.roll(y, 4, dims=2)
    if mutation == "extra_bf16_rounding":
        y = y.to(torch.bfloat16).float()
    return y.to(torch.bfloat16) if fmt == "bf16" else cr.e4m3_bytes(y)


def per_env(b):
    return b.repeat_interleave(cr.CENV, dim=0)[:, None, :]


@pytest.fixture(scope="module")
def layers(pol):
    """Per layer: emulation inputs, the reference of the unmutated layer,
    and the honest emulation's output, which feeds the next layer."""
    v = cr.policy_views(pol)
    obs = cr.obs_reference(pol["znoise"], pol["state"], pol["gtab"])
    w1 = cr.e4m3_val(pol["w1_fp8"]).reshape(M, 16, 8, 8, 4)
    L = {}
    L[1] = dict(x=obs, w=w1, b=v["b1"].float(), stride=4, fmt="bf16",
                K=cr.K_LAYER1,
                ref=cr.layer1_reference(obs, pol["w1_fp8"], v["b1"]))
    act1 = emulate(obs, w1, v["b1"], 4, "bf16")
    L[2] = dict(x=act1.float().reshape(E, 20, 20, 16),
                w=v["w2"].float().reshape(M, 32, 4, 4, 16),
                b=v["b2"].float(), stride=2, fmt="e4m3", K=cr.K_LAYER2,
                ref=cr.layer2_reference(act1, v["w2"], v["b2"]))
    act2 = emulate(L[2]["x"], L[2]["w"], v["b2"], 2, "e4m3")
    pre, absdot = cr.fc_reference(act2.reshape(E, -1), pol["w3_fp8"],
                                  v["b3"])
    L[3] = dict(x=cr.e4m3_val(act2).reshape(E, 9, 9, 32),
                w=cr.e4m3_val(pol["w3_fp8"]).reshape(M, 256, 9, 9, 32),
                b=v["b3"].float(), stride=1, fmt="bf16", K=cr.K_FC,
                ref=(pre[:, None, :], absdot[:, None, :]))
    return L


# ---------------------------------------------------------------------------
# formats
# ---------------------------------------------------------------------------


def test_ulp_known_values():
    assert float(cr.ulp_bf16(1.0)) == 2.0 ** -7
    assert float(cr.ulp_bf16(0.999)) == 2.0 ** -8
    assert float(cr.ulp_bf16(-3.0)) == 2.0 ** -6
    assert float(cr.ulp_e4m3(1.0)) == 2.0 ** -3
    assert float(cr.ulp_e4m3(448.0)) == 32.0
    assert float(cr.ulp_e4m3(2.0 ** -6)) == 2.0 ** -9
    assert float(cr.ulp_e4m3(1e-4)) == 2.0 ** -9
    assert float(cr.ulp_e4m3(0.0)) == 2.0 ** -9


def test_ulp_matches_torch_rounding():
    """RNE to the format moves a value by at most ulp/2, and some value
    in every binade moves by more than ulp/4 (the ulp is not too big)."""
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(200000, generator=gen, dtype=torch.float64) * 2 - 1)
    x = x * torch.pow(2.0, torch.randint(-8, 2, x.shape, generator=gen)
                      .double())
    for ulp, rnd in ((cr.ulp_bf16, lambda t: t.float().to(torch.bfloat16)),
                     (cr.ulp_e4m3, lambda t: t.float().to(_F8))):
        xr = x.float().double()  # representable in fp32 first
        d = (rnd(xr).float().double() - xr).abs()
        assert bool((d <= 0.5 * ulp(xr)).all())
        assert float((d / ulp(xr)).max()) > 0.49


# ---------------------------------------------------------------------------
# references against conv2d / matmul
# ---------------------------------------------------------------------------


def test_obs_reference_explicit_pixels(pol):
    obs = cr.obs_reference(pol["znoise"], pol["state"], pol["gtab"])
    assert obs.shape == (E, 84, 84, 4)
    zn = cr.e4m3_val(pol["znoise"]).float().reshape(16, 84, 84, 4)
    g = pol["gtab"].float().reshape(84, 84)
    for be, y, x, ic in ((0, 0, 0, 0), (17, 83, 83, 3), (47, 5, 80, 2),
                         (31, 40, 1, 1), (16, 0, 83, 0)):
        r = zn[be % 16, y, x, ic] + pol["state"][be, ic] * g[y, x]
        assert float(obs[be, y, x, ic]) == float(r.to(_F8).float())
    # the state term is visible: members differ although znoise is shared
    assert not torch.equal(obs[0], obs[16])


@pytest.mark.parametrize("layer", [1, 2, 3])
def test_reference_matches_conv2d(layers, layer):
    c = layers[layer]
    pre, absdot = c["ref"]
    want = conv_f(c["x"].double(), c["w"].double(), c["b"].double(),
                  c["stride"], torch.float64)
    assert pre.shape == want.shape and pre.dtype == torch.float64
    assert float((pre - want).abs().max()) < 1e-12
    want_abs = conv_f(c["x"].double().abs(), c["w"].double().abs(),
                      torch.zeros_like(c["b"]).double(), c["stride"],
                      torch.float64)
    assert float((absdot - want_abs).abs().max()) < 1e-12
    # |p| <= 4 is what TAU is derived for
    assert float(pre.abs().max()) <= 4.0


def test_fc_reference_matches_matmul(pol, layers):
    v = cr.policy_views(pol)
    act2 = cr.e4m3_bytes(layers[3]["x"].reshape(E, -1))
    pre, _ = cr.fc_reference(act2, pol["w3_fp8"], v["b3"])
    w3 = cr.e4m3_val(pol["w3_fp8"]).reshape(M, 256, 2592)
    for m in range(M):
        sl = slice(m * 16, (m + 1) * 16)
        want = cr.e4m3_val(act2[sl]) @ w3[m].T + v["b3"][m].double()
        assert float((pre[sl] - want).abs().max()) < 1e-12


def test_head_env_reference(pol):
    v = cr.policy_views(pol)
    gen = torch.Generator().manual_seed(3)
    act3 = (torch.rand(E, 256, generator=gen) * 2 - 1).to(torch.bfloat16)
    env_A = torch.randn(4, 4, generator=gen) * 0.5
    env_B = torch.randn(4, generator=gen)
    racc = torch.full((E,), 3.25)
    logits, action, snew, racc_new, bound = cr.head_env_reference(
        act3, v["w4"], v["b4"], pol["state"], env_A, env_B, racc)
    s = pol["state"].double()
    for m in range(M):
        sl = slice(m * 16, (m + 1) * 16)
        lg = act3[sl].double() @ v["w4"][m].double().reshape(6, 256).T \
            + v["b4"][m].double()
        assert float((logits[sl] - lg).abs().max()) < 1e-12
        a = lg.argmax(dim=1)
        assert torch.equal(action[sl], a)
        force = (a.double() - 2.5) * 0.4
        want = 0.97 * s[sl] + 0.08 * torch.tanh(s[sl] @ env_A.double().T) \
            + 0.05 * env_B.double() * force[:, None]
        assert float((snew[sl] - want).abs().max()) < 1e-6
        assert float((racc_new[sl] - (3.25 + 1 - 0.1 * (want * want)
                                      .sum(1))).abs().max()) < 1e-6
    assert bound.shape == (E, 6) and bool((bound > 0).all())
    # first maximum wins
    z = torch.zeros(M, 6 * 256)
    b4 = torch.tensor([[1., 1, 1, 1, 1, 1], [0, 0, 2, 0, 2, 0],
                       [0, 0, 0, 0, 0, 3]])
    _, action, _, _, _ = cr.head_env_reference(
        act3, z, b4, pol["state"], env_A, env_B, racc)
    assert action.reshape(M, 16).tolist() == [[0] * 16, [2] * 16, [5] * 16]


# ---------------------------------------------------------------------------
# checker power
# ---------------------------------------------------------------------------


def rejected(c, mutation):
    pre, absdot = c["ref"]
    out = emulate(c["x"], c["w"], c["b"], c["stride"], c["fmt"], mutation)
    ok = cr.check_layer(out, pre, absdot, c["K"], c["fmt"],
                        bias=per_env(c["b"]), raise_on_fail=False)
    return int((~ok).sum()), ok.numel()


@pytest.mark.parametrize("layer", [1, 2, 3])
def test_checker_accepts_fp32_emulation(layers, layer):
    c = layers[layer]
    pre, absdot = c["ref"]
    out = emulate(c["x"], c["w"], c["b"], c["stride"], c["fmt"])
    ok = cr.check_layer(out, pre, absdot, c["K"], c["fmt"],
                        bias=per_env(c["b"]), what="layer %d" % layer)
    assert bool(ok.all())
    print("layer %d unmutated: 0 of %d rejected, worst margin %.3f"
          % (layer, ok.numel(),
             cr.worst_margin(out, pre, absdot, c["K"], c["fmt"],
                             per_env(c["b"]))))


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("layer", [1, 2, 3])
def test_checker_rejects_mutation(layers, layer, mutation):
    c = layers[layer]
    if mutation == "extra_bf16_rounding" and c["fmt"] == "bf16":
        # a second bf16 rounding of a bf16 output changes nothing: the
        # mutation only exists where the output is e4m3 (layer 2)
        out = emulate(c["x"], c["w"], c["b"], c["stride"], c["fmt"])
        again = emulate(c["x"], c["w"], c["b"], c["stride"], c["fmt"],
                        mutation)
        assert torch.equal(out, again)
        return
    n, total = rejected(c, mutation)
    print("layer %d %-28s rejected %6d of %d" % (layer, mutation, n, total))
    assert n > 0


def test_check_layer_raises_with_decoded_index(layers):
    c = layers[2]
    pre, absdot = c["ref"]
    out = emulate(c["x"], c["w"], c["b"], c["stride"], c["fmt"]).clone()
    be, pos, ch = 2 * 16 + 5, 80, 31
    out[be, pos, ch] = 0x7E if out[be, pos, ch] != 0x7E else 0x00  # 448
    with pytest.raises(AssertionError) as ei:
        cr.check_layer(out, pre, absdot, c["K"], c["fmt"],
                       bias=per_env(c["b"]))
    assert "member 2 env 5 pos 80 ch 31" in str(ei.value)
    assert "1 of %d" % pre.numel() in str(ei.value)


def test_check_layer_rejects_nan(layers):
    c = layers[1]
    pre, absdot = c["ref"]
    out = emulate(c["x"], c["w"], c["b"], c["stride"], c["fmt"]).clone()
    out[0, 0, 0] = float("nan")
    ok = cr.check_layer(out, pre, absdot, c["K"], c["fmt"],
                        raise_on_fail=False)
    assert not bool(ok[0, 0, 0]) and int((~ok).sum()) == 1


# ---------------------------------------------------------------------------
# exact-arithmetic data
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def exact():
    return cr.exact_policy(M, 777)


def test_exact_policy_is_exact_in_fp32(exact):
    """sum|a*b| + 1 < q * 2^24: every partial sum, in any order and with
    the bias, is a multiple of q below 2^24 * q, i.e. an fp32 number.
    The fp32 emulation then has slack = TAU only, and passes."""
    v = cr.policy_views(exact)
    obs = cr.obs_reference(exact["znoise"], exact["state"], exact["gtab"])
    assert torch.equal(cr.e4m3_bytes(obs).reshape(E, -1),
                       exact["znoise"].repeat(M, 1))  # state = 0
    cases = [
        (1, cr.layer1_reference(obs, exact["w1_fp8"], v["b1"]), 2.0 ** -8,
         dict(x=obs, w=cr.e4m3_val(exact["w1_fp8"]).reshape(M, 16, 8, 8, 4),
              b=v["b1"], stride=4, fmt="bf16")),
        (2, cr.layer2_reference(exact["act1"], v["w2"], v["b2"]), 2.0 ** -8,
         dict(x=exact["act1"].float().reshape(E, 20, 20, 16),
              w=v["w2"].float().reshape(M, 32, 4, 4, 16), b=v["b2"],
              stride=2, fmt="e4m3")),
    ]
    pre, absdot = cr.fc_reference(exact["act2"], exact["w3_fp8"], v["b3"])
    cases.append(
        (3, (pre[:, None], absdot[:, None]), 2.0 ** -9,
         dict(x=cr.e4m3_val(exact["act2"]).reshape(E, 9, 9, 32),
              w=cr.e4m3_val(exact["w3_fp8"]).reshape(M, 256, 9, 9, 32),
              b=v["b3"], stride=1, fmt="bf16")))
    for layer, (pre, absdot), q, c in cases:
        assert float(absdot.max()) + 1 < q * 2 ** 24
        assert bool((pre / q == torch.round(pre / q)).all())
        assert float(pre.abs().max()) <= 4.0
        pre32 = conv_f(c["x"], c["w"].float(), c["b"].float(), c["stride"],
                       torch.float32)
        assert torch.equal(pre32.double(), pre)
        out = emulate(c["x"], c["w"], c["b"], c["stride"], c["fmt"])
        cr.check_layer(out, pre, None, 0, c["fmt"],
                       what="exact layer %d" % layer)
    assert float(cases[2][1][1].max()) < 16


def test_exact_fc_marked_tiles(exact):
    """Skipping or doubling any of the twelve marked k-tiles moves every
    fc pre-activation by at least 2^-3, and the weights there are
    values no other position has."""
    w3 = cr.e4m3_val(exact["w3_fp8"]).reshape(M, 256, 2592)
    a2 = cr.e4m3_val(exact["act2"]).reshape(M, 16, 2592)
    marked = exact["fc_marked_k"]
    tiles = sorted(k // 32 for k in marked)
    assert tiles == sorted([5, 24, 25, 26, 27 + 12, 27 + 24, 27 + 25,
                            27 + 26, 54 + 19, 54 + 24, 54 + 25, 54 + 26])
    others = torch.ones(2592, dtype=torch.bool)
    others[marked] = False
    assert float(w3[:, :, others].abs().max()) < 2.0 ** -3
    for m in range(M):
        for o in (0, 100, 255):
            assert sorted((w3[m, o, marked] * 8).tolist()) == \
                [-6, -5, -4, -3, -2, -1, 1, 2, 3, 4, 5, 6]
    assert bool((a2[:, :, marked] == 1).all())
    # the property that matters: the checker sees every skipped tile
    v = cr.policy_views(exact)
    pre, _ = cr.fc_reference(exact["act2"], exact["w3_fp8"], v["b3"])
    for t in tiles:
        wm = w3.clone()
        wm[:, :, t * 32:t * 32 + 32] = 0
        p2 = torch.einsum("mek,mok->meo", a2, wm).reshape(E, 256) \
            + v["b3"].double().repeat_interleave(16, dim=0)
        out = torch.tanh(p2).float().to(torch.bfloat16)
        ok = cr.check_layer(out, pre, None, 0, "bf16", raise_on_fail=False)
        assert int((~ok).sum()) > 0.9 * ok.numel(), (t, int((~ok).sum()))


# ---------------------------------------------------------------------------
# why the per-layer tests exist: the rollout fitness barely sees the policy
# ---------------------------------------------------------------------------


def test_constant_action_fitness_delta_is_recorded():
    """conv_rollout_reference's arithmetic with the policy's action
    replaced by a constant (local copy of its env loop; horizon 3,
    members [0, 1]).  The distance to the real fitness is what a policy
    with garbage layers could move test_rollout_vs_fp32_reference by;
    its tolerance is 5e-2.  Recorded (profiles/conv_layer_tests.md), not
    asserted."""
    from fiber_amd.es import conv_policy, philox_ref
    from fiber_amd.es.engine import make_env_params

    cfg = conv_policy.ConvESConfig(pop_per_gpu=2, horizon=3)
    cpu = torch.device("cpu")
    theta = conv_policy.init_conv_theta(cfg.seed, cpu)
    env_A, env_B = make_env_params(cfg.seed, cpu)
    gtab = conv_policy.make_gtab(cfg.seed, cpu)
    real = conv_policy.conv_rollout_reference(
        theta, cfg.sigma, cfg.seed, 0, cfg.horizon, [0, 1], env_A, env_B,
        gtab)
    s0 = torch.from_numpy(philox_ref.env_init_state(cfg.seed, 0, 16))
    for a in range(6):
        s = s0.clone()
        racc = torch.zeros(16)
        force = torch.full((16,), (a - 2.5) * 0.4)
        for _ in range(cfg.horizon):
            drive = torch.tanh(s @ env_A.T)
            snew = 0.97 * s + 0.08 * drive + 0.05 * env_B * force[:, None]
            racc += 1.0 - 0.1 * (snew * snew).sum(dim=1)
            s = snew
        delta = (real - float(racc.mean())).abs().max()
        print("constant action %d: fitness %.5f, |delta| to the real "
              "policy's %.5f/%.5f = %.5f (tolerance 5e-2)"
              % (a, float(racc.mean()), float(real[0]), float(real[1]),
                 float(delta)))
