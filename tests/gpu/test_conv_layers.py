"""Layer-by-layer GPU tests of the ConvNet-policy kernels against the
fp64 references of fiber_amd/es/conv_reference.py.

Every MFMA layer is checked on its own, fed with what the GPU itself
produced for the layer before (or with a hand-made input), under the
per-element criterion derived in conv_reference.py: no tolerance here is
fitted to a kernel's output and no element is skipped.  The CPU side
(tests/test_conv_reference.py) shows that criterion rejects transposed
taps, swapped/dropped K-tiles, shifted biases, member/env mix-ups and a
double rounding.

3 members = 48 envs: odd, so a member-stride error cannot alias.
"""

import numpy as np
import pytest
import torch

from fiber_amd.es import conv_reference as cr

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

if torch.cuda.is_available():
    from fiber_amd import ops
    from fiber_amd.es import conv_policy, philox_ref
    from fiber_amd.es.engine import make_env_params

M = 3
E = M * cr.CENV
SENT16 = 0x5A5A  # bf16 1.5e16: no tanh output
SENT8 = 0x7F     # e4m3 NaN: no tanh output
N1, N2, N3 = 400 * 16, 2592, 256


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cuda(p, *names):
    return {k: p[k].cuda().contiguous() for k in names}


def _outputs(nenv_rows):
    """Sentinel-filled act1/act2/act3 with room for nenv_rows env rows."""
    dev = torch.device("cuda")
    a1 = torch.full((nenv_rows, N1), SENT16, dtype=torch.int16, device=dev)
    a2 = torch.full((nenv_rows, N2), SENT8, dtype=torch.uint8, device=dev)
    a3 = torch.full((nenv_rows, N3), SENT16, dtype=torch.int16, device=dev)
    return a1, a2, a3


def _bf(t_i16):
    return t_i16.cpu().view(torch.bfloat16)


def _per_env(b):
    return b.repeat_interleave(cr.CENV, dim=0)


def _forward(p, nmembers=M, first_member=0, rows=E + 1):
    """One conv_forward over members [first_member, first_member +
    nmembers) of policy p, into fresh sentinel buffers of `rows` env rows
    (base pointers advanced the way ConvESEngine._rollout_half does)."""
    o = ops._require_ops()
    d = _cuda(p, "wpert", "w1_fp8", "w3_fp8", "state", "gtab", "znoise")
    a1, a2, a3 = _outputs(rows)
    m0, e0 = first_member, first_member * cr.CENV
    o.conv_forward(d["wpert"][m0:].data_ptr(), d["w3_fp8"][m0:].data_ptr(),
                   d["w1_fp8"][m0:].data_ptr(), d["state"][e0:].data_ptr(),
                   d["gtab"].data_ptr(), d["znoise"].data_ptr(),
                   a1[e0:].data_ptr(), a2[e0:].data_ptr(),
                   a3[e0:].data_ptr(), nmembers, _stream())
    torch.cuda.synchronize()
    return a1.cpu(), a2.cpu(), a3.cpu()


@pytest.fixture(scope="module")
def pol():
    return cr.random_policy(M, 20241)


@pytest.fixture(scope="module")
def fwd(pol):
    return _forward(pol)


@requires_gpu
class TestForwardRandom:
    """1. conv_forward on random data, each layer against the fp64
    reference of the GPU's own previous layer."""

    def test_act1(self, pol, fwd):
        v = cr.policy_views(pol)
        obs = cr.obs_reference(pol["znoise"], pol["state"], pol["gtab"])
        pre, absdot = cr.layer1_reference(obs, pol["w1_fp8"], v["b1"])
        assert float(pre.abs().max()) <= 4.0
        got = fwd[0][:E].view(torch.bfloat16).reshape(E, 400, 16)
        bias = _per_env(v["b1"])[:, None, :]
        print("act1 worst (err - ulp/2)/slack = %.4f" % cr.worst_margin(
            got, pre, absdot, cr.K_LAYER1, "bf16", bias))
        cr.check_layer(got, pre, absdot, cr.K_LAYER1, "bf16", bias,
                       what="act1")

    def test_act2(self, pol, fwd):
        v = cr.policy_views(pol)
        act1 = fwd[0][:E].view(torch.bfloat16)
        pre, absdot = cr.layer2_reference(act1, v["w2"], v["b2"])
        assert float(pre.abs().max()) <= 4.0
        got = fwd[1][:E].reshape(E, 81, 32)
        bias = _per_env(v["b2"])[:, None, :]
        print("act2 worst (err - ulp/2)/slack = %.4f" % cr.worst_margin(
            got, pre, absdot, cr.K_LAYER2, "e4m3", bias))
        cr.check_layer(got, pre, absdot, cr.K_LAYER2, "e4m3", bias,
                       what="act2")

    def test_act3(self, pol, fwd):
        v = cr.policy_views(pol)
        pre, absdot = cr.fc_reference(fwd[1][:E], pol["w3_fp8"], v["b3"])
        assert float(pre.abs().max()) <= 4.0
        got = fwd[2][:E].view(torch.bfloat16)
        bias = _per_env(v["b3"])
        print("act3 worst (err - ulp/2)/slack = %.4f" % cr.worst_margin(
            got, pre, absdot, cr.K_FC, "bf16", bias))
        cr.check_layer(got, pre, absdot, cr.K_FC, "bf16", bias, what="act3")

    def test_padding_and_ownership(self, fwd):
        """2. The guard env row after each buffer is untouched (81->96
        padded N lanes of layer 2, the p+3 < 84*84 obs loop, the last
        member's stores) and every element inside was written."""
        a1, a2, a3 = fwd
        assert bool((a1[E:] == SENT16).all())
        assert bool((a2[E:] == SENT8).all())
        assert bool((a3[E:] == SENT16).all())
        assert not bool((a1[:E] == SENT16).any())
        assert not bool((a2[:E] == SENT8).any())
        assert not bool((a3[:E] == SENT16).any())

    def test_slice_invariance(self, pol, fwd):
        """5. nmembers=1 with every base pointer advanced to member 1
        equals member 1 of the full run bit for bit; znoise is shared."""
        a1, a2, a3 = _forward(pol, nmembers=1, first_member=1)
        sl = slice(cr.CENV, 2 * cr.CENV)
        for got, full, sent in ((a1, fwd[0], SENT16), (a2, fwd[1], SENT8),
                                (a3, fwd[2], SENT16)):
            assert torch.equal(got[sl], full[sl])
            assert bool((got[:cr.CENV] == sent).all())
            assert bool((got[2 * cr.CENV:] == sent).all())


@requires_gpu
class TestExactArithmetic:
    """3. Inputs on power-of-two grids (cr.exact_policy: every partial
    sum is an fp32 number, in any order), through the single-layer
    launchers; the criterion runs with slack = TAU only."""

    @pytest.fixture(scope="class")
    def exact(self):
        return cr.exact_policy(M, 777)

    @staticmethod
    def _report(name, got, pre, fmt):
        err, half_ulp, _ = cr.layer_errors(got, pre, None, 0, fmt)
        print("%s exact: max(|got - tanh p| - ulp/2) = %.3e (TAU %.3e)"
              % (name, float((err - half_ulp).max()), cr.TAU))

    def test_layer1(self, exact):
        o = ops._require_ops()
        v = cr.policy_views(exact)
        obs = cr.obs_reference(exact["znoise"], exact["state"],
                               exact["gtab"])
        pre, absdot = cr.layer1_reference(obs, exact["w1_fp8"], v["b1"])
        # products on the 2^-8 grid, sum|a*b| + |bias| < 2^16
        assert float(absdot.max()) + 1 < 2.0 ** 16
        assert float(pre.abs().max()) <= 4.0
        d = _cuda(exact, "wpert", "w1_fp8", "state", "gtab", "znoise")
        a1, _, _ = _outputs(E + 1)
        o.conv_layer1(d["wpert"].data_ptr(), d["w1_fp8"].data_ptr(),
                      d["state"].data_ptr(), d["gtab"].data_ptr(),
                      d["znoise"].data_ptr(), a1.data_ptr(), M, _stream())
        torch.cuda.synchronize()
        assert bool((a1[E:] == SENT16).all())
        got = _bf(a1[:E]).reshape(E, 400, 16)
        self._report("layer1", got, pre, "bf16")
        cr.check_layer(got, pre, None, 0, "bf16", what="exact layer1")

    def test_layer2(self, exact):
        o = ops._require_ops()
        v = cr.policy_views(exact)
        pre, absdot = cr.layer2_reference(exact["act1"], v["w2"], v["b2"])
        assert float(absdot.max()) + 1 < 2.0 ** 16  # grid 2^-8
        assert float(pre.abs().max()) <= 4.0
        d = _cuda(exact, "wpert", "act1")
        _, a2, _ = _outputs(E + 1)
        o.conv_layer2(d["wpert"].data_ptr(), d["act1"].data_ptr(),
                      a2.data_ptr(), M, _stream())
        torch.cuda.synchronize()
        assert bool((a2[E:] == SENT8).all())
        got = a2[:E].cpu().reshape(E, 81, 32)
        self._report("layer2", got, pre, "e4m3")
        cr.check_layer(got, pre, None, 0, "e4m3", what="exact layer2")

    def test_fc(self, exact):
        o = ops._require_ops()
        v = cr.policy_views(exact)
        pre, absdot = cr.fc_reference(exact["act2"], exact["w3_fp8"],
                                      v["b3"])
        # terms are multiples of 2^-9 (finer than the 2^-12 needed) and
        # sum|a*b| < 16: every partial sum has at most 14 bits
        assert float(absdot.max()) < 16.0
        assert float(pre.abs().max()) <= 4.0
        d = _cuda(exact, "wpert", "w3_fp8", "act2")
        _, _, a3 = _outputs(E + 1)
        o.conv_fc(d["wpert"].data_ptr(), d["w3_fp8"].data_ptr(),
                  d["act2"].data_ptr(), a3.data_ptr(), M, _stream())
        torch.cuda.synchronize()
        assert bool((a3[E:] == SENT16).all())
        got = _bf(a3[:E])
        self._report("fc", got, pre, "bf16")
        cr.check_layer(got, pre, None, 0, "bf16", what="exact fc")


W1_TAPS = [(0, 0, 0, 0), (15, 7, 7, 3), (5, 0, 7, 1),
           (9, 7, 0, 2), (3, 2, 5, 0), (12, 4, 1, 3)]
W2_TAPS = [(0, 0, 0, 0), (31, 3, 3, 15), (7, 0, 3, 8),
           (16, 3, 0, 7), (20, 1, 2, 9), (11, 2, 1, 3)]


def _tap_read_instead(got, x, bias, k, stride, nout):
    """Which (ky, kx, ic) tap explains channel values got[E][oy][ox] best
    (for the failure message)."""
    best = None
    for ky in range(k):
        for kx in range(k):
            for ic in range(x.shape[3]):
                tap = x[:, ky:ky + stride * nout:stride,
                        kx:kx + stride * nout:stride, ic]
                err = float((torch.tanh(tap + bias) - got).abs().max())
                if best is None or err < best[0]:
                    best = (err, (ky, kx, ic))
    return "closest tap (ky, kx, ic) = %s, max err %.3g" % (best[1], best[0])


@requires_gpu
class TestOneHot:
    """4. A single 1.0 in W1 / W2: the output channel must be
    tanh(one input tap + bias), exact in fp32 (slack = TAU), and every
    other channel tanh(bias).  Member m carries its own tap."""

    @pytest.mark.parametrize("first", [0, 3])
    def test_w1(self, pol, first):
        o = ops._require_ops()
        taps = W1_TAPS[first:first + M]
        v = cr.policy_views(pol)
        wpert = torch.zeros_like(pol["wpert"])
        wpert[:, cr.OFF_B1:cr.OFF_W2] = v["b1"]
        w1 = torch.zeros(M, 16, 8, 8, 4)
        for m, (oc, ky, kx, ic) in enumerate(taps):
            w1[m, oc, ky, kx, ic] = 1.0
        w1b = cr.e4m3_bytes(w1.reshape(M, -1))
        obs = cr.obs_reference(pol["znoise"], pol["state"],
                               pol["gtab"]).double()
        # obs is on the 2^-9 grid below 4, b1 has 8 significant bits at
        # >= 2^-4: obs + b1 is an fp32 number
        pre = _per_env(v["b1"].double())[:, None, :].repeat(1, 400, 1)
        for m, (oc, ky, kx, ic) in enumerate(taps):
            sl = slice(m * 16, m * 16 + 16)
            pre[sl, :, oc] += obs[sl, ky:ky + 80:4, kx:kx + 80:4,
                                  ic].reshape(16, 400)
        assert float(pre.abs().max()) <= 4.0
        d = _cuda(pol, "state", "gtab", "znoise")
        a1, _, _ = _outputs(E + 1)
        o.conv_layer1(wpert.cuda().data_ptr(), w1b.cuda().data_ptr(),
                      d["state"].data_ptr(), d["gtab"].data_ptr(),
                      d["znoise"].data_ptr(), a1.data_ptr(), M, _stream())
        torch.cuda.synchronize()
        got = _bf(a1[:E]).reshape(E, 400, 16)
        ok = cr.check_layer(got, pre, None, 0, "bf16", raise_on_fail=False)
        if not bool(ok.all()):
            msgs = []
            for m, (oc, ky, kx, ic) in enumerate(taps):
                sl = slice(m * 16, m * 16 + 16)
                if not bool(ok[sl, :, oc].all()):
                    msgs.append("member %d tap %s: %s" % (
                        m, (oc, ky, kx, ic), _tap_read_instead(
                            got[sl, :, oc].double().reshape(16, 20, 20),
                            obs[sl], float(v["b1"][m, oc]), 8, 4, 20)))
            print("\n".join(msgs))
            cr.check_layer(got, pre, None, 0, "bf16", what="one-hot W1")

    @pytest.mark.parametrize("first", [0, 3])
    def test_w2(self, pol, first):
        o = ops._require_ops()
        taps = W2_TAPS[first:first + M]
        v = cr.policy_views(pol)
        gen = torch.Generator().manual_seed(99 + first)
        # multiples of 1/256 in (-1, 1): exact in bf16, and act1 + b2
        # (b2 on a grid no finer than 2^-11) is an fp32 number
        act1 = (torch.randint(-255, 256, (E, 20, 20, 16), generator=gen)
                .float() / 256)
        wpert = torch.zeros(M, cr.NP_CONV_PAD)
        wpert[:, cr.OFF_B2:cr.OFF_W3] = v["b2"].float()
        w2 = torch.zeros(M, 32, 4, 4, 16)
        for m, (oc, ky, kx, ic) in enumerate(taps):
            w2[m, oc, ky, kx, ic] = 1.0
        wpert[:, cr.OFF_W2:cr.OFF_B2] = w2.reshape(M, -1)
        pre = _per_env(v["b2"].double())[:, None, :].repeat(1, 81, 1)
        for m, (oc, ky, kx, ic) in enumerate(taps):
            sl = slice(m * 16, m * 16 + 16)
            pre[sl, :, oc] += act1[sl, ky:ky + 18:2, kx:kx + 18:2,
                                   ic].double().reshape(16, 81)
        _, a2, _ = _outputs(E + 1)
        a1d = act1.to(torch.bfloat16).cuda().contiguous()
        assert torch.equal(a1d.cpu().float(), act1)
        o.conv_layer2(wpert.to(torch.bfloat16).cuda().data_ptr(),
                      a1d.data_ptr(), a2.data_ptr(), M, _stream())
        torch.cuda.synchronize()
        got = a2[:E].cpu().reshape(E, 81, 32)
        ok = cr.check_layer(got, pre, None, 0, "e4m3", raise_on_fail=False)
        if not bool(ok.all()):
            msgs = []
            for m, (oc, ky, kx, ic) in enumerate(taps):
                sl = slice(m * 16, m * 16 + 16)
                if not bool(ok[sl, :, oc].all()):
                    msgs.append("member %d tap %s: %s" % (
                        m, (oc, ky, kx, ic), _tap_read_instead(
                            cr.e4m3_val(got[sl, :, oc]).reshape(16, 9, 9),
                            act1[sl].double(), float(v["b2"][m, oc]),
                            4, 2, 9)))
            print("\n".join(msgs))
            cr.check_layer(got, pre, None, 0, "e4m3", what="one-hot W2")


@requires_gpu
class TestHeadEnv:
    """6. conv_head_env against the fp64 reference."""

    TOL = 2.0 ** -18  # a handful of fp32 roundings below 4, + 0.08 TAU

    def _run(self, wpert, act3, state, racc, env_A, env_B):
        o = ops._require_ops()
        st = state.cuda().contiguous()
        ra = racc.cuda().contiguous()
        o.conv_head_env(wpert.cuda().data_ptr(),
                        act3.cuda().contiguous().data_ptr(), M,
                        env_A.data_ptr(), env_B.data_ptr(), st.data_ptr(),
                        ra.data_ptr(), _stream())
        torch.cuda.synchronize()
        return st.cpu(), ra.cpu()

    def _data(self):
        # seed chosen on the CPU so that test_random's gap precondition
        # holds for all 48 envs (smallest gap is 43x what it requires)
        gen = torch.Generator().manual_seed(38)
        act3 = (torch.rand(E, 256, generator=gen) * 2 - 1).to(
            torch.bfloat16)  # distinct per env
        state = torch.rand(E, 4, generator=gen) * 2 - 1
        racc = torch.full((E,), 3.25)  # non-zero: "+=" is tested, not "="
        env_A, env_B = make_env_params(4321, torch.device("cuda"))
        return act3, state, racc, env_A, env_B

    def test_random(self, pol):
        v = cr.policy_views(pol)  # distinct W4 / b4 per member
        act3, state, racc, env_A, env_B = self._data()
        logits, action, snew, racc_new, bound = cr.head_env_reference(
            act3, v["w4"], v["b4"], state, env_A.cpu(), env_B.cpu(), racc)
        # precondition, zero envs exempt: the top-two gap of every env
        # exceeds 4x the worst-case fp32 logit error
        top2 = torch.topk(logits, 2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
        assert bool((gap > 4 * bound.max(dim=1).values).all())
        assert len(set(action.tolist())) >= 4
        # the six forces must be distinguishable in the state update
        assert float((0.02 * env_B.cpu().abs()).max()) > 100 * self.TOL
        st, ra = self._run(pol["wpert"], act3, state, racc, env_A, env_B)
        assert float((st.double() - snew).abs().max()) <= self.TOL
        assert float((ra.double() - racc_new).abs().max()) <= self.TOL

    def test_exact_ties(self, pol):
        act3, state, racc, env_A, env_B = self._data()
        wpert = torch.zeros_like(pol["wpert"])  # W4 = 0
        b4 = torch.tensor([[.5, .5, .5, .5, .5, .5], [0, 0, 2, 0, 2, 0],
                           [0, 0, 0, 0, 0, 3]])
        wpert[:, cr.OFF_B4:cr.NP_CONV] = b4.to(torch.bfloat16)
        _, action, snew, racc_new, _ = cr.head_env_reference(
            act3, torch.zeros(M, 6 * 256), b4, state, env_A.cpu(),
            env_B.cpu(), racc)
        assert action.reshape(M, 16).tolist() == \
            [[0] * 16, [2] * 16, [5] * 16]
        st, ra = self._run(wpert, act3, state, racc, env_A, env_B)
        assert float((st.double() - snew).abs().max()) <= self.TOL
        assert float((ra.double() - racc_new).abs().max()) <= self.TOL


# theta values planted for the sigma = 0 comparison: e4m3 midpoints (ties
# to even), subnormals, signed zeros, and the top of the finite range
# (|x| <= 416 keeps overflow semantics out of it)
PLANTED = [1.0625, 1.1875, -1.0625, -1.1875, 2.0 ** -10, 3 * 2.0 ** -10,
           -3 * 2.0 ** -10, 7.5 * 2.0 ** -9, 2.0 ** -9, 3 * 2.0 ** -9,
           -5 * 2.0 ** -9, 7 * 2.0 ** -9, 0.0, -0.0, 400.0, -400.0, 416.0,
           -416.0, 368.0, 415.5, 2.0 ** -6, 0.0166]


@requires_gpu
class TestPerturbOutputs:
    """7. es_perturb's fp8 side outputs, the weights conv1 and fc
    actually consume."""

    SEED = 11

    def _perturb(self, theta, sigma, iteration, member_offset, pop):
        o = ops._require_ops()
        dev = torch.device("cuda")
        wpert = torch.full((pop, o.NP_CONV_PAD), SENT16, dtype=torch.int16,
                           device=dev)
        w3 = torch.full((pop + 1, 256 * 2592), SENT8, dtype=torch.uint8,
                        device=dev)
        w1 = torch.full((pop + 1, 4096), SENT8, dtype=torch.uint8,
                        device=dev)
        iterp = torch.full((1,), iteration, dtype=torch.int32, device=dev)
        o.es_perturb(theta.cuda().data_ptr(), cr.NP_CONV, o.NP_CONV_PAD,
                     sigma, self.SEED, iterp.data_ptr(), member_offset, pop,
                     wpert.data_ptr(), w3.data_ptr(), w1.data_ptr(),
                     _stream())
        torch.cuda.synchronize()
        assert bool((w3[pop:] == SENT8).all())
        assert bool((w1[pop:] == SENT8).all())
        return wpert.cpu(), w3[:pop].cpu(), w1[:pop].cpu()

    def test_sigma_zero_is_bitwise(self):
        theta = conv_policy.init_conv_theta(self.SEED, torch.device("cpu"))
        planted = torch.tensor(PLANTED, dtype=torch.float32)
        n = len(PLANTED)
        for off in (0, 4096 - n, cr.OFF_W3, cr.OFF_B3 - n, cr.OFF_B1,
                    cr.OFF_W4):
            theta[off:off + n] = planted
        wpert, w3, w1 = self._perturb(theta, 0.0, 3, 0, 2)
        # theta + 0 * z keeps theta, except that IEEE -0 + +0 = +0: the
        # sign of an exact -0 in theta follows the sign of z.  Only there
        # is the sign bit left out of the comparison.
        neg0 = (theta == 0) & torch.signbit(theta)
        assert int(neg0.sum()) == 6
        want16 = theta.to(torch.bfloat16).view(torch.int16)
        want3 = cr.e4m3_bytes(theta[cr.OFF_W3:cr.OFF_B3])
        want1 = cr.e4m3_bytes(theta[:4096])
        for m in (0, 1):
            for got, want, z, mask in (
                (wpert[m, :cr.NP_CONV], want16, neg0, 0x7FFF),
                (w3[m], want3, neg0[cr.OFF_W3:cr.OFF_B3], 0x7F),
                (w1[m], want1, neg0[:4096], 0x7F),
            ):
                assert torch.equal(got[~z], want[~z]), (
                    m, torch.nonzero(got != want)[:8].tolist())
                assert bool(((got[z] & mask) == 0).all())
            # the 16-byte alignment pad is nobody's to write
            assert bool((wpert[m, cr.NP_CONV:] == SENT16).all())

    def test_sigma_nonzero_roundings_agree(self):
        theta = conv_policy.init_conv_theta(self.SEED, torch.device("cpu"))
        sigma, it = 0.02, 3
        wpert, w3, w1 = self._perturb(theta, sigma, it, 4, 2)
        bfv = wpert[:, :cr.NP_CONV].view(torch.bfloat16).double()
        for m in (0, 1):
            # two roundings of the same fp32 value
            for f8, b in ((w3[m], bfv[m, cr.OFF_W3:cr.OFF_B3]),
                          (w1[m], bfv[m, :4096])):
                d = (cr.e4m3_val(f8) - b).abs()
                assert bool((d <= 0.5 * cr.ulp_e4m3(b)
                             + 0.5 * cr.ulp_bf16(b)).all())
        # antithetic pair: wpert+ + wpert- = 2 theta within one bf16 ulp
        # each
        d = (bfv[0] + bfv[1] - 2 * theta.double()).abs()
        assert bool((d <= cr.ulp_bf16(bfv[0]) + cr.ulp_bf16(bfv[1])).all())
        assert not torch.equal(wpert[0], wpert[1])
        # members 4, 5 are pair 2 of this iteration (margin: device libm
        # vs numpy, as in test_perturb_matches_reference)
        eps = torch.from_numpy(philox_ref.noise_for_pair(
            self.SEED, it, 2, cr.NP_CONV)).double()
        assert float((bfv[0] - (theta + sigma * eps)).abs().max()) < 5e-3
        assert float((bfv[1] - (theta - sigma * eps)).abs().max()) < 5e-3


@requires_gpu
class TestNoiseAndInit:
    """8. conv_noisegen and conv_env_init against the numpy Philox
    mirror."""

    SEED = 4321

    @pytest.mark.parametrize("t,iteration", [(0, 0), (5, 7)])
    def test_noisegen_bitwise(self, t, iteration):
        o = ops._require_ops()
        dev = torch.device("cuda")
        nb = 84 * 84 * 4
        zn = torch.full((17, nb), SENT8, dtype=torch.uint8, device=dev)
        iterp = torch.full((1,), iteration, dtype=torch.int32, device=dev)
        o.conv_noisegen(self.SEED, iterp.data_ptr(), t, 16, zn.data_ptr(),
                        _stream())
        torch.cuda.synchronize()
        zn = zn.cpu()
        assert bool((zn[16] == SENT8).all())
        p = np.arange(84 * 84, dtype=np.uint32)
        for e in range(16):
            # integer -> float32 conversion and one float32 product: the
            # numpy mirror is exact, so are the e4m3 bytes
            z = philox_ref.uniform4(self.SEED, iteration,
                                    np.uint32(e) * np.ones_like(p), p,
                                    np.uint32(0x45530003), np.uint32(t))
            want = cr.e4m3_bytes(torch.from_numpy(
                (np.float32(0.52) * z).astype(np.float32))).reshape(-1)
            assert torch.equal(zn[e, -16:], want[-16:]), (e, "last quad")
            assert torch.equal(zn[e], want), (
                e, torch.nonzero(zn[e] != want)[:8].tolist())

    def test_env_init(self):
        o = ops._require_ops()
        dev = torch.device("cuda")
        state = torch.full((E + 1, 4), 7.0, device=dev)
        racc = torch.full((M + 1, 16), 7.0, device=dev)
        iterp = torch.full((1,), 7, dtype=torch.int32, device=dev)
        o.conv_env_init(self.SEED, iterp.data_ptr(), M, state.data_ptr(),
                        racc.data_ptr(), _stream())
        torch.cuda.synchronize()
        state, racc = state.cpu(), racc.cpu()
        assert bool((racc[:M] == 0).all()) and bool((racc[M] == 7).all())
        assert bool((state[E] == 7).all())
        want = torch.from_numpy(philox_ref.env_init_state(self.SEED, 7, 16))
        for m in range(M):
            assert torch.equal(state[m * 16:m * 16 + 16], state[:16])
        # device libm margin, as in
        # test_es_grad_regenerates_reference_noise
        assert float((state[:16] - want).abs().max()) < 1e-5
