"""GPU numerics tests for the ConvNet-policy ES pipeline."""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

if torch.cuda.is_available():
    from fiber_amd import ops
    from fiber_amd.es import conv_policy
    from fiber_amd.es.conv_policy import (
        ConvESConfig,
        ConvESEngine,
        conv_rollout_reference,
    )


@requires_gpu
class TestConvPipeline:
    def test_perturb_matches_reference(self):
        from fiber_amd.es import philox_ref

        o = ops._require_ops()
        device = torch.device("cuda")
        theta = conv_policy.init_conv_theta(11, device)
        pop = 4
        wpert = torch.empty(pop, o.NP_CONV_PAD, dtype=torch.bfloat16,
                            device=device)
        iterp = torch.zeros(1, dtype=torch.int32, device=device)
        w3_fp8 = torch.empty(pop, 256 * 2592, dtype=torch.uint8,
                             device=device)
        w1_fp8 = torch.empty(pop, 16 * 256, dtype=torch.uint8,
                             device=device)
        o.es_perturb(theta.data_ptr(), conv_policy.NP_CONV, o.NP_CONV_PAD,
                     0.02, 11, iterp.data_ptr(), 0, pop, wpert.data_ptr(),
                     w3_fp8.data_ptr(), w1_fp8.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for m in (0, 1, 3):
            eps = torch.from_numpy(
                philox_ref.noise_for_pair(11, 0, m // 2,
                                          conv_policy.NP_CONV)
            )
            sgn = -0.02 if m % 2 else 0.02
            want = (theta.cpu() + sgn * eps).to(torch.bfloat16).float()
            got = wpert[m, : conv_policy.NP_CONV].cpu().float()
            # device libm (sinf/cosf, fma contraction) differs from numpy
            # by ~1 ulp fp32, which can flip the bf16 rounding of a few
            # of the 677k values — require near-total agreement instead
            # of bitwise equality.
            close = torch.isclose(got, want, atol=1e-3, rtol=2e-2)
            frac = close.float().mean().item()
            assert frac > 0.9999, frac
            assert (got - want).abs().max().item() < 5e-3

    def test_rollout_vs_fp32_reference(self):
        """Coarse; the chain is checked step by step in
        tests/gpu/test_conv_rollout_chain_gpu.py."""
        device = torch.device("cuda")
        cfg = ConvESConfig(pop_per_gpu=2, horizon=3)
        eng = ConvESEngine(cfg, ctx=None, device=device)
        fit = eng.rollout(0)
        torch.cuda.synchronize()
        ref = conv_rollout_reference(
            eng.theta, cfg.sigma, cfg.seed, 0, cfg.horizon, [0, 1],
            eng.env_A, eng.env_B, eng.gtab,
        )
        err = (fit.cpu() - ref).abs().max().item()
        assert err < 5e-2, (fit.cpu(), ref)

    def test_engine_step(self):
        device = torch.device("cuda")
        cfg = ConvESConfig(pop_per_gpu=8, horizon=4)
        eng = ConvESEngine(cfg, ctx=None, device=device)
        stats = eng.step()
        torch.cuda.synchronize()
        assert stats["grad_norm"] > 0
        assert stats["rollouts"] == 8 * 16
        stats2 = eng.step()
        assert stats2["fitness_mean"] == stats2["fitness_mean"]  # not NaN

    def test_rollout_deterministic(self):
        device = torch.device("cuda")
        cfg = ConvESConfig(pop_per_gpu=4, horizon=4)
        eng = ConvESEngine(cfg, ctx=None, device=device)
        f1 = eng.rollout(5).clone()
        f2 = eng.rollout(5).clone()
        torch.cuda.synchronize()
        assert torch.equal(f1, f2)


@requires_gpu
class TestGraphEquivalence:
    def test_graph_replay_matches_eager(self):
        """The hipGraph-replayed rollout must produce bitwise-identical
        fitness to eager kernel launches."""
        device = torch.device("cuda")
        cfg = ConvESConfig(pop_per_gpu=16, horizon=6)
        eager = ConvESEngine(cfg, ctx=None, device=device)
        eager.use_graph = False
        f_eager = eager.rollout(2).clone()
        graphed = ConvESEngine(cfg, ctx=None, device=device)
        f_graph = graphed.rollout(2).clone()
        torch.cuda.synchronize()
        assert graphed._graph is not None, "graph capture did not engage"
        assert torch.equal(f_eager, f_graph)
