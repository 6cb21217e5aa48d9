"""Deep GA with safe mutations through output gradients (Lehman et al., "Safe
Mutations for Deep and Recurrent Neural Networks through Output Gradients",
the SM-G family): ``GAEngine`` with a mutation step per parent and per
parameter instead of one scalar.

Before a generation's rollout, ``sm_steps`` runs one forward and one
backward pass of every parent on a fixed probe batch of 64 normalised
observations and returns ``steps[t][j] = sigma / max(sens[t][j], s_min)``,
where ``sens`` is the sensitivity of the two logits to weight ``j``: the
2-norm over the outputs of the batch mean of ``|d logit_k / d theta_j|``
(``mode="abs"``, SM-G-ABS) or of the signed derivative (``mode="sum"``,
SM-G-SUM).  A child of parent ``t`` is ``parent + steps[t] * z`` with
``GAEngine``'s draw ``z``, so a weight the outputs hardly feel moves far and
one they hinge on moves little.

``sigma`` keeps its name but not its meaning: it is the step of a weight with
unit sensitivity (``b3`` has exactly that), not the step of every weight.
With ``init_theta`` and the default probe the median sensitivity is about
0.055 in abs mode, so the typical step is some 20 sigma; the default sigma,
0.001, makes the median step GAConfig's 0.02 (the sweep in
profiles/safe_mutation.md; every sigma tried there learned the task equally
well).  ``s_min`` caps the step at ``sigma / s_min``.

SM-G-SUM washes out: signed per-sample gradients cancel over the batch, the
median sensitivity of the same policy is about 0.005 and three quarters of
the parameters sit under ``s_min = 0.01`` and get ``100 sigma``.  It is here
for completeness; abs is the default.

The seed-chain encoding survives because a step depends only on the parent's
weights and the fixed probe.  One generation of a decode is ``ga_survivors_sm
(rows, sm_steps(rows), ...)``: the kernels the run itself used, generation by
generation, so ``decode(genome(t))`` equals ``parents[t]`` bit for bit.  A
checkpoint stores the chains, ``theta0``, the probe, ``mode`` and ``s_min``.

Out of scope: MAP-Elites with safe mutations, the second-order SM-G-SO, a
probe taken from the parent's own rollout (it would break decoding from
chains alone), normalising the steps to a target RMS, and everything
``GAEngine`` leaves out.
"""

import dataclasses
import math

import numpy as np
import torch

from .. import ops, tracing
from . import philox_ref
from .ga import GAConfig, GAEngine

TAG_SM_PROBE = np.uint32(0x45530006)
PROBE_CLIP = 5.0


def default_probe(seed):
    """float32 [64][4]: standard normals clipped to +-5, row ``b`` the
    Philox draw keyed by (seed, 0) at counter (b, 0, TAG_SM_PROBE, 0)."""
    rows = np.arange(ops.SM_PROBE_ROWS, dtype=np.uint32)
    z = philox_ref.normal4(np.uint32(int(seed) & 0xFFFFFFFF), np.uint32(0),
                           rows, np.uint32(0), TAG_SM_PROBE, np.uint32(0))
    return np.clip(z[:, : ops.OBS_DIM], -PROBE_CLIP, PROBE_CLIP).astype(
        np.float32)


def check_probe(probe):
    """A user probe as a float32 CPU tensor [64][4]; ValueError unless it
    is that shape and dtype and finite."""
    if not torch.is_tensor(probe):
        probe = torch.from_numpy(np.asarray(probe))
    if probe.dtype != torch.float32:
        raise ValueError("probe must be float32, got %s" % probe.dtype)
    if tuple(probe.shape) != (ops.SM_PROBE_ROWS, ops.OBS_DIM):
        raise ValueError("probe must be [%d, %d], got %s"
                         % (ops.SM_PROBE_ROWS, ops.OBS_DIM,
                            tuple(probe.shape)))
    probe = probe.detach().cpu().contiguous().clone()
    if not torch.isfinite(probe).all():
        raise ValueError("probe must be finite")
    return probe


@dataclasses.dataclass
class SafeGAConfig(GAConfig):
    # the step of a weight with unit sensitivity (see the module docstring).
    # 0.001 gives a median step of 0.02, GAConfig's sigma, in abs mode
    # (the sweep in profiles/safe_mutation.md)
    sigma: float = 0.001
    mode: str = "abs"             # "abs" (SM-G-ABS) or "sum" (SM-G-SUM)
    s_min: float = 0.01           # sensitivity floor: step <= sigma / s_min

    def validate(self):
        """GAConfig's checks, and ValueError unless mode is "abs" or "sum"
        and s_min is finite and > 0."""
        super().validate()
        if self.mode not in ops.SM_MODES:
            raise ValueError("mode must be one of %r, got %r"
                             % (ops.SM_MODES, self.mode))
        if not 0.0 < self.s_min < math.inf:  # also refuses a NaN
            raise ValueError("s_min must be finite and > 0, got %r"
                             % self.s_min)


class SafeGAEngine(GAEngine):
    def __init__(self, config: SafeGAConfig, ctx=None, device=None,
                 env_params=None, probe=None):
        super().__init__(config, ctx=ctx, device=device,
                         env_params=env_params)
        if probe is None:
            probe = torch.from_numpy(default_probe(config.seed))
        else:
            probe = check_probe(probe)
        # uploaded once; part of state_dict()
        self.probe = probe.to(self.device).contiguous()

    def _steps(self, rows):
        cfg = self.cfg
        return ops.sm_steps(rows, self.probe, cfg.sigma, cfg.s_min, cfg.mode)

    # -- one generation ------------------------------------------------------
    def step(self):
        """GAEngine.step with one sm_steps launch in front and the step rows
        in place of sigma."""
        cfg = self.cfg
        g = self.generation
        T_cur = self.parents.shape[0]
        n_elite = min(cfg.n_elite, T_cur)

        parent_idx, slot = ops.ga_parents(cfg.seed, g, cfg.pop, n_elite,
                                          T_cur, self.device)
        with tracing.range("safe_ga.steps"):
            steps = self._steps(self.parents)
        with tracing.range("safe_ga.rollout"):
            fitness, obs_stat = ops.ga_rollout_mlp_sm(
                self.parents, steps, parent_idx, slot, cfg.seed, g,
                cfg.horizon, self.obs_mu, self.obs_nu, self.env_A,
                self.env_B)
        order = ops.ga_truncate(fitness, cfg.truncation)
        with tracing.range("safe_ga.survivors"):
            new_parents = ops.ga_survivors_sm(self.parents, steps,
                                              parent_idx, slot, order,
                                              cfg.seed, g)

        # seed chains of the survivors (plumbing: torch indexing)
        cap = self.lineage.shape[1]
        if g >= cap:
            cap *= 2
        chosen = order.long()
        lineage = torch.full((cfg.truncation, cap), -1, dtype=torch.int32,
                             device=self.device)
        lineage[:, :g] = self.lineage[parent_idx[chosen].long(), :g]
        lineage[:, g] = slot[chosen]

        self.parents, self.lineage = new_parents, lineage
        self.generation = g + 1
        self.last = {"fitness": fitness, "parent_idx": parent_idx,
                     "slot": slot, "order": order, "steps": steps}

        # running obs normalization (applied next generation)
        self.obs_sum += obs_stat[: cfg.obs_dim]
        self.obs_sumsq += obs_stat[cfg.obs_dim : 2 * cfg.obs_dim]
        self.obs_count += obs_stat[2 * cfg.obs_dim]
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()

        return {
            "fitness_mean": float(fitness.mean()),
            "fitness_max": float(fitness.max()),
            "elite_fitness": float(fitness[0]),
            "rollouts": cfg.pop * cfg.envs_per_member,
            "env_steps": cfg.pop * cfg.envs_per_member * cfg.horizon,
            "generation": self.generation,
        }

    # -- the compact encoding --------------------------------------------------
    def _fold(self, rows):
        """Weights [N][NPARAMS] of the chains ``rows`` (int32 [N][G] on the
        device): theta0, then per generation the step rows of the weights so
        far and ga_survivors_sm, ping-ponging two buffers."""
        N, G = rows.shape
        # a copy even for N = 1, where expand().contiguous() would be a view
        # of theta0 and the second generation would be written over it
        cur = self.theta0.unsqueeze(0).repeat(N, 1)
        if N == 0 or G == 0:
            return cur
        other = torch.empty_like(cur)
        ident = torch.arange(N, dtype=torch.int32, device=self.device)
        for c in range(G):
            slot = rows[:, c].contiguous()
            ops.ga_survivors_sm(cur, self._steps(cur), ident, slot, ident,
                                self.cfg.seed, c, out=other)
            cur, other = other, cur
        return cur

    def decode(self, lineage_rows):
        """Weights [N][NPARAMS] of the seed chains ``lineage_rows`` (as for
        GAEngine.decode), rebuilt from ``theta0`` with this engine's sigma,
        seed, mode, s_min and probe."""
        if not torch.is_tensor(lineage_rows):
            lineage_rows = torch.from_numpy(
                np.asarray(lineage_rows, dtype=np.int32))
        if lineage_rows.dim() == 1:
            lineage_rows = lineage_rows.unsqueeze(0)
        if lineage_rows.dim() != 2 \
                or not 1 <= lineage_rows.shape[0] <= ops.GA_ROWS_MAX:
            raise ValueError("lineage rows must be [N, G] with N in [1, %d], "
                             "got %s" % (ops.GA_ROWS_MAX,
                                         tuple(lineage_rows.shape)))
        return self._fold(lineage_rows.to(device=self.device,
                                          dtype=torch.int32).contiguous())

    # -- checkpoint / resume -------------------------------------------------
    def state_dict(self):
        """GAEngine's state and the probe; mode and s_min ride in the
        config."""
        state = super().state_dict()
        state["probe"] = self.probe.cpu()
        return state

    def load_state_dict(self, state):
        """Rebuild ``parents`` from the saved chains.  The checkpoint's
        sigma, seed, mode, s_min and probe must be this engine's (ValueError
        otherwise): the chains mean nothing under other steps."""
        if "lineage" not in state or "theta0" not in state \
                or "probe" not in state:
            raise ValueError("the checkpoint holds no seed chains or no "
                             "probe: it is not a SafeGAEngine's")
        saved = state["config"]
        for key in ("sigma", "seed", "mode", "s_min"):
            if key not in saved or saved[key] != getattr(self.cfg, key):
                raise ValueError("the checkpoint was written with %s = %r, "
                                 "this engine has %r"
                                 % (key, saved.get(key),
                                    getattr(self.cfg, key)))
        probe = state["probe"]
        if tuple(probe.shape) != tuple(self.probe.shape) \
                or not torch.equal(probe.cpu(), self.probe.cpu()):
            raise ValueError("the checkpoint was written with another probe")
        generation = int(state["generation"])
        lineage = state["lineage"]
        if lineage.dim() != 2 or lineage.shape[1] != generation \
                or not 1 <= lineage.shape[0] <= ops.GA_ROWS_MAX:
            raise ValueError("checkpoint lineage has shape %s at generation "
                             "%d" % (tuple(lineage.shape), generation))
        if tuple(state["theta0"].shape) != tuple(self.theta0.shape):
            raise ValueError("checkpoint theta0 has shape %s"
                             % (tuple(state["theta0"].shape),))
        self.theta0.copy_(state["theta0"].to(self.device))
        rows = lineage.to(device=self.device, dtype=torch.int32).contiguous()
        self.parents = self._fold(rows)
        cap = 8
        while cap < generation:
            cap *= 2
        self.lineage = torch.full((rows.shape[0], cap), -1,
                                  dtype=torch.int32, device=self.device)
        self.lineage[:, :generation] = rows
        self.generation = generation
        self.last = None
        self.obs_sum.copy_(state["obs_sum"].to(self.device))
        self.obs_sumsq.copy_(state["obs_sumsq"].to(self.device))
        self.obs_count.copy_(state["obs_count"].to(self.device))
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()
