"""Cost and effect of safe mutations against the plain Deep GA (MI355X only).

Timing, at the shapes of scripts/ga_rate.py, (pop 32768, truncation 1024,
horizon 256) and (pop 1024, truncation 32, horizon 200), in one process:

  GAEngine.step twice (A/A)            the run-to-run noise, measured first
  GAEngine.step / SafeGAEngine.step    ms per generation, abs mode
  sm_steps                             ms per launch, T = truncation rows
  ga_rollout_mlp / ga_rollout_mlp_sm   ms per launch (+ obs_stat_reduce)

The GA arm is this tree's GAEngine, whose code the safe-mutation kernels do
not touch.  The arms of a group alternate inside one process, each warmed up
and timed with device events around a batch of calls.  Before timing,
ga_rollout_mlp_sm with constant steps is checked against ga_rollout_mlp bit
for bit.

Learning (--learn), at tests/ga_cases.py's LEARN size (pop 256, truncation
16, horizon 32, 30 generations): plain GA over --ga-sigmas and both SM modes
over --sm-sigmas.  Per run: evaluate(iteration=0) of theta0 and of the final
theta, theta0 under the learned normaliser, the last elite fitness, and the
distribution over 256 children of the final parents of the mean |change of
the logits| on the probe (mlp_policy_forward of child and parent).

Nothing is asserted.  Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fiber_amd import ops
from fiber_amd.es import GAConfig, GAEngine, SafeGAConfig, SafeGAEngine

SHAPES = ((32768, 1024, 256), (1024, 32, 200))
LEARN = dict(pop=256, truncation=16, horizon=32)
LEARN_GENERATIONS = 30
CHILDREN = 256


def timed_ms(fn, inner):
    """Device-event time of ``inner`` back-to-back calls of fn, per call."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def interleaved(arms, repeats, inner, warmup):
    """{name: [ms per call, ...]}, arms alternating within each repeat."""
    for fn in arms.values():  # warm-up: code objects, allocator
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            out[name].append(timed_ms(fn, inner))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms), "spread_ms": max(ms) - min(ms),
            "repeats": len(ms)}


def compare(base, new):
    delta = new["median_ms"] - base["median_ms"]
    return {"delta_median_ms": delta,
            "ratio": new["median_ms"] / base["median_ms"],
            "within_3x_spread": abs(delta) <= 3.0 * base["spread_ms"]}


def measure(pop, truncation, horizon, args, device):
    inner = args.inner if pop >= 8192 else 8 * args.inner
    shape = dict(pop=pop, truncation=truncation, horizon=horizon)
    plain = GAEngine(GAConfig(**shape), device=device)
    twin = GAEngine(GAConfig(**shape), device=device)
    safe = SafeGAEngine(SafeGAConfig(**shape), device=device)

    noise = interleaved({"a": plain.step, "b": twin.step}, args.repeats,
                        inner, args.warmup)
    na, nb = summary(noise["a"]), summary(noise["b"])
    out = dict(shape, calls_per_timing=inner)
    out["noise_GAEngine.step_A"] = na
    out["noise_GAEngine.step_B"] = dict(nb, **compare(na, nb))

    steps = interleaved({"GAEngine.step": plain.step,
                         "SafeGAEngine.step": safe.step},
                        args.repeats, inner, args.warmup)
    base = summary(steps["GAEngine.step"])
    new = summary(steps["SafeGAEngine.step"])
    out["GAEngine.step"] = base
    out["SafeGAEngine.step"] = dict(new, **compare(base, new))

    # the launches on their own, from the safe engine's current state
    g, cfg = safe.generation, safe.cfg
    parents = safe.parents
    pidx, slot = ops.ga_parents(cfg.seed, g, pop, cfg.n_elite,
                                parents.shape[0], device)
    tail = (safe.obs_mu, safe.obs_nu, safe.env_A, safe.env_B)
    rows = safe._steps(parents)
    const = torch.full_like(parents, 0.02)
    got, _s = ops.ga_rollout_mlp_sm(parents, const, pidx, slot, cfg.seed, g,
                                    horizon, *tail)
    want, _s = ops.ga_rollout_mlp(parents, pidx, slot, 0.02, cfg.seed, g,
                                  horizon, *tail)
    out["constant_steps_bit_identical_to_ga_rollout_mlp"] = bool(
        torch.equal(got, want))
    out["survivors_bit_identical_to_decode"] = bool(torch.equal(
        safe.decode(safe.lineage[:4, : safe.generation]), safe.parents[:4]))

    rollout = interleaved(
        {"ga_rollout_mlp":
         lambda: ops.ga_rollout_mlp(parents, pidx, slot, 0.02, cfg.seed, g,
                                    horizon, *tail),
         "ga_rollout_mlp_sm":
         lambda: ops.ga_rollout_mlp_sm(parents, rows, pidx, slot, cfg.seed,
                                       g, horizon, *tail)},
        args.repeats, inner, args.warmup)
    base = summary(rollout["ga_rollout_mlp"])
    new = summary(rollout["ga_rollout_mlp_sm"])
    out["ga_rollout_mlp"] = base
    out["ga_rollout_mlp_sm"] = dict(new, **compare(base, new))

    small = interleaved({"sm_steps": lambda: safe._steps(parents)},
                        args.repeats, args.small_inner, args.warmup)
    out["sm_steps"] = dict(summary(small["sm_steps"]),
                           rows=int(parents.shape[0]))
    return out


def logit_moves(engine, steps, device):
    """Mean |change of the logits| on the probe, for CHILDREN children of
    the engine's parents: [CHILDREN] on the CPU.  ``steps`` is the step rows
    of the parents (constant for the plain GA)."""
    cfg = engine.cfg
    parents = engine.parents
    T = parents.shape[0]
    pidx, slot = ops.ga_parents(cfg.seed, 10 ** 6, CHILDREN, 0, T, device)
    order = torch.arange(CHILDREN, dtype=torch.int32, device=device)
    kids = ops.ga_survivors_sm(parents, steps, pidx, slot, order, cfg.seed,
                               10 ** 6)
    probe = engine.probe if hasattr(engine, "probe") else None
    if probe is None:
        from fiber_amd.es.safe_ga import default_probe

        probe = torch.from_numpy(default_probe(cfg.seed)).to(device)
    base = torch.stack([ops.mlp_policy_forward(parents[t], probe)
                        for t in range(T)])
    moves = torch.empty(CHILDREN, device=device)
    for m, p in enumerate(pidx.tolist()):
        lg = ops.mlp_policy_forward(kids[m], probe)
        moves[m] = (lg - base[p]).abs().mean()
    return moves.cpu()


def quantiles(v):
    q = torch.quantile(v.double(), torch.tensor([0.1, 0.5, 0.9, 1.0],
                                                dtype=torch.float64))
    return {"p10": float(q[0]), "median": float(q[1]), "p90": float(q[2]),
            "max": float(q[3]), "mean": float(v.mean())}


def learn_run(engine, device):
    start = float(engine.evaluate(iteration=0))
    for _ in range(LEARN_GENERATIONS):
        stats = engine.step()
    final = float(engine.evaluate(iteration=0))
    cfg = engine.cfg
    drift = float(ops.es_eval_matrix(
        engine.theta0.unsqueeze(0), engine.obs_mu.unsqueeze(0),
        engine.obs_nu.unsqueeze(0), engine.env_A.unsqueeze(0),
        engine.env_B.unsqueeze(0), cfg.seed, 0, cfg.horizon))
    if isinstance(engine, SafeGAEngine):
        steps = engine._steps(engine.parents)
    else:
        steps = torch.full_like(engine.parents, cfg.sigma)
    finite = steps[torch.isfinite(steps)]
    return {"sigma": cfg.sigma, "theta0": start, "final": final,
            "theta0_learned_normaliser": drift,
            "last_elite_fitness": stats["elite_fitness"],
            "last_fitness_max": stats["fitness_max"],
            "step_median": float(finite.median()),
            "step_max": float(finite.max()),
            "logit_move": quantiles(logit_moves(engine, steps, device))}


def learn(args, device):
    out = {"size": dict(LEARN, generations=LEARN_GENERATIONS), "runs": []}
    for sigma in args.ga_sigmas:
        eng = GAEngine(GAConfig(sigma=sigma, **LEARN), device=device)
        out["runs"].append(dict(learn_run(eng, device), arm="GA"))
    for mode in ops.SM_MODES:
        for sigma in args.sm_sigmas:
            eng = SafeGAEngine(SafeGAConfig(sigma=sigma, mode=mode, **LEARN),
                               device=device)
            out["runs"].append(dict(learn_run(eng, device),
                                    arm="SM-G-" + mode.upper()))
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--inner", type=int, default=5)
    parser.add_argument("--small-inner", type=int, default=50)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--learn", action="store_true",
                        help="run the learning sweep instead of the timings")
    parser.add_argument("--ga-sigmas", type=float, nargs="+",
                        default=[0.01, 0.02, 0.04])
    parser.add_argument("--sm-sigmas", type=float, nargs="+",
                        default=[0.0005, 0.001, 0.002, 0.004])
    args = parser.parse_args()
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats: their spread is the noise "
                         "floor")
    if not torch.cuda.is_available():
        raise SystemExit("safe_ga_rate.py needs an MI355X")
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0)}
    if args.learn:
        out["learn"] = learn(args, device)
    else:
        out["shapes"] = [measure(*shape, args, device) for shape in SHAPES]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
