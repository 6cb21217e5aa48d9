"""Cost of a Deep GA generation against an OpenAI-ES iteration (MI355X only).

At (pop 32768, truncation 1024, horizon 256), bench.py's MLP shape, and at
(pop 1024, truncation 32, horizon 200), GAConfig's defaults, in one process:

  ESEngine.step twice (A/A)           the run-to-run noise, measured first
  ESEngine.step / GAEngine.step       ms per step, the same pop and horizon
  es_rollout_mlp / ga_rollout_mlp     ms per launch (+ obs_stat_reduce)
  ga_parents, ga_truncate,            ms per launch
  ga_survivors

The baseline arm is this tree's ESEngine.  It stands in for the commit before
the GA, which is not checked out or timed here: engine.py, es_kernels.hip
and the build flags are the same in both.  The arms of a group alternate
inside one process, each warmed up and timed with device events around a
batch of calls.  Before timing, the outputs that must agree bit for bit are
checked.  Ratios are reported, not asserted.  Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fiber_amd import ops
from fiber_amd.es import ESConfig, ESEngine, GAConfig, GAEngine

SHAPES = ((32768, 1024, 256), (1024, 32, 200))


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
    # enough work per timing at the small shape too
    inner = args.inner if pop >= 8192 else 8 * args.inner
    es_cfg = ESConfig(pop_per_gpu=pop, horizon=horizon)
    plain = ESEngine(es_cfg, device=device)
    twin = ESEngine(es_cfg, device=device)
    ga = GAEngine(GAConfig(pop=pop, truncation=truncation, horizon=horizon),
                  device=device)

    # the noise first: the same code against itself
    noise = interleaved({"a": plain.step, "b": twin.step}, args.repeats,
                        inner, args.warmup)
    na, nb = summary(noise["a"]), summary(noise["b"])
    out = {"pop": pop, "truncation": truncation, "horizon": horizon,
           "calls_per_timing": inner,
           "noise_ESEngine.step_A": na,
           "noise_ESEngine.step_B": dict(nb, **compare(na, nb))}

    steps = interleaved({"ESEngine.step": plain.step,
                         "GAEngine.step": ga.step},
                        args.repeats, inner, args.warmup)
    base, new = summary(steps["ESEngine.step"]), summary(steps["GAEngine.step"])
    out["ESEngine.step"] = base
    out["GAEngine.step"] = dict(new, **compare(base, new))

    # the launches on their own, from the GA's current state (truncation
    # parents, every member with its own parent row and draw)
    g = ga.generation
    cfg = ga.cfg
    T_cur = ga.parents.shape[0]
    pidx, slot = ops.ga_parents(cfg.seed, g, pop, cfg.n_elite, T_cur, device)
    tail = (ga.obs_mu, ga.obs_nu, ga.env_A, ga.env_B)
    fit, _stat = ops.ga_rollout_mlp(ga.parents, pidx, slot, cfg.sigma,
                                    cfg.seed, g, horizon, *tail)
    order = ops.ga_truncate(fit, truncation)

    # one parent, slot m: the bits of es_rollout_mlp's even members
    few = min(pop, 256)
    one = ga.parents[:1].contiguous()
    zeros = torch.zeros(few, dtype=torch.int32, device=device)
    ramp = torch.arange(few, dtype=torch.int32, device=device)
    got, _s = ops.ga_rollout_mlp(one, zeros, ramp, cfg.sigma, cfg.seed, g,
                                 horizon, *tail)
    want, _s = ops.es_rollout_mlp(one[0], cfg.sigma, cfg.seed, g, horizon, 0,
                                  2 * few, *tail)
    out["mutated_members_bit_identical_to_es_rollout_mlp"] = bool(
        torch.equal(got, want[0::2]))
    out["survivors_bit_identical_to_decode"] = bool(torch.equal(
        ga.decode(ga.lineage[:, : ga.generation]), ga.parents))

    rollout = interleaved(
        {"es_rollout_mlp":
         lambda: ops.es_rollout_mlp(one[0], cfg.sigma, cfg.seed, g, horizon,
                                    0, pop, *tail),
         "ga_rollout_mlp":
         lambda: ops.ga_rollout_mlp(ga.parents, pidx, slot, cfg.sigma,
                                    cfg.seed, g, horizon, *tail)},
        args.repeats, inner, args.warmup)
    base = summary(rollout["es_rollout_mlp"])
    new = summary(rollout["ga_rollout_mlp"])
    out["es_rollout_mlp"] = base
    out["ga_rollout_mlp"] = dict(new, **compare(base, new))

    small = interleaved(
        {"ga_parents":
         lambda: ops.ga_parents(cfg.seed, g, pop, cfg.n_elite, T_cur, device),
         "ga_truncate": lambda: ops.ga_truncate(fit, truncation),
         "ga_survivors":
         lambda: ops.ga_survivors(ga.parents, pidx, slot, order, cfg.sigma,
                                  cfg.seed, g)},
        args.repeats, args.small_inner, args.warmup)
    for name, ms in small.items():
        out[name] = summary(ms)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--inner", type=int, default=5,
                        help="steps or rollout launches per timing at the "
                        "large shape (8x as many at the small one)")
    parser.add_argument("--small-inner", type=int, default=50,
                        help="launches per timing of the small kernels")
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats: their spread is the noise "
                         "floor")
    if not torch.cuda.is_available():
        raise SystemExit("ga_rate.py needs an MI355X")
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0),
           "shapes": [measure(*shape, args, device) for shape in SHAPES]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
