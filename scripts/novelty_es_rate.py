"""Cost of novelty search on top of the plain ES step (MI355X only).

At bench.py's MLP shape (pop 32768, horizon 256), in one process:

  es_rollout_mlp      ms per launch; the spread of its repeats is the
                      noise floor the others are read against
  es_rollout_mlp_bc   ms per launch, the same arguments
  bc_knn_novelty      ms per launch, N = pop queries, R archive rows, k
  ESEngine.step / NoveltyESEngine.step (nsr)   ms per step

The arms of a group alternate inside one process, each warmed up and timed
with device events around a batch of calls.  Before timing, the two rollout
kernels are checked to give the same fitness and obs statistics.  Prints
one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fiber_amd import ops
from fiber_amd.es import (ESConfig, ESEngine, NoveltyConfig,
                          NoveltyESEngine)


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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pop", type=int, default=32768)
    parser.add_argument("--horizon", type=int, default=256)
    parser.add_argument("--archive", type=int, default=4096)
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--inner", type=int, default=5,
                        help="calls per timing")
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats: their spread is the noise "
                         "floor")
    if not torch.cuda.is_available():
        raise SystemExit("novelty_es_rate.py needs an MI355X")
    device = torch.device("cuda", 0)
    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon)
    plain = ESEngine(cfg, device=device)
    novel = NoveltyESEngine(
        cfg, NoveltyConfig(mode="nsr", k=args.k,
                           archive_capacity=args.archive), device=device)

    roll_args = (plain.theta, cfg.sigma, cfg.seed, 0, cfg.horizon, 0,
                 args.pop, plain.obs_mu, plain.obs_nu, plain.env_A,
                 plain.env_B)
    fit, stat = ops.es_rollout_mlp(*roll_args)
    fit_bc, stat_bc, bc = ops.es_rollout_mlp_bc(*roll_args)
    same = bool(torch.equal(fit, fit_bc) and torch.equal(stat, stat_bc))

    rollout = interleaved(
        {"es_rollout_mlp": lambda: ops.es_rollout_mlp(*roll_args),
         "es_rollout_mlp_bc": lambda: ops.es_rollout_mlp_bc(*roll_args)},
        args.repeats, args.inner, args.warmup)

    # an archive of real BCs: the members' own, so the kept lists churn
    archive = bc[: args.archive].contiguous()
    knn = interleaved(
        {"bc_knn_novelty": lambda: ops.bc_knn_novelty(bc, archive, args.k)},
        args.repeats, args.inner, args.warmup)

    steps = interleaved({"ESEngine.step": plain.step,
                         "NoveltyESEngine.step": novel.step},
                        args.repeats, args.inner, args.warmup)

    base = summary(rollout["es_rollout_mlp"])
    with_bc = summary(rollout["es_rollout_mlp_bc"])
    print(json.dumps({
        "device": torch.cuda.get_device_name(0),
        "pop": args.pop, "horizon": args.horizon,
        "calls_per_timing": args.inner,
        "rollout_outputs_bit_identical": same,
        "es_rollout_mlp": base,
        "es_rollout_mlp_bc": with_bc,
        "bc_minus_plain_median_ms": with_bc["median_ms"] - base["median_ms"],
        "within_3x_spread": abs(with_bc["median_ms"] - base["median_ms"])
        <= 3.0 * base["spread_ms"],
        "bc_knn_novelty": dict(summary(knn["bc_knn_novelty"]), N=args.pop,
                               R=int(archive.shape[0]), k=args.k),
        "ESEngine.step": summary(steps["ESEngine.step"]),
        "NoveltyESEngine.step_nsr": summary(steps["NoveltyESEngine.step"]),
    }))


if __name__ == "__main__":
    main()
