"""Cost of the separable-NES kernels against their scalar-sigma siblings
(MI355X only).

At bench.py's MLP shape (pop 32768, horizon 256), in one process:

  es_rollout_mlp / es_rollout_mlp_sigma   ms per launch, the same arguments,
                                          sigma_vec = full(sigma)
  es_grad / es_grad_sigma                 ms per launch over pop/2 pairs
  ESEngine.step / SNESEngine.step         ms per step

The arms of a group alternate inside one process, each warmed up and timed
with device events around a batch of calls; the spread of the sibling's
repeats is the noise floor the new kernel is read against.  Before timing,
the outputs that must agree bit for bit are checked.  Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fiber_amd import ops
from fiber_amd.es import ESConfig, ESEngine, SNESEngine


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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pop", type=int, default=32768)
    parser.add_argument("--horizon", type=int, default=256)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--inner", type=int, default=5,
                        help="rollout launches or steps per timing")
    parser.add_argument("--grad-inner", type=int, default=50,
                        help="gradient launches per timing")
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats: their spread is the noise "
                         "floor")
    if not torch.cuda.is_available():
        raise SystemExit("snes_rate.py needs an MI355X")
    device = torch.device("cuda", 0)
    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon)
    plain = ESEngine(cfg, device=device)
    snes = SNESEngine(cfg, device=device)

    tail = (cfg.seed, 0, cfg.horizon, 0, args.pop, plain.obs_mu,
            plain.obs_nu, plain.env_A, plain.env_B)
    fit, stat = ops.es_rollout_mlp(plain.theta, cfg.sigma, *tail)
    fit_s, stat_s = ops.es_rollout_mlp_sigma(plain.theta, snes.sigma, *tail)
    same_rollout = bool(torch.equal(fit, fit_s) and torch.equal(stat, stat_s))

    rollout = interleaved(
        {"es_rollout_mlp":
         lambda: ops.es_rollout_mlp(plain.theta, cfg.sigma, *tail),
         "es_rollout_mlp_sigma":
         lambda: ops.es_rollout_mlp_sigma(plain.theta, snes.sigma, *tail)},
        args.repeats, args.inner, args.warmup)

    ranks = ops.centered_rank(fit)
    wdiff = (ranks[0::2] - ranks[1::2]).contiguous()
    wsum = (ranks[0::2] + ranks[1::2]).contiguous()
    pairs = args.pop // 2
    g = ops.es_grad(wdiff, 0, pairs, cfg.seed, 0, device)
    g_mu, _g_sig = ops.es_grad_sigma(wdiff, wsum, 0, pairs, cfg.seed, 0,
                                     device)
    same_grad = bool(torch.equal(g, g_mu))

    grad = interleaved(
        {"es_grad": lambda: ops.es_grad(wdiff, 0, pairs, cfg.seed, 0, device),
         "es_grad_sigma": lambda: ops.es_grad_sigma(wdiff, wsum, 0, pairs,
                                                    cfg.seed, 0, device)},
        args.repeats, args.grad_inner, args.warmup)

    steps = interleaved({"ESEngine.step": plain.step,
                         "SNESEngine.step": snes.step},
                        args.repeats, args.inner, args.warmup)

    out = {"device": torch.cuda.get_device_name(0), "pop": args.pop,
           "horizon": args.horizon, "rollout_calls_per_timing": args.inner,
           "grad_calls_per_timing": args.grad_inner,
           "rollout_outputs_bit_identical": same_rollout,
           "g_mu_bit_identical_to_es_grad": same_grad}
    for group, base_name, new_name in (
            (rollout, "es_rollout_mlp", "es_rollout_mlp_sigma"),
            (grad, "es_grad", "es_grad_sigma"),
            (steps, "ESEngine.step", "SNESEngine.step")):
        base, new = summary(group[base_name]), summary(group[new_name])
        out[base_name] = base
        out[new_name] = dict(new, **compare(base, new))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
