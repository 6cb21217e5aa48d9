"""Rate of ESPopulation.step() against the loop it replaces (MI355X only).

One inner ES step of a POET population of P pairs, two ways:

  batched      one ESPopulation.step(): a batched rollout, rank and
               gradient launch each, row-wise Adam, no host sync
  engine_loop  P x ESEngine.step(), one pair after the other: the only
               path without ESPopulation

Both arms are warmed up, timed with device events around a batch of
steps (so the launches and host syncs of the loop are part of its time,
as they are for a user) and repeated; the arms alternate inside one
process.  The configurations are given as P:pop, by default the POET
example's own (8:512) and a wider one (32:256).  Before timing, the two
are checked to have computed the same thetas.  Prints one JSON line.
"""

import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fiber_amd.es import ESConfig, ESEngine, ESPopulation, make_env_params


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
            "max_ms": max(ms), "repeats": len(ms)}


def measure(P, pop, horizon, repeats, inner, warmup, device):
    cfg = ESConfig(pop_per_gpu=pop, horizon=horizon)
    seeds = [1234 + p for p in range(P)]
    gen = torch.Generator().manual_seed(P * 7919 + pop)
    A0, B0 = make_env_params(1234, "cpu")
    envs = [(A0 + 0.1 * torch.randn(4, 4, generator=gen),
             B0 + 0.1 * torch.randn(4, generator=gen)) for _ in range(P)]
    population = ESPopulation(cfg, seeds, envs, device=device)
    engines = [ESEngine(dataclasses.replace(cfg, seed=seeds[p]), ctx=None,
                        device=device, env_params=envs[p])
               for p in range(P)]

    def batched():
        population.step()

    def engine_loop():
        for eng in engines:
            eng.step()

    # both arms take the same number of steps throughout, so the states
    # can be compared at any point
    batched()
    engine_loop()
    same = all(torch.equal(population.theta[p], engines[p].theta)
               for p in range(P))
    ms = interleaved({"batched": batched, "engine_loop": engine_loop},
                     repeats, inner, warmup)
    same = same and all(torch.equal(population.theta[p], engines[p].theta)
                        for p in range(P))
    b, e = summary(ms["batched"]), summary(ms["engine_loop"])
    return {
        "P": P, "pop": pop, "horizon": horizon,
        "steps_per_timing": inner,
        "batched": b,
        "engine_loop_%d_steps" % P: e,
        "speedup_median": e["median_ms"] / b["median_ms"],
        "ranges_disjoint": b["max_ms"] < e["min_ms"],
        "thetas_bit_identical": bool(same),
    }


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--configs", default="8:512,32:256",
                        help="comma-separated P:pop")
    parser.add_argument("--horizon", type=int, default=64)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--inner", type=int, default=20,
                        help="steps per timing")
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("es_population_rate.py needs an MI355X")
    device = torch.device("cuda", 0)
    results = []
    for item in args.configs.split(","):
        P, pop = (int(v) for v in item.split(":"))
        results.append(measure(P, pop, args.horizon, args.repeats,
                               args.inner, args.warmup, device))
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "configs": results}))


if __name__ == "__main__":
    main()
