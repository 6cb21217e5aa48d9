"""Launch time of es_rollout_mlp_lowrank next to es_rollout_mlp, for
profiles/lmmaes.md.

  python scripts/lmmaes_rate.py --pop 32768 --horizons 256 16 --reps 7

Per horizon the three launches (es_rollout_mlp; lowrank at J = 0; lowrank at
J = 29 with LM-MA-ES-like directions) are timed with device events in
alternation, `reps` rounds after a warm-up of every shape; the script
prints the median and the min-max spread of each, one JSON line per
horizon.  At J = 0 the outputs are also compared bit for bit.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pop", type=int, default=32768)
    parser.add_argument("--horizons", type=int, nargs="+", default=[256, 16])
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--dirs", type=int, default=29)
    args = parser.parse_args()

    import torch

    from fiber_amd import ops
    from fiber_amd.es import ESConfig, ESEngine

    dev = torch.device("cuda", 0)
    eng = ESEngine(ESConfig(pop_per_gpu=args.pop), device=dev)
    env = (eng.obs_mu, eng.obs_nu, eng.env_A, eng.env_B)
    gen = torch.Generator().manual_seed(1)
    dirs = (torch.randn(args.dirs, ops.NPARAMS, generator=gen)
            * 0.01).to(dev)
    mix = torch.tril(torch.randn(args.dirs, args.dirs, generator=gen)
                     * 0.01).to(dev)
    none = (dirs[:0], mix[:0, :0].contiguous(), 1.0)

    def timed(fn):
        start, stop = (torch.cuda.Event(enable_timing=True) for _ in "ab")
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop), out

    for horizon in args.horizons:
        tail = (1234, 0, horizon, 0, args.pop) + env
        launches = {
            "es_rollout_mlp": lambda: ops.es_rollout_mlp(
                eng.theta, 0.05, *tail),
            "lowrank_J0": lambda: ops.es_rollout_mlp_lowrank(
                eng.theta, 0.05, *none, *tail),
            "lowrank_J%d" % args.dirs: lambda: ops.es_rollout_mlp_lowrank(
                eng.theta, 0.05, dirs, mix, 0.99, *tail),
        }
        outs = {name: timed(fn)[1] for name, fn in launches.items()}
        same = all(torch.equal(a, b) for a, b in zip(
            outs["es_rollout_mlp"], outs["lowrank_J0"]))
        ms = {name: [] for name in launches}
        for _ in range(args.reps):
            for name, fn in launches.items():
                ms[name].append(timed(fn)[0])
        print(json.dumps({
            "pop": args.pop, "horizon": horizon, "reps": args.reps,
            "J0_bits_equal": same,
            **{name: {"median_ms": round(statistics.median(v), 3),
                      "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
               for name, v in ms.items()}}), flush=True)


if __name__ == "__main__":
    main()
