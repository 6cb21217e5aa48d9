"""Timings behind profiles/map_elites.md: MapElitesEngine.step against
GAEngine.step, ga_rollout_mlp_bc against ga_rollout_mlp, and the archive
kernels at two grid sizes.

  python scripts/map_elites_rate.py

Per arm 3 warm-up calls, then --repeats timings with device events, the arms
of a group alternating; each timing covers --inner back-to-back calls.
Prints the median and the spread (max - min) in ms per call.
"""

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def time_group(arms, repeats, inner):
    """arms: {name: callable}.  Returns {name: (median, spread)} in ms per
    call."""
    import torch

    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(inner):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / inner)
    return {name: (statistics.median(t), max(t) - min(t))
            for name, t in times.items()}


def report(title, result):
    print(title)
    for name, (median, spread) in result.items():
        print("  %-34s median %9.4f ms  spread %7.4f ms"
              % (name, median, spread))
    sys.stdout.flush()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pop", type=int, default=4096)
    parser.add_argument("--horizon", type=int, default=200)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--inner", type=int, default=10)
    args = parser.parse_args()

    import torch

    from fiber_amd import ops
    from fiber_amd.es import (GAConfig, GAEngine, MapElitesConfig,
                              MapElitesEngine)

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    pop, h = args.pop, args.horizon

    me = MapElitesEngine(MapElitesConfig(pop=pop, bins=(32, 32, 1, 1),
                                         horizon=h), device=dev)
    ga = GAEngine(GAConfig(pop=pop, truncation=1024, horizon=h), device=dev)
    for _ in range(5):                      # past generation 0 of both
        me.step()
        ga.step()
    report("engine step, pop %d, horizon %d (ME 32 x 32 cells, GA "
           "truncation 1024)" % (pop, h),
           time_group({"MapElitesEngine.step": me.step,
                       "GAEngine.step": ga.step,
                       "MapElitesEngine.step (again)": me.step},
                      args.repeats, args.inner))
    print("  ME coverage %.4f after %d generations"
          % (int(me.n_filled) / me.cells, me.generation))

    # the rollout alone, both kernels on the same inputs
    pidx, slot = me.last["parent_idx"], me.last["slot"]
    common = (me.arch_theta, pidx, slot, me.cfg.sigma, me.cfg.seed,
              me.generation, h, me.obs_mu, me.obs_nu, me.env_A, me.env_B)
    res = time_group(
        {"ga_rollout_mlp (+ stat reduce)": lambda: ops.ga_rollout_mlp(*common),
         "ga_rollout_mlp_bc (+ stat reduce)":
             lambda: ops.ga_rollout_mlp_bc(*common),
         "ga_rollout_mlp (again)": lambda: ops.ga_rollout_mlp(*common)},
        args.repeats, args.inner)
    report("rollout launch, pop %d, horizon %d, %d filled cells as parents"
           % (pop, h, int(me.n_filled)), res)
    print("  ratio bc / plain %.4f"
          % (res["ga_rollout_mlp_bc (+ stat reduce)"][0]
             / res["ga_rollout_mlp (+ stat reduce)"][0]))

    # the archive kernels at two grid sizes, on this generation's results
    fitness, _stat, bc = ops.ga_rollout_mlp_bc(*common)
    for bins in ((32, 32, 1, 1), (254, 258, 1, 1)):
        C = bins[0] * bins[1]
        eng = MapElitesEngine(MapElitesConfig(
            pop=pop, bins=bins, horizon=h, bc_lo=me.bc_lo, bc_hi=me.bc_hi),
            device=dev)
        for _ in range(3):
            eng.step()
        af, ab, afl = eng.arch_fitness, eng.arch_bc, eng.arch_filled
        _cell, _winner, order = ops.me_insert(fitness, bc, bins, eng.bc_lo,
                                              eng.bc_hi, af, ab, afl)
        report("archive kernels, pop %d, C = %d (%d filled)"
               % (pop, C, int(eng.n_filled)), time_group({
                   "me_insert (memset, assign, commit)":
                       lambda: ops.me_insert(fitness, bc, bins, eng.bc_lo,
                                             eng.bc_hi, af, ab, afl),
                   "me_compact": lambda: ops.me_compact(
                       afl, out_filled_idx=eng.filled_idx,
                       out_n_filled=eng.n_filled),
                   "me_parents": lambda: ops.me_parents(
                       1, 7, pop, eng.filled_idx, eng.n_filled, C),
                   "ga_survivors, C + 1 rows": lambda: ops.ga_survivors(
                       eng.arch_theta, eng._parent_ext, eng._slot_ext, order,
                       eng.cfg.sigma, eng.cfg.seed, eng.generation,
                       out=eng._spare_theta)},
                   args.repeats, args.inner))
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
