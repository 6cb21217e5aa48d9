"""Deep GA with safe mutations (SM-G): every weight's mutation step is sigma
over the sensitivity of the policy's logits to that weight, measured by one
backward pass per parent on a fixed probe batch.

  python examples/safe_ga_train.py --generations 50 --pop 4096 --truncation 64

As examples/ga_train.py, with a step per parent and per parameter.  --sigma
is the step of a weight with unit sensitivity, not of every weight: typical
weights move some 20 sigma, none more than sigma / --s-min.  --mode sum is
SM-G-SUM, whose signed gradients cancel over the batch: most weights then sit
at the floor and get sigma / s_min.  Single process, one GPU.
"""

import os as _os
import sys as _sys

_REPO_ROOT = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
if _REPO_ROOT not in _sys.path:
    _sys.path.insert(0, _REPO_ROOT)


import argparse
import time


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--generations", type=int, default=50)
    parser.add_argument("--pop", type=int, default=4096)
    parser.add_argument("--truncation", type=int, default=64)
    parser.add_argument("--elite", type=int, default=1)
    parser.add_argument("--horizon", type=int, default=256)
    parser.add_argument("--sigma", type=float, default=None,
                        help="step of a weight with unit sensitivity "
                        "(default: SafeGAConfig's)")
    parser.add_argument("--mode", choices=("abs", "sum"), default="abs")
    parser.add_argument("--s-min", type=float, default=0.01,
                        help="sensitivity floor: no step above sigma / s_min")
    args = parser.parse_args()
    if args.generations < 1:
        parser.error("--generations must be >= 1")

    import torch

    from fiber_amd.es import SafeGAConfig, SafeGAEngine

    device = torch.device("cuda", 0)
    extra = {} if args.sigma is None else {"sigma": args.sigma}
    engine = SafeGAEngine(
        SafeGAConfig(pop=args.pop, truncation=args.truncation,
                     n_elite=args.elite, horizon=args.horizon,
                     mode=args.mode, s_min=args.s_min, **extra),
        device=device)
    start = float(engine.evaluate(iteration=0))
    t0 = time.perf_counter()
    for _ in range(args.generations):
        s = engine.step()
        steps = engine.last["steps"]
        print("gen %4d  fitness mean %+8.3f  max %+8.3f  elite %+8.3f  "
              "step median %.4f  at the floor %4.1f%%"
              % (s["generation"], s["fitness_mean"], s["fitness_max"],
                 s["elite_fitness"], float(steps.median()),
                 100.0 * float((steps >= steps.max()).float().mean())))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    genome = engine.genome(0)
    print("best genome: %d mutations over %d generations, %d bytes as seeds "
          "against %d as weights"
          % (int((genome >= 0).sum()), engine.generation, genome.numel() * 4,
             engine.theta.numel() * 4))
    rebuilt = engine.decode(genome)[0]
    print("  decoded from theta0 bit for bit:",
          bool(torch.equal(rebuilt, engine.theta)))
    print("evaluate(iteration=0): theta0 %+.4f -> best %+.4f"
          % (start, float(engine.evaluate(iteration=0))))
    print("%.1fs, %.1fM rollouts/s"
          % (elapsed, s["rollouts"] * args.generations / elapsed / 1e6))


if __name__ == "__main__":
    main()
