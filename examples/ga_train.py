"""Deep GA on the MLP policy: truncation selection over Gaussian mutations,
every individual stored as its chain of mutation seeds.

  python examples/ga_train.py --generations 50 --pop 4096 --truncation 64

Each generation evaluates --pop members in one launch (the best --elite
survivors unmutated, the rest mutations of uniformly drawn survivors), keeps
the best --truncation and records which child slot produced each of them.
The final best policy is printed as its genome and rebuilt from it.  Constant
sigma, no separate elite re-evaluation, single process, one GPU.
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
    parser.add_argument("--sigma", type=float, default=0.02,
                        help="mutation step, constant over the run")
    args = parser.parse_args()
    if args.generations < 1:
        parser.error("--generations must be >= 1")

    import torch

    from fiber_amd.es import GAConfig, GAEngine

    device = torch.device("cuda", 0)
    engine = GAEngine(
        GAConfig(pop=args.pop, truncation=args.truncation,
                 n_elite=args.elite, sigma=args.sigma, horizon=args.horizon),
        device=device)
    start = float(engine.evaluate(iteration=0))
    t0 = time.perf_counter()
    for _ in range(args.generations):
        s = engine.step()
        print("gen %4d  fitness mean %+8.3f  max %+8.3f  elite %+8.3f"
              % (s["generation"], s["fitness_mean"], s["fitness_max"],
                 s["elite_fitness"]))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    genome = engine.genome(0)
    applied = int((genome >= 0).sum())
    print("best genome: %d mutations over %d generations, %d bytes as seeds "
          "against %d as weights"
          % (applied, engine.generation, genome.numel() * 4,
             engine.theta.numel() * 4))
    print("  slots:", genome.tolist())
    rebuilt = engine.decode(genome)[0]
    print("  decoded from theta0 bit for bit:",
          bool(torch.equal(rebuilt, engine.theta)))
    print("evaluate(iteration=0): theta0 %+.4f -> best %+.4f"
          % (start, float(engine.evaluate(iteration=0))))
    print("%.1fs, %.1fM rollouts/s"
          % (elapsed, s["rollouts"] * args.generations / elapsed / 1e6))


if __name__ == "__main__":
    main()
