"""Novelty-seeking ES on the MLP policy: NS-ES, NSR-ES or NSRA-ES.

  python examples/ns_es_train.py --mode nsra --meta-size 3 --iters 50

A member's behaviour characterisation is the mean final state of its 64
episodes; novelty is the mean distance to the k nearest archived ones.
Single process, one GPU.
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
    parser.add_argument("--mode", choices=("ns", "nsr", "nsra"),
                        default="nsr")
    parser.add_argument("--meta-size", type=int, default=1)
    parser.add_argument("--iters", type=int, default=50)
    parser.add_argument("--pop", type=int, default=4096)
    parser.add_argument("--horizon", type=int, default=256)
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--weight", type=float, default=1.0,
                        help="nsra: initial fitness weight")
    args = parser.parse_args()

    import torch

    from fiber_amd.es import ESConfig, NoveltyConfig, NoveltyESEngine

    device = torch.device("cuda", 0)
    engine = NoveltyESEngine(
        ESConfig(pop_per_gpu=args.pop, horizon=args.horizon),
        NoveltyConfig(mode=args.mode, k=args.k, meta_size=args.meta_size,
                      weight=args.weight),
        device=device)
    t0 = time.perf_counter()
    for i in range(args.iters):
        s = engine.step()
        print("iter %4d  agent %d  fitness mean %+8.3f  max %+8.3f  "
              "novelty %.5f  w %.2f  score %+8.3f  archive %d  |g| %.4f"
              % (i, s["agent"], s["fitness_mean"], s["fitness_max"],
                 s["novelty_mean"], s["weight"], s["agent_score"],
                 s["archive_size"], s["grad_norm"]))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    print("%.1fs, %.1fM rollouts/s"
          % (elapsed, s["rollouts"] * args.iters / elapsed / 1e6))


if __name__ == "__main__":
    main()
