"""Separable NES on the MLP policy: OpenAI-ES with a step size per
parameter that adapts during the run.

  python examples/snes_train.py --iters 50 --lr-sigma 0.1

Every parameter starts at --sigma; after each iteration sigma[j] is
multiplied by exp(lr_sigma / (2 pop) * sum_k wsum[k] (z_k[j]^2 - 1)) and
clamped to [1e-3, 10] x --sigma.  The default --lr-sigma is the SNES
paper's rule and has not been tuned for this workload.  Single process,
one GPU.
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
    parser.add_argument("--iters", type=int, default=50)
    parser.add_argument("--pop", type=int, default=4096)
    parser.add_argument("--horizon", type=int, default=256)
    parser.add_argument("--sigma", type=float, default=0.05,
                        help="initial step size of every parameter")
    parser.add_argument("--lr-sigma", type=float, default=None,
                        help="default: (3 + ln d) / (5 sqrt(d)), d = 4610")
    args = parser.parse_args()

    import torch

    from fiber_amd.es import ESConfig, SNESConfig, SNESEngine

    device = torch.device("cuda", 0)
    engine = SNESEngine(
        ESConfig(pop_per_gpu=args.pop, horizon=args.horizon,
                 sigma=args.sigma),
        SNESConfig(lr_sigma=args.lr_sigma), device=device)
    print("lr_sigma %.5f  sigma rails [%.2e, %.2e]"
          % (engine.snes.lr_sigma, engine.snes.sigma_min,
             engine.snes.sigma_max))
    t0 = time.perf_counter()
    for i in range(args.iters):
        s = engine.step()
        print("iter %4d  fitness mean %+8.3f  max %+8.3f  |g| %.4f  "
              "sigma mean %.5f  [%.5f, %.5f]"
              % (i, s["fitness_mean"], s["fitness_max"], s["grad_norm"],
                 s["sigma_mean"], s["sigma_min"], s["sigma_max"]))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # the spread per layer: which parts of the policy asked for more noise
    sig = engine.sigma
    for name, lo, hi in (("W1", 0, 256), ("b1", 256, 320),
                         ("W2", 320, 4416), ("b2", 4416, 4480),
                         ("W3", 4480, 4608), ("b3", 4608, 4610)):
        print("sigma %s mean %.5f" % (name, float(sig[lo:hi].mean())))
    print("%.1fs, %.1fM rollouts/s"
          % (elapsed, s["rollouts"] * args.iters / elapsed / 1e6))


if __name__ == "__main__":
    main()
