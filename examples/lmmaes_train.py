"""LM-MA-ES on the MLP policy: a population sampled through 29 learned
direction vectors, with a global step size that adapts during the run.

  python examples/lmmaes_train.py --iters 50

theta moves by the recombination of the best half of the population; sigma
starts at --sigma and is multiplied each iteration by exp((c_sigma / 2)
(|p_sigma|^2 / n - 1)), clamped to [1e-3, 10] x --sigma.  The rates are the
paper's at its default population and have not been tuned for this
workload.  Single process, one GPU.
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
                        help="initial global step size")
    parser.add_argument("--lr-mean", type=float, default=1.0)
    parser.add_argument("--n-dirs", type=int, default=None,
                        help="default: 4 + floor(3 ln n) = 29, at most 32")
    args = parser.parse_args()

    import torch

    from fiber_amd.es import ESConfig, LMMAESConfig, LMMAESEngine

    device = torch.device("cuda", 0)
    engine = LMMAESEngine(
        ESConfig(pop_per_gpu=args.pop, horizon=args.horizon,
                 sigma=args.sigma),
        LMMAESConfig(n_dirs=args.n_dirs, lr_mean=args.lr_mean),
        device=device)
    print("n_dirs %d  c_sigma %.5f  sigma rails [%.2e, %.2e]"
          % (engine.lm.n_dirs, engine.lm.c_sigma, engine.lm.sigma_min,
             engine.lm.sigma_max))
    t0 = time.perf_counter()
    for i in range(args.iters):
        s = engine.step()
        print("iter %4d  fitness mean %+8.3f  max %+8.3f  |g_d| %.4f  "
              "sigma %.5f  dirs %d  theta %+8.3f"
              % (i, s["fitness_mean"], s["fitness_max"], s["grad_norm"],
                 s["sigma"], s["n_active"], float(engine.evaluate())))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # how far the sampling distribution has left the identity
    active, scale, mix = engine.sampling()
    print("T = %.5f I + M^t L M, |M rows| %s"
          % (scale, ["%.3f" % v for v in active.norm(dim=1).tolist()[:8]]))
    print("%.1fs, %.1fM rollouts/s"
          % (elapsed, s["rollouts"] * args.iters / elapsed / 1e6))


if __name__ == "__main__":
    main()
