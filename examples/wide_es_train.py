"""Train a wide feed-forward policy (4 -> H -> H -> 2, H = 128 or 256) with
OpenAI-ES on the synthetic environment.

  python examples/wide_es_train.py --hidden 256 --iters 30

Prints the fitness curve, then serves a batch of observations with act().
"""

import argparse

import torch

from fiber_amd import ops
from fiber_amd.es import ESConfig, WideESEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=256,
                    choices=ops.WIDE_HIDDEN)
    ap.add_argument("--pop", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()

    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon, seed=args.seed)
    engine = WideESEngine(cfg, args.hidden, device=torch.device("cuda", 0))
    print("hidden=%d nparams=%d pop=%d horizon=%d"
          % (args.hidden, engine.nparams, args.pop, args.horizon))
    for it in range(args.iters):
        stats = engine.step()
        print("iter %3d  fitness mean %9.4f  max %9.4f  eval %9.4f"
              % (it, stats["fitness_mean"], stats["fitness_max"],
                 float(engine.evaluate())))
    obs = 0.3 * torch.randn(8, 4, device=engine.device)
    print("actions for 8 random observations:", engine.act(obs).tolist())


if __name__ == "__main__":
    main()
