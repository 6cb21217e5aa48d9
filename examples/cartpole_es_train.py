"""Train the MLP policy on CartPole with OpenAI-ES.

  python examples/cartpole_es_train.py --iters 50

Prints the mean episode length of the population (at most --horizon) and the
environment steps actually taken at each iteration.
"""

import argparse

import torch

from fiber_amd.es import CartPoleESEngine, ESConfig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=2048)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()

    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon, seed=args.seed)
    engine = CartPoleESEngine(cfg, device=torch.device("cuda", 0))
    for it in range(args.iters):
        stats = engine.step()
        print("iter %3d  mean length %7.2f  max %7.2f  eval %7.2f  "
              "env steps %d" % (it, stats["fitness_mean"],
                                stats["fitness_max"],
                                float(engine.evaluate()), stats["env_steps"]))


if __name__ == "__main__":
    main()
