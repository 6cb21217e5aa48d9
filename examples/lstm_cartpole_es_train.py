"""Train the LSTM policy on CartPole with OpenAI-ES, velocities hidden.

  python examples/lstm_cartpole_es_train.py --iters 50 --mask 5

--mask is the set of state dims the policy sees (bit 0 x, bit 1 x_dot, bit 2
theta, bit 3 theta_dot).  With --mask 15 it sees the whole state and the task
is CartPole as examples/cartpole_es_train.py runs it; expect the mean episode
length to climb within a few iterations (on one seed: 30 at iteration 0, 184
at 5, the horizon of 200 from about 12 on).  With --mask 5 (the default) both
velocities are hidden and the policy has to estimate them from successive
positions through its hidden and cell state: expect a slower climb to the
same place (same seed: 11 at iteration 0, 47 at 5, 162 at 17, 199.7 at 35).

Prints the mean episode length of the population (at most --horizon) and the
environment steps actually taken at each iteration.
"""

import argparse

import torch

from fiber_amd.es import ESConfig, LSTMCartPoleESEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=2048)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--mask", type=int, default=0b0101)
    args = ap.parse_args()

    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon, seed=args.seed)
    engine = LSTMCartPoleESEngine(cfg, device=torch.device("cuda", 0),
                                  obs_mask=args.mask)
    for it in range(args.iters):
        stats = engine.step()
        print("iter %3d  mean length %7.2f  max %7.2f  eval %7.2f  "
              "env steps %d" % (it, stats["fitness_mean"],
                                stats["fitness_max"],
                                float(engine.evaluate()), stats["env_steps"]))


if __name__ == "__main__":
    main()
