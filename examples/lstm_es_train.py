"""Train the LSTM recurrent policy with OpenAI-ES on the partially observed
synthetic environment.

  python examples/lstm_es_train.py --obs-mask 0b0011 --iters 30

Bit d of --obs-mask says that observation dim d reaches the policy; the
default hides two of the four.  Prints the fitness curve.
"""

import argparse

import torch

from fiber_amd.es import ESConfig, LSTMESEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs-mask", type=lambda s: int(s, 0), default=0b0011)
    ap.add_argument("--pop", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()

    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon, seed=args.seed)
    engine = LSTMESEngine(cfg, device=torch.device("cuda", 0),
                          obs_mask=args.obs_mask)
    print("obs_mask=%s pop=%d horizon=%d" % (bin(args.obs_mask), args.pop,
                                            args.horizon))
    for it in range(args.iters):
        stats = engine.step()
        print("iter %3d  fitness mean %9.4f  max %9.4f  eval %9.4f"
              % (it, stats["fitness_mean"], stats["fitness_max"],
                 float(engine.evaluate())))


if __name__ == "__main__":
    main()
