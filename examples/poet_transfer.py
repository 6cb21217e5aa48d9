"""POET generation loop on the device — BASELINE config 5 with real kernels.

N (policy, environment) pairs, each an ESEngine on its own environment
(``make_env_params`` perturbed by a seeded generator).  One generation:

  1. a few ES ``step()``s per pair (the inner loop: es_rollout_mlp);
  2. ``transfer_matrix``: every agent on every environment, one
     es_eval_matrix launch for the whole N x N matrix;
  3. ``select_transfers`` / ``apply_transfers``: an environment takes the
     policy that beats its incumbent;
  4. the environment of the pair with the highest incumbent score is
     mutated (it has been solved best, so it moves on).

Prints one line per generation and, at the end, generations per second.
``examples/poet_loop.py`` is the CPU-plumbing toy of the same outer loop.

``--batched`` runs the same loop on one ``ESPopulation``: the inner ES
steps of all pairs are one batched rollout / rank / gradient launch each
instead of one ``ESEngine.step()`` per pair, with the same results (the
``gen`` lines are identical).
"""

import os as _os
import sys as _sys

_REPO_ROOT = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
if _REPO_ROOT not in _sys.path:
    _sys.path.insert(0, _REPO_ROOT)


import argparse
import dataclasses
import time

import torch

from fiber_amd.es import (ESConfig, ESEngine, ESPopulation, apply_transfers,
                          make_env_params, select_transfers,
                          transfer_matrix)


def perturbed_env(base, gen, scale):
    """A neighbour of the environment ``base`` = (env_A, env_B)."""
    env_A, env_B = base
    return (env_A + scale * torch.randn(env_A.shape, generator=gen),
            env_B + scale * torch.randn(env_B.shape, generator=gen))


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=8)
    parser.add_argument("--generations", type=int, default=5)
    parser.add_argument("--pop", type=int, default=512,
                        help="ES population per pair (even)")
    parser.add_argument("--horizon", type=int, default=64)
    parser.add_argument("--inner-steps", type=int, default=2,
                        help="ES steps per pair per generation")
    parser.add_argument("--seed", type=int, default=1234)
    parser.add_argument("--margin", type=float, default=0.0)
    parser.add_argument("--batched", action="store_true",
                        help="advance all pairs together (ESPopulation)")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("poet_transfer.py needs an MI355X")
    device = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(args.seed ^ 0x90E7)
    base = make_env_params(args.seed, "cpu")
    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon,
                   seed=args.seed)

    envs = [perturbed_env(base, gen, 0.1) for _ in range(args.pairs)]
    if args.batched:
        return run_batched(args, cfg, envs, gen, device)
    engines = []
    for i, env in enumerate(envs):
        # one noise stream and one initial policy per pair
        pair_cfg = dataclasses.replace(cfg, seed=args.seed + i)
        engines.append(ESEngine(pair_cfg, ctx=None, device=device,
                                env_params=env))

    total_transfers = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g in range(args.generations):
        for eng in engines:
            for _ in range(args.inner_steps):
                eng.step()
        scores = transfer_matrix(engines, args.horizon, args.seed, g)
        transfers = select_transfers(scores, args.margin)
        apply_transfers(engines, transfers)
        total_transfers += len(transfers)

        # after the transfers column m's incumbent holds the column best
        diag = scores.diagonal().cpu()
        incumbent = diag.clone()
        for m, k in transfers:
            incumbent[m] = float(scores[k, m])
        solved = int(torch.argmax(incumbent))
        envs[solved] = perturbed_env(envs[solved], gen, 0.05)
        engines[solved].env_A.copy_(envs[solved][0])
        engines[solved].env_B.copy_(envs[solved][1])
        print("gen %d  transfers=%d  diag_mean=%.4f  best_incumbent=%.4f  "
              "mutated_env=%d"
              % (g, len(transfers), float(diag.mean()),
                 float(incumbent.max()), solved))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d generations of %d pairs in %.3f s: %.2f generations/s, "
          "%d transfers in all"
          % (args.generations, args.pairs, dt, args.generations / dt,
             total_transfers))
    return total_transfers


def run_batched(args, cfg, envs, gen, device):
    """The loop of main() on an ESPopulation: pair i has seed
    ``args.seed + i``, as engine i has there."""
    pop = ESPopulation(cfg, [args.seed + i for i in range(args.pairs)],
                       envs, device=device)
    total_transfers = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g in range(args.generations):
        for _ in range(args.inner_steps):
            pop.step()
        scores = pop.transfer_matrix(args.horizon, args.seed, g)
        transfers = select_transfers(scores, args.margin)
        pop.apply_transfers(transfers)
        total_transfers += len(transfers)

        diag = scores.diagonal().cpu()
        incumbent = diag.clone()
        for m, k in transfers:
            incumbent[m] = float(scores[k, m])
        solved = int(torch.argmax(incumbent))
        envs[solved] = perturbed_env(envs[solved], gen, 0.05)
        pop.set_env(solved, *envs[solved])
        print("gen %d  transfers=%d  diag_mean=%.4f  best_incumbent=%.4f  "
              "mutated_env=%d"
              % (g, len(transfers), float(diag.mean()),
                 float(incumbent.max()), solved))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d generations of %d pairs in %.3f s: %.2f generations/s, "
          "%d transfers in all (batched)"
          % (args.generations, args.pairs, dt, args.generations / dt,
             total_transfers))
    return total_transfers


if __name__ == "__main__":
    main()
