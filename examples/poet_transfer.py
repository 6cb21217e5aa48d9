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

``--reproduce`` (implies ``--batched``) replaces step 4 by POET's
environment reproduction, ``fiber_amd.es.reproduce``: pairs whose own
score reaches ``--repro-threshold`` propose perturbed child environments,
the children that pass the minimal criterion are ranked by PATA-EC
novelty against the active and archived environments, the most novel are
admitted as new pairs seeded with the agent that does best on them, and
past ``--max-pairs`` the oldest pairs retire to the archive.
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
                          make_env_params, reproduce, select_transfers,
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
    parser.add_argument("--reproduce", action="store_true",
                        help="grow the population by environment "
                             "reproduction (implies --batched)")
    parser.add_argument("--max-pairs", type=int, default=12,
                        help="--reproduce: pairs kept active; older ones "
                             "retire to the archive")
    parser.add_argument("--children", type=int, default=16,
                        help="--reproduce: children proposed per generation")
    parser.add_argument("--max-admit", type=int, default=2,
                        help="--reproduce: children admitted per generation")
    parser.add_argument("--repro-threshold", type=float,
                        default=float("-inf"),
                        help="--reproduce: own score a pair needs to "
                             "propose children")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("poet_transfer.py needs an MI355X")
    device = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(args.seed ^ 0x90E7)
    base = make_env_params(args.seed, "cpu")
    cfg = ESConfig(pop_per_gpu=args.pop, horizon=args.horizon,
                   seed=args.seed)

    envs = [perturbed_env(base, gen, 0.1) for _ in range(args.pairs)]
    if args.batched or args.reproduce:
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
    archive, next_seed, admitted_total = None, args.seed + args.pairs, 0
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
        if args.reproduce:
            # the returns of this toy lie in [-horizon, horizon]: a child
            # is kept if its best agent neither fails nor has solved it
            rec = reproduce(
                pop, scores, archive=archive,
                repro_threshold=args.repro_threshold,
                n_children=args.children, mutate_scale=0.05, generator=gen,
                mc_lo=0.0, mc_hi=0.98 * args.horizon, clip_lo=0.0,
                clip_hi=float(args.horizon), knn=5,
                max_admit=args.max_admit, max_pairs=args.max_pairs,
                child_seeds=[next_seed + c for c in range(args.children)],
                horizon=args.horizon, seed=args.seed, iteration=g)
            next_seed += args.children
            admitted_total += len(rec["admitted"])
            if rec["retired"][2]:
                old = archive or (rec["retired"][0][:0],
                                  rec["retired"][1][:0])
                archive = (torch.cat([old[0], rec["retired"][0]]),
                           torch.cat([old[1], rec["retired"][1]]))
            print("gen %d  transfers=%d  diag_mean=%.4f  parents=%d  "
                  "passed=%d/%d  admitted=%s  donors=%s  retired=%d  "
                  "pairs=%d  archive=%d"
                  % (g, len(transfers), float(diag.mean()),
                     len(rec["parents"]), int(rec["passed"].sum()),
                     len(rec["parent_of"]), rec["admitted"], rec["donors"],
                     len(rec["retired"][2]), pop.P,
                     0 if archive is None else archive[0].shape[0]))
            continue
        solved = int(torch.argmax(incumbent))
        envs[solved] = perturbed_env(envs[solved], gen, 0.05)
        pop.set_env(solved, *envs[solved])
        print("gen %d  transfers=%d  diag_mean=%.4f  best_incumbent=%.4f  "
              "mutated_env=%d"
              % (g, len(transfers), float(diag.mean()),
                 float(incumbent.max()), solved))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.reproduce:
        print("%d generations from %d to %d pairs in %.3f s: %.2f "
              "generations/s, %d transfers, %d admissions in all "
              "(batched, reproduce)"
              % (args.generations, args.pairs, pop.P, dt,
                 args.generations / dt, total_transfers, admitted_total))
        return total_transfers
    print("%d generations of %d pairs in %.3f s: %.2f generations/s, "
          "%d transfers in all (batched)"
          % (args.generations, args.pairs, dt, args.generations / dt,
             total_transfers))
    return total_transfers


if __name__ == "__main__":
    main()
