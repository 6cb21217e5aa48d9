"""MAP-Elites on the MLP policy: a grid over behaviour space with the best
policy found for each kind of behaviour, every elite stored as its chain of
mutation seeds.

  python examples/map_elites_train.py --generations 50 --pop 4096 --bins 32 32 1 1

The behaviour of a policy is the mean final state over its 64 episodes, 4
floats; --bins sets the bins per dimension (1 ignores a dimension).  Each
generation mutates --pop elites drawn uniformly from the filled cells in one
launch, and a child takes the cell its behaviour falls in only if it is
strictly fitter than the occupant.  The grid's bounds are fixed from
generation 0.  Elites are not re-scored, constant sigma, single process, one
GPU.
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
    parser.add_argument("--bins", type=int, nargs=4, default=(32, 32, 1, 1))
    parser.add_argument("--horizon", type=int, default=256)
    parser.add_argument("--sigma", type=float, default=0.02,
                        help="mutation step, constant over the run")
    args = parser.parse_args()
    if args.generations < 1:
        parser.error("--generations must be >= 1")

    import torch

    from fiber_amd.es import MapElitesConfig, MapElitesEngine

    device = torch.device("cuda", 0)
    engine = MapElitesEngine(
        MapElitesConfig(pop=args.pop, bins=tuple(args.bins),
                        sigma=args.sigma, horizon=args.horizon),
        device=device)
    t0 = time.perf_counter()
    for _ in range(args.generations):
        s = engine.step()
        print("gen %4d  coverage %6.4f  qd-score %+12.3f  best %+8.3f  "
              "inserted %5d"
              % (s["generation"], s["coverage"], s["qd_score"],
                 s["fitness_max"], s["inserted"]))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    print("bounds: lo %s hi %s" % (engine.bc_lo, engine.bc_hi))
    cell = engine.best_cell()
    theta, fitness, bc, genome = engine.elite(cell)
    applied = int((genome >= 0).sum())
    print("best elite: cell %d, fitness %+.4f, bc %s, %d mutations, born in "
          "generation %d"
          % (cell, fitness, [round(x, 4) for x in bc.tolist()], applied,
             int(engine.arch_born[cell])))
    rebuilt = engine.decode(genome)[0]
    print("  decoded from theta0 bit for bit:",
          bool(torch.equal(rebuilt, theta)))
    print("%.1fs, %.1fM rollouts/s"
          % (elapsed, s["rollouts"] * args.generations / elapsed / 1e6))


if __name__ == "__main__":
    main()
