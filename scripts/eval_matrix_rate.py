"""Rate of es_eval_matrix against the paths it replaces (MI355X only).

(a) One es_eval_matrix launch at K = M = 8, T = 256 against the only way
    to fill the same 8 x 8 matrix without it: 64 calls of
    ops.es_rollout_mlp(sigma=0, pop_shard=1).
(b) Cells per second of es_eval_matrix at K*M = 32768, T = 256 against
    members per second of es_rollout_mlp at pop_shard 32768.

Every arm is warmed up, timed with device events around a batch of calls
(so launch overhead of the looped path is part of its time, as it is for
a user), and repeated; the arms of a comparison alternate inside one
process.  Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fiber_amd import ops
from fiber_amd.es import init_theta, make_env_params


def timed_ms(fn, inner):
    """Device-event time of ``inner`` back-to-back calls of fn, per call."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def interleaved(arms, repeats, inner):
    """{name: [ms per call, ...]}, arms alternating within each repeat."""
    for fn in arms.values():  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            out[name].append(timed_ms(fn, inner))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms), "repeats": len(ms)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--horizon", type=int, default=256)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--small", type=int, default=8, help="K = M of (a)")
    parser.add_argument("--cells", type=int, default=32768,
                        help="K*M of (b), a multiple of 128")
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_matrix_rate.py needs an MI355X")
    device = torch.device("cuda", 0)
    T, seed, it = args.horizon, 1234, 0

    def population(K, M):
        gen = torch.Generator().manual_seed(K * 7919 + M)
        base = init_theta(1, "cpu")
        thetas = base + 0.05 * torch.randn(K, ops.NPARAMS, generator=gen)
        mu = 0.1 * torch.randn(K, 4, generator=gen)
        nu = 0.5 + torch.rand(K, 4, generator=gen)
        A0, B0 = make_env_params(seed, "cpu")
        env_A = A0 + 0.1 * torch.randn(M, 4, 4, generator=gen)
        env_B = B0 + 0.1 * torch.randn(M, 4, generator=gen)
        return [t.to(device).contiguous()
                for t in (thetas, mu, nu, env_A, env_B)]

    # ---- (a) small matrix vs the loop it replaces ------------------------
    n = args.small
    thetas, mu, nu, env_A, env_B = population(n, n)

    def one_launch():
        return ops.es_eval_matrix(thetas, mu, nu, env_A, env_B, seed, it, T)

    def looped():
        rows = []
        for k in range(n):
            for m in range(n):
                f, _stat = ops.es_rollout_mlp(
                    thetas[k], 0.0, seed, it, T, 0, 1, mu[k], nu[k],
                    env_A[m], env_B[m])
                rows.append(f)
        return torch.cat(rows).view(n, n)

    same = bool(torch.equal(one_launch(), looped()))
    a = interleaved({"eval_matrix": one_launch, "rollout_loop": looped},
                    args.repeats, inner=20)
    a_eval, a_loop = summary(a["eval_matrix"]), summary(a["rollout_loop"])

    # ---- (b) full-chip rate vs the rollout kernel ------------------------
    cells = args.cells
    K, M = cells // 128, 128
    bt, bmu, bnu, bA, bB = population(K, M)
    theta1, mu1, nu1, A1, B1 = bt[0], bmu[0], bnu[0], bA[0], bB[0]

    def big_eval():
        return ops.es_eval_matrix(bt, bmu, bnu, bA, bB, seed, it, T)

    def big_rollout():
        return ops.es_rollout_mlp(theta1, 0.05, seed, it, T, 0, cells, mu1,
                                  nu1, A1, B1)

    b = interleaved({"eval_matrix": big_eval, "rollout": big_rollout},
                    args.repeats, inner=3)
    b_eval, b_roll = summary(b["eval_matrix"]), summary(b["rollout"])

    print(json.dumps({
        "device": torch.cuda.get_device_name(0),
        "horizon": T,
        "a_small_matrix": {
            "K": n, "M": n,
            "eval_matrix": a_eval,
            "rollout_loop_%d_calls" % (n * n): a_loop,
            "speedup_median": a_loop["median_ms"] / a_eval["median_ms"],
            "outputs_bit_identical": same,
        },
        "b_full_chip": {
            "K": K, "M": M, "cells": cells,
            "eval_matrix": b_eval,
            "rollout_pop_%d" % cells: b_roll,
            "eval_cells_per_s": cells / (b_eval["median_ms"] * 1e-3),
            "rollout_members_per_s": cells / (b_roll["median_ms"] * 1e-3),
            "eval_over_rollout_rate":
                b_roll["median_ms"] / b_eval["median_ms"],
        },
    }))


if __name__ == "__main__":
    main()
