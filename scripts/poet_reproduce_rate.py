"""Cost of POET environment reproduction (MI355X only).

Two measurements, each a child process of its own under a time limit; a
step that fails or runs out of time ends the script, nothing is started
after it:

  novelty     ops.env_novelty (pata_ec_codes + pata_ec_knn, two launches)
              against what a user would write without it, a torch
              composition on the same device: clip, double argsort per
              column, torch.cdist, topk.  K=256 agents, 4096 references,
              512 candidates, k=5, heavily clipped scores.  The arms are
              warmed up and alternate; device-event time per call.  Also
              checks the kernels against the numpy oracle and counts the
              candidates that the torch path (fp32 distances, index-order
              tie-break) puts at another place in the novelty order.
  generation  examples/poet_transfer.py, seconds per generation with
              --reproduce against --batched alone, 8 pairs x pop 512, the
              two alternating.

Prints one JSON line per step.
"""

import argparse
import contextlib
import io
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = {"novelty": 240, "generation": 300}


def timed_ms(fn, inner):
    import torch
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms), "repeats": len(ms)}


def torch_novelty(scores, n_ref, k, lo, hi):
    """The composition the kernels replace: ranks with argsort's
    index-order tie-break, fp32 distances, a Q x R matrix."""
    import torch
    K = scores.shape[0]
    c = torch.where(torch.isnan(scores), torch.full_like(scores, lo),
                    scores.clamp(lo, hi))
    ranks = torch.argsort(torch.argsort(c, dim=0), dim=0).float()
    rows = ranks.t().contiguous()
    dist = torch.cdist(rows[n_ref:], rows[:n_ref])
    near = torch.topk(dist, min(k, n_ref), dim=1, largest=False).values
    return near.sum(dim=1) / (min(k, n_ref) * (K - 1))


def order_positions(novelty):
    """Place of every candidate in the admission order (novelty
    descending, ties to the lowest index)."""
    import numpy as np
    order = np.lexsort((np.arange(len(novelty)), -novelty))
    place = np.empty(len(novelty), dtype=np.int64)
    place[order] = np.arange(len(novelty))
    return place


def step_novelty(args):
    import numpy as np
    import torch
    from fiber_amd import ops
    from fiber_amd.es import novelty_oracle as no

    K, n_ref, Q, k = args.K, args.n_ref, args.Q, args.k
    lo, hi = 0.0, 1.5  # half of a standard normal sits at lo
    gen = torch.Generator().manual_seed(20)
    scores = torch.randn(K, n_ref + Q, generator=gen).cuda()

    def kernel():
        return ops.env_novelty(scores, n_ref, k, lo, hi)

    def composition():
        return torch_novelty(scores, n_ref, k, lo, hi)

    arms = {"kernels": kernel, "torch": composition}
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(args.repeats):
        for name, fn in arms.items():
            ms[name].append(timed_ms(fn, args.inner))

    nov, d2 = ops.env_novelty(scores, n_ref, k, lo, hi,
                              return_neighbours=True)
    codes = no.codes_oracle(scores.cpu().numpy(), lo, hi)
    want_d2, want_nov = no.knn_oracle(codes, n_ref, k)
    nov64 = nov.double().cpu().numpy()
    exact = bool(np.array_equal(d2.cpu().numpy(), want_d2))
    in_bound = bool((np.abs(nov64 - want_nov)
                     <= no.novelty_bound(want_nov, min(k, n_ref))).all())
    torch_nov = composition().double().cpu().numpy()
    moved = int((order_positions(torch_nov)
                 != order_positions(want_nov)).sum())
    moved_kernel = int((order_positions(nov64)
                        != order_positions(want_nov)).sum())
    a, b = summary(ms["kernels"]), summary(ms["torch"])
    print(json.dumps({
        "step": "novelty", "device": torch.cuda.get_device_name(0),
        "K": K, "n_ref": n_ref, "Q": Q, "k": k,
        "calls_per_timing": args.inner, "kernels": a, "torch": b,
        "speedup_median": b["median_ms"] / a["median_ms"],
        "ranges_disjoint": a["max_ms"] < b["min_ms"],
        "knn_d2_equals_oracle": exact, "novelty_in_bound": in_bound,
        "candidates_torch_places_differently": moved,
        "candidates_kernels_place_differently": moved_kernel,
        "max_rel_dev_torch_novelty": float(
            np.max(np.abs(torch_nov - want_nov)
                   / np.maximum(want_nov, 1e-30))),
    }))
    if not (exact and in_bound):
        raise SystemExit("the kernels disagree with the oracle")


def step_generation(args):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import poet_transfer

    base = ["--pairs", "8", "--pop", "512", "--horizon", "64",
            "--generations", str(args.generations)]

    def run(extra):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            poet_transfer.main(base + extra)
        last = out.getvalue().strip().splitlines()[-1]
        seconds = float(re.search(r"in ([0-9.]+) s", last).group(1))
        return 1e3 * seconds / args.generations, last

    arms = {"batched": ["--batched"],
            "reproduce": ["--reproduce", "--max-pairs", "8"]}
    for extra in arms.values():  # warm-up
        run(extra)
    ms = {name: [] for name in arms}
    last = {}
    for _ in range(args.repeats):
        for name, extra in arms.items():
            t, last[name] = run(extra)
            ms[name].append(t)
    a, b = summary(ms["batched"]), summary(ms["reproduce"])
    print(json.dumps({
        "step": "generation", "device": torch.cuda.get_device_name(0),
        "pairs": 8, "pop": 512, "horizon": 64,
        "generations_per_timing": args.generations,
        "batched_ms_per_generation": a, "reproduce_ms_per_generation": b,
        "extra_ms_per_generation_median": b["median_ms"] - a["median_ms"],
        "last_line_reproduce": last["reproduce"],
    }))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    parser.add_argument("--K", type=int, default=256)
    parser.add_argument("--n-ref", dest="n_ref", type=int, default=4096)
    parser.add_argument("--Q", type=int, default=512)
    parser.add_argument("--k", type=int, default=5)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--inner", type=int, default=50,
                        help="novelty: calls per timing")
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--generations", type=int, default=10)
    args = parser.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("poet_reproduce_rate.py needs an MI355X")
        return {"novelty": step_novelty,
                "generation": step_generation}[args.step](args)
    # the driver: it never touches the GPU itself
    passed_on = [a for a in sys.argv[1:]]
    for step in ("novelty", "generation"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]),
               sys.executable, os.path.abspath(__file__), "--step", step]
        rc = subprocess.run(cmd + passed_on).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d; stopping"
                             % (step, rc))


if __name__ == "__main__":
    main()
