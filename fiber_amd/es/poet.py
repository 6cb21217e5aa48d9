"""POET transfer step on the device.

A POET population is a list of (policy, environment) pairs; here each pair
is one ESEngine built with its own ``env_params``.  Every generation the
transfer step scores every agent on every environment and moves a policy
to an environment where it beats the incumbent:

    scores = transfer_matrix(engines, horizon, seed, iteration)   # 1 launch
    moves = select_transfers(scores, margin)
    apply_transfers(engines, moves)

The K x K scores come from one ``ops.es_eval_matrix`` launch (one
workgroup per cell) instead of K*K single-member rollouts.
"""

import torch

from .. import ops


def transfer_matrix(engines, horizon, seed, iteration):
    """scores[K][K] on the engines' device: row k is engine k's current
    theta (with its own obs normaliser), column m is engine m's
    environment.  All cells see the same 64 episode start states (common
    random numbers from seed, iteration), so a column compares policies
    on equal terms."""
    if not engines:
        raise ValueError("transfer_matrix needs at least one engine")
    thetas = torch.stack([e.theta for e in engines])
    obs_mu = torch.stack([e.obs_mu for e in engines])
    obs_nu = torch.stack([e.obs_nu for e in engines])
    env_A = torch.stack([e.env_A for e in engines])
    env_B = torch.stack([e.env_B for e in engines])
    return ops.es_eval_matrix(thetas, obs_mu, obs_nu, env_A, env_B, seed,
                              iteration, horizon)


def select_transfers(scores, margin=0.0):
    """Transfer decision on a square score matrix (CPU or device tensor).

    For each environment (column) m the best policy (row) is found; ties
    go to the lowest k and a NaN score never wins.  Returns the list of
    ``(m, k)`` with ``k != m`` and ``scores[k, m] > scores[m, m] +
    margin``: environment m should receive policy k.  An incumbent whose
    own score is NaN loses to any policy with a real score."""
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be square, got %s"
                         % (tuple(scores.shape),))
    s = scores.detach().to("cpu", torch.float64)
    n = s.shape[0]
    transfers = []
    for m in range(n):
        best_k, best = None, None
        for k in range(n):
            v = float(s[k, m])
            if v != v:  # NaN never wins
                continue
            if best is None or v > best:  # strict: lowest k keeps a tie
                best_k, best = k, v
        if best_k is None or best_k == m:
            continue
        own = float(s[m, m])
        if own != own or best > own + margin:
            transfers.append((m, best_k))
    return transfers


def apply_transfers(engines, transfers):
    """Copy theta and the obs statistics of engine k into engine m for
    every ``(m, k)`` and zero m's Adam moments (the moments belong to the
    policy that was replaced).  All donors are read from the pre-transfer
    state, so chains such as [(0, 1), (1, 2)] do not depend on list
    order.  ``t_step`` and the environment of m stay as they are."""
    fields = ("theta", "obs_sum", "obs_sumsq", "obs_count", "obs_mu",
              "obs_nu")
    donors = {}
    for _m, k in transfers:
        if k not in donors:
            donors[k] = {f: getattr(engines[k], f).clone() for f in fields}
    for m, k in transfers:
        dst = engines[m]
        for f in fields:
            # in place, like load_state_dict: nothing aliases the donor
            getattr(dst, f).copy_(donors[k][f])
        dst.adam_m.zero_()
        dst.adam_v.zero_()
