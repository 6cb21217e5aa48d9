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


# ---------------------------------------------------------------------------
# Environment reproduction: the open-ended half of POET.
#
#     record = reproduce(pop, scores, archive=archive, ...)
#
# proposes child environments from the pairs that are ready, keeps those
# that pass the minimal criterion (neither too easy nor too hard), ranks
# them by PATA-EC novelty against the active and archived environments
# (ops.env_novelty), admits the most novel as new pairs seeded with the
# agent that does best on them, and retires the oldest pairs when the
# population is over capacity.
# ---------------------------------------------------------------------------


def propose_children(env_A, env_B, parents, n_children, scale, generator):
    """``n_children`` perturbed copies of the environments ``env_A[P][4][4]``,
    ``env_B[P][4]``, taking the parents round-robin from ``parents``.

    Host side and seeded: the draws come from the CPU ``generator`` in a
    fixed order (child by child, env_A then env_B).  Returns
    ``(child_A[C][4][4], child_B[C][4], parent_of[C])`` with CPU tensors
    and a list of parent indices."""
    parents = [int(p) for p in parents]
    n_children = int(n_children)
    if n_children < 0:
        raise ValueError("n_children must be >= 0, got %d" % n_children)
    if n_children and not parents:
        raise ValueError("propose_children needs at least one parent")
    P = env_A.shape[0]
    for p in parents:
        if not 0 <= p < P:
            raise IndexError("parent %d outside 0..%d" % (p, P - 1))
    env_A = env_A.detach().to("cpu", torch.float32)
    env_B = env_B.detach().to("cpu", torch.float32)
    child_A = torch.empty((n_children,) + tuple(env_A.shape[1:]))
    child_B = torch.empty((n_children,) + tuple(env_B.shape[1:]))
    parent_of = []
    for c in range(n_children):
        p = parents[c % len(parents)]
        child_A[c] = env_A[p] + scale * torch.randn(env_A[p].shape,
                                                    generator=generator)
        child_B[c] = env_B[p] + scale * torch.randn(env_B[p].shape,
                                                    generator=generator)
        parent_of.append(p)
    return child_A, child_B, parent_of


def minimal_criterion(child_scores, lo, hi):
    """bool ``[C]`` on the device of ``child_scores[K][C]``: child c passes
    if the best non-NaN score any agent reaches on it lies in ``[lo, hi]``,
    so it is neither too hard nor too easy.  An all-NaN column fails."""
    if child_scores.dim() != 2:
        raise ValueError("child_scores must be [K, C], got %s"
                         % (tuple(child_scores.shape),))
    if child_scores.shape[0] == 0:
        return torch.zeros(child_scores.shape[1], dtype=torch.bool,
                           device=child_scores.device)
    neg_inf = torch.full_like(child_scores, float("-inf"))
    isnan = torch.isnan(child_scores)
    best = torch.where(isnan, neg_inf, child_scores).max(dim=0).values
    return (~isnan.all(dim=0)) & (best >= lo) & (best <= hi)


def select_children(novelty, passed, max_admit):
    """Indices of at most ``max_admit`` children, by novelty descending.
    Only children with ``passed`` set are considered, a NaN novelty never
    wins and ties go to the lowest index.  Returns a list of ints."""
    nov = novelty.detach().to("cpu", torch.float64).tolist()
    ok = passed.detach().to("cpu").tolist()
    if len(nov) != len(ok):
        raise ValueError("%d novelties but %d pass flags"
                         % (len(nov), len(ok)))
    max_admit = int(max_admit)
    if max_admit < 0:
        raise ValueError("max_admit must be >= 0, got %d" % max_admit)
    cand = [c for c in range(len(nov)) if ok[c] and nov[c] == nov[c]]
    cand.sort(key=lambda c: (-nov[c], c))
    return cand[:max_admit]


def _best_agent(column):
    """Row of the best score in a column (list of floats): the lowest
    index wins a tie, NaN never wins; None if every score is NaN."""
    best_k, best = None, None
    for k, v in enumerate(column):
        if v != v:
            continue
        if best is None or v > best:
            best_k, best = k, v
    return best_k


def _empty_record(pop):
    n = pop.cfg.obs_dim
    return {
        "parents": [], "parent_of": [], "admitted": [], "donors": [],
        "novelty": torch.empty(0), "passed": torch.zeros(0, dtype=torch.bool),
        "child_A": torch.empty(0, n, n), "child_B": torch.empty(0, n),
        "retired": (torch.empty(0, n, n), torch.empty(0, n), []),
    }


def reproduce(pop, scores, *, archive=None, repro_threshold, n_children,
              mutate_scale, generator, mc_lo, mc_hi, clip_lo, clip_hi, knn,
              max_admit, max_pairs, child_seeds, horizon, seed, iteration):
    """One POET reproduction step on an ``ESPopulation``.

    ``scores`` is this generation's ``pop.transfer_matrix``; ``archive`` is
    ``None`` or ``(env_A[R][4][4], env_B[R][4])`` of retired environments;
    ``child_seeds[c]`` is the seed (noise stream) child c gets if admitted.

    1. parents: pairs whose own score ``scores[p][p] >= repro_threshold``;
       none gives an empty record;
    2. ``propose_children`` and one ``es_eval_matrix`` launch of all P
       policies on active + archived + child environments;
    3. ``minimal_criterion`` on the child columns and ``ops.env_novelty``
       with ``n_ref = P + |archive|``;
    4. ``select_children`` admits up to ``max_admit``;
    5. the donor of an admitted child is the best agent on its column;
    6. ``pop.add_pairs``;
    7. over ``max_pairs`` the lowest indices (the oldest pairs) are
       removed and returned for the caller's archive.

    Returns a dict: ``parents``, ``parent_of``, ``admitted`` (child
    indices), ``donors``, ``novelty[C]`` and ``passed[C]`` (CPU), the
    proposed ``child_A`` / ``child_B``, and ``retired`` = ``(env_A, env_B,
    seeds)`` as ``remove_pairs`` returns it.  The device is waited for
    once, when the child scores, pass mask and novelties come to the
    host."""
    P = pop.P
    if tuple(scores.shape) != (P, P):
        raise ValueError("scores must be [%d, %d], got %s"
                         % (P, P, tuple(scores.shape)))
    n_children, max_admit = int(n_children), int(max_admit)
    max_pairs = int(max_pairs)
    if max_pairs < 1:
        raise ValueError("max_pairs must be >= 1, got %d" % max_pairs)
    if len(child_seeds) < n_children:
        raise ValueError("%d child_seeds for %d children"
                         % (len(child_seeds), n_children))
    diag = scores.diagonal().detach().to("cpu", torch.float64).tolist()
    parents = [p for p in range(P) if diag[p] >= repro_threshold]
    if not parents or n_children < 1:
        return _empty_record(pop)

    child_A, child_B, parent_of = propose_children(
        pop.env_A, pop.env_B, parents, n_children, mutate_scale, generator)
    dev = pop.device
    parts_A, parts_B = [pop.env_A], [pop.env_B]
    n_arch = 0
    if archive is not None and archive[0].shape[0]:
        n_arch = archive[0].shape[0]
        parts_A.append(archive[0].to(dev, torch.float32))
        parts_B.append(archive[1].to(dev, torch.float32))
    parts_A.append(child_A.to(dev))
    parts_B.append(child_B.to(dev))
    all_scores = ops.es_eval_matrix(
        pop.theta, pop.obs_mu, pop.obs_nu, torch.cat(parts_A).contiguous(),
        torch.cat(parts_B).contiguous(), seed, iteration, horizon)
    n_ref = P + n_arch
    child_scores = all_scores[:, n_ref:]
    passed = minimal_criterion(child_scores, mc_lo, mc_hi)
    novelty = ops.env_novelty(all_scores, n_ref, knn, clip_lo, clip_hi)

    child_cpu = child_scores.to("cpu", torch.float64)  # the host sync
    passed, novelty = passed.cpu(), novelty.cpu()
    admitted = select_children(novelty, passed, max_admit)
    donors = [_best_agent(child_cpu[:, c].tolist()) for c in admitted]
    pop.add_pairs([child_seeds[c] for c in admitted],
                  [(child_A[c], child_B[c]) for c in admitted], donors)
    retired = _empty_record(pop)["retired"]
    if pop.P > max_pairs:
        retired = pop.remove_pairs(range(pop.P - max_pairs))
    return {
        "parents": parents, "parent_of": parent_of, "admitted": admitted,
        "donors": donors, "novelty": novelty, "passed": passed,
        "child_A": child_A, "child_B": child_B, "retired": retired,
    }
