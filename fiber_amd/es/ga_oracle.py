"""Numpy oracle of the Deep GA kernels (fiber_amd/csrc/ops/ga_kernels.hip)
and of GAEngine's bookkeeping.  Runs anywhere; nothing here comes from a GPU
run.  Derivations: profiles/ga.md.

  parents_exact   ga_parents, integer for integer
  truncate_exact  ga_truncate's order rule, by a stable sort
  lineage_step    the seed-chain gather of one generation
  decode_fp64     ga_decode in float64 with a per-element bound
  member_rollout  one member of ga_rollout_mlp through rollout_oracle
"""

import numpy as np

from . import philox_ref
from . import rollout_oracle
from .rollout_oracle import NPARAMS, U, Z_REL

TAG_GA_PARENT = np.uint32(0x45530004)


def parents_exact(seed, gen, pop, n_elite, T_cur):
    """int32 (parent_idx[pop], slot[pop]) of generation ``gen``: members
    below ``n_elite`` are the survivors of that index, unmutated (slot -1);
    member m above them mutates survivor ``(u_m * T_cur) >> 32`` with the
    draw of slot m, ``u_m`` the first word of philox4x32_10 keyed (seed,
    gen) at counter (m, 0, TAG_GA_PARENT, 0)."""
    pop, n_elite, T_cur = int(pop), int(n_elite), int(T_cur)
    if not 0 <= n_elite <= min(T_cur, pop) or T_cur < 1 or pop < 1:
        raise ValueError("need 0 <= n_elite <= min(T_cur, pop), got "
                         "n_elite %d, T_cur %d, pop %d"
                         % (n_elite, T_cur, pop))
    m = np.arange(pop, dtype=np.uint32)
    u = philox_ref.philox4x32_10(
        np.uint32(int(seed) & 0xFFFFFFFF), np.uint32(int(gen) & 0xFFFFFFFF),
        m, np.uint32(0), TAG_GA_PARENT, np.uint32(0))[0]
    parent_idx = ((u.astype(np.uint64) * np.uint64(T_cur))
                  >> np.uint64(32)).astype(np.int32)
    slot = m.astype(np.int32)
    parent_idx[:n_elite] = np.arange(n_elite, dtype=np.int32)
    slot[:n_elite] = -1
    return parent_idx, slot


def truncate_exact(f, T):
    """order[T]: the indices of the T best of ``f`` in descending order,
    ties by ascending index, NaNs after every number (and by index among
    themselves), -0 equal to +0.  A stable three-key sort, written without
    reference to the kernel's comparison count."""
    f = np.asarray(f)
    n, T = f.size, int(T)
    if f.ndim != 1 or n < 2 or not 1 <= T <= n:
        raise ValueError("need a vector of n >= 2 and 1 <= T <= n, got "
                         "shape %s, T %d" % (f.shape, T))
    nan = np.isnan(f)
    # descending value = ascending negation; -(+0) and -(-0) compare equal
    neg = -np.where(nan, 0.0, f.astype(np.float64))
    # lexsort: the last key is the primary one
    order = np.lexsort((np.arange(n), neg, nan))
    return order[:T].astype(np.int32)


def lineage_step(lineage, parent_idx, slot, order, g):
    """The seed chains after generation ``g``: survivor t is member
    ``order[t]``, which inherits columns [0, g) of its parent's chain and
    gets its own slot (or -1) in column g.  Returns int32 [T][g + 1]."""
    lineage = np.asarray(lineage)
    order = np.asarray(order)
    g = int(g)
    new = np.empty((order.size, g + 1), dtype=np.int32)
    new[:, :g] = lineage[np.asarray(parent_idx)[order], :g]
    new[:, g] = np.asarray(slot)[order]
    return new


def decode_fp64(theta0, rows, sigma, seed):
    """(value, tol), both float64 [N][NPARAMS]: ga_decode of the int
    chains ``rows[N][G]`` and the bound on |device - value|.

    Per applied generation the device forms ``acc = fma(sigma, z, acc)``
    from its own draw; here the float64 sum uses numpy's.  The two draws
    agree to Z_REL, the product and sum round once (U of the result), and
    the bound on the previous acc carries over unchanged:
    ``tol += |sigma z| (Z_REL + U) + U |acc|``.  First order, like the other
    oracles: the device rounds its own sum ``acc_d``, not the oracle's
    ``acc``, and ``U |acc_d|`` exceeds ``U |acc|`` by at most U times the
    bound so far (about 6e-8 * 5e-7 here); that second-order term is
    dropped.  A generation with a negative entry adds nothing, so an
    elite-only chain has tol 0."""
    th = np.asarray(theta0, dtype=np.float32).astype(np.float64)
    assert th.shape == (NPARAMS,)
    rows = np.asarray(rows)
    assert rows.ndim == 2
    sig = float(np.float32(sigma))
    value = np.empty((rows.shape[0], NPARAMS))
    tol = np.empty_like(value)
    for n, row in enumerate(rows):
        acc = th.copy()
        bound = np.zeros(NPARAMS)
        for c, s in enumerate(row):
            if s < 0:
                continue
            z = philox_ref.noise_for_pair(seed, c, int(s), NPARAMS)
            sz = sig * z.astype(np.float64)
            acc = acc + sz
            bound += np.abs(sz) * (Z_REL + U) + U * np.abs(acc)
        value[n], tol[n] = acc, bound
    return value, tol


def member_rollout(parent_row, sigma, seed, gen, slot, horizon, obs_mu,
                   obs_nu, env_A, env_B):
    """One block of ga_rollout_mlp: ``parent_row`` as it is for ``slot <
    0``, otherwise perturbed by +sigma times the draw of ``slot`` in
    generation ``gen``; the episodes start from the states of (seed,
    gen)."""
    s0, s0_err = rollout_oracle.init_states(seed, gen)
    if slot < 0:
        pol = rollout_oracle.make_policy(parent_row)
    else:
        z = philox_ref.noise_for_pair(seed, gen, int(slot), NPARAMS)
        pol = rollout_oracle.make_policy(parent_row, float(sigma), z)
    return rollout_oracle.rollout(pol, obs_mu, obs_nu, env_A, env_B, s0,
                                  horizon, s0_err)
