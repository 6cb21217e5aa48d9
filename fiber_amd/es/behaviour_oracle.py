"""float64 oracle of the novelty-search kernels and host mirrors of the
NoveltyESEngine bookkeeping.  CPU only: numpy, no torch, no GPU.

Two things are held to it (tests/gpu/test_novelty_es_gpu.py):

* the behaviour characterisation (BC) that ``ops.es_rollout_mlp_bc`` and
  ``ops.es_eval_bc`` report, against the per-episode rollout oracle
  (``rollout_oracle``), see ``bc_of_rollout``;
* ``ops.bc_knn_novelty`` against a brute-force float64 k-nearest-neighbour
  search, see ``knn_novelty`` and ``knn_bounds``.

Every bound below is derived from the kernels' arithmetic and evaluated on
the oracle's own magnitudes.  No constant comes from a GPU run.

Bound of ``bc_knn_novelty``
---------------------------
With U = 2^-24, the unit roundoff of fp32 round-to-nearest, and query q,
archive row a (both exact fp32 inputs), the kernel computes

    d_i  = fl(q_i - a_i)                        i = 0..3
    acc  = fl(d_0 d_0);  acc = fl(d_i d_i + acc)  i = 1..3   (fma)

* each d_i carries one rounding, so d_i^2 carries a factor (1+e)^2;
* the term d_0^2 then passes the rounding of its own product and of the
  three fmas, the term d_i^2 that of fmas i..3: at most 4 more factors.
  All terms are non-negative, so nothing cancels and

      |d2_fp32 - d2| <= ((1 + U)^6 - 1) d2 + UNDERFLOW,

  6 U d2 to first order.  UNDERFLOW = 4 * 2^-126 covers the four rounded
  operations of the sum should a result fall below the normal range, where
  the error is absolute (below 2^-126 per operation even if the hardware
  flushes denormals to zero) instead of relative.  It is nil unless
  distances are below 1e-19; it is what keeps the bound positive at d2 = 0.
  A query equal to an archive row gives d_i = 0 and d2 = 0 exactly;
* the reported distance is sqrtf(d2_fp32), taken as accurate to 1 ulp:
  a factor (1 + e), |e| <= ULP = 2^-23.  With b2 the bound on d2,

      sqrt(max(d2 - b2, 0)) (1 - ULP) <= dist_fp32 <= sqrt(d2 + b2) (1 + ULP),

  which is (3 U + ULP) dist = 5 U dist to first order;
* selection.  The kernel picks its k nearest by the fp32 d2, not the exact
  one.  Order statistics are monotone in every coordinate and 1-Lipschitz
  in the sup norm: if every fp32 value lies in [lo(d2_r), hi(d2_r)] for
  non-decreasing lo, hi, the j-th smallest fp32 value lies in
  [lo(d2_(j)), hi(d2_(j))], d2_(j) the j-th smallest exact value.  So
  ``knn_d2[j]`` is compared with the j-th smallest exact d2 under the
  bound evaluated there, whichever archive row the kernel actually chose,
  and far rows, whose absolute errors are larger, do not enter;
* novelty = fl(sum_j dist_j) / k: k - 1 rounded adds of non-negative
  terms in ascending order and one rounded division by the exact integer
  k, a factor within (1 + U)^k of the sum of the fp32 distances.

The float64 arithmetic of the oracle itself is about 1e-16 relative, nine
orders below these bounds.
"""

import numpy as np

from . import rollout_oracle

U = rollout_oracle.U        # 2^-24
ULP = rollout_oracle.ULP    # 2^-23
BC_DIM = 4
KNN_MAX = 16                # BC_KNN_MAX of the kernel
D2_REL = (1.0 + U) ** 6 - 1.0
UNDERFLOW = 4.0 * 2.0 ** -126


# ---- behaviour characterisation of an oracle rollout ----------------------

def bc_of_rollout(ro, horizon):
    """``(bc[4], tol[4])`` of one member or cell from its oracle rollout:
    the mean over the 64 envs of ``ro.states[:, horizon]`` and the bound on
    ``|kernel's bc - it|``, valid while every env is decided through
    ``horizon`` steps.  Each final state is within ``state_err`` of the
    kernel's; the kernel sums the 64 fp32 values of a dim in a 6-level
    shuffle tree, each value passing 6 rounded adds, and divides by 64
    exactly: ``mean(state_err) + 6 U mean|s|``."""
    s = ro.states[:, horizon]
    err = ro.state_err[:, horizon]
    return s.mean(axis=0), err.mean(axis=0) + 6.0 * U * np.abs(s).mean(axis=0)


# ---- brute-force kNN novelty ------------------------------------------------

def _as_fp32_rows(a, name):
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError("%s must be float32 (the kernel's exact inputs)"
                        % name)
    if a.ndim != 2 or a.shape[1] != BC_DIM:
        raise ValueError("%s must be [*, %d]" % (name, BC_DIM))
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % name)
    return a.astype(np.float64)


def knn_novelty(bc, archive, k):
    """``(knn_d2[N][k], novelty[N])`` in float64 for fp32 ``bc[N][4]`` and
    ``archive[R][4]``: the k smallest exact squared distances of every
    query in ascending order (duplicate rows are separate neighbours) and
    the mean of their square roots.  ``1 <= k <= min(R, 16)``."""
    q = _as_fp32_rows(bc, "bc")
    a = _as_fp32_rows(archive, "archive")
    k = int(k)
    if a.shape[0] < 1:
        raise ValueError("the archive is empty")
    if k < 1 or k > min(a.shape[0], KNN_MAX):
        raise ValueError("k must be in [1, min(R, %d)]" % KNN_MAX)
    diff = q[:, None, :] - a[None, :, :]          # exact in float64
    d2 = (diff * diff).sum(axis=-1)               # [N][R]
    knn_d2 = np.partition(d2, k - 1, axis=1)[:, :k]
    knn_d2.sort(axis=1)
    return knn_d2, np.sqrt(knn_d2).mean(axis=1)


def d2_bound(d2):
    """Bound on ``|fp32 squared distance - d2|`` (module docstring)."""
    return D2_REL * np.asarray(d2, dtype=np.float64) + UNDERFLOW


def dist_interval(d2):
    """``(lo, hi)`` enclosing the kernel's ``sqrtf`` of the fp32 squared
    distance whose exact value is ``d2``."""
    d2 = np.asarray(d2, dtype=np.float64)
    b2 = d2_bound(d2)
    lo = np.sqrt(np.maximum(d2 - b2, 0.0)) * (1.0 - ULP)
    hi = np.sqrt(d2 + b2) * (1.0 + ULP)
    return lo, hi


def knn_bounds(knn_d2):
    """``(d2_tol[N][k], novelty_tol[N])`` for the oracle's ascending
    ``knn_d2``: the bound on ``|kernel's knn_d2[q][j] - knn_d2[q][j]|`` and
    on ``|kernel's novelty[q] - novelty[q]|``."""
    knn_d2 = np.asarray(knn_d2, dtype=np.float64)
    k = knn_d2.shape[1]
    dist = np.sqrt(knn_d2)
    lo, hi = dist_interval(knn_d2)
    grow = (1.0 + U) ** k
    nov = dist.mean(axis=1)
    nov_hi = hi.mean(axis=1) * grow
    nov_lo = lo.mean(axis=1) / grow
    return d2_bound(knn_d2), np.maximum(nov_hi - nov, nov - nov_lo)


# ---- host mirrors of the engine's bookkeeping -------------------------------

MODES = ("ns", "nsr", "nsra")


def combine_weights(mode, rank_fitness, rank_novelty, weight=1.0):
    """Member weights from the centered ranks of fitness and novelty, in
    float64: NS-ES follows novelty alone, NSR-ES the average of the two,
    NSRA-ES ``w * fitness + (1 - w) * novelty``."""
    rf = np.asarray(rank_fitness, dtype=np.float64)
    rn = np.asarray(rank_novelty, dtype=np.float64)
    if rf.shape != rn.shape:
        raise ValueError("rank shapes differ")
    if mode == "ns":
        return rn.copy()
    if mode == "nsr":
        return 0.5 * (rf + rn)
    if mode == "nsra":
        w = float(weight)
        return w * rf + (1.0 - w) * rn
    raise ValueError("mode must be one of %s, got %r" % (MODES, mode))


def nsra_update(weight, best, stall, score, delta, patience):
    """One step of the NSRA-ES schedule: ``(weight, best, stall)`` after an
    updated agent scored ``score``.  A new best raises the fitness weight
    by ``delta`` (at most 1) and clears the stall count; otherwise the
    count grows, and on reaching ``patience`` the weight drops by ``delta``
    (at least 0) and the count clears."""
    if score > best:
        return min(1.0, weight + delta), score, 0
    stall += 1
    if stall >= patience:
        return max(0.0, weight - delta), best, 0
    return weight, best, stall


class ArchiveMirror:
    """The engine's archive: at most ``capacity`` rows, first in first out.
    Row ``total % capacity`` of the ring is overwritten by each append."""

    def __init__(self, capacity):
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.capacity = int(capacity)
        self.ring = np.zeros((self.capacity, BC_DIM), dtype=np.float32)
        self.total = 0

    @property
    def count(self):
        return min(self.total, self.capacity)

    def append(self, bc):
        self.ring[self.total % self.capacity] = np.asarray(
            bc, dtype=np.float32).reshape(BC_DIM)
        self.total += 1

    def rows(self):
        """The archived rows, oldest first."""
        if self.total <= self.capacity:
            return self.ring[: self.total].copy()
        head = self.total % self.capacity
        return np.concatenate([self.ring[head:], self.ring[:head]])


def choice_probabilities(novelty):
    """Probability of picking each agent of the meta-population: in
    proportion to the novelty of its current BC, uniform when every novelty
    is 0."""
    nov = np.asarray(novelty, dtype=np.float64)
    if nov.ndim != 1 or nov.size < 1:
        raise ValueError("novelty must be a non-empty vector")
    if (nov < 0).any() or not np.isfinite(nov).all():
        raise ValueError("novelty must be finite and >= 0")
    total = nov.sum()
    if total == 0.0:
        return np.full(nov.size, 1.0 / nov.size)
    return nov / total
