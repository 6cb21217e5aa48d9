"""numpy oracle of the PATA-EC novelty kernels (``ops.pata_ec_codes``,
``ops.env_novelty``).  No GPU, no torch.

An environment is characterised by the clipped, rank-normalised vector of
all agents' scores on it (Enhanced POET's PATA-EC); its novelty is the
mean Euclidean distance to its k nearest neighbours among the reference
environments.  Codes and squared distances are integers, so the kernels
must reproduce ``codes_oracle`` and the ``knn_d2`` of ``knn_oracle``
exactly; only the last step (square roots, their sum, one division) is
floating point, and ``novelty_bound`` is its derived error bound.

The oracle is written independently of the kernels: ranks come from a
sort and ``searchsorted``, not from the kernels' O(K^2) count, and
distances from int64 numpy arithmetic.
"""

import numpy as np


def clip_scores(scores, clip_lo, clip_hi):
    """The kernels' clip: fp32 bounds (the launch passes floats), NaN
    counts as ``clip_lo``, +-inf clip to the bounds."""
    s = np.asarray(scores, dtype=np.float32)
    lo, hi = np.float32(clip_lo), np.float32(clip_hi)
    if not lo <= hi:
        raise ValueError("clip_lo must be <= clip_hi")
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(s, lo), hi)
    return np.where(np.isnan(s), lo, c)


def codes_oracle(scores, clip_lo, clip_hi):
    """int64 ``codes[M][K]`` from ``scores[K][M]``: for every column the
    clipped scores' mid-ranks times two, ``#less + #less_or_equal - 1``, in
    ``[0, 2 (K - 1)]``.  Ties (``-0.0 == +0.0`` included) share a code."""
    c = clip_scores(scores, clip_lo, clip_hi).astype(np.float64)
    if c.ndim != 2:
        raise ValueError("scores must be [K, M]")
    K, M = c.shape
    if K < 2:
        raise ValueError("K must be >= 2")
    codes = np.empty((M, K), dtype=np.int64)
    for m in range(M):
        col = c[:, m]
        srt = np.sort(col)
        less = np.searchsorted(srt, col, side="left")
        less_eq = np.searchsorted(srt, col, side="right")
        codes[m] = less + less_eq - 1
    return codes


def knn_oracle(codes, n_ref, k):
    """``(knn_d2[Q][k'], novelty[Q])`` in int64 / float64 from
    ``codes[M][K]``: queries are rows ``[n_ref, M)``, references rows
    ``[0, n_ref)`` and only those, ``k' = min(k, n_ref)``.  ``knn_d2`` is
    ascending; ``novelty = mean_j sqrt(knn_d2[:, j]) / (2 (K - 1))``."""
    codes = np.asarray(codes, dtype=np.int64)
    M, K = codes.shape
    n_ref, k = int(n_ref), int(k)
    if not 1 <= n_ref < M:
        raise ValueError("need 1 <= n_ref < M")
    if k < 1:
        raise ValueError("k must be >= 1")
    k_eff = min(k, n_ref)
    refs = codes[:n_ref]
    Q = M - n_ref
    knn_d2 = np.empty((Q, k_eff), dtype=np.int64)
    for q in range(Q):
        diff = refs - codes[n_ref + q]
        d2 = np.einsum("rk,rk->r", diff, diff)
        knn_d2[q] = np.sort(d2)[:k_eff]
    novelty = (np.sqrt(knn_d2.astype(np.float64)).sum(axis=1)
               / float(k_eff * 2 * (K - 1)))
    return knn_d2, novelty


def novelty_bound(novelty64, k_eff):
    """Bound on ``|novelty_fp32 - novelty64|`` for the kernel's float tail,
    given that its ``knn_d2`` is exact.  With u = 2^-24, the unit roundoff
    of fp32 round-to-nearest:

    * ``(float)d2``: d2 < 2^30 may not fit 24 bits, relative error <= u;
      the square root halves it: <= u/2 on ``sqrt(d2)``;
    * ``sqrtf`` is correctly rounded: a factor (1 + e), |e| <= u;
    * the k' terms are summed one after another in ascending order, k'-1
      additions of non-negative numbers.  Each partial sum is rounded
      once, and a term passes through at most k'-1 of those roundings, so
      with no cancellation the sum's relative error is <= (k'-1) u to
      first order;
    * the divisor k' * 2 (K-1) <= 65,408 is an exactly representable
      integer and the division is correctly rounded: one more u.

    To first order that is (1/2 + 1 + (k'-1) + 1) u = (k' + 3/2) u.  The
    higher-order terms are below ((k'+2) u)^2 <= 1.6e-11, far inside the
    remaining u/2 = 3e-8, so

        |novelty - oracle| <= (k' + 2) * 2^-24 * oracle.

    The float64 oracle's own error (~1e-16 relative) is negligible
    against it."""
    return (int(k_eff) + 2) * 2.0 ** -24 * np.asarray(novelty64,
                                                      dtype=np.float64)
