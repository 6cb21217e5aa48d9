"""Python wrappers for the CDNA4 ES kernels (fiber_amd._ops).

Fail-loud policy: on a machine with a GPU, a missing/unbuilt extension is
an error — there is deliberately NO eager/PyTorch fallback for the hot
ops, so a silently-degraded bench is impossible.
"""

import torch

_OPS = None
_IMPORT_ERROR = None

try:
    from fiber_amd import _ops as _OPS  # built in-tree by setup.py
except ImportError as exc:  # pragma: no cover
    _IMPORT_ERROR = exc


NPARAMS = _OPS.NPARAMS if _OPS else 4610
ENVS_PER_MEMBER = _OPS.ENVS_PER_MEMBER if _OPS else 64
OBS_DIM = 4
ACT_DIM = 2
HIDDEN = 64


def _require_ops():
    if _OPS is None:
        raise RuntimeError(
            "fiber_amd._ops (gfx950 HIP extension) is not built: %r. "
            "Run `python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)." % (_IMPORT_ERROR,)
        )
    return _OPS


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(t, name, dtype=torch.float32, device=True):
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if device and not t.is_cuda:
        raise TypeError("%s must be a CUDA (ROCm) tensor" % name)
    if not t.is_contiguous():
        raise TypeError("%s must be contiguous" % name)
    return t


def _partial_buffer(device, numel):
    """Scratch for per-block partial sums that a second kernel reduces in a
    fixed order (what keeps the reductions reproducible run to run).
    Allocated per call on the current stream, the one both kernels are
    launched on, so the caching allocator only hands the block out again
    after them in stream order: safe with several engines or streams."""
    return torch.empty(numel, dtype=torch.float32, device=device)


def es_rollout_mlp(theta, sigma, seed, iteration, horizon, member_offset,
                   pop_shard, obs_mu, obs_nu, env_A, env_B):
    """One persistent-kernel launch rolling out ``pop_shard`` perturbed
    members x 64 envs for ``horizon`` steps.  Returns (fitness[pop_shard],
    obs_stat[2*OBS+1]) on device."""
    ops = _require_ops()
    _check(theta, "theta")
    assert theta.numel() == NPARAMS
    fitness = torch.empty(pop_shard, dtype=torch.float32,
                          device=theta.device)
    obs_stat = torch.zeros(2 * OBS_DIM + 1, dtype=torch.float32,
                           device=theta.device)
    part = _partial_buffer(theta.device, int(pop_shard) * 2 * OBS_DIM)
    ops.es_rollout_mlp(
        theta.data_ptr(), float(sigma), int(seed) & 0xFFFFFFFF,
        int(iteration) & 0xFFFFFFFF, int(horizon), int(member_offset),
        int(pop_shard), _check(obs_mu, "obs_mu").data_ptr(),
        _check(obs_nu, "obs_nu").data_ptr(),
        _check(env_A, "env_A").data_ptr(),
        _check(env_B, "env_B").data_ptr(), fitness.data_ptr(),
        part.data_ptr(), obs_stat.data_ptr(), _stream())
    return fitness, obs_stat


def es_eval_matrix(thetas, obs_mu, obs_nu, env_A, env_B, seed, iteration,
                   horizon, return_episodes=False):
    """Roll out K explicit (unperturbed) policies on M environments in one
    launch, one workgroup per (policy, environment) cell.

    ``thetas[K][NPARAMS]``, ``obs_mu[K][4]`` / ``obs_nu[K][4]`` (each
    policy owns its normaliser), ``env_A[M][4][4]``, ``env_B[M][4]``.  The
    64 episodes per cell start from the same states as ``es_rollout_mlp``
    at (seed, iteration) and run the same step loop, so ``scores[k][m]``
    is bit-identical to that kernel's fitness for ``thetas[k]`` at
    ``sigma=0``.  Returns ``scores[K][M]`` (mean return over the 64
    episodes), or ``(scores, episodes[K][M][64])``.

    Every argument is validated before anything is launched: TypeError
    for dtype, device or contiguity, ValueError for shape or horizon."""
    ops = _require_ops()
    named = (("thetas", thetas), ("obs_mu", obs_mu), ("obs_nu", obs_nu),
             ("env_A", env_A), ("env_B", env_B))
    for name, t in named:
        _check(t, name)
        if t.device != thetas.device:
            raise TypeError("%s is on %s, thetas on %s"
                            % (name, t.device, thetas.device))
    if thetas.dim() != 2 or thetas.shape[1] != NPARAMS:
        raise ValueError("thetas must be [K, %d], got %s"
                         % (NPARAMS, tuple(thetas.shape)))
    K = thetas.shape[0]
    if env_A.dim() != 3 or tuple(env_A.shape[1:]) != (OBS_DIM, OBS_DIM):
        raise ValueError("env_A must be [M, %d, %d], got %s"
                         % (OBS_DIM, OBS_DIM, tuple(env_A.shape)))
    M = env_A.shape[0]
    for name, t, want in (("obs_mu", obs_mu, (K, OBS_DIM)),
                          ("obs_nu", obs_nu, (K, OBS_DIM)),
                          ("env_B", env_B, (M, OBS_DIM))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if K * M >= 2 ** 31:
        raise ValueError("K*M = %d exceeds the launch grid" % (K * M))
    device = thetas.device
    scores = torch.empty(K, M, dtype=torch.float32, device=device)
    episodes = None
    if return_episodes:
        episodes = torch.empty(K, M, ENVS_PER_MEMBER, dtype=torch.float32,
                               device=device)
    with torch.cuda.device(device):
        ops.es_eval_matrix(
            thetas.data_ptr(), obs_mu.data_ptr(), obs_nu.data_ptr(),
            env_A.data_ptr(), env_B.data_ptr(), int(seed) & 0xFFFFFFFF,
            int(iteration) & 0xFFFFFFFF, horizon, K, M, scores.data_ptr(),
            episodes.data_ptr() if return_episodes else 0, _stream())
    if return_episodes:
        return scores, episodes
    return scores


def es_grad(wpair, pair_begin, pair_end, seed, iteration, device,
            nparams=None):
    """Noise-weighted gradient over local pairs; eps regenerated on-chip."""
    ops = _require_ops()
    _check(wpair, "wpair")
    if nparams is None:
        nparams = NPARAMS
    grad = torch.zeros(nparams, dtype=torch.float32, device=device)
    chunks = ops.es_grad_chunks(int(pair_end) - int(pair_begin),
                                int(nparams))
    part = _partial_buffer(grad.device, chunks * int(nparams))
    ops.es_grad(wpair.data_ptr(), int(pair_begin), int(pair_end),
                int(seed) & 0xFFFFFFFF, int(iteration) & 0xFFFFFFFF,
                int(nparams), part.data_ptr(), grad.data_ptr(), _stream())
    return grad


_rank_workspace = {}  # device -> (n, uint8 tensor); grow-only cache


def centered_rank(fitness):
    """Centered rank transform in [-0.5, 0.5].

    The O(n^2) comparison kernel wins for small populations (one launch,
    no sort); past 16k members (e.g. the named 8-GPU config at pop
    131,072) a stable device radix sort (rocPRIM) + scatter takes over —
    identical output incl. the index-order tie-break."""
    _check(fitness, "fitness")
    n = fitness.numel()
    if n < 2:
        # rank / (n - 1) is 0/0 for a single member
        raise ValueError("centered_rank needs at least 2 members, got %d"
                         % n)
    ops = _require_ops()
    out = torch.empty_like(fitness)
    if n > 16384:
        dev = fitness.device
        cached = _rank_workspace.get(dev)
        if cached is None or cached[0] < n:
            need = ops.centered_rank_sorted_workspace(n)
            cached = (n, torch.empty(need, dtype=torch.uint8, device=dev))
            _rank_workspace[dev] = cached
        ws = cached[1]
        ops.centered_rank_sorted(fitness.data_ptr(), n, out.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream())
        return out
    ops.centered_rank(fitness.data_ptr(), n, out.data_ptr(), _stream())
    return out


def centered_rank_ref(fitness):
    """Pure-torch fp32 reference (any device) for tests."""
    n = fitness.numel()
    order = torch.argsort(torch.argsort(fitness, stable=True))
    return order.float() / (n - 1) - 0.5


def _check_forward_batch(batch):
    """The kernel indexes ``x`` with a 32-bit ``row * OBS_DIM + d``."""
    if batch < 0 or batch * OBS_DIM >= 2 ** 31:
        raise ValueError("batch = %d: row * %d leaves the int32 index range"
                         % (batch, OBS_DIM))
    return batch


def mlp_policy_forward(theta, x, out=None):
    """Batched policy forward via the MFMA path: ``logits[batch][2]`` for
    ``x[batch][4]`` and the flat ``theta[NPARAMS]``, all fp32 on one device.

    ``x`` is used as it is: the rollout kernels feed the policy the
    normalised, clamped observation, and so must the caller
    (``ESEngine.act`` does).  ``x``, ``h1`` and ``h2`` are rounded to bf16;
    the rollout step loop keeps ``h2`` in fp32, so its logits differ from
    these by up to ``sum_i |w3[a][i]| * spacing(h2_i) / 2``
    (profiles/forward_oracle.md).

    ``out``, if given, is contiguous fp32 ``[batch][2]`` storage on the
    device of ``x``; it is written and returned.  Rows are independent: a
    non-finite row of ``x`` gives non-finite logits in that row only.
    ``batch == 0`` returns an empty ``[0][2]`` tensor without a launch.

    Everything is validated before the launch: TypeError for dtype, device
    or contiguity, ValueError for a shape or a batch past the kernel's
    32-bit index."""
    ops = _require_ops()
    named = [("theta", theta), ("x", x)]
    if out is not None:
        named.append(("out", out))
    for name, t in named:
        _check(t, name)
        if t.device != x.device:
            raise TypeError("%s is on %s, x on %s"
                            % (name, t.device, x.device))
    if tuple(theta.shape) != (NPARAMS,):
        raise ValueError("theta must be [%d], got %s"
                         % (NPARAMS, tuple(theta.shape)))
    if x.dim() != 2 or x.shape[1] != OBS_DIM:
        raise ValueError("x must be [batch, %d], got %s"
                         % (OBS_DIM, tuple(x.shape)))
    batch = _check_forward_batch(x.shape[0])
    if out is not None and tuple(out.shape) != (batch, ACT_DIM):
        raise ValueError("out must be [%d, %d], got %s"
                         % (batch, ACT_DIM, tuple(out.shape)))
    logits = out if out is not None else torch.empty(
        batch, ACT_DIM, dtype=torch.float32, device=x.device)
    if batch == 0:
        return logits
    with torch.cuda.device(x.device):
        ops.mlp_policy_forward(theta.data_ptr(), x.data_ptr(), batch,
                               logits.data_ptr(), _stream())
    return logits


def mlp_policy_forward_ref(theta, x):
    """fp32 torch reference of the same policy (tests compare this to the
    bf16 MFMA kernel with a loose tolerance)."""
    w1 = theta[:256].view(HIDDEN, OBS_DIM)
    b1 = theta[256:320]
    w2 = theta[320:4416].view(HIDDEN, HIDDEN)
    b2 = theta[4416:4480]
    w3 = theta[4480:4608].view(ACT_DIM, HIDDEN)
    b3 = theta[4608:4610]
    # the kernel rounds every operand to bf16 before the matmuls
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    h1 = torch.tanh(bf(x) @ bf(w1).T + b1)
    h2 = torch.tanh(bf(h1) @ bf(w2).T + b2)
    return bf(h2) @ bf(w3).T + b3


def mfma_gemm64_probe(a, b):
    """C = tanh(A @ B) for 64x64 fp32 inputs through the MFMA strip path
    (hardware verification of the fragment layout assumptions)."""
    ops = _require_ops()
    _check(a, "a")
    _check(b, "b")
    out_t = torch.empty(64, 64, dtype=torch.float32, device=a.device)
    ops.mfma_gemm64_probe(a.data_ptr(), b.data_ptr(), out_t.data_ptr(),
                          _stream())
    # kernel stores C transposed ([col][row]); undo here
    return out_t.T.contiguous()


def logits_reduce_probe(p0, p1):
    """The rollout loop's cross-lane logits reduce on its own: for per-lane
    partials ``p0[4][64]``, ``p1[4][64]`` (4 column tiles x 64 lanes)
    returns ``(shfl, swap)``, the ``[64 env][2 logits]`` partial row as
    written by the shfl_xor tree and by the permlane-swap form the step
    loop runs.  The two must agree bit for bit."""
    ops = _require_ops()
    for name, t in (("p0", p0), ("p1", p1)):
        _check(t, name)
        if tuple(t.shape) != (4, 64):
            raise ValueError("%s must be [4, 64], got %s"
                             % (name, tuple(t.shape)))
    if p1.device != p0.device:
        raise TypeError("p1 is on %s, p0 on %s" % (p1.device, p0.device))
    shfl = torch.empty(ENVS_PER_MEMBER, ACT_DIM, dtype=torch.float32,
                       device=p0.device)
    swap = torch.empty_like(shfl)
    with torch.cuda.device(p0.device):
        ops.logits_reduce_probe(p0.data_ptr(), p1.data_ptr(),
                                shfl.data_ptr(), swap.data_ptr(), _stream())
    return shfl, swap


# ---------------------------------------------------------------------------
# Per-pair batched ops: P independent (policy, environment) pairs per
# launch, each with its own theta, normaliser, environment and noise seed.
# For pair p every op returns the bits of its single-pair counterpart.
# ---------------------------------------------------------------------------

PAIRS_MAX = 65535           # the pair index rides grid.y / grid.z
RANK_PAIRS_MAX_N = 16384    # where centered_rank switches to the radix path


def pair_seeds(seeds, device):
    """int32 device tensor [P] carrying the 32-bit patterns of the Python
    ints ``seeds``, masked with the same ``& 0xFFFFFFFF`` that the scalar
    ops apply to their ``seed`` argument."""
    vals = []
    for s in seeds:
        v = int(s) & 0xFFFFFFFF
        vals.append(v - (1 << 32) if v >= (1 << 31) else v)
    return torch.tensor(vals, dtype=torch.int32).to(device).contiguous()


def _check_pairs_on(named, anchor_name, anchor):
    """dtype / device / contiguity of every (name, tensor, dtype), all on
    the device of ``anchor``."""
    for name, t, dtype in named:
        _check(t, name, dtype=dtype)
        if t.device != anchor.device:
            raise TypeError("%s is on %s, %s on %s"
                            % (name, t.device, anchor_name, anchor.device))


def _check_pair_count(P):
    if P < 1 or P > PAIRS_MAX:
        raise ValueError("P must be in [1, %d], got %d" % (PAIRS_MAX, P))


def es_rollout_mlp_pairs(thetas, sigma, seeds, iteration, horizon, pop,
                         obs_mu, obs_nu, env_A, env_B):
    """``pop`` perturbed members for each of P pairs in one launch, one
    workgroup per (pair, member).

    ``thetas[P][NPARAMS]``, ``seeds`` int32 ``[P]`` (see ``pair_seeds``),
    ``obs_mu[P][4]``, ``obs_nu[P][4]``, ``env_A[P][4][4]``,
    ``env_B[P][4]``; ``sigma``, ``iteration`` and ``horizon`` are shared.
    Returns ``(fitness[P][pop], obs_stat[P][9])``; row p of both is
    bit-identical to ``es_rollout_mlp(thetas[p], sigma, seed_p, iteration,
    horizon, 0, pop, obs_mu[p], obs_nu[p], env_A[p], env_B[p])``.

    Every argument is validated before anything is launched: TypeError
    for dtype, device or contiguity, ValueError for shapes and sizes."""
    ops = _require_ops()
    _check_pairs_on(
        (("thetas", thetas, torch.float32), ("seeds", seeds, torch.int32),
         ("obs_mu", obs_mu, torch.float32), ("obs_nu", obs_nu, torch.float32),
         ("env_A", env_A, torch.float32), ("env_B", env_B, torch.float32)),
        "thetas", thetas)
    if thetas.dim() != 2 or thetas.shape[1] != NPARAMS:
        raise ValueError("thetas must be [P, %d], got %s"
                         % (NPARAMS, tuple(thetas.shape)))
    P = thetas.shape[0]
    _check_pair_count(P)
    for name, t, want in (("seeds", seeds, (P,)),
                          ("obs_mu", obs_mu, (P, OBS_DIM)),
                          ("obs_nu", obs_nu, (P, OBS_DIM)),
                          ("env_A", env_A, (P, OBS_DIM, OBS_DIM)),
                          ("env_B", env_B, (P, OBS_DIM))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    pop, horizon = int(pop), int(horizon)
    if pop < 2 or pop % 2:
        raise ValueError("pop must be even and >= 2 (antithetic pairs), "
                         "got %d" % pop)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if P * pop >= 2 ** 31:
        raise ValueError("P*pop = %d exceeds the launch grid" % (P * pop))
    device = thetas.device
    fitness = torch.empty(P, pop, dtype=torch.float32, device=device)
    obs_stat = torch.zeros(P, 2 * OBS_DIM + 1, dtype=torch.float32,
                           device=device)
    with torch.cuda.device(device):
        part = _partial_buffer(device, P * pop * 2 * OBS_DIM)
        ops.es_rollout_mlp_pairs(
            thetas.data_ptr(), float(sigma), seeds.data_ptr(),
            int(iteration) & 0xFFFFFFFF, horizon, P, pop, obs_mu.data_ptr(),
            obs_nu.data_ptr(), env_A.data_ptr(), env_B.data_ptr(),
            fitness.data_ptr(), part.data_ptr(), obs_stat.data_ptr(),
            _stream())
    return fitness, obs_stat


def centered_rank_pairs(fitness):
    """Centered rank of every row of ``fitness[P][n]`` in one launch:
    ``ranks[p]`` is bit-identical to ``centered_rank(fitness[p])``, the
    index-order tie-break included.  Only the O(n^2) comparison kernel is
    batched, so ``n`` stops at 16384."""
    ops = _require_ops()
    _check(fitness, "fitness")
    if fitness.dim() != 2:
        raise ValueError("fitness must be [P, n], got %s"
                         % (tuple(fitness.shape),))
    P, n = fitness.shape
    _check_pair_count(P)
    if n < 2:
        raise ValueError("n must be >= 2, got %d" % n)
    if n > RANK_PAIRS_MAX_N:
        raise ValueError("n = %d exceeds %d, the limit of the batched rank"
                         % (n, RANK_PAIRS_MAX_N))
    out = torch.empty_like(fitness)
    with torch.cuda.device(fitness.device):
        ops.centered_rank_pairs(fitness.data_ptr(), P, n, out.data_ptr(),
                                _stream())
    return out


def es_grad_pairs(wpair, seeds, iteration):
    """Noise-weighted gradient of every pair: ``grad[P][NPARAMS]`` from
    ``wpair[P][pop/2]`` and the int32 ``seeds[P]``.  Row p is bit-identical
    to ``es_grad(wpair[p], 0, pop/2, seed_p, iteration, device)``: the
    same chunk split, partials summed in chunk order."""
    ops = _require_ops()
    _check_pairs_on((("wpair", wpair, torch.float32),
                     ("seeds", seeds, torch.int32)), "wpair", wpair)
    if wpair.dim() != 2 or wpair.shape[1] < 1:
        raise ValueError("wpair must be [P, pop/2], got %s"
                         % (tuple(wpair.shape),))
    P, npairs = wpair.shape
    _check_pair_count(P)
    if tuple(seeds.shape) != (P,):
        raise ValueError("seeds must be [%d], got %s"
                         % (P, tuple(seeds.shape)))
    if 2 * P * npairs >= 2 ** 31:
        raise ValueError("P*pop = %d exceeds the launch grid"
                         % (2 * P * npairs))
    device = wpair.device
    grad = torch.empty(P, NPARAMS, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        chunks = ops.es_grad_chunks(npairs, NPARAMS)
        part = _partial_buffer(device, P * chunks * NPARAMS)
        ops.es_grad_pairs(wpair.data_ptr(), P, npairs, seeds.data_ptr(),
                          int(iteration) & 0xFFFFFFFF, NPARAMS,
                          part.data_ptr(), grad.data_ptr(), _stream())
    return grad


# ---------------------------------------------------------------------------
# PATA-EC environment novelty (poet_kernels.hip): integer rank codes per
# environment and exact k-nearest-neighbour squared distances between them.
# ---------------------------------------------------------------------------

PATA_K_MAX = 512    # D2 <= K * 4 (K-1)^2 = 534,773,760 < 2^31 up to here
PATA_KNN_MAX = 64   # neighbours per query


def _check_pata_scores(scores, clip_lo, clip_hi):
    _check(scores, "scores")
    if scores.dim() != 2:
        raise ValueError("scores must be [K, M], got %s"
                         % (tuple(scores.shape),))
    K, M = scores.shape
    if K < 2 or K > PATA_K_MAX:
        raise ValueError("K must be in [2, %d], got %d" % (PATA_K_MAX, K))
    if M < 1:
        raise ValueError("scores has no columns")
    clip_lo, clip_hi = float(clip_lo), float(clip_hi)
    if not clip_lo <= clip_hi:  # also refuses a NaN bound
        raise ValueError("clip_lo must be <= clip_hi, got %r, %r"
                         % (clip_lo, clip_hi))
    return K, M, clip_lo, clip_hi


def _launch_pata_codes(ops, scores, K, M, clip_lo, clip_hi):
    Kpad = (K + 7) // 8 * 8
    codes = torch.empty(M, Kpad, dtype=torch.int16, device=scores.device)
    ops.pata_ec_codes(scores.data_ptr(), K, M, Kpad, clip_lo, clip_hi,
                      codes.data_ptr(), _stream())
    return codes


def pata_ec_codes(scores, clip_lo, clip_hi):
    """PATA-EC rank codes of every environment.

    ``scores[K][M]`` (row = agent, column = environment, as
    ``es_eval_matrix`` returns it) becomes int16 ``codes[M][Kpad]``,
    environment-major, ``Kpad`` = K rounded up to 8 with the pad entries
    0.  Column m is clipped to ``[clip_lo, clip_hi]`` (NaN counts as
    ``clip_lo``) and ``code[i] = 2 #{j: c_j < c_i} + #{j: c_j == c_i} - 1``,
    twice the mid-rank: tied scores, which clipping makes common, share a
    code.

    TypeError for dtype, device or contiguity, ValueError for shape,
    ``K`` outside ``[2, 512]`` or ``clip_lo > clip_hi``, all before the
    launch."""
    ops = _require_ops()
    K, M, clip_lo, clip_hi = _check_pata_scores(scores, clip_lo, clip_hi)
    with torch.cuda.device(scores.device):
        return _launch_pata_codes(ops, scores, K, M, clip_lo, clip_hi)


def env_novelty(scores, n_ref, k, clip_lo, clip_hi, return_neighbours=False):
    """PATA-EC novelty of the environments in columns ``[n_ref, M)`` of
    ``scores[K][M]`` against the reference environments in columns
    ``[0, n_ref)``.

    With the codes of ``pata_ec_codes``, ``D2(q, r)`` is the exact int32
    squared Euclidean distance between two code rows, ``knn_d2[Q][k']``
    the ``k' = min(k, n_ref)`` smallest of a query in ascending order, and
    ``novelty[q] = sum_j sqrt(knn_d2[q][j]) / (k' * 2 * (K - 1))``, the
    mean Euclidean distance to the k' nearest rank vectors with the ranks
    scaled to [0, 1], summed in a fixed order (two calls give the same
    bits).  Returns ``novelty[Q]`` (fp32),
    or ``(novelty, knn_d2)``.

    Validation as in ``pata_ec_codes``, plus ValueError unless
    ``1 <= k <= 64``, ``n_ref >= 1`` and ``Q = M - n_ref >= 1``."""
    ops = _require_ops()
    K, M, clip_lo, clip_hi = _check_pata_scores(scores, clip_lo, clip_hi)
    n_ref, k = int(n_ref), int(k)
    if k < 1 or k > PATA_KNN_MAX:
        raise ValueError("k must be in [1, %d], got %d" % (PATA_KNN_MAX, k))
    if n_ref < 1:
        raise ValueError("n_ref must be >= 1, got %d" % n_ref)
    Q = M - n_ref
    if Q < 1:
        raise ValueError("no query columns: M = %d, n_ref = %d" % (M, n_ref))
    k_eff = min(k, n_ref)
    device = scores.device
    with torch.cuda.device(device):
        codes = _launch_pata_codes(ops, scores, K, M, clip_lo, clip_hi)
        knn_d2 = torch.empty(Q, k_eff, dtype=torch.int32, device=device)
        novelty = torch.empty(Q, dtype=torch.float32, device=device)
        ops.pata_ec_knn(codes.data_ptr(), codes.shape[1], K, n_ref, Q, k_eff,
                        knn_d2.data_ptr(), novelty.data_ptr(), _stream())
    if return_neighbours:
        return novelty, knn_d2
    return novelty


# ---------------------------------------------------------------------------
# Novelty search (ns_kernels.hip): the rollout kernels with a behaviour
# characterisation (BC) per member or cell, and k-nearest-neighbour novelty
# of BCs against an archive.  The BC is the mean over the 64 episodes of the
# final state s_H, 4 floats.
# ---------------------------------------------------------------------------

BC_DIM = OBS_DIM
BC_KNN_MAX = _OPS.BC_KNN_MAX if _OPS else 16     # neighbours per query
BC_KNN_TILE = _OPS.BC_KNN_TILE if _OPS else 1024  # archive rows per LDS tile


def es_rollout_mlp_bc(theta, sigma, seed, iteration, horizon, member_offset,
                      pop_shard, obs_mu, obs_nu, env_A, env_B,
                      return_final_states=False):
    """``es_rollout_mlp`` that also reports each member's behaviour
    characterisation: ``bc[pop_shard][4]``, the mean over the member's 64
    episodes of the final state ``s_horizon``, summed in a fixed order.

    Returns ``(fitness, obs_stat, bc)``, or ``(fitness, obs_stat, bc,
    final_states[pop_shard][64][4])``.  ``fitness`` and ``obs_stat`` are
    bit-identical to ``es_rollout_mlp`` for the same arguments.

    Every argument is validated before anything is launched: TypeError for
    dtype, device or contiguity, ValueError for shape, horizon or
    ``pop_shard``."""
    ops = _require_ops()
    named = (("theta", theta), ("obs_mu", obs_mu), ("obs_nu", obs_nu),
             ("env_A", env_A), ("env_B", env_B))
    for name, t in named:
        _check(t, name)
        if t.device != theta.device:
            raise TypeError("%s is on %s, theta on %s"
                            % (name, t.device, theta.device))
    for name, t, want in (("theta", theta, (NPARAMS,)),
                          ("obs_mu", obs_mu, (OBS_DIM,)),
                          ("obs_nu", obs_nu, (OBS_DIM,)),
                          ("env_A", env_A, (OBS_DIM, OBS_DIM)),
                          ("env_B", env_B, (OBS_DIM,))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    horizon, pop_shard = int(horizon), int(pop_shard)
    member_offset = int(member_offset)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if pop_shard < 1:
        raise ValueError("pop_shard must be >= 1, got %d" % pop_shard)
    if member_offset < 0 or member_offset + pop_shard >= 2 ** 31:
        raise ValueError("member_offset %d with pop_shard %d leaves the "
                         "int32 member range" % (member_offset, pop_shard))
    device = theta.device
    fitness = torch.empty(pop_shard, dtype=torch.float32, device=device)
    obs_stat = torch.zeros(2 * OBS_DIM + 1, dtype=torch.float32,
                           device=device)
    bc = torch.empty(pop_shard, BC_DIM, dtype=torch.float32, device=device)
    final = None
    if return_final_states:
        final = torch.empty(pop_shard, ENVS_PER_MEMBER, OBS_DIM,
                            dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        part = _partial_buffer(device, pop_shard * 2 * OBS_DIM)
        ops.es_rollout_mlp_bc(
            theta.data_ptr(), float(sigma), int(seed) & 0xFFFFFFFF,
            int(iteration) & 0xFFFFFFFF, horizon, member_offset, pop_shard,
            obs_mu.data_ptr(), obs_nu.data_ptr(), env_A.data_ptr(),
            env_B.data_ptr(), fitness.data_ptr(), part.data_ptr(),
            obs_stat.data_ptr(), bc.data_ptr(),
            final.data_ptr() if return_final_states else 0, _stream())
    if return_final_states:
        return fitness, obs_stat, bc, final
    return fitness, obs_stat, bc


def es_eval_bc(thetas, obs_mu, obs_nu, env_A, env_B, seed, iteration,
               horizon, return_final_states=False, return_episodes=False):
    """``es_eval_matrix`` that also reports the behaviour characterisation
    of every (policy, environment) cell: ``bc[K][M][4]``, the mean over the
    cell's 64 episodes of the final state ``s_horizon``.

    Arguments as ``es_eval_matrix``.  Returns ``(scores[K][M], bc)``,
    followed by ``final_states[K][M][64][4]`` and ``episodes[K][M][64]`` if
    asked for, in that order.  ``scores`` and ``episodes`` are bit-identical
    to ``es_eval_matrix``; ``bc[k][m]`` is bit-identical to the ``bc`` that
    ``es_rollout_mlp_bc`` gives for ``thetas[k]`` at ``sigma=0``.

    Every argument is validated before anything is launched: TypeError for
    dtype, device or contiguity, ValueError for shape or horizon."""
    ops = _require_ops()
    named = (("thetas", thetas), ("obs_mu", obs_mu), ("obs_nu", obs_nu),
             ("env_A", env_A), ("env_B", env_B))
    for name, t in named:
        _check(t, name)
        if t.device != thetas.device:
            raise TypeError("%s is on %s, thetas on %s"
                            % (name, t.device, thetas.device))
    if thetas.dim() != 2 or thetas.shape[1] != NPARAMS:
        raise ValueError("thetas must be [K, %d], got %s"
                         % (NPARAMS, tuple(thetas.shape)))
    K = thetas.shape[0]
    if env_A.dim() != 3 or tuple(env_A.shape[1:]) != (OBS_DIM, OBS_DIM):
        raise ValueError("env_A must be [M, %d, %d], got %s"
                         % (OBS_DIM, OBS_DIM, tuple(env_A.shape)))
    M = env_A.shape[0]
    if K < 1 or M < 1:
        raise ValueError("need at least one policy and one environment, "
                         "got K = %d, M = %d" % (K, M))
    for name, t, want in (("obs_mu", obs_mu, (K, OBS_DIM)),
                          ("obs_nu", obs_nu, (K, OBS_DIM)),
                          ("env_B", env_B, (M, OBS_DIM))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if K * M >= 2 ** 31:
        raise ValueError("K*M = %d exceeds the launch grid" % (K * M))
    device = thetas.device
    scores = torch.empty(K, M, dtype=torch.float32, device=device)
    bc = torch.empty(K, M, BC_DIM, dtype=torch.float32, device=device)
    final = episodes = None
    if return_final_states:
        final = torch.empty(K, M, ENVS_PER_MEMBER, OBS_DIM,
                            dtype=torch.float32, device=device)
    if return_episodes:
        episodes = torch.empty(K, M, ENVS_PER_MEMBER, dtype=torch.float32,
                               device=device)
    with torch.cuda.device(device):
        ops.es_eval_bc(
            thetas.data_ptr(), obs_mu.data_ptr(), obs_nu.data_ptr(),
            env_A.data_ptr(), env_B.data_ptr(), int(seed) & 0xFFFFFFFF,
            int(iteration) & 0xFFFFFFFF, horizon, K, M, scores.data_ptr(),
            episodes.data_ptr() if return_episodes else 0, bc.data_ptr(),
            final.data_ptr() if return_final_states else 0, _stream())
    out = (scores, bc)
    if return_final_states:
        out += (final,)
    if return_episodes:
        out += (episodes,)
    return out


def bc_knn_novelty(bc, archive, k, return_neighbours=False, out=None,
                   out_neighbours=None):
    """Novelty of the behaviour characterisations ``bc[N][4]`` against
    ``archive[R][4]``: ``novelty[q]`` is the mean Euclidean distance from
    ``bc[q]`` to its ``k`` nearest archive rows, ``1 <= k <= min(R, 16)``.
    Duplicate archive rows count as separate neighbours.  Returns
    ``novelty[N]``, or ``(novelty, knn_d2[N][k])`` with the ``k`` smallest
    squared distances in ascending order.

    ``out`` / ``out_neighbours`` are written instead of fresh tensors when
    given: fp32, contiguous, on the device of ``bc``, with at least N
    (N * k) elements, of which only the first N (N * k) are touched.

    All values must be finite: with a NaN or an infinity in ``bc`` or
    ``archive`` the novelty is unspecified.

    Everything is validated before the launch: TypeError for dtype, device
    or contiguity, ValueError for shape, an empty ``bc`` or ``archive``
    (``R == 0``) and ``k`` outside ``[1, min(R, 16)]``."""
    ops = _require_ops()
    named = [("bc", bc), ("archive", archive)]
    if out is not None:
        named.append(("out", out))
    if out_neighbours is not None:
        named.append(("out_neighbours", out_neighbours))
    for name, t in named:
        _check(t, name)
        if t.device != bc.device:
            raise TypeError("%s is on %s, bc on %s"
                            % (name, t.device, bc.device))
    for name, t in (("bc", bc), ("archive", archive)):
        if t.dim() != 2 or t.shape[1] != BC_DIM:
            raise ValueError("%s must be [*, %d], got %s"
                             % (name, BC_DIM, tuple(t.shape)))
    N, R, k = bc.shape[0], archive.shape[0], int(k)
    if N < 1:
        raise ValueError("bc has no rows")
    if R < 1:
        raise ValueError("the archive is empty (R == 0)")
    if k < 1 or k > BC_KNN_MAX:
        raise ValueError("k must be in [1, %d], got %d" % (BC_KNN_MAX, k))
    if k > R:
        raise ValueError("k = %d exceeds the %d archive rows" % (k, R))
    if N * k >= 2 ** 31:
        raise ValueError("N*k = %d exceeds the launch limits" % (N * k))
    if out is not None and out.numel() < N:
        raise ValueError("out holds %d elements, need %d" % (out.numel(), N))
    if out_neighbours is not None and out_neighbours.numel() < N * k:
        raise ValueError("out_neighbours holds %d elements, need %d"
                         % (out_neighbours.numel(), N * k))
    device = bc.device
    want_nb = return_neighbours or out_neighbours is not None
    novelty = out if out is not None else torch.empty(
        N, dtype=torch.float32, device=device)
    knn_d2 = out_neighbours
    if want_nb and knn_d2 is None:
        knn_d2 = torch.empty(N, k, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        ops.bc_knn_novelty(bc.data_ptr(), N, archive.data_ptr(), R, k,
                           novelty.data_ptr(),
                           knn_d2.data_ptr() if want_nb else 0, _stream())
    if want_nb:
        return novelty, knn_d2
    return novelty


# ---------------------------------------------------------------------------
# Separable NES (snes_kernels.hip): the rollout with a step size per
# parameter, and the gradient with the second-moment row that adapts it.
# ---------------------------------------------------------------------------


def es_rollout_mlp_sigma(theta, sigma_vec, seed, iteration, horizon,
                         member_offset, pop_shard, obs_mu, obs_nu, env_A,
                         env_B):
    """``es_rollout_mlp`` with a step size per parameter: member ``m``
    evaluates ``theta[j] + s_j * z[j]`` with ``s_j = sigma_vec[j]`` for even
    ``m`` and ``-sigma_vec[j]`` for odd ``m``, ``z`` the draws of pair
    ``m // 2``.  Returns ``(fitness[pop_shard], obs_stat[9])``; for
    ``sigma_vec = full(s)`` both are bit-identical to ``es_rollout_mlp`` at
    ``sigma = s``.

    ``sigma_vec`` is fp32 ``[NPARAMS]`` on the device of ``theta``.  Its
    values must be finite and >= 0; this is not checked on the device, and a
    NaN, an infinity or a negative entry gives an unspecified policy.

    Every argument is validated before anything is launched: TypeError for
    dtype, device or contiguity, ValueError for shape, ``horizon < 1``,
    ``pop_shard < 1`` or a member range that leaves int32."""
    ops = _require_ops()
    if not torch.is_tensor(sigma_vec):
        raise TypeError("sigma_vec must be a tensor [%d], got %s (for a "
                        "scalar sigma use es_rollout_mlp)"
                        % (NPARAMS, type(sigma_vec).__name__))
    named = (("theta", theta), ("sigma_vec", sigma_vec), ("obs_mu", obs_mu),
             ("obs_nu", obs_nu), ("env_A", env_A), ("env_B", env_B))
    for name, t in named:
        _check(t, name)
        if t.device != theta.device:
            raise TypeError("%s is on %s, theta on %s"
                            % (name, t.device, theta.device))
    for name, t, want in (("theta", theta, (NPARAMS,)),
                          ("sigma_vec", sigma_vec, (NPARAMS,)),
                          ("obs_mu", obs_mu, (OBS_DIM,)),
                          ("obs_nu", obs_nu, (OBS_DIM,)),
                          ("env_A", env_A, (OBS_DIM, OBS_DIM)),
                          ("env_B", env_B, (OBS_DIM,))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    horizon, pop_shard = int(horizon), int(pop_shard)
    member_offset = int(member_offset)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if pop_shard < 1:
        raise ValueError("pop_shard must be >= 1, got %d" % pop_shard)
    if member_offset < 0 or member_offset + pop_shard >= 2 ** 31:
        raise ValueError("member_offset %d with pop_shard %d leaves the "
                         "int32 member range" % (member_offset, pop_shard))
    device = theta.device
    fitness = torch.empty(pop_shard, dtype=torch.float32, device=device)
    obs_stat = torch.zeros(2 * OBS_DIM + 1, dtype=torch.float32,
                           device=device)
    with torch.cuda.device(device):
        part = _partial_buffer(device, pop_shard * 2 * OBS_DIM)
        ops.es_rollout_mlp_sigma(
            theta.data_ptr(), sigma_vec.data_ptr(), int(seed) & 0xFFFFFFFF,
            int(iteration) & 0xFFFFFFFF, horizon, member_offset, pop_shard,
            obs_mu.data_ptr(), obs_nu.data_ptr(), env_A.data_ptr(),
            env_B.data_ptr(), fitness.data_ptr(), part.data_ptr(),
            obs_stat.data_ptr(), _stream())
    return fitness, obs_stat


def es_grad_sigma(wdiff, wsum, pair_begin, pair_end, seed, iteration, device,
                  nparams=None):
    """Both rows of the separable-NES gradient over the pairs ``pair_begin
    <= k < pair_end``, from one regeneration of each draw ``z_k``:

      ``g_mu[j]  = sum_k wdiff[k] * z_k[j]``
      ``g_sig[j] = sum_k wsum[k] * (z_k[j]**2 - 1)``

    ``wdiff`` and ``wsum`` are fp32 vectors of equal length, indexed by the
    pair number like ``es_grad``'s ``wpair``; nothing outside the range is
    read.  Returns ``(g_mu, g_sig)``, the two rows of one ``[2, nparams]``
    tensor.  ``g_mu`` is bit-identical to ``es_grad(wdiff, ...)``; both rows
    are sums in a fixed order, so two calls give the same bits.

    Everything is validated before the launch: TypeError for dtype, device
    or contiguity, ValueError for shape, a bad pair range, ``nparams < 1``,
    and ``wdiff`` / ``wsum`` of different length or shorter than
    ``pair_end``."""
    ops = _require_ops()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise TypeError("device must be a CUDA (ROCm) device, got %s" % dev)
    for name, t in (("wdiff", wdiff), ("wsum", wsum)):
        _check(t, name)
        if t.device != wdiff.device or (dev.index is not None
                                        and t.device != dev):
            raise TypeError("%s is on %s, expected %s"
                            % (name, t.device, device))
    if nparams is None:
        nparams = NPARAMS
    nparams = int(nparams)
    pair_begin, pair_end = int(pair_begin), int(pair_end)
    for name, t in (("wdiff", wdiff), ("wsum", wsum)):
        if t.dim() != 1:
            raise ValueError("%s must be 1-d, got %s"
                             % (name, tuple(t.shape)))
    if wdiff.numel() != wsum.numel():
        raise ValueError("wdiff holds %d weights, wsum %d"
                         % (wdiff.numel(), wsum.numel()))
    if pair_begin < 0 or pair_end < pair_begin or pair_end >= 2 ** 30:
        raise ValueError("bad pair range [%d, %d)" % (pair_begin, pair_end))
    if wdiff.numel() < pair_end:
        raise ValueError("the weights hold %d pairs, pair_end is %d"
                         % (wdiff.numel(), pair_end))
    if nparams < 1 or nparams >= 2 ** 30:
        raise ValueError("nparams must be in [1, 2**30), got %d" % nparams)
    device = wdiff.device
    grad = torch.zeros(2, nparams, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        chunks = ops.es_grad_chunks(pair_end - pair_begin, nparams)
        part = _partial_buffer(device, chunks * 2 * nparams)
        ops.es_grad_sigma(wdiff.data_ptr(), wsum.data_ptr(), pair_begin,
                          pair_end, int(seed) & 0xFFFFFFFF,
                          int(iteration) & 0xFFFFFFFF, nparams,
                          part.data_ptr(), grad.data_ptr(), _stream())
    return grad[0], grad[1]


# ---------------------------------------------------------------------------
# Deep GA (ga_kernels.hip): a population of mutated copies of T parents,
# truncation selection with an exact tie order, and weights rebuilt from
# chains of mutation seeds.  The mutation of child slot i in generation g is
# the draw es_rollout_mlp uses for pair i at iteration g.
# ---------------------------------------------------------------------------

GA_TRUNCATE_MAX = _OPS.GA_TRUNCATE_MAX if _OPS else 65536  # members ranked
GA_ROWS_MAX = _OPS.GA_ROWS_MAX if _OPS else 65535  # rows that ride grid.y


def _check_ga_on(named, anchor_name, anchor):
    """dtype / device / contiguity of every (name, tensor, dtype), all on
    the device of ``anchor``."""
    for name, t, dtype in named:
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s"
                            % (name, type(t).__name__))
        _check(t, name, dtype=dtype)
        if t.device != anchor.device:
            raise TypeError("%s is on %s, %s on %s"
                            % (name, t.device, anchor_name, anchor.device))


def _check_ga_sigma(sigma):
    sigma = float(sigma)
    if not 0.0 <= sigma < float("inf"):  # also refuses a NaN
        raise ValueError("sigma must be finite and >= 0, got %r" % sigma)
    return sigma


def ga_parents(seed, generation, pop, n_elite, T_cur, device):
    """Who mutates whom in one generation: int32 ``(parent_idx[pop],
    slot[pop])``.  Member ``m < n_elite`` is survivor ``m`` unmutated
    (``parent_idx = m``, ``slot = -1``); member ``m >= n_elite`` has ``slot
    = m`` and ``parent_idx = (u * T_cur) >> 32`` with ``u`` the first word
    of one Philox draw keyed by ``(seed, generation, m)``.  Integer
    arithmetic only: ``ga_oracle.parents_exact`` reproduces it exactly.

    TypeError for a device that is not a GPU; ValueError unless ``1 <= pop <
    2**31``, ``1 <= T_cur < 2**31`` and ``0 <= n_elite <= min(T_cur,
    pop)``."""
    ops = _require_ops()
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError("device must be a CUDA (ROCm) device, got %s"
                        % device)
    pop, n_elite, T_cur = int(pop), int(n_elite), int(T_cur)
    if pop < 1 or pop >= 2 ** 31:
        raise ValueError("pop must be in [1, 2**31), got %d" % pop)
    if T_cur < 1 or T_cur >= 2 ** 31:
        raise ValueError("T_cur must be in [1, 2**31), got %d" % T_cur)
    if n_elite < 0 or n_elite > T_cur or n_elite > pop:
        raise ValueError("n_elite must be in [0, min(T_cur, pop)] = [0, %d], "
                         "got %d" % (min(T_cur, pop), n_elite))
    parent_idx = torch.empty(pop, dtype=torch.int32, device=device)
    slot = torch.empty(pop, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        ops.ga_parents(int(seed) & 0xFFFFFFFF, int(generation) & 0xFFFFFFFF,
                       pop, n_elite, T_cur, parent_idx.data_ptr(),
                       slot.data_ptr(), _stream())
    return parent_idx, slot


def ga_rollout_mlp(parents, parent_idx, slot, sigma, seed, generation,
                   horizon, obs_mu, obs_nu, env_A, env_B):
    """Roll out a population in which member ``m`` is row ``parent_idx[m]``
    of ``parents[T][NPARAMS]``, as it is for ``slot[m] < 0`` and otherwise
    mutated: ``parent[j] + sigma * z[j]`` in one fma, ``z`` the draw of
    child slot ``slot[m]`` in this generation.  Returns ``(fitness[pop],
    obs_stat[9])`` like ``es_rollout_mlp``.  A mutated member carries the
    bits of that kernel's member ``2 * slot`` for the same parent, an
    unmutated one those of ``es_eval_matrix`` for its row.

    The caller's contract, which cannot be checked without a host sync:
    every ``parent_idx[m]`` lies in ``[0, T)`` (another value reads outside
    ``parents``) and every ``slot[m]`` is below ``2**31``.  ``ga_parents``
    writes such values.

    Everything else is validated before anything is launched: TypeError for
    dtype, device or contiguity, ValueError for shapes, ``horizon < 1`` or a
    sigma that is negative or not finite."""
    ops = _require_ops()
    _check_ga_on(
        (("parents", parents, torch.float32),
         ("parent_idx", parent_idx, torch.int32),
         ("slot", slot, torch.int32), ("obs_mu", obs_mu, torch.float32),
         ("obs_nu", obs_nu, torch.float32), ("env_A", env_A, torch.float32),
         ("env_B", env_B, torch.float32)), "parents", parents)
    if parents.dim() != 2 or parents.shape[1] != NPARAMS \
            or parents.shape[0] < 1:
        raise ValueError("parents must be [T, %d] with T >= 1, got %s"
                         % (NPARAMS, tuple(parents.shape)))
    if parent_idx.dim() != 1 or parent_idx.numel() < 1:
        raise ValueError("parent_idx must be [pop] with pop >= 1, got %s"
                         % (tuple(parent_idx.shape),))
    pop = parent_idx.numel()
    for name, t, want in (("slot", slot, (pop,)),
                          ("obs_mu", obs_mu, (OBS_DIM,)),
                          ("obs_nu", obs_nu, (OBS_DIM,)),
                          ("env_A", env_A, (OBS_DIM, OBS_DIM)),
                          ("env_B", env_B, (OBS_DIM,))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if pop >= 2 ** 31:
        raise ValueError("pop = %d exceeds the launch grid" % pop)
    sigma = _check_ga_sigma(sigma)
    device = parents.device
    fitness = torch.empty(pop, dtype=torch.float32, device=device)
    obs_stat = torch.zeros(2 * OBS_DIM + 1, dtype=torch.float32,
                           device=device)
    with torch.cuda.device(device):
        part = _partial_buffer(device, pop * 2 * OBS_DIM)
        ops.ga_rollout_mlp(
            parents.data_ptr(), parent_idx.data_ptr(), slot.data_ptr(),
            sigma, int(seed) & 0xFFFFFFFF, int(generation) & 0xFFFFFFFF,
            horizon, pop, obs_mu.data_ptr(), obs_nu.data_ptr(),
            env_A.data_ptr(), env_B.data_ptr(), fitness.data_ptr(),
            part.data_ptr(), obs_stat.data_ptr(), _stream())
    return fitness, obs_stat


def ga_truncate(fitness, T):
    """Truncation selection: int32 ``order[T]``, ``order[r]`` the index of
    the member of descending rank ``r``, where ``rank(i) = #{j : f[j] > f[i]
    or (f[j] == f[i] and j < i)}``.  A NaN ranks below every number, NaNs
    among themselves by index, and ``-0 == +0``.  Exact: comparisons only.

    TypeError for dtype, device or contiguity; ValueError unless ``fitness``
    is 1-d with ``2 <= n <= 65536`` and ``1 <= T <= n``."""
    ops = _require_ops()
    _check_ga_on((("fitness", fitness, torch.float32),), "fitness", fitness)
    if fitness.dim() != 1:
        raise ValueError("fitness must be 1-d, got %s"
                         % (tuple(fitness.shape),))
    n, T = fitness.numel(), int(T)
    if n < 2 or n > GA_TRUNCATE_MAX:
        raise ValueError("n must be in [2, %d], got %d"
                         % (GA_TRUNCATE_MAX, n))
    if T < 1 or T > n:
        raise ValueError("T must be in [1, n] = [1, %d], got %d" % (n, T))
    order = torch.empty(T, dtype=torch.int32, device=fitness.device)
    with torch.cuda.device(fitness.device):
        ops.ga_truncate(fitness.data_ptr(), n, T, order.data_ptr(),
                        _stream())
    return order


def ga_survivors(parents, parent_idx, slot, order, sigma, seed, generation,
                 out=None):
    """The weights the survivors were evaluated with: row ``t`` of
    ``new_parents[T][NPARAMS]`` is member ``order[t]`` of the launch that
    ``ga_rollout_mlp`` made from the same ``(parents, parent_idx, slot,
    sigma, seed, generation)``, its parent row as it is for ``slot < 0`` and
    the same multiply-add otherwise.  Out of place: ``out``, if given, is
    fp32 ``[T][NPARAMS]`` storage that shares no memory with ``parents``.

    The caller's contract: ``order`` values in ``[0, pop)``, ``parent_idx``
    values in ``[0, T_cur)``, as ``ga_truncate`` and ``ga_parents`` write
    them.  TypeError for dtype, device or contiguity, ValueError for shapes,
    ``T`` outside ``[1, 65535]``, an ``out`` that overlaps ``parents`` or a
    bad sigma."""
    ops = _require_ops()
    named = [("parents", parents, torch.float32),
             ("parent_idx", parent_idx, torch.int32),
             ("slot", slot, torch.int32), ("order", order, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.float32))
    _check_ga_on(named, "parents", parents)
    if parents.dim() != 2 or parents.shape[1] != NPARAMS \
            or parents.shape[0] < 1:
        raise ValueError("parents must be [T_cur, %d] with T_cur >= 1, got %s"
                         % (NPARAMS, tuple(parents.shape)))
    if parent_idx.dim() != 1 or parent_idx.numel() < 1:
        raise ValueError("parent_idx must be [pop] with pop >= 1, got %s"
                         % (tuple(parent_idx.shape),))
    pop = parent_idx.numel()
    if tuple(slot.shape) != (pop,):
        raise ValueError("slot must be [%d], got %s"
                         % (pop, tuple(slot.shape)))
    if order.dim() != 1:
        raise ValueError("order must be 1-d, got %s" % (tuple(order.shape),))
    T = order.numel()
    if T < 1 or T > GA_ROWS_MAX or T > pop:
        raise ValueError("T must be in [1, min(pop, %d)], got %d"
                         % (GA_ROWS_MAX, T))
    sigma = _check_ga_sigma(sigma)
    device = parents.device
    if out is None:
        out = torch.empty(T, NPARAMS, dtype=torch.float32, device=device)
    else:
        if tuple(out.shape) != (T, NPARAMS):
            raise ValueError("out must be [%d, %d], got %s"
                             % (T, NPARAMS, tuple(out.shape)))
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
        plo = parents.data_ptr()
        phi = plo + parents.numel() * 4
        if lo < phi and plo < hi:
            raise ValueError("out overlaps parents: ga_survivors is out of "
                             "place")
    with torch.cuda.device(device):
        ops.ga_survivors(parents.data_ptr(), parent_idx.data_ptr(),
                         slot.data_ptr(), order.data_ptr(), T, sigma,
                         int(seed) & 0xFFFFFFFF,
                         int(generation) & 0xFFFFFFFF, out.data_ptr(),
                         _stream())
    return out


def ga_decode(theta0, lineage, sigma, seed, out=None):
    """Weights from seed chains.  ``lineage`` is int32 ``[N][G]``: column
    ``c`` of a row holds the child slot whose draw was applied in generation
    ``c``, or a negative value for a generation the genome passed through
    unmutated.  ``thetas[n] = theta0``, then for ``c = 0 .. G-1`` in order
    ``acc = fma(sigma, z(seed, c, lineage[n][c]), acc)``: the fold
    ``ga_survivors`` performs generation by generation, so the result
    carries the bits of the parents it materialised.  ``G = 0`` gives copies
    of ``theta0``.  ``out``, if given, is fp32 ``[N][NPARAMS]``.

    TypeError for dtype, device or contiguity, ValueError for shapes, ``N``
    outside ``[1, 65535]`` or a bad sigma."""
    ops = _require_ops()
    named = [("theta0", theta0, torch.float32),
             ("lineage", lineage, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.float32))
    _check_ga_on(named, "theta0", theta0)
    if tuple(theta0.shape) != (NPARAMS,):
        raise ValueError("theta0 must be [%d], got %s"
                         % (NPARAMS, tuple(theta0.shape)))
    if lineage.dim() != 2:
        raise ValueError("lineage must be [N, G], got %s"
                         % (tuple(lineage.shape),))
    N, G = lineage.shape
    if N < 1 or N > GA_ROWS_MAX:
        raise ValueError("N must be in [1, %d], got %d" % (GA_ROWS_MAX, N))
    sigma = _check_ga_sigma(sigma)
    device = theta0.device
    if out is None:
        out = torch.empty(N, NPARAMS, dtype=torch.float32, device=device)
    elif tuple(out.shape) != (N, NPARAMS):
        raise ValueError("out must be [%d, %d], got %s"
                         % (N, NPARAMS, tuple(out.shape)))
    with torch.cuda.device(device):
        ops.ga_decode(theta0.data_ptr(), lineage.data_ptr(), N, G, sigma,
                      int(seed) & 0xFFFFFFFF, out.data_ptr(), _stream())
    return out


# ---------------------------------------------------------------------------
# Safe mutations (sm_kernels.hip): per-parent, per-parameter mutation steps
# from the sensitivity of the logits on a probe batch, and the GA rollout /
# survivors kernels that take such a step row per parent instead of one
# scalar sigma.
# ---------------------------------------------------------------------------

SM_MODES = ("abs", "sum")
SM_PROBE_ROWS = ENVS_PER_MEMBER


def _check_sm_mode(mode):
    if mode not in SM_MODES:
        raise ValueError("mode must be one of %r, got %r" % (SM_MODES, mode))
    return SM_MODES.index(mode)


def _check_sm_floor(s_min):
    s_min = float(s_min)
    if not 0.0 < s_min < float("inf"):  # also refuses a NaN
        raise ValueError("s_min must be finite and > 0, got %r" % s_min)
    return s_min


def _check_overlap(out, other, other_name, op):
    lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
    plo = other.data_ptr()
    phi = plo + other.numel() * 4
    if lo < phi and plo < hi:
        raise ValueError("out overlaps %s: %s is out of place"
                         % (other_name, op))


def sm_steps(thetas, probe, sigma, s_min=0.01, mode="abs", out=None,
             return_sens=False):
    """Safe-mutation steps of ``thetas[T][NPARAMS]`` on ``probe[64][4]``
    (normalised observations): ``steps[t][j] = sigma / max(sens[t][j],
    s_min)`` with ``sens = sqrt(m_0^2 + m_1^2)`` and ``m_k[j]`` the mean
    over the probe rows of ``|d logit_k / d theta_j|`` (``mode="abs"``) or
    of the signed derivative (``mode="sum"``).  One workgroup per row; row
    ``t`` of the result depends on row ``t`` of ``thetas`` only.  Returns
    ``steps``, or ``(steps, sens)`` with ``return_sens``.  ``out``, if
    given, is fp32 ``[T][NPARAMS]`` storage for ``steps``.  ``T = 0`` gives
    empty results.

    TypeError for dtype, device or contiguity, ValueError for shapes, ``T >
    65535``, a sigma that is negative or not finite, an ``s_min`` that is
    not finite and positive, or an unknown mode."""
    ops = _require_ops()
    # the scalars first: they need no tensor to be judged
    sigma = _check_ga_sigma(sigma)
    s_min = _check_sm_floor(s_min)
    mode_id = _check_sm_mode(mode)
    named = [("thetas", thetas, torch.float32),
             ("probe", probe, torch.float32)]
    if out is not None:
        named.append(("out", out, torch.float32))
    _check_ga_on(named, "thetas", thetas)
    if thetas.dim() != 2 or thetas.shape[1] != NPARAMS:
        raise ValueError("thetas must be [T, %d], got %s"
                         % (NPARAMS, tuple(thetas.shape)))
    if tuple(probe.shape) != (SM_PROBE_ROWS, OBS_DIM):
        raise ValueError("probe must be [%d, %d], got %s"
                         % (SM_PROBE_ROWS, OBS_DIM, tuple(probe.shape)))
    T = thetas.shape[0]
    if T > GA_ROWS_MAX:
        raise ValueError("T must be <= %d, got %d" % (GA_ROWS_MAX, T))
    device = thetas.device
    if out is None:
        out = torch.empty(T, NPARAMS, dtype=torch.float32, device=device)
    else:
        if tuple(out.shape) != (T, NPARAMS):
            raise ValueError("out must be [%d, %d], got %s"
                             % (T, NPARAMS, tuple(out.shape)))
        _check_overlap(out, thetas, "thetas", "sm_steps")
    sens = (torch.empty(T, NPARAMS, dtype=torch.float32, device=device)
            if return_sens else None)
    if T > 0:
        with torch.cuda.device(device):
            ops.sm_steps(thetas.data_ptr(), probe.data_ptr(), T, sigma,
                         s_min, mode_id, out.data_ptr(),
                         sens.data_ptr() if return_sens else 0, _stream())
    return (out, sens) if return_sens else out


def _check_sm_steps_rows(steps, parents):
    if tuple(steps.shape) != tuple(parents.shape):
        raise ValueError("steps must have the shape of parents %s, got %s"
                         % (tuple(parents.shape), tuple(steps.shape)))


def ga_rollout_mlp_sm(parents, steps, parent_idx, slot, seed, generation,
                      horizon, obs_mu, obs_nu, env_A, env_B):
    """``ga_rollout_mlp`` with a step row per parent: a mutated member is
    ``parent[j] + steps[parent_idx[m]][j] * z[j]`` in one fma, ``z`` the
    draw of child slot ``slot[m]``; ``slot[m] < 0`` takes the row as it is.
    With every step equal to ``sigma`` the result carries the bits of
    ``ga_rollout_mlp``.  Returns ``(fitness[pop], obs_stat[9])``.

    The caller's contract and the validation are ``ga_rollout_mlp``'s;
    ``steps`` is fp32 with the shape of ``parents`` (``sm_steps`` writes
    it), finite where a member is mutated."""
    ops = _require_ops()
    _check_ga_on(
        (("parents", parents, torch.float32),
         ("steps", steps, torch.float32),
         ("parent_idx", parent_idx, torch.int32),
         ("slot", slot, torch.int32), ("obs_mu", obs_mu, torch.float32),
         ("obs_nu", obs_nu, torch.float32), ("env_A", env_A, torch.float32),
         ("env_B", env_B, torch.float32)), "parents", parents)
    if parents.dim() != 2 or parents.shape[1] != NPARAMS \
            or parents.shape[0] < 1:
        raise ValueError("parents must be [T, %d] with T >= 1, got %s"
                         % (NPARAMS, tuple(parents.shape)))
    _check_sm_steps_rows(steps, parents)
    if parent_idx.dim() != 1 or parent_idx.numel() < 1:
        raise ValueError("parent_idx must be [pop] with pop >= 1, got %s"
                         % (tuple(parent_idx.shape),))
    pop = parent_idx.numel()
    for name, t, want in (("slot", slot, (pop,)),
                          ("obs_mu", obs_mu, (OBS_DIM,)),
                          ("obs_nu", obs_nu, (OBS_DIM,)),
                          ("env_A", env_A, (OBS_DIM, OBS_DIM)),
                          ("env_B", env_B, (OBS_DIM,))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if pop >= 2 ** 31:
        raise ValueError("pop = %d exceeds the launch grid" % pop)
    device = parents.device
    fitness = torch.empty(pop, dtype=torch.float32, device=device)
    obs_stat = torch.zeros(2 * OBS_DIM + 1, dtype=torch.float32,
                           device=device)
    with torch.cuda.device(device):
        part = _partial_buffer(device, pop * 2 * OBS_DIM)
        ops.ga_rollout_mlp_sm(
            parents.data_ptr(), steps.data_ptr(), parent_idx.data_ptr(),
            slot.data_ptr(), int(seed) & 0xFFFFFFFF,
            int(generation) & 0xFFFFFFFF, horizon, pop, obs_mu.data_ptr(),
            obs_nu.data_ptr(), env_A.data_ptr(), env_B.data_ptr(),
            fitness.data_ptr(), part.data_ptr(), obs_stat.data_ptr(),
            _stream())
    return fitness, obs_stat


def ga_survivors_sm(parents, steps, parent_idx, slot, order, seed,
                    generation, out=None):
    """``ga_survivors`` with a step row per parent: row ``t`` of the result
    is the weights member ``order[t]`` of ``ga_rollout_mlp_sm``'s launch
    from the same arguments was evaluated with.  Out of place: ``out``, if
    given, is fp32 ``[T][NPARAMS]`` storage that shares no memory with
    ``parents`` or ``steps``.

    One generation ``c`` of a seed-chain decode over ``N`` rows is
    ``ga_survivors_sm(rows, sm_steps(rows), arange(N), lineage[:, c],
    arange(N), seed, c)``.

    Contract and validation are ``ga_survivors``'s; ``steps`` is fp32 with
    the shape of ``parents``."""
    ops = _require_ops()
    named = [("parents", parents, torch.float32),
             ("steps", steps, torch.float32),
             ("parent_idx", parent_idx, torch.int32),
             ("slot", slot, torch.int32), ("order", order, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.float32))
    _check_ga_on(named, "parents", parents)
    if parents.dim() != 2 or parents.shape[1] != NPARAMS \
            or parents.shape[0] < 1:
        raise ValueError("parents must be [T_cur, %d] with T_cur >= 1, got %s"
                         % (NPARAMS, tuple(parents.shape)))
    _check_sm_steps_rows(steps, parents)
    if parent_idx.dim() != 1 or parent_idx.numel() < 1:
        raise ValueError("parent_idx must be [pop] with pop >= 1, got %s"
                         % (tuple(parent_idx.shape),))
    pop = parent_idx.numel()
    if tuple(slot.shape) != (pop,):
        raise ValueError("slot must be [%d], got %s"
                         % (pop, tuple(slot.shape)))
    if order.dim() != 1:
        raise ValueError("order must be 1-d, got %s" % (tuple(order.shape),))
    T = order.numel()
    if T < 1 or T > GA_ROWS_MAX or T > pop:
        raise ValueError("T must be in [1, min(pop, %d)], got %d"
                         % (GA_ROWS_MAX, T))
    device = parents.device
    if out is None:
        out = torch.empty(T, NPARAMS, dtype=torch.float32, device=device)
    else:
        if tuple(out.shape) != (T, NPARAMS):
            raise ValueError("out must be [%d, %d], got %s"
                             % (T, NPARAMS, tuple(out.shape)))
        _check_overlap(out, parents, "parents", "ga_survivors_sm")
        _check_overlap(out, steps, "steps", "ga_survivors_sm")
    with torch.cuda.device(device):
        ops.ga_survivors_sm(parents.data_ptr(), steps.data_ptr(),
                            parent_idx.data_ptr(), slot.data_ptr(),
                            order.data_ptr(), T, int(seed) & 0xFFFFFFFF,
                            int(generation) & 0xFFFFFFFF, out.data_ptr(),
                            _stream())
    return out


# ---------------------------------------------------------------------------
# MAP-Elites ops (me_kernels.hip): parents drawn from the filled cells of a
# behaviour grid, the GA rollout with a behaviour characterisation, the
# per-cell competition and the compact list of filled cells.  The archive's
# weights are materialised by ga_survivors from the ``order`` that me_insert
# writes.
# ---------------------------------------------------------------------------

# cells of the grid: the archive's rows and the root row ride grid.y
ME_CELLS_MAX = _OPS.ME_CELLS_MAX if _OPS else GA_ROWS_MAX - 1


def _check_me_bins(bins):
    """The 4 bin counts as ints and their product C; ValueError unless every
    count is >= 1 and ``C <= ME_CELLS_MAX``."""
    try:
        bins = tuple(int(b) for b in bins)
    except TypeError:
        raise ValueError("bins must be 4 ints, got %r" % (bins,))
    if len(bins) != BC_DIM:
        raise ValueError("bins must be %d ints, got %r" % (BC_DIM, bins))
    C = 1
    for b in bins:
        if b < 1:
            raise ValueError("every bins entry must be >= 1, got %r"
                             % (bins,))
        C *= b
    if C + 1 > GA_ROWS_MAX:
        raise ValueError("bins %r give %d cells, more than %d"
                         % (bins, C, ME_CELLS_MAX))
    return bins, C


def me_grid(bins, lo, hi):
    """The grid description me_insert passes to the device: ``(bins, lo32,
    inv32, C)``, with ``lo32[d]`` the lower bound rounded to fp32 and
    ``inv32[d] = bins[d] / (hi[d] - lo[d])`` computed in double precision
    and then rounded to fp32, both returned as Python floats.

    ValueError unless there are 4 dimensions, every ``bins[d] >= 1``, the
    product ``C`` satisfies ``C + 1 <= GA_ROWS_MAX``, the bounds are finite
    with ``hi[d] > lo[d]``, and ``inv32[d]`` is finite and positive."""
    import numpy as np

    bins, C = _check_me_bins(bins)
    try:
        lo = tuple(float(x) for x in lo)
        hi = tuple(float(x) for x in hi)
    except TypeError:
        raise ValueError("lo and hi must be 4 floats each")
    if len(lo) != BC_DIM or len(hi) != BC_DIM:
        raise ValueError("lo and hi must be %d floats each, got %r and %r"
                         % (BC_DIM, lo, hi))
    lo32, inv32 = [], []
    for d in range(BC_DIM):
        if not (abs(lo[d]) < float("inf") and abs(hi[d]) < float("inf")):
            raise ValueError("the bounds of dimension %d are not finite: "
                             "[%r, %r]" % (d, lo[d], hi[d]))
        if not hi[d] > lo[d]:
            raise ValueError("need hi > lo in dimension %d, got [%r, %r]"
                             % (d, lo[d], hi[d]))
        with np.errstate(over="ignore"):
            l32 = float(np.float32(lo[d]))
            i32 = float(np.float32(np.float64(bins[d])
                                   / (np.float64(hi[d]) - np.float64(lo[d]))))
        if not (abs(l32) < float("inf") and 0.0 < i32 < float("inf")):
            raise ValueError("the bounds of dimension %d, [%r, %r], leave "
                             "the fp32 range" % (d, lo[d], hi[d]))
        lo32.append(l32)
        inv32.append(i32)
    return bins, tuple(lo32), tuple(inv32), C


def me_parents(seed, generation, pop, filled_idx, n_filled, root_row,
               out_parent_idx=None, out_slot=None):
    """Who mutates whom in one MAP-Elites generation: int32 ``(parent_idx[pop],
    slot[pop])``.  Member ``m`` has ``slot = m`` and mutates the elite of cell
    ``filled_idx[(u * n) >> 32]``, ``u`` the first word of one Philox draw
    keyed by ``(seed, generation, m)`` and ``n`` the value of the one-element
    int32 device tensor ``n_filled``, read on the device.  While ``n`` is 0
    every parent is ``root_row``.  Integer arithmetic only:
    ``map_elites_oracle.parents_exact`` reproduces it exactly.

    The caller's contract: ``0 <= n <= filled_idx.numel()``, as ``me_compact``
    writes it.  TypeError for dtype, device or contiguity; ValueError unless
    ``1 <= pop <= GA_TRUNCATE_MAX``, ``filled_idx`` is 1-d and not empty,
    ``n_filled`` has one element, ``0 <= root_row < 2**31`` and the outputs,
    if given, are ``[pop]``."""
    ops = _require_ops()
    named = [("filled_idx", filled_idx, torch.int32),
             ("n_filled", n_filled, torch.int32)]
    if out_parent_idx is not None:
        named.append(("out_parent_idx", out_parent_idx, torch.int32))
    if out_slot is not None:
        named.append(("out_slot", out_slot, torch.int32))
    _check_ga_on(named, "filled_idx", filled_idx)
    pop, root_row = int(pop), int(root_row)
    if pop < 1 or pop > GA_TRUNCATE_MAX:
        raise ValueError("pop must be in [1, %d], got %d"
                         % (GA_TRUNCATE_MAX, pop))
    if filled_idx.dim() != 1 or filled_idx.numel() < 1:
        raise ValueError("filled_idx must be [C] with C >= 1, got %s"
                         % (tuple(filled_idx.shape),))
    if n_filled.numel() != 1:
        raise ValueError("n_filled must hold one element, got %s"
                         % (tuple(n_filled.shape),))
    if root_row < 0 or root_row >= 2 ** 31:
        raise ValueError("root_row must be in [0, 2**31), got %d" % root_row)
    device = filled_idx.device
    for name, t in (("out_parent_idx", out_parent_idx),
                    ("out_slot", out_slot)):
        if t is not None and tuple(t.shape) != (pop,):
            raise ValueError("%s must be [%d], got %s"
                             % (name, pop, tuple(t.shape)))
    if out_parent_idx is None:
        out_parent_idx = torch.empty(pop, dtype=torch.int32, device=device)
    if out_slot is None:
        out_slot = torch.empty(pop, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        ops.me_parents(int(seed) & 0xFFFFFFFF, int(generation) & 0xFFFFFFFF,
                       pop, filled_idx.data_ptr(), n_filled.data_ptr(),
                       root_row, out_parent_idx.data_ptr(),
                       out_slot.data_ptr(), _stream())
    return out_parent_idx, out_slot


def ga_rollout_mlp_bc(parents, parent_idx, slot, sigma, seed, generation,
                      horizon, obs_mu, obs_nu, env_A, env_B,
                      return_final_states=False):
    """``ga_rollout_mlp`` that also reports each member's behaviour
    characterisation ``bc[pop][4]``, the mean over the member's 64 episodes
    of the final state, summed in a fixed order.

    Returns ``(fitness, obs_stat, bc)``, or ``(fitness, obs_stat, bc,
    final_states[pop][64][4])``.  ``fitness`` and ``obs_stat`` are
    bit-identical to ``ga_rollout_mlp`` for the same arguments; the BC of a
    mutated member is that of ``es_rollout_mlp_bc``'s member ``2 * slot`` for
    the same parent, the BC of an unmutated one that of ``es_eval_bc`` for
    its row.

    Contract and validation as ``ga_rollout_mlp``."""
    ops = _require_ops()
    _check_ga_on(
        (("parents", parents, torch.float32),
         ("parent_idx", parent_idx, torch.int32),
         ("slot", slot, torch.int32), ("obs_mu", obs_mu, torch.float32),
         ("obs_nu", obs_nu, torch.float32), ("env_A", env_A, torch.float32),
         ("env_B", env_B, torch.float32)), "parents", parents)
    if parents.dim() != 2 or parents.shape[1] != NPARAMS \
            or parents.shape[0] < 1:
        raise ValueError("parents must be [T, %d] with T >= 1, got %s"
                         % (NPARAMS, tuple(parents.shape)))
    if parent_idx.dim() != 1 or parent_idx.numel() < 1:
        raise ValueError("parent_idx must be [pop] with pop >= 1, got %s"
                         % (tuple(parent_idx.shape),))
    pop = parent_idx.numel()
    for name, t, want in (("slot", slot, (pop,)),
                          ("obs_mu", obs_mu, (OBS_DIM,)),
                          ("obs_nu", obs_nu, (OBS_DIM,)),
                          ("env_A", env_A, (OBS_DIM, OBS_DIM)),
                          ("env_B", env_B, (OBS_DIM,))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be >= 1, got %d" % horizon)
    if pop >= 2 ** 31:
        raise ValueError("pop = %d exceeds the launch grid" % pop)
    sigma = _check_ga_sigma(sigma)
    device = parents.device
    fitness = torch.empty(pop, dtype=torch.float32, device=device)
    obs_stat = torch.zeros(2 * OBS_DIM + 1, dtype=torch.float32,
                           device=device)
    bc = torch.empty(pop, BC_DIM, dtype=torch.float32, device=device)
    final = None
    if return_final_states:
        final = torch.empty(pop, ENVS_PER_MEMBER, OBS_DIM,
                            dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        part = _partial_buffer(device, pop * 2 * OBS_DIM)
        ops.ga_rollout_mlp_bc(
            parents.data_ptr(), parent_idx.data_ptr(), slot.data_ptr(),
            sigma, int(seed) & 0xFFFFFFFF, int(generation) & 0xFFFFFFFF,
            horizon, pop, obs_mu.data_ptr(), obs_nu.data_ptr(),
            env_A.data_ptr(), env_B.data_ptr(), fitness.data_ptr(),
            part.data_ptr(), obs_stat.data_ptr(), bc.data_ptr(),
            final.data_ptr() if return_final_states else 0, _stream())
    if return_final_states:
        return fitness, obs_stat, bc, final
    return fitness, obs_stat, bc


def me_insert(fitness, bc, bins, lo, hi, arch_fitness, arch_bc, arch_filled):
    """One generation's competition for the cells of the archive, in place.

    The cell of member ``m``: per dimension ``t = (bc[m][d] - lo32[d]) *
    inv32[d]`` in fp32, each operation rounded once (``me_grid`` gives
    ``lo32`` and ``inv32``), ``b_d = clamp(floor(t), 0, bins[d] - 1)``, and
    ``cell = ((b_0 * bins[1] + b_1) * bins[2] + b_2) * bins[3] + b_3``.  A
    member with a NaN in its BC or a NaN fitness has cell -1 and is never
    inserted.  The winner of a cell is the fittest child that lands in it,
    in ``ga_truncate``'s order (-0 equals +0), the lower member index among
    equals; it displaces the occupant only if it is strictly fitter.

    Updates ``arch_fitness[C]``, ``arch_bc[C][4]`` (the winner's bits) and
    int32 ``arch_filled[C]``, and returns int32 ``(cell[pop], winner[C],
    order[C + 1])``: ``winner[c]`` is the member index or -1 where the cell
    is unchanged, and ``order[c] = winner[c] if winner[c] >= 0 else pop + c``
    with ``order[C] = pop + C``, which ``ga_survivors`` turns into the
    archive's weights when ``parent_idx`` and ``slot`` are extended by ``C +
    1`` pseudo-members (parent ``c``, slot -1).  The result does not depend
    on scheduling.

    TypeError for dtype, device or contiguity; ValueError for shapes, a
    ``bins`` entry below 1, ``C + 1 > GA_ROWS_MAX``, bounds that are not
    finite or not ``hi > lo``, or ``pop`` outside ``[1, GA_TRUNCATE_MAX]``."""
    ops = _require_ops()
    _check_ga_on((("fitness", fitness, torch.float32),
                  ("bc", bc, torch.float32),
                  ("arch_fitness", arch_fitness, torch.float32),
                  ("arch_bc", arch_bc, torch.float32),
                  ("arch_filled", arch_filled, torch.int32)),
                 "fitness", fitness)
    bins, lo32, inv32, C = me_grid(bins, lo, hi)
    if fitness.dim() != 1:
        raise ValueError("fitness must be 1-d, got %s"
                         % (tuple(fitness.shape),))
    pop = fitness.numel()
    if pop < 1 or pop > GA_TRUNCATE_MAX:
        raise ValueError("pop must be in [1, %d], got %d"
                         % (GA_TRUNCATE_MAX, pop))
    for name, t, want in (("bc", bc, (pop, BC_DIM)),
                          ("arch_fitness", arch_fitness, (C,)),
                          ("arch_bc", arch_bc, (C, BC_DIM)),
                          ("arch_filled", arch_filled, (C,))):
        if tuple(t.shape) != want:
            raise ValueError("%s must be %s, got %s"
                             % (name, list(want), tuple(t.shape)))
    for name, t in (("bc", bc), ("arch_bc", arch_bc)):
        if t.data_ptr() % 16:
            raise ValueError("%s must be 16-byte aligned" % name)
    device = fitness.device
    cell = torch.empty(pop, dtype=torch.int32, device=device)
    winner = torch.empty(C, dtype=torch.int32, device=device)
    order = torch.empty(C + 1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        best = torch.empty(C, dtype=torch.int64, device=device)
        ops.me_insert(fitness.data_ptr(), bc.data_ptr(), pop, bins, lo32,
                      inv32, arch_fitness.data_ptr(), arch_bc.data_ptr(),
                      arch_filled.data_ptr(), best.data_ptr(),
                      cell.data_ptr(), winner.data_ptr(), order.data_ptr(),
                      _stream())
    return cell, winner, order


def me_compact(arch_filled, out_filled_idx=None, out_n_filled=None):
    """The compact list of filled cells, in one launch and without a host
    sync: int32 ``(filled_idx[C], n_filled[1])`` with ``filled_idx[0 ..
    n_filled)`` the indices ``c`` with ``arch_filled[c] != 0`` in ascending
    order and -1 behind them.

    TypeError for dtype, device or contiguity; ValueError unless
    ``arch_filled`` is 1-d with ``1 <= C <= ME_CELLS_MAX`` and the outputs,
    if given, are ``[C]`` and one element."""
    ops = _require_ops()
    named = [("arch_filled", arch_filled, torch.int32)]
    if out_filled_idx is not None:
        named.append(("out_filled_idx", out_filled_idx, torch.int32))
    if out_n_filled is not None:
        named.append(("out_n_filled", out_n_filled, torch.int32))
    _check_ga_on(named, "arch_filled", arch_filled)
    if arch_filled.dim() != 1:
        raise ValueError("arch_filled must be 1-d, got %s"
                         % (tuple(arch_filled.shape),))
    C = arch_filled.numel()
    if C < 1 or C > ME_CELLS_MAX:
        raise ValueError("C must be in [1, %d], got %d" % (ME_CELLS_MAX, C))
    device = arch_filled.device
    if out_filled_idx is None:
        out_filled_idx = torch.empty(C, dtype=torch.int32, device=device)
    elif tuple(out_filled_idx.shape) != (C,):
        raise ValueError("out_filled_idx must be [%d], got %s"
                         % (C, tuple(out_filled_idx.shape)))
    if out_n_filled is None:
        out_n_filled = torch.empty(1, dtype=torch.int32, device=device)
    elif out_n_filled.numel() != 1:
        raise ValueError("out_n_filled must hold one element, got %s"
                         % (tuple(out_n_filled.shape),))
    with torch.cuda.device(device):
        ops.me_compact(arch_filled.data_ptr(), C, out_filled_idx.data_ptr(),
                       out_n_filled.data_ptr(), _stream())
    return out_filled_idx, out_n_filled


def ops_available():
    return _OPS is not None
