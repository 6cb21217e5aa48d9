"""Host tests of the novelty-search oracle and host mirrors
(fiber_amd/es/behaviour_oracle.py) and of the validation of the novelty ops
wrappers.  No GPU."""

import collections

import numpy as np
import pytest
import torch

import rollout_oracle_cases as C
from fiber_amd import ops
from fiber_amd.es import behaviour_oracle as bo

u = C.bits._unit


def _rows(n, salt, scale=1.0):
    return (u(n * 4, salt).reshape(n, 4) * scale).astype(np.float32)


def _independent_knn(bc, archive, k):
    """A second computation with no code in common with the oracle: python
    loops, exact rational-free float64 sums per row, a full sort."""
    d2 = []
    for q in bc:
        row = []
        for a in archive:
            acc = 0.0
            for i in range(4):
                d = float(q[i]) - float(a[i])
                acc += d * d
            row.append(acc)
        d2.append(sorted(row)[:k])
    d2 = np.array(d2)
    return d2, np.array([sum(np.sqrt(v) for v in row) / k for row in d2])


@pytest.mark.parametrize("n_q,n_r,k", [(5, 7, 1), (5, 7, 3), (3, 7, 7),
                                       (2, 40, 16), (1, 1, 1)])
def test_oracle_knn_matches_independent_sort(n_q, n_r, k):
    bc = _rows(n_q, 11)
    archive = _rows(n_r, 12)
    if n_r >= 4:
        archive[3] = archive[0]      # duplicated archive rows
        archive[n_r - 1] = archive[0]
        bc[0] = archive[2]           # a query equal to an archive row
    d2, nov = bo.knn_novelty(bc, archive, k)
    want_d2, want_nov = _independent_knn(bc, archive, k)
    assert d2.shape == (n_q, k) and nov.shape == (n_q,)
    assert (np.diff(d2, axis=1) >= 0).all()
    np.testing.assert_allclose(d2, want_d2, rtol=1e-14, atol=0)
    np.testing.assert_allclose(nov, want_nov, rtol=1e-14, atol=0)
    if n_r >= 4:
        assert d2[0, 0] == 0.0
    if n_r >= 4 and k >= 3:
        # the query sitting on archive[2] has one neighbour at 0; the three
        # copies of archive[0] are three separate, equal entries of any
        # query's list that reaches them
        full, _ = bo.knn_novelty(archive[:1], archive, min(n_r, 16, 3))
        assert (full[0] == 0.0).all()


def test_oracle_knn_rejects_bad_input():
    bc, archive = _rows(2, 1), _rows(3, 2)
    with pytest.raises(ValueError):
        bo.knn_novelty(bc, archive, 4)        # k > R
    with pytest.raises(ValueError):
        bo.knn_novelty(bc, archive, 0)
    with pytest.raises(ValueError):
        bo.knn_novelty(bc, archive[:0], 1)    # R == 0
    with pytest.raises(TypeError):
        bo.knn_novelty(bc.astype(np.float64), archive, 1)
    bad = bc.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        bo.knn_novelty(bad, archive, 1)


def test_knn_bound_positive_and_scales_with_magnitude():
    bc, archive = _rows(6, 21), _rows(20, 22)
    bc[0] = archive[5]
    d2, nov = bo.knn_novelty(bc, archive, 5)
    d2_tol, nov_tol = bo.knn_bounds(d2)
    assert (d2_tol > 0).all() and (nov_tol > 0).all()   # at d2 == 0 too
    # first order: 6 U d2 and (3 U + ULP + k U) novelty
    far = d2 > 1e-6
    np.testing.assert_allclose(d2_tol[far], 6 * bo.U * d2[far], rtol=1e-5)
    assert (nov_tol[1:] >= 5 * bo.U * nov[1:]).all()
    assert (nov_tol[1:] <= (5 + 5 + 1) * bo.U * nov[1:]).all()
    # scaling the inputs by 1024 (exact in fp32) scales the bounds with them
    s = np.float32(1024.0)
    d2s, novs = bo.knn_novelty(bc * s, archive * s, 5)
    d2s_tol, novs_tol = bo.knn_bounds(d2s)
    np.testing.assert_allclose(d2s, d2 * 1024.0 ** 2, rtol=1e-14)
    np.testing.assert_allclose(d2s_tol[far], d2_tol[far] * 1024.0 ** 2,
                               rtol=1e-9)
    np.testing.assert_allclose(novs_tol[1:], nov_tol[1:] * 1024.0, rtol=1e-6)


def test_combine_weights_three_modes():
    rf = np.array([-0.5, 0.0, 0.5, 0.25])
    rn = np.array([0.5, -0.5, 0.0, 0.25])
    assert np.array_equal(bo.combine_weights("ns", rf, rn), rn)
    assert np.array_equal(bo.combine_weights("nsr", rf, rn),
                          [0.0, -0.25, 0.25, 0.25])
    assert np.array_equal(bo.combine_weights("nsra", rf, rn, 1.0), rf)
    assert np.array_equal(bo.combine_weights("nsra", rf, rn, 0.0), rn)
    assert np.array_equal(bo.combine_weights("nsra", rf, rn, 0.25),
                          0.25 * rf + 0.75 * rn)
    with pytest.raises(ValueError):
        bo.combine_weights("fit", rf, rn)
    with pytest.raises(ValueError):
        bo.combine_weights("ns", rf, rn[:3])


def test_nsra_schedule():
    w, best, stall = 0.5, float("-inf"), 0
    # an improvement raises w and clears the count
    w, best, stall = bo.nsra_update(w, best, stall, 1.0, 0.25, 3)
    assert (w, best, stall) == (0.75, 1.0, 0)
    # patience - 1 stalls change nothing but the count (a tie is a stall)
    w, best, stall = bo.nsra_update(w, best, stall, 1.0, 0.25, 3)
    w, best, stall = bo.nsra_update(w, best, stall, 0.0, 0.25, 3)
    assert (w, best, stall) == (0.75, 1.0, 2)
    # the patience-th stall lowers w and clears the count
    w, best, stall = bo.nsra_update(w, best, stall, 0.5, 0.25, 3)
    assert (w, best, stall) == (0.5, 1.0, 0)
    # clipped at 0 ...
    for _ in range(9):
        w, best, stall = bo.nsra_update(w, best, stall, 0.0, 0.25, 3)
    assert (w, best, stall) == (0.0, 1.0, 0)
    # ... and at 1
    for i in range(6):
        w, best, stall = bo.nsra_update(w, best, stall, 2.0 + i, 0.25, 3)
    assert (w, best, stall) == (1.0, 7.0, 0)
    # delta 0 leaves w alone either way
    assert bo.nsra_update(1.0, 0.0, 0, 5.0, 0.0, 1)[0] == 1.0
    assert bo.nsra_update(1.0, 9.0, 0, 5.0, 0.0, 1)[0] == 1.0


def test_archive_fifo_order_past_capacity():
    arc = bo.ArchiveMirror(4)
    rows = _rows(7, 31)
    assert arc.count == 0 and arc.rows().shape == (0, 4)
    for i in range(3):
        arc.append(rows[i])
    assert arc.count == 3 and np.array_equal(arc.rows(), rows[:3])
    for i in range(3, 7):
        arc.append(rows[i])
    assert arc.count == 4 and arc.total == 7
    assert np.array_equal(arc.rows(), rows[3:7])   # oldest first
    # the ring itself holds them rotated: slot total % capacity is next
    assert np.array_equal(arc.ring[7 % 4], rows[3])
    with pytest.raises(ValueError):
        bo.ArchiveMirror(0)


def test_choice_probabilities_and_all_zero_fallback():
    p = bo.choice_probabilities([1.0, 3.0, 0.0, 4.0])
    assert np.array_equal(p, [0.125, 0.375, 0.0, 0.5])
    assert np.array_equal(bo.choice_probabilities([0.0, 0.0, 0.0, 0.0]),
                          [0.25] * 4)
    assert np.array_equal(bo.choice_probabilities([0.0]), [1.0])
    for bad in ([], [1.0, -1.0], [float("nan"), 1.0]):
        with pytest.raises(ValueError):
            bo.choice_probabilities(bad)


def test_bc_of_rollout_is_the_mean_final_state():
    ro = C.cell(0, 0)
    for h in C.HORIZONS:
        bc, tol = bo.bc_of_rollout(ro, h)
        want = np.stack([ro.states[e, h] for e in range(64)]).sum(0) / 64.0
        np.testing.assert_allclose(bc, want, rtol=1e-14)
        assert bc.shape == (4,) and tol.shape == (4,)
        want_tol = (ro.state_err[:, h].mean(0)
                    + 6 * bo.U * np.abs(ro.states[:, h]).mean(0))
        np.testing.assert_allclose(tol, want_tol, rtol=1e-14)
        assert (tol > 0).all()
    # horizon 0 is the init state
    bc0, _ = bo.bc_of_rollout(ro, 0)
    np.testing.assert_allclose(bc0, ro.states[:, 0].mean(0), rtol=1e-14)
    # a Rollout-shaped stand-in: a known mean, dim by dim
    Fake = collections.namedtuple("Fake", ["states", "state_err"])
    states = np.zeros((64, 2, 4))
    states[:, 1] = np.arange(64)[:, None] * np.array([1.0, 2.0, -1.0, 0.0])
    bc, tol = bo.bc_of_rollout(Fake(states, np.zeros((64, 2, 4))), 1)
    assert np.array_equal(bc, [31.5, 63.0, -31.5, 0.0])
    assert np.array_equal(tol, 6 * bo.U * np.array([31.5, 63.0, 31.5, 0.0]))


# ---- wrapper validation: everything is refused before a launch, so the
# dtype / device / contiguity errors need no GPU ---------------------------

def test_wrappers_export_the_kernel_limits():
    assert ops.ops_available()
    assert ops.BC_KNN_MAX == 16 == bo.KNN_MAX
    assert ops.BC_KNN_TILE >= 256 and ops.BC_DIM == 4


def test_bc_knn_novelty_refuses_host_and_wrong_dtype_tensors():
    bc, archive = torch.zeros(3, 4), torch.zeros(5, 4)
    with pytest.raises(TypeError):
        ops.bc_knn_novelty(bc, archive, 1)             # not on the device
    with pytest.raises(TypeError):
        ops.bc_knn_novelty(bc.double(), archive, 1)
    with pytest.raises(TypeError):
        ops.bc_knn_novelty(bc, archive.to(torch.int32), 1)


def test_rollout_bc_wrappers_refuse_host_and_wrong_dtype_tensors():
    theta = torch.zeros(ops.NPARAMS)
    mu, nu = torch.zeros(4), torch.ones(4)
    A, B = torch.zeros(4, 4), torch.zeros(4)
    with pytest.raises(TypeError):
        ops.es_rollout_mlp_bc(theta, 0.05, 1, 0, 4, 0, 2, mu, nu, A, B)
    with pytest.raises(TypeError):
        ops.es_rollout_mlp_bc(theta.double(), 0.05, 1, 0, 4, 0, 2, mu, nu,
                              A, B)
    with pytest.raises(TypeError):
        ops.es_eval_bc(theta[None], mu[None], nu[None], A[None], B[None],
                       1, 0, 4)
    with pytest.raises(TypeError):
        ops.es_eval_bc(theta[None].half(), mu[None], nu[None], A[None],
                       B[None], 1, 0, 4)


def test_engine_refuses_a_ring_context_and_bad_configs():
    from fiber_amd.es import ESConfig, NoveltyConfig, NoveltyESEngine

    cfg = ESConfig(pop_per_gpu=8, horizon=4)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        NoveltyESEngine(cfg, NoveltyConfig(), ctx=object())
    cpu = torch.device("cpu")
    for bad in (NoveltyConfig(mode="fitness"), NoveltyConfig(k=17),
                NoveltyConfig(k=0), NoveltyConfig(meta_size=0),
                NoveltyConfig(meta_size=3, archive_capacity=2),
                NoveltyConfig(weight=1.5), NoveltyConfig(patience=0)):
        with pytest.raises(ValueError):
            NoveltyESEngine(cfg, bad, device=cpu)
    with pytest.raises(ValueError):
        NoveltyESEngine(ESConfig(pop_per_gpu=7), NoveltyConfig(), device=cpu)
