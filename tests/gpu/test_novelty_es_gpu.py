"""GPU tests of novelty-search ES: the BC rollout kernels, the kNN novelty
kernel and NoveltyESEngine.

Two kinds of check.  The new rollout kernels are pinned to the bits of
their siblings (es_rollout_mlp, es_eval_matrix) wherever they compute the
same thing, and the engine to ESEngine's when its weights are fitness
ranks.  What is new — final states, BC, novelty — is held to references
that share no code with it: the per-episode fp64 rollout oracle
(fiber_amd/es/rollout_oracle.py) and the brute-force fp64 kNN of
fiber_amd/es/behaviour_oracle.py, with the bounds derived there.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import rollout_oracle_cases as C  # noqa: E402
from fiber_amd.es import behaviour_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

if torch.cuda.is_available():
    from fiber_amd import ops
    from fiber_amd.es import (ESConfig, ESEngine, NoveltyConfig,
                              NoveltyESEngine)

U = bo.U
CELLS = [(k, m) for k in range(C.K) for m in range(C.M)]


def _dev():
    return torch.device("cuda", 0)


def _device_member_args():
    return [torch.from_numpy(a).to(_dev()).contiguous()
            for a in C.member_args()]


def _f64(t):
    return t.cpu().double().numpy()


# ---- 1. rollout bit-identity -------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("offset", (0, 3))
@pytest.mark.parametrize("horizon", (8, 17))
def test_rollout_bc_keeps_the_bits_of_es_rollout_mlp(horizon, offset):
    """fitness and obs_stat, both parities of horizon & 1, an offset that
    splits an antithetic pair; with and without the final-state store."""
    theta, mu, nu, A, B = _device_member_args()
    args = (theta, 0.05, C.SEED, C.ITER, horizon, offset, 8, mu, nu, A, B)
    fit, stat = ops.es_rollout_mlp(*args)
    fit2, stat2, bc = ops.es_rollout_mlp_bc(*args)
    fit3, stat3, bc3, final = ops.es_rollout_mlp_bc(
        *args, return_final_states=True)
    assert torch.equal(fit2, fit) and torch.equal(stat2, stat)
    assert torch.equal(fit3, fit) and torch.equal(stat3, stat)
    assert torch.equal(bc3, bc)
    assert tuple(bc.shape) == (8, 4) and tuple(final.shape) == (8, 64, 4)
    assert torch.isfinite(bc).all() and torch.isfinite(final).all()


# ---- 2. final states and BC of perturbed members against the oracle ----------

@requires_gpu
@pytest.mark.parametrize("sigma", C.SIGMAS)
def test_member_final_states_and_bc_against_oracle(sigma):
    theta, mu, nu, A, B = _device_member_args()
    compared = 0
    for seed, off, h_max in C.LAUNCHES[sigma]:
        ros = C.launch(sigma, seed, off)
        assert len(ros) == C.POP
        for h in range(1, h_max + 1):
            # from the oracle alone: all POP * 64 episodes decided through h
            assert all(ro.decided[:, h - 1].all() for ro in ros), (
                sigma, seed, off, h)
            _fit, _stat, bc, final = ops.es_rollout_mlp_bc(
                theta, sigma, seed, C.ITER, h, off, C.POP, mu, nu, A, B,
                return_final_states=True)
            bc, final = _f64(bc), _f64(final)
            for i, ro in enumerate(ros):
                err = np.abs(final[i] - ro.states[:, h])
                tol = ro.state_err[:, h]
                want_bc, bc_tol = bo.bc_of_rollout(ro, h)
                bc_err = np.abs(bc[i] - want_bc)
                print("sigma=%g seed=%d off=%d h=%d member %d: state max "
                      "err/tol %.3f, bc err %s tol %s"
                      % (sigma, seed, off, h, off + i, (err / tol).max(),
                         bc_err, bc_tol))
                assert (err <= tol).all(), (
                    sigma, seed, off, h, i, np.argwhere(err > tol).tolist())
                assert (bc_err <= bc_tol).all(), (
                    sigma, seed, off, h, i, bc[i], want_bc, bc_tol)
                compared += 1
    assert compared >= 2 * C.POP


# ---- 3. es_eval_bc -----------------------------------------------------------------

def _assert_coverage():
    """The coverage conditions, from the oracle alone."""
    seen = {h: np.zeros(64, bool) for h in C.HORIZONS}
    for k, m in CELLS:
        dec = C.cell(k, m).decided
        for h in C.HORIZONS:
            share = dec[:, h - 1].mean()
            if h <= C.CAP_SHORT_H:
                assert share >= C.CAP_SHORT, (k, m, h, share)
            if h <= C.CAP_LONG_H:
                assert share >= C.CAP_LONG, (k, m, h, share)
            seen[h] |= dec[:, h - 1]
    for h in C.HORIZONS:
        assert seen[h].all(), (h, np.flatnonzero(~seen[h]))


@requires_gpu
def test_eval_bc_bits_of_eval_matrix_and_final_states_against_oracle():
    _assert_coverage()
    inp = C.inputs_torch(_dev())
    for h in C.HORIZONS:
        scores, episodes = ops.es_eval_matrix(*inp, C.SEED, C.ITER, h,
                                              return_episodes=True)
        s2, bc, final, ep2 = ops.es_eval_bc(
            *inp, C.SEED, C.ITER, h, return_final_states=True,
            return_episodes=True)
        s3, bc3 = ops.es_eval_bc(*inp, C.SEED, C.ITER, h)
        assert torch.equal(s2, scores) and torch.equal(ep2, episodes)
        assert torch.equal(s3, scores) and torch.equal(bc3, bc)
        assert tuple(bc.shape) == (C.K, C.M, 4)
        assert tuple(final.shape) == (C.K, C.M, 64, 4)
        bc, final = _f64(bc), _f64(final)
        assert np.isfinite(final).all()
        for k, m in CELLS:
            ro = C.cell(k, m)
            dec = ro.decided[:, h - 1]
            err = np.abs(final[k, m] - ro.states[:, h])
            tol = ro.state_err[:, h]
            print("h=%d cell(%d,%d): compared %d/64, max err/tol %.3f"
                  % (h, k, m, dec.sum(), (err[dec] / tol[dec]).max()))
            bad = dec[:, None] & (err > tol)
            assert not bad.any(), (h, k, m, np.argwhere(bad).tolist())
            # the BC is the tree mean of the kernel's own final states:
            # each of the 64 values passes 6 rounded adds, / 64 is exact
            mean = final[k, m].mean(0)
            assert (np.abs(bc[k, m] - mean)
                    <= 6 * U * np.abs(final[k, m]).mean(0)).all(), (h, k, m)
            if dec.all():
                want_bc, bc_tol = bo.bc_of_rollout(ro, h)
                assert (np.abs(bc[k, m] - want_bc) <= bc_tol).all()


# ---- 4. sigma = 0 agreement ------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("horizon", (8, 17))
def test_rollout_bc_at_sigma_zero_equals_eval_bc(horizon):
    thetas, mu, nu, A, B = C.inputs_torch(_dev())
    scores, bc, final = ops.es_eval_bc(thetas, mu, nu, A, B, C.SEED, C.ITER,
                                       horizon, return_final_states=True)
    for k, m in CELLS:
        fit, _stat, mbc, mfinal = ops.es_rollout_mlp_bc(
            thetas[k], 0.0, C.SEED, C.ITER, horizon, 0, 2, mu[k], nu[k],
            A[m], B[m], return_final_states=True)
        for member in (0, 1):   # both members of the pair
            assert torch.equal(mbc[member], bc[k, m]), (k, m, member)
            assert torch.equal(mfinal[member], final[k, m])
            assert torch.equal(fit[member], scores[k, m])
    # distinct cells: a k / m mix-up cannot pass by accident
    assert len({tuple(r) for r in bc.reshape(-1, 4).cpu().tolist()}) \
        == len(CELLS)


# ---- 5. bc_knn_novelty against the fp64 oracle -------------------------------------

KNN_N = (1, 63, 64, 257)
SENTINEL = -12345.0


def _knn_cases():
    tile = ops.BC_KNN_TILE if torch.cuda.is_available() else 1024
    cases = [(R, k, 1.0)
             for R in (1, 16, tile - 1, tile, tile + 1, 2 * tile + 3)
             for k in (1, 3, 16) if k <= R]
    cases.append((tile + 1, 3, 1e3))
    return cases


def _knn_inputs(N, R, scale):
    """Hash inputs (no library RNG): archive rows in [-scale/2, scale/2)^4
    with duplicated rows, queries of which some sit on archive rows."""
    u = C.bits._unit
    archive = (u(R * 4, 70 + R % 7).reshape(R, 4) * scale).astype(np.float32)
    bc = (u(N * 4, 90 + N % 5).reshape(N, 4) * scale).astype(np.float32)
    if R > 2:
        archive[R // 2] = archive[0]
        archive[R - 1] = archive[0]
    bc[0] = archive[R // 3]           # distance 0
    if N > 2:
        bc[N - 1] = archive[0]        # distance 0, to a duplicated row
    return bc, archive


@requires_gpu
@pytest.mark.parametrize("R,k,scale", _knn_cases())
def test_bc_knn_novelty_against_oracle(R, k, scale):
    for N in KNN_N:
        bc, archive = _knn_inputs(N, R, scale)
        want_d2, want_nov = bo.knn_novelty(bc, archive, k)
        d2_tol, nov_tol = bo.knn_bounds(want_d2)
        out = torch.full((N + 7,), SENTINEL, device=_dev())
        out_nb = torch.full(((N + 7) * k,), SENTINEL, device=_dev())
        nov, nb = ops.bc_knn_novelty(
            torch.from_numpy(bc).to(_dev()),
            torch.from_numpy(archive).to(_dev()), k, out=out,
            out_neighbours=out_nb)
        assert nov.data_ptr() == out.data_ptr()
        out, out_nb = _f64(out), _f64(out_nb)
        # rows past N are untouched
        assert (out[N:] == SENTINEL).all()
        assert (out_nb[N * k:] == SENTINEL).all()
        got_nov, got_d2 = out[:N], out_nb[:N * k].reshape(N, k)
        assert (np.diff(got_d2, axis=1) >= 0).all()      # ascending
        d2_err = np.abs(got_d2 - want_d2)
        nov_err = np.abs(got_nov - want_nov)
        print("N=%d R=%d k=%d scale=%g: d2 max err/tol %.3f, novelty max "
              "err/tol %.3f" % (N, R, k, scale, (d2_err / d2_tol).max(),
                                (nov_err / nov_tol).max()))
        assert (d2_err <= d2_tol).all(), np.argwhere(d2_err > d2_tol)
        assert (nov_err <= nov_tol).all(), np.argwhere(nov_err > nov_tol)
        assert got_d2[0, 0] == 0.0        # the query on an archive row
        # without the optional output the novelty has the same bits
        plain = ops.bc_knn_novelty(torch.from_numpy(bc).to(_dev()),
                                   torch.from_numpy(archive).to(_dev()), k)
        assert np.array_equal(_f64(plain), got_nov)


@requires_gpu
def test_novelty_wrappers_validate_before_launching():
    dev = _dev()
    bc, archive = torch.zeros(3, 4, device=dev), torch.zeros(5, 4, device=dev)
    for bad_k in (0, 6, 17, -1):
        with pytest.raises(ValueError):
            ops.bc_knn_novelty(bc, archive, bad_k)       # k > R, k > 16 ...
    with pytest.raises(ValueError):
        ops.bc_knn_novelty(bc, archive[:0], 1)           # R == 0
    with pytest.raises(ValueError):
        ops.bc_knn_novelty(bc[:0], archive, 1)
    with pytest.raises(ValueError):
        ops.bc_knn_novelty(torch.zeros(3, 3, device=dev), archive, 1)
    with pytest.raises(ValueError):
        ops.bc_knn_novelty(bc, archive, 1, out=torch.zeros(2, device=dev))
    with pytest.raises(TypeError):
        ops.bc_knn_novelty(bc, torch.zeros(5, 8, device=dev)[:, :4], 1)
    with pytest.raises(TypeError):
        ops.bc_knn_novelty(bc.cpu(), archive, 1)
    theta, mu, nu, A, B = _device_member_args()
    with pytest.raises(ValueError):
        ops.es_rollout_mlp_bc(theta, 0.05, 1, 0, 0, 0, 2, mu, nu, A, B)
    with pytest.raises(ValueError):
        ops.es_rollout_mlp_bc(theta[:-1].contiguous(), 0.05, 1, 0, 4, 0, 2,
                              mu, nu, A, B)
    with pytest.raises(ValueError):
        ops.es_rollout_mlp_bc(theta, 0.05, 1, 0, 4, 0, 0, mu, nu, A, B)
    with pytest.raises(ValueError):
        ops.es_eval_bc(theta[None], mu[None], nu[None], A[None], B[None],
                       1, 0, 0)
    with pytest.raises(ValueError):
        ops.es_eval_bc(theta[None], mu[None], nu[None], A, B[None], 1, 0, 4)


# ---- 6. pure-fitness equivalence ------------------------------------------------------

def _engine(mode="nsr", pop=64, horizon=8, **kw):
    return NoveltyESEngine(ESConfig(pop_per_gpu=pop, horizon=horizon),
                           NoveltyConfig(mode=mode, **kw), device=_dev())


@requires_gpu
def test_nsra_with_unit_weight_is_the_plain_es_engine():
    cfg = ESConfig(pop_per_gpu=64, horizon=8)
    plain = ESEngine(cfg, device=_dev())
    ns = NoveltyESEngine(
        cfg, NoveltyConfig(mode="nsra", weight=1.0, weight_delta=0.0,
                           meta_size=1), device=_dev())
    assert torch.equal(ns.thetas[0], plain.theta)
    for _ in range(3):
        plain.step()
        stats = ns.step()
        assert stats["weight"] == 1.0 and stats["agent"] == 0
    assert plain.theta.abs().sum() > 0
    assert torch.equal(ns.thetas[0], plain.theta)
    assert torch.equal(ns.adam_m[0], plain.adam_m)
    assert torch.equal(ns.adam_v[0], plain.adam_v)
    for f in ("obs_sum", "obs_sumsq", "obs_count", "obs_mu", "obs_nu"):
        assert torch.equal(getattr(ns, f), getattr(plain, f)), f
    assert ns.t_steps == [3] and plain.t_step == 3
    assert stats["archive_size"] == 4


# ---- 7. weights ----------------------------------------------------------------------------

@requires_gpu
def test_nsr_weights_and_novelty_of_a_step():
    eng = _engine("nsr")
    for _ in range(3):
        eng.step()
    archive = eng.archive_rows().cpu().numpy()     # before the step
    assert archive.shape == (4, 4)
    stats = eng.step()
    assert stats["weight"] == 0.5 and stats["archive_size"] == 5
    # novelty of the members' BCs against that archive, k_eff = min(10, 4)
    want_d2, want_nov = bo.knn_novelty(eng.last_bc.cpu().numpy(), archive, 4)
    _d2_tol, nov_tol = bo.knn_bounds(want_d2)
    nov_err = np.abs(_f64(eng.last_novelty) - want_nov)
    assert (nov_err <= nov_tol).all(), (nov_err / nov_tol).max()
    assert abs(stats["novelty_mean"] - want_nov.mean()) <= 1e-5 * want_nov.mean()
    # weights: the host mirror on the reference ranks.  The engine forms
    # fl(0.5 * fl(rf + rn)) in fp32 from fp32 ranks: one rounding in the
    # add, at most U |rf + rn|, and the halving is exact.  Each rank is
    # fl(fl(rank / (n-1)) - 0.5), two roundings of values <= 1, which the
    # kernel and the reference may each place differently: 2 U per rank,
    # halved, for two ranks.
    rf = ops.centered_rank_ref(eng.last_fitness.cpu())
    rn = ops.centered_rank_ref(eng.last_novelty.cpu())
    want_w = bo.combine_weights("nsr", rf.double().numpy(),
                                rn.double().numpy())
    w_tol = U * np.abs(rf.double().numpy() + rn.double().numpy()) + 2 * U
    w_err = np.abs(_f64(eng.last_weights) - want_w)
    assert (w_err <= w_tol).all(), (w_err.max(), w_tol.min())
    assert np.abs(want_w).max() > 0.25      # not a vacuous comparison


# ---- 8. archive ---------------------------------------------------------------------------------

@requires_gpu
def test_archive_is_fifo_and_holds_the_bc_of_each_updated_agent():
    eng = _engine("ns", archive_capacity=4)
    init_bc = eng.agent_bc[0].cpu().numpy().copy()
    assert np.array_equal(eng.archive_rows().cpu().numpy(), init_bc[None])
    snaps = []
    for step in range(6):
        stats = eng.step()
        snaps.append((eng.thetas[0].clone(), eng.obs_mu.clone(),
                      eng.obs_nu.clone(), eng.iteration))
        assert stats["archive_size"] == min(4, step + 2)
    rows = eng.archive_rows()
    assert tuple(rows.shape) == (4, 4)
    for row, (theta, mu, nu, it) in zip(rows, snaps[-4:]):
        _s, bc = ops.es_eval_bc(
            theta[None], mu[None], nu[None], eng.env_A[None],
            eng.env_B[None], eng.cfg.seed, it, eng.cfg.horizon)
        assert torch.equal(row, bc[0, 0])
    assert len({tuple(r) for r in rows.cpu().tolist()}) == 4
    # the host mirror keeps the same order
    mirror = bo.ArchiveMirror(4)
    mirror.append(init_bc)                          # the construction BC
    for theta, mu, nu, it in snaps:
        _s, bc = ops.es_eval_bc(
            theta[None], mu[None], nu[None], eng.env_A[None],
            eng.env_B[None], eng.cfg.seed, it, eng.cfg.horizon)
        mirror.append(bc[0, 0].cpu().numpy())
    assert np.array_equal(mirror.rows(), rows.cpu().numpy())
    assert np.array_equal(mirror.ring, eng.archive.cpu().numpy())


# ---- 9. checkpoint ------------------------------------------------------------------------------

def _assert_state_equal(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if torch.is_tensor(a[key]):
            assert torch.equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


@requires_gpu
def test_checkpoint_resumes_bit_identically(tmp_path):
    kw = dict(meta_size=2, weight=0.5, weight_delta=0.25, patience=1,
              archive_capacity=5)
    first = _engine("nsra", **kw)
    for _ in range(2):
        first.step()
    path = str(tmp_path / "ns.pt")
    first.save(path)
    second = _engine("nsra", **kw)
    second.load(path)
    _assert_state_equal(first.state_dict(), second.state_dict())
    for _ in range(2):
        a, b = first.step(), second.step()
        assert a == b
    state = first.state_dict()
    _assert_state_equal(state, second.state_dict())
    assert state["iteration"] == 4 and state["archive_total"] == 6
    assert sum(state["t_steps"]) == 4


# ---- 10. meta-population --------------------------------------------------------------------------

@requires_gpu
def test_meta_population_is_reproducible_and_updates_one_agent():
    runs = []
    for _ in range(2):
        eng = _engine("nsr", meta_size=3)
        assert eng.archive_size == 3
        assert not torch.equal(eng.thetas[0], eng.thetas[1])
        probs = eng.choice_probabilities()
        want = bo.choice_probabilities(
            _f64(ops.bc_knn_novelty(eng.agent_bc, eng.archive[:3], 3)))
        np.testing.assert_allclose(probs.numpy(), want, rtol=1e-14)
        assert abs(want.sum() - 1.0) < 1e-12 and (want > 0).all()
        agents = []
        for _step in range(4):
            before = eng.thetas.clone()
            stats = eng.step()
            agents.append(stats["agent"])
            for m in range(3):
                same = torch.equal(eng.thetas[m], before[m])
                assert same == (m != stats["agent"]), (m, stats["agent"])
        runs.append((agents, eng.thetas.clone(), eng.archive.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])
