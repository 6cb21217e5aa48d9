"""GPU tests of the PATA-EC novelty kernels against the numpy oracle
(fiber_amd/es/novelty_oracle.py, itself checked by hand-worked cases in
tests/test_poet_reproduce.py).

``pata_ec_codes`` and ``knn_d2`` are integers and must equal the oracle
exactly; ``novelty`` must lie within ``novelty_bound``, the derived bound
of the kernel's float tail.  The shapes are the smallest that reach every
path of the kernels: K that is no multiple of 8 (the pad) or of 64 (a
partial LDS K-tile) up to the cap of 512, n_ref below, at and above one
512-row reference tile (1, 3, 257, 1000), Q that leaves a block's query
slots empty (1, 3, 65 = 16 blocks + 1), and k = 1, 5, 64 including
k > n_ref.
"""

import numpy as np
import pytest
import torch

from fiber_amd.es import novelty_oracle as no

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

if torch.cuda.is_available():
    from fiber_amd import ops

NAN, INF = float("nan"), float("inf")

# (K, n_ref, Q, k, kind)
CASES = [
    (2, 1, 1, 1, "random"),
    (2, 3, 3, 5, "clipped"),       # k > n_ref
    (5, 3, 65, 64, "special"),     # k > n_ref
    (5, 257, 3, 5, "random"),
    (67, 257, 65, 64, "clipped"),
    (67, 1000, 3, 5, "special"),
    (67, 1000, 1, 64, "duplicate"),
    (130, 1, 3, 1, "duplicate"),
    (130, 257, 1, 5, "special"),
    (130, 1000, 65, 64, "random"),
    (512, 3, 1, 5, "antipodal"),   # k > n_ref
    (512, 257, 3, 5, "random"),
    (512, 1000, 65, 64, "clipped"),
]


def _case_id(case):
    return "K%d-ref%d-Q%d-k%d-%s" % case


def _inputs(case):
    """(scores[K][M] fp32 numpy, clip_lo, clip_hi), seeded by the case."""
    K, n_ref, Q, k, kind = case
    M = n_ref + Q
    rng = np.random.default_rng(K * 100003 + n_ref * 101 + Q * 7 + k)
    scores = rng.normal(size=(K, M)).astype(np.float32)
    lo, hi = -1.0, 1.0
    if kind == "clipped":
        lo, hi = 0.2, 1.5  # P(x <= 0.2) = 0.58: most entries sit at lo
    elif kind == "special":
        for value in (NAN, INF, -INF, 0.0, -0.0):
            hit = rng.random(size=scores.shape) < 0.08
            scores[hit] = value
        scores[:, M - 1] = NAN  # a query nobody finished
        scores[0, 0], scores[1, 0] = 0.0, -0.0
    elif kind == "duplicate":
        # the last query repeats a reference, another reference repeats it
        scores[:, M - 1] = scores[:, n_ref // 2]
        if n_ref > 2:
            scores[:, 0] = scores[:, n_ref // 2]
    elif kind == "antipodal":
        # permutations, unclipped: reference 0 ascending, the query
        # descending, the largest D2 that rank vectors can have
        lo, hi = -INF, INF
        up = np.arange(K, dtype=np.float32)
        scores[:, 0] = up
        scores[:, n_ref - 1] = np.roll(up, 1)
        scores[:, n_ref] = up[::-1]
    return scores, lo, hi


def _run(case, scores, lo, hi):
    K, n_ref, Q, k, _kind = case
    dev_scores = torch.from_numpy(scores).cuda()
    codes = ops.pata_ec_codes(dev_scores, lo, hi)
    novelty, knn_d2 = ops.env_novelty(dev_scores, n_ref, k, lo, hi,
                                      return_neighbours=True)
    return codes, novelty, knn_d2


@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_codes_and_neighbours_exact_novelty_in_bound(case):
    K, n_ref, Q, k, kind = case
    M, Kpad, k_eff = n_ref + Q, (K + 7) // 8 * 8, min(k, n_ref)
    scores, lo, hi = _inputs(case)
    want_codes = no.codes_oracle(scores, lo, hi)
    want_d2, want_nov = no.knn_oracle(want_codes, n_ref, k)

    codes, novelty, knn_d2 = _run(case, scores, lo, hi)
    assert codes.dtype == torch.int16 and tuple(codes.shape) == (M, Kpad)
    assert knn_d2.dtype == torch.int32 and tuple(knn_d2.shape) == (Q, k_eff)
    assert novelty.dtype == torch.float32 and tuple(novelty.shape) == (Q,)
    codes = codes.cpu().numpy().astype(np.int64)
    knn_d2 = knn_d2.cpu().numpy().astype(np.int64)
    novelty = novelty.cpu().numpy().astype(np.float64)

    assert np.array_equal(codes[:, :K], want_codes)
    assert not codes[:, K:].any()  # the pad entries
    assert np.array_equal(knn_d2, want_d2)
    err = np.abs(novelty - want_nov)
    bound = no.novelty_bound(want_nov, k_eff)
    print("%s: max |novelty - oracle| = %.3e, bound there %.3e, max D2 %d"
          % (_case_id(case), err.max(), bound[err.argmax()], want_d2.max()))
    assert (err <= bound).all(), (err.max(), bound[err.argmax()])

    # the case is what its name says
    if kind == "clipped":
        assert (no.clip_scores(scores, lo, hi) == np.float32(lo)).mean() >= 0.5
    if kind == "duplicate":
        assert want_d2[-1, 0] == 0 and novelty[-1] >= 0.0
        if k_eff == 1:
            assert novelty[-1] == 0.0
    if kind == "antipodal":
        # 4 K (K^2 - 1) / 3, of the 2^31 that int32 holds
        assert want_d2[0, -1] == 4 * K * (K * K - 1) // 3 == 178956288
    if kind == "special":
        assert (want_codes[M - 1] == K - 1).all()  # the all-NaN column ties


@requires_gpu
def test_case_grid_covers_every_size_class():
    assert {c[0] for c in CASES} == {2, 5, 67, 130, 512}
    assert {c[1] for c in CASES} == {1, 3, 257, 1000}
    assert {c[2] for c in CASES} == {1, 3, 65}
    assert {c[3] for c in CASES} == {1, 5, 64}
    assert any(c[3] > c[1] for c in CASES)
    assert {c[4] for c in CASES} == {"random", "clipped", "special",
                                     "duplicate", "antipodal"}
    assert len(set(CASES)) == len(CASES)


@requires_gpu
def test_pad_region_is_zeroed_whatever_the_buffer_held():
    """K = 5 leaves 3 pad entries per row.  The codes buffer is taken from
    the caching allocator, so a freed block of its size full of 0x7F7F is
    what it gets; the pads must come out 0 and the distances must be those
    of the 5 real entries (hand-built: D2 by hand below)."""
    scores = torch.tensor([[0.0, 4.0, 0.0],
                           [1.0, 3.0, 1.0],
                           [2.0, 2.0, 2.0],
                           [3.0, 1.0, 3.0],
                           [4.0, 0.0, 4.0]], device="cuda")
    poison = torch.full((3, 8), 0x7F7F, dtype=torch.int16, device="cuda")
    ptr = poison.data_ptr()
    del poison
    codes = ops.pata_ec_codes(scores, -10.0, 10.0)
    print("codes reuses the poisoned block:", codes.data_ptr() == ptr)
    assert codes.cpu().tolist() == [[0, 2, 4, 6, 8, 0, 0, 0],
                                    [8, 6, 4, 2, 0, 0, 0, 0],
                                    [0, 2, 4, 6, 8, 0, 0, 0]]
    poison = torch.full((3, 8), 0x7F7F, dtype=torch.int16, device="cuda")
    del poison
    novelty, knn_d2 = ops.env_novelty(scores, 2, 2, -10.0, 10.0,
                                      return_neighbours=True)
    # query = reference 0; reference 1 is its reverse: 64+16+0+16+64
    assert knn_d2.cpu().tolist() == [[0, 160]]
    want = np.sqrt(160.0) / (2 * 2 * 4)
    assert abs(float(novelty[0]) - want) <= no.novelty_bound(want, 2)


@requires_gpu
def test_two_calls_give_identical_bits():
    case = (67, 1000, 65, 64, "clipped")
    scores, lo, hi = _inputs(case)
    first = _run(case, scores, lo, hi)
    second = _run(case, scores, lo, hi)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype
        raw = torch.int32 if a.dtype == torch.float32 else a.dtype
        assert torch.equal(a.view(raw), b.view(raw))
    # return_neighbours=False returns the same novelty alone
    alone = ops.env_novelty(torch.from_numpy(scores).cuda(), 1000, 64, lo, hi)
    assert torch.equal(alone.view(torch.int32), first[1].view(torch.int32))


@requires_gpu
def test_bad_arguments_raise_before_any_launch(monkeypatch):
    dev = torch.device("cuda", 0)
    good = torch.rand(4, 6, device=dev)
    launches = []

    class Recorder:
        def pata_ec_codes(self, *args):
            launches.append("codes")

        def pata_ec_knn(self, *args):
            launches.append("knn")

    monkeypatch.setattr(ops, "_OPS", Recorder())

    def novelty(scores=good, n_ref=4, k=2, lo=-1.0, hi=1.0):
        return ops.env_novelty(scores, n_ref, k, lo, hi)

    for bad in (good.double(), good.half(), good.cpu(),
                torch.rand(4, 12, device=dev)[:, ::2]):
        with pytest.raises(TypeError):
            novelty(scores=bad)
        with pytest.raises(TypeError):
            ops.pata_ec_codes(bad, -1.0, 1.0)
    for kwargs in (dict(scores=torch.rand(1, 6, device=dev)),
                   dict(scores=torch.rand(513, 6, device=dev)),
                   dict(scores=torch.rand(4, device=dev)),
                   dict(scores=torch.rand(2, 4, 6, device=dev)),
                   dict(scores=torch.rand(4, 0, device=dev)),
                   dict(k=0), dict(k=65), dict(k=-1),
                   dict(n_ref=0), dict(n_ref=-2),
                   dict(n_ref=6), dict(n_ref=7),
                   dict(lo=1.0, hi=-1.0), dict(lo=NAN), dict(hi=NAN)):
        with pytest.raises(ValueError):
            novelty(**kwargs)
    for args in ((torch.rand(1, 6, device=dev), -1.0, 1.0),
                 (torch.rand(513, 6, device=dev), -1.0, 1.0),
                 (good, 1.0, -1.0)):
        with pytest.raises(ValueError):
            ops.pata_ec_codes(*args)
    assert launches == []
    # the recorder does see valid calls: the checks above are live
    novelty()
    ops.pata_ec_codes(good, -1.0, 1.0)
    novelty(scores=torch.rand(512, 2, device=dev), n_ref=1, k=64)
    assert launches == ["codes", "knn", "codes", "codes", "knn"]
