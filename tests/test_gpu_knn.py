"""The k smallest squared distances on the device (include/mcpc.h: mcpc_knn_accumulate; csrc/mcpc_knn.h) against fp64 brute force on the
same fp32 rows, under the bound derived in tests/knn_cases.py; exactly on integer data; bitwise whatever the chunking and the order of
the reference rows; and the estimator built on it against the values the reference's own KLdivergence recorded
(tests/golden/g17_knn_kl/g17_knn_kl.npz).

Shapes: nq on both sides of a workgroup's queries (256 lanes x 2..8 rows), nr of one row, fewer than k, a ragged first tile, several
tiles and several splits with a ragged tail (tiles hold 256 or 128 rows), every d at and above a power of two -- 1, 3, 5, 8 have
their own instantiation, 17 runs on 24, 32 on 32 -- and every k."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import knn_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ = (1, 63, 257, 1000)
NR = (1, 2, 65, 1025, 4099)
DS = (1, 3, 5, 8, 17, 32)
KS = (1, 2, 4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_knn_kl", "g17_knn_kl.npz")


def _rows(seed, n, d, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-64, 65, size=(n, d)).astype(np.float32)
    return rng.standard_normal((n, d)).astype(np.float32)


def _knn(q, ref, k, accumulate=False, best=None, poison=-7.0):
    """best [nq, k] as numpy; `best` (a device tensor) is updated in place when given, else a poisoned one is made."""
    from montecarlopredictivecoding_amd.engine import knn_accumulate
    qd, rd = torch.tensor(q, device=DEV), torch.tensor(ref, device=DEV)
    if best is None:
        best = torch.full((q.shape[0], k), poison, dtype=torch.float32, device=DEV)
    knn_accumulate(qd, rd, k, best, accumulate=accumulate)
    return best.cpu().numpy()


_REF = {}


def _reference(nq, nr, d, integer=False):
    """(q, ref, fp64 4-best) of a shape; computed once, shared, never modified."""
    key = (nq, nr, d, integer)
    if key not in _REF:
        q, ref = _rows(100 + nq + d, nq, d, integer), _rows(200 + nr + d, nr, d, integer)
        if integer and nr >= 3 and nq >= 2:
            ref[nr // 2], ref[nr // 3] = q[0], q[0]                     # exact ties, and a distance of 0
        want = R.kbest(q, ref, 4)
        for a in (q, ref, want):
            a.setflags(write=False)
        _REF[key] = (q, ref, want)
    return _REF[key]


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("nq", NQ)
def test_against_fp64_brute_force(nq, d):
    worst = 0.0
    for nr in NR:
        q, ref, want = _reference(nq, nr, d)
        finite = want[np.isfinite(want)]
        assert finite.size == 0 or float(finite[finite > 0].min()) > 1e-30          # no squared distance is subnormal
        for k in KS:
            got = _knn(q, ref, k)
            w = want[:, :k]
            assert got.shape == (nq, k) and got.dtype == np.float32
            assert np.array_equal(np.isinf(got), np.isinf(w)), (nr, k)              # nr < k: the trailing slots are +inf
            assert bool((got[:, :-1] <= got[:, 1:]).all())                          # ascending
            m = np.isfinite(w)
            err = np.abs(got[m].astype(np.float64) - w[m]) / w[m]
            if err.size:
                worst = max(worst, float(err.max()))
            assert err.size == 0 or float(err.max()) <= R.dist_bound(d), (nr, k, float(err.max()), R.dist_bound(d))
    print("nq=%d d=%d: worst relative error %.3g of (d + 3) 2^-24 = %.3g" % (nq, d, worst, R.dist_bound(d)))


@pytest.mark.parametrize("d", DS)
def test_integer_coordinates_are_exact(d):
    """Coordinates in [-64, 64]: differences, squares (<= 2^14) and sums (<= 2^19) are integers below 2^24, every fp32 operation is exact."""
    for nq in NQ:
        for nr in NR:
            q, ref, want = _reference(nq, nr, d, integer=True)
            for k in KS:
                got = _knn(q, ref, k)
                assert np.array_equal(got.astype(np.float64), want[:, :k]), (nq, nr, k)           # ties and +inf included


@pytest.mark.parametrize("d, k", [(1, 1), (3, 4), (5, 2), (8, 3), (17, 2), (32, 4)])
def test_bitwise_invariance_under_chunking_and_order(d, k):
    from montecarlopredictivecoding_amd.engine import knn_accumulate
    nq, nr = 257, 4099
    q, ref, _ = _reference(nq, nr, d)
    qd = torch.tensor(q, device=DEV)
    whole = torch.full((nq + 2, k), -7.0, dtype=torch.float32, device=DEV)             # rows 0 and nq + 1 guard the output
    knn_accumulate(qd, torch.tensor(ref, device=DEV), k, whole[1:nq + 1], accumulate=False)
    assert bool((whole[0] == -7.0).all()) and bool((whole[nq + 1] == -7.0).all())      # nothing outside best is written
    one = whole[1:nq + 1].clone()
    assert bool((one >= 0).all())                                                      # an overwriting call leaves no poison
    perm = np.random.default_rng(9).permutation(nr)
    for rows in (ref, ref[perm]):
        for chunks in (1, 2, 7):
            best = torch.full((nq, k), float("nan"), dtype=torch.float32, device=DEV)  # the first call overwrites, whatever it held
            cuts = np.linspace(0, nr, chunks + 1).astype(int)
            for j in range(chunks):
                part = torch.tensor(rows[cuts[j]:cuts[j + 1]], device=DEV)
                knn_accumulate(qd, part, k, best, accumulate=j > 0)
            assert torch.equal(best, one), (chunks, rows is ref)
    # accumulating onto +inf is the plain call; a NaN in the old best reads as +inf
    for fill in (float("inf"), float("nan")):
        best = torch.full((nq, k), fill, dtype=torch.float32, device=DEV)
        knn_accumulate(qd, torch.tensor(ref, device=DEV), k, best, accumulate=True)
        assert torch.equal(best, one)
    # an empty reference set: +inf when overwriting, nothing when accumulating
    none = torch.empty(0, d, dtype=torch.float32, device=DEV)
    best = one.clone()
    knn_accumulate(qd, none, k, best, accumulate=True)
    assert torch.equal(best, one)
    knn_accumulate(qd, none, k, best, accumulate=False)
    assert bool(torch.isinf(best).all())


def test_fewer_reference_rows_than_k():
    q, ref, _ = _reference(63, 2, 5)
    got = _knn(q, ref, 4)
    assert bool(np.isfinite(got[:, :2]).all()) and bool(np.isposinf(got[:, 2:]).all())
    got = _knn(q, ref[:1], 2)
    assert bool(np.isfinite(got[:, 0]).all()) and bool(np.isposinf(got[:, 1]).all())


@pytest.mark.parametrize("d, k", [(5, 2), (17, 4), (3, 1)])
def test_non_finite_rows(d, k):
    nq, nr = 257, 1025
    q, ref, _ = _reference(nq, nr, d)
    q, ref = q.copy(), ref.copy()
    ref[100] = np.nan                                       # in the middle of the first tile
    ref[101, d - 1] = np.nan
    ref[300, 0] = np.inf
    ref[301] = -np.inf
    q[7, 0] = np.nan
    q[130] = np.nan
    q[131, d - 1] = np.inf                                   # every distance of this row is +inf (or NaN against ref[300] for d = 1)
    want = R.kbest(q, ref, k)
    got = _knn(q, ref, k)
    assert not np.isnan(got).any()                          # a NaN distance is never selected
    assert bool(np.isposinf(got[[7, 130, 131]]).all())      # a query row that holds a NaN keeps +inf
    m = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), m)
    assert float((np.abs(got[m] - want[m]) / want[m]).max()) <= R.dist_bound(d)       # the neighbours are unaffected
    clean = R.kbest(q, np.delete(ref, [100, 101, 300, 301], axis=0), k)
    assert np.array_equal(want, clean)                      # (the reference agrees: those four rows never win)


def test_argument_errors_launch_nothing():
    from montecarlopredictivecoding_amd import _lib
    lib = _lib.load()
    nq, nr, d, k = 63, 65, 5, 2
    q = torch.zeros(nq, d, device=DEV)
    ref = torch.zeros(nr, d, device=DEV)
    best = torch.full((nq, 4), -7.0, device=DEV)
    need = lib.mcpc_knn_workspace_bytes(nq, nr, d, k)
    ws = torch.empty(4 * need, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(d=d, k=k, best=p(best), ws_bytes=need):
        return lib.mcpc_knn_accumulate(0, p(q), nq, p(ref), nr, d, k, best, 0, p(ws), ws_bytes, None)

    for kw in (dict(d=33), dict(k=5), dict(k=0), dict(best=None), dict(ws_bytes=need - 1)):
        assert call(**kw) == -1, kw                                                   # MCPC_EINVAL
        assert lib.mcpc_last_error().decode().startswith("knn:")
    torch.cuda.synchronize()
    assert bool((best == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((best.flatten()[:nq * k] == 0).all()) and bool((best.flatten()[nq * k:] == -7.0).all())


def test_engine_argument_checks():
    from montecarlopredictivecoding_amd.engine import knn_accumulate, knn_workspace_bytes
    q, ref = torch.zeros(10, 5, device=DEV), torch.zeros(20, 5, device=DEV)
    best = torch.zeros(10, 2, device=DEV)
    with pytest.raises(ValueError, match="k: 5"):
        knn_accumulate(q, ref, 5, best)
    with pytest.raises(ValueError, match="33 coordinates"):
        knn_accumulate(torch.zeros(10, 33, device=DEV), torch.zeros(20, 33, device=DEV), 2, best)
    with pytest.raises(ValueError, match="ref: expected shape"):
        knn_accumulate(q, torch.zeros(20, 4, device=DEV), 2, best)
    with pytest.raises(ValueError, match="best: expected shape"):
        knn_accumulate(q, ref, 1, best)
    with pytest.raises(TypeError, match="best: expected torch.float32"):
        knn_accumulate(q, ref, 2, best.double())
    with pytest.raises(ValueError, match="q: expected a tensor on a HIP device"):
        knn_accumulate(q.cpu(), ref, 2, best)
    with pytest.raises(ValueError, match="tensor must be contiguous"):
        knn_accumulate(torch.zeros(5, 10, device=DEV).t(), ref, 2, best)
    with pytest.raises(ValueError, match="workspace: 4 bytes, knn_workspace_bytes asks for"):
        knn_accumulate(q, ref, 2, best, workspace=torch.empty(4, dtype=torch.uint8, device=DEV))
    assert knn_workspace_bytes(10, 20, 5, 2) == 10 * 2 * 4


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_kl_divergence_on_the_fixture_clouds(name):
    from montecarlopredictivecoding_amd import cloud as K
    from montecarlopredictivecoding_amd.utils.training_evaluation import knn_kl_divergence
    g = np.load(GOLDEN)
    x, y, ref = g["x_" + name], g["y_" + name], float(g["kl_" + name])
    n, d = x.shape
    got = K.kl_divergence(x, y)
    assert got.dtype == torch.float64 and got.dim() == 0 and got.device.type == "cuda"
    exact = R.kl_exact(x, y)
    print("%s: device %.12g, exact fp64 %.12g (off by %.3g), reference %.12g (off by %.3g, tolerance %.3g)"
          % (name, float(got), exact, abs(float(got) - exact), ref, abs(float(got) - ref), R.kl_tolerance(d)))
    assert abs(float(got) - ref) <= R.kl_tolerance(d)
    assert abs(float(got) - exact) <= (d + 3) * 2.0 ** -23 * d
    # the same bits from CPU tensors, device tensors, a Cloud, the utility, and a reference set streamed in small chunks
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    as_cloud = K.Cloud(points=xd.reshape(n // 4, 4, d), units=tuple(range(d)), layer=0)
    for a, b in ((torch.from_numpy(x), torch.from_numpy(y)), (xd, yd), (as_cloud, yd)):
        assert torch.equal(K.kl_divergence(a, b), got)
    assert torch.equal(knn_kl_divergence(x, y), got)
    s_whole = K.knn_sqdist(xd, yd, 1)
    s_cut = K.knn_sqdist(xd, yd, 1, chunk_bytes=4 * d * 97)
    assert tuple(s_whole.shape) == (n, 1) and torch.equal(s_whole, s_cut)
    r = K.knn_sqdist(xd, xd, 2)
    assert bool((r[:, 0] == 0).all()) and bool((r[:, 1] > 0).all())                   # no row is skipped as "self"
    with pytest.raises(ValueError, match="non-finite"):
        K.kl_divergence(np.where(np.arange(n)[:, None] == 3, np.nan, x).astype(np.float32), y)
    with pytest.raises(ValueError, match="x has %d coordinates, y has %d" % (d, d + 1)):
        K.knn_sqdist(xd, torch.zeros(5, d + 1, device=DEV), 1)
