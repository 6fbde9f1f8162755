"""Posterior covariances on the device, the kernel: `engine.cov_accumulate` (csrc/mcpc_cov.h, the fp64 MFMA) against sums of outer
products formed on the host in np.longdouble from the fp32 records.

The bound, per entry, for identity blocks: |got - want| <= (R + G + 2) * 2^-52 * sum |v_i v_j| (+ 2^-52 |acc0| when accumulating), R the
rows contracted, G the pooled groups (0 per chain): the products are exact in fp64, any order of R fp64 additions errs by at most
(R - 1) * 2^-53 of the sum of magnitudes, one more rounding per group and per call, times two for the unspecified order inside an MFMA."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -52
WINDOWS = [(0, 1, 1), (0, 1, 2), (3, 2, 7), (5, 7, 8), (0, 1, 37)]
# (widths, B, floats of offset into the allocation)
SHAPES = [((1,), 1, 0), ((15,), 5, 0), ((15,), 5, 1), ((6, 16, 16), 37, 0), ((15, 1, 33), 70, 1)]


def _blocks(n_rec, B, widths, seed, rows=None, offset=0, special=False):
    """One [n_rec, B, w] fp32 buffer per width on the device, `offset` floats into its allocation; values 3 N(0,1) + 1.5.  With `rows`,
    every record NOT in it holds NaN.  Returns (device tensors, host arrays)."""
    g = torch.Generator().manual_seed(seed)
    dev, host = [], []
    for w in widths:
        h = 3.0 * torch.randn(n_rec, B, w, generator=g) + 1.5
        if special:
            vals = torch.tensor([1e18, -1e18, 1e-40, -1e-42, 1.17549435e-38, 0.0, -0.0, 1.5], dtype=torch.float32)
            h = vals[torch.randint(0, len(vals), (n_rec, B, w), generator=g)]
        if rows is not None:
            keep = torch.zeros(n_rec, dtype=torch.bool)
            keep[list(rows)] = True
            h[~keep] = float("nan")
        alloc = torch.empty(n_rec * B * w + offset, dtype=torch.float32, device=DEV)
        d = alloc[offset:].view(n_rec, B, w)
        d.copy_(h)
        assert d.is_contiguous() and d.data_ptr() == alloc.data_ptr() + 4 * offset
        dev.append(d)
        host.append(h.numpy())
    return dev, host


def _host_outer(host, rows, pool, sigmoid=None):
    """(sum of v v^T, sum of |v| |v|^T) over the rows in np.longdouble: [B, D, D], or [D, D] pooled."""
    cols = []
    for j, h in enumerate(host):
        v = h[list(rows)].astype(np.float64)
        if sigmoid is not None and sigmoid[j]:
            v = 1.0 / (1.0 + np.exp(-v))
        cols.append(v.astype(np.longdouble))
    v = np.concatenate(cols, axis=2)                                   # [n, B, D]
    a = np.abs(v)
    if pool:
        v2, a2 = v.reshape(-1, v.shape[2]), a.reshape(-1, a.shape[2])
        return v2.T @ v2, a2.T @ a2
    v, a = v.transpose(1, 0, 2), a.transpose(1, 0, 2)                  # [B, n, D]
    return np.matmul(v.transpose(0, 2, 1), v), np.matmul(a.transpose(0, 2, 1), a)


def _groups(widths, B, pool):
    """The pooled groups of a shape (0 per chain), from the size of the workspace: [groups][Dpad][Dpad] fp64."""
    from montecarlopredictivecoding_amd.engine import cov_workspace_bytes
    if not pool:
        assert cov_workspace_bytes(B, widths, pool=False) == 0
        return 0
    dpad = sum((w + 15) // 16 * 16 for w in widths)
    need = cov_workspace_bytes(B, widths)
    assert need % (8 * dpad * dpad) == 0
    return need // (8 * dpad * dpad)


def _bound(mags, n, B, widths, pool, acc0=None):
    R = n * B if pool else n
    b = (R + _groups(widths, B, pool) + 2) * EPS * mags
    if acc0 is not None:
        b = b + EPS * np.abs(acc0).astype(np.longdouble)
    return b


def _check(got_t, want, bound, what):
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.longdouble) - want)
    worst = float((err / np.maximum(bound, np.finfo(np.longdouble).tiny)).max())
    print(f"{what}: max |error| / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)
    assert np.array_equal(got.view(np.int64), np.swapaxes(got, -1, -2).copy().view(np.int64)), f"{what}: not bitwise symmetric"
    return got


def _outer_like(B, D, pool, fill):
    shape = (D, D) if pool else (B, D, D)
    g = torch.Generator().manual_seed(9)
    if fill == "garbage":
        t = torch.randn(shape, generator=g, dtype=torch.float64) * 1e9
        t.view(-1)[::3] = float("nan")
        return t
    t = torch.randn(shape, generator=g, dtype=torch.float64) * 1e3
    return t + t.transpose(-1, -2)                                     # known values: symmetric, as every result of the kernel is


def _run_case(widths, B, offset, first, stride, n, pool):
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    D = sum(widths)
    rows = [first + k * stride for k in range(n)]
    recs, host = _blocks(rows[-1] + 3, B, widths, seed=D + n, rows=rows, offset=offset)
    want, mags = _host_outer(host, rows, pool)
    # accumulate = 0 onto garbage
    out = _outer_like(B, D, pool, "garbage").to(DEV)
    cov_accumulate(recs, first, stride, n, out, pool=pool, accumulate=False)
    a = _check(out, want, _bound(mags, n, B, widths, pool), "overwrite")
    # ... and the same bits from a second run
    out2 = _outer_like(B, D, pool, "garbage").to(DEV)
    cov_accumulate(recs, first, stride, n, out2, pool=pool, accumulate=False)
    assert np.array_equal(a.view(np.int64), out2.cpu().numpy().view(np.int64)), "two runs differ"
    # accumulate = 1 onto known values
    acc0 = _outer_like(B, D, pool, "known")
    out = acc0.to(DEV)
    cov_accumulate(recs, first, stride, n, out, pool=pool, accumulate=True)
    _check(out, want + acc0.numpy().astype(np.longdouble), _bound(mags, n, B, widths, pool, acc0.numpy()), "accumulate")


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("first, stride, n", WINDOWS)
@pytest.mark.parametrize("widths, B, offset", SHAPES)
def test_kernel_against_longdouble(widths, B, offset, first, stride, n, pool):
    _run_case(widths, B, offset, first, stride, n, pool)


@pytest.mark.parametrize("pool", [False, True])
def test_more_than_one_job_per_group(pool):
    """276 columns are 18 tiles: 5 blocks of tiles, 15 jobs per chain group."""
    _run_case((20, 128, 128), 3, 0, 0, 1, 9, pool)


def test_seventy_chains_end_in_a_ragged_group():
    """Pooled groups are runs of a multiple of 4 chains: with more than one group, 70 chains leave a last group of another length."""
    assert _groups((15, 1, 33), 70, True) > 1 and 70 % 4 != 0


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("widths, B", [((6, 16, 16), 37), ((15, 1, 33), 70)])
def test_chunk_invariance_within_the_bound(widths, B, pool):
    """Records 0..36 in one call against calls of 1, 5 and 31: not bitwise (an MFMA groups four terms), both within the bound."""
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    D = sum(widths)
    recs, host = _blocks(37, B, widths, seed=11)
    want, mags = _host_outer(host, range(37), pool)
    bound = _bound(mags, 37, B, widths, pool)
    one = torch.empty(*((D, D) if pool else (B, D, D)), dtype=torch.float64, device=DEV)
    cov_accumulate(recs, 0, 1, 37, one, pool=pool, accumulate=False)
    parts = torch.zeros_like(one)
    for first, n in ((0, 1), (1, 5), (6, 31)):
        cov_accumulate(recs, first, 1, n, parts, pool=pool, accumulate=True)
    a = _check(one, want, bound, "one call")
    b = _check(parts, want, bound, "three calls")
    diff = np.abs(a.astype(np.longdouble) - b.astype(np.longdouble))
    print(f"one call against three: max |difference| / bound = {float((diff / bound).max()):.3f}")
    assert (diff <= bound).all()


@pytest.mark.parametrize("pool", [False, True])
def test_diagonal_against_moments_sumsq(pool):
    from montecarlopredictivecoding_amd.engine import cov_accumulate, moments_accumulate
    widths, B, n = (6, 16, 16), 37, 37
    D = sum(widths)
    recs, host = _blocks(n, B, widths, seed=12)
    _, mags = _host_outer(host, range(n), pool)
    out = torch.empty(*((D, D) if pool else (B, D, D)), dtype=torch.float64, device=DEV)
    cov_accumulate(recs, 0, 1, n, out, pool=pool, accumulate=False)
    sq = []
    for r, w in zip(recs, widths):
        s = torch.empty(B, w, dtype=torch.float64, device=DEV)
        q = torch.empty(B, w, dtype=torch.float64, device=DEV)
        moments_accumulate(r, 0, 1, n, s, q, accumulate=False)
        sq.append(q)
    sq = torch.cat(sq, dim=1)
    if pool:
        sq = sq.sum(0)
    diag = torch.diagonal(out, dim1=-2, dim2=-1)
    err = (diag - sq).abs().cpu().numpy().astype(np.longdouble)
    bound = np.diagonal(_bound(mags, n, B, widths, pool), axis1=-2, axis2=-1)
    print(f"diagonal against sumsq: max |difference| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("pool", [False, True])
def test_sigmoid_block(pool):
    """sigmoid_f is within 4.8e-7 of the fp64 sigmoid per sample (tests/test_gpu_moments.py: test_sigmoid_transform); the product of
    two values <= 1 is then within 1e-6, and a mean cannot be further off than one sample."""
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    B, w, n = 5, 24, 64
    g = torch.Generator().manual_seed(6)
    logits = torch.rand(n, B, w, generator=g) * 60.0 - 30.0
    rec = logits.to(DEV)
    out = torch.empty(*((w, w) if pool else (B, w, w)), dtype=torch.float64, device=DEV)
    cov_accumulate([rec], 0, 1, n, out, transforms=["sigmoid"], pool=pool, accumulate=False)
    want, _ = _host_outer([logits.numpy()], range(n), pool, sigmoid=[True])
    N = n * B if pool else n
    err = float(np.abs(out.cpu().numpy() / N - (want / N).astype(np.float64)).max())
    print(f"sigmoid block: max |mean product error| {err:.3e} (bound 1e-6)")
    assert err <= 1e-6
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.int64), np.swapaxes(got, -1, -2).copy().view(np.int64))


@pytest.mark.parametrize("pool", [False, True])
def test_mixed_transforms(pool):
    """An identity block next to a sigmoid block: the identity-identity part keeps the identity bound."""
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    widths, B, n = (6, 24), 5, 9
    recs, host = _blocks(n, B, widths, seed=14)
    out = torch.empty(*((30, 30) if pool else (B, 30, 30)), dtype=torch.float64, device=DEV)
    cov_accumulate(recs, 0, 1, n, out, transforms=["identity", "sigmoid"], pool=pool, accumulate=False)
    want, mags = _host_outer(host, range(n), pool, sigmoid=[False, True])
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.longdouble) - want)
    assert (err[..., :6, :6] <= _bound(mags, n, B, widths, pool)[..., :6, :6]).all()
    N = n * B if pool else n
    # a sigmoid value is within 4.8e-7; times an identity value of magnitude |v|
    vmax = max(float(np.abs(h).max()) for h in host)
    assert float(err.max()) / N <= 1e-6 * max(1.0, vmax)


@pytest.mark.parametrize("pool", [False, True])
def test_extreme_values_and_denormals(pool):
    widths, B, n = (15, 33), 6, 12
    rows = [1, 3, 5, 7, 9]
    recs, host = _blocks(n, B, widths, seed=3, special=True)
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    D = sum(widths)
    out = torch.empty(*((D, D) if pool else (B, D, D)), dtype=torch.float64, device=DEV)
    cov_accumulate(recs, 1, 2, 5, out, pool=pool, accumulate=False)
    want, mags = _host_outer(host, rows, pool)
    assert float(mags.max()) > 1e36 and (np.abs(np.concatenate([h.ravel() for h in host])) < 1.17549435e-38).any()
    _check(out, want, _bound(mags, 5, B, widths, pool), "extreme values")


@pytest.mark.parametrize("pool", [False, True])
def test_n_zero(pool):
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    recs, _ = _blocks(2, 3, (5, 16), seed=0)
    out = torch.full((21, 21) if pool else (3, 21, 21), 7.0, dtype=torch.float64, device=DEV)
    cov_accumulate(recs, 0, 1, 0, out, pool=pool, accumulate=True)
    assert (out == 7.0).all()
    cov_accumulate(recs, 0, 1, 0, out, pool=pool, accumulate=False)
    assert (out == 0.0).all()


def test_einval_cases():
    from montecarlopredictivecoding_amd import _lib as L
    lib = L.load()
    B = 4
    rec = [torch.zeros(4, B, 8, dtype=torch.float32, device=DEV), torch.zeros(4, B, 3, dtype=torch.float32, device=DEV)]
    out = torch.zeros(11, 11, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    PTRS = (C.c_void_p * 2)(rec[0].data_ptr(), rec[1].data_ptr())
    need = lib.mcpc_cov_workspace_bytes(B, (C.c_int32 * 2)(8, 3), 2, 1)
    assert 0 < need <= ws.numel()

    def call(ptrs=PTRS, widths=(8, 3), xf=(0, 0), n_blocks=2, first=0, stride=1, n=2, pool=1, outer=C.c_void_p(out.data_ptr()),
             wsp=C.c_void_p(ws.data_ptr()), ws_bytes=ws.numel(), b=B):
        w = None if widths is None else (C.c_int32 * len(widths))(*widths)
        x = None if xf is None else (C.c_int32 * len(xf))(*xf)
        code = lib.mcpc_cov_accumulate(0, ptrs, w, x, n_blocks, b, first, stride, n, pool, outer, 0, wsp, ws_bytes, stream)
        return code, lib.mcpc_last_error().decode()

    assert call()[0] == 0
    assert call(xf=None)[0] == 0                                  # transforms NULL: all identity
    one_null = (C.c_void_p * 2)(rec[0].data_ptr(), None)
    for kw, word in ((dict(outer=None), "outer is null"), (dict(ptrs=None), "rec is null"), (dict(ptrs=one_null), "rec[1] is null"),
                     (dict(widths=None), "widths is null"), (dict(stride=0), "stride=0"), (dict(first=-1), "first=-1"),
                     (dict(n=-1), "n=-1"), (dict(widths=(8, 0)), "widths[1]=0"), (dict(xf=(0, 2)), "unknown transform 2"),
                     (dict(n_blocks=0), "n_blocks=0"), (dict(n_blocks=L.MAX_LATENT + 2), f"n_blocks={L.MAX_LATENT + 2}"),
                     (dict(b=0), "B=0"), (dict(b=1 << 26, pool=0), "jobs"), (dict(pool=2), "pool=2"), (dict(wsp=None), "workspace is null"),
                     (dict(ws_bytes=need - 1), "too small")):
        code, msg = call(**kw)
        assert code == -1 and word in msg, (kw, code, msg)
    assert call(ptrs=None, n=0, wsp=None, ws_bytes=0)[0] == 0     # nothing is read: no records, no workspace
    per_chain = torch.zeros(B, 11, 11, dtype=torch.float64, device=DEV)
    assert call(pool=0, outer=C.c_void_p(per_chain.data_ptr()), wsp=None, ws_bytes=0)[0] == 0
    assert lib.mcpc_cov_workspace_bytes(B, (C.c_int32 * 2)(8, 0), 2, 1) == -1 and "widths[1]=0" in lib.mcpc_last_error().decode()
    assert lib.mcpc_cov_workspace_bytes(B, (C.c_int32 * 2)(8, 3), 2, 0) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()


def test_binding_checks_its_tensors():
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    rec = [torch.zeros(4, 3, 8, dtype=torch.float32, device=DEV), torch.zeros(4, 3, 5, dtype=torch.float32, device=DEV)]
    out = torch.zeros(3, 13, 13, dtype=torch.float64, device=DEV)
    cov_accumulate(rec, 0, 1, 4, out)
    with pytest.raises(ValueError, match="hold 4 records"):
        cov_accumulate(rec, 1, 2, 3, out)
    with pytest.raises(TypeError):
        cov_accumulate(rec, 0, 1, 2, out.float())
    with pytest.raises(TypeError):
        cov_accumulate(rec[0], 0, 1, 2, out)
    with pytest.raises(TypeError):
        cov_accumulate([rec[0], rec[1][0]], 0, 1, 2, out)
    with pytest.raises(ValueError, match="shape"):
        cov_accumulate(rec, 0, 1, 2, out[:, :12, :12].clone())
    with pytest.raises(ValueError, match="shape"):
        cov_accumulate(rec, 0, 1, 2, out, pool=True)
    with pytest.raises(ValueError, match="shape"):
        cov_accumulate([rec[0], rec[1][:, :2]], 0, 1, 2, out)
    with pytest.raises(ValueError, match="contiguous"):
        cov_accumulate([rec[0][:, :, ::2], rec[1]], 0, 1, 2, torch.zeros(3, 9, 9, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="device"):
        cov_accumulate(rec, 0, 1, 2, out.cpu())
    with pytest.raises(ValueError, match="transforms"):
        cov_accumulate(rec, 0, 1, 2, out, transforms=["identity"])
    with pytest.raises(ValueError, match="transforms"):
        cov_accumulate(rec, 0, 1, 2, out, transforms=["identity", "tanh"])
    with pytest.raises(ValueError, match="blocks"):
        cov_accumulate([rec[0]] * 8, 0, 1, 2, out)
    with pytest.raises(ValueError, match="workspace"):
        cov_accumulate(rec, 0, 1, 2, out[0].clone(), pool=True, workspace=torch.zeros(8, dtype=torch.uint8, device=DEV))


def test_offsets_are_64_bit():
    from montecarlopredictivecoding_amd.engine import cov_accumulate
    B, w = 16384, 64
    try:
        rec = torch.empty(2049, B, w, dtype=torch.float32, device=DEV)        # 8.6 GB; record 2048 starts at element 2^31
    except RuntimeError as exc:                                                # (torch.OutOfMemoryError is one)
        pytest.skip(f"no room for the 8.6 GB record buffer: {exc}")
    g = torch.Generator().manual_seed(4)
    rows = []
    for r in (2040, 2044, 2048):
        h = 3.0 * torch.randn(B, w, generator=g) + 1.5
        rec[r].copy_(h)
        rows.append(h.numpy().astype(np.float64))
    out = torch.empty(w, w, dtype=torch.float64, device=DEV)
    cov_accumulate([rec], 2040, 4, 3, out, pool=True, accumulate=False)
    v = np.concatenate(rows, axis=0)
    want = np.zeros((w, w), np.longdouble)
    for i in range(0, v.shape[0], 4096):
        c = v[i:i + 4096].astype(np.longdouble)
        want += c.T @ c
    mags = (np.abs(v).T @ np.abs(v)).astype(np.longdouble)             # (a magnitude for the bound: fp64 is plenty)
    _check(out, want, _bound(mags, 3, B, (w,), True), "records past 2^31 elements")
    del rec
    torch.cuda.empty_cache()
