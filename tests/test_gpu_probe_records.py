"""The probe as a derived record, the kernel: `engine.probe_records` writes bitwise the link values `engine.probe_accumulate` adds.
The sum of ONE sample into a zeroed accumulator is `(double)p`, exact, so `probe_accumulate(first=k, n=1, accumulate=False)` recovers
the fp32 value the accumulating kernel formed for record k, and the two are compared bit for bit, NaNs as NaNs."""
import numpy as np
import pytest
import torch

from tests import probe_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N = 5, 11                                                                          # more than one block of 8 samples, and not a multiple
WIDTHS = (1, 5, 64, 65, 130)
LINKS = ("identity", "sigmoid", "softmax")


def _case(C, width, seed):
    rng = np.random.default_rng(seed)
    r = rng.normal(0.0, 1.0, size=(N, B, width)).astype(np.float32)
    r[2, 1, 0], r[5, 3, width - 1], r[7, 0, width // 2], r[9, 4, 0] = np.nan, np.inf, -np.inf, 3e38
    W = (rng.normal(0.0, 1.0, size=(C, width)) / np.sqrt(width)).astype(np.float32)
    bias = rng.normal(0.0, 0.5, size=(C,)).astype(np.float32)
    return r, W, bias


def _same_bits(a, b):
    """Bitwise, NaNs compared as NaNs."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _per_sample(rec, W, bias, link, C):
    """fp32 [N, B, C]: what `probe_accumulate` adds for each record on its own."""
    from montecarlopredictivecoding_amd.engine import probe_accumulate
    from montecarlopredictivecoding_amd.probe import new_state
    st = new_state(B, C, link, DEV)
    out = np.empty((rec.shape[0], B, C), dtype=np.float32)
    for k in range(rec.shape[0]):
        probe_accumulate(rec, k, 1, 1, W, bias, link, st["psum"], None, st["votes"], st["entsum"], accumulate=False)
        p64 = st["psum"].cpu().numpy()
        out[k] = p64.astype(np.float32)
        assert bool(((out[k] == p64) | np.isnan(p64)).all())                          # (double)p: the rounding back is exact
    return out


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("C", [1, 2, 3, 10, 33, 64])
def test_records_are_bitwise_what_the_accumulating_kernel_adds(C, link):
    from montecarlopredictivecoding_amd.engine import probe_records
    for width in WIDTHS:
        r, W, bias = _case(C, width, 1000 * C + width)
        rec, Wd, bd = (torch.from_numpy(a).to(DEV) for a in (r, W, bias))
        got = probe_records(rec, 0, 1, N, Wd, bd, link)
        assert tuple(got.shape) == (N, B, C) and got.dtype == torch.float32 and got.is_contiguous()
        got = got.cpu().numpy()
        assert _same_bits(got, _per_sample(rec, Wd, bd, link, C)), (C, width, link)
        v = pc.logits(r, W, bias)
        if link == "identity":
            assert _same_bits(got, v), (C, width)
        elif link == "softmax":
            clean = np.isfinite(v).all(axis=-1)                                       # a chain's special values stay in its own row
            assert clean.sum() >= N * B - 4
            p64, _ = pc.softmax64(v)
            assert np.abs(got.astype(np.float64) - p64)[clean].max() <= pc.p_bound(C), (C, width)
            assert np.isnan(got[np.isnan(v).any(axis=-1)]).all()                      # a NaN logit reaches every class of its sample
        # without a bias, through a buffer of the caller
        out = torch.full((N, B, C), 7.0, dtype=torch.float32, device=DEV)
        assert probe_records(rec, 0, 1, N, Wd, None, link, out=out) is out
        assert _same_bits(out.cpu().numpy(), _per_sample(rec, Wd, None, link, C)), (C, width, link, "no bias")


@pytest.mark.parametrize("link", LINKS)
def test_a_strided_window_lands_in_the_right_rows(link):
    from montecarlopredictivecoding_amd.engine import probe_records
    r, W, bias = _case(10, 20, 5)
    rec, Wd, bd = (torch.from_numpy(a).to(DEV) for a in (r, W, bias))
    every = probe_records(rec, 0, 1, N, Wd, bd, link).cpu().numpy()
    some = probe_records(rec, 1, 3, 4, Wd, bd, link).cpu().numpy()                    # records 1, 4, 7, 10
    assert some.shape == (4, B, 10) and _same_bits(some, every[1:11:3])
    assert tuple(probe_records(rec, 0, 1, 0, Wd, bd, link).shape) == (0, B, 10)       # no sample: nothing is launched


def test_many_samples_are_dealt_out_over_workgroups_alike():
    """Enough samples for several blocks per workgroup row (gridDim.y below the blocks): the same bits as in pieces."""
    from montecarlopredictivecoding_amd.engine import probe_records
    rng = np.random.default_rng(9)
    n = 8 * 300 + 3
    rec = torch.from_numpy(rng.normal(0, 1, size=(n, 2048, 2)).astype(np.float32)).to(DEV)   # 64 chain groups: 64 rows of 300 blocks
    W = torch.from_numpy(rng.normal(0, 1, size=(2, 2)).astype(np.float32)).to(DEV)
    whole = probe_records(rec, 0, 1, n, W, None, "softmax")
    parts = torch.cat([probe_records(rec, k0, 1, min(701, n - k0), W, None, "softmax") for k0 in range(0, n, 701)])
    assert torch.equal(whole, parts)
    v = pc.logits(rec[-3:].cpu().numpy(), W.cpu().numpy())
    assert np.abs(whole[-3:].cpu().numpy() - pc.softmax64(v)[0]).max() <= pc.p_bound(2)


def test_the_wrapper_checks_its_tensors():
    from montecarlopredictivecoding_amd.engine import probe_records
    rec, W = torch.zeros(4, 3, 5, device=DEV), torch.zeros(2, 5, device=DEV)
    with pytest.raises(ValueError, match="link"):
        probe_records(rec, 0, 1, 4, W, None, "tanh")
    with pytest.raises(ValueError, match="W: expected shape"):
        probe_records(rec, 0, 1, 4, torch.zeros(2, 4, device=DEV), None, "softmax")
    with pytest.raises(ValueError, match="out: expected shape"):
        probe_records(rec, 0, 1, 4, W, None, "softmax", out=torch.zeros(3, 3, 2, device=DEV))
    with pytest.raises(ValueError, match="last one asked for is 4"):
        probe_records(rec, 0, 1, 5, W, None, "softmax")
