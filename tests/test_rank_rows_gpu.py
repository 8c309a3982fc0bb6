"""GPU: blim_rank_rows (csrc/kernels.hip: rank_rows -- tvg_rank_kernel's select and sort over GIVEN values) against tests/tvg_rank_ref.py's order on those values.

idx exactly the first k of the columns by (is NaN, -value, index) -- descending, ties to the lower index, -0 = +0, -inf after every finite value, NaN last and by
index among themselves --, val the chosen inputs' own bits (a -0 stays -0, a NaN keeps its payload), a second launch the same bits, nothing written behind
n_rows * k, the padding columns (NaN) never ranked.  Every refusal, k's in blim_tvg_rank's words.

n: 1 / 2 the smallest; 255 / 256 / 257 around one step of the workgroup; 1000 (k = 1000: the sort padded to 1024); 4099 odd, the smallest with k = 1024.  Every
case ranks five rows, one per family: equal, dups (the values of ranks k - 3 .. k + 3 made one value), zeros (+0 and -0 mixed among few distinct values), inf
(+inf, -inf and finite values) and nan (several NaNs of different payloads, both signs)."""
import zlib

import numpy as np
import pytest
import torch

import tvg_rank_ref as R
from blim_amd import engine as eng

pytestmark = pytest.mark.gpu

SENT32 = 0x7E7E7E7E
f32 = np.float32
NS = (1, 2, 255, 256, 257, 1000, 4099)
KS = (1, 2, 16, 1024)
CASES = [(n, k) for n in NS for k in sorted({k for k in KS + (n,) if k <= min(n, 1024)})]
FAMILIES = ("equal", "dups", "zeros", "inf", "nan")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sent(shape, dtype=torch.float32):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(dtype)


def bits(t):
    return t.view(torch.int32).cpu().numpy()


def _row(rs, n, k, family):
    if family in ("equal", "dups"):
        return R._row(rs, n, k, family)
    x = rs.standard_normal(n).astype(f32)
    if family == "zeros":
        x = np.round(x).astype(f32)                                               # few distinct values: long runs of ties
        z = x == 0
        x[z] = np.where(rs.rand(int(z.sum())) < 0.5, f32(0.0), f32(-0.0))
        x[rs.randint(n)] = f32(-0.0)
    if family == "inf":
        x[rs.choice(n, max(1, n // 4), replace=False)] = -np.inf
        x[rs.choice(n, max(1, n // 8), replace=False)] = np.inf
    if family == "nan":
        at = rs.choice(n, max(1, n // 5), replace=False)
        x.view(np.uint32)[at] = (0x7FC00000 | rs.randint(0, 1 << 22, len(at)) | (rs.randint(0, 2, len(at)).astype(np.int64) << 31)).astype(np.uint32)
        if n > 2:
            x[rs.choice(n, 2, replace=False)] = (np.inf, -np.inf)
    return x


def run(values, n, k, rows):
    idx, val = sent((rows * k + 8,), torch.int32), sent((rows * k + 8,))
    eng.rank_rows(values, n, k, idx, val, n_rows=rows)
    torch.cuda.synchronize()
    ib, vb = bits(idx), bits(val)
    assert (ib[rows * k:] == SENT32).all() and (vb[rows * k:] == SENT32).all(), "idx_out / val_out written beyond n_rows * k"
    return ib[:rows * k].reshape(rows, k), vb[:rows * k].reshape(rows, k)


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(map(str, s)))
def test_rank_rows(spec):
    n, k = spec
    rs = np.random.RandomState(zlib.crc32(repr(spec).encode()) & 0x7FFFFFFF)
    rows = len(FAMILIES)
    buf = np.full((rows, n + 3), np.nan, f32)                                      # ld = n + 3: the padding is never ranked
    for r, fam in enumerate(FAMILIES):
        buf[r, :n] = _row(rs, n, k, fam)
    values = dev(buf)
    idx, val = run(values, n, k, rows)
    want = R.order(buf[:, :n], k)
    assert (want == np.stack([np.lexsort((np.arange(n), np.where(np.isnan(row), f32(0), -row), np.isnan(row)))[:k] for row in buf[:, :n]])).all()
    bad = idx != want
    assert not bad.any(), f"idx differs from the order in {int(bad.sum())} places, rows {sorted(set(np.nonzero(bad)[0].tolist()))} of {FAMILIES}"
    want_bits = np.take_along_axis(buf[:, :n].view(np.int32), want.astype(np.int64), 1)
    assert (val == want_bits).all(), "val does not hold the input's own bits"
    idx2, val2 = run(values, n, k, rows)
    assert (idx2 == idx).all() and (val2 == val).all(), "a second launch gave other bits"
    assert (idx[0] == np.arange(k)).all()                                          # equal: by index


def test_one_row_alone_equals_the_row_among_others():
    n, k = 1000, 16
    rs = np.random.RandomState(3)
    buf = np.stack([_row(rs, n, k, fam) for fam in FAMILIES])
    whole = run(dev(buf), n, k, len(FAMILIES))
    for r in range(len(FAMILIES)):
        one = run(dev(buf[r:r + 1]), n, k, 1)
        assert (one[0][0] == whole[0][r]).all() and (one[1][0] == whole[1][r]).all()


def test_refusals():
    """Every host refusal: BLIM_ERR_ARG, the message names the argument (k's in blim_tvg_rank's words), nothing written."""
    n, rows, k = 70, 2, 4
    vals = dev(np.zeros((rows, n + 3), f32))
    idx, val = sent((rows * k,), torch.int32), sent((rows * k,))
    lib = eng.load_library()

    def refused(word, values=vals, ld=n + 3, n=n, n_rows=rows, k=k, idx=idx, val=val):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.blim_rank_rows(p(values), ld, n, n_rows, k, p(idx), p(val), None)
        assert rc == -1 and word in lib.blim_last_error().decode(), (word, rc, lib.blim_last_error().decode())

    refused("values is null", values=None)
    refused("idx_out is null", idx=None)
    refused("val_out is null", val=None)
    refused("n = 0", n=0)
    refused("n_rows = 0", n_rows=0)
    refused("tvg_rank: k = 0 outside 1 .. n_vocab", k=0)
    refused(f"tvg_rank: k = {n + 1} outside 1 .. n_vocab = {n}", k=n + 1)
    refused("tvg_rank: k = 1025 above BLIM_TVG_RANK_MAX_K", n=2000, ld=2000, k=1025)   # (refused before anything is read)
    refused("ld =", ld=n - 1)
    torch.cuda.synchronize()
    assert (bits(idx) == SENT32).all() and (bits(val) == SENT32).all()
