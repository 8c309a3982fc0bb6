"""GPU: blim_tvg_cols (csrc/kernels.hip: tvg_cols_kernel) alone, on host-made f32 rows of tests/tvg_rank_ref.py's families.

out[c][out0 + r] is BIT-equal to blim_tvg_criterion of row r with label cols[c] at clips = 1 and to column cols[c] of blim_tvg_rank's logprob_out row r, on the same
device (the three kernels form one normaliser: one wave through rank_lse), and within the float64 statement's tolerance of tvg_rank_ref.log_softmax_rows (printed
as TVG_COLS_MEASURE).  cols repeat; an entry of -1 and one of n_vocab store NaN.  The logits' padding columns hold NaN and are never read; every cell of out that
the call does not own keeps its sentinel.  Every refusal.

Shapes: n_vocab 1 / 2 the smallest, 63 / 64 / 65 around one lane-strided step of the normaliser's wave, 255 / 257 around one step of a workgroup, 1000 the
measured gallery; n_cols 70 is more than one wave of stores; rows, the padding, n_cols, out0 and the families rotate over the list."""
import math
import zlib

import numpy as np
import pytest
import torch

import tvg_rank_ref as R
from blim_amd import engine as eng
from score_kernel_inputs import ratio

pytestmark = pytest.mark.gpu

SENT32 = 0x7E7E7E7E
f32 = np.float32
FAMILIES = ("gauss1", "gauss30", "equal", "neginf", "nan")
NS = (1, 2, 63, 64, 65, 255, 257, 1000)
CASES = [(N, (1, 3, 5)[i % 3], (0, 3)[i % 2], (1, 3, 70)[(i // 2) % 3], (0, 7)[(i // 3) % 2], (n * 6 + i) % 5) for n, N in enumerate(NS) for i in range(6)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sent(shape, dtype=torch.float32):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(dtype)


def bits(t):
    return t.view(torch.int32).cpu().numpy()


def _inputs(spec):
    N, rows, pad, n_cols, out0, fam0 = spec
    rs = np.random.RandomState(zlib.crc32(repr(spec).encode()) & 0x7FFFFFFF)
    buf = np.full((rows, N + pad), np.nan, f32)                                    # columns [N, ld) are never read
    fams = [FAMILIES[(fam0 + i) % 5] for i in range(rows)]
    for i, fam in enumerate(fams):
        buf[i, :N] = R._row(rs, N, 1, fam)
    cols = rs.randint(0, N, n_cols).astype(np.int32)
    if n_cols == 70:
        cols[2], cols[69] = cols[0], cols[0]                                       # repeats, in two waves of stores
        cols[1], cols[64] = -1, N                                                  # one entry below the row, one past it
    elif n_cols == 3:                                                              # [x, -1, N], or a repeat and one of the two
        cols[1:] = (-1, N) if fam0 % 2 else (cols[0], (-1, N)[(fam0 // 2) % 2])
    elif fam0 % 3:
        cols[0] = (-1, N)[fam0 % 2]                                                # the single column of some cases lies outside
    return buf, fams, cols


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(map(str, s)))
def test_tvg_cols(spec):
    N, rows, pad, n_cols, out0, _ = spec
    buf, fams, cols = _inputs(spec)
    lg = dev(buf)
    ld_out = out0 + rows + 5
    out = sent((n_cols + 2, ld_out))
    eng.tvg_cols(lg, N, dev(cols), out, out0=out0, n_rows=rows, n_cols=n_cols)
    # the two kernels the value is defined by, on the same device
    idx, val, lpo = sent((rows,), torch.int32), sent((rows,)), sent((rows, N))
    eng.tvg_rank(lg, N, 1, idx, val, logprob_out=lpo, n_rows=rows)
    inside = (cols >= 0) & (cols < N)
    labs = cols[inside]
    crit = None
    if len(labs):
        rep = lg[:, None, :].expand(rows, len(labs), N + pad).reshape(rows * len(labs), N + pad).contiguous()
        score = sent((rows * len(labs),))
        eng.tvg_criterion(rep, N, dev(np.tile(labs, rows).astype(np.int32)), rows * len(labs), 1, score)
        crit = bits(score).reshape(rows, len(labs))
    torch.cuda.synchronize()
    ob = bits(out)
    own = np.zeros(ob.shape, bool)
    own[:n_cols, out0:out0 + rows] = True
    assert (ob[~own] == SENT32).all(), "a cell outside rows < n_cols, columns out0 .. out0 + n_rows - 1 was written"
    got = out.cpu().numpy()[:n_cols, out0:out0 + rows]                             # [n_cols, rows]
    gb = ob[:n_cols, out0:out0 + rows]
    assert np.isnan(got[~inside]).all() and ((gb[~inside] & 0x7FFFFFFF) == 0x7FC00000).all(), "a column outside 0 .. n_vocab - 1 must store a quiet NaN"
    if len(labs):
        lp_bits = bits(lpo)[:, labs].T
        print(f"TVG_COLS_MEASURE case={'-'.join(map(str, spec))} vs_rank={int((gb[inside] != lp_bits).sum())} vs_criterion={int((gb[inside] != crit.T).sum())}")
        assert (gb[inside] == lp_bits).all(), "differs from blim_tvg_rank's logprob_out column"
        assert (gb[inside] == crit.T).all(), "differs from blim_tvg_criterion at clips = 1"
        ref, tol = R.log_softmax_rows(buf[:, :N].astype(np.float64))
        fig = ratio(got[inside], ref[:, labs].T, tol[:, labs].T)
        print(f"TVG_COLS_MEASURE case={'-'.join(map(str, spec))} lp={fig:.4g}")
        assert math.isfinite(fig) and fig <= 1.0, (spec, fig)
        for r, fam in enumerate(fams):
            if fam == "nan":
                assert np.isnan(got[inside][:, r]).all()


def test_refusals():
    """Every host refusal: BLIM_ERR_ARG, the message names the argument, nothing written."""
    N, rows, n_cols = 70, 2, 3
    lg, cols, out = dev(np.zeros((rows, N + 3), f32)), dev(np.zeros(n_cols, np.int32)), sent((n_cols, 16))
    lib = eng.load_library()

    def refused(word, logits=lg, ld=N + 3, n_vocab=N, n_rows=rows, cols=cols, n_cols=n_cols, out=out, ld_out=16, out0=0):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.blim_tvg_cols(p(logits), ld, n_vocab, n_rows, p(cols), n_cols, p(out), ld_out, out0, None)
        assert rc == -1 and word in lib.blim_last_error().decode(), (word, rc, lib.blim_last_error().decode())

    refused("logits is null", logits=None)
    refused("cols is null", cols=None)
    refused("out is null", out=None)
    refused("n_vocab = 0", n_vocab=0)
    refused("n_rows = 0", n_rows=0)
    refused("n_cols = 0", n_cols=0)
    refused("ld =", ld=N - 1)
    refused("out0 = -1", out0=-1)
    refused("ld_out", ld_out=rows - 1)
    refused("ld_out", ld_out=16, out0=15)
    torch.cuda.synchronize()
    assert (bits(out) == SENT32).all()
