"""GPU: blim_tvg_rank (csrc/kernels.hip: tvg_rank_kernel) alone, against the numpy statement of tests/tvg_rank_ref.py on that module's inputs.

lp (logprob_out) within the float64 statement's tolerance (printed as TVG_RANK_MEASURE), and EQUAL AS FLOATS to blim_tvg_criterion at clips = 1 for every label at
N <= 257 and for 16 labels per row above; idx / val exactly the stable argsort of the numpy-f32 term formed from the kernel's own lp rows (the prior's lp rows come
from a launch of their own); the outputs' sentinels behind the last row and in the padding columns intact; input columns past n_vocab hold NaN.  Every refusal."""
import math

import numpy as np
import pytest
import torch

import tvg_rank_ref as R
from blim_amd import engine as eng
from score_kernel_inputs import ratio

pytestmark = pytest.mark.gpu

SENT32 = 0x7E7E7E7E
f32 = np.float32
_quiet = dict(over="ignore", invalid="ignore", divide="ignore")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sent(shape, dtype=torch.float32):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(dtype)


def bits(t):
    return t.view(torch.int32).cpu().numpy()


def same_floats(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def run(logits, N, k, rows, prior=None, prior_of=None, alpha=0.0, n_prior=None, pad_out=3):
    """One launch -> (idx [rows, k], val [rows, k], lp [rows, N]); checks the sentinels."""
    idx, val = sent((rows * k + 8,), torch.int32), sent((rows * k + 8,))
    lpo = sent((rows + 1, N + pad_out))
    eng.tvg_rank(logits, N, k, idx, val, prior_logits=prior, prior_of=prior_of, alpha=alpha, logprob_out=lpo, n_rows=rows, n_prior=n_prior)
    torch.cuda.synchronize()
    assert (bits(idx)[rows * k:] == SENT32).all() and (bits(val)[rows * k:] == SENT32).all(), "idx_out / val_out written beyond n_rows * k"
    lb = bits(lpo)
    assert (lb[rows:] == SENT32).all() and (lb[:rows, N:] == SENT32).all(), "logprob_out: a padding column or a row >= n_rows was written"
    return idx.cpu().numpy()[:rows * k].reshape(rows, k), val.cpu().numpy()[:rows * k].reshape(rows, k), lpo.cpu().numpy()[:rows, :N]


@pytest.mark.parametrize("spec", R.CASES, ids=lambda s: "-".join(map(str, s)))
def test_tvg_rank(spec):
    c = R.case(spec)
    N, k, rows = c.N, c.k, c.rows
    lg = dev(c.buf)
    pl = None
    if c.prior_of is not None:
        pr = dev(c.pbuf)
        pl = run(pr, N, 1, c.n_prior)[2]                                         # the prior rows' lp, by the kernel itself
        idx, val, lp = run(lg, N, k, rows, prior=pr, prior_of=dev(c.prior_of), alpha=c.alpha)
    else:
        idx, val, lp = run(lg, N, k, rows)
    # ---- lp against float64
    fig = ratio(lp, c.ref.lp, c.ref.tol)
    print(f"TVG_RANK_MEASURE case={'-'.join(map(str, spec))} lp={fig:.4g}")
    assert math.isfinite(fig) and fig <= 1.0, (spec, fig)
    # ---- lp == blim_tvg_criterion(row r, label j, clips = 1) as floats
    labs = np.arange(N) if N <= 257 else np.unique(np.concatenate([[0, 63, 64, N - 1], np.random.RandomState(N + k).randint(0, N, 12)]))
    rep = lg[:, None, :].expand(rows, len(labs), c.ld).reshape(rows * len(labs), c.ld).contiguous()
    score = sent((rows * len(labs) + 2,))
    eng.tvg_criterion(rep, N, dev(np.tile(labs, rows).astype(np.int32)), rows * len(labs), 1, score)
    torch.cuda.synchronize()
    crit = score.cpu().numpy()[:rows * len(labs)].reshape(rows, len(labs))
    assert same_floats(crit, lp[:, labs]), "lp differs from the criterion's value for the same row and label"
    # ---- the order and the values, exactly, from the kernel's own lp
    with np.errstate(**_quiet):
        term = R.term_of(lp, pl, c.prior_of, c.n_prior, c.alpha)
        want = np.stack([np.argsort(-term[r], kind="stable")[:k] for r in range(rows)])
    assert (want == R.order(term, k)).all()
    assert (idx == want).all(), f"idx differs from the stable argsort in {int((idx != want).sum())} places"
    want_val = np.take_along_axis(term, want.astype(np.int64), 1)
    assert ((val.view(np.int32) == want_val.view(np.int32)) | (np.isnan(val) & np.isnan(want_val))).all(), "val is not term[idx] bit for bit"
    for r, fam in enumerate(c.families):
        if fam == "nan":
            assert np.isnan(lp[r]).all()
        if fam in ("nan", "equal") and (c.prior_of is None or c.prior_of[r] < 0):
            assert (idx[r] == np.arange(k)).all()
        if c.prior_of is not None and c.prior_of[r] >= c.n_prior:
            assert np.isnan(val[r]).all() and (idx[r] == np.arange(k)).all()


def test_null_prior_of_and_negative_entries_give_the_same_bits():
    c = R.case((257, 16, 3, 3, 0, 1, 0.7))
    lg, pr = dev(c.buf), dev(c.pbuf)
    a = run(lg, c.N, c.k, c.rows)
    b = run(lg, c.N, c.k, c.rows, prior=pr, prior_of=dev(np.full(c.rows, -1, np.int32)), alpha=0.7)
    z = run(lg, c.N, c.k, c.rows, prior=pr, prior_of=dev(np.zeros(c.rows, np.int32)), alpha=0.7, n_prior=0)         # n_prior = 0: every entry >= n_prior
    assert (a[0] == b[0]).all() and (a[1].view(np.int32) == b[1].view(np.int32)).all() and (a[2].view(np.int32) == b[2].view(np.int32)).all()
    assert np.isnan(z[1]).all() and (z[0] == np.arange(c.k)).all() and (a[2].view(np.int32) == z[2].view(np.int32)).all()


def test_refusals():
    """Every host refusal: BLIM_ERR_ARG, the message names the argument, nothing written."""
    N, rows, k = 70, 2, 4
    lg, pr = dev(np.zeros((rows, N + 3), f32)), dev(np.zeros((1, N + 3), f32))
    po = dev(np.zeros(rows, np.int32))
    idx, val, lpo = sent((rows * k,), torch.int32), sent((rows * k,)), sent((rows, N + 3))
    lib = eng.load_library()

    def refused(word, logits=lg, ld=N + 3, n_vocab=N, n_rows=rows, prior=None, ld_prior=0, n_prior=0, prior_of=None, k=k, idx=idx, val=val, lp=None, ld_out=0):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.blim_tvg_rank(p(logits), ld, n_vocab, n_rows, p(prior), ld_prior, n_prior, p(prior_of), 0.5, k, p(idx), p(val), p(lp), ld_out, None)
        assert rc == -1 and word in lib.blim_last_error().decode(), (word, rc, lib.blim_last_error().decode())

    refused("logits", logits=None)
    refused("idx_out", idx=None)
    refused("val_out", val=None)
    refused("n_vocab", n_vocab=0)
    refused("n_rows", n_rows=0)
    refused("k = 0", k=0)
    refused("n_vocab", k=N + 1)
    refused("BLIM_TVG_RANK_MAX_K", n_vocab=2000, ld=2000, k=1025)                  # (refused before anything is read)
    refused("ld =", ld=N - 1)
    refused("ld_prior", prior=pr, ld_prior=N - 1, n_prior=1, prior_of=po)
    refused("ld_out", lp=lpo, ld_out=N - 1)
    refused("prior_of without prior_logits", prior_of=po)
    refused("n_prior", prior=pr, ld_prior=N + 3, n_prior=-1, prior_of=po)
    torch.cuda.synchronize()
    assert (bits(idx) == SENT32).all() and (bits(val) == SENT32).all() and (bits(lpo) == SENT32).all()
