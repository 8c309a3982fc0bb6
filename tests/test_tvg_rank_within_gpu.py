"""GPU: blim_tvg_rank_within (csrc/kernels.hip: tvg_rank_within_kernel) alone, against the numpy statement of tests/tvg_rank_within_ref.py on that module's inputs.

No tolerance: lp is blim_tvg_rank's logprob_out for the same rows on the same device (the prior's from a launch of its own), the term is formed in numpy f32 as
tvg_rank_ref.term_of forms it, idx must be equal exactly and val bit for bit (NaN places compared as NaN); the canaries around idx_out / val_out stay untouched.
With within = arange(N) and the identity row_of the outputs are blim_tvg_rank's.  Every host refusal."""
import numpy as np
import pytest
import torch

import tvg_rank_within_ref as W
from blim_amd import engine as eng

pytestmark = pytest.mark.gpu

SENT32 = 0x7E7E7E7E
PRE = 8
f32 = np.float32


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sent(shape, dtype=torch.float32):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(dtype)


def bits(t):
    return t.view(torch.int32).cpu().numpy()


def lp_of(buf, N):
    """The rows' lp by blim_tvg_rank itself."""
    rows = buf.shape[0]
    idx, val, lpo = sent((rows,), torch.int32), sent((rows,)), sent((rows, N))
    eng.tvg_rank(buf, N, 1, idx, val, logprob_out=lpo, n_rows=rows)
    torch.cuda.synchronize()
    return lpo.cpu().numpy()


def run(lg, N, k, within, off, row_of=None, prior=None, prior_of=None, alpha=0.0, n_rows=None, n_prior=None):
    """One launch -> (idx [n_q, k], val [n_q, k]); checks the canaries on both sides of both outputs."""
    n_q = len(off) - 1
    idx, val = sent((PRE + n_q * k + 8,), torch.int32), sent((PRE + n_q * k + 8,))
    wd = dev(np.concatenate([within, np.zeros(1, np.int32)]))                    # (never an empty tensor: a null pointer is a refusal)
    eng.tvg_rank_within(lg, N, k, wd, dev(off), idx[PRE:], val[PRE:], row_of=dev(row_of), prior_logits=prior, prior_of=dev(prior_of), alpha=alpha, n_rows=n_rows,
                        n_prior=n_prior, n_within=len(within))
    torch.cuda.synchronize()
    for o in (idx, val):
        b = bits(o)
        assert (b[:PRE] == SENT32).all() and (b[PRE + n_q * k:] == SENT32).all(), "idx_out / val_out written outside [n_q, k]"
    return idx.cpu().numpy()[PRE:PRE + n_q * k].reshape(n_q, k), val.cpu().numpy()[PRE:PRE + n_q * k].reshape(n_q, k)


@pytest.mark.parametrize("spec", W.CASES, ids=lambda s: "-".join(map(str, s)))
def test_tvg_rank_within(spec):
    c = W.case(spec)
    lg, pr = dev(c.buf), dev(c.pbuf)
    lp = lp_of(lg, c.N)
    pl = None if pr is None else lp_of(pr, c.N)
    idx, val = run(lg, c.N, c.k, c.within, c.within_off, row_of=c.row_of, prior=pr, prior_of=c.prior_of, alpha=c.alpha)
    want_idx, want_val, _ = W.expect(c, lp, pl)
    assert (idx == want_idx).all(), f"idx differs in {int((idx != want_idx).sum())} places"
    assert W.same_bits(val, want_val), "val is not the term bit for bit"
    for q, (r, lst) in enumerate(W.lists_of(c)):
        kk = min(c.k, len(lst))
        assert (idx[q, kk:] == -1).all() and (val[q, kk:].view(np.int32) == 0x7FC00000).all()
        if r is None:
            assert (idx[q, :kk] == np.arange(kk)).all() and np.isnan(val[q, :kk]).all()


@pytest.mark.parametrize("N,k,pad,prior", [(1, 1, 0, False), (65, 16, 3, True), (257, 64, 0, True), (1000, 1000, 3, False), (4099, 1024, 3, True)])
def test_whole_vocabulary_equals_tvg_rank(N, k, pad, prior):
    rs = np.random.RandomState(N)
    rows = 3
    buf = np.full((rows, N + pad), np.nan, f32)
    buf[:, :N] = rs.standard_normal((rows, N))
    buf[1, :N] = np.round(buf[1, :N] * 4) / 4                                   # ties
    lg = dev(buf)
    pr = po = None
    if prior:
        pr = dev(rs.standard_normal((2, N + pad)).astype(f32))
        po = np.array([1, -1, 0], np.int32)
    a_idx, a_val = sent((rows * k,), torch.int32), sent((rows * k,))
    eng.tvg_rank(lg, N, k, a_idx, a_val, prior_logits=pr, prior_of=dev(po), alpha=0.7)
    within = np.tile(np.arange(N, dtype=np.int32), rows)
    off = (np.arange(rows + 1) * N).astype(np.int32)
    for row_of in (None, np.arange(rows, dtype=np.int32)):
        idx, val = run(lg, N, k, within, off, row_of=row_of, prior=pr, prior_of=po, alpha=0.7)
        assert (idx == a_idx.cpu().numpy().reshape(rows, k)).all() and (val.view(np.int32) == bits(a_val).reshape(rows, k)).all()


def test_refusals():
    """Every host refusal: BLIM_ERR_ARG, the message names the argument, nothing written."""
    N, rows, k, n_q, n_w = 70, 2, 4, 3, 9
    lg, pr = dev(np.zeros((rows, N + 3), f32)), dev(np.zeros((1, N + 3), f32))
    po, ro = dev(np.zeros(n_q, np.int32)), dev(np.zeros(n_q, np.int32))
    wi, wo = dev(np.zeros(n_w, np.int32)), dev(np.array([0, 3, 6, 9], np.int32))
    idx, val = sent((n_q * k,), torch.int32), sent((n_q * k,))
    lib = eng.load_library()

    def refused(word, logits=lg, ld=N + 3, n_vocab=N, n_rows=rows, prior=None, ld_prior=0, n_prior=0, n_q=n_q, row_of=ro, prior_of=None, within=wi, within_off=wo,
                n_within=n_w, k=k, idx=idx, val=val):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.blim_tvg_rank_within(p(logits), ld, n_vocab, n_rows, p(prior), ld_prior, n_prior, n_q, p(row_of), p(prior_of), p(within), p(within_off), n_within,
                                      0.5, k, p(idx), p(val), None)
        assert rc == -1 and word in lib.blim_last_error().decode(), (word, rc, lib.blim_last_error().decode())

    refused("logits", logits=None)
    refused("within is null", within=None)
    refused("within_off", within_off=None)
    refused("idx_out", idx=None)
    refused("val_out", val=None)
    refused("n_vocab", n_vocab=0)
    refused("n_rows", n_rows=0)
    refused("n_q", n_q=0)
    refused("n_within", n_within=-1)
    refused("k = 0", k=0)
    refused("BLIM_TVG_RANK_MAX_K", k=1025)
    refused("ld =", ld=N - 1)
    refused("ld_prior", prior=pr, ld_prior=N - 1, n_prior=1, prior_of=po)
    refused("prior_of without prior_logits", prior_of=po)
    refused("n_prior", prior=pr, ld_prior=N + 3, n_prior=-1, prior_of=po)
    torch.cuda.synchronize()
    assert (bits(idx) == SENT32).all() and (bits(val) == SENT32).all()
    # k above every list's length is no error
    assert lib.blim_tvg_rank_within(lg.data_ptr(), N + 3, N, rows, None, 0, 0, n_q, ro.data_ptr(), None, wi.data_ptr(), wo.data_ptr(), n_w, 0.0, k, idx.data_ptr(),
                                    val.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy().reshape(n_q, k)[:, 3] == -1).all()
