"""CPU (-m "not gpu"): tests/tvg_rank_within_ref.py -- the numpy statement of blim_tvg_rank_within's rule -- pinned on hand-made rows, its case list against what the
kernel distinguishes, and the wrong rules: each must change an index or a value's bits on at least one of the GPU test's inputs, which compares both exactly."""
import types

import numpy as np
import pytest

import tvg_rank_ref as R
import tvg_rank_within_ref as W

f32 = np.float32


def hand(buf, within, off, k, row_of=None, prior_of=None, pbuf=None, alpha=0.0):
    buf = np.asarray(buf, f32)
    c = types.SimpleNamespace(buf=buf, N=buf.shape[1], k=k, rows=buf.shape[0], ld=buf.shape[1], alpha=alpha, n_prior=0, prior_of=None, pbuf=None, ldp=0,
                              n_q=len(off) - 1, within=np.asarray(within, np.int32), within_off=np.asarray(off, np.int32), n_within=len(within),
                              row_of=None if row_of is None else np.asarray(row_of, np.int32))
    if pbuf is not None:
        c.pbuf, c.n_prior, c.ldp, c.prior_of = np.asarray(pbuf, f32), len(pbuf), buf.shape[1], np.asarray(prior_of, np.int32)
    return c


def test_hand_made_rows():
    # one row, log-probabilities ln(1/2), ln(1/4), ln(1/8), ln(1/8) exactly: logits = their logs, the normaliser is 0
    row = np.log(np.array([[0.5, 0.25, 0.125, 0.125]]))
    lp = R.log_softmax_rows(row.astype(f32))[0].astype(f32)                                   # (= the logits to within an ulp)
    assert np.allclose(lp, row, rtol=0, atol=1e-6)
    c = hand(row, [3, 1, 2, 1, 0, 7, -1], [0, 4, 4, 7, 7], 3, row_of=[0, 0, 0, 5])
    got = W.rank_within(c)
    assert same(got.val[0], lp[0, [1, 1, 3]]) and (got.idx[0] == [1, 3, 0]).all()         # entries 3 1 2 1: column 1 twice, the lower position first; then the tie 3 / 2
    assert (got.idx[1] == -1).all() and np.isnan(got.val[1]).all()                          # an empty list
    assert (got.idx[2] == [0, 1, 2]).all() and same(got.val[2], [lp[0, 0], np.nan, np.nan])  # entries 0 7 -1: the two bad entries NaN, last and by position
    assert (got.idx[3] == -1).all()                                                          # off[3] == off[4]: empty, whatever its row
    # the value is the whole row's: a list that leaves column 0 out still sees ln(1/4), not the subset's ln(1/2)
    c = hand(row, [1, 2, 3], [0, 3], 2)
    got = W.rank_within(c)
    assert (got.idx[0] == [0, 1]).all() and same(got.val[0], lp[0, [1, 2]])
    sub = W.rank_within(c, "subset_norm").val[0]
    assert same(sub, R.log_softmax_rows(row.astype(f32)[:, 1:])[0].astype(f32)[0, :2]) and np.allclose(sub, np.log([0.5, 0.25]), rtol=0, atol=1e-6)
    # a row outside the rows: NaN terms in position order; k above the list's length: -1 / NaN behind it
    c = hand(row, [1, 2, 3], [0, 3], 5, row_of=[1])
    got = W.rank_within(c)
    assert (got.idx[0] == [0, 1, 2, -1, -1]).all() and np.isnan(got.val[0]).all()
    # offsets: negative and beyond n_within are clamped, a decreasing pair is empty
    c = hand(row, [0, 1, 2], [-5, 2, 1, 99], 3, row_of=[0, 0, 0])
    got = W.rank_within(c)
    assert (got.idx == [[0, 1, -1], [-1, -1, -1], [0, 1, -1]]).all() and same(got.val[2], [lp[0, 1], lp[0, 2], np.nan])
    # the prior: term = lp - alpha * pl in f32, per query
    pr = np.log(np.array([[0.125, 0.125, 0.25, 0.5]]))
    c = hand(row, [0, 1, 2, 3] * 2, [0, 4, 8], 4, row_of=[0, 0], prior_of=[0, -1], pbuf=pr, alpha=1.0)
    got = W.rank_within(c)
    want = (lp[0] - R.log_softmax_rows(pr.astype(f32))[0].astype(f32)[0]).astype(f32)
    assert np.allclose(want, np.log([4, 2, 0.5, 0.25]), rtol=0, atol=1e-6)
    assert (got.idx[0] == [0, 1, 2, 3]).all() and same(got.val[0], want) and (got.idx[1] == [0, 1, 2, 3]).all() and same(got.val[1], lp[0])


def same(a, b):
    return W.same_bits(np.asarray(a, f32), np.asarray(b, f32))


def test_the_case_list_covers_what_the_kernel_distinguishes():
    cs = [W.case(s) for s in W.CASES]
    assert {c.N for c in cs} == set(W.NS)
    for N in W.NS:
        assert {c.ld - c.N for c in cs if c.N == N} == {0, 3}
    assert {c.k for c in cs} == set(W.KS) and {c.alpha for c in cs} == {0.0, 0.7}
    assert {c.k for c in cs if c.N == 4099} >= {64, 1024} or {c.k for c in cs if c.N == 1000} >= {64, 1024}
    assert {f for c in cs for f in c.families} >= {"equal", "dups", "neginf", "nan"}
    assert {(c.prior_of is None, c.ldp - c.N if c.prior_of is not None else 0) for c in cs} == {(True, 0), (False, 0), (False, 5)}
    assert any(c.row_of is None for c in cs) and any(c.row_of is not None and (c.row_of >= c.rows).any() for c in cs) and any(
        c.row_of is not None and (c.row_of < 0).any() for c in cs)
    for c in cs:
        lens = [len(l) for _, l in W.lists_of(c)]
        assert set(lens) >= {0, 1, 63, 64, 65, 255, 256, 257, 1024, 1025, c.N, c.k}
        assert any(m < c.k for m in lens) and any(m == c.k for m in lens)
        for bad in (-1, c.N, 2 ** 31 - 1):
            assert (c.within == bad).any()
        d = np.diff(c.within_off.astype(np.int64))
        assert (d < 0).any() and (c.within_off > c.n_within).any() and c.within_off[0] < 0
        if c.row_of is not None:                        # two and three (and more) queries on one row with different lists
            assert np.bincount(c.row_of[(c.row_of >= 0) & (c.row_of < c.rows)]).min() >= 3
    assert any(c.k < m for c in cs for m in c.ms)
    # a list with a repeated entry among its first k places, and a term list that holds NaN beside finite values
    assert any(len(np.unique(c.within[:64])) < 64 for c in cs)
    assert any(np.isnan(t).any() and np.isfinite(t).any() for c in cs for t in c.ref.terms)


@pytest.mark.parametrize("spec", W.CASES, ids=lambda s: "-".join(map(str, s)))
def test_statement_equals_the_unfiltered_order_filtered(spec):
    """A query's answer is the whole row's stable order, every column's positions in the list taken in list order, then the bad entries by position."""
    c = W.case(spec)
    full = R.rank(types.SimpleNamespace(N=c.N, k=c.N, rows=c.rows, ld=c.ld, buf=c.buf, alpha=c.alpha, n_prior=c.n_prior, pbuf=c.pbuf, ldp=c.ldp,
                                        prior_of=None if c.prior_of is None else np.full(c.rows, -1, np.int32)))
    for q, (r, lst) in enumerate(W.lists_of(c)):
        m, kk = len(lst), min(c.k, len(lst))
        assert (c.ref.idx[q, kk:] == -1).all() and np.isnan(c.ref.val[q, kk:]).all()
        if not m:
            continue
        assert same(c.ref.val[q, :kk], c.ref.terms[q][c.ref.idx[q, :kk]])
        if r is None:
            assert (c.ref.idx[q, :kk] == np.arange(kk)).all() and np.isnan(c.ref.val[q, :kk]).all()
        elif c.prior_of is None or c.prior_of[q] < 0:
            ok = (lst >= 0) & (lst < c.N)
            nan_col = np.isnan(full.term[r])
            pos = [p for j in full.idx[r] if not nan_col[j] for p in np.flatnonzero(lst == j)]
            pos += [p for p in range(m) if not ok[p] or nan_col[lst[p]]]
            # columns with equal terms interleave by position, so compare where the whole row's terms are distinct
            t = c.ref.terms[q]
            fin = t[~np.isnan(t)]
            if len(np.unique(fin)) == len(np.unique(lst[ok & ~np.isnan(t)])):
                assert (c.ref.idx[q, :kk] == pos[:kk]).all()


@pytest.mark.parametrize("rule", W.RULES)
def test_wrong_rules_are_told_apart(rule):
    seen = 0
    for spec in W.CASES:
        c = W.case(spec)
        w = W.rank_within(c, rule)
        seen += bool((w.idx != c.ref.idx).any() or not W.same_bits(w.val, c.ref.val))
    assert seen, rule
