"""CPU (-m "not gpu"): tests/tvg_rank_ref.py -- the numpy statement of blim_tvg_rank's rule -- pinned against np.argsort and a plain float64 log-softmax on the inputs
of tests/test_tvg_rank_gpu.py, its tolerance against oracle/score_kernels_ref.py's, and the wrong rules: each must change an index list or move lp by more than
ten tolerances on at least one of those inputs, so that the GPU test would see it.  One rule cannot do either: a prior without its normaliser shifts a row's terms
by one constant, which no order can show; it must change the VALUES beside the indices, which the GPU test compares bit for bit."""
import numpy as np
import pytest

import tvg_rank_ref as R
from oracle import score_kernels_ref as S

f32 = np.float32
_quiet = dict(over="ignore", invalid="ignore", divide="ignore")


def test_the_case_list_covers_what_the_kernel_distinguishes():
    ns = {c[0] for c in R.CASES}
    assert ns == set(R.NS)
    for N in R.NS:
        assert {c[1] for c in R.CASES if c[0] == N} == {k for k in R.KS + (N,) if k <= min(N, 1024)}
    cs = [R.case(s) for s in R.CASES]
    assert {c.rows for c in cs} == {1, 3, 5} and {c.ld - c.N for c in cs} == {0, 3} and {c.alpha for c in cs} == {0.0, 0.7}
    fams = {f for c in cs for f in c.families}
    assert fams == set(R.FAMILIES)
    po = np.concatenate([c.prior_of for c in cs if c.prior_of is not None])
    assert (po == -1).any() and (po >= 2).any() and (po == 0).any() and (po == 1).any() and any(c.prior_of is None for c in cs)
    assert any(c.ldp > c.N for c in cs if c.prior_of is not None)
    # a term row that holds NaN beside finite values (NaN last is then a rule the inputs can see), and one with a tie across the k-th place
    assert any(np.isnan(t).any() and np.isfinite(t).any() for c in cs for t in c.ref.term)
    tie = False
    for c in cs:
        for r in range(c.rows):
            t = c.ref.term[r]
            if c.k < c.N and not np.isnan(t).any():
                s = np.sort(-t, kind="stable")
                tie |= bool(s[c.k - 1] == s[c.k])
    assert tie


@pytest.mark.parametrize("spec", R.CASES, ids=lambda s: "-".join(map(str, s)))
def test_statement_equals_argsort_and_plain_log_softmax(spec):
    c = R.case(spec)
    ref = c.ref
    with np.errstate(**_quiet):
        want = np.stack([np.argsort(-ref.term[r], kind="stable")[:c.k] for r in range(c.rows)])
        assert (ref.idx == want).all()
        x = c.buf[:, :c.N].astype(np.float64)
        mx = x.max(1, keepdims=True)
        plain = x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))
    assert np.array_equal(np.isnan(plain), np.isnan(ref.lp))
    ok = ~np.isnan(plain)
    assert (plain[ok] == ref.lp[ok]).all()
    assert np.isnan(ref.lp[[f == "nan" for f in c.families]]).all()                     # one NaN in a row: every lp of the row is NaN
    for r in range(c.rows):                                                                # ... and the order is then 0 .. k - 1, as for an all-equal row
        if c.families[r] in ("nan", "equal") and (c.prior_of is None or c.prior_of[r] < 0):
            assert (ref.idx[r] == np.arange(c.k)).all()


def test_the_tolerance_is_the_criterions_row_bound():
    """Twice _log_softmax_label's bound at depth ceil(N / 64) + 6, for every label; S.tvg_criterion(clips = 1) states the same value with a wider bound (its mean)."""
    for spec in R.CASES:
        c = R.case(spec)
        fin = [r for r in range(c.rows) if np.isfinite(c.buf[r, :c.N]).all()]
        if not fin or c.N > 4099:
            continue
        lg = c.buf[fin][:, :c.N].astype(np.float64)
        labs = np.unique(np.linspace(0, c.N - 1, 7).astype(int))
        for j in labs:
            v, pre = S._log_softmax_label(lg, np.full(len(fin), j), -(-c.N // 64) + 6)
            assert (v == c.ref.lp[fin, j]).all() and np.allclose(2.0 * pre, c.ref.tol[fin, j], rtol=1e-12, atol=0)
        flat = np.ascontiguousarray(c.buf[fin]).reshape(-1)
        sc, tol = S.tvg_criterion(flat, c.ld, c.N, np.full(len(fin), labs[-1]), len(fin), 1)
        assert (sc == c.ref.lp[fin, labs[-1]]).all() and (tol >= c.ref.tol[fin, labs[-1]]).all()


@pytest.mark.parametrize("rule", R.RULES)
def test_wrong_rules_are_told_apart(rule):
    seen = 0
    for spec in R.CASES:
        c = R.case(spec)
        if c.N > 4099:
            continue
        with np.errstate(**_quiet):
            w = R.rank(c, rule)
            far = np.abs(w.lp - c.ref.lp) > 10.0 * c.ref.tol
        differs = (w.idx != c.ref.idx).any() or far.any()
        if rule == "prior_norm_omitted":
            assert not differs
            differs = (w.val.view(np.int32) != c.ref.val.view(np.int32)).any()
        seen += bool(differs)
    assert seen, rule
