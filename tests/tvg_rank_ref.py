"""TEST INFRASTRUCTURE: the numpy statement of blim_tvg_rank's rule (include/blim.h) and the inputs of tests/test_tvg_rank_gpu.py; tests/test_tvg_rank_ref.py pins the
statement on the CPU and shows that these inputs tell the wrong rules from the right one.

lp: float64 log-softmax of the row, with the bound oracle/score_kernels_ref.py derives for the criterion's row at depth ceil(N / 64) + 6 (its _log_softmax_label,
restated here for every label of a row at once and for rows that hold -inf; twice that bound is the tolerance, as for ce_rows).  term and the order are exact rules:
term = lp, or f32(lp - f32(alpha * pl)) in numpy f32 arithmetic; the order is the first k of the columns sorted by (is NaN, -term, index)."""
import functools
import types
import zlib

import numpy as np

from oracle import score_kernels_ref as S

f32 = np.float32
RULES = ("ties_high", "prior_norm_omitted", "alpha_on_lp", "k_minus_1", "ld_as_N", "nan_first")
_quiet = dict(over="ignore", invalid="ignore", divide="ignore")


def rows_of(flat, ld, n_vocab, n_rows):
    flat = np.asarray(flat).reshape(-1)
    return np.stack([flat[r * ld:r * ld + n_vocab] for r in range(n_rows)])


def log_softmax_rows(lg):
    """lg float64 [n, N] -> (lp [n, N], tol [n, N])."""
    lg = np.asarray(lg, np.float64)
    N = lg.shape[1]
    depth = -(-N // 64) + 6
    with np.errstate(**_quiet):
        mx = lg.max(1, keepdims=True)
        a = lg - mx
        e = np.exp(a)
        s = e.sum(1, keepdims=True)
        e_s = np.where(e > 0, e * S._rel_exp(np.where(e > 0, a, 0.0)), 0.0).sum(1, keepdims=True) + N * S.TINY + depth * S.U * s
        tot = mx + np.log(s)
        out = lg - tot
        pre = 2 * S.ULP.log * S.U * np.abs(np.log(s)) + e_s / s + S.U * np.abs(tot) + S.U * np.abs(out)
    return out, 2.0 * pre


def term_of(lp32, pl32, prior_of, n_prior, alpha, rule=None):
    """lp32 f32 [n, N], pl32 f32 [n_prior, N] or None, prior_of int [n] or None -> term f32 [n, N]."""
    lp32 = np.asarray(lp32, f32)
    term = lp32.copy()
    if prior_of is None:
        return term
    al = f32(alpha)
    with np.errstate(**_quiet):
        for r, po in enumerate(np.asarray(prior_of)):
            if po < 0:
                continue
            if po >= n_prior:
                term[r] = np.nan
            elif rule == "alpha_on_lp":
                term[r] = (al * lp32[r]).astype(f32) - pl32[po]
            else:
                term[r] = lp32[r] - (al * pl32[po]).astype(f32)
    return term


def order(term, k, rule=None):
    """term f32 [n, N] -> idx int32 [n, k]: columns by (is NaN, -term, index), the first k."""
    term = np.asarray(term, f32)
    n, N = term.shape
    out = np.full((n, k), -1, np.int32)
    for r in range(n):
        nan = np.isnan(term[r])
        neg = np.where(nan, f32(0), -term[r])
        ix = np.arange(N)
        keys = (-ix if rule == "ties_high" else ix, neg, ~nan if rule == "nan_first" else nan)
        o = np.lexsort(keys)[:k]
        if rule == "k_minus_1":
            o = np.concatenate([o[:k - 1], [-1]])
        out[r] = o
    return out


def rank(c, rule=None):
    """The whole rule on a case of `cases`: lp (float64) and its tolerance, and idx / val formed from f32(lp) -- the GPU test forms them from the kernel's own lp."""
    stride = c.N if rule == "ld_as_N" else c.ld
    lp, tol = log_softmax_rows(rows_of(c.buf, stride, c.N, c.rows))
    pl32 = None
    if c.prior_of is not None:
        pr = rows_of(c.pbuf, c.N if rule == "ld_as_N" else c.ldp, c.N, c.n_prior)
        pl32 = (pr if rule == "prior_norm_omitted" else log_softmax_rows(pr)[0]).astype(f32)
    with np.errstate(**_quiet):
        term = term_of(lp.astype(f32), pl32, c.prior_of, c.n_prior, c.alpha, rule)
    idx = order(term, c.k, rule)
    val = np.stack([np.where(idx[r] >= 0, term[r][idx[r]], f32(0)) for r in range(c.rows)])
    return types.SimpleNamespace(lp=lp, tol=tol, term=term, idx=idx, val=val)


# ---------------------------------------------------------------------------- inputs
# N: 1 / 2 the smallest; 63 / 64 / 65 around one lane-strided step of the normaliser's wave; 255 / 256 / 257 around one step of the workgroup; 1000 the measured
# gallery (k = 1000: the survivors' sort padded to 1024); 4099 odd, the smallest with k = 1024; 70001 several hundred steps, more than 2^16 columns.  k: 1, 2, 16, 64, 1024
# and N wherever k <= min(N, 1024).  Rows 1 / 3 / 5, ld = N and N + 3, the row families, the prior and alpha rotate over the list, so every value of each appears
# at small and large N; row i of a case takes family (case + i) mod 6.
NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099, 70001)
KS = (1, 2, 16, 64, 1024)
FAMILIES = ("gauss1", "gauss30", "equal", "dups", "neginf", "nan")


def _case_list():
    out, i = [], 0
    for N in NS:
        for k in sorted({k for k in KS + (N,) if k <= min(N, 1024)}):
            out.append((N, k, (1, 3, 5)[i % 3], (0, 3)[(i // 2) % 2], i % 6, (0, 1, 2)[(i // 3) % 3], (0.0, 0.7)[(i // 5) % 2]))
            i += 1
    return out


CASES = _case_list()          # (N, k, rows, pad, first family, prior: 0 none / 1 prior_of given / 2 given, ld_prior = N + 5, alpha)


def _row(rs, N, k, family):
    x = rs.standard_normal(N) * (30.0 if family == "gauss30" else 1.0)
    if family == "equal":
        x[:] = 0.25
    if family == "dups" and N > 1:                       # the values of ranks k - 3 .. k + 3 become one value, at scattered columns
        o = np.argsort(-x, kind="stable")
        x[o[max(0, k - 4):min(N, k + 3)]] = x[o[min(k, N) - 1]]
    x = x.astype(f32)
    if family == "neginf" and N > 1:
        x[rs.choice(N, max(1, N // 3), replace=False)] = -np.inf
    if family == "nan":
        x[rs.randint(N)] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def case(spec):
    N, k, rows, pad, fam0, prior, alpha = spec
    rs = np.random.RandomState(zlib.crc32(repr(spec).encode()) & 0x7FFFFFFF)
    c = types.SimpleNamespace(N=N, k=k, rows=rows, ld=N + pad, alpha=alpha, n_prior=0, prior_of=None, pbuf=None, ldp=0)
    buf = np.full((rows, c.ld), np.nan, f32)              # columns [N, ld) are never read
    c.families = [FAMILIES[(fam0 + i) % 6] for i in range(rows)]
    for i, fam in enumerate(c.families):
        buf[i, :N] = _row(rs, N, k, fam)
    c.buf = buf
    if prior:
        c.n_prior, c.ldp = 2, N + (5 if prior == 2 else 0)
        pb = np.full((2, c.ldp), np.nan, f32)
        pb[0, :N] = _row(rs, N, k, "gauss1")
        pb[1, :N] = _row(rs, N, k, "neginf")              # -inf in the prior: alpha * pl is -inf, or NaN at alpha = 0, so a row's term holds SOME NaN or +inf
        c.pbuf = pb
        c.prior_of = np.array([(0, -1, 1, 2, 0)[(fam0 + i) % 5] for i in range(rows)], np.int32)       # -1: none; 2: >= n_prior, a NaN row
    c.ref = rank(c)
    return c
