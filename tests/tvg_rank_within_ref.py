"""TEST INFRASTRUCTURE: the numpy statement of blim_tvg_rank_within's rule (include/blim.h), built on tests/tvg_rank_ref.py's log_softmax_rows, term_of and order,
and the inputs of tests/test_tvg_rank_within_gpu.py; tests/test_tvg_rank_within_ref.py pins the statement on hand-made rows and shows that these inputs tell the
wrong rules from the right one.

Per query q: its row r = row_of[q] (None: q), its list = within[clamp(off[q]) : clamp(off[q + 1])] (clamped to 0 .. n_within; a decreasing pair is empty), the term of
position p = term_of(whole-row lp)[list[p]] -- NaN for an entry outside 0 .. N - 1 or a row outside 0 .. n_rows - 1 --, idx = the first min(k, m) POSITIONS by
(is NaN, -term, position), val = their terms; places from m on hold -1 / NaN."""
import functools
import types
import zlib

import numpy as np

import tvg_rank_ref as R

f32 = np.float32
RULES = ("subset_norm", "ties_high", "entries_for_positions", "row_of_ignored", "offsets_off_by_one", "k_not_clipped", "nan_first")
_quiet = dict(over="ignore", invalid="ignore", divide="ignore")
BAD = (-1, None, 2 ** 31 - 1)          # None: N itself


def clamp(o, n_within):
    return min(max(int(o), 0), n_within)


def lists_of(c, rule=None):
    """-> per query (row or None when it lies outside the rows, the list's entries)."""
    out = []
    d = 1 if rule == "offsets_off_by_one" else 0
    for q in range(c.n_q):
        r = q if (c.row_of is None or rule == "row_of_ignored") else int(c.row_of[q])
        o0, o1 = clamp(c.within_off[q] + d, c.n_within), clamp(c.within_off[q + 1] + d, c.n_within)
        out.append((r if 0 <= r < c.rows else None, c.within[o0:max(o0, o1)]))
    return out


def expect(c, lp32, pl32, rule=None):
    """lp32 f32 [rows, N] (pl32 f32 [n_prior, N]): the whole-row log-softmax rows -> (idx int32 [n_q, k], val f32 [n_q, k], term: per query f32 [m_q])."""
    idx = np.full((c.n_q, c.k), -1, np.int32)
    val = np.full((c.n_q, c.k), np.nan, f32)
    terms = []
    for q, (r, lst) in enumerate(lists_of(c, rule)):
        m = len(lst)
        ok = (lst >= 0) & (lst < c.N)
        t = np.full(m, np.nan, f32)
        if r is not None and m:
            po = None if c.prior_of is None else c.prior_of[q:q + 1]
            lp_row = lp32[r:r + 1]
            pl = pl32
            if rule == "subset_norm":                     # the normalisers over the list's own columns
                cols = np.unique(lst[ok])
                sub = lambda buf, i: np.where(np.isin(np.arange(c.N), cols), buf[i, :c.N].astype(np.float64), -np.inf)[None]
                lp_row = R.log_softmax_rows(sub(c.buf, r))[0].astype(f32)
                if pl32 is not None:
                    pl = np.concatenate([R.log_softmax_rows(sub(c.pbuf, i))[0] for i in range(c.n_prior)]).astype(f32)
            with np.errstate(**_quiet):
                row = R.term_of(lp_row, pl, po, c.n_prior, c.alpha)[0]
            t[ok] = row[lst[ok]]
        terms.append(t)
        kk = min(c.k, m)
        if kk:
            o = R.order(t[None], kk, rule if rule in ("ties_high", "nan_first") else None)[0]
            idx[q, :kk] = lst[o] if rule == "entries_for_positions" else o
            val[q, :kk] = t[o]
        if rule == "k_not_clipped" and m and m < c.k:     # the places behind the list taken as if the list went on
            idx[q, m:] = np.arange(m, c.k)
            val[q, m:] = 0
    return idx, val, terms


def rank_within(c, rule=None):
    """The whole rule on a case, lp from the float64 statement (the GPU test forms it from the kernel's own lp)."""
    lp = R.log_softmax_rows(R.rows_of(c.buf, c.ld, c.N, c.rows))[0].astype(f32)
    pl = None if c.prior_of is None else R.log_softmax_rows(R.rows_of(c.pbuf, c.ldp, c.N, c.n_prior))[0].astype(f32)
    idx, val, terms = expect(c, lp, pl, rule)
    return types.SimpleNamespace(idx=idx, val=val, terms=terms)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------- inputs
# N: 1 the smallest; 65 / 257 one past a wave's and a workgroup's step; 1000 the measured gallery; 4099 odd and above every list length.  Every N with ld = N and N + 3
# and two of the four k.  The list lengths of one case: 0; 1; 63 / 64 / 65 and 255 / 256 / 257 around the select's steps; 1024 / 1025 around the largest k; N; k itself
# (k = m_q; the others give k > m_q and k < m_q).  Entries are drawn WITH replacement (repeats; at N = 1 every entry is column 0, so the order is the tie rule alone),
# and lists of 3 and more get the entries -1, N and 2^31 - 1.  `shared`: three rows and row_of = q mod 3, so five queries share a row with different lists, one query
# names a row outside the rows; otherwise row_of is None and every query has its own row.  Three more queries have the offsets past n_within, decreasing, and
# overlapping the first lists; the first offset is negative.
NS = (1, 65, 257, 1000, 4099)
KS = (1, 16, 64, 1024)
FAMILIES = ("gauss1", "equal", "dups", "neginf", "nan")


def _case_list():
    out, i = [], 0
    for N in NS:
        for pad in (0, 3):
            for j in (0, 2):
                out.append((N, pad, KS[(i + j) % 4], i % 5, (0, 1, 2)[i % 3], (0.0, 0.7)[(i // 2) % 2], i % 4 != 3))
            i += 1
    return out


CASES = _case_list()          # (N, pad, k, first family, prior: 0 none / 1 prior_of given / 2 given, ld_prior = N + 5, alpha, shared)


@functools.lru_cache(maxsize=None)
def case(spec):
    N, pad, k, fam0, prior, alpha, shared = spec
    rs = np.random.RandomState(zlib.crc32(repr(spec).encode()) & 0x7FFFFFFF)
    ms = [0, 1, 63, 64, 65, 255, 256, 257, 1024, 1025, N, k]
    lists = []
    for m in ms:
        lst = rs.randint(0, N, m).astype(np.int64)
        if m >= 3:
            at = rs.choice(m, 3, replace=False)
            lst[at] = [N if b is None else b for b in BAD]
        lists.append(lst)
    within = np.concatenate(lists).astype(np.int32)
    n_within = len(within)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    off[0] = -3                                              # clamped to 0
    off = np.concatenate([off, [n_within + 7, 5, min(70, n_within)]]).astype(np.int32)       # ... an empty list past the end, a decreasing pair, within[5:70]
    n_q = len(off) - 1
    rows = 3 if shared else n_q
    c = types.SimpleNamespace(N=N, k=k, rows=rows, ld=N + pad, alpha=alpha, n_prior=0, prior_of=None, pbuf=None, ldp=0, n_q=n_q, within=within, within_off=off,
                              n_within=n_within, ms=ms, shared=shared)
    buf = np.full((rows, c.ld), np.nan, f32)                # columns [N, ld) are never read
    c.families = [FAMILIES[(fam0 + i) % 5] for i in range(rows)]
    for i, fam in enumerate(c.families):
        buf[i, :N] = R._row(rs, N, min(k, N), fam)
    c.buf = buf
    c.row_of = None
    if shared:
        c.row_of = (np.arange(n_q) % 3).astype(np.int32)
        c.row_of[4] = (3, -1)[fam0 % 2]                      # outside the rows: every term of the query is NaN
    if prior:
        c.n_prior, c.ldp = 2, N + (5 if prior == 2 else 0)
        pb = np.full((2, c.ldp), np.nan, f32)
        pb[0, :N] = R._row(rs, N, min(k, N), "gauss1")
        pb[1, :N] = R._row(rs, N, min(k, N), "neginf")
        c.pbuf = pb
        c.prior_of = np.array([(0, -1, 1, 2, 0)[(fam0 + q) % 5] for q in range(n_q)], np.int32)       # -1: none; 2: >= n_prior, a NaN query
    c.ref = rank_within(c)
    return c
