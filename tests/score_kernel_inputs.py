"""TEST INFRASTRUCTURE: the inputs of tests/test_score_kernels_gpu.py, made on the host as exact f32 / 16-bit values, with their float64 references
(oracle/score_kernels_ref.py) computed once per case.  tests/test_score_kernels_ref.py runs its wrong rules over exactly these cases.

The shapes are the smallest at which each kernel takes another path (the case lists say which), not the workload's; the lists cover every value the kernels' code
distinguishes, not the full cross product.  Labels, table and feature indices are always in range (the kernels do not guard them); only the RMSNorm gather
index is taken out of range, because that kernel guards it."""
import functools
import types
import zlib

import numpy as np

from oracle import score_kernels_ref as S
from oracle.attention_ref import round16

DTYPES = ("f16", "bf16")
RMS_EPS = 1e-6
MASSIVE_COL, MASSIVE_W = 5, 2.0e4          # the `massive` family: x[:, 5] = 3e4 under a weight of 2e4 -- the output there is w sqrt(H) >= 1.6e5, beyond fp16
f32 = np.float32


def ratio(got, ref, tol):
    """max |got - ref| / tol over the elements with a tolerance.  inf (a failure) when: the reference states a non-finite element and the output is not that very
    value (NaN for NaN, the same infinity), the output is non-finite anywhere else, or an element with tolerance 0 is not exact."""
    got, ref, tol = (np.asarray(a, np.float64) for a in (got, ref, tol))
    stated = ~np.isfinite(ref)
    g, r = got[stated], ref[stated]
    if (np.isnan(g) != np.isnan(r)).any() or (g[~np.isnan(r)] != r[~np.isnan(r)]).any() or not np.isfinite(got[~stated]).all():
        return float("inf")
    err, t = np.abs(got[~stated] - ref[~stated]), tol[~stated]
    if (err[t == 0] != 0).any():
        return float("inf")
    return float(np.max(err[t > 0] / t[t > 0])) if (t > 0).any() else 0.0


def untouched(before, after, own):
    """True when every element outside the mask `own` holds the bits it held before the call (sentinels: row padding, rows past n_rows)."""
    return bool((np.asarray(after)[~own] == np.asarray(before)[~own]).all())


def rs_of(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# ---- RMSNorm.  H: 64 fewer float4 than lanes; 256 rmsnorm_kernel<4>, the last H before the wide kernel; 260 H % 8 == 4 stays on <4>; 264 the smallest wide shape
# (33 chunks: a partly filled second pass); 1028 rmsnorm_kernel<16>; 3584 the model's; 4096 the wide kernel's maximum; 4096 with ldo = 4100 <16> at its maximum
# (ldo % 8 != 0 is the only in-process way to <16> at H % 8 == 0).  n_rows 1 / 5 / 7: the last block has idle waves.  ldx = H + xpad.  ldo "H" | "2H" | "2H+8" |
# "4100"; with 2H.. the lo half sits H elements into the row (the compensated mode's [hi | lo]), else in a buffer of its own.  outs: h = out16, l = out_lo,
# f = out_f32.  gather: repeated indices, n_src < n_rows, one index -1 and one == n_src.  (H, n_rows, xpad, ldo, outs, gather, family, saturate)
RMS = [(64, 1, 0, "H", "hlf", 0, "gauss", 1), (64, 5, 12, "2H", "hlf", 1, "gauss", 1), (64, 5, 0, "H", "hlf", 0, "tiny", 1), (64, 7, 0, "2H", "hlf", 0, "massive", 1),
       (256, 7, 0, "2H+8", "hlf", 0, "gauss", 1), (256, 5, 12, "H", "hf", 1, "massive", 1), (256, 5, 0, "2H", "hlf", 0, "tiny", 1),
       (260, 5, 0, "H", "hf", 0, "gauss", 1), (260, 7, 12, "2H", "hlf", 1, "nonfinite", 1),
       (264, 1, 0, "H", "hlf", 0, "gauss", 1), (264, 7, 12, "2H+8", "hlf", 1, "gauss", 1), (264, 5, 0, "2H", "hlf", 0, "zero", 1),
       (1028, 5, 0, "2H", "hlf", 0, "gauss", 1), (1028, 7, 12, "H", "hl", 1, "gauss", 1), (1028, 5, 0, "2H", "hlf", 0, "nonfinite", 1),
       (1028, 5, 12, "2H", "hlf", 0, "massive", 1), (1028, 5, 0, "H", "hlf", 0, "massive", 0),
       (3584, 5, 12, "2H", "hlf", 1, "massive", 1), (3584, 7, 0, "H", "h", 0, "gauss", 1), (3584, 5, 0, "2H", "hlf", 0, "massive", 0),
       (3584, 5, 0, "2H", "hlf", 0, "nonfinite", 1), (3584, 5, 0, "2H", "hlf", 0, "tiny", 1), (3584, 7, 12, "2H", "hl", 1, "gauss", 1),
       (4096, 7, 0, "2H+8", "hlf", 1, "gauss", 1), (4096, 5, 12, "4100", "hlf", 1, "gauss", 1), (4096, 1, 0, "H", "f", 0, "tiny", 1), (4096, 5, 0, "4100", "hf", 0, "zero", 1)]
# out6 (the wide kernel's tile writer): one row group / one row past a 256-row tile; ldo = H with out_lo NULL and ldo = 2H with out_lo = out16 + H, the two forms
# run_layers launches.  (H, n_rows, ldo, gather)
RMS6 = [(384, 3, "H", 0), (384, 257, "2H", 1), (3584, 3, "2H", 1), (3584, 257, "H", 0)]
RMS_F8 = [(64, 5, "gauss"), (1028, 5, "zero"), (4096, 3, "gauss"), (256, 1, "tiny")]


def ldo_of(H, kind):
    return {"H": H, "2H": 2 * H, "2H+8": 2 * H + 8, "4100": 4100}[kind]


def _rms_x(rs, n_src, H, family):
    x = rs.standard_normal((n_src, H))
    if family == "massive":
        x[:, MASSIVE_COL] = 3.0e4 * np.where(np.arange(n_src) % 2, -1.0, 1.0)
    if family == "tiny":
        x[0] *= 1e-20 / np.linalg.norm(x[0])                      # eps decides
    if family == "zero":
        x[0] = 0.0
    x = x.astype(f32)
    if family == "nonfinite":
        x[0, 3] = np.nan
        x[1, H - 2] = np.inf
    return x


def _gather(rs, n, on):
    """(rows or None, n_src)."""
    if not on or n < 3:
        return None, n
    if n < 5:                                                     # three rows: a valid one and the two poisoned ones (with the block's idle wave: every path of the kernel in one workgroup)
        return np.array([1, -1, 2], np.int32)[:n], 2
    n_src = n - 2 if n < 64 else 200
    rows = rs.randint(0, n_src, size=n)
    rows[0], rows[1], rows[3] = n_src - 1, 0, n_src - 1           # a repeated index; the last and the first source row
    rows[2], rows[4] = -1, n_src                                  # the two the kernel must poison
    return rows.astype(np.int32), n_src


@functools.lru_cache(maxsize=None)
def rms(case):
    H, n, xpad, ldo, outs, gather, family, sat = case
    rs = rs_of("rms", case)
    c = types.SimpleNamespace(H=H, n=n, ldx=H + xpad, ldo=ldo_of(H, ldo), outs=outs, family=family, sat=sat, lo_inside=ldo in ("2H", "2H+8"))
    c.rows, c.n_src = _gather(rs, n, gather)
    c.x = _rms_x(rs, c.n_src, H, family)
    c.w = (1.0 + 0.2 * rs.standard_normal(H)).astype(f32)
    if family == "massive":
        c.w[MASSIVE_COL] = MASSIVE_W
    c.form = S.rmsnorm_form(H, c.ldx, c.ldo)
    c.ref = S.rmsnorm(c.x, c.w, RMS_EPS, H, rows=c.rows, n_src=c.n_src, form=c.form, ldx=c.ldx)
    return c


@functools.lru_cache(maxsize=None)
def rms6(case):
    H, n, ldo, gather = case
    return rms((H, n, 0, ldo, "hlf" if ldo == "2H" else "hf", gather, "gauss", 1))


@functools.lru_cache(maxsize=None)
def rms_f8(case):
    H, n, family = case
    rs = rs_of("rms8", case)
    c = types.SimpleNamespace(H=H, n=n, ldx=H + 12, family=family)
    c.x = _rms_x(rs, n, H, family)
    c.w = (1.0 + 0.2 * rs.standard_normal(H)).astype(f32)
    c.ref = S.rmsnorm_f8(c.x, c.w, RMS_EPS, H)
    return c


# ---- lse_combine: 64 lanes over n_tiles -- 1, 3 (idle lanes), 64 (every lane once), 65 (one lane twice), 594 = ceil(152064 / 256) (the model's).  Four rows per
# block: 1 / 5 / 9.  (n_tiles, n_rows, family)
LSE = [(1, 1, "gauss"), (3, 5, "one_dominant"), (3, 9, "masked"), (64, 9, "gauss"), (64, 5, "far_apart"), (65, 5, "far_apart"), (65, 9, "gauss"), (65, 5, "empty_tiles"),
       (594, 5, "empty_tiles"), (594, 9, "masked"), (594, 1, "gauss"), (594, 5, "one_dominant")]


@functools.lru_cache(maxsize=None)
def lse(case):
    T, n, family = case
    rs = rs_of("lse", case)
    c = types.SimpleNamespace(T=T, n=n, family=family)
    m = rs.standard_normal((n, T)) * 3.0
    s = rs.uniform(1.0, 256.0, size=(n, T))
    if family == "one_dominant":
        m[np.arange(n), rs.randint(0, T, size=n)] += 30.0
    if family == "far_apart":                                     # maxima 200 apart: exp underflows
        m -= 200.0 * (np.arange(T) % 2)[None, :]
    if family == "empty_tiles":                                   # (-inf, 0) at the front and at the back
        m[:, :2], s[:, :2], m[:, -2:], s[:, -2:] = -np.inf, 0.0, -np.inf, 0.0
    c.m, c.s = m.astype(f32), s.astype(f32)
    c.ll = (rs.standard_normal(n) * 3.0).astype(f32)
    c.labels = rs.randint(0, 1000, size=n).astype(np.int32)
    if family == "masked":
        c.labels[::3] = -100
    c.ref, c.tol = S.lse_combine(c.m, c.s, c.ll, c.labels)
    return c


# ---- ce_rows: 256 threads over V -- 1, 37 (idle threads), 256, 257 (one thread twice), 1000, 152064 (the model's).  (V, ld - V, n_rows, family)
CE = [(1, 0, 1, "gauss"), (37, 5, 3, "gauss"), (37, 0, 3, "masked"), (256, 0, 3, "shifted"), (257, 5, 3, "masked"), (257, 0, 1, "peaked"), (1000, 5, 3, "shifted"),
      (1000, 0, 3, "gauss"), (152064, 5, 3, "gauss"), (152064, 0, 1, "peaked")]


@functools.lru_cache(maxsize=None)
def ce(case):
    V, pad, n, family = case
    rs = rs_of("ce", case)
    c = types.SimpleNamespace(V=V, ld=V + pad, n=n, family=family)
    lg = rs.standard_normal((n, V)) * 2.0
    c.labels = rs.randint(0, V, size=n).astype(np.int32)
    if family == "shifted":                                       # every logit near +90 / -90: expf without the max overflows / vanishes
        lg = lg * 0.5 + np.where(np.arange(n) % 2, -90.0, 90.0)[:, None]
    if family == "peaked":
        lg[np.arange(n), (c.labels + 1) % V] += 40.0
    if family == "masked":
        c.labels[1::3] = -100
    buf = np.full((n, c.ld), np.nan, f32)                         # columns [V, ld) are never read
    buf[:, :V] = lg
    c.buf = buf
    c.ref, c.tol = S.ce_rows(np.nan_to_num(buf), c.ld, V, c.labels)
    return c


# ---- TVG criterion: four waves take the clips round-robin -- 1, 3 (idle waves), 4, 5 (one wave twice), 9; 64 lanes over n_vocab -- 1, 63, 64, 65, 1000.
# (clips, n_vocab, ld - n_vocab, n_pairs)
TVG = [(1, 1, 0, 1), (3, 63, 3, 3), (4, 64, 0, 3), (5, 65, 3, 3), (9, 1000, 3, 3), (9, 64, 0, 1), (5, 1000, 0, 3), (1, 65, 3, 3), (4, 63, 3, 1), (9, 63, 0, 3)]


@functools.lru_cache(maxsize=None)
def tvg(case):
    clips, nv, pad, npairs = case
    rs = rs_of("tvg", case)
    c = types.SimpleNamespace(clips=clips, nv=nv, ld=nv + pad, n_pairs=npairs)
    buf = np.full((npairs * clips, c.ld), np.nan, f32)
    buf[:, :nv] = rs.standard_normal((npairs * clips, nv)) * 3.0
    c.buf = buf
    c.labels = ((np.arange(npairs) * 7 + 3) % nv).astype(np.int32)        # differs per pair
    c.ref, c.tol = S.tvg_criterion(np.nan_to_num(buf), c.ld, nv, c.labels, npairs, clips)
    return c


# ---- segment_mean: one thread per pair, 128 per block -- 1 and 129 pairs; lengths 1 .. 300 with exact zeros inside, one all-zero and one empty segment.
SEG = [(1, 0), (1, 1), (129, 0), (129, 1)]


@functools.lru_cache(maxsize=None)
def seg(case):
    n_pairs, mode = case
    rs = rs_of("seg", n_pairs)
    lens = rs.randint(1, 301, size=n_pairs)
    if n_pairs > 4:
        lens[:4] = 1, 300, 0, 5                                   # the shortest, the longest, an empty one, the all-zero one
    else:
        lens[0] = 17
    c = types.SimpleNamespace(n_pairs=n_pairs, mode=mode)
    c.row_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    lp = -np.abs(rs.standard_normal(c.row_start[-1] + 1)) * 4.0   # (+ one element behind the last segment: finite, never read)
    lp[7::7] = 0.0
    if n_pairs > 4:
        lp[c.row_start[3]:c.row_start[4]] = 0.0
    c.lp = lp.astype(f32)
    c.ref, c.tol = S.segment_mean(c.lp, c.row_start, mode)
    return c


# ---- group_mean: (group, n_out, H, split)
GM = [(1, 1, 8, 0), (1, 5, 8, 1), (3, 5, 8, 1), (3, 5, 1024, 0), (3, 1, 1024, 1), (64, 5, 1024, 0), (64, 1, 1024, 1), (64, 5, 8, 1), (64, 1, 8, 0)]


@functools.lru_cache(maxsize=None)
def gm(case, dtype):
    group, n_out, H, split = case
    rs = rs_of("gm", case, dtype)
    c = types.SimpleNamespace(group=group, n_out=n_out, H=H, split=split, dtype=dtype)
    v = rs.standard_normal((n_out * group, H))
    hi = round16(v, dtype)
    c.x = np.concatenate([hi, round16(v - hi, dtype)], 1) if split else hi        # split inputs carry a non-zero lo half
    c.ref = S.group_mean(c.x, group, dtype, split)
    return c


# ---- assemble: (H, split).  Seven tokens: table and feature rows mixed, feature index 0 (src = -1) and the last table / feature row among them.
ASM = [(8, 0), (8, 1), (3584, 0), (3584, 1)]
ASM_SRC = np.array([0, -1, 5, -4, 2, -1, 3], np.int32)
ASM_TABLE_ROWS, ASM_FEAT_ROWS = 6, 4


@functools.lru_cache(maxsize=None)
def asm(case):
    H, split = case
    rs = rs_of("asm", case)
    c = types.SimpleNamespace(H=H, split=split, src=ASM_SRC)
    c.table = rs.randint(1, 0x7BFF, size=(ASM_TABLE_ROWS, H)).astype(np.uint16)
    c.feats = rs.randint(1, 0x7BFF, size=(ASM_FEAT_ROWS, (2 if split else 1) * H)).astype(np.uint16)
    c.ref = S.assemble(c.src, c.table, c.feats, H, split)
    return c
