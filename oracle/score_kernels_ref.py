"""Float64 statements of the scoring path's row kernels (csrc/kernels.hip: the three forward RMSNorm kernels and rmsnorm_f8, lse_combine, ce_rows, the TVG
criterion, segment_mean, group_mean plain and split, assemble plain and split), in plain numpy, each with a per-element bound on |kernel - reference|.  The only
source of tolerances of tests/test_score_kernels_gpu.py; tests/test_score_kernels_ref.py pins every function to an independent statement and shows that the
wrong rules (RULES) leave the bounds on the GPU tests' inputs.

    tol = 2 * (sum of the named first-order terms)            -- the project's factor 2 (oracle/train_kernels_ref.py)

U = 2^-24 is one f32 rounding; every bound is formed from the reference's own magnitudes, nothing is fitted to a kernel's output.  U, TINY, err16, store16,
round16 and _red_depth are oracle/train_kernels_ref.py's, e2m3_tiles oracle/gemm_ref.py's (whose e4m3_decode the tests use for rmsnorm_f8's codes).

Device math functions.  Neither the ROCm documentation installed beside the compiler nor the compiler's own help states an ulp bound for sqrtf, 1.0f / x, a / b,
expf and logf as this build compiles them (-O3, no fast-math: the OCML functions, and correctly rounded division and square root, the HIP default), so ULP below
was MEASURED on an MI355X against float64 over the arguments these tests' own inputs produce (every sqrtf / reciprocal argument of the RMSNorm cases, every
expf / logf argument of the lse_combine, ce_rows and TVG cases, every quotient of segment_mean and TVG), error in ulps of the f32 result:
    function    arguments   worst seen      allowance = 2 x worst, rounded up to a whole ulp
    sqrtf       592         0.4999 ulp      1 ulp
    1.0f / x    605         0.4985 ulp      1 ulp
    a / b       895         0.4942 ulp      1 ulp
    expf        677,324     0.8312 ulp      2 ulp       (320 results below 2^-126 came back as 0: the 2^-126 term of `exp` below)
    logf        214         2.0006 ulp      5 ulp
(tools/math_ulp_args.py writes the arguments, tools/math_ulp_probe.hip measures; measured against float64, never against another run of a kernel.)
One ulp is 2 U relative.  The terms:
  ss            RMSNorm's sum of squares: the lane's own terms (4 ceil(H / 256) in rmsnorm_kernel<4 / 16> and rmsnorm_f8, 8 ceil(H / 512) in rmsnorm_wide_kernel),
                six shuffle levels, one rounding per square (an fma only removes roundings).  Every term is >= 0, so the bound is RELATIVE: depth U ss.  Squares
                below 2^-126 may be flushed: + H 2^-126 absolute, which only a row whose eps decides ever sees.
  rms           / H, + eps: U each on their results; sqrtf halves the relative error of its argument and adds ULP.sqrt; the reciprocal adds ULP.rcp; x * inv and
                w * (.) one U each.  A result below 2^-126: + 2^-126.
  16-bit        hi and lo are FUNCTIONS of the kernel's own f32 value o: hi = round16(o) (fp16 + saturate: finite overflow -> +-65504), lo = round16(fl32(o - hi)).
                They are compared bit for bit with split16(out_f32 of the same launch) -- not with the float64 reference: one f32 ulp of o can flip a 16-bit
                rounding and move lo by a whole 16-bit ulp.  Without an f32 output hi + lo is within store16 applied twice.
  non-finite    float64 evaluates the kernel's own rule: a NaN in a row makes ss NaN and the whole row NaN; an inf makes ss inf, inv = 0 and the row 0 * x: exactly 0
                where x is finite, NaN at the inf.  A gather index outside [0, n_src) is a POISONED row: NaN in hi and f32, ZERO in lo and in the tiles.
  exp           expf(a), a = x - max formed in f32: U |a| for the subtraction's rounding moved through exp, U |a| for the argument reduction, ULP.exp:
                (2 |a| + 2 ULP.exp) U relative (oracle/train_kernels_ref.ce_fwd_bwd's model); a result below 2^-126 may be flushed: + 2^-126 absolute.
  log           logf(s): 2 ULP.log U |log s| + the error of s over s.
  sums          depth U (sum of magnitudes), depth = the longest chain: lse_combine ceil(n_tiles / 64) + 6; ce_rows _red_depth(ceil(V / 256)); TVG per clip
                ceil(n_vocab / 64) + 6, then ceil(clips / 4) sequential adds per wave, three adds, one division; segment_mean the segment's length; group_mean
                `group` (split: 2 group, each row adds hi + lo first).
  segment_mean  sum / count_nonzero (mode 0) or sum / rows (mode 1): what the reference's retrieval_utils forms.  A segment without a non-zero entry in mode 0 and an
                empty segment in mode 1 are 0 / 0 = NaN -- pinned here and in the tests so that a later change is deliberate.
"""
import types

import numpy as np

from oracle.gemm_ref import FP8_MAX, e2m3_tiles
from oracle.train_kernels_ref import TINY, U, _red_depth, err16, round16, store16

f32 = np.float32
ULP = types.SimpleNamespace(sqrt=1, rcp=1, div=1, exp=2, log=5)         # measured allowances, in whole ulps (the table above)
RULES = {
    "rmsnorm": ("eps_outside_sqrt", "mean_over_ldx", "tail_chunk_dropped", "gather_ignored", "neighbour_row", "poison_missing"),
    "rmsnorm16": ("lo_dropped", "lo_from_unsaturated_hi", "saturate_ignored"),
    "lse_combine": ("first_64_tiles_only", "no_rescale", "empty_tile_counted", "masked_label_not_zero"),
    "ce_rows": ("ld_taken_as_V", "no_max_subtraction", "tail_dropped"),
    "tvg": ("first_four_clips_only", "divide_by_four", "ld_ignored", "label_of_pair_0"),
    "segment_mean": ("mode_swapped", "end_inclusive"),
    "group_mean": ("hi_only", "group_minus_one", "divide_after_round"),
    "assemble": ("lo_half_of_table_rows_not_zero", "feature_index_off_by_one"),
}
_quiet = dict(over="ignore", invalid="ignore", divide="ignore")


# ---------------------------------------------------------------------------- RMSNorm
def rmsnorm_form(H, ldx, ldo):
    """The kernel launch_rmsnorm picks: "wide", "narrow4", "narrow16", or None where it refuses the shape."""
    ldo = ldo or H
    if H % 4 or ldx % 4 or ldo % 4:
        return None
    if H % 8 == 0 and 256 < H <= 4096 and ldo % 8 == 0:
        return "wide"
    return "narrow4" if H <= 1024 else "narrow16" if H <= 4096 else None


def rmsnorm(x, w, eps, H, rows=None, n_src=None, form="narrow4", ldx=None, rule=None):
    """x f32 [source rows, >= H] (columns [0, H) are the rows), w f32 [H]; rows: the gather (int [n]) among n_src valid rows, None = the identity.
    Returns a namespace: o [n, H] = w x rsqrt(mean x^2 + eps) with NaN exactly where the kernel's rule gives NaN (module docstring: non-finite), pre (the bound on
    the kernel's f32 value before the factor 2), tol = 2 pre (0 where o is NaN or an exact 0 of an inf row), poison [n] bool."""
    x, w = np.asarray(x, np.float64)[:, :H], np.asarray(w, np.float64)
    n_src = x.shape[0] if n_src is None else n_src
    src = np.arange(x.shape[0] if rows is None else len(rows)) if rows is None or rule == "gather_ignored" else np.asarray(rows, np.int64)
    n = len(src)
    if rule == "gather_ignored":
        src = src % n_src
    poison = (src < 0) | (src >= n_src)
    if rule == "poison_missing":
        src, poison = np.clip(src, 0, n_src - 1), np.zeros(n, bool)
    if rule == "neighbour_row":
        src = np.where(poison, src, (src + 1) % n_src)
    xr = x[np.where(poison, 0, src)]
    chunk = 512 if form == "wide" else 256
    terms = (8 if form == "wide" else 4) * -(-H // chunk)
    keep = (H // chunk) * chunk if rule == "tail_chunk_dropped" else H
    fe = float(f32(eps))
    with np.errstate(**_quiet):
        ss = (xr[:, :keep] ** 2).sum(1, keepdims=True)
        mean = ss / (ldx if rule == "mean_over_ldx" else H)
        var = mean + fe
        inv = 1.0 / (np.sqrt(mean) + fe) if rule == "eps_outside_sqrt" else 1.0 / np.sqrt(var)
        o = w * (xr * inv)
        e_var = mean * ((terms + 7) * U + U) + TINY + U * var
        rel = 0.5 * e_var / var + (2 * ULP.sqrt + 2 * ULP.rcp + 2) * U
        pre = np.abs(o) * rel + TINY
    o[poison] = np.nan
    exact = ~np.isfinite(o) | ~np.isfinite(ss)            # NaN elements, and the exact zeros of a row whose ss is inf
    pre = np.where(exact, 0.0, pre)
    return types.SimpleNamespace(o=o, pre=pre, tol=2.0 * pre, poison=poison)


def _sat(v, o, dtype, saturate):
    """fp16 with MODE.FP16_OVFL: a FINITE value beyond the format becomes +-65504; infinities and NaN pass."""
    if dtype != "f16" or not saturate:
        return v
    return np.where(np.isfinite(np.asarray(o, np.float64)), np.clip(v, -65504.0, 65504.0), v)


def split16(o32, dtype, saturate=True, poison=None, rule=None):
    """The 16-bit outputs as functions of the kernel's own f32 values o32 [n, H]: (hi, lo) float64 of the 16-bit values, hi = round16(o) (saturated),
    lo = round16(fl32(o - hi)) (saturated alike); a poisoned row is NaN / 0."""
    o = np.asarray(o32, f32)
    with np.errstate(**_quiet):
        raw = round16(o.astype(np.float64), dtype)
        hi = raw if rule == "saturate_ignored" else _sat(raw, o, dtype, saturate)
        d = o - (raw if rule == "lo_from_unsaturated_hi" else hi).astype(f32)
        lo = _sat(round16(d.astype(np.float64), dtype), d, dtype, saturate)
    if rule == "lo_dropped":
        lo = np.zeros_like(lo)
    if poison is not None:
        hi[poison], lo[poison] = np.nan, 0.0
    return hi, lo


def same16(got, want):
    """Elementwise: equal as 16-bit VALUES (float64 of them), NaN matching NaN; the sign of a zero counts."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return ((got == want) & (np.signbit(got) == np.signbit(want))) | (np.isnan(got) & np.isnan(want))


def tol_hi_lo(r, dtype):
    """Bound on |hi + lo - o| where no f32 output says what the kernel held: store16 applied twice."""
    return 2.0 * (r.pre + err16(err16(np.abs(np.nan_to_num(r.o)) + r.pre, dtype), dtype))


def tol_hi(r, dtype):
    return 2.0 * store16(np.nan_to_num(r.o), r.pre, dtype)


def tiles_of(lo_rows):
    """The out6 image of the lo rows [n, H] (16-bit values): gemm_ref.e2m3_tiles of an A operand, flat, rows up to the next multiple of 256 zero."""
    return e2m3_tiles(lo_rows, w_side=False).reshape(-1)


def rmsnorm_f8(x, w, eps, H, rule=None):
    """rmsnorm_f8 (the narrow kernels' arithmetic): returns a namespace o, scale [n] = max|o| / 448 (exactly 1 for an all-zero row), tol_scale, and tol_val(scale_got):
    the bound on |decode(code) scale_got - o| -- e4m3's half ulp of o / scale (2^-4 relative; below 2^-6 the subnormal step 2^-9, half of it 2^-10), the two
    roundings of 1 / scale and o * (1 / scale) (ULP.rcp, U; v_cvt_pk_fp8_f32 itself rounds once, to nearest even), and the f32 bound of o."""
    r = rmsnorm(x, w, eps, H, form="narrow4" if H <= 1024 else "narrow16", rule=rule)
    amax = np.abs(r.o).max(1)
    scale = np.where(amax > 0, amax / FP8_MAX, 1.0)
    tol_scale = np.where(amax > 0, 2.0 * (r.pre.max(1) / FP8_MAX + 2 * ULP.div * U * scale), 0.0)
    r.scale, r.tol_scale = scale, tol_scale
    r.tol_val = lambda sg: 2.0 * (np.maximum(2.0 ** -4 * (np.abs(r.o) + r.pre), 2.0 ** -10 * np.asarray(sg, np.float64)[:, None])
                                  + r.pre + (2 * ULP.rcp + 2) * U * np.abs(r.o))
    return r


# ---------------------------------------------------------------------------- the criteria
def _rel_exp(a):
    return (2.0 * np.abs(a) + 2 * ULP.exp) * U


def lse_combine(m, s, label_logit, labels, rule=None):
    """m, s f32 [n, T]: the per-tile (max, sum exp(x - max)) partials, an empty tile (-inf, 0); -> (logprob [n], tol): label_logit - logsumexp, exactly 0 where
    labels < 0."""
    m, s, ll, labels = np.asarray(m, np.float64), np.asarray(s, np.float64), np.asarray(label_logit, np.float64), np.asarray(labels)
    n, T = m.shape
    if rule == "first_64_tiles_only":
        m, s, T = m[:, :64], s[:, :64], min(T, 64)
    live = m > -np.inf
    big = m.max(1, keepdims=True)
    with np.errstate(**_quiet):
        a = np.where(live, m - big, 0.0)
        e = np.where(live, np.ones_like(a) if rule == "no_rescale" else np.exp(a), 0.0)
        term = s * e + (np.where(live, 0.0, 1.0) if rule == "empty_tile_counted" else 0.0)
        sm = term.sum(1)
        depth = -(-T // 64) + 6
        e_sm = (term * (_rel_exp(a) + U)).sum(1) + TINY * np.abs(s).sum(1) + depth * U * sm
        lg = np.log(sm)
        tot = big[:, 0] + lg
        out = ll - tot
        pre = 2 * ULP.log * U * np.abs(lg) + e_sm / sm + U * np.abs(tot) + U * np.abs(out)
    masked = (labels < 0) & (rule != "masked_label_not_zero")
    return np.where(masked, 0.0, out), np.where(masked, 0.0, 2.0 * pre)


def _log_softmax_label(lg, lab, depth):
    """Rows lg [n, V] float64, labels lab [n] in range -> (log_softmax[label], pre) for a reduction of the given depth."""
    mx = lg.max(1, keepdims=True)
    a = lg - mx
    e = np.exp(a)
    s = e.sum(1)
    e_s = (e * _rel_exp(a)).sum(1) + lg.shape[1] * TINY + depth * U * s
    ll = lg[np.arange(len(lg)), lab]
    tot = mx[:, 0] + np.log(s)
    out = ll - tot
    return out, 2 * ULP.log * U * np.abs(np.log(s)) + e_s / s + U * np.abs(tot) + U * np.abs(out)


def ce_rows(logits, ld, V, labels, rule=None):
    """logits: the flat f32 buffer of n rows of stride ld (columns [V, ld) are never read); labels int [n], < 0 = masked (exactly 0), else in [0, V).
    -> (logprob [n], tol)."""
    flat, labels = np.asarray(logits, np.float64).reshape(-1), np.asarray(labels)
    n = len(labels)
    stride = V if rule == "ld_taken_as_V" else ld
    lg = np.stack([flat[r * stride:r * stride + V] for r in range(n)])
    lab = np.where(labels < 0, 0, labels)
    out, pre = _log_softmax_label(lg, lab, _red_depth(-(-V // 256)))
    if rule == "tail_dropped":
        keep = (V // 256) * 256
        with np.errstate(**_quiet):
            mx = lg[:, :keep].max(1, initial=-np.inf)
            out = lg[np.arange(n), lab] - (mx + np.log(np.exp(lg[:, :keep] - mx[:, None]).sum(1)))
    if rule == "no_max_subtraction":                      # expf(x) in f32: overflows beyond 88.7, vanishes below -103
        with np.errstate(**_quiet):
            e = np.exp(lg.astype(f32)).astype(np.float64)
            out = lg[np.arange(n), lab] - np.log(e.sum(1))
    return np.where(labels < 0, 0.0, out), np.where(labels < 0, 0.0, 2.0 * pre)


def tvg_criterion(logits, ld, n_vocab, labels, n_pairs, clips, rule=None):
    """logits: the flat f32 buffer of n_pairs * clips rows of stride ld (row p * clips + c = pair p, clip c); labels int [n_pairs] in [0, n_vocab).
    -> (score [n_pairs] = mean over the clips of log_softmax[label], tol)."""
    flat, labels = np.asarray(logits, np.float64).reshape(-1), np.asarray(labels)
    stride = n_vocab if rule == "ld_ignored" else ld
    lg = np.stack([flat[r * stride:r * stride + n_vocab] for r in range(n_pairs * clips)])
    lab = np.repeat(np.full_like(labels, labels[0]) if rule == "label_of_pair_0" else labels, clips)
    v, pre = _log_softmax_label(lg, lab, -(-n_vocab // 64) + 6)
    v, pre = v.reshape(n_pairs, clips), pre.reshape(n_pairs, clips)
    used = v[:, :4] if rule == "first_four_clips_only" else v
    den = 4.0 if rule == "divide_by_four" else float(clips)
    score = used.sum(1) / den
    chain = -(-clips // 4) + 3
    return score, 2.0 * ((pre.sum(1) + chain * U * np.abs(v).sum(1)) / clips + 2 * ULP.div * U * np.abs(score))


def segment_mean(logprob, row_start, mode, rule=None):
    """logprob f32 [>= row_start[-1]], row_start int [n_pairs + 1] -> (score [n_pairs], tol): the sequential f32 sum of the segment over the count of its non-zero
    entries (mode 0) or over its length (mode 1); 0 / 0 = NaN (module docstring)."""
    lp, rs = np.asarray(logprob, np.float64), np.asarray(row_start)
    if rule == "mode_swapped":
        mode = 1 - mode
    score, tol = np.zeros(len(rs) - 1), np.zeros(len(rs) - 1)
    for p in range(len(rs) - 1):
        seg = lp[rs[p]:rs[p + 1] + (1 if rule == "end_inclusive" else 0)]
        den = float(np.count_nonzero(seg)) if mode == 0 else float(len(seg))
        with np.errstate(**_quiet):
            score[p] = seg.sum() / den if den else np.nan
        tol[p] = 0.0 if not den else 2.0 * (len(seg) * U * np.abs(seg).sum() / den + 2 * ULP.div * U * abs(score[p]))
    return score, tol


# ---------------------------------------------------------------------------- clip mean, assembly
def group_mean(x, group, dtype, split=False, rule=None):
    """x: 16-bit values [n_out * group, H] (split: [.., 2 H] = [hi | lo]) -> namespace mean [n_out, H] (float64), pre (the bound on the kernel's f32 value: the
    sequential sum, 1 / group -- a correctly rounded quotient, ULP.div -- and the product), tol (plain: the 16-bit output), and for split tol_sum (hi + lo, store16
    applied twice) and hi_lo / hi_hi: the range round16 of a value within 2 pre can take (rounding is monotonic): the hi half must lie inside, bit-exact where both ends agree."""
    x = np.asarray(x, np.float64)
    H = x.shape[1] // (2 if split else 1)
    v = x[:, :H] + (x[:, H:] if split and rule != "hi_only" else 0.0)
    v = v.reshape(-1, group, H)
    mag = np.abs(x[:, :H]).reshape(-1, group, H).sum(1) + (np.abs(x[:, H:]).reshape(-1, group, H).sum(1) if split else 0.0)
    used = v[:, :group - 1] if rule == "group_minus_one" else v
    if rule == "divide_after_round":
        mean = round16(used.sum(1), dtype) / group
    else:
        mean = used.sum(1) / group
    pre = ((2 if split else 1) * group + 2 * ULP.div + 2) * U * mag / group
    r = types.SimpleNamespace(mean=mean, pre=pre, tol=2.0 * store16(mean, pre, dtype))
    if split:
        r.tol_sum = 2.0 * (pre + err16(err16(np.abs(mean) + pre, dtype), dtype))
        r.hi_lo, r.hi_hi = round16(mean - 2.0 * pre, dtype), round16(mean + 2.0 * pre, dtype)
    return r


def assemble(src, table, feats, H, split=False, rule=None):
    """src int [n]; table uint16 [rows, H]; feats uint16 [rows, H] (split: [rows, 2 H]) -> the output's bit patterns uint16 [n, H] (split: [n, 2 H], a table row's
    lo half zero): out[t] = table[src[t]] for src[t] >= 0, feats[-(src[t] + 1)] otherwise.  Exact."""
    src, table, feats = np.asarray(src), np.asarray(table, np.uint16), np.asarray(feats, np.uint16)
    out = np.zeros((len(src), 2 * H if split else H), np.uint16)
    for t, s in enumerate(src):
        if s >= 0:
            out[t, :H] = table[s]
            if split and rule == "lo_half_of_table_rows_not_zero":
                out[t, H:] = table[(s + 1) % len(table)]          # what the unguarded walk over 2 H columns of a table row reads
        else:
            f = -s if rule == "feature_index_off_by_one" else -(s + 1)
            out[t] = feats[f % len(feats)]
    return out
