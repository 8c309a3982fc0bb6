"""Float64 statement of the GEMM's epilogues and operand forms (csrc/gemm.hpp, csrc/gemm.hip), in numpy, and the per-element tolerance of a kernel against it.

The operands are taken as the exact 16-bit (or e4m3 / e2m3) VALUES the kernel sees; every function works on acc = a . w^T in float64 in W's STORED row order
(the order the kernel meets) and returns its result in the order the kernel stores.  What tests/test_gemm_gpu.py compares blim_gemm with, what
tests/test_gemm_ref.py pins to gemm.hpp's words and to the oracle's decoder layer.

`rule` evaluates DELIBERATELY WRONG variants (RULES): the tests use them to show that their inputs tell a wrong kernel from a right one, never as a reference.

Tolerance.  Every epilogue returns, beside its result, `pre`: a bound on |f32 value the kernel holds before its output rounding - the float64 result|, built from
  U = 2^-24, the unit roundoff of f32 (one rounding to nearest: relative error <= U; "1 ulp" of a hardware approximation: <= 2 U);
  gamma_K A, gamma_K = K U, A = sum_k |a_mk w_nk|: the error of an f32 sum of K exact products in ANY order (16-bit x 16-bit, e4m3 x e4m3 and scaled
      e2m3 x e2m3 products are exact in f32), which makes the bound independent of the order of accumulation inside and between the MFMAs;
  one U |value| per f32 operation of the epilogue; the accumulation term times |f'| (float64) through a nonlinear epilogue;
  the approximations' own bounds: gelu_erf 1.5e-7 absolute on erf (Abramowitz & Stegun 7.1.26, gemm.hip), v_rcp_f32 / v_exp_f32 1 ulp (gemm.hip's comments, the
      CDNA ISA's stated accuracy), __expf(x) = v_exp_f32(x log2 e): the rounding of the product moves the result by |x| U relative.
`tolerance(ref, pre, out)` then adds the output's own rounding and doubles the sum (the factor the attention tests use): nothing in it is fitted to a kernel."""
import math

import numpy as np

from oracle.attention_ref import EPS, bits16, from_bits16, round16  # noqa: F401  (re-exported: the tests take the 16-bit helpers from here)

U = 2.0 ** -24
F16_FLOOR = 2.0 ** -25              # half the spacing of fp16 subnormals: the absolute rounding error of a result below 2^-14
F32_TINY = 2.0 ** -126              # below this f32 results are flushed or denormal
GELU_ERF_ABS = 1.5e-7               # gemm.hip: gelu_erf
FP8_MAX = 448.0
RULES = ("rope_partner32", "rope_sin_sign", "bias_after_rope", "last_k_head_plain", "first_v_head_rotated", "gate_up_swapped", "interleave32", "silu_of_up",
         "a_lo_dropped", "w_not_wrapped", "resid_no_bias", "resid_in_ignored", "resid_twice", "scale_ignored", "lse_pad_exp0", "label_next_tile", "lo_is_round_x",
         "e4m3_scale_small")


def gamma(K):
    return K * U


# ---------------------------------------------------------------------------- the product
def product(a, w, w_wrap_k=0, rule=None):
    """a [M, K], w [N, K] (w_wrap_k: a [M, 2 w_wrap_k] = [hi | lo], w [N, w_wrap_k] walked twice) -> (acc [M, N] = a . w^T, A [M, N] = sum_k |a_mk w_nk|), float64."""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    if w_wrap_k:
        assert a.shape[1] == 2 * w_wrap_k and w.shape[1] == w_wrap_k
        hi, lo = a[:, :w_wrap_k], a[:, w_wrap_k:]
        if rule == "a_lo_dropped":
            lo = np.zeros_like(lo)
        w2 = np.zeros_like(w) if rule == "w_not_wrapped" else w
        return hi @ w.T + lo @ w2.T, np.abs(hi) @ np.abs(w).T + np.abs(lo) @ np.abs(w2).T
    assert a.shape[1] == w.shape[1]
    return a @ w.T, np.abs(a) @ np.abs(w).T


# ---------------------------------------------------------------------------- weight-row layouts (gemm.hpp)
def qkv_perm_row(c):
    """gemm.hpp: stored row c' (0..127 within a q/k head) holds natural row 16 (c' >> 5) + (c' & 15) + 64 ((c' >> 4) & 1)."""
    c = np.asarray(c)
    return 16 * (c >> 5) + (c & 15) + 64 * ((c >> 4) & 1)


def qkv_row_order(nh, nkv):
    """nat[r] = the natural row of [q heads | k heads | v heads] that stored row r holds: q / k heads pair-interleaved, v heads in natural order."""
    r = np.arange((nh + 2 * nkv) * 128)
    head, c = r >> 7, r & 127
    return np.where(head < nh + nkv, head * 128 + qkv_perm_row(c), r)


def swiglu_row_order(I, group=16):
    """nat[r] = the row of the natural [gate (I rows); up (I rows)] matrix that stored row r of the fused matrix holds: `group` gate rows, `group` up rows, ..."""
    r = np.arange(2 * I)
    g, t = r // (2 * group), r % (2 * group)
    return np.where(t < group, group * g + t, I + group * g + (t - group))


def inverse(order):
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    return inv


# ---------------------------------------------------------------------------- 16-bit rules
def split16(x, dtype, rule=None):
    """The compensated outputs: hi = round16(x), lo = round16(x - hi)."""
    hi = round16(x, dtype)
    lo = round16(x, dtype) if rule == "lo_is_round_x" else round16(np.asarray(x, np.float64) - hi, dtype)
    return hi, lo


def saturate16(x, dtype, saturate=True):
    """fp16 stores of a value beyond the format: +-65504 (f16_saturate) or +-inf; NaN stays NaN."""
    r = round16(x, dtype)
    if dtype == "f16" and saturate:
        r = np.where(np.isnan(r), r, np.clip(r, -65504.0, 65504.0))
    return r


def tolerance(ref, pre, out, split=False):
    """Per-element bound on |kernel - ref|.  out "f32": 2 pre (the output is the f32 value itself).  out "f16" / "bf16": 2 (pre + eps |ref| (+ 2^-25 for fp16: a
    result in the subnormal range is rounded absolutely)).  split: the output judged on hi + lo, 2 (pre + eps^2 |ref| (+ 2^-25: the lo half underflows first))."""
    ref = np.abs(np.asarray(ref, np.float64))
    if out == "f32":
        return 2.0 * pre
    e = EPS[out] ** 2 if split else EPS[out]
    return 2.0 * (pre + e * ref + (F16_FLOOR if out == "f16" else 0.0))


# ---------------------------------------------------------------------------- elementary functions and their f32 error
def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def silu(x):
    return x * _sigmoid(x)


def silu_grad(x):
    s = _sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def sigmoid_rel_err(x):
    """Relative error of rcp(1 + __expf(-x)) in f32: exp's ((|x| + 2) U: the log2 e product, then 1 ulp) weighs (1 - sigmoid), + U for the sum, + 2 U for the rcp."""
    return ((np.abs(x) + 2.0) * (1.0 - _sigmoid(x)) + 3.0) * U


def gelu(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


def gelu_grad(x):
    x = np.asarray(x, np.float64)
    return 0.5 * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------------------- epilogues
def epi_bf16(acc, A, K, bias=None, act=0):
    """act(acc + bias); act 1 = exact-erf GELU.  Returns (ref, pre)."""
    x = acc + (0.0 if bias is None else np.asarray(bias, np.float64)[None, :])
    pre = gamma(K) * A + (U * np.abs(x) if bias is not None else 0.0)
    if act == 0:
        return x, pre
    g = gelu(x)
    # gelu_erf: erf_abs (<= 1) by the polynomial: 1.5e-7 + about ten f32 operations on values <= 1 (U each); then 0.5 x (1 + erf): three more roundings
    return g, np.abs(gelu_grad(x)) * pre + 0.5 * np.abs(x) * (GELU_ERF_ABS + 10.0 * U) + 3.0 * U * np.abs(g)


def epi_f32(acc, A, K, scale=1.0, rule=None):
    s = 1.0 if rule == "scale_ignored" else float(np.float32(scale))
    ref = acc * s
    return ref, gamma(K) * A * abs(s) + U * np.abs(ref)


def epi_resid(acc, A, K, resid, bias=None, rule=None, c_before=None):
    """resid + (acc + bias): resid = resid_in, or C's content before the call (in place).  rule "resid_in_ignored" adds c_before instead."""
    r = np.asarray(c_before if rule == "resid_in_ignored" else resid, np.float64)
    b = 0.0 if (bias is None or rule == "resid_no_bias") else np.asarray(bias, np.float64)[None, :]
    x = acc + b
    ref = r + x + (r if rule == "resid_twice" else 0.0)
    return ref, gamma(K) * A + (U * np.abs(x) if bias is not None else 0.0) + U * np.abs(ref)


def epi_qkv(acc, A, K, bias, cos, sin, nh, nkv, rule=None):
    """acc / A / bias in W's stored row order; cos / sin [M, 64]: the table rows of every row's position.  bias, then the half-split rotation (partner d + 64) on the
    q and k heads, bias only on the v heads.  Returns (ref, pre) in NATURAL column order [M, (nh + 2 nkv) 128]."""
    nat = inverse(qkv_row_order(nh, nkv))
    x = (acc + np.asarray(bias, np.float64)[None, :])[:, nat]
    e = (gamma(K) * A + U * np.abs(acc + np.asarray(bias, np.float64)[None, :]))[:, nat]
    if rule == "bias_after_rope":
        x = acc[:, nat]
    M = x.shape[0]
    nhead = nh + 2 * nkv
    x, e = x.reshape(M, nhead, 128), e.reshape(M, nhead, 128)
    half = 32 if rule == "rope_partner32" else 64
    c, s = np.asarray(cos, np.float64)[:, None, :], np.asarray(sin, np.float64)[:, None, :]
    if rule == "rope_sin_sign":
        s = -s
    out, pre = x.copy(), e.copy()
    rot = np.zeros(nhead, bool)
    rot[:nh + nkv] = True
    if rule == "last_k_head_plain":
        rot[nh + nkv - 1] = False
    if rule == "first_v_head_rotated":
        rot[nh + nkv] = True
    if half == 64:
        x1, x2, e1, e2 = x[..., :64], x[..., 64:], e[..., :64], e[..., 64:]
        lo, hi = x1 * c - x2 * s, x2 * c + x1 * s
        # two products and a sum (or an fma) in f32: U on each product and on the result
        plo = e1 * np.abs(c) + e2 * np.abs(s) + U * (np.abs(x1 * c) + np.abs(x2 * s) + np.abs(lo))
        phi = e2 * np.abs(c) + e1 * np.abs(s) + U * (np.abs(x2 * c) + np.abs(x1 * s) + np.abs(hi))
        r, p = np.concatenate([lo, hi], -1), np.concatenate([plo, phi], -1)
    else:   # wrong rule: partner d + 32 inside each half
        xr = x.reshape(M, nhead, 2, 2, 32)
        c2, s2 = c.reshape(M, 1, 2, 32), s.reshape(M, 1, 2, 32)
        lo, hi = xr[:, :, :, 0] * c2 - xr[:, :, :, 1] * s2, xr[:, :, :, 1] * c2 + xr[:, :, :, 0] * s2
        r, p = np.stack([lo, hi], 3).reshape(M, nhead, 128), e
    out[:, rot], pre[:, rot] = r[:, rot], p[:, rot]
    if rule == "bias_after_rope":
        out = out + np.asarray(bias, np.float64)[nat].reshape(1, nhead, 128)
    return out.reshape(M, -1), pre.reshape(M, -1)


def epi_swiglu(acc, A, K, rule=None):
    """acc [M, N] in the stored order (16 gate / 16 up columns interleaved) -> (silu(gate) * up [M, N / 2], pre)."""
    M, N = acc.shape
    grp = 32 if rule == "interleave32" else 16
    v, a = acc.reshape(M, N // (2 * grp), 2, grp), A.reshape(M, N // (2 * grp), 2, grp)
    g, u, eg, eu = v[:, :, 0].reshape(M, -1), v[:, :, 1].reshape(M, -1), gamma(K) * a[:, :, 0].reshape(M, -1), gamma(K) * a[:, :, 1].reshape(M, -1)
    if rule == "gate_up_swapped":
        g, u = u, g
    if rule == "silu_of_up":
        return silu(u) * g, None
    ref = silu(g) * u
    # silu_f = g * rcp(1 + __expf(-g)), times u: the sigmoid's relative error + two products.  The sigmoid itself is only good to f32's smallest normal number:
    # below g = -87.3 it is a denormal (flushed by the reciprocal), below -88.7 exp(-g) overflows and the reciprocal is 0 -- an absolute 2^-126 on it, times |g u|
    return ref, np.abs(silu_grad(g) * u) * eg + np.abs(silu(g)) * eu + (sigmoid_rel_err(g) + 2.0 * U) * np.abs(ref) + F32_TINY * (1.0 + np.abs(g * u))


def epi_lse(acc, A, K, labels, rule=None):
    """Per (row, 256-column tile): m = max, s = sum exp(x - m) over the tile's valid columns; the label's logit.  Returns a dict: m, s [M, tiles], tol_m, tol_s,
    label [M] (nan where the label is < 0 or >= N), tol_label, lse [M] = log sum exp over the row, tol_lse."""
    M, N = acc.shape
    nt = (N + 255) // 256
    e = gamma(K) * A
    m, s, tm, ts = (np.zeros((M, nt)) for _ in range(4))
    for t in range(nt):
        x, ex = acc[:, 256 * t:256 * (t + 1)], e[:, 256 * t:256 * (t + 1)]
        n = x.shape[1]
        m[:, t] = x.max(axis=1)
        em = ex.max(axis=1)                                     # the kernel's maximum is the maximum of ITS values: it moves by at most the largest error
        d = x - m[:, t:t + 1]
        p = np.exp(d)
        s[:, t] = p.sum(axis=1) + ((256 - n) if rule == "lse_pad_exp0" else 0.0)
        # every term: the argument's error (both accumulators, the subtraction, the log2 e product), then 1 ulp of v_exp_f32 -- and, as the issue of this
        # test states it, the relative error of __expf (2 U) once per term of the sum (n terms + the four-way combine with its own exps and products)
        ts[:, t] = (p * (ex + em[:, None] + 2.0 * U * np.abs(d))).sum(axis=1) + (n + 8) * 2.0 * U * s[:, t]
        tm[:, t] = em
    labels = np.asarray(labels)
    ok = (labels >= 0) & (labels < N)
    lab = np.where(ok, labels, 0)
    if rule == "label_next_tile":
        lab = np.where(lab + 256 < N, lab + 256, lab - 256 if N > 256 else lab)
        lab = np.clip(lab, 0, N - 1)
    rows = np.arange(M)
    big = acc.max(axis=1)
    lse = big + np.log(np.exp(acc - big[:, None]).sum(axis=1))
    return dict(m=m, s=s, tol_m=2.0 * tm, tol_s=2.0 * ts, label=np.where(ok, acc[rows, lab], np.nan), tol_label=2.0 * e[rows, lab],
                lse=lse, tol_lse=2.0 * (e.max(axis=1) + (ts / s).max(axis=1)))


def lse_combine(m, s):
    """log sum exp of a row from its (max, sum exp) partials, float64."""
    m, s = np.asarray(m, np.float64), np.asarray(s, np.float64)
    big = m.max(axis=1)
    return big + np.log((s * np.exp(m - big[:, None])).sum(axis=1))


# ---------------------------------------------------------------------------- the trainer's fused SwiGLU forms (EPI_BF16)
def train_swiglu_act(c16):
    """Forward: the tile is gate | up (stored order) and leaves as 16-bit values c16; act = silu(gate16) * up16 from those ROUNDED values.  Returns (ref, pre)."""
    M, N = c16.shape
    v = np.asarray(c16, np.float64).reshape(M, N // 32, 2, 16)
    g, u = v[:, :, 0].reshape(M, -1), v[:, :, 1].reshape(M, -1)
    ref = silu(g) * u
    return ref, (sigmoid_rel_err(g) + 2.0 * U) * np.abs(ref) + F32_TINY * (1.0 + np.abs(g * u))        # (the sigmoid's absolute 2^-126: epi_swiglu)


def train_swiglu_gu(acc, A, K, gu16, dtype):
    """Backward: the tile d = d act [M, I] is rounded to 16 bits on its way through LDS and never stored; the saved gate | up rows gu16 [M, 2 I] (stored order) become
    [d gate | d up] = [d u sig (1 + g (1 - sig)) | d g sig] in the same columns.  Returns (ref [M, 2 I], pre)."""
    M, I = acc.shape
    v = np.asarray(gu16, np.float64).reshape(M, I // 16, 2, 16)
    g, u = v[:, :, 0].reshape(M, I), v[:, :, 1].reshape(M, I)
    sg = _sigmoid(g)
    f = 1.0 + g * (1.0 - sg)
    ed = gamma(K) * A + EPS[dtype] * np.abs(acc) + (F16_FLOOR if dtype == "f16" else 0.0)    # d: accumulation + its 16-bit rounding
    rs = sigmoid_rel_err(g)
    ef = np.abs(g) * sg * rs + 3.0 * U * (1.0 + np.abs(g))                                     # 1 + g (1 - sig) in f32
    dg, du = acc * u * sg * f, acc * g * sg
    # (+ the sigmoid's absolute 2^-126 for very negative g, as in epi_swiglu, through both factors that hold it)
    pg = np.abs(u * sg * f) * ed + np.abs(acc * u) * sg * (ef + np.abs(f) * rs) + 3.0 * U * np.abs(dg) + F32_TINY * (1.0 + np.abs(acc * u) * (1.0 + 2.0 * np.abs(g)))
    pu = np.abs(g * sg) * ed + (rs + 2.0 * U) * np.abs(du) + F32_TINY * (1.0 + np.abs(acc * g))
    out, pre = np.stack([dg.reshape(M, I // 16, 16), du.reshape(M, I // 16, 16)], 2), np.stack([pg.reshape(M, I // 16, 16), pu.reshape(M, I // 16, 16)], 2)
    return out.reshape(M, 2 * I), pre.reshape(M, 2 * I)


# ---------------------------------------------------------------------------- e4m3 (OCP fp8, "fn": no inf, max 448) and the fused quantiser
def _e4m3_table():
    v = np.zeros(127)
    for c in range(127):
        ex, m = c >> 3, c & 7
        v[c] = m / 8.0 * 2.0 ** -6 if ex == 0 else (1.0 + m / 8.0) * 2.0 ** (ex - 7)
    return v


E4M3_VALUES = _e4m3_table()           # magnitude of codes 0 .. 126 (0x7f is NaN), increasing


def e4m3_decode(b):
    b = np.asarray(b, np.uint8)
    return np.where(b & 0x80, -1.0, 1.0) * E4M3_VALUES[np.minimum(b & 0x7f, 126)]


def e4m3_encode(x):
    """Round to the nearest e4m3 value, ties to the even code, saturating at 448."""
    x = np.asarray(x, np.float64)
    a = np.minimum(np.abs(x), FP8_MAX)
    hi = np.clip(np.searchsorted(E4M3_VALUES, a, side="left"), 0, 126)
    lo = np.maximum(hi - 1, 0)
    dl, dh = a - E4M3_VALUES[lo], E4M3_VALUES[hi] - a
    code = np.where((dh < dl) | ((dh == dl) & (hi % 2 == 0)), hi, lo)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def e4m3_ulp(a):
    """Spacing of the e4m3 grid at magnitude a (<= 448)."""
    a = np.maximum(np.abs(a), 2.0 ** -6)
    return 2.0 ** (np.floor(np.log2(a)) - 3)


def e8m0_exponent(amax, rule=None):
    """gemm.hpp / gemm.hip: the smallest e with amax 2^-e <= 448 (0 for an all-zero block), clipped to [-127, 127]."""
    amax = np.asarray(amax, np.float64)
    safe = np.where(amax > 0, amax, 1.0)
    e = np.ceil(np.log2(safe / FP8_MAX)).astype(np.int64)
    e = np.where(safe * 2.0 ** -e.astype(np.float64) > FP8_MAX, e + 1, e)
    e = np.where(safe * 2.0 ** -(e - 1).astype(np.float64) <= FP8_MAX, e - 1, e)
    e = np.where(amax > 0, np.clip(e, -127, 127), 0)
    return e - 1 if rule == "e4m3_scale_small" else e


def quant_e4m3_mx(x, rule=None):
    """x [M, C] (C % 128 == 0) -> (bytes [M, C], e [M, C / 128] exponents, dequantised values): one E8M0 scale 2^e per (row, 128 columns)."""
    x = np.asarray(x, np.float64)
    M, C = x.shape
    b = x.reshape(M, C // 128, 128)
    e = e8m0_exponent(np.abs(b).max(axis=2), rule)
    sc = 2.0 ** e.astype(np.float64)[:, :, None]
    q = e4m3_encode(b / sc)
    return q.reshape(M, C), e, (e4m3_decode(q) * sc).reshape(M, C)


def mx_index(row, kstep, mx_stride):
    """gemm.hpp (out_mx / a_mx): the byte of (row, K-step) in the E8M0 table: [K-step][256-row tile][(wm 16 + fr) 8 + mi], row in tile = 128 wm + 16 mi + fr."""
    row = np.asarray(row)
    r = row & 255
    return kstep * mx_stride + (row >> 8) * 256 + ((r >> 7) * 16 + (r & 15)) * 8 + ((r >> 4) & 7)


# ---------------------------------------------------------------------------- e2m3 operand tiles ("lo6": gemm.hpp A6 / W6 / out6)
E2M3_VALUES = np.array([m / 8.0 for m in range(8)] + [(1 + m / 8.0) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)])        # magnitude of code 0 .. 31
F6_TILE_BYTES = 25600


def e2m3_quant(x):
    """x [R, K] (K % 32 == 0) -> (codes uint8 incl. the sign bit [R, K], E8M0 bytes [R, K / 32], dequantised values): a block of 32 shares the smallest power of
    two scale with max|x| / scale <= 7.5; values round to nearest even on the e2m3 grid; an all-zero block is stored as zeros with scale byte 0."""
    x = np.asarray(x, np.float64)
    b = x.reshape(x.shape[0], -1, 32)
    amax = np.abs(b).max(axis=-1, keepdims=True)
    mant, ex = np.frexp(amax / 7.5)
    s = np.where(mant == 0.5, ex - 1, ex)
    s = np.where(amax > 0, np.clip(s, -127, 127), -127)
    a = np.minimum(np.abs(b) * np.where(amax > 0, 2.0 ** (-s.astype(np.float64)), 0.0), 7.5)
    bin_ = np.where(a < 2, 0, np.where(a < 4, 1, 2))
    q = np.rint(a * np.choose(bin_, [8.0, 4.0, 2.0])).astype(np.int64)
    code = np.minimum(q + 8 * bin_, 31)
    val = np.sign(b) * E2M3_VALUES[code] * 2.0 ** s.astype(np.float64)
    code = np.where(amax > 0, code | np.where(b < 0, 32, 0), 0)
    return code.astype(np.uint8).reshape(x.shape), (s[..., 0] + 127).astype(np.uint8), val.reshape(x.shape)


def e2m3_tiles(x, w_side):
    """The operand-tile image of x [R, K] (K % 128 == 0) as gemm.hpp lays it out: uint8 [row tiles, K / 128, 25600]; rows beyond R are zero blocks, scale byte 0."""
    x = np.asarray(x, np.float64)
    R, K = x.shape
    nt, nk = (R + 255) // 256, K // 128
    xp = np.zeros((nt * 256, K))
    xp[:R] = x
    codes, e8, _ = e2m3_quant(xp)
    e8 = e8.copy()
    e8[R:] = 0
    bits = ((codes.reshape(nt, 16, 16, nk, 4, 32)[..., None] >> np.arange(6)) & 1).astype(np.uint8)        # [tile][fb][r][step][g][j][bit]
    packed = np.packbits(bits.reshape(nt, 16, 16, nk, 4, 192), axis=-1, bitorder="little")                # 24 bytes per block
    packed = packed.transpose(0, 3, 1, 4, 2, 5)                                                            # [tile][step][fb][g][r][24]
    out = np.zeros((nt, nk, F6_TILE_BYTES), np.uint8)
    data = np.concatenate([packed[..., :16].reshape(nt, nk, 16, 1024), packed[..., 16:].reshape(nt, nk, 16, 512)], axis=-1)
    out[:, :, :24576] = data.reshape(nt, nk, 24576)
    rl = np.arange(256)
    sc = e8.reshape(nt, 256, nk, 4)
    for g in range(4):
        idx = ((rl >> 6) * 4 + g) * 64 + (rl & 15) * 4 + ((rl >> 4) & 3) if w_side else ((rl >> 7) * 4 + g) * 128 + (rl & 15) * 8 + ((rl >> 4) & 7)
        out[:, :, 24576 + idx] = sc[:, :, :, g].transpose(0, 2, 1)
    return out


# ---------------------------------------------------------------------------- the RoPE table (engine.hip: rope_table_kernel / rope_rows_kernel)
def rope_rows_layout(cos, sin, positions, stride, max_positions):
    """cos / sin [max_positions, 64] -> the chunk-major table [8 = {cos, sin} x 4 groups of 16 dims][stride][16] of the clamped positions; rows >= len(positions) nan."""
    p = np.clip(np.asarray(positions), 0, max_positions - 1)
    out = np.full((8, stride, 16), np.nan, np.float32)
    for q in range(4):
        out[q, :len(p)] = cos[p][:, 16 * q:16 * q + 16]
        out[4 + q, :len(p)] = sin[p][:, 16 * q:16 * q + 16]
    return out


def rope_rows_unpack(table, n):
    """The inverse: (cos [n, 64], sin [n, 64]) of the first n rows of a chunk-major table."""
    t = np.asarray(table)
    return np.concatenate([t[q, :n] for q in range(4)], axis=1), np.concatenate([t[4 + q, :n] for q in range(4)], axis=1)


def rope_table_tolerance(positions, theta, max_positions):
    """|cos or sin from the device's table - the float32 oracle's| <= this, per (row, dim k).  Both compute inv_k = 1 / theta^(2k/128) and ang = pos inv_k in f32 with
    different library functions: powf and the division are within 1 ulp = 2 U each on either side and the product adds U, so the angles differ by at most
    |ang| (2 (2 + 2) + 2) U = 10 |ang| U, which cos / sin pass on one to one; their own results are within 2 ulp = 4 U (|value| <= 1) on either side."""
    p = np.clip(np.asarray(positions, np.float64), 0, max_positions - 1)
    inv = 1.0 / theta ** (np.arange(0, 128, 2) / 128.0)
    return 10.0 * U * np.abs(p[:, None] * inv[None, :]) + 8.0 * U
