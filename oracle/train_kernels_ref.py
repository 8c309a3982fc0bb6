"""Float64 statements of the trainer's small kernels (csrc/train_kernels.hip: lora_down, lora_wgrad (dB, dA), lora_du, lora_dx, rmsnorm_bwd plain and fused,
ce_fwd_bwd, gelu, adamw, grad_stats), in plain numpy, each with a per-element bound on |kernel - reference|.  The only source of tolerances of
tests/test_train_kernels_gpu.py; tests/test_train_kernels_ref.py pins every function to torch float64 autograd / torch.optim.AdamW and shows that the bounds hold an
emulation of the kernels' roundings and reject the wrong rules (RULES) on the GPU tests' inputs.

    tol = 2 * (sum of the named first-order terms)            -- the project's factor 2 (oracle/attention_ref.tolerance, oracle/attention_bwd_ref.py)

Every bound is formed from the reference's own magnitudes; nothing is fitted to a kernel's output.  U = 2^-24 is one f32 rounding, eps = EPS[dtype] half an ulp of
a 16-bit value.  The terms:
  A_round, Bt_round, xm_round   The 16-bit roundings of A (lora_a16), B^T (lora_bt) and drop(x) * m are part of the OPERATION: round-to-nearest-even of an f32
                is a function, so the reference applies it (A16 = round16(A), xs = round16(fl32(x * m)) with m = fl32(1 / (1 - p))) and the terms contribute 0.
                That is what makes the wrong rule `A_unrounded` visible.  The products of two 16-bit values are exact in f32.
  out16         every 16-bit output: err16(|ref| + pre) -- eps relative, and for fp16 at least 2^-25 for a non-zero value (subnormal spacing 2^-24 below 2^-14);
                `pre` is the error of the f32 value that is rounded.
  f32           accumulation in f32: n U sum |a| |b| with n the length of the longest chain of additions the code forms (the MFMA K loop of a split, the
                partial sums, the block reduction's 4 ceil(H / 1024) + 9 levels), plus one U per further f32 operation, relative to its result.
  dA_split      du enters as hi = round16(du / 256), lo = round16(du - 256 hi): |du - 256 hi - lo| is evaluated exactly (du / 256 and du - 256 hi are exact in
                f32), fp16 subnormal spacing included -- for fp16 a du of 1e-3 has a subnormal hi AND lo, error up to 2^-25 absolute = 3e-5 relative.
  rsqrt         rsqrtf: 2 ulp = 4 U relative.       div: 1 ulp = 2 U.
  exp_native    __expf(a) = v_exp_f32(a log2 e): the product's rounding is an absolute error U |a log2 e| of the exponent, i.e. relative U |a| of the result, the
                instruction adds 2 ulp: (|a| + 4) U, plus U |a| for the subtraction that formed a; results below 2^-126 may be flushed: + 2^-126 absolute.
  log_native    __logf(s) = v_log_f32(s) ln 2: 4 U |log s| + the error of s.
  erf           erff: 4 ulp = 8 U relative, and the argument x / sqrt 2 carries 2 U: |erf'(z)| |z| 2 U.
  cancel        rs w dy - x c: each product carries its own relative error, so the bound is on the magnitudes of the two terms, never on their difference.
  bias_corr     AdamW's 1 - powf(beta, step) comes from the host's powf: 2 U beta^t / (1 - beta^t) relative.
"""
import math
import types

import numpy as np

from oracle.attention_ref import EPS, round16
from oracle.train_oracle import drop_mult

U = 2.0 ** -24
TINY = 2.0 ** -126
RULES = ("lo_dropped", "A_unrounded", "mask_site_plus1", "mask_ldx", "c_no_H", "rs2", "accumulate_ignored", "label_div_ignored", "pad_not_zeroed",
         "du_accumulated", "dA_not_transposed", "kslice_skipped", "tsplit_skipped")
TSPLIT = 1024                        # lora_wgrad_kernel: rows per time split
f32 = np.float32


def err16(x, dtype):
    """Bound on |16-bit(x) - x|: eps |x|; fp16: at least 2^-25 for a non-zero x (subnormal spacing)."""
    a = np.abs(np.asarray(x, np.float64))
    e = EPS[dtype] * a
    return np.maximum(e, np.where(a > 0, 2.0 ** -25, 0.0)) if dtype == "f16" else e


def store16(ref, pre, dtype):
    """Error of a 16-bit store of an f32 value that is `pre` off the reference: the rounding of a value of that size, plus pre."""
    return err16(np.abs(ref) + pre, dtype) + pre


def keep_mult(p):
    return float(f32(1.0) / (f32(1.0) - f32(p)))


def mask(seed, site, T, K, p, stride=None):
    """drop_mult4's multipliers of rows [0, T) x columns [0, K) (float64 of the f32 values); stride: the row stride of the element index (K in every kernel)."""
    if p <= 0.0:
        return np.ones((T, K))
    return drop_mult(seed, site, T, K if stride is None else stride, 0, p).astype(np.float64)[:, :K]


def dropped(x, m, dtype):
    """round16(fl32(x * m)): x 16-bit values, m the f32 multipliers -- the product is formed in f32, then stored as 16 bits (exactly what every kernel does)."""
    return round16((np.asarray(x, f32) * np.asarray(m, f32)).astype(np.float64), dtype)


def du_splits(T, Np):
    """csrc/train_kernels.hip: lora_du_splits -> (steps per slice, slices) for Np = round_up(N, 16) columns."""
    row_blocks, steps = (T + 127) // 128, Np // 16
    n_split = max(1, min((1024 + row_blocks - 1) // row_blocks, (steps + 15) // 16))
    per = (steps + n_split - 1) // n_split
    return per, (steps + per - 1) // per


def _red_depth(n_per_thread):
    """Longest chain of f32 additions of a 256-thread block reduction: the thread's own terms, six shuffle levels, three adds of the wave sums."""
    return n_per_thread + 9


# ---------------------------------------------------------------------------- LoRA
def lora_down(x, A, r, scale, p, seed, site, dtype, ldx=None, rule=None):
    """x [T, K] 16-bit values, A a list of f32 [r, K] -> (u [T, n r], tol): u[t, seg r + j] = fl32(scale) sum_k xs_seg[t, k] A16_seg[j, k], stored as 16 bits."""
    x = np.asarray(x, np.float64)
    T, K = x.shape
    sc = float(f32(scale))
    u, pre = np.zeros((T, len(A) * r)), np.zeros((T, len(A) * r))
    for seg, Aseg in enumerate(A):
        A16 = np.asarray(Aseg, np.float64) if rule == "A_unrounded" else round16(Aseg, dtype)
        m = mask(seed, site + (0 if rule == "mask_site_plus1" else seg), T, K, p, stride=ldx if rule == "mask_ldx" else None)
        xs = dropped(x, m, dtype) if p > 0.0 else x
        if rule == "kslice_skipped":                 # the last of the four waves' K slices never summed
            steps = K // 16
            per = (steps + 3) // 4
            xs = xs.copy()
            xs[:, 16 * min(steps - 1, 3 * per):] = 0.0
        u[:, seg * r:(seg + 1) * r] = sc * (xs @ A16.T)
        pre[:, seg * r:(seg + 1) * r] = (16 * -(-(K // 16) // 4) + 4) * U * abs(sc) * (np.abs(xs) @ np.abs(A16).T)      # f32: a wave's share of the K products, 3 adds, scale
    return u, 2.0 * store16(u, pre, dtype)


def lora_dB(dy, u, dB0, rule=None):
    """dy [T, N], u [T, r] 16-bit values, dB0 f32 [N, r] -> (dB, tol): dB = dB0 + dy^T u, f32 partial sums per 1,024-row split added in split order."""
    dy, u, dB0 = (np.asarray(a, np.float64) for a in (dy, u, dB0))
    T = dy.shape[0]
    if rule == "tsplit_skipped":
        dy = dy.copy()
        dy[TSPLIT:2 * TSPLIT] = 0.0
    ns = -(-T // TSPLIT)
    n = min(T, TSPLIT) + ns + 1
    return dB0 + dy.T @ u, 2.0 * n * U * (np.abs(dB0) + np.abs(dy).T @ np.abs(u))


def split_hilo(du, dtype):
    """(hi, lo) of the kernel's du split, float64 of the 16-bit values: hi = round16(du / 256), lo = round16(du - 256 hi)."""
    du = np.asarray(du, np.float64)
    hi = round16(du / 256.0, dtype)
    return hi, round16(du - 256.0 * hi, dtype)


def lora_dA(du, x, dA0, p, seed, site, dtype, ldx=None, rule=None):
    """du f32 [T, r], x [T, K] 16-bit values, dA0 f32 [r, K] -> (dA [r, K], tol): dA = dA0 + du^T drop(x)."""
    du, x, dA0 = (np.asarray(a, np.float64) for a in (du, x, dA0))
    T, K = x.shape
    r = du.shape[1]
    m = mask(seed, site + (1 if rule == "mask_site_plus1" else 0), T, K, p, stride=ldx if rule == "mask_ldx" else None)
    xs = dropped(x, m, dtype) if p > 0.0 else x
    hi, lo = split_hilo(du, dtype)
    ns = -(-T // TSPLIT)
    n = min(T, TSPLIT) + ns + 3                                   # the split's MFMA chain, 256 acc_hi + acc_lo, the ordered sum
    ax = np.abs(xs)
    tol = 2.0 * (np.abs(du - 256.0 * hi - lo).T @ ax + n * U * (np.abs(dA0) + (256.0 * np.abs(hi) + np.abs(lo)).T @ ax))
    if rule == "lo_dropped":
        return dA0 + (256.0 * hi).T @ xs, tol
    if rule == "tsplit_skipped":
        du = du.copy()
        du[TSPLIT:2 * TSPLIT] = 0.0
    out = dA0 + du.T @ xs
    if rule == "dA_not_transposed":
        out = dA0 + (xs.T @ du).reshape(r, K)                     # the [K, r] layout written into the [r, K] array
    return out, tol


def lora_du(dy, B, scale, dtype, du0=None, rule=None):
    """dy [T, Np] 16-bit values (columns N.. zero), B f32 [N, r] -> (du [T, r], tol): du = fl32(scale) dy Bt16^T, OVERWRITTEN (du0 is what the array held)."""
    dy = np.asarray(dy, np.float64)
    T, N = dy.shape[0], B.shape[0]
    B16 = round16(B, dtype)
    sc = float(f32(scale))
    per, ns = du_splits(T, -(-N // 16) * 16)
    du = sc * (dy[:, :N] @ B16)
    if rule == "du_accumulated":
        du = du + np.asarray(du0, np.float64)
    return du, 2.0 * (16 * per + ns + 2) * U * abs(sc) * (np.abs(dy[:, :N]) @ np.abs(B16))


def _dx_term(du, A, r, p, seed, site, T, K, rule=None):
    """sum_seg m_seg o (du_seg A_seg) and the bound on its f32 evaluation (2 r roundings per dot product, the mask product, the sum over the adapters)."""
    l, mag = np.zeros((T, K)), np.zeros((T, K))
    for seg in range(len(A)):
        m = mask(seed, site + (0 if rule == "mask_site_plus1" else seg), T, K, p)
        d, a = np.asarray(du[seg], np.float64), np.asarray(A[seg], np.float64)
        l += m * (d @ a)
        mag += m * (np.abs(d) @ np.abs(a))
    return l, (2 * r + len(A) + 1) * U * mag


def lora_dx(dx0, du, A, r, p, seed, site, dtype=None, rule=None):
    """dx0 f32 [T, K], du list of f32 [T, r], A list of f32 [r, K] -> (dx, tol, tol16): dx = dx0 + the adapters' term; tol16 the bound of the 16-bit form."""
    dx0 = np.asarray(dx0, np.float64)
    T, K = dx0.shape
    l, pre = _dx_term(du, A, r, p, seed, site, T, K, rule)
    dx = dx0 + l
    pre = pre + U * (np.abs(dx0) + np.abs(l))
    return dx, 2.0 * pre, (2.0 * store16(dx, pre, dtype) if dtype else None)


# ---------------------------------------------------------------------------- RMSNorm backward
def rmsnorm_bwd(dy, x, w, eps, prior=None, dtype=None, lora=None, rule=None):
    """dy, x f32 [n, H] (x already gathered), w f32 [H]; prior: what dx held (accumulate) or None; lora = (du, A, r, p, seed, site): the fused adapters.
    Returns (dx, tol, tol16): dx = rs w d - x c (+ prior), rs = rsqrt(mean x^2 + eps), c = rs^3 sum(w d x) / H, d = dy (+ the adapters' term)."""
    dy, x, w = (np.asarray(a, np.float64) for a in (dy, x, w))
    n, H = x.shape
    d, dd = dy, np.zeros_like(dy)
    if lora is not None:
        du, A, r, p, seed, site = lora
        l, dd = _dx_term(du, A, r, p, seed, site, n, H, rule)
        d = dy + l
        dd = dd + U * (np.abs(dy) + np.abs(l))
    depth = _red_depth(4 * -(-H // 1024)) + 1
    fe = float(f32(eps))
    ss = (x * x).sum(1, keepdims=True)
    dot = (w * d * x).sum(1, keepdims=True)
    var = ss / H + fe
    rs = var ** -0.5
    e_rs = 0.5 * ((depth * U * ss / H + 3 * U * var) / var) + 4 * U                         # relative: the sum, / H and + eps, rsqrt
    e_dot = (depth + 3) * U * np.abs(w * d * x).sum(1, keepdims=True) + (np.abs(w * x) * dd).sum(1, keepdims=True)
    c = (rs ** (2 if rule == "rs2" else 3)) * dot / (1.0 if rule == "c_no_H" else H)
    c_true = rs ** 3 * dot / H
    e_c = np.abs(c_true) * (3 * e_rs + 5 * U) + rs ** 3 / H * e_dot
    t1, t2 = rs * w * d, x * c
    g = t1 - t2
    pre = np.abs(rs * w * d) * (e_rs + 3 * U) + rs * np.abs(w) * dd + np.abs(x) * e_c + U * np.abs(x * c_true) + U * np.abs(g)      # cancel: both magnitudes
    if prior is not None and rule != "accumulate_ignored":
        g = g + np.asarray(prior, np.float64)
    if prior is not None:
        pre = pre + U * (np.abs(prior) + np.abs(t1 - x * c_true))
    return g, 2.0 * pre, (2.0 * store16(g, pre, dtype) if dtype else None)


# ---------------------------------------------------------------------------- cross-entropy
def ce_fwd_bwd(logits, labels, label_div, coef, ldd, loss0, dtype=None, pad=None, rule=None):
    """logits f32 [R, V], labels int [ceil(R / label_div)] -> namespace: d [R, ldd] = coef (softmax - onehot), columns V.. zero, an all-zero row for a label outside
    [0, V); loss = loss0 + sum of the row losses; tol_d (f32 form), tol_d16 (with dtype), tol_loss, row_loss.  pad: what the padding columns held (pad_not_zeroed)."""
    lg = np.asarray(logits, np.float64)
    R, V = lg.shape
    lab = np.asarray(labels)[np.minimum(np.arange(R) // (1 if rule == "label_div_ignored" else label_div), len(labels) - 1)]
    ok = (lab >= 0) & (lab < V)
    co = float(f32(coef))
    mx = lg.max(1, keepdims=True)
    a = lg - mx
    e = np.exp(a)
    s = e.sum(1, keepdims=True)
    rel_e = (2 * np.abs(a) + 4) * U
    depth = _red_depth(-(-V // 256))
    e_s = (e * rel_e).sum(1, keepdims=True) + V * TINY + depth * U * s
    prob = e / s
    e_p = prob * (rel_e + e_s / s + 4 * U) + TINY
    onehot = np.zeros((R, V))
    onehot[np.arange(R)[ok], lab[ok]] = 1.0
    d = np.zeros((R, ldd))
    diff = prob - onehot
    diff[onehot == 1] = -((e * (1.0 - onehot)).sum(1) / s[:, 0])[ok]          # p - 1 = -(the other columns' share): no cancellation in the reference itself
    d[:, :V] = np.where(ok[:, None], co * diff, 0.0)
    if rule == "pad_not_zeroed":
        d[:, V:] = pad
    pre = np.zeros((R, ldd))
    pre[:, :V] = np.where(ok[:, None], abs(co) * (e_p + U * np.abs(diff)) + U * np.abs(d[:, :V]), 0.0)
    lab_c = np.where(ok, lab, 0)
    ll = a[np.arange(R), lab_c][:, None]
    row = np.where(ok[:, None], -(ll - np.log(s)), 0.0)[:, 0]
    e_row = np.where(ok[:, None], 2 * U * np.abs(ll) + 4 * U * np.abs(np.log(s)) + e_s / s + 2 * U * np.abs(ll - np.log(s)), 0.0)[:, 0]
    total = float(f32(loss0)) + row.sum()
    tol_loss = 2.0 * (e_row.sum() + _red_depth(-(-R // 256)) * U * np.abs(row).sum() + U * (abs(float(loss0)) + abs(total)))
    return types.SimpleNamespace(d=d, tol_d=2.0 * pre, tol_d16=(2.0 * store16(d, pre, dtype) if dtype else None), loss=total, tol_loss=tol_loss, row_loss=row, ok=ok)


# ---------------------------------------------------------------------------- GELU
_erf = np.vectorize(math.erf, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def gelu(x, dtype, dh=None):
    """x 16-bit values; forward: (x Phi(x), tol); backward (dh f32): (dh (Phi(x) + x phi(x)), tol).  Both are stored as 16 bits."""
    x = np.asarray(x, np.float64)
    z = x / math.sqrt(2.0)
    cdf = 0.5 * _erfc(-z)                                        # = 0.5 (1 + erf z) without the cancellation
    erf = _erf(z)
    e_cdf = 0.5 * (8 * U * np.abs(erf) + 2.0 / math.sqrt(math.pi) * np.exp(-z * z) * np.abs(z) * 2 * U + U * (1.0 + np.abs(erf))) + U * cdf
    if dh is None:
        y = x * cdf
        return y, 2.0 * store16(y, np.abs(x) * e_cdf + U * np.abs(y), dtype)
    dh = np.asarray(dh, np.float64)
    a = -0.5 * x * x
    phi = np.exp(a) / math.sqrt(2.0 * math.pi)
    e_phi = phi * ((np.abs(a) + 4 + 2) * U + 2 * U) + TINY
    gp = cdf + x * phi
    y = dh * gp
    pre = np.abs(dh) * (e_cdf + np.abs(x) * e_phi + U * np.abs(x * phi) + U * np.abs(gp)) + U * np.abs(y)
    return y, 2.0 * store16(y, pre, dtype)


# ---------------------------------------------------------------------------- AdamW, gradient statistics
def bias_corrections(b1, b2, step):
    """(c1, c2) as blim_adamw_raw forms them: 1 - powf(beta, step) in f32."""
    return float(f32(1.0) - f32(f32(b1) ** f32(step))), float(f32(1.0) - f32(f32(b2) ** f32(step)))


def adamw(p, g, m, v, lr, b1, b2, eps, wd, inv_scale, step):
    """One step on f32 arrays (csrc/train.hpp): gr = g inv_scale; p *= 1 - lr wd; m, v updated; p -= lr / c1 * m / (sqrt(v) / sqrt(c2) + eps).
    Returns a namespace p, m, v, tol_p, tol_m, tol_v."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, inv = (float(f32(a)) for a in (lr, b1, b2, eps, wd, inv_scale))
    c1, c2 = bias_corrections(b1, b2, step)
    gr = g * inv
    pv = p * (1.0 - lr * wd)
    mv = b1 * m + (1.0 - b1) * gr
    vv = b2 * v + (1.0 - b2) * gr * gr
    e_m = 4 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * gr))
    e_v = 6 * U * (b2 * v + (1.0 - b2) * gr * gr)
    root = np.sqrt(vv)
    den = root / math.sqrt(c2) + eps
    e_root = np.where(vv > 0, 0.5 * e_v / np.where(vv > 0, root, 1.0), np.sqrt(e_v)) + U * root
    e_den = (e_root + root * (4 * U + U * b2 ** step / c2)) / math.sqrt(c2) + U * den
    upd = (lr / c1) * mv / den
    e_upd = (lr / c1) / den * e_m + np.abs(upd) * (e_den / den + 4 * U + 2 * U * b1 ** step / c1)
    pn = pv - upd
    return types.SimpleNamespace(p=pn, m=mv, v=vv, tol_p=2.0 * (3 * U * np.abs(pv) + e_upd + U * np.abs(pn)), tol_m=2.0 * e_m, tol_v=2.0 * e_v)


def grad_stats(g, inv_scale, stats0):
    """stats[0] = stats0[0] + sum (g inv_scale)^2; stats[1] = 1 when any v = fl32(g inv_scale) fails |v| <= 3.0e38f (the kernel's test: inf, NaN, and
    the finite values between 3.0e38 and FLT_MAX), else stats0[1] untouched.  Returns (stats [2], tol of stats[0])."""
    g = np.asarray(g, np.float64)
    n = g.size
    grid = min(1024, -(-n // 256))
    with np.errstate(over="ignore", invalid="ignore"):
        vsq = (g * float(f32(inv_scale))) ** 2
        bad = not (np.abs(np.asarray(g, f32) * f32(inv_scale)) <= f32(3.0e38)).all()
        total = vsq.sum()
    depth = _red_depth(-(-n // (256 * grid))) + _red_depth(-(-grid // 256)) + 1
    s0 = float(stats0[0]) + total
    tol = 2.0 * ((depth + 3) * U * total + U * (abs(float(stats0[0])) + abs(s0)))
    return np.array([s0, 1.0 if bad else float(stats0[1])]), tol
