"""Float64 statement of the decoder's packed attention (include/blim.h: blim_batch; csrc/attention.hpp), in numpy.

Query i (index inside its sequence) of sequence s sees the prefix keys [pfx_start[s], +pfx_len[s]) and its own keys own_start[i] .. i, each restricted to
key_visible != 0; a query without a visible key gives zeros.  What the GPU tests of the attention kernel compare with (tests/test_attention_gpu.py), and what
tests/test_attention_ref.py pins to the oracle's decoder layer -- itself pinned to the reference project's goldens.

`rule` evaluates DELIBERATELY WRONG variants of the rule: the tests use them to show that their inputs tell a wrong kernel from a right one (a wrong-rule result
must leave the tolerance), never as a reference."""
import numpy as np

RULES = ("ignore_key_visible", "diag+1", "diag-1", "own_start-1", "pfx_len+1", "pfx_len-1", "no_prefix")
EPS = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}          # half an ulp of a 16-bit value relative to its binade
EMPTY_LSE = 1e30


def packed_attention(q, k, v, key_visible, seq_start, seq_len, pfx_start, pfx_len, scale, own_start=None, rule=None, pfx_all_visible=None, return_sig=False):
    """q [T, num_heads, D], k / v [T, num_kv_heads, D] (query head h reads KV head h // (num_heads / num_kv_heads)); the batch arrays as in blim_batch.
    pfx_all_visible ([n_seqs] bool, optional): sequences whose PREFIX keys ignore key_visible (the prefix-cache forms: every cached key is visible).
    Returns (out [T, num_heads, D], A [T, num_heads, D] = sum_k p_k |v_kd|, lse [T, num_heads] = natural log-sum-exp of the scaled visible scores, 1e30 for a row
    without a visible key, sub [T, num_heads] = n_sub max|v| / l: n_sub the number of visible keys whose weight is below 2^-14 of the row's largest, max|v| over
    the row's visible keys, l = sum_k exp(s_k - max) -- what `tolerance` needs for fp16); rows of no sequence are 0 everywhere.
    With return_sig also sig [T]: a number that differs between two rules exactly where the multiset of keys a query sees differs."""
    assert rule is None or rule in RULES, rule
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    T, nh, D = q.shape
    nkv = k.shape[1]
    G = nh // nkv
    vis = np.ones(T, bool) if rule == "ignore_key_visible" else np.asarray(key_visible) != 0
    out, A, lse, sub, sig = np.zeros((T, nh, D)), np.zeros((T, nh, D)), np.zeros((T, nh)), np.zeros((T, nh)), np.zeros(T)
    weight = np.random.RandomState(12345).rand(T) + 1.0
    for s in range(len(seq_start)):
        s0, n, p0, pn = int(seq_start[s]), int(seq_len[s]), int(pfx_start[s]), int(pfx_len[s])
        pidx = np.arange(p0, p0 + pn)
        if rule == "no_prefix":
            pidx = pidx[:0]
        elif rule == "pfx_len-1":
            pidx = pidx[:-1]
        elif rule == "pfx_len+1" and pn > 0:
            pidx = np.concatenate([pidx, pidx[-1:]])
        i = np.arange(n)
        first = np.zeros(n, np.int64) if own_start is None else np.asarray(own_start[s0:s0 + n], np.int64)
        if rule == "own_start-1":
            first = np.maximum(first - 1, 0)
        last = i + (1 if rule == "diag+1" else -1 if rule == "diag-1" else 0)
        pvis = np.ones(len(pidx), bool) if (pfx_all_visible is not None and pfx_all_visible[s]) else vis[pidx]
        see = np.concatenate([np.broadcast_to(pvis, (n, len(pidx))),
                              (i[None, :] <= last[:, None]) & (i[None, :] >= first[:, None]) & vis[s0:s0 + n][None, :]], axis=1)      # [n queries, keys]
        kidx = np.concatenate([pidx, s0 + i])
        sig[s0:s0 + n] = see @ weight[kidx]
        qs = q[s0:s0 + n].reshape(n, nkv, G, D)
        sc = scale * np.einsum("qgrd,kgd->grqk", qs, k[kidx])
        sc = np.where(see[None, None], sc, -np.inf)
        m = sc.max(axis=-1, keepdims=True)
        empty = ~np.isfinite(m)
        p = np.exp(sc - np.where(empty, 0.0, m))
        l = p.sum(axis=-1, keepdims=True)
        vmax = np.where(see[None, :, :], np.abs(v[kidx]).max(axis=2).T[:, None, :], 0.0).max(axis=-1)                       # [g, q]
        sub[s0:s0 + n] = ((see[None, None] & (p < 2.0 ** -14)).sum(axis=-1) * vmax[:, None, :] / np.where(empty, 1.0, l)[..., 0]).transpose(2, 0, 1).reshape(n, nh)
        p = p / np.where(empty, 1.0, l)
        tr = lambda a: a.transpose(2, 0, 1, 3).reshape(n, nh, -1)
        out[s0:s0 + n] = tr(np.einsum("grqk,kgd->grqd", p, v[kidx]))
        A[s0:s0 + n] = tr(np.einsum("grqk,kgd->grqd", p, np.abs(v[kidx])))
        lse[s0:s0 + n] = tr(np.where(empty, EMPTY_LSE, np.where(empty, 0.0, m) + np.log(np.where(empty, 1.0, l))))[..., 0]
    return (out, A, lse, sub, sig) if return_sig else (out, A, lse, sub)


def tolerance(ref, A, dtype, c_o=1.0, c_p=1.0, sub=None):
    """Per-element bound on |kernel - ref|: 2 eps (c_o |ref| + c_p A) (+ 2^-24 sub for fp16, below).  The bracket with c = 1 is the first-order worst case of ONE 16-bit rounding of every P
    (relative error eps each: sum_k p_k |v_kd| eps = eps A after normalisation) and one of the output (eps |ref|), everything else in fp32; the factor 2 covers
    the native exp2 and the accumulation order inside the MFMA.  c_p = 1/64 where P travels as hi + lo, c_o = 1/64 where the output does (moderate logits).
    fp16 (sub = packed_attention's fourth result): a P below 2^-14 of the exponent's reference is an fp16 SUBNORMAL -- spacing 2^-24, so its rounding error is up
    to 2^-25 absolute, not eps relative, and a lo part cannot carry what is below the format's smallest step either.  The MFMA keeps such operands (it does not
    flush them: the emulation with gradual underflow reproduces the hardware's error to the last digit), so every such key adds at most 2^-25 |v| / l, doubled
    like the rest: 2^-24 n_sub max|v| / l -- 1 / 1024 of the n_keys 2^-14 max|v| / l that a flushing MFMA would have needed.  Zero where no weight is that small
    (the moderate family).  bf16 has fp32's exponent range: no such term."""
    tol = 2.0 * EPS[dtype] * (c_o * np.abs(ref) + c_p * A)
    if dtype == "f16" and sub is not None:
        tol = tol + 2.0 ** -24 * np.asarray(sub)[..., None]
    return tol


def round16(x, dtype):
    """x rounded to the nearest fp16 / bf16 value (ties to even), returned as float64."""
    x = np.asarray(x, dtype=np.float64)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)
    b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64).reshape(x.shape)


def bits16(x, dtype):
    """The 16-bit patterns (uint16) of values that round16 produced."""
    x = np.asarray(x)
    if dtype == "f16":
        return x.astype(np.float16).view(np.uint16)
    return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits16(b, dtype):
    b = np.asarray(b, dtype=np.uint16)
    if dtype == "f16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def emulate_kernel(q, k, v, see, scale, dtype, q_lo=None, k_lo=None, v_lo=None, window=8.0, keep_p_lo=True):
    """One query head as csrc/attention.hip computes it, in numpy: 32-key tiles in order, the lazy reference maximum (moved when a tile's maximum exceeds it by more
    than 2^window), P rounded to 16 bits (SPLIT: hi + lo, the lo.lo terms dropped), sums in float32.  What it does not model: v_exp_f32's last bits and the order
    of accumulation inside an MFMA.  q [n, D], k / v [K, D], see [n, K] bool; the lo parts select the three-term form (a zero lo part, or keep_p_lo = False, is that form with one first-order term
    lost).  Returns the float32 result before the
    output's own rounding, [n, D]."""
    f32 = np.float32
    split = q_lo is not None
    n, nk = see.shape
    c = f32(f32(scale) * f32(1.4426950408889634))
    neg = f32(-1.0e30)
    o = np.zeros((n, q.shape[1]), f32)
    m_run = np.full(n, neg, f32)
    l_run = np.zeros(n, f32)
    for k0 in range(0, nk, 32):
        ks = slice(k0, min(k0 + 32, nk))
        s = (q @ k[ks].T)
        if split:
            s = s + q_lo @ k[ks].T + q @ k_lo[ks].T
        s = np.where(see[:, ks], s.astype(f32), neg)
        tmax = s.max(axis=1)
        move = tmax * c > m_run * c + f32(window)
        m_new = np.where(move, np.maximum(m_run, tmax), m_run)
        alpha = np.exp2(((m_run - m_new) * c).astype(np.float64)).astype(f32)
        l_run = l_run * alpha
        o = o * alpha[:, None]
        mc = np.where(m_new > f32(0.5) * neg, m_new * c, f32(0))
        with np.errstate(under="ignore"):
            e = np.exp2((s * c - mc[:, None]).astype(np.float64)).astype(f32)
        l_run = l_run + e.sum(axis=1, dtype=f32)
        m_run = m_new
        p_hi = round16(e, dtype)
        pv = p_hi @ v[ks]
        if split:
            p_lo = round16(e.astype(np.float64) - p_hi, dtype) if keep_p_lo else np.zeros_like(p_hi)
            pv = pv + p_lo @ v[ks] + p_hi @ v_lo[ks]
        o = (o + pv.astype(f32)).astype(f32)
    inv = np.where(l_run > 0, f32(1) / np.where(l_run > 0, l_run, f32(1)), f32(0))
    return o * inv[:, None]
