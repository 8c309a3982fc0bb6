"""Float64 statement of the trainer's attention backward (csrc/train.hpp: AttnBwdParams; csrc/train_kernels.hip) and of the RoPE backward that follows it, in numpy.

packed_attention_bwd is the exact backward of oracle/attention_ref.packed_attention without prefixes and with own_start = 0: per sequence and query head,
P = softmax(scale q.k) over the visible keys j <= i,  dV = sum over the group's heads of P^T dO,  dP = dO V^T,  D = rowsum(P o dP),  dS = scale P o (dP - D),
dQ = dS K,  dK = sum over the group's heads of dS^T Q.  tests/test_attention_bwd_ref.py pins it to central finite differences of packed_attention and to
torch.autograd; tests/test_attention_bwd_gpu.py compares the kernels with it per element.

`rule` evaluates DELIBERATELY WRONG variants (RULES): the tests use them to show that their inputs tell a wrong kernel from a right one, never as a reference.
keys_to_round32 is not read literally: keys L .. round_up(L, 32) counted as visible would change nothing, because a query i < L never sees a key j > i.  What a
contraction that runs to round_up(L, 32) without its `i < L` guard does (attn_tn_kernel stages 32 query rows at a time) is let the ROWS L .. round_up(L, 32) --
tokens behind the sequence -- join the sums of dK and dV as queries over the sequence's keys; that is the rule evaluated under this name."""
import types

import numpy as np

from oracle import attention_ref as R
from oracle import gemm_ref as G

RULES = ("ignore_key_visible", "diag+1", "diag-1", "no_D", "scale_twice", "group_first_head_only", "kv_head_mod", "lse_other_head", "keys_to_round32")
EPS = R.EPS
U = 2.0 ** -24                      # one f32 rounding, relative
TERMS = ("P_round", "dS_round", "D_o16", "P_sub", "dS_sub", "f32", "lse_f32")


def _err16(x, dtype, drop, name):
    """Bound on |16-bit(x) - x|: eps |x| (term `name`_round), and for fp16 at least 2^-25 for a non-zero x (term `name`_sub): below 2^-14 fp16 is subnormal, spacing
    2^-24, and the MFMA keeps such operands (profiles/r12_attention_direct.md), so the error is absolute there.  bf16 has fp32's exponent range: no such part."""
    a = np.abs(x)
    rel = np.zeros_like(a) if name + "_round" in drop else EPS[dtype] * a
    if dtype != "f16" or name + "_sub" in drop:
        return rel
    return rel + np.where(a > 0, np.maximum(2.0 ** -25 - EPS[dtype] * a, 0.0), 0.0)


def packed_attention_bwd(q, k, v, dout, key_visible, seq_start, seq_len, scale, rule=None, dtype=None, drop=(), o_err=None, lse_err=None):
    """q, dout [T, num_heads, D], k, v [T, num_kv_heads, D] (query head h belongs to KV head h // (num_heads / num_kv_heads)); key_visible [T], seq_start / seq_len as
    in blim_batch.  Returns a namespace with dq [T, num_heads, D], dk, dv [T, num_kv_heads, D] (zero on rows without a visible key and on tokens of no sequence),
    out, lse (packed_attention's: what the kernel is given as o16 and lse), sig_q / sig_k [T] (numbers that differ between two rules exactly where the set of keys
    a query sees, resp. the set of (query, its visible set) that see a key, differs), nvis [T] (visible keys per query), seen2 [T] (the key is seen by a query with
    two or more visible keys), and -- with dtype ("f16" / "bf16") -- tol_dq, tol_dk, tol_dv, the per-element bound on |kernel - reference|:

        tol = 2 * (sum over the contraction of the first-order error of each 16-bit operand times the magnitude of the other operand + the f32 accumulation)

    with these terms (TERMS; `drop` leaves named ones out -- the tests use that to show which ones the emulation needs):
      P_round   one 16-bit rounding of every P: eps P.  Reaches dV as eps sum_i P_ij |dO_id| and, through dS = scale P (dP - D), dQ and dK as eps |dS| |K| / |Q|.
      dS_round  one 16-bit rounding of every dS: eps |dS|.
      D_o16     D is formed from the 16-bit forward output: |D - rowsum(P o dP)| <= sum_d |dO_d| o_err_d with o_err = eps |O| (or what the caller states for an
                output that a kernel wrote); enters dS as scale P times that.
      P_sub, dS_sub   fp16 only: a non-zero P or dS below 2^-14 is rounded with an ABSOLUTE error up to 2^-25 (_err16).
      f32       P's exponent scale q.k - lse is formed in f32: the 128-term accumulation (128 U scale sum_d |q_d k_d|), the product with scale, the subtraction
                (U each, relative to their results); dP likewise (128 U sum_d |dO_d v_d|), D's own sum (128 U sum_d |dO_d O_d|), the three f32 operations of the dS
                epilogue (3 U |dS|), and the accumulation of the three products over their contraction length n: n U sum |a| |b|.
      lse_f32   lse travels as f32: lse_err = U |lse| by default (the nearest f32 of the reference's lse), relative error of P of that size.
    The overall factor 2 covers the native exp and the accumulation order inside the MFMA (attention_ref.tolerance's precedent)."""
    assert rule is None or rule in RULES, rule
    q, k, v, dout = (np.asarray(a, dtype=np.float64) for a in (q, k, v, dout))
    T, nh, D = q.shape
    nkv = k.shape[1]
    Gq = nh // nkv
    vis = np.ones(T, bool) if rule == "ignore_key_visible" else np.asarray(key_visible) != 0
    z = np.zeros((len(seq_start),), np.int32)
    out, _, lse, _ = R.packed_attention(q, k, v, key_visible, seq_start, seq_len, z, z, scale)        # the RIGHT forward: what every variant is handed
    r = types.SimpleNamespace(dq=np.zeros((T, nh, D)), dk=np.zeros((T, nkv, D)), dv=np.zeros((T, nkv, D)), out=out, lse=lse, sig_q=np.zeros(T), sig_k=np.zeros(T),
                              nvis=np.zeros(T, np.int64), seen2=np.zeros(T, bool))
    want_tol = dtype is not None
    if want_tol:
        r.tol_dq, r.tol_dk, r.tol_dv = np.zeros((T, nh, D)), np.zeros((T, nkv, D)), np.zeros((T, nkv, D))
        eps = EPS[dtype]
        o_err_ = eps * np.abs(out) if o_err is None else np.asarray(o_err, np.float64)
        lse_err_ = U * np.abs(lse) if lse_err is None else np.asarray(lse_err, np.float64)
        f32 = 0.0 if "f32" in drop else 1.0
    weight = np.random.RandomState(12345).rand(T) + 1.0
    weight2 = np.random.RandomState(54321).rand(T) + 1.0
    kv_of = (lambda h: h % nkv) if rule == "kv_head_mod" else (lambda h: h // Gq)
    for s in range(len(seq_start)):
        s0, L = int(seq_start[s]), int(seq_len[s])
        n = min((L + 31) // 32 * 32, T - s0) if rule == "keys_to_round32" else L      # the wrong rule: the rows up to the next multiple of 32 take part as queries
        if n == 0:
            continue
        i = np.arange(n)
        last = i + (1 if rule == "diag+1" else -1 if rule == "diag-1" else 0)
        see = (i[None, :] <= last[:, None]) & vis[s0:s0 + n][None, :]                 # [query, key]
        if rule == "keys_to_round32":
            see[:, L:] = False                                                        # ... over the sequence's own keys
        sl = slice(s0, s0 + n)
        r.sig_q[sl][:L] = (see @ weight[sl])[:L]
        r.sig_k[s0:s0 + L] = ((see * (see @ weight[sl])[:, None] * weight2[sl][:, None]).sum(axis=0))[:L]
        nv = see.sum(axis=1)
        r.nvis[s0:s0 + L] = nv[:L]
        r.seen2[s0:s0 + L] = (see & (nv >= 2)[:, None]).any(axis=0)[:L]
        for h in range(nh):
            g = kv_of(h)
            Q, K, V, dO = q[sl, h], k[sl, g], v[sl, g], dout[sl, h]
            sc = scale * (Q @ K.T)
            if rule in ("ignore_key_visible", "diag+1", "diag-1", "keys_to_round32"):   # variants whose rows differ: their own softmax
                m = np.where(see, sc, -np.inf).max(axis=1, keepdims=True)
                m = np.where(np.isfinite(m), m, 0.0)
                e = np.where(see, np.exp(np.where(see, sc, 0.0) - m), 0.0)
                l = e.sum(axis=1, keepdims=True)
                row_lse = np.where(l > 0, m + np.log(np.where(l > 0, l, 1.0)), R.EMPTY_LSE)[:, 0]
            else:
                row_lse = lse[sl, (h + 1) % nh if rule == "lse_other_head" else h]
            with np.errstate(over="ignore"):
                P = np.where(see, np.exp(np.minimum(np.where(see, sc, 0.0) - row_lse[:, None], 80.0)), 0.0)
            dP = dO @ V.T
            Drow = (P * dP).sum(axis=1) if rule in ("ignore_key_visible", "diag+1", "diag-1", "keys_to_round32") else (dO * out[sl, h]).sum(axis=1)
            dS = scale * P * (dP if rule == "no_D" else dP - Drow[:, None])
            if rule == "scale_twice":
                dS = scale * dS
            r.dq[s0:s0 + L, h] = (dS @ K)[:L]
            if not (rule == "group_first_head_only" and h % Gq != 0):
                r.dk[s0:s0 + L, g] += (dS.T @ Q)[:L]
                r.dv[s0:s0 + L, g] += (P.T @ dO)[:L]
            if want_tol and rule is None:
                aK, aQ, adO = np.abs(K), np.abs(Q), np.abs(dO)
                d_logit = f32 * U * (128 * scale * (aQ @ aK.T) + np.abs(sc) + np.abs(sc - row_lse[:, None])) + (0.0 if "lse_f32" in drop else lse_err_[sl, h][:, None])
                eP = np.where(see, _err16(P, dtype, drop, "P") + P * d_logit, 0.0)
                d_D = (0.0 if "D_o16" in drop else (adO * o_err_[sl, h]).sum(axis=1)) + f32 * 128 * U * (adO * np.abs(out[sl, h])).sum(axis=1)
                d_dP = f32 * 128 * U * (adO @ np.abs(V).T)
                eS = np.where(see, _err16(dS, dtype, drop, "dS") + scale * np.abs(dP - Drow[:, None]) * eP + scale * P * (d_D[:, None] + d_dP) + f32 * 3 * U * np.abs(dS), 0.0)
                aS = np.abs(dS)
                r.tol_dq[sl, h] = 2.0 * (eS @ aK + f32 * L * U * (aS @ aK))
                r.tol_dk[sl, g] += 2.0 * (eS.T @ aQ + f32 * L * Gq * U * (aS.T @ aQ))
                r.tol_dv[sl, g] += 2.0 * (eP.T @ adO + f32 * L * Gq * U * (P.T @ adO))
    return r


def emulate_kernel(q, k, v, dout, o16, lse32, see, scale, dtype):
    """One KV head's group as csrc/train_kernels.hip computes it, in numpy: q, dout, o16 [G, n, D] (16-bit values), k, v [n, D], lse32 [G, n] (float32), see [n, n]
    bool.  P16 = 16-bit(exp(f32(scale q.k) - lse)), D = f32 sum(dO o o16), dS16 = 16-bit(scale P16 (dP - D)) from the P16 that is read back, the products as f32
    sums.  What it does not model: __expf's last bits and the order of accumulation inside an MFMA.  Returns (dq [G, n, D], dk [n, D], dv [n, D]) as float32."""
    f32 = np.float32
    sc_ = f32(scale)
    Gq, n, Dh = q.shape
    dq, dk, dv = np.zeros((Gq, n, Dh), f32), np.zeros((n, Dh)), np.zeros((n, Dh))
    for h in range(Gq):
        s = (q[h] @ k.T).astype(f32)
        with np.errstate(under="ignore", over="ignore"):
            x = (s * sc_ - lse32[h][:, None].astype(f32)).astype(f32)
            p = np.where(see, np.exp(x.astype(np.float64)).astype(f32), f32(0))
        P16 = R.round16(p, dtype)
        Dr = (dout[h] * o16[h]).sum(axis=1).astype(f32)
        dP = (dout[h] @ v.T).astype(f32)
        dS = ((sc_ * P16.astype(f32)).astype(f32) * (dP - Dr[:, None]).astype(f32)).astype(f32)
        dS16 = np.where(see, R.round16(dS, dtype), 0.0)
        dq[h] = (dS16 @ k).astype(f32)
        dk += dS16.T @ q[h]
        dv += P16.T @ dout[h]
    return dq, dk.astype(f32), dv.astype(f32)


# ---------------------------------------------------------------------------- RoPE backward (train_kernels.hip: rope_bwd_kernel)
def rope_fwd(x, cos, sin, nh, nkv):
    """The float64 RoPE that gemm_ref.epi_qkv states for the QKV epilogue, on x [T, (nh + 2 nkv) 128] in natural column order, cos / sin [T, 64]: a product with
    the identity (no bias, no accumulation error) through epi_qkv itself."""
    x = np.asarray(x, np.float64)
    order = G.qkv_row_order(nh, nkv)
    return G.epi_qkv(x[:, order], np.zeros_like(x), 128, np.zeros(x.shape[1]), cos, sin, nh, nkv)[0]


def clamp_positions(positions, n_pos):
    return np.clip(np.asarray(positions, np.int64), 0, n_pos - 1)


def rope_bwd_ref(dy, rope_cols, positions, cos_table, sin_table):
    """dy [T, qkv_n] (float64) -> (dx, pre): dx the gradient w.r.t. the pre-RoPE values -- on the columns < rope_cols the inverse rotation of every pair
    (d, d + 64) of a 128-wide head, x1 = y1 c + y2 s, x2 = y2 c - y1 s with (c, s) = row min(max(position, 0), n_pos - 1) of the tables [n_pos, 64]; beyond
    rope_cols dy itself -- and pre, the bound on the f32 evaluation's error before the 16-bit store: two products and a sum, U each (zero beyond rope_cols)."""
    dy = np.asarray(dy, np.float64)
    T, n = dy.shape
    pp = clamp_positions(positions, len(cos_table))
    c, s = np.asarray(cos_table, np.float64)[pp][:, None, :], np.asarray(sin_table, np.float64)[pp][:, None, :]
    y = dy.reshape(T, n // 128, 128)
    y1, y2 = y[..., :64], y[..., 64:]
    x1, x2 = y1 * c + y2 * s, y2 * c - y1 * s
    p1 = U * (np.abs(y1 * c) + np.abs(y2 * s) + np.abs(x1))
    p2 = U * (np.abs(y2 * c) + np.abs(y1 * s) + np.abs(x2))
    dx, pre = y.copy(), np.zeros_like(y)
    nrot = rope_cols // 128
    dx[:, :nrot] = np.concatenate([x1, x2], -1)[:, :nrot]
    pre[:, :nrot] = np.concatenate([p1, p2], -1)[:, :nrot]
    return dx.reshape(T, n), pre.reshape(T, n)


def rope_bwd_tolerance(dx, pre, dtype):
    """Half an ulp of the 16-bit result (eps |dx|; fp16 below 2^-14: 2^-25 absolute) plus the three f32 operations (pre), the rounding applied to a value that far off."""
    a = np.abs(dx) + pre
    half_ulp = EPS[dtype] * a
    if dtype == "f16":
        half_ulp = np.maximum(half_ulp, np.where(a > 0, 2.0 ** -25, 0.0))
    return half_ulp * (1 + 2 * EPS[dtype]) + pre


def touched(rule, ref, wrong, key_visible, owned, seq_start, seq_len):
    """The elements a wrong rule can move at all, as boolean masks (tq [T, num_heads], tk, tv [T, num_kv_heads]; every head dim of a marked row counts):
    ref / wrong = packed_attention_bwd's results under the right and the wrong rule.
      the visibility rules (ignore_key_visible, diag+-1): dQ where the query's set of keys differs (sig_q) and one of the two sets has two keys or more (softmax over
        a single key is constant: dQ = 0 under both); dK, dV where the set of (query, its keys) that see the key differs (sig_k);
      no_D: dQ of every query with a visible key, dK of every visible key;  scale_twice, lse_other_head: dQ of the queries with two or more visible keys, dK of the
        keys such a query sees (a single-key row has dS = 0 whatever the factor), lse_other_head also dV of every visible key;
      group_first_head_only: dK (keys seen by a query with two or more keys) and dV (visible keys) when a group has more than one head;
      kv_head_mod: dQ of the heads with h % nkv != h // G, dK and dV of the visible keys;
      keys_to_round32: dK and dV of the visible keys of a sequence whose length is no multiple of 32 and that has a token behind it."""
    T, nh = ref.dq.shape[:2]
    nkv = ref.dk.shape[1]
    Gq = nh // nkv
    vis = (np.asarray(key_visible) != 0) & owned
    tq, tk, tv = np.zeros((T, nh), bool), np.zeros((T, nkv), bool), np.zeros((T, nkv), bool)
    two = (ref.nvis >= 2)[:, None]
    if rule in ("ignore_key_visible", "diag+1", "diag-1"):
        tq[:] = ((ref.sig_q != wrong.sig_q) & ((ref.nvis >= 2) | (wrong.nvis >= 2)))[:, None]
        tk[:] = (ref.sig_k != wrong.sig_k)[:, None]
        tv[:] = tk
    elif rule == "no_D":
        tq[:], tk[:] = (ref.nvis >= 1)[:, None], vis[:, None]
    elif rule in ("scale_twice", "lse_other_head"):
        tq[:], tk[:] = two, ref.seen2[:, None]
        if rule == "lse_other_head":
            tv[:] = vis[:, None]
    elif rule == "group_first_head_only":
        if Gq > 1:
            tk[:], tv[:] = ref.seen2[:, None], vis[:, None]
    elif rule == "kv_head_mod":
        moved = np.array([h % nkv != h // Gq for h in range(nh)])
        tq[:] = (ref.nvis >= 1)[:, None] & moved[None, :]
        if moved.any():
            tk[:], tv[:] = vis[:, None], vis[:, None]
    elif rule == "keys_to_round32":
        for s0, n in zip(seq_start, seq_len):
            if n % 32 and s0 + n < T:
                tk[s0:s0 + n], tv[s0:s0 + n] = vis[s0:s0 + n, None], vis[s0:s0 + n, None]
    else:
        raise ValueError(rule)
    return tq, tk, tv
