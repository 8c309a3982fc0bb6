"""Input builders shared by tests/test_attention_ref.py (CPU: the sensitivity conditions) and tests/test_attention_gpu.py (the kernel against the float64
reference): packed batches with gaps, shared prefixes, masks and own_start segments, and Q / K / V families that make a wrong visible set show.

Every value handed to the kernel is a 16-bit value made here (compensated forms: hi and lo = 16-bit(x - hi)); the reference sees exactly hi (+ lo) in float64."""
import functools
import types

import numpy as np

from oracle import attention_ref as R

D = 128
SCALE = 128 ** -0.5
# A second scale, for rows without a visible key.  The kernel's exponent is fma(s, c, -m c) with c = fp32(scale log2 e), and such a row has s = m = -1e30: without
# the kernel's select on m the argument is the rounding error of the fp32 product -1e30 c, some +-1e21.  At SCALE that error is negative (exp2 gives 0, as the
# select does); at SCALE_UP it is positive (exp2 gives inf), so only there does a kernel without the select show.  tests/test_attention_ref.py checks both signs.
SCALE_UP = 0.0885


def _pack(spec, gaps=(3, 2, 0, 5, 1)):
    """spec: list of ("pool", name, n) -- n tokens of no sequence, usable as a prefix -- or ("seq", name, n, pfx_name or None, pfx_len).  A prefix may name a pool or an
    earlier sequence.  Gaps (tokens of no sequence) of cycling sizes go in front of every entry."""
    start, t = {}, 0
    seqs = []
    for i, e in enumerate(spec):
        t += gaps[i % len(gaps)]
        start[e[1]] = t
        if e[0] == "seq":
            seqs.append((t, e[2], start[e[3]] if e[3] else 0, e[4] if e[3] else 0))
        t += e[2]
    T = t + 4
    a = np.array(seqs, dtype=np.int32)
    b = types.SimpleNamespace(T=T, seq_start=a[:, 0].copy(), seq_len=a[:, 1].copy(), pfx_start=a[:, 2].copy(), pfx_len=a[:, 3].copy(),
                              key_visible=np.ones(T, np.uint8), own_start=None, start=start, sinks=[])
    b.owned = np.zeros(T, bool)
    for s0, n in zip(b.seq_start, b.seq_len):
        b.owned[s0:s0 + n] = True
    return b


def batch_shapes():
    """Group 1: own lengths {1, 31, 32, 33, 64, 65, 97} x prefix lengths {0, 1, 31, 32, 33, 70}; several sequences share one prefix; the 70-key prefix is the head of
    a sequence of the batch."""
    return _pack([("seq", "A", 97, None, 0), ("pool", "P", 70), ("seq", "s1", 1, "A", 70), ("seq", "s2", 31, "A", 70), ("seq", "s3", 32, "P", 1),
                  ("seq", "s4", 33, "P", 31), ("seq", "s5", 64, "P", 32), ("seq", "s6", 65, "P", 33), ("seq", "s7", 1, None, 0), ("seq", "s8", 33, "P", 33)])


def batch_masks(seed=5):
    """Group 2: a prefix whose first 32-key tile is invisible, a sequence with an invisible tile in the middle, queries without any visible key, a sequence whose only
    visible key is its last one, random invisible keys (prefix and own parts, diagonal keys among them).  The last key of every prefix in use is visible: the sink."""
    b = _pack([("pool", "P", 70), ("seq", "A", 97, None, 0), ("seq", "B", 33, "P", 33), ("seq", "C", 65, "P", 70), ("seq", "Dd", 64, "A", 40),
               ("seq", "E", 40, None, 0), ("seq", "F", 37, None, 0), ("seq", "Gg", 40, "P", 70), ("seq", "H", 50, "A", 40)])
    rs = np.random.RandomState(seed)
    v, st = b.key_visible, b.start
    v[st["P"]:st["P"] + 32] = 0
    v[st["P"] + 33:st["P"] + 69][rs.rand(36) < 0.15] = 0
    v[st["A"] + 32:st["A"] + 64] = 0
    v[st["A"] + 64:st["A"] + 97][rs.rand(33) < 0.15] = 0
    v[st["A"]:st["A"] + 32][rs.rand(32) < 0.1] = 0
    for name, n in (("B", 33), ("C", 65), ("Dd", 64), ("Gg", 40), ("H", 50)):
        v[st[name]:st[name] + n][rs.rand(n) < 0.1] = 0
    v[st["E"]:st["E"] + 5] = 0
    v[st["F"]:st["F"] + 36] = 0
    b.sinks = [st["P"] + 32, st["P"] + 69, st["A"] + 39]
    v[b.sinks] = 1
    return b


def batch_segments(kind):
    """Group 4: own_start segments over a shared prefix -- "tvg": segments of 3 tokens; "ragged": lengths 1 .. 40.  3 does not divide 32 and the ragged cuts fall
    anywhere, so segments straddle the 32-query blocks and the 32-key tiles."""
    if kind == "tvg":
        lens = [[3] * 30, [3] * 11]
    else:
        lens = [[1, 40, 2, 31, 33, 5, 1, 17], [7, 32, 1, 1, 26]]
    b = _pack([("pool", "P", 40)] + [("seq", f"s{i}", int(sum(l)), "P", 40 if i == 0 else 33) for i, l in enumerate(lens)])
    b.own_start = np.zeros(b.T, np.int32)
    for s0, l in zip(b.seq_start, lens):
        c = np.concatenate([[0], np.cumsum(l)])
        for a, e in zip(c[:-1], c[1:]):
            b.own_start[s0 + a:s0 + e] = a
    b.key_visible[b.start["P"] + 7] = 0
    b.sinks = [b.start["P"] + 39, b.start["P"] + 32]
    return b


def batch_cache():
    """Group 6: batch_shapes with invisible tokens inside both prefixes -- the cached forms see them (every cached key is visible), the in-batch prefixes do not."""
    b = batch_shapes()
    b.key_visible[[b.start["P"] + 5, b.start["P"] + 20, b.start["A"] + 3]] = 0
    return b


RAMP_RATES = (4.0, 7.9, 8.1, 30.0, -4.0, -7.9, -8.1, -30.0, 9.6, 0.0, 1.0)     # log2 units per 32-key tile; 9.6 = a creep of 0.3 per key


def batch_ramp():
    """Group 3: a 200-key prefix (and a 97-token causal sequence) whose K lie along one direction with the key index as the coefficient; the queries' coefficients are
    RAMP_RATES in turn, so neighbouring queries of one 32-query block climb (or descend) at different rates."""
    return _pack([("pool", "P", 200), ("seq", "R1", 40, "P", 200), ("seq", "R2", 33, "P", 128), ("seq", "R3", 97, None, 0), ("seq", "R4", 12, "P", 70)])


FAMILIES = ("gauss", "self", "next", "prev", "prevseg", "sink", "ramp")


def fill(b, family, nh, nkv, dtype, seed=0, split=False):
    """Q / K / V of a family on batch b as 16-bit values (float64 arrays): a namespace with q [T, nh, D], k, v [T, nkv, D] = what the reference sees (hi + lo when
    split), and q_hi .. v_lo, the parts the kernel gets.
      gauss: independent N(0, 1): logit std 1 -- the moderate family;
      self / next / prev: the query heads of a KV head share a base vector per token and K_j = 0.9 base_j / base_{j-1} / base_{j+1} + 0.3 noise: the hot key of query
        i is key i (a missing diagonal shows) / key i + 1 (just beyond the diagonal) / key i - 1 (for a segment's first query: in the previous segment);
      prevseg (segmented batches): the queries of a segment share a base vector and every key of the segment BEFORE it is aligned with it, so the key just in front
        of a segment is hot for each of the segment's queries, not only for the first;
      sink: the queries share a mean vector; the keys in b.sinks are aligned with it and carry V = 8;
      ramp: batch_ramp's.
    Invisible keys carry trap values V = +-8 in every family."""
    rs = np.random.RandomState(1000 + seed)
    T, G = b.T, nh // nkv
    base = rs.randn(T, nkv, D)
    q, k, v = rs.randn(T, nh, D), rs.randn(T, nkv, D), rs.randn(T, nkv, D)
    if family in ("self", "next", "prev"):
        q = np.repeat(base, G, axis=1) + 0.25 * q
        k = 0.9 * np.roll(base, {"self": 0, "next": 1, "prev": -1}[family], axis=0) + 0.3 * k
    elif family == "prevseg":
        first = np.arange(T)                                   # packed index of the first token of each token's segment, and of the segment after it
        nxt = np.arange(T)
        for s0, n in zip(b.seq_start, b.seq_len):
            os_ = b.own_start[s0:s0 + n]
            ends = np.concatenate([np.nonzero(np.diff(os_))[0] + 1, [n]])
            first[s0:s0 + n] = s0 + os_
            nxt[s0:s0 + n] = s0 + np.minimum(ends[np.searchsorted(ends, np.arange(n), side="right")], n - 1)
        q = np.repeat(base[first], G, axis=1) + 0.25 * q
        k = 0.9 * base[nxt] + 0.3 * k
    elif family == "sink":
        mu = 0.5 * np.sign(rs.randn(D))
        q = q + mu
        k[b.sinks] = 1.3 * mu
        v[b.sinks] = 8.0
    elif family == "ramp":
        u = np.sign(rs.randn(D))
        rate = np.array(RAMP_RATES)[np.arange(T) % len(RAMP_RATES)]
        coef = np.zeros(T)
        for name, n in (("P", 200), ("R3", 97)):
            coef[b.start[name]:b.start[name] + n] = np.arange(n) / 32.0
        beta = 1.0 / (D * SCALE * 1.4426950408889634 * 0.25)
        q = 0.05 * q + (rate * beta)[:, None, None] * u
        k = 0.05 * k + (coef * 0.25)[:, None, None] * u
    elif family != "gauss":
        raise ValueError(family)
    inv = b.key_visible == 0
    v[inv] = 8.0 * np.sign(rs.randn(int(inv.sum()), nkv, D))
    f = types.SimpleNamespace(dtype=dtype, nh=nh, nkv=nkv, split=split)
    for name, x in (("q", q), ("k", k), ("v", v)):
        hi = R.round16(x, dtype)
        lo = R.round16(x - hi, dtype) if split else np.zeros_like(hi)
        setattr(f, name + "_hi", hi); setattr(f, name + "_lo", lo); setattr(f, name, hi + lo)
    return f


def reference(b, f, rule=None, pfx_len=None, pfx_all_visible=None, return_sig=False, scale=SCALE):
    return R.packed_attention(f.q, f.k, f.v, b.key_visible, b.seq_start, b.seq_len, b.pfx_start, b.pfx_len if pfx_len is None else pfx_len, scale,
                              own_start=b.own_start, rule=rule, pfx_all_visible=pfx_all_visible, return_sig=return_sig)


BATCHES = {"shapes": batch_shapes, "masks": batch_masks, "seg_tvg": lambda: batch_segments("tvg"), "seg_ragged": lambda: batch_segments("ragged"), "ramp": batch_ramp, "cache": batch_cache}


@functools.lru_cache(maxsize=None)
def problem(batch, family, nh, nkv, dtype, split=False, scale=SCALE):
    """(batch, values, (out, A, lse, sub)) -- built once per process and shared; nobody writes to them."""
    b = BATCHES[batch]()
    f = fill(b, family, nh, nkv, dtype, seed=len(batch) + 7 * FAMILIES.index(family), split=split)
    return b, f, reference(b, f, scale=scale)


# (rule, batch, family): the inputs on which each wrong rule must show (tests/test_attention_ref.py), all of them inputs of the GPU tests
SENSITIVITY = [("ignore_key_visible", "masks", "gauss"), ("diag-1", "masks", "self"), ("diag+1", "masks", "next"), ("own_start-1", "seg_tvg", "prevseg"),
               ("own_start-1", "seg_ragged", "prevseg"), ("pfx_len+1", "masks", "sink"), ("pfx_len-1", "masks", "sink"), ("no_prefix", "masks", "sink"),
               ("diag-1", "seg_ragged", "self"), ("diag+1", "seg_tvg", "next")]
