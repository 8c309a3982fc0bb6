"""Input builders shared by tests/test_attention_bwd_ref.py (CPU: the reference's pins, the emulation, the sensitivity conditions) and
tests/test_attention_bwd_gpu.py (the trainer's attention backward against the float64 reference of oracle/attention_bwd_ref.py).

Every value handed to the kernel is a 16-bit value made here; the reference sees exactly those in float64.  lse and o16 come from the float64 forward
(lse as the nearest f32, o16 = round16(out)), so the backward's inputs do not depend on another kernel."""
import functools
import types

import numpy as np

from oracle import attention_bwd_ref as B
from oracle import attention_ref as R

D = 128
SCALE = 128 ** -0.5
SINGLE_L = (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 161, 192, 193, 257)
GQA = ((2, 2), (4, 2), (7, 1), (8, 2))


def _pack(lens, gaps=(3, 2, 0, 5, 1)):
    """Sequences of the given lengths with gaps (tokens of no sequence) of cycling sizes in front of each and 4 tokens behind the last."""
    t, start = 0, []
    for i, n in enumerate(lens):
        t += gaps[i % len(gaps)]
        start.append(t)
        t += n
    T = t + 4
    b = types.SimpleNamespace(T=T, seq_start=np.array(start, np.int32), seq_len=np.array(lens, np.int32), key_visible=np.ones(T, np.uint8), max_len=int(max(lens)))
    b.owned = np.zeros(T, bool)
    for s0, n in zip(b.seq_start, b.seq_len):
        b.owned[s0:s0 + n] = True
    return b


def batch_masks():
    """Left padding as the trainer's collate makes it (the first keys of a row invisible: their queries see nothing), masked keys in the middle, at position L - 1
    and at multiples of 64, a fully masked sequence, and a sequence whose only visible key is its last."""
    b = _pack([97, 70, 33, 129, 40, 65])
    v, st = b.key_visible, b.seq_start
    v[st[0]:st[0] + 20] = 0                                  # left padding
    v[st[0] + 64] = 0
    v[st[1] + np.array([5, 6, 30, 31, 32, 33, 64, 69])] = 0  # the middle, across the 32-edge, position 64, position L - 1
    v[st[2]:st[2] + 33] = 0                                  # nothing visible
    v[st[3] + np.array([0, 63, 64, 127, 128])] = 0
    v[st[4]:st[4] + 39] = 0                                  # the last key alone
    v[st[5] + np.arange(1, 65, 2)] = 0                       # every other key
    return b


def batch_short():
    """Many short sequences (1 .. 12 tokens): few keys per row, so that one key more or less, or one head more or less, moves every element."""
    return _pack([5, 3, 8, 2, 12, 7, 4, 6, 1, 8, 5, 3])


def batch_tiny():
    """1 .. 5 tokens per sequence with 7 - 13 tokens of no sequence between them."""
    return _pack([2, 3, 4, 5, 3, 2, 4, 5, 1, 3, 4, 2, 5, 3, 2, 4], gaps=(11, 7, 13, 9))


def batch_pairs(masked=False):
    """One or two tokens per sequence (masked: two or three, one key of each invisible): the rows on which the wrong rules must show at bf16 too -- ten bf16
    tolerances are a quarter of the bound's sum of magnitudes, more than one key among three or more moves."""
    if not masked:
        return _pack([2, 2, 1, 2, 2, 2, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2], gaps=(11, 7, 13, 9))
    b = _pack([2, 3, 2, 3, 3, 2, 3, 2, 2, 3, 3, 2, 3, 2, 3, 3], gaps=(11, 7, 13, 9))
    for s0, n in zip(b.seq_start, b.seq_len):
        b.key_visible[s0 + (0 if n == 2 else 1)] = 0
    return b


def batch_short_masked():
    b = _pack([5, 8, 7, 4, 6, 8, 5, 8, 7, 6])
    for s0, n in zip(b.seq_start, b.seq_len):
        b.key_visible[s0 + 1] = 0
        if n > 6:
            b.key_visible[s0 + 4] = 0
    return b


BATCHES = {"masks": batch_masks, "short": batch_short, "tiny": batch_tiny, "pairs": batch_pairs, "pairs_masked": lambda: batch_pairs(True), "short_masked": batch_short_masked, "mix193": lambda: _pack([193, 5, 64]), "mix33": lambda: _pack([33, 129]),
           "gap40": lambda: _pack([40], gaps=(7,))}
for _L in SINGLE_L:
    BATCHES[f"L{_L}"] = functools.partial(_pack, [_L])

FAMILIES = ("gauss", "peaked", "next", "dout_small", "dout_big", "aligned", "sink", "aligned_m")


def fill(b, family, nh, nkv, dtype, seed=0):
    """q, k, v, dout of a family on batch b as 16-bit values (float64 arrays) in a namespace, with o16 = round16(out) and lse32 from the float64 forward.
      gauss: independent N(0, 1): logit std 1 -- the moderate family;
      peaked: the query heads of a KV head share a base vector per token and K_j = 0.9 base_j + 0.3 noise: key i carries nearly all of query i's weight and the
        others' P are fp16 subnormals;  next: K_j = 0.9 base_{j-1} + 0.3 noise: the hot key of query i is key i + 1, just beyond the diagonal;
      dout_small / dout_big: gauss with dout scaled by 2^-12 / 2^6 (the trainer's loss scaler moves it): dS in fp16's subnormal range / far above 1;
      sink: every query carries a common vector u and key 0 of each sequence is 1.3 u: key 0 takes nearly all of every row's weight and the keys j >= 1 get
        fp16-subnormal P only, their own diagonal included -- dV of those keys is a sum of subnormal P alone (in `peaked` each key's column also holds its
        diagonal P ~ 1, whose eps hides them);
      aligned: built so that a wrong rule moves every element by a large share of the bound's sum of magnitudes, in bf16 too.  With par_t = (-1)^t:
        K_t = par_t w + u + 0.15 noise, Q_t = par_t w2 + (h / (scale 128)) u + 0.15 noise with w, w2, u orthogonal and every entry away from zero -- the logits are
        near 0 (P near uniform), the heads' lse are h apart while P stays as it was, and dQ = dS K, dK = dS^T Q add up with one sign per head dim; V_t lives on
        the 16 dims of block t % 4 (|V_t|^2 ~ 128; invisible keys keep their dense traps), and dO_t = par_t sum_{r = t-2 .. t+1} par_r V_r + a dense part
        par_t (1 or 3 by head) sign(w) on dims >= 64 where V is zero: dP = dO V^T is +-128 with the parity of i + j on the keys next to the diagonal, the one
        beyond it included, so that dS alternates with the key's parity like K does;
      aligned_m: aligned with Q_t = par_t (w2 + 0.06 w): keys of the query's own parity carry most of the weight, so that D = rowsum(P o dP) is far from 0.
    Invisible keys carry trap values V = +-8 in every family.  Tokens of no sequence carry ordinary values here, dout 8 times as large (a wrong rule that reads them must show);
    the GPU tests hand the kernel NaN there."""
    rs = np.random.RandomState(2000 + seed)
    T, G = b.T, nh // nkv
    base = rs.randn(T, nkv, D)
    q, k, v, dout = rs.randn(T, nh, D), rs.randn(T, nkv, D), rs.randn(T, nkv, D), rs.randn(T, nh, D)
    if family in ("peaked", "next"):
        q = np.repeat(base, G, axis=1) + 0.25 * q
        k = 0.9 * np.roll(base, 1 if family == "next" else 0, axis=0) + 0.3 * k
    elif family == "dout_small":
        dout = dout * 2.0 ** -12
    elif family == "dout_big":
        dout = dout * 2.0 ** 6
    elif family == "sink":
        u = np.sign(rs.randn(D))
        q = q + u
        k[b.seq_start] = 1.3 * u
    elif family not in ("gauss", "aligned", "aligned_m"):
        raise ValueError(family)
    inv = b.key_visible == 0
    v[inv] = 8.0 * np.sign(rs.randn(int(inv.sum()), nkv, D))
    if family in ("aligned", "aligned_m"):
        w = 1.5 * np.sign(rs.randn(D))
        walsh = lambda n: 1.0 - 2.0 * ((np.arange(D) // n) % 2)
        w2, u = w * walsh(1), np.abs(w) / 1.5 * walsh(2)              # w, w2, u: orthogonal to each other, every entry away from zero
        par = (1.0 - 2.0 * (np.arange(T) % 2))[:, None, None]
        k = par * w + 0.15 * k + u
        q = par * (w2 + (0.06 if family == "aligned_m" else 0.0) * w) + 0.15 * q + (1.0 * np.arange(nh) / (SCALE * D))[None, :, None] * u
        block = (np.arange(D)[None, :] // 16 == (np.arange(T) % 4)[:, None])[:, None, :]
        v = np.where(inv[:, None, None], v, np.where(block, 8.0 ** 0.5 * v, 0.0))
        z = sum(np.roll(par * v, r, axis=0) for r in range(-1, 3))
        dout = np.repeat(par * z, G, axis=1) + par * (1.0 + 2.0 * (np.arange(nh) % 2))[None, :, None] * ((np.arange(D) >= 64) * np.sign(w)) + 0.25 * dout
    dout[~b.owned] *= 8.0
    f = types.SimpleNamespace(dtype=dtype, nh=nh, nkv=nkv, family=family)
    for name, x in (("q", q), ("k", k), ("v", v), ("dout", dout)):
        setattr(f, name, R.round16(x, dtype))
    return f


def reference(b, f, rule=None, drop=(), dtype=True, **kw):
    return B.packed_attention_bwd(f.q, f.k, f.v, f.dout, b.key_visible, b.seq_start, b.seq_len, SCALE, rule=rule, dtype=f.dtype if dtype and rule is None else None,
                                  drop=drop, **kw)


@functools.lru_cache(maxsize=None)
def problem(batch, family, nh, nkv, dtype):
    """(batch, values, reference) -- built once per process and shared; nobody writes to them.  values also carries o16 (float64 of the 16-bit forward output) and
    lse32 (float32)."""
    b = BATCHES[batch]()
    f = fill(b, family, nh, nkv, dtype, seed=sum(map(ord, batch)) + 7 * FAMILIES.index(family) + nh)
    ref = reference(b, f)
    f.o16 = R.round16(ref.out, dtype)
    f.lse32 = ref.lse.astype(np.float32)
    return b, f, ref


def emulate(b, f):
    """oracle.attention_bwd_ref.emulate_kernel over the whole batch: (dq, dk, dv) float64, zero outside the sequences."""
    T, nh, nkv = b.T, f.nh, f.nkv
    G = nh // nkv
    dq, dk, dv = np.zeros((T, nh, D)), np.zeros((T, nkv, D)), np.zeros((T, nkv, D))
    for s0, n in zip(b.seq_start, b.seq_len):
        sl = slice(int(s0), int(s0 + n))
        see = (np.arange(n)[None, :] <= np.arange(n)[:, None]) & (b.key_visible[sl] != 0)[None, :]
        for g in range(nkv):
            hs = slice(g * G, (g + 1) * G)
            tr = lambda a: a.transpose(1, 0, 2)
            a, c, e = B.emulate_kernel(tr(f.q[sl, hs]), f.k[sl, g], f.v[sl, g], tr(f.dout[sl, hs]), tr(f.o16[sl, hs]), f.lse32[sl, hs].T, see, SCALE, f.dtype)
            dq[sl, hs], dk[sl, g], dv[sl, g] = tr(a), c, e
    return dq, dk, dv


# (batch, family, nh, nkv): what the GPU tests run beyond the single-sequence lengths, and what the emulation is checked on (both dtypes each)
GPU_CASES = [("pairs", "aligned", 4, 2), ("pairs", "aligned", 7, 1), ("pairs", "aligned_m", 4, 2), ("pairs_masked", "aligned", 4, 2), ("short", "sink", 4, 2), ("L33", "sink", 4, 2), ("mix193", "sink", 7, 1), ("tiny", "aligned", 4, 2), ("short", "aligned", 4, 2), ("short_masked", "aligned", 4, 2), ("masks", "aligned", 8, 2), ("masks", "gauss", 4, 2), ("masks", "peaked", 2, 2), ("masks", "next", 4, 2), ("short", "gauss", 4, 2), ("short_masked", "gauss", 4, 2),
             ("short", "peaked", 4, 2), ("mix193", "gauss", 7, 1), ("mix193", "peaked", 8, 2), ("mix33", "gauss", 8, 2), ("mix33", "dout_small", 4, 2),
             ("mix33", "dout_big", 4, 2), ("short", "dout_small", 2, 2), ("short", "dout_big", 7, 1), ("mix33", "peaked", 7, 1)]

# (rule, batch, family, nh, nkv): the inputs on which each wrong rule must show (tests/test_attention_bwd_ref.py), all of them among GPU_CASES, in both dtypes
_SENS_CASE = {"ignore_key_visible": ("pairs_masked", "aligned", 4, 2), "no_D": ("pairs", "aligned_m", 4, 2), "group_first_head_only": ("pairs", "aligned", 7, 1)}
SENSITIVITY = [(r,) + _SENS_CASE.get(r, ("pairs", "aligned", 4, 2)) for r in B.RULES]
