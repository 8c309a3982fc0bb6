"""GPU: the decoder's attention kernels (csrc/attention.hip), form by form, through blim_attention against the float64 reference of oracle/attention_ref.py.

Inputs: tests/attention_inputs.py (16-bit values made on the host; the reference sees exactly those).  Tolerance, per element and from the reference alone:
tol = 2 eps (c_o |ref| + c_p A), eps = 2^-11 (fp16) / 2^-8 (bf16), A = sum_k p_k |v_kd| (fp16: + 2^-24 per visible key whose weight is an fp16 subnormal, times
max|v| / l) -- R.tolerance states where it comes from; c = 1 for the plain form and
for the compensated forms at large logits, c_p = 1/64 (SPLIT) and c_o = 1/64 (OUT_LO) on the moderate family.  Every output buffer holds a sentinel pattern before
the call, and what the call does not own (tokens of no sequence, columns beyond the heads) must still hold it afterwards.  tests/test_attention_ref.py shows on
the CPU that these inputs tell the wrong rules from the right one.  Measured figures: profiles/r12_attention_direct.md (each test prints its own as ATTN_MEASURE)."""
import numpy as np
import pytest
import torch

import attention_inputs as AI
from blim_amd import engine as eng
from oracle import attention_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7E7E                       # fp16: a NaN; bf16: 5.3e37 -- never a value these inputs produce
NAN16 = {"f16": 0x7E00, "bf16": 0x7FC0}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ("f16", "bf16")


def _dev16(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(TDT[dtype])


def _host16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def launch(b, f, tr=1, split=False, out_lo=False, lse=False, f8=False, cache=None, pfx_len=None, scale=AI.SCALE):
    """One blim_attention call on batch b with values f.  Rows of no sequence that are nobody's prefix, and the padding columns, hold NaN in qkv.  Returns a namespace:
    out / out_lo [T, nh, 128] float64, raw (the whole 16-bit output buffer), lse, out8, mx (where asked for)."""
    dtype, nh, nkv, T = f.dtype, f.nh, f.nkv, b.T
    qn, pad = (nh + 2 * nkv) * AI.D, 8
    v_lo_off = qn + pad if split else 0
    ldq = 2 * (qn + pad) if split else qn + pad
    rows = np.full((T, ldq), NAN16[dtype], np.uint16)
    used = b.owned.copy()
    for p0, pn in zip(b.pfx_start, b.pfx_len):
        used[p0:p0 + pn] = True
    parts = [(0, f.q_hi, f.k_hi, f.v_hi)] + ([(v_lo_off, f.q_lo, f.k_lo, f.v_lo)] if split else [])
    for off, q, k, v in parts:
        rows[:, off:off + qn] = R.bits16(np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], axis=1), dtype)
    rows[~used] = NAN16[dtype]
    hn = nh * AI.D
    out_lo_off = hn + 4 if out_lo else 0
    ldo = 2 * (hn + 4) if out_lo else hn + 4
    out = _dev16(np.full((T, ldo), SENT, np.uint16), dtype)
    pb = eng.PackedBatch(np.zeros(T, np.int32), b.key_visible, b.seq_start, b.seq_len, b.pfx_start, b.pfx_len if pfx_len is None else pfx_len, own_start=b.own_start)
    kw = {}
    if lse:
        kw["lse_out"] = torch.from_numpy(np.full((T, nh), 0x7E7E7E7E, np.int32)).cuda().view(torch.float32)
    if f8:
        kw["out8"] = torch.full((T, hn + 4), 0x7E, dtype=torch.uint8, device="cuda")
        kw["mx_stride"] = (T + 255) // 256 * 256
        kw["out_mx"] = torch.full((nh * kw["mx_stride"],), 0x7E, dtype=torch.uint8, device="cuda")
    if cache is not None:
        kw.update(cache)
    eng.attention(_dev16(rows, dtype), pb, nh, nkv, out, scale=scale, use_tr_read=tr, v_lo_off=v_lo_off, out_lo_off=out_lo_off, **kw)
    torch.cuda.synchronize()
    raw = _host16(out)
    r = type("Result", (), {})()
    r.raw, r.hn, r.out_lo_off = raw, hn, out_lo_off
    r.out = R.from_bits16(raw[:, :hn], dtype).reshape(T, nh, AI.D)
    r.out_lo = R.from_bits16(raw[:, out_lo_off:out_lo_off + hn], dtype).reshape(T, nh, AI.D) if out_lo else None
    r.lse = kw["lse_out"].cpu().numpy() if lse else None
    r.out8 = kw["out8"].cpu().numpy() if f8 else None
    r.mx = kw["out_mx"].cpu().numpy().reshape(nh, -1) if f8 else None
    return r


def assert_untouched(b, r):
    """Tokens of no sequence and the columns beyond the heads still hold the sentinel."""
    assert (r.raw[~b.owned] == SENT).all(), "a row of no sequence was written"
    cols = np.ones(r.raw.shape[1], bool)
    cols[:r.hn] = False
    if r.out_lo_off:
        cols[r.out_lo_off:r.out_lo_off + r.hn] = False
    assert (r.raw[:, cols] == SENT).all(), "a column beyond the heads was written"


def ratio(b, got, ref, A, sub, dtype, c_o=1.0, c_p=1.0):
    """max |got - ref| / tol over the owned rows; where tol = 0 (rows without a visible key) the result must be exactly 0."""
    own = b.owned
    assert np.isfinite(got[own]).all(), "non-finite output"
    err, tol = np.abs(got - ref)[own], R.tolerance(ref, A, dtype, c_o, c_p, sub)[own]
    assert (err[tol == 0] == 0).all(), "a row without a visible key is not exactly zero"
    return float(np.max(err[tol > 0] / tol[tol > 0]))


def measure(**kw):
    print("ATTN_MEASURE " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def check_plain(batch, family, nh, nkv, dtype, tr, what, scale=AI.SCALE):
    b, f, (ref, A, _, sub) = AI.problem(batch, family, nh, nkv, dtype, scale=scale)
    r = launch(b, f, tr=tr, scale=scale)
    assert_untouched(b, r)
    x = ratio(b, r.out, ref, A, sub, dtype)
    measure(test=what, form="plain", dtype=dtype, G=nh // nkv, nkv=nkv, tr=tr, batch=batch, family=family, ratio=x)
    assert x <= 1.0, (batch, family, x)
    return r


# ---- 1. shapes and head groupings, plain form
@pytest.mark.parametrize("tr", [1, 0])
@pytest.mark.parametrize("nkv", [1, 2])
@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_and_head_groupings(dtype, G, nkv, tr):
    """Own lengths {1, 31, 32, 33, 64, 65, 97} x prefix lengths {0, 1, 31, 32, 33, 70} in one packed batch with gaps and shared prefixes, every head grouping the
    dispatch tells apart (G = 5 .. 8 with transposed reads: two workgroups per KV head, G = 5, 7 with an idle wave), Gaussian Q / K and the coupled families (the hot
    key on, just beyond and just before the diagonal)."""
    for family in ("gauss", "self", "next", "prev"):
        check_plain("shapes", family, G * nkv, nkv, dtype, tr, "shapes")


# ---- 2. masks
@pytest.mark.parametrize("tr", [1, 0])
@pytest.mark.parametrize("G", [2, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_masks(dtype, G, tr):
    """Random invisible keys in prefix and own parts (with trap values), an invisible first prefix tile (m_run stays NEG, then moves), an invisible tile in the
    middle, invisible diagonal keys, queries without any visible key (exactly zero), a sequence whose only visible key is its last.  Once more at AI.SCALE_UP, the
    scale at which a row without a visible key needs the kernel's select on its reference maximum (attention_inputs.py)."""
    check_plain("masks", "gauss", G, 1, dtype, tr, "masks_scale_up", scale=AI.SCALE_UP)
    for family in ("gauss", "self", "next", "sink"):
        r = check_plain("masks", family, G, 1, dtype, tr, "masks")
    b = AI.problem("masks", "sink", G, 1, dtype)[0]
    e0, f0 = b.start["E"], b.start["F"]
    assert (r.out[e0:e0 + 5] == 0).all() and (r.out[f0:f0 + 36] == 0).all()


# ---- 3. the lazy reference maximum
@pytest.mark.parametrize("tr", [1, 0])
@pytest.mark.parametrize("G", [2, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lazy_maximum(dtype, G, tr):
    """Row maxima that climb or fall by 4 / 7.9 / 8.1 / 30 log2 units per 32-key tile (below, on either side of and far beyond the 2^8 window) and creep by 0.3 per
    key over 200 keys, neighbouring queries of a block on different ramps: the plain tolerance holds and every value is finite."""
    check_plain("ramp", "ramp", G, 1, dtype, tr, "ramp")


# ---- 4. own_start segments
@pytest.mark.parametrize("kind", ["seg_tvg", "seg_ragged"])
@pytest.mark.parametrize("G", [2, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_own_start_segments(dtype, G, kind):
    """Segments of 3 tokens and of ragged lengths 1 - 40 over a shared prefix, straddling query blocks and key tiles; neighbour-coupled Q / K, so that a key of the
    previous segment (or a missing first key) would dominate the row."""
    for family in ("prev", "prevseg", "self", "next"):
        check_plain(kind, family, G, 1, dtype, 1, "segments")
    check_plain(kind, "prevseg", G, 1, dtype, 0, "segments")


# ---- 5. compensated forms
def check_form(b, f, ref, A, sub, dtype, split, out_lo, moderate, what, **kw):
    r = launch(b, f, split=split, out_lo=out_lo, **kw)
    assert_untouched(b, r)
    got = r.out + r.out_lo if out_lo else r.out
    wide = ratio(b, got, ref, A, sub, dtype)
    c_o, c_p = (1 / 64 if out_lo else 1.0), (1 / 64 if split else 1.0)
    tight = ratio(b, got, ref, A, sub, dtype, c_o, c_p) if moderate else float("nan")
    measure(test=what, form=f"split{int(split)}_lo{int(out_lo)}", dtype=dtype, G=f.nh // f.nkv, moderate=int(moderate), ratio_c1=wide, ratio_tight=tight)
    assert wide <= 1.0, wide
    if moderate:
        assert tight <= 1.0, (c_o, c_p, tight)
    return r


@pytest.mark.parametrize("out_lo", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("G", [1, 2, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compensated_forms(dtype, G, split, out_lo):
    """SPLIT x OUT_LO (helper waves at G < 7, five staging chunks per thread at G = 7; OUT_LO alone takes the plain kernels' grouping: two workgroups of three
    waves at G = 5, 6) on the batches of groups 1 and 2.  On the moderate family the part that
    travels as hi + lo must be 64 times closer to the reference than one 16-bit rounding allows: a missing first-order term (K_lo.Q_hi, K_hi.Q_lo, V_lo.P, V.P_lo, an
    unwritten lo output) costs the whole bracket."""
    for batch, family in (("shapes", "gauss"), ("masks", "gauss"), ("masks", "self")):
        b, f, (ref, A, _, sub) = AI.problem(batch, family, G, 1, dtype, split)
        check_form(b, f, ref, A, sub, dtype, split, out_lo, family == "gauss", "compensated")


# ---- 6. prefix-cache forms
def cache_of(b, f, slots, max_len, split):
    """The cache buffer the gallery would hold, built from the same K / V (and lo) rows: slots = [(first token, filled length)]; strides of the test's choice."""
    nkv, dtype = f.nkv, f.dtype
    w = 2 * nkv * AI.D
    ld = (2 * w if split else w) + 8
    stride = max_len * ld + 16
    buf = np.full(len(slots) * stride, NAN16[dtype], np.uint16)
    for i, (t0, n) in enumerate(slots):
        img = buf[i * stride:i * stride + max_len * ld].reshape(max_len, ld)
        n = min(n, max_len)
        img[:n, :w] = R.bits16(np.concatenate([f.k_hi[t0:t0 + n].reshape(n, -1), f.v_hi[t0:t0 + n].reshape(n, -1)], axis=1), dtype)
        if split:
            img[:n, w:2 * w] = R.bits16(np.concatenate([f.k_lo[t0:t0 + n].reshape(n, -1), f.v_lo[t0:t0 + n].reshape(n, -1)], axis=1), dtype)
    return dict(pfx_cache=_dev16(buf, dtype), pc_slot_stride=stride, pc_ld=ld, pc_lo_off=w if split else 0, pc_n_slots=len(slots), pc_max_len=max_len)


@pytest.mark.parametrize("out_lo", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("G", [2, 5, 6, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_cache_forms(dtype, G, split, out_lo):
    """One batch mixes slot -1, a slot >= pc_n_slots (both: the in-batch prefix, key_visible honoured), valid slots (every cached key visible, whatever key_visible says)
    and a prefix longer than pc_max_len (clamped).  Within tolerance of the reference everywhere; bit-equal to the uncached call where the visible set is the same."""
    b, f, _ = AI.problem("cache", "gauss", G, 1, dtype, split)
    max_len = 64
    #                A   s1(A,70) s2(A,70) s3(P,1) s4(P,31) s5(P,32) s6(P,33) s7  s8(P,33)
    slot = np.array([-1, 0,       -1,      1,      5,       1,       1,       1,  -1], np.int32)
    cached = (slot >= 0) & (slot < 2) & (b.pfx_len > 0)
    cache = cache_of(b, f, [(b.start["A"], 70), (b.start["P"], 33)], max_len, split)
    cache["pfx_slot"] = torch.from_numpy(slot).cuda()
    ref, A, _, sub = AI.reference(b, f, pfx_len=np.where(cached, np.minimum(b.pfx_len, max_len), b.pfx_len), pfx_all_visible=cached)
    r = check_form(b, f, ref, A, sub, dtype, split, out_lo, True, "cache", cache=cache)
    u = launch(b, f, split=split, out_lo=out_lo)
    same = np.zeros(b.T, bool)
    for s in (0, 2, 3, 4, 7, 8):          # uncached sequences, and s3: its one cached key is visible in the batch too
        same[b.seq_start[s]:b.seq_start[s] + b.seq_len[s]] = True
    assert (r.raw[same] == u.raw[same]).all()
    assert (r.raw[b.owned & ~same] != u.raw[b.owned & ~same]).any()          # the other sequences do see another key set: the comparison above is not vacuous


# ---- 7. lse_out
@pytest.mark.parametrize("case", [("shapes", "gauss"), ("shapes", "self"), ("masks", "gauss"), ("masks", "sink"), ("ramp", "ramp")])
@pytest.mark.parametrize("G", [2, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_out(dtype, G, case):
    """The log-sum-exp the backward reads: fp32 arithmetic on values up to a few hundred -> 1e-4 max(1, |lse|); exactly 1e30 for a row without a visible key; the
    output does not change when it is asked for; rows of no sequence are not written."""
    b, f, (ref, A, lse, _) = AI.problem(case[0], case[1], G, 1, dtype)
    for tr in (1, 0):
        r, plain = launch(b, f, tr=tr, lse=True), launch(b, f, tr=tr)
        assert (r.raw == plain.raw).all()
        assert (r.lse[~b.owned].view(np.int32) == 0x7E7E7E7E).all()
        empty = (lse == R.EMPTY_LSE) & b.owned[:, None]
        assert (r.lse[empty] == np.float32(1e30)).all()
        live = b.owned[:, None] & ~empty
        dev = float(np.max(np.abs(r.lse[live] - lse[live]) / np.maximum(1.0, np.abs(lse[live]))))
        measure(test="lse", dtype=dtype, G=G, tr=tr, batch=case[0], family=case[1], lse_dev=dev, lse_absmax=float(np.abs(lse[live]).max()))
        assert dev <= 1e-4, dev


# ---- 8. fused e4m3 + E8M0 output
def e4m3_table():
    """OCP e4m3 (bias 7, no infinities, 0x7F / 0xFF = NaN) as float64 [256]."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    val = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    val = np.where((c & 0x7F) == 0x7F, np.nan, val)
    return np.where(c >= 128, -val, val)


@pytest.mark.parametrize("case", [("shapes", "gauss"), ("shapes", "self"), ("masks", "gauss"), ("masks", "self")])
@pytest.mark.parametrize("G", [2, 4, 7])
def test_fused_fp8_output(G, case):
    """out8 / out_mx (fp16): one E8M0 exponent per (token, head) at the place gemm.hpp's `a_mx` documents -- [head][256-row tile][(wm * 16 + fr) * 8 + mi], row in tile =
    128 wm + 16 mi + fr -- and e4m3 values; the dequantised value is within the plain tolerance + half an e4m3 ulp of the reference, no scaled value leaves the
    format, and the exponent is the smallest that fits except where the reference maximum sits within tolerance of a boundary."""
    dtype = "f16"
    b, f, (ref, A, _, sub) = AI.problem(case[0], case[1], G, 1, dtype)
    T, nh = b.T, G
    for tr in (1, 0):
        r = launch(b, f, tr=tr, f8=True)
        assert (r.raw == SENT).all()                                               # the 16-bit buffer is not this form's output
        assert (r.out8[~b.owned] == 0x7E).all() and (r.out8[:, nh * AI.D:] == 0x7E).all()
        tok = np.arange(T)
        rl = tok & 255
        where = (tok >> 8) * 256 + ((rl >> 7) * 16 + (rl & 15)) * 8 + ((rl >> 4) & 7)
        mine = np.zeros(r.mx.shape[1], bool)
        mine[where[b.owned]] = True
        assert (r.mx[:, ~mine] == 0x7E).all()
        e = r.mx[:, where].T.astype(np.int64) - 127                                  # [T, nh]
        codes = r.out8[:, :nh * AI.D].reshape(T, nh, AI.D)
        assert not ((codes[b.owned] & 0x7F) == 0x7F).any(), "a scaled value left e4m3's range"
        d = e4m3_table()[codes] * 2.0 ** e[:, :, None]
        tol = R.tolerance(ref, A, dtype, sub=sub)
        h = np.where(np.abs(ref) * 2.0 ** -e[:, :, None] >= 2.0 ** -6, 2.0 ** -4 * np.abs(ref), 2.0 ** -10 * 2.0 ** e[:, :, None])
        own = b.owned
        x = float(np.max((np.abs(d - ref)[own]) / np.maximum((tol + h)[own], 1e-300)))
        amax = np.abs(ref).max(axis=2)
        with np.errstate(divide="ignore"):
            e_ref = np.where(amax > 0, np.ceil(np.log2(np.maximum(amax, 1e-300) / 448.0)), 0).astype(np.int64)
        tmax = tol.max(axis=2)
        off = own[:, None] & (e != e_ref)
        up, down = off & (e == e_ref + 1), off & (e == e_ref - 1)
        near = (up & (448.0 * 2.0 ** e_ref - amax <= tmax)) | (down & (amax - 448.0 * 2.0 ** (e_ref - 1.0) <= tmax))
        share = float(off.sum()) / float(own.sum() * nh)
        measure(test="fp8", dtype=dtype, G=G, tr=tr, batch=case[0], family=case[1], ratio=x, exponent_exceptions=share)
        assert x <= 1.0, x
        assert (off == near).all(), "an exponent that is not the smallest one, away from a boundary"
        assert share < 0.05, share
