"""GPU: the trainer's attention backward (csrc/train_kernels.hip: attn_rowdot_kernel, attn_bgemm_kernel<S | dP | dQ>, attn_tn_kernel<dV | dK>) and the RoPE backward
that follows it, through blim_attention_bwd / blim_rope_bwd against the float64 reference of oracle/attention_bwd_ref.py.

Inputs: tests/attention_bwd_inputs.py -- 16-bit values made on the host, lse (f32) and o16 = round16(out) from the float64 forward, so no other kernel takes part
(one family chains blim_attention's own out and lse_out instead: the trainer's flow).  EVERY element of dqkv on the sequences' rows is compared, with the
per-element tolerance that packed_attention_bwd derives from the reference alone.  The workspace (D | P16 | dS16) is filled with NaN patterns before each call,
the rows of no sequence of every input hold NaN, dqkv holds a sentinel, and what the call does not own -- rows of no sequence, the columns [qn, ldq) -- must still
hold it afterwards.  tests/test_attention_bwd_ref.py shows on the CPU that these inputs tell the wrong rules from the right one.
Measured figures: profiles/r14_attention_bwd_direct.md (each test prints its own as ATTN_BWD_MEASURE)."""
import numpy as np
import pytest
import torch

import attention_bwd_inputs as AI
from blim_amd import engine as eng
from oracle import attention_bwd_ref as B
from oracle import attention_ref as R

pytestmark = pytest.mark.gpu

NAN16 = {"f16": 0x7E00, "bf16": 0x7FC0}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ("f16", "bf16")
SENT32 = 0x7E7E7E7E                 # 8.4e37 as f32: never a gradient of these inputs


def _dev16(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(TDT[dtype])


def _rows16(x, T, ld, owned, dtype):
    """x [T, heads, 128] as 16-bit rows of stride ld; the padding columns and the rows of no sequence hold NaN."""
    rows = np.full((T, ld), NAN16[dtype], np.uint16)
    rows[:, :x.shape[1] * AI.D] = R.bits16(x.reshape(T, -1), dtype)
    rows[~owned] = NAN16[dtype]
    return rows


def poisoned_workspace(b, nh, max_len):
    n = eng.attention_bwd_workspace_bytes(b.T, len(b.seq_start), nh, max_len)
    return torch.full((n + 64,), 0xFF, dtype=torch.uint8, device="cuda")          # 0xFFFF / 0xFFFFFFFF: NaN in fp16, bf16 and f32


def launch(b, f, max_len=None, o16=None, lse=None, ws=None):
    """One blim_attention_bwd call.  Row strides: ldq = qn + 8, ldo = hn + 8, ldo16 = hn + 2.  Returns a namespace: dq [T, nh, 128], dk, dv [T, nkv, 128] (float64),
    raw (dqkv's int32 bit patterns [T, ldq]), ws (the workspace as the call left it)."""
    dtype, nh, nkv, T = f.dtype, f.nh, f.nkv, b.T
    qn, hn = (nh + 2 * nkv) * AI.D, nh * AI.D
    max_len = b.max_len if max_len is None else max_len
    qkv = _rows16(np.concatenate([f.q, f.k, f.v], axis=1), T, qn + 8, b.owned, dtype)
    dout = _rows16(f.dout, T, hn + 8, b.owned, dtype)
    o16_rows = _rows16(f.o16, T, hn + 2, b.owned, dtype) if o16 is None else o16
    if lse is None:
        lse = torch.from_numpy(np.where(b.owned[:, None], f.lse32, np.float32("nan")).astype(np.float32)).cuda()
    pb = eng.PackedBatch(np.zeros(T, np.int32), b.key_visible, b.seq_start, b.seq_len)
    dqkv = torch.from_numpy(np.full((T, qn + 8), SENT32, np.int32)).cuda().view(torch.float32)
    ws = poisoned_workspace(b, nh, max_len) if ws is None else ws
    eng.attention_bwd(_dev16(qkv, dtype), _dev16(dout, dtype), o16_rows if torch.is_tensor(o16_rows) else _dev16(o16_rows, dtype), lse, pb, nh, nkv, max_len, dqkv, ws)
    torch.cuda.synchronize()
    r = type("Result", (), {})()
    r.raw = dqkv.view(torch.int32).cpu().numpy()
    g = dqkv.cpu().numpy().astype(np.float64)[:, :qn].reshape(T, nh + 2 * nkv, AI.D)
    r.dq, r.dk, r.dv, r.ws, r.qn = g[:, :nh], g[:, nh:nh + nkv], g[:, nh + nkv:], ws, qn
    return r


def assert_untouched(b, r):
    assert (r.raw[~b.owned] == SENT32).all(), "a row of no sequence was written"
    assert (r.raw[:, r.qn:] == SENT32).all(), "a column beyond q | k | v was written"


def ratios(b, r, ref):
    """max |got - ref| / tol over EVERY element of the sequences' rows, for dq, dk, dv; where tol = 0 (rows without a visible key) the result must be exactly 0."""
    out = []
    for name in ("dq", "dk", "dv"):
        got, want, tol = getattr(r, name)[b.owned], getattr(ref, name)[b.owned], getattr(ref, "tol_" + name)[b.owned]
        assert np.isfinite(got).all(), f"{name}: non-finite values (a poisoned workspace element or a row of no sequence was read)"
        err = np.abs(got - want)
        assert (err[tol == 0] == 0).all(), f"{name}: a row without a visible key is not exactly zero"
        out.append(float(np.max(err[tol > 0] / tol[tol > 0])) if (tol > 0).any() else 0.0)
    return out


def check(batch, family, nh, nkv, dtype, what, **kw):
    b, f, ref = AI.problem(batch, family, nh, nkv, dtype)
    r = launch(b, f, **kw)
    assert_untouched(b, r)
    x = ratios(b, r, ref)
    print(f"ATTN_BWD_MEASURE test={what} dtype={dtype} nh={nh} nkv={nkv} batch={batch} family={family} dq={x[0]:.4g} dk={x[1]:.4g} dv={x[2]:.4g}")
    assert max(x) <= 1.0, (batch, family, x)
    return b, f, ref, r


# ---- 1. single sequences across the 32-, 64- and 128-edges (Lm = 192 is no multiple of 128; L = 257: three key blocks); the head groupings in turn
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", AI.SINGLE_L)
def test_single_sequence_lengths(L, dtype):
    nh, nkv = AI.GQA[AI.SINGLE_L.index(L) % len(AI.GQA)]
    check(f"L{L}", "gauss", nh, nkv, dtype, "lengths")


# ---- 2. mixed batches, masks, head groupings, magnitude families
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", AI.GPU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_batches_masks_and_families(case, dtype):
    check(*case, dtype, "cases")


# ---- 3. max_len larger than the longest sequence: the same result, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
def test_max_len_larger_than_the_longest_sequence(dtype):
    b, f, ref, exact = check("gap40", "gauss", 4, 2, dtype, "max_len=40")
    _, _, _, wide = check("gap40", "gauss", 4, 2, dtype, "max_len=200", max_len=200)
    assert (exact.raw == wide.raw).all()


# ---- 4. the workspaces are reused without clearing: a second call on what the first left, and on a fresh poison, gives the same bits
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [("mix193", "gauss", 7, 1), ("masks", "gauss", 4, 2)], ids=lambda c: c[0])
def test_same_call_twice_is_bit_identical(case, dtype):
    b, f, ref, first = check(*case, dtype, "twice-1")
    again = launch(b, f, ws=first.ws)
    fresh = launch(b, f)
    assert (first.raw == again.raw).all() and (first.raw == fresh.raw).all()
    # ... and a shorter batch run on the workspace a longer one used (the trainer across steps): stale P / dS of the other batch all over it
    b2, f2, ref2 = AI.problem("mix33", "gauss", case[2], case[3], dtype)
    assert first.ws.numel() >= eng.attention_bwd_workspace_bytes(b2.T, 2, case[2], b2.max_len)
    assert (launch(b2, f2, ws=first.ws).raw == launch(b2, f2).raw).all()


# ---- 5. the trainer's flow: blim_attention writes out and lse_out, blim_attention_bwd reads them
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [("masks", "gauss", 4, 2), ("mix193", "peaked", 8, 2), ("short", "aligned", 4, 2)], ids=lambda c: "-".join(map(str, c)))
def test_chained_after_the_forward_kernel(case, dtype):
    """o16 and lse are the forward kernel's: o16 is within attention_ref.tolerance of the reference's out instead of one rounding (o_err), and lse carries the f32
    evaluation of m + log(l): l a sum of nvis terms (nvis U), its terms' exponents formed in f32 (U sum p |arg| <= U log nvis), log, the conversions and the
    final sum (a few U |lse|) -- lse_err = U (8 |lse| + nvis + 16), far below eps either way."""
    batch, family, nh, nkv = case
    b, f, plain = AI.problem(batch, family, nh, nkv, dtype)
    T, qn, hn = b.T, (nh + 2 * nkv) * AI.D, nh * AI.D
    z = np.zeros(len(b.seq_start), np.int32)
    out_ref, A, lse_ref, sub = R.packed_attention(f.q, f.k, f.v, b.key_visible, b.seq_start, b.seq_len, z, z, AI.SCALE)
    qkv = _dev16(_rows16(np.concatenate([f.q, f.k, f.v], axis=1), T, qn + 8, b.owned, dtype), dtype)
    o16 = _dev16(np.full((T, hn + 4), NAN16[dtype], np.uint16), dtype)          # blim_attention wants ldo % 4 == 0; still != the backward's ldo
    lse = torch.full((T, nh), float("nan"), dtype=torch.float32, device="cuda")
    eng.attention(qkv, eng.PackedBatch(np.zeros(T, np.int32), b.key_visible, b.seq_start, b.seq_len), nh, nkv, o16, lse_out=lse)
    ref = AI.reference(b, f, o_err=R.tolerance(out_ref, A, dtype, sub=sub),
                       lse_err=B.U * (8 * np.abs(np.where(lse_ref == R.EMPTY_LSE, 0.0, lse_ref)) + plain.nvis[:, None] + 16))
    r = launch(b, f, o16=o16, lse=lse)
    assert_untouched(b, r)
    x = ratios(b, r, ref)
    print(f"ATTN_BWD_MEASURE test=chained dtype={dtype} nh={nh} nkv={nkv} batch={batch} family={family} dq={x[0]:.4g} dk={x[1]:.4g} dv={x[2]:.4g}")
    assert max(x) <= 1.0, (case, x)


# ---- 6. argument errors the entry reports itself
def test_refusals():
    b, f, _ = AI.problem("L33", "gauss", 4, 2, "f16")
    small = torch.zeros(eng.attention_bwd_workspace_bytes(b.T, 1, 4, 33) - 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(eng.BlimError, match="workspace"):
        launch(b, f, ws=small)
    with pytest.raises(eng.BlimError):
        launch(b, f, max_len=0)
    assert eng.attention_bwd_workspace_bytes(10, 1, 4, 33) == 10 * 4 * 4 + 2 * 4 * 64 * 64 * 2 and eng.attention_bwd_workspace_bytes(0, 1, 4, 33) == -1


# ---- 7. blim_rope_bwd
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nh,nkv", AI.GQA)
def test_rope_bwd(nh, nkv, dtype):
    """T = 77 tokens, positions with 0, n_pos - 1, values out of range on both sides and repeats; rope_cols = (nh + nkv) 128: the V columns pass through.  Tolerance:
    half an ulp of the 16-bit result plus the three f32 operations (rope_bwd_tolerance); 64 values behind the output keep their sentinel."""
    rs = np.random.RandomState(nh * 10 + nkv)
    T, n_pos, qn, rope_cols = 77, 50, (nh + 2 * nkv) * 128, (nh + nkv) * 128
    pos = rs.randint(0, n_pos, T).astype(np.int32)
    pos[:8] = [0, n_pos - 1, -1, -1000, n_pos, n_pos + 1000, 7, 7]
    ang = rs.rand(n_pos, 64) * 6.28
    cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    dy = (rs.randn(T, qn) * np.exp2(rs.randint(-16, 4, (T, 1)))).astype(np.float32)
    want, pre = B.rope_bwd_ref(dy, rope_cols, pos, cos, sin)
    out = _dev16(np.full(T * qn + 64, 0x7E7E, np.uint16), dtype)
    eng.rope_bwd(torch.from_numpy(dy).cuda(), rope_cols, torch.from_numpy(pos).cuda(), torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda(), out)
    torch.cuda.synchronize()
    raw = out.view(torch.int16).cpu().numpy().view(np.uint16)
    assert (raw[T * qn:] == 0x7E7E).all(), "written beyond T * qkv_n"
    got = R.from_bits16(raw[:T * qn], dtype).reshape(T, qn)
    tol = B.rope_bwd_tolerance(want, pre, dtype)
    x = float(np.max(np.abs(got - want) / np.maximum(tol, 1e-300)))
    print(f"ATTN_BWD_MEASURE test=rope_bwd dtype={dtype} nh={nh} nkv={nkv} ratio={x:.4g}")
    assert x <= 1.0
    assert (got[:, rope_cols:] == R.round16(dy[:, rope_cols:], dtype)).all()          # the V columns: the plain 16-bit rounding
