"""GPU: the scoring path's row kernels (csrc/kernels.hip) -- the forward RMSNorm in its three kernel and four output forms, rmsnorm_f8, lse_combine, ce_rows, the TVG
criterion, segment_mean, group_mean and assemble -- each driven alone through blim_rmsnorm / blim_rmsnorm_f8 / blim_lse_combine / blim_ce_rows /
blim_tvg_criterion / blim_segment_mean / blim_group_mean_rows / blim_assemble_rows against the float64 reference of oracle/score_kernels_ref.py.

Inputs: tests/score_kernel_inputs.py -- exact f32 / 16-bit values made on the host, references computed once per case.  EVERY element a call owns is compared:
max |got - ref| / tol <= 1 with the per-element tolerance the reference derives (printed as SCORE_KERNEL_MEASURE); where tol = 0 the result must be exact, a
non-finite output fails unless the reference states it.  RMSNorm's 16-bit outputs are compared BIT FOR BIT with split16 of the f32 output the same launch wrote, its
tiles byte for byte with the e2m3 image of the lo rows it stored.  What a call does not own -- row padding, rows at n_rows and beyond, the bytes behind the tile
image -- holds a sentinel before the call and must hold it afterwards; inputs a kernel never reads (x and logit columns past the row) hold NaN.
tests/test_score_kernels_ref.py shows on the CPU that these inputs tell the wrong rules from the right one and that the exact checks fail on a variant's bytes."""
import math

import numpy as np
import pytest
import torch

import score_kernel_inputs as I
from blim_amd import engine as eng
from oracle import gemm_ref as G
from oracle import score_kernels_ref as S
from oracle.attention_ref import bits16, from_bits16

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
SENT16 = 0x7B7B                     # 61280 as fp16, 1.3e36 as bf16: never a result of these inputs
SENT32 = 0x7E7E7E7E                 # 8.4e37 as f32
SENT8 = 0xA5
ids = lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


def dev16(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).cuda().view(TDT[dtype])


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def devi(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()


def sent16(shape, dtype):
    return dev16(np.full(shape, SENT16, np.uint16), dtype)


def sent32(shape):
    return dev32(np.full(shape, SENT32, np.int32).view(np.float32))


def bits_of(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.element_size() == 2 else t.view(torch.int32).cpu().numpy()


def measure(kernel, dtype, case, **figs):
    print(f"SCORE_KERNEL_MEASURE kernel={kernel} dtype={dtype} case={ids(case)} " + " ".join(f"{k}={v:.4g}" for k, v in figs.items()))
    assert all(math.isfinite(v) and v <= 1.0 for v in figs.values()), (kernel, dtype, case, figs)          # a NaN or inf figure fails too


# ---------------------------------------------------------------------------- RMSNorm
def run_rmsnorm(c, dtype, tiles=False):
    """One launch; returns the stored hi / lo values [n, H] (None where not requested), the f32 output, the tile bytes."""
    n, H, extra = c.n, c.H, 3
    xh = np.full((c.n_src + 1, c.ldx), np.nan, np.float32)                       # columns [H, ldx): never read; the row behind the sources: finite, never read
    xh[:c.n_src, :H] = c.x
    xh[c.n_src, :H] = 7.0
    want_lo = "l" in c.outs
    o16 = sent16((n + extra, c.ldo), dtype) if "h" in c.outs else None
    lo_t = sent16((n + extra, c.ldo), dtype) if want_lo and not c.lo_inside else None
    of = sent32((n + extra, H)) if "f" in c.outs else None
    o6 = torch.full((eng.f6_tiles_bytes(n, H) + 64,), SENT8, dtype=torch.uint8, device="cuda") if tiles else None
    eng.rmsnorm(dev32(xh), dev32(c.w), I.RMS_EPS, n, H, dtype, ldx=c.ldx, rows=None if c.rows is None else devi(c.rows), n_src=c.n_src if c.rows is not None else 0,
                out16=o16, ldo=c.ldo, out_lo=lo_t, lo_offset=H if want_lo and c.lo_inside else None, out_f32=of, saturate=bool(c.sat), out6=o6)
    torch.cuda.synchronize()
    hi = lo = f = t = None
    if o16 is not None:
        b = bits_of(o16)
        own = np.zeros(b.shape, bool)
        own[:n, :H * (2 if want_lo and c.lo_inside else 1)] = True
        assert I.untouched(np.full(b.shape, SENT16, np.uint16), b, own), "out16: a pad column or a row >= n_rows was written"
        hi = from_bits16(b[:n, :H], dtype)
        if want_lo and c.lo_inside:
            lo = from_bits16(b[:n, H:2 * H], dtype)
    if lo_t is not None:
        b = bits_of(lo_t)
        own = np.zeros(b.shape, bool)
        own[:n, :H] = True
        assert I.untouched(np.full(b.shape, SENT16, np.uint16), b, own), "out_lo: a pad column or a row >= n_rows was written"
        lo = from_bits16(b[:n, :H], dtype)
    if of is not None:
        assert (bits_of(of)[n:] == SENT32).all(), "out_f32: a row >= n_rows was written"
        f = of.cpu().numpy()[:n]
    if o6 is not None:
        t = o6.cpu().numpy()
        assert (t[-64:] == SENT8).all(), "out6: written behind blim_f6_tiles_bytes(n_rows, H)"
        t = t[:-64]
    return hi, lo, f, t


def check_rmsnorm(c, dtype, case, kernel, hi, lo, f, t=None):
    r = c.ref
    figs = {}
    if f is not None:
        figs["f32"] = I.ratio(f, r.o, r.tol)
        want_hi, want_lo = S.split16(f, dtype, c.sat, poison=r.poison)
        if hi is not None:
            assert S.same16(hi, want_hi).all(), "hi != round16 (saturated) of the f32 value the same launch wrote"
        if lo is not None:
            assert S.same16(lo, want_lo).all(), "lo != round16(o - hi) of the f32 value the same launch wrote"
    elif lo is not None:
        assert (lo[r.poison] == 0).all() and np.isnan(hi[r.poison]).all(), "a poisoned row is NaN in hi and zero in lo"
        figs["hi_lo"] = I.ratio(hi + lo, r.o, S.tol_hi_lo(r, dtype))
    else:
        figs["hi"] = I.ratio(hi, r.o, S.tol_hi(r, dtype))
    if t is not None:
        lo_rows = lo if lo is not None else S.split16(f, dtype, c.sat, poison=r.poison)[1]
        assert (lo_rows[r.poison] == 0).all()
        want = S.tiles_of(lo_rows)
        assert t.shape == want.shape and (t == want).all(), f"out6: {(t != want).sum()} bytes differ from the e2m3 image of the lo rows (zero rows up to 256 included)"
    measure(kernel, dtype, case, **figs)


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("case", I.RMS, ids=ids)
def test_rmsnorm(case, dtype):
    """A non-finite x (family `nonfinite`), a poisoned gather row and fp16 overflow (`massive`: +-65504 with saturate, +-inf without) are stated by the reference."""
    c = I.rms(case)
    check_rmsnorm(c, dtype, case, "rmsnorm_" + c.form, *run_rmsnorm(c, dtype)[:3])


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("case", I.RMS6, ids=ids)
def test_rmsnorm_tiles(case, dtype):
    c = I.rms6(case)
    assert c.form == "wide"
    check_rmsnorm(c, dtype, case, "rmsnorm_out6", *run_rmsnorm(c, dtype, tiles=True))


@pytest.mark.parametrize("case", I.RMS_F8, ids=ids)
def test_rmsnorm_f8(case):
    c = I.rms_f8(case)
    xh = np.full((c.n, c.ldx), np.nan, np.float32)
    xh[:, :c.H] = c.x
    o8 = torch.full((c.n + 1, c.H), SENT8, dtype=torch.uint8, device="cuda")
    sc = sent32((c.n + 1,))
    eng.rmsnorm_f8(dev32(xh), dev32(c.w), I.RMS_EPS, c.n, c.H, o8, sc, ldx=c.ldx)
    torch.cuda.synchronize()
    codes, scale = o8.cpu().numpy(), sc.cpu().numpy()
    assert (codes[c.n:] == SENT8).all() and bits_of(sc)[c.n] == SENT32, "a row >= n_rows was written"
    val = G.e4m3_decode(codes[:c.n]) * scale[:c.n, None].astype(np.float64)
    measure("rmsnorm_f8", "f8", case, scale=I.ratio(scale[:c.n], c.ref.scale, c.ref.tol_scale), value=I.ratio(val, c.ref.o, c.ref.tol_val(scale[:c.n])))


def test_rmsnorm_refusals():
    """H = 4100 (beyond every kernel), out6 with H = 320 (H % 128 != 0) and out_lo without out16: BLIM_ERR_ARG, nothing written."""
    def call(H, **kw):
        x, w = dev32(np.ones((2, H), np.float32)), dev32(np.ones(H, np.float32))
        bufs = dict(out16=sent16((2, H), "f16"), out_f32=sent32((2, H)))
        bufs.update(kw)
        with pytest.raises(eng.BlimError, match=r"code -1"):
            eng.rmsnorm(x, w, I.RMS_EPS, 2, H, "f16", **bufs)
        torch.cuda.synchronize()
        for b in bufs.values():
            if b is not None and b.dtype != torch.uint8:
                assert (bits_of(b) == (SENT16 if b.element_size() == 2 else SENT32)).all()
    call(4100)
    call(320, out6=torch.zeros(eng.f6_tiles_bytes(2, 384), dtype=torch.uint8, device="cuda"))
    call(256, out16=None, out_lo=sent16((2, 256), "f16"))


# ---------------------------------------------------------------------------- the criteria
@pytest.mark.parametrize("case", I.LSE, ids=ids)
def test_lse_combine(case):
    c = I.lse(case)
    out = sent32((c.n + 2,))
    eng.lse_combine(dev32(np.stack([c.m, c.s], -1)), dev32(c.ll), devi(c.labels), out)
    torch.cuda.synchronize()
    assert (bits_of(out)[c.n:] == SENT32).all(), "logprob was written beyond n_rows"
    measure("lse_combine", "f32", case, logprob=I.ratio(out.cpu().numpy()[:c.n], c.ref, c.tol))


@pytest.mark.parametrize("case", I.CE, ids=ids)
def test_ce_rows(case):
    c = I.ce(case)
    out = eng.ce_rows(dev32(c.buf), devi(c.labels), V=c.V)
    torch.cuda.synchronize()
    measure("ce_rows", "f32", case, logprob=I.ratio(out.cpu().numpy(), c.ref, c.tol))


@pytest.mark.parametrize("case", I.TVG, ids=ids)
def test_tvg_criterion(case):
    c = I.tvg(case)
    out = sent32((c.n_pairs + 2,))
    eng.tvg_criterion(dev32(c.buf), c.nv, devi(c.labels), c.n_pairs, c.clips, out)
    torch.cuda.synchronize()
    assert (bits_of(out)[c.n_pairs:] == SENT32).all(), "score was written beyond n_pairs"
    measure("tvg_criterion", "f32", case, score=I.ratio(out.cpu().numpy()[:c.n_pairs], c.ref, c.tol))


@pytest.mark.parametrize("case", I.SEG, ids=ids)
def test_segment_mean(case):
    """An empty segment, and in mode 0 a segment without a non-zero entry, is 0 / 0 = NaN: stated by the reference, so NaN is REQUIRED there."""
    c = I.seg(case)
    out = eng.segment_mean(dev32(c.lp), devi(c.row_start), c.mode)
    torch.cuda.synchronize()
    measure("segment_mean", "f32", case, score=I.ratio(out.cpu().numpy(), c.ref, c.tol))


# ---------------------------------------------------------------------------- clip mean, assembly
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("case", I.GM, ids=ids)
def test_group_mean(case, dtype):
    c = I.gm(case, dtype)
    W = c.H * (2 if c.split else 1)
    out = sent16((c.n_out + 1, W), dtype)
    eng.group_mean_rows(out, dev16(bits16(c.x, dtype), dtype), c.n_out, c.group, c.H, dtype, split=bool(c.split))
    torch.cuda.synchronize()
    b = bits_of(out)
    assert (b[c.n_out:] == SENT16).all(), "a row >= n_out was written"
    got = from_bits16(b[:c.n_out], dtype)
    if not c.split:
        measure("group_mean", dtype, case, mean=I.ratio(got, c.ref.mean, c.ref.tol))
        return
    hi, lo = got[:, :c.H], got[:, c.H:]
    assert ((c.ref.hi_lo <= hi) & (hi <= c.ref.hi_hi)).all(), "hi is not round16 of a value inside the f32 bound"
    measure("group_mean_split", dtype, case, hi_lo=I.ratio(hi + lo, c.ref.mean, c.ref.tol_sum))


@pytest.mark.parametrize("case", I.ASM, ids=ids)
def test_assemble(case):
    c = I.asm(case)
    n, W = len(c.src), c.H * (2 if c.split else 1)
    out = sent16((n + 1, W), "bf16")
    eng.assemble_rows(out, devi(c.src), n, c.H, dev16(c.table, "bf16"), dev16(c.feats, "bf16"), split=bool(c.split))
    torch.cuda.synchronize()
    b = bits_of(out)
    assert (b[n:] == SENT16).all(), "a row >= n_tokens was written"
    assert (b[:n] == c.ref).all(), "assemble: bytes differ (split: a table row's lo half must be zero)"
    measure("assemble", "bits", case, exact=0.0)
