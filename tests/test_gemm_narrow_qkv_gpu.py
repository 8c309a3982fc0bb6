"""GPU: the narrow-tile QKV GEMM (csrc/gemm.hip: gemm_nqkv_kernel; blim_gemm's `tile_qkv`) against the 256 x 256 kernel on the same operands, BIT FOR BIT on the whole
output buffer.  The narrow kernel gives every accumulator the wide kernel's chain (the 16-bit K walk, with w_wrap_k and lda > K, then -- A6 / W6 -- one block-scaled
e2m3 MFMA per 128-value step) and every element the wide kernel's epilogue (bias, the half-split rotation with the rope_rows table's values by the same two contracted
forms, 16-bit rounding inside the fp16 saturation window, hi | lo), so equality is by construction and is the acceptance test.

Every case makes two calls on the same operands, tile_qkv = 0 then tile_qkv = 2, each on a fresh sentinel-filled buffer [M + XROWS, ldc], and checks (a) the two buffers'
bits -- hi half, lo half, the sentinels in columns N .. ldc - 1, in the hi | lo gap and in rows >= M; (b) the host counters: gemm_narrow_qkv_launches() + 0 / + 1, the
two older counters unmoved (without them equality would hold vacuously on a library that ignores the field); (c) the narrow output against the float64 reference
R.epi_qkv at test_gemm_gpu.py's tolerance.

Forms: plain output over the plain walk, over the compensated layout (lda = 2 K) and over the w_wrap_k walk; hi | lo output over the plain and the w_wrap_k walk and
behind the e2m3 second pass (the images built by the tile_qkv = 0 call, read by the other).  Shapes: heads (1,1) .. (4,2) -- N = 384 .. 1024, the rope / plain boundary at
every 64-column tile edge position inside a 256-column tile; M over the 64-row tile edges, two tiles + 1, a second 256-row image (257, 326); K = 64 .. 384 around the
four-slot ring, K6 of 1 - 5 second-pass steps, K = 3584 once per pass structure; ldc = 4 mod 8 (the wide kernel's element-store path); rope_stride > M."""
import types

import numpy as np
import pytest
import torch

import gemm_inputs as GI
import test_gemm_gpu as TG
from blim_amd import engine as eng
from oracle import gemm_ref as R

pytestmark = pytest.mark.gpu

MS = (1, 63, 64, 65, 129, 257, 326)


def _cases():
    """(form, (nh, nkv), M, K, dtype, ld4).  K: the length of ONE walk (wrap forms walk it twice, lo6 adds K6 = K)."""
    out = []
    dt = lambda i: ("f16", "bf16")[i % 2]
    for heads in TG.QKV_HEADS:                                                           # every head layout, every output form, both dtypes
        for form in ("plain", "split", "lo6"):
            for dtype in TG.DTYPES:
                out.append((form, heads, 326, 128, dtype, False))
    for i, M in enumerate(MS):                                                           # every M edge
        for j, form in enumerate(("plain", "split", "lo6")):
            out.append((form, (2, 1), M, 128 if form == "lo6" else 192, dt(i + j), False))
    for i, K in enumerate((64, 128, 192, 256, 320, 384)):                                # the K walk around the ring's depth of four
        for j, form in enumerate(("plain", "split")):
            out.append((form, (1, 1), 129, K, dt(i + j), False))
    for K in (128, 256, 384, 512, 640):                                                  # second pass: 1 - 5 steps behind 2 - 10
        for dtype in TG.DTYPES:
            out.append(("lo6", (2, 1), 257, K, dtype, False))
    for i, K in enumerate((64, 192, 320)):                                               # the w_wrap_k walk, with and without lo_off
        for form in ("wrap", "splitwrap"):
            for j, dtype in enumerate(TG.DTYPES):
                out.append((form, (2, 1), (65, 257)[(i + j) % 2], K, dtype, False))
    for dtype in TG.DTYPES:                                                              # a plain unit over the compensated layout
        out.append(("plain2k", (3, 1), 129, 128, dtype, False))
    for form in ("plain", "split", "lo6", "splitwrap"):                                  # ldc = 4 mod 8
        for dtype in TG.DTYPES:
            out.append((form, (1, 1), 257, 128, dtype, True))
    out += [("plain", (4, 2), 326, 3584, "f16", False), ("lo6", (1, 1), 326, 3584, "bf16", False)]
    return out


CASES = _cases()


def _problem(form, heads, M, K, dtype):
    """Operands in W's stored row order, the device table and the float64 reference."""
    nh, nkv = heads
    c = types.SimpleNamespace(M=M, nh=nh, nkv=nkv, K=K, N=(nh + 2 * nkv) * 128, kw={}, lda=K, Kcall=K)
    N = c.N
    c.pos = GI.positions(M, form)
    if form == "plain":
        q = GI.qkv_case(M, nh, nkv, K, dtype, tag="narrow")
        c.a, c.w, c.bias, c.pos, acc, A, chain = q.a, q.w, q.bias, q.pos, q.acc, q.A, K
    elif form == "split":
        q = GI.qkv_case(M, nh, nkv, K, dtype, tag="narrow-split")
        c.a, c.w, c.bias, c.pos, acc, A, chain = q.a, q.w, q.bias, q.pos, q.acc, q.A, K
    elif form in ("wrap", "splitwrap"):
        c.a, c.w = GI.wrapped(M, N, K, dtype, tag="narrow-qkv")
        acc, A = R.product(c.a, c.w, w_wrap_k=K)
        c.bias, chain, c.lda, c.Kcall = GI.bias_for(N, K, "narrow-qkv"), 2 * K, 2 * K, 2 * K
        c.kw["w_wrap_k"] = K
    else:                                                                                # "plain2k", "lo6": a = [hi | lo] with true lo parts
        c.a, c.w, acc6, A6 = TG.lo6_operands(M, N, K, dtype, tag="narrow-qkv")
        c.bias, c.lda = GI.bias_for(N, K, "narrow-qkv"), 2 * K
        if form == "lo6":
            acc, A, chain = acc6, A6, 2 * K
        else:
            acc, A = R.product(c.a[:, :K], c.w)
            chain = K
    c.stride = M + 9                                                                     # rope_stride > M
    c.table, cos, sin = TG.rope_table(c.pos, c.stride)
    c.ref, c.pre = R.epi_qkv(acc, A, chain, c.bias, cos.astype(np.float64), sin.astype(np.float64), nh, nkv)
    return c


def _counters():
    return eng.gemm_narrow_qkv_launches(), eng.gemm_narrow_launches(), eng.gemm_narrow_lo6_launches()


def _call(c, dev, dtype, o, **fields):
    kw = dict(c.kw)
    kw.update(fields)
    eng.gemm("qkv", dtype, dev.a, dev.w, c.M, c.N, c.Kcall, o.t, lda=c.lda, bias=dev.bias, rope_cols=(c.nh + c.nkv) * 128, rope_rows=c.table, rope_stride=c.stride,
             lo_off=o.lo_off, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) if isinstance(x, bool) else "x".join(map(str, x)) if isinstance(x, tuple) else str(x) for x in c))
def test_narrow_qkv_equals_the_wide_kernel_bit_for_bit(case):
    form, heads, M, K, dtype, ld4 = case
    c = _problem(form, heads, M, K, dtype)
    dev = types.SimpleNamespace(a=TG.dev16(c.a, dtype), w=TG.dev16(c.w, dtype), bias=TG.dev32(c.bias))
    split = form in ("split", "splitwrap", "lo6")
    wide, narrow = TG.Out16(M, c.N, dtype, ld4, split), TG.Out16(M, c.N, dtype, ld4, split)
    f6_wide, f6_narrow = {}, {}
    if form == "lo6":
        a6, w6 = TG.f6_buffers(M, c.N, K)
        f6_wide, f6_narrow = dict(A6=a6, W6=w6, f6_build=1), dict(A6=a6, W6=w6, K6=K, f6_build=0)
    n0 = _counters()
    _call(c, dev, dtype, wide, tile_qkv=0, **f6_wide)
    assert _counters() == n0, "tile_qkv = 0 launched a narrow kernel"
    _call(c, dev, dtype, narrow, tile_qkv=2, **f6_narrow)
    n1 = _counters()
    assert n1[0] == n0[0] + 1, "tile_qkv = 2 did not launch the narrow QKV kernel (exactly once)"
    assert n1[1:] == n0[1:], "an older narrow kernel's counter moved"
    TG.check16(narrow, c.ref, c.pre, "narrow_qkv", form=form, nh=heads[0], nkv=heads[1], M=M, K=K)      # (c), and every sentinel of the narrow buffer
    diff = TG.host16(wide.t) != narrow.raw                                                                   # (a): the whole buffer
    where = np.argwhere(diff)
    TG.measure(test="narrow_qkv_bits", form=form, dtype=dtype, M=M, N=c.N, K=K, differing=int(diff.sum()))
    assert not diff.any(), f"{int(diff.sum())} elements differ from the 256 x 256 kernel's, first at {where[0]}, columns {sorted(set((where[:, 1] % narrow.ldc).tolist()))[:16]}"


# ---------------------------------------------------------------------------- fp16 saturation
@pytest.mark.parametrize("saturate", [1, 0])
@pytest.mark.parametrize("split", [False, True])
def test_f16_saturation_is_the_wide_kernels(split, saturate):
    """test_gemm_gpu.test_f16_saturation's QKV case on both kernels: accumulators of +-131072 leave as +-65504 (f16_saturate = 1) or +-inf (0), a NaN operand as NaN."""
    dtype, M, K, N = "f16", 257, 64, 384
    a = np.full((M, K), 8.0)
    w = np.full((N, K), 256.0)
    w[1::2] = -256.0
    a[5, 3] = np.nan
    table, _, _ = TG.rope_table(np.zeros(M, np.int32), M)                                # position 0: the identity rotation
    ad, wd, bias = TG.dev16(a, dtype), TG.dev16_bits(R.bits16(w, dtype), dtype), TG.dev32(np.zeros(N))
    outs = []
    n0 = _counters()
    for tile in (0, 2):
        o = TG.Out16(M, N, dtype, split=split)
        eng.gemm("qkv", dtype, ad, wd, M, N, K, o.t, f16_saturate=saturate, lo_off=o.lo_off, bias=bias, rope_cols=256, rope_rows=table, rope_stride=M, tile_qkv=tile)
        torch.cuda.synchronize()
        outs.append(o)
    assert _counters() == (n0[0] + 1,) + n0[1:]
    hi, _ = outs[1].read()
    assert np.isnan(hi[5]).all(), "a NaN operand did not give NaN"
    big = 65504.0 if saturate else np.inf
    sign = np.where(np.arange(N) % 2 == 1, -1.0, 1.0)                                    # (the row permutation keeps a row's parity: test_gemm_gpu.py)
    rest = np.delete(hi, 5, axis=0)
    assert np.array_equal(rest, np.broadcast_to(big * sign, rest.shape)), (split, saturate)
    assert np.array_equal(TG.host16(outs[0].t), outs[1].raw), "the two kernels' buffers differ"


# ---------------------------------------------------------------------------- refusals: nothing launched, C still all sentinel, the field named
def _small(dtype="f16", M=8, N=384, K=128):
    a, w, _, _ = TG.lo6_operands(M, N, K, "f16" if dtype == "f8" else dtype, tag="refuse-qkv")
    if dtype == "f8":
        return TG.dev8(a[:, :K]), TG.dev8(w)
    return TG.dev16(a, dtype), TG.dev16(w, dtype)


def _qkv_kw(M, N):
    table, _, _ = TG.rope_table(GI.positions(M), M)
    return dict(bias=TG.dev32(np.zeros(N)), rope_cols=256, rope_rows=table, rope_stride=M)


def test_tile_qkv_outside_its_range_f8_and_the_second_pass_without_lo_off_are_refused():
    M, N, K = 8, 384, 128
    a, w = _small()
    c = TG.sent16(M, 2 * N + 16, "f16")
    kw = _qkv_kw(M, N)
    a6, w6 = TG.f6_buffers(M, N, K)
    n0 = _counters()
    for v in (3, -1):
        with pytest.raises(eng.BlimError, match=r"tile_qkv = "):
            eng.gemm("qkv", "f16", a, w, M, N, K, c, lda=2 * K, tile_qkv=v, **kw)
    with pytest.raises(eng.BlimError, match=r"tile_qkv = 2.*lo_off"):
        eng.gemm("qkv", "f16", a, w, M, N, K, c, lda=2 * K, A6=a6, W6=w6, f6_build=1, tile_qkv=2, **kw)
    a8, w8 = _small("f8")
    with pytest.raises(eng.BlimError, match=r"tile_qkv = 2.*dtype"):
        eng.gemm("qkv", "f8", a8, w8, M, N, K, c, tile_qkv=2, row_scale=TG.dev32(np.ones(M)), col_scale=TG.dev32(np.ones(N)), **kw)
    torch.cuda.synchronize()
    assert _counters() == n0 and (TG.host16(c) == TG.SENT16).all()
    assert (a6.cpu().numpy() == TG.SENT8).all() and (w6.cpu().numpy() == TG.SENT8).all()


@pytest.mark.parametrize("epi", ["bf16", "f32", "resid", "swiglu", "lse"])
def test_tile_qkv_2_is_refused_with_every_other_epilogue(epi):
    M, N, K = 8, 384, 128
    a, w = _small()
    c = None if epi == "lse" else (TG.sent32(M, N + 4) if epi in ("f32", "resid") else TG.sent16(M, N + 8, "f16"))
    n0 = _counters()
    with pytest.raises(eng.BlimError, match=r"tile_qkv = 2.*epi"):
        eng.gemm(epi, "f16", a, w, M, N, K, c, lda=2 * K, tile_qkv=2)
    torch.cuda.synchronize()
    assert _counters() == n0
    if c is not None:
        assert (TG.bits32(c) == TG.SENT32).all() if c.dtype == torch.float32 else (TG.host16(c) == TG.SENT16).all()


def test_the_older_fields_keep_refusing_qkv():
    """`tile` = 2 and `tile_lo6` = 2 refuse the QKV epilogue as before, whatever tile_qkv says."""
    M, N, K = 8, 384, 128
    a, w = _small()
    c = TG.sent16(M, 2 * N + 16, "f16")
    kw = _qkv_kw(M, N)
    n0 = _counters()
    for v in (0, 1, 2):
        with pytest.raises(eng.BlimError, match=r"tile = 2.*epi"):
            eng.gemm("qkv", "f16", a, w, M, N, K, c, lda=2 * K, tile=2, tile_qkv=v, **kw)
        with pytest.raises(eng.BlimError, match=r"tile_lo6 = 2.*epi"):
            eng.gemm("qkv", "f16", a, w, M, N, K, c, lda=2 * K, tile_lo6=2, tile_qkv=v, **kw)
    torch.cuda.synchronize()
    assert _counters() == n0 and (TG.host16(c) == TG.SENT16).all()


# ---------------------------------------------------------------------------- tile_qkv = 1: both sides of the auto rule, the threshold read from the library
def test_auto_rule_both_sides():
    T = eng.gemm_narrow_qkv_threshold()                                                  # narrow when ceil(M / 256) * ceil(N / 256) < T
    assert 0 <= T <= 512
    K, dtype = 64, "f16"

    def pair(M, N):
        """The tile_qkv = 1 and the tile_qkv = 0 result on the same operands, and how far the auto call moved the counters."""
        a, w = GI.moderate(M, N, K, dtype, "auto-qkv")
        ad, wd = TG.dev16(a, dtype), TG.dev16(w, dtype)
        table, _, _ = TG.rope_table(GI.positions(M), M)
        kw = dict(bias=TG.dev32(GI.bias_for(N, K, "auto-qkv")), rope_cols=N - 128, rope_rows=table, rope_stride=M)
        ref = TG.sent16(M, N + 8, dtype)
        eng.gemm("qkv", dtype, ad, wd, M, N, K, ref, tile_qkv=0, **kw)
        n0 = _counters()
        got = TG.sent16(M, N + 8, dtype)
        eng.gemm("qkv", dtype, ad, wd, M, N, K, got, tile_qkv=1, **kw)
        torch.cuda.synchronize()
        n1 = _counters()
        assert n1[1:] == n0[1:]
        return got, ref, n1[0] - n0[0]

    got, ref, n = pair(65, 384)                                                          # two tiles of 256 x 256
    assert n == (1 if T > 2 else 0) and torch.equal(got.view(torch.int16), ref.view(torch.int16))
    got, ref, n = pair(256, 256 * max(T, 1))                                             # exactly T tiles: not below the threshold
    assert n == 0, "a grid of `threshold` tiles took the narrow kernel"
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    if T > 1:                                                                            # ... and T - 1 tiles: the last grid below it
        got, ref, n = pair(256, 256 * (T - 1))
        assert n == 1 and torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_an_ineligible_form_under_auto_takes_the_wide_kernel_silently():
    M, N, K, dtype = 8, 384, 128, "f16"
    a, w = _small()
    n0 = _counters()
    c = TG.sent32(M, N + 4)
    c[:, :N] = 0
    eng.gemm("resid", dtype, a, w, M, N, K, c, lda=2 * K, tile_qkv=1)                    # another epilogue
    o = TG.sent16(M, N // 2 + 8, dtype)
    eng.gemm("swiglu", dtype, a, w, M, N, K, o, lda=2 * K, tile_qkv=1)
    a8, w8 = _small("f8")
    o8 = TG.sent16(M, N + 8, dtype)
    eng.gemm("qkv", "f8", a8, w8, M, N, K, o8, tile_qkv=1, row_scale=TG.dev32(np.ones(M)), col_scale=TG.dev32(np.ones(N)), **_qkv_kw(M, N))      # fp8 QKV
    torch.cuda.synchronize()
    assert _counters() == n0
    assert (TG.bits32(c)[:, :N] != TG.SENT32).all() and (TG.bits32(c)[:, N:] == TG.SENT32).all()
    assert (TG.host16(o)[:, :N // 2] != TG.SENT16).all() and (TG.host16(o8)[:, :N] != TG.SENT16).all()
