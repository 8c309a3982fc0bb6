"""GPU: the narrow-tile residual GEMM with the e2m3 second pass (csrc/gemm.hip: gemm_narrow_lo6_kernel; blim_gemm's `tile_lo6`) against the 256 x 256 kernel on the
same operands and the SAME A6 / W6 tile images, BIT FOR BIT on every element of C: the narrow kernel gives every accumulator the wide kernel's chain -- the 16-bit
walk over the hi operand, then one block-scaled e2m3 MFMA per 128-value K-step in ascending order -- so equality is by construction and is the acceptance test.

Operands are test_gemm_gpu.lo6_operands' (A = [hi | lo] with lda = 2 K and true lo parts, ragged block magnitudes).  The images are built once per case by the
tile_lo6 = 0 call (f6_build = 1); the tile_lo6 = 2 call reads them (f6_build = 0) on a fresh sentinel-framed C.  Every case checks (1) the bits; (2) the two host
counters: gemm_narrow_lo6_launches() + 1 per tile_lo6 = 2 call and + 0 per tile_lo6 = 0 call, gemm_narrow_launches() unmoved by both -- without them the equality
would hold vacuously on a library that ignores the field; (3) C against the float64 reference hi . w + e2m3(lo) . e2m3(w) within test_gemm_gpu.py's tolerance for the
residual epilogue (chain length 2 K, as the other lo6 tests pass it); (4) the sentinels in columns N .. ldc - 1 and rows >= M; (5) the image bytes after the call.

Shapes: M over every 64-row quarter q = 0 .. 3 of a 256-row image tile, both 128-row scale halves and a second image; N over the element-store path (134), a partial
tile (136), the column groups qn = 2, 3 and a second W image; K = K6 of 2 - 10 first-pass and 1 - 5 second-pass steps around the four-slot ring; one case each at
N = 3584, K = 3584 and down's K = 18944; in place and with resid_in, with and without bias."""
import types

import numpy as np
import pytest
import torch

import gemm_inputs as GI
import test_gemm_gpu as TG
from blim_amd import engine as eng
from oracle import gemm_ref as R

pytestmark = pytest.mark.gpu

MS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 500)
NS = (128, 134, 136, 192, 256, 320, 384)
KS = (128, 256, 384, 512, 640)


def _cases():
    """(M, N, K, dtype, with_in, with_bias): a pruned cross product of MS x NS x KS."""
    out = []
    dt = lambda i: ("f16", "bf16")[i % 2]
    flip = lambda i: (bool(i & 1), bool(i & 2))
    for i, M in enumerate(MS):                                                           # every M edge, a partial N tile, ring depth + 2 / + 3 steps
        out.append((M, 136, 384, dt(i)) + flip(i))
    for i, N in enumerate(NS):                                                           # every N, both dtypes
        for j, dtype in enumerate(("f16", "bf16")):
            out.append((129, N, 256, dtype) + flip(i + j))
    for i, K in enumerate(KS):                                                           # the K walk, both dtypes; q = 3, qn = 0 .. 2
        for j, dtype in enumerate(("f16", "bf16")):
            out.append((193, 192, K, dtype) + flip(i + j + 1))
    for i, (M, N, K) in enumerate(((255, 320, 128), (191, 384, 640), (257, 134, 512), (500, 256, 640), (63, 320, 512), (256, 384, 128), (192, 128, 640), (65, 192, 128))):
        out.append((M, N, K, dt(i + 1)) + flip(i))
    out += [(257, 3584, 128, "f16", True, True), (500, 384, 3584, "bf16", False, False), (65, 136, 18944, "f16", False, True)]
    for dtype in ("f16", "bf16"):                                                        # the four residual / bias forms at one shape
        for i in range(4):
            out.append((127, 136, 128, dtype) + flip(i))
    return out


CASES = _cases()


def _problem(M, N, K, dtype, with_in, with_bias):
    c = types.SimpleNamespace(M=M, N=N, K=K)
    c.a, c.w, acc, A = TG.lo6_operands(M, N, K, dtype, tag="narrow")
    g = GI.rng("narrow-lo6-resid", M, N, K, dtype)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    c.c_before = f32(g.randn(M, N))
    c.resid_in = f32(g.randn(M, N)) if with_in else None
    c.bias = GI.bias_for(N, K, "narrow-lo6") if with_bias else None
    c.ref, c.pre = R.epi_resid(acc, A, 2 * K, c.resid_in if with_in else c.c_before, c.bias)
    return c


def _run(c, dtype, dev, **fields):
    """One call on a fresh C buffer [M + XROWS, ldc] (sentinels outside [M, N]); returns the buffer's bits before and after, and the tensor."""
    M, N = c.M, c.N
    ldc = (N + 3) // 4 * 4 + 4
    buf = np.full((M + TG.XROWS, ldc), TG.SENT32, np.int32)
    if c.resid_in is None:
        buf[:M, :N] = c.c_before.astype(np.float32).view(np.int32)
    t = torch.from_numpy(buf).cuda().view(torch.float32)
    kw = dict(dev.kw)
    if c.resid_in is not None:
        rin = np.full((M, ldc), np.nan, np.float32)
        rin[:, :N] = c.resid_in
        kw["resid_in"] = torch.from_numpy(rin).cuda()
    kw.update(fields)
    eng.gemm("resid", dtype, dev.a, dev.w, M, N, c.K, t, lda=2 * c.K, **kw)
    torch.cuda.synchronize()
    return buf, TG.bits32(t), t


def _dev(c, dtype):
    dev = types.SimpleNamespace(a=TG.dev16(c.a, dtype), w=TG.dev16(c.w, dtype), kw={})
    if c.bias is not None:
        dev.kw["bias"] = TG.dev32(c.bias)
    return dev


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) if isinstance(x, bool) else str(x) for x in c))
def test_narrow_lo6_equals_the_wide_kernel_bit_for_bit(case):
    M, N, K, dtype, with_in, with_bias = case
    c = _problem(*case)
    dev = _dev(c, dtype)
    a6, w6 = TG.f6_buffers(M, N, K)
    n0, p0 = eng.gemm_narrow_lo6_launches(), eng.gemm_narrow_launches()
    before, wide, _ = _run(c, dtype, dev, A6=a6, W6=w6, f6_build=1, tile_lo6=0)
    assert eng.gemm_narrow_lo6_launches() == n0, "tile_lo6 = 0 launched the narrow kernel"
    img_a, img_w = a6.cpu().numpy().copy(), w6.cpu().numpy().copy()
    _, narrow, t = _run(c, dtype, dev, A6=a6, W6=w6, K6=K, f6_build=0, tile_lo6=2)
    assert eng.gemm_narrow_lo6_launches() == n0 + 1, "tile_lo6 = 2 did not launch the narrow e2m3 kernel (exactly once)"
    assert eng.gemm_narrow_launches() == p0, "the plain narrow kernel's counter moved"
    got = TG.read_f32(t, M, N, before=before)                                            # sentinels: columns N .. ldc - 1, rows >= M
    x = TG.ratio(got, c.ref, R.tolerance(c.ref, c.pre, "f32"))
    diff = narrow != wide
    TG.measure(test="narrow_lo6", dtype=dtype, M=M, N=N, K=K, resid_in=int(with_in), bias=int(with_bias), ratio=x, differing=int(diff.sum()))
    assert x <= 1.0, (case, x)
    assert not diff.any(), f"{int(diff.sum())} elements differ from the 256 x 256 kernel's, first at {np.argwhere(diff)[0]}"
    assert np.array_equal(a6.cpu().numpy(), img_a) and np.array_equal(w6.cpu().numpy(), img_w), "the narrow call changed a tile image"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_the_inputs_let_a_missing_second_pass_show(dtype):
    """The same call without A6 / W6 (the hi product alone, on the plain narrow kernel) differs from the compensated result on most elements."""
    case = (193, 192, 256, dtype, False, False)
    c = _problem(*case)
    dev = _dev(c, dtype)
    a6, w6 = TG.f6_buffers(c.M, c.N, c.K)
    _run(c, dtype, dev, A6=a6, W6=w6, f6_build=1, tile_lo6=0)
    _, both, _ = _run(c, dtype, dev, A6=a6, W6=w6, K6=c.K, tile_lo6=2)
    _, hi_only, _ = _run(c, dtype, dev, tile=2)
    differing = (both[:c.M, :c.N] != hi_only[:c.M, :c.N]).mean()
    TG.measure(test="narrow_lo6_second_pass_shows", dtype=dtype, differing=float(differing))
    assert differing > 0.5, differing


# ---------------------------------------------------------------------------- refusals: nothing launched, C still all sentinel, the field named
def _small(dtype="f16", M=8, N=128, K=128):
    a, w, _, _ = TG.lo6_operands(M, N, K, "f16" if dtype == "f8" else dtype, tag="refuse")
    if dtype == "f8":
        return TG.dev8(a[:, :K]), TG.dev8(w)
    return TG.dev16(a, dtype), TG.dev16(w, dtype)


def _counters():
    return eng.gemm_narrow_lo6_launches(), eng.gemm_narrow_launches()


def test_tile_lo6_outside_its_range_and_without_the_second_pass_is_refused():
    a, w = _small()
    c = TG.sent32(8, 132)
    a6, w6 = TG.f6_buffers(8, 128, 128)
    n0 = _counters()
    for v in (3, -1):
        with pytest.raises(eng.BlimError, match=r"tile_lo6 = "):
            eng.gemm("resid", "f16", a, w, 8, 128, 128, c, lda=256, A6=a6, W6=w6, K6=128, tile_lo6=v)
        with pytest.raises(eng.BlimError, match=r"tile_lo6 = "):
            eng.gemm("resid", "f16", a, w, 8, 128, 128, c, lda=256, tile_lo6=v)
    with pytest.raises(eng.BlimError, match=r"tile_lo6 = 2.*A6"):
        eng.gemm("resid", "f16", a, w, 8, 128, 128, c, lda=256, tile_lo6=2)
    a8, w8 = _small("f8")
    with pytest.raises(eng.BlimError, match=r"tile_lo6 = 2.*dtype"):
        eng.gemm("resid", "f8", a8, w8, 8, 128, 128, c, tile_lo6=2, row_scale=TG.dev32(np.ones(8)), col_scale=TG.dev32(np.ones(128)))
    with pytest.raises(eng.BlimError, match=r"tile_lo6 = 2.*w_wrap_k"):
        eng.gemm("resid", "f16", a, w, 8, 128, 256, c, lda=256, w_wrap_k=128, A6=a6, W6=w6, K6=128, tile_lo6=2)
    torch.cuda.synchronize()
    assert _counters() == n0 and (TG.bits32(c) == TG.SENT32).all()
    assert (a6.cpu().numpy() == TG.SENT8).all() and (w6.cpu().numpy() == TG.SENT8).all()


@pytest.mark.parametrize("epi", ["qkv", "swiglu", "lse"])
def test_tile_lo6_2_is_refused_with_every_other_epilogue(epi):
    a, w = _small()
    a6, w6 = TG.f6_buffers(8, 128, 128)
    c = None if epi == "lse" else TG.sent16(8, 264, "f16")
    n0 = _counters()
    with pytest.raises(eng.BlimError, match=r"tile_lo6 = 2.*epi"):
        eng.gemm(epi, "f16", a, w, 8, 128, 128, c, lda=256, A6=a6, W6=w6, K6=128, tile_lo6=2)
    torch.cuda.synchronize()
    assert _counters() == n0
    if c is not None:
        assert (TG.host16(c) == TG.SENT16).all()


def test_tile_keeps_its_refusal_of_the_second_pass():
    """`tile` = 2 with A6 / W6 is refused as before, whatever tile_lo6 says: the two fields choose for disjoint forms."""
    a, w = _small()
    c = TG.sent32(8, 132)
    a6, w6 = TG.f6_buffers(8, 128, 128)
    n0 = _counters()
    for v in (0, 1, 2):
        with pytest.raises(eng.BlimError, match=r"tile = 2.*A6"):
            eng.gemm("resid", "f16", a, w, 8, 128, 128, c, lda=256, tile=2, tile_lo6=v, A6=a6, W6=w6, K6=128)
    torch.cuda.synchronize()
    assert _counters() == n0 and (TG.bits32(c) == TG.SENT32).all()


# ---------------------------------------------------------------------------- tile_lo6 = 1: both sides of the auto rule, the threshold read from the library
def test_auto_rule_both_sides():
    T = eng.gemm_narrow_lo6_threshold()                                                  # narrow when ceil(M / 256) * ceil(N / 256) < T
    assert 0 <= T <= 512
    K, dtype = 128, "f16"

    def pair(M, N):
        """The tile_lo6 = 1 and the tile_lo6 = 0 result on the same images, and how far the auto call moved the counter."""
        a, w, _, _ = TG.lo6_operands(M, N, K, dtype, tag="auto")
        ad, wd = TG.dev16(a, dtype), TG.dev16(w, dtype)
        a6, w6 = TG.f6_buffers(M, N, K)
        ref = torch.zeros((M, N + 4), dtype=torch.float32, device="cuda")
        eng.gemm("resid", dtype, ad, wd, M, N, K, ref, lda=2 * K, A6=a6, W6=w6, f6_build=1, tile_lo6=0)
        n0 = _counters()
        got = torch.zeros((M, N + 4), dtype=torch.float32, device="cuda")
        eng.gemm("resid", dtype, ad, wd, M, N, K, got, lda=2 * K, A6=a6, W6=w6, K6=K, tile_lo6=1)
        torch.cuda.synchronize()
        n1 = _counters()
        assert n1[1] == n0[1]
        return got, ref, n1[0] - n0[0]

    got, ref, n = pair(65, 136)                                                          # one tile of 256 x 256
    assert n == (1 if T > 1 else 0) and torch.equal(got, ref)
    got, ref, n = pair(256, 256 * max(T, 1))                                             # exactly T tiles: not below the threshold
    assert n == 0, "a grid of `threshold` tiles took the narrow kernel"
    assert torch.equal(got, ref)
    if T > 1:                                                                            # ... and T - 1 tiles: the last grid below it
        got, ref, n = pair(256, 256 * (T - 1))
        assert n == 1 and torch.equal(got, ref)


def test_an_ineligible_form_under_auto_takes_the_wide_kernel_silently():
    M, N, K, dtype = 8, 128, 128, "f16"
    a, w = _small()
    n0 = _counters()
    c = TG.sent32(M, N + 4)
    c[:, :N] = 0
    eng.gemm("resid", dtype, a, w, M, N, K, c, lda=2 * K, tile_lo6=1)                    # no second pass: `tile`'s form, and tile = 0
    eng.gemm("resid", dtype, a, w, M, N, 2 * K, c, lda=2 * K, w_wrap_k=K, tile_lo6=1)    # the w_wrap_k form
    a6, w6 = TG.f6_buffers(M, N, K)
    o = TG.sent16(M, 136, dtype)
    eng.gemm("swiglu", dtype, a, w, M, N, K, o, lda=2 * K, A6=a6, W6=w6, f6_build=1, tile_lo6=1)   # another epilogue with the second pass
    torch.cuda.synchronize()
    assert _counters() == n0
    assert (TG.bits32(c)[:, :N] != TG.SENT32).all() and (TG.bits32(c)[:, N:] == TG.SENT32).all()
    assert (TG.host16(o)[:, :N // 2] != TG.SENT16).all()
