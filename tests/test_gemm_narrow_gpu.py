"""GPU: the narrow-tile residual GEMM (csrc/gemm.hip: gemm_narrow_kernel; blim_gemm's `tile`) against the 256 x 256 kernel on the same buffers, BIT FOR BIT on every
element of C -- the narrow kernel walks K in the same order with the same MFMAs, so equality is by construction and is the acceptance test.

Inputs are the real-valued families of tests/gemm_inputs.py (small integers sum exactly in any order and would hide a wrong K walk).  Every case also checks
(1) the host-side counter of narrow launches: + 1 per tile = 2 call, + 0 per tile = 0 call -- without it the bit-equality would hold vacuously on a library that
ignores `tile`; (2) C against the float64 reference of oracle/gemm_ref.py within test_gemm_gpu.py's tolerance for the residual epilogue; (3) the sentinels in the
columns N .. ldc - 1 and in the rows behind M.  Shapes: the smallest that can go wrong -- M and N around the 64-row / 64-column tile and the 256-tile of the other
kernel, N = 136 (a partial tile) and N = 134 (the element-store path: col + 3 >= N), K of one step, the four-step ring's depth - 1 / depth + 1 / + 2, many wraps
(3584) and down's real K (18944); in place and with resid_in, with and without bias, the w_wrap_k form (K = 2 w_wrap_k) and lda = 2 K."""
import types

import numpy as np
import pytest
import torch

import gemm_inputs as GI
import test_gemm_gpu as TG
from blim_amd import engine as eng
from oracle import gemm_ref as R

pytestmark = pytest.mark.gpu


def _cases():
    """(M, N, K, dtype, form, with_in, with_bias); K is the GEMM's K (the wrap form: both halves).  A pruned cross-product of the issue's M, N and K sets."""
    out = []
    flip = lambda i: (bool(i & 1), bool(i & 2))
    for i, M in enumerate((1, 63, 64, 65, 127, 128, 129, 257, 500)):                    # every M edge, one partial N tile, ring depth + 1
        out.append((M, 136, 320, ("f16", "bf16")[i % 2], "plain") + flip(i))
    for i, N in enumerate((128, 134, 136, 256, 384)):                                   # every N, both dtypes
        for dtype in ("f16", "bf16"):
            out.append((65, N, 384, dtype, "plain") + flip(i + (dtype == "bf16")))
    for dtype in ("f16", "bf16"):
        out.append((257, 3584, 128, dtype, "plain", dtype == "f16", True))              # 5 x 56 narrow tiles, 2 x 14 wide ones
    for i, K in enumerate((64, 128, 192, 256, 320, 384)):                               # the K walk: 1 - 6 steps around the ring's depth of four
        for dtype in ("f16", "bf16"):
            out.append((129, 136, K, dtype, "plain") + flip(i))
    out += [(500, 384, 3584, "f16", "plain", False, False), (64, 3584, 3584, "bf16", "plain", True, False),
            (65, 136, 18944, "bf16", "plain", False, True), (500, 256, 18944, "f16", "plain", True, True)]
    for i, K in enumerate((128, 384, 640, 3584)):                                       # w_wrap_k = K / 2: W's K-step index wraps inside the ring
        for j, M in enumerate((63, 257)):
            out.append((M, (136, 256)[j], K, ("f16", "bf16")[(i + j) % 2], "wrap") + flip(i + j))
    out.append((127, 134, 18944, "bf16", "wrap", False, True))
    for i, K in enumerate((64, 320, 384)):                                              # lda = 2 K: a plain unit over [hi | lo] rows reads the hi halves
        for j, M in enumerate((1, 128, 500)):
            out.append((M, (128, 136, 384)[j], K, ("f16", "bf16")[(i + j) % 2], "lda2") + flip(i + j))
    for dtype in ("f16", "bf16"):                                                       # the four residual / bias forms at one shape
        for i in range(4):
            out.append((127, 136, 128, dtype, "plain") + flip(i))
    return out


CASES = _cases()


def _problem(M, N, K, dtype, form, with_in, with_bias):
    c = types.SimpleNamespace(M=M, N=N, K=K, lda=K, wrap=0)
    if form == "wrap":
        c.a, c.w = GI.wrapped(M, N, K // 2, dtype, "narrow")
        c.wrap = K // 2
        acc, A = R.product(c.a, c.w, w_wrap_k=K // 2)
    elif form == "lda2":
        c.a, c.w = GI.wrapped(M, N, K, dtype, "narrow-lda")                              # [M, 2 K] rows: the second halves must not be read
        c.lda = 2 * K
        acc, A = R.product(c.a[:, :K], c.w)
    else:
        c.a, c.w = GI.moderate(M, N, K, dtype, "narrow")
        acc, A = R.product(c.a, c.w)
    g = GI.rng("narrow-resid", M, N, K, dtype, form)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    c.c_before = f32(g.randn(M, N))
    c.resid_in = f32(g.randn(M, N)) if with_in else None
    c.bias = GI.bias_for(N, K, "narrow") if with_bias else None
    c.ref, c.pre = R.epi_resid(acc, A, K, c.resid_in if with_in else c.c_before, c.bias)
    return c


def _run(c, dtype, tile, dev):
    """One call on a fresh C buffer [M + XROWS, ldc] (sentinels outside [M, N]); returns the buffer's bits before and after."""
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
    eng.gemm("resid", dtype, dev.a, dev.w, M, N, c.K, t, lda=c.lda, tile=tile, **kw)
    torch.cuda.synchronize()
    return buf, TG.bits32(t), t


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) if isinstance(x, bool) else str(x) for x in c))
def test_narrow_equals_the_wide_kernel_bit_for_bit(case):
    M, N, K, dtype, form, with_in, with_bias = case
    c = _problem(*case)
    dev = types.SimpleNamespace(a=TG.dev16(c.a, dtype), w=TG.dev16(c.w, dtype), kw={})
    if c.wrap:
        dev.kw["w_wrap_k"] = c.wrap
    if c.bias is not None:
        dev.kw["bias"] = TG.dev32(c.bias)
    n0 = eng.gemm_narrow_launches()
    before, wide, _ = _run(c, dtype, 0, dev)
    assert eng.gemm_narrow_launches() == n0, "tile = 0 launched the narrow kernel"
    _, narrow, t = _run(c, dtype, 2, dev)
    assert eng.gemm_narrow_launches() == n0 + 1, "tile = 2 did not launch the narrow kernel (exactly once)"
    got = TG.read_f32(t, M, N, before=before)                                           # sentinels: columns N .. ldc - 1, rows >= M
    x = TG.ratio(got, c.ref, R.tolerance(c.ref, c.pre, "f32"))
    diff = narrow != wide
    TG.measure(test="narrow", dtype=dtype, M=M, N=N, K=K, form=form, resid_in=int(with_in), bias=int(with_bias), ratio=x, differing=int(diff.sum()))
    assert x <= 1.0, (case, x)
    assert not diff.any(), f"{int(diff.sum())} elements differ from the 256 x 256 kernel's, first at {np.argwhere(diff)[0]}"


# ---------------------------------------------------------------------------- refusals: every form the narrow kernel does not exist for, the field named
def _small(dtype="f16", M=8, N=128, K=128):
    a, w = GI.moderate(M, N, K, "f16" if dtype == "f8" else dtype, "refuse")
    if dtype == "f8":
        return TG.dev8(a), TG.dev8(w)
    return TG.dev16(a, dtype), TG.dev16(w, dtype)


@pytest.mark.parametrize("epi", ["bf16", "f32", "qkv", "swiglu", "lse"])
def test_tile_2_is_refused_with_every_other_epilogue(epi):
    a, w = _small()
    c = None if epi == "lse" else (TG.sent32(8, 136) if epi == "f32" else TG.sent16(8, 136, "f16"))
    n0 = eng.gemm_narrow_launches()
    with pytest.raises(eng.BlimError, match=r"tile = 2.*epi"):
        eng.gemm(epi, "f16", a, w, 8, 128, 128, c, tile=2)
    assert eng.gemm_narrow_launches() == n0
    if c is not None:
        torch.cuda.synchronize()
        assert (TG.bits32(c) == TG.SENT32).all() if epi == "f32" else (TG.host16(c) == TG.SENT16).all()


def test_tile_2_is_refused_with_the_e2m3_pass_with_f8_and_beyond_its_range():
    a, w = _small()
    c = TG.sent32(8, 132)
    a6, w6 = TG.f6_buffers(8, 128, 128)
    n0 = eng.gemm_narrow_launches()
    with pytest.raises(eng.BlimError, match=r"tile = 2.*A6"):
        eng.gemm("resid", "f16", a, w, 8, 128, 128, c, tile=2, A6=a6, W6=w6, K6=128)
    a8, w8 = _small("f8")
    with pytest.raises(eng.BlimError, match=r"tile = 2.*dtype"):
        eng.gemm("resid", "f8", a8, w8, 8, 128, 128, c, tile=2, row_scale=TG.dev32(np.ones(8)), col_scale=TG.dev32(np.ones(128)))
    for tile in (3, -1):
        with pytest.raises(eng.BlimError, match=r"tile = "):
            eng.gemm("resid", "f16", a, w, 8, 128, 128, c, tile=tile)
    torch.cuda.synchronize()
    assert eng.gemm_narrow_launches() == n0 and (TG.bits32(c) == TG.SENT32).all()


# ---------------------------------------------------------------------------- tile = 1: both sides of the auto rule, the threshold read from the library
def test_auto_rule_both_sides():
    T = eng.gemm_narrow_threshold()                                                     # narrow when ceil(M / 256) * ceil(N / 256) < T
    assert 0 <= T <= 512
    K, dtype = 64, "f16"

    def call(M, N, tile):
        a, w = GI.moderate(M, N, K, dtype, "auto")
        c = torch.zeros((M, N + 4), dtype=torch.float32, device="cuda")
        eng.gemm("resid", dtype, TG.dev16(a, dtype), TG.dev16(w, dtype), M, N, K, c, tile=tile)
        torch.cuda.synchronize()
        return c

    n0 = eng.gemm_narrow_launches()
    got = call(65, 136, 1)                                                              # one tile of 256 x 256
    assert eng.gemm_narrow_launches() == n0 + (1 if T > 1 else 0)
    assert torch.equal(got, call(65, 136, 0))
    n0 = eng.gemm_narrow_launches()
    tiles_n = max(T, 1)                                                                 # exactly T tiles: not below the threshold
    got = call(256, 256 * tiles_n, 1)
    assert eng.gemm_narrow_launches() == n0, "a grid of `threshold` tiles took the narrow kernel"
    if T > 1:                                                                           # ... and T - 1 tiles: the last grid below it
        n0 = eng.gemm_narrow_launches()
        got = call(256, 256 * (T - 1), 1)
        assert eng.gemm_narrow_launches() == n0 + 1
        assert torch.equal(got, call(256, 256 * (T - 1), 0))
    # an ineligible form under tile = 1 silently takes the 256 x 256 kernel
    n0 = eng.gemm_narrow_launches()
    a, w = _small()
    o = TG.sent16(8, 136, "f16")
    eng.gemm("bf16", "f16", a, w, 8, 128, 128, o, tile=1)
    torch.cuda.synchronize()
    assert eng.gemm_narrow_launches() == n0 and (TG.host16(o)[:, :128] != TG.SENT16).all()
