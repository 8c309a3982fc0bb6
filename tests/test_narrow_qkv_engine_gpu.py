"""GPU: engine option "narrow_qkv" (blim.h) -- run_layers hands it to its QKV launch, which then runs on the narrow-tile QKV GEMM (csrc/gemm.hip: gemm_nqkv_kernel) in
whatever 16-bit form the call has: plain, a plain unit over [hi | lo] rows, hi | lo outputs over the w_wrap_k walk (bf16's compensated calls) or behind the e2m3 second
pass (fp16's compensated calls, every TVG call).  Like "narrow_gemm" and "narrow_lo6" the option changes which kernel computes, never a value: PairScorer.vtg / .tvg
scores, blim_decode's hidden states and a lazy gallery's passes -- whose hit pass reads back K / V that the narrow kernel wrote -- are compared BIT FOR BIT with option
0, on the fixtures of test_narrow_gemm_engine_gpu.py (tiny: 2 layers, H = 256; wide: 7B width, one layer).  The kernel's own host counter
(engine.gemm_narrow_qkv_launches) shows that it ran; the two older counters show that their kernels' launches stayed their own."""
import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_lazy_gallery_gpu as LZ
from blim_amd import engine as eng
from test_gallery_gpu import lora  # noqa: F401  (fixture: lora_tiny with the adapters apart, fp16 and bf16)
from test_narrow_gemm_engine_gpu import _bits, _pairs, models  # noqa: F401  (fixture: the tiny and the 7B-width cases, built once per module)

pytestmark = pytest.mark.gpu

F16 = ["tiny-f16", "wide-f16"]
ALL = ["tiny-f16", "tiny-bf16", "wide-f16"]


def _with(t, fn, narrow_qkv=0, narrow_lo6=0, narrow_gemm=0):
    """fn() under the three options -> (its result, launches of the narrow QKV kernel, of the e2m3 narrow kernel, of the plain narrow kernel)."""
    e = t.model.engine
    e.set_option("narrow_qkv", narrow_qkv)
    e.set_option("narrow_lo6", narrow_lo6)
    e.set_option("narrow_gemm", narrow_gemm)
    try:
        t.model.clear_cache()
        q0, n0, p0 = eng.gemm_narrow_qkv_launches(), eng.gemm_narrow_lo6_launches(), eng.gemm_narrow_launches()
        out = fn()
        torch.cuda.synchronize()
        return out, eng.gemm_narrow_qkv_launches() - q0, eng.gemm_narrow_lo6_launches() - n0, eng.gemm_narrow_launches() - p0
    finally:
        e.set_option("narrow_qkv", 0)
        e.set_option("narrow_lo6", 0)
        e.set_option("narrow_gemm", 0)


@pytest.mark.parametrize("name", ["tiny-f16", "tiny-bf16"])
def test_option_values(models, name):
    """The test that fails without the feature: the option does not exist there ("unknown option")."""
    e = models(name).model.engine
    for v in (0, 1, 2, 0):
        e.set_option("narrow_qkv", v)
    for v in (3, -1):
        with pytest.raises(eng.BlimError, match="narrow_qkv"):
            e.set_option("narrow_qkv", v)
    e.set_option("narrow_qkv", 1)                                       # a refused value left the option settable
    e.set_option("narrow_qkv", 0)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("mode", ["none", "full"])
def test_vtg_is_bit_equal_and_the_kernel_ran(models, name, mode):
    """"none": the plain form.  "full": hi | lo outputs behind the e2m3 second pass (fp16) or over the w_wrap_k walk (bf16)."""
    t = models(name)
    G._set_mode(t, mode)
    try:
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = _pairs(t)
        ref, q, n, p = _with(t, lambda: sc.vtg(pairs))
        assert (q, n, p) == (0, 0, 0) and np.all(np.isfinite(ref))
        for v in (2, 1):
            got, q, n, p = _with(t, lambda: sc.vtg(pairs), narrow_qkv=v)
            assert np.array_equal(_bits(got), _bits(ref)), (v, np.max(np.abs(got - ref)))
            assert (n, p) == (0, 0), (v, n, p)                           # the older kernels' launches are not this option's
            if v == 2:
                assert q >= t.dims.num_layers, (v, q)                    # the QKV launch of every layer, in every call of the pass
        # the older options alone never launch the new kernel
        got, q, n, p = _with(t, lambda: sc.vtg(pairs), narrow_gemm=2, narrow_lo6=2)
        assert np.array_equal(_bits(got), _bits(ref)) and q == 0, q
    finally:
        G._set_mode(t, "none")


def test_a_mixed_select_mask(models):
    """Layer 0 compensated in every unit (bits 15), layer 1 in its QKV alone (bits 1): both layers' QKV launches write hi | lo behind the second pass, and layer 1's
    o_proj and down are plain units over [hi | lo] rows; all three narrow kernels run in one call."""
    t = models("tiny-f16")
    G._set_mode(t, "select")
    try:
        assert list(t.model.engine.layer_mask[:2]) == [15, 1]
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = _pairs(t)
        ref, q, n, p = _with(t, lambda: sc.vtg(pairs))
        assert (q, n, p) == (0, 0, 0) and np.all(np.isfinite(ref))
        got, q, n, p = _with(t, lambda: sc.vtg(pairs), narrow_qkv=2)
        assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
        assert q >= 2 and (n, p) == (0, 0), (q, n, p)
        got, q, n, p = _with(t, lambda: sc.vtg(pairs), narrow_qkv=2, narrow_lo6=2, narrow_gemm=2)
        assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
        assert q >= 2 and n >= 2 and p >= 2 and q == n == p, (q, n, p)   # per call: two QKV launches, two compensated and two plain residual launches
    finally:
        G._set_mode(t, "none")


@pytest.mark.parametrize("name", F16)
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_tvg_is_bit_equal_and_the_kernel_ran(models, name, mode):
    """Every TVG call is compensated in QKV: hi | lo outputs behind the e2m3 second pass."""
    t = models(name)
    t.model.tvg_precise = mode
    try:
        sc = G._scorer(t)
        pairs = _pairs(t)
        ref, q, n, p = _with(t, lambda: sc.tvg(pairs))
        assert (q, n, p) == (0, 0, 0) and np.all(np.isfinite(ref))
        got, q, n, p = _with(t, lambda: sc.tvg(pairs), narrow_qkv=2)
        assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
        assert q >= t.dims.num_layers and (n, p) == (0, 0), (mode, q, n, p)
    finally:
        t.model.tvg_precise = "full"


def test_adapters_apart(lora):
    """The QKV launch carries the adapters (its W and W6 are the augmented ones, K extended): VTG full and TVG on the engine with the adapters apart."""
    t = lora
    G._set_mode(t, "full")
    try:
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = G._t2v_pairs(t)
        for fn in (lambda: sc.vtg(pairs), lambda: sc.tvg(pairs)):
            ref, q, n, p = _with(t, fn)
            assert q == 0 and np.all(np.isfinite(ref))
            got, q, n, p = _with(t, fn, narrow_qkv=2)
            assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
            assert q >= t.dims.num_layers and (n, p) == (0, 0), (t.dtype, q, n, p)
    finally:
        G._set_mode(t, "none")


@pytest.mark.parametrize("name", F16)
@pytest.mark.parametrize("precise", [False, True])
def test_decode_hidden_states_are_bit_equal(models, name, precise):
    t = models(name)
    e = t.model.engine
    L, Hd = 70, t.dims.hidden_size
    batch = eng.PackedBatch(np.arange(L, dtype=np.int32), np.ones(L, np.uint8), np.array([0], np.int32), np.array([L], np.int32))
    g = torch.Generator(device="cpu").manual_seed(5)
    emb = (torch.randn((L, Hd), generator=g) * 0.02).to(e.torch_dtype).cuda()
    rows = torch.tensor([3, L - 1], dtype=torch.int32, device="cuda")
    e.set_precise(precise)
    try:
        for out_rows in (None, rows):                                  # every row, and the last layer's pruned rows
            (ref, _), q, n, p = _with(t, lambda: e.decode(batch, emb, out_rows=out_rows))
            assert (q, n, p) == (0, 0, 0) and torch.isfinite(ref.float()).all()
            for v in (2, 1):
                (got, _), q, n, p = _with(t, lambda: e.decode(batch, emb, out_rows=out_rows), narrow_qkv=v)
                assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (v, out_rows is None)
                qkv_n = (t.dims.num_heads + 2 * t.dims.num_kv_heads) * 128
                if v == 2 or eng.gemm_narrow_qkv_threshold() > -(-qkv_n // 256):          # 70 rows: one row of 256 x 256 tiles
                    assert q == t.dims.num_layers and (n, p) == (0, 0), (v, q, n, p)
    finally:
        e.set_precise(False)


@pytest.mark.parametrize("mode", ["none", "full"])
def test_lazy_gallery_passes_equal_pair_scorer(models, mode):
    """The miss pass captures K / V that the narrow QKV kernel wrote; the hit pass scores against them.  All three narrow options on together."""
    t = models("tiny-f16")
    G._set_mode(t, mode)
    try:
        sc = LZ._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = G._t2v_pairs(t)
        ref, q, n, p = _with(t, lambda: sc.vtg(pairs))
        assert (q, n, p) == (0, 0, 0)
        gal = LZ._lazy(sc)
        try:
            def passes():
                first, d1 = LZ._delta(gal, lambda: gal.vtg_pairs(pairs))                # all misses
                second, d2 = LZ._delta(gal, lambda: gal.vtg_pairs(pairs))               # all hits
                return first, d1, second, d2
            (first, d1, second, d2), q, n, p = _with(t, passes, narrow_qkv=2, narrow_lo6=2, narrow_gemm=2)
            assert d1["hits"] == 0 and d1["misses"] == d1["admitted"] > 0 and d2["misses"] == 0 and d2["hits"] == d1["misses"]
            assert np.array_equal(_bits(first), _bits(ref)) and np.array_equal(_bits(second), _bits(ref))
            assert q >= 2 * t.dims.num_layers, q                                        # both passes
            assert (n > 0 and p == 0) if mode == "full" else (n == 0 and p > 0), (mode, n, p)
        finally:
            gal.close()
    finally:
        G._set_mode(t, "none")
