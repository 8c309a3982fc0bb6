"""GPU: engine option "narrow_lo6" (blim.h) -- run_layers hands it to its o_proj and down launches, which then run on the narrow-tile residual GEMM with the e2m3
second pass (csrc/gemm.hip: gemm_narrow_lo6_kernel) where they carry that pass: the compensated launches of fp16 engines, and of bf16 engines under
`second_pass = "e2m3"`.  Like "narrow_gemm" the option changes which kernel computes, never a value: PairScorer.vtg / .tvg scores, blim_decode's hidden states and a
lazy gallery's passes are compared BIT FOR BIT with option 0, on the fixtures of test_narrow_gemm_engine_gpu.py (tiny: 2 layers, H = 256; wide: 7B width, one
layer).  The kernel's own host counter (engine.gemm_narrow_lo6_launches) shows that it ran; the plain narrow kernel's counter shows which launches stayed its own."""
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


def _with(t, fn, narrow_lo6=0, narrow_gemm=0):
    """fn() under the two options -> (its result, launches of the e2m3 narrow kernel, launches of the plain narrow kernel)."""
    e = t.model.engine
    e.set_option("narrow_lo6", narrow_lo6)
    e.set_option("narrow_gemm", narrow_gemm)
    try:
        t.model.clear_cache()
        n0, p0 = eng.gemm_narrow_lo6_launches(), eng.gemm_narrow_launches()
        out = fn()
        torch.cuda.synchronize()
        return out, eng.gemm_narrow_lo6_launches() - n0, eng.gemm_narrow_launches() - p0
    finally:
        e.set_option("narrow_lo6", 0)
        e.set_option("narrow_gemm", 0)


@pytest.mark.parametrize("name", ["tiny-f16", "tiny-bf16"])
def test_option_values(models, name):
    """The test that fails without the feature: the option does not exist there ("unknown option")."""
    e = models(name).model.engine
    for v in (0, 1, 2, 0):
        e.set_option("narrow_lo6", v)
    for v in (3, -1):
        with pytest.raises(eng.BlimError, match="narrow_lo6"):
            e.set_option("narrow_lo6", v)
    e.set_option("narrow_lo6", 1)                                       # a refused value left the option settable
    e.set_option("narrow_lo6", 0)


@pytest.mark.parametrize("name", F16)
def test_vtg_full_is_bit_equal_and_the_kernel_ran(models, name):
    t = models(name)
    assert t.model.engine.lo6
    G._set_mode(t, "full")
    try:
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = _pairs(t)
        ref, n, p = _with(t, lambda: sc.vtg(pairs))
        assert n == 0 and p == 0 and np.all(np.isfinite(ref))
        got, n, p = _with(t, lambda: sc.vtg(pairs), narrow_lo6=2)
        assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
        assert n >= 2 * t.dims.num_layers and p == 0, (n, p)              # o_proj and down of every layer, in every call of the pass
        # "narrow_gemm" alone keeps its meaning: a launch with the second pass takes no narrow kernel of either kind
        got, n, p = _with(t, lambda: sc.vtg(pairs), narrow_gemm=2)
        assert np.array_equal(_bits(got), _bits(ref)) and n == 0 and p == 0, (n, p)
    finally:
        G._set_mode(t, "none")


def test_a_mixed_select_mask_moves_both_counters(models):
    """Layer 0 compensated in every unit (bits 15), layer 1 in its QKV alone (bits 1): layer 0's o_proj and down carry the second pass and take the new kernel,
    layer 1's are plain units over [hi | lo] rows and take the old one."""
    t = models("tiny-f16")
    G._set_mode(t, "select")
    try:
        assert list(t.model.engine.layer_mask[:2]) == [15, 1]
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = _pairs(t)
        ref, n, p = _with(t, lambda: sc.vtg(pairs))
        assert n == 0 and p == 0 and np.all(np.isfinite(ref))
        got, n, p = _with(t, lambda: sc.vtg(pairs), narrow_lo6=2, narrow_gemm=2)
        assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
        assert n >= 2 and p >= 2 and n == p, (n, p)                       # one compensated and one plain layer, two launches each per call
    finally:
        G._set_mode(t, "none")


@pytest.mark.parametrize("name", F16)
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_tvg_is_bit_equal_and_the_kernel_ran(models, name, mode):
    """TVG "attn": o_proj alone is compensated (down is a plain unit: the old kernel's under "narrow_gemm"); "full": both."""
    t = models(name)
    t.model.tvg_precise = mode
    try:
        sc = G._scorer(t)
        pairs = _pairs(t)
        ref, n, p = _with(t, lambda: sc.tvg(pairs))
        assert n == 0 and p == 0 and np.all(np.isfinite(ref))
        got, n, p = _with(t, lambda: sc.tvg(pairs), narrow_lo6=2)
        assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
        assert n >= (2 if mode == "full" else 1) * t.dims.num_layers and p == 0, (mode, n, p)
    finally:
        t.model.tvg_precise = "full"


def test_adapters_apart(lora):
    """o_proj carries an adapter (its W and W6 are the augmented ones): VTG full and TVG on the engine with the adapters apart."""
    t = lora
    lo6 = bool(t.model.engine.lo6)
    G._set_mode(t, "full")
    try:
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = G._t2v_pairs(t)
        for fn in (lambda: sc.vtg(pairs), lambda: sc.tvg(pairs)):
            ref, n, p = _with(t, fn)
            assert n == 0 and np.all(np.isfinite(ref))
            got, n, p = _with(t, fn, narrow_lo6=2)
            assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
            assert (n >= 2 * t.dims.num_layers) if lo6 else (n == 0), (t.dtype, n)
    finally:
        G._set_mode(t, "none")


@pytest.mark.parametrize("name", F16)
def test_decode_hidden_states_are_bit_equal(models, name):
    t = models(name)
    e = t.model.engine
    L, Hd = 70, t.dims.hidden_size
    batch = eng.PackedBatch(np.arange(L, dtype=np.int32), np.ones(L, np.uint8), np.array([0], np.int32), np.array([L], np.int32))
    g = torch.Generator(device="cpu").manual_seed(5)
    emb = (torch.randn((L, Hd), generator=g) * 0.02).to(e.torch_dtype).cuda()
    rows = torch.tensor([3, L - 1], dtype=torch.int32, device="cuda")
    e.set_precise(True)
    try:
        for out_rows in (None, rows):                                  # every row, and the last layer's pruned rows
            (ref, _), n, p = _with(t, lambda: e.decode(batch, emb, out_rows=out_rows))
            assert n == 0 and p == 0 and torch.isfinite(ref.float()).all()
            for v in (2, 1):
                (got, _), n, p = _with(t, lambda: e.decode(batch, emb, out_rows=out_rows), narrow_lo6=v)
                assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (v, out_rows is None)
                if v == 2 or eng.gemm_narrow_lo6_threshold() > -(-t.dims.hidden_size // 256):      # 70 rows: one row of 256 x 256 tiles
                    assert n == 2 * t.dims.num_layers and p == 0, (v, n, p)
    finally:
        e.set_precise(False)


def test_bf16_engine_under_the_e2m3_second_pass(models):
    t = models("tiny-bf16")
    G._set_mode(t, "full")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = _pairs(t)
    try:
        # its default second pass (a second walk in bf16: the w_wrap_k form, "narrow_gemm"'s): the new kernel never runs
        assert not t.model.engine.lo6
        ref, n, p = _with(t, lambda: sc.vtg(pairs))
        got, n, p = _with(t, lambda: sc.vtg(pairs), narrow_lo6=2)
        assert np.array_equal(_bits(got), _bits(ref)) and n == 0 and p == 0, (n, p)
        # ... and the opt-in e2m3 pass
        t.model.second_pass = "e2m3"
        assert t.model.engine.lo6
        ref, n, p = _with(t, lambda: sc.vtg(pairs))
        assert n == 0 and np.all(np.isfinite(ref))
        got, n, p = _with(t, lambda: sc.vtg(pairs), narrow_lo6=2)
        assert np.array_equal(_bits(got), _bits(ref)), np.max(np.abs(got - ref))
        assert n >= 2 * t.dims.num_layers and p == 0, (n, p)
    finally:
        t.model.second_pass = "16bit"
        G._set_mode(t, "none")


def test_lazy_gallery_passes_under_auto_equal_pair_scorer(models):
    t = models("tiny-f16")
    G._set_mode(t, "full")
    try:
        sc = LZ._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = G._t2v_pairs(t)
        ref, n, p = _with(t, lambda: sc.vtg(pairs))
        assert n == 0
        gal = LZ._lazy(sc)
        try:
            def passes():
                first, d1 = LZ._delta(gal, lambda: gal.vtg_pairs(pairs))                # all misses
                second, d2 = LZ._delta(gal, lambda: gal.vtg_pairs(pairs))               # all hits
                return first, d1, second, d2
            (first, d1, second, d2), n, p = _with(t, passes, narrow_lo6=1)
            assert d1["hits"] == 0 and d1["misses"] == d1["admitted"] > 0 and d2["misses"] == 0 and d2["hits"] == d1["misses"]
            assert np.array_equal(_bits(first), _bits(ref)) and np.array_equal(_bits(second), _bits(ref))
            if eng.gemm_narrow_lo6_threshold() > 1:
                assert n > 0 and p == 0, (n, p)
        finally:
            gal.close()
    finally:
        G._set_mode(t, "none")
