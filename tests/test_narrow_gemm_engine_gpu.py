"""GPU: engine option "narrow_gemm" (blim.h) -- run_layers hands it to its o_proj and down launches, which then run on the narrow-tile residual GEMM
(csrc/gemm.hip: gemm_narrow_kernel) where their form is eligible.  The option changes which kernel computes, never a value: PairScorer.vtg / .tvg scores, the
final-norm hidden states of blim_decode and a lazy gallery's passes are compared BIT FOR BIT with option 0, on the tiny synthetic engine (2 layers, H = 256) and at
the `wide` case's dimensions (7B width, one layer: down has K = 18,944), in fp16 and bf16, plain and compensated.  The host-side counter of narrow launches
(engine.gemm_narrow_launches) shows that the kernel under test ran -- and that it did not where the form is not eligible (fp16 engines' compensated launches carry
the e2m3 second pass)."""
import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_gpu_parity as P
import test_lazy_gallery_gpu as LZ
from blim_amd import engine as eng

pytestmark = pytest.mark.gpu


ALL = ["tiny-f16", "tiny-bf16", "wide-f16", "wide-bf16"]
TINY = ["tiny-f16", "tiny-bf16"]


@pytest.fixture(scope="module")
def models():
    """name -> the case built once per module (tiny: 2 layers, H = 256; wide: 7B width, one layer, device-made weights)."""
    built = {}

    def get(name):
        if name not in built:
            case, dtype = name.split("-")
            built[name] = P._build(case, device_synth=case == "wide", dtype=dtype)
        return built[name]
    yield get
    for t in built.values():
        t.model.engine.close()


def _pairs(t, k=12):
    n = t.spec["n"]
    return np.array([[j, i] for i in range(n) for j in range(n)], np.int64)[:k]


def _with_option(t, value, fn):
    e = t.model.engine
    e.set_option("narrow_gemm", value)
    try:
        t.model.clear_cache()
        n0 = eng.gemm_narrow_launches()
        out = fn()
        torch.cuda.synchronize()
        return out, eng.gemm_narrow_launches() - n0
    finally:
        e.set_option("narrow_gemm", 0)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("name", TINY)
def test_option_values(models, name):
    """The test that fails without the feature: the option does not exist there ("unknown option")."""
    e = models(name).model.engine
    for v in (0, 1, 2, 0):
        e.set_option("narrow_gemm", v)
    for v in (3, -1):
        with pytest.raises(eng.BlimError, match="narrow_gemm"):
            e.set_option("narrow_gemm", v)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("mode", ["none", "full"])
def test_scores_are_bit_equal_and_the_narrow_kernel_ran(models, name, mode):
    """VTG in the plain and the fully compensated mode, TVG in its default (compensated) mode.  bf16 engines' compensated launches are the w_wrap_k form (eligible);
    fp16 engines' carry the e2m3 second pass (option "precise_lo6", their default): not eligible, the counter stays where it was."""
    t = models(name)
    G._set_mode(t, mode)
    try:
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = _pairs(t)
        ref_v, n = _with_option(t, 0, lambda: sc.vtg(pairs))
        assert n == 0 and np.all(np.isfinite(ref_v))
        got_v, n_v = _with_option(t, 2, lambda: sc.vtg(pairs))
        assert np.array_equal(_bits(got_v), _bits(ref_v)), (mode, np.max(np.abs(got_v - ref_v)))
        lo6 = t.dtype == "f16" and t.model.engine.lo6
        if mode == "full" and lo6:
            assert n_v == 0, "a launch with the e2m3 second pass took the narrow kernel"
        else:
            assert n_v >= 2 * t.dims.num_layers, n_v                  # o_proj and down of every layer, in every call of the pass
        ref_t, n = _with_option(t, 0, lambda: sc.tvg(pairs))
        assert n == 0 and np.all(np.isfinite(ref_t))
        got_t, n_t = _with_option(t, 2, lambda: sc.tvg(pairs))
        assert np.array_equal(_bits(got_t), _bits(ref_t)), (mode, np.max(np.abs(got_t - ref_t)))
        if t.model.tvg_mode() == "full":
            assert (n_t == 0) if lo6 else (n_t >= 2 * t.dims.num_layers), n_t
    finally:
        G._set_mode(t, "none")


@pytest.mark.parametrize("name", ALL)
def test_decode_hidden_states_are_bit_equal(models, name):
    t = models(name)
    e = t.model.engine
    L, Hd = 70, t.dims.hidden_size
    batch = eng.PackedBatch(np.arange(L, dtype=np.int32), np.ones(L, np.uint8), np.array([0], np.int32), np.array([L], np.int32))
    g = torch.Generator(device="cpu").manual_seed(5)
    emb = (torch.randn((L, Hd), generator=g) * 0.02).to(e.torch_dtype).cuda()
    rows = torch.tensor([3, L - 1], dtype=torch.int32, device="cuda")
    for out_rows in (None, rows):                                      # every row, and the last layer's pruned rows
        (ref, _), n = _with_option(t, 0, lambda: e.decode(batch, emb, out_rows=out_rows))
        assert n == 0 and torch.isfinite(ref.float()).all()
        for v in (2, 1):
            (got, _), n = _with_option(t, v, lambda: e.decode(batch, emb, out_rows=out_rows))
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (v, out_rows is None)
            if v == 2 or eng.gemm_narrow_threshold() > -(-t.dims.hidden_size // 256):      # 70 rows: one row of 256 x 256 tiles
                assert n == 2 * t.dims.num_layers, (v, n)


@pytest.mark.parametrize("name", TINY)
def test_lazy_gallery_passes_under_auto_equal_pair_scorer(models, name):
    t = models(name)
    G._set_mode(t, "none")
    sc = LZ._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = G._t2v_pairs(t)
    ref, n = _with_option(t, 0, lambda: sc.vtg(pairs))
    assert n == 0
    gal = LZ._lazy(sc)
    try:
        def passes():
            first, d1 = LZ._delta(gal, lambda: gal.vtg_pairs(pairs))                # all misses
            second, d2 = LZ._delta(gal, lambda: gal.vtg_pairs(pairs))               # all hits
            return first, d1, second, d2
        (first, d1, second, d2), n = _with_option(t, 1, passes)
        assert d1["hits"] == 0 and d1["misses"] == d1["admitted"] > 0 and d2["misses"] == 0 and d2["hits"] == d1["misses"]
        assert np.array_equal(_bits(first), _bits(ref)) and np.array_equal(_bits(second), _bits(ref))
        if eng.gemm_narrow_threshold() > 1 and not (t.dtype == "f16" and t.model.vtg_mode() == "full"):
            assert n > 0
    finally:
        gal.close()
