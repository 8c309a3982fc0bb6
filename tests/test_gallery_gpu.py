"""GPU: the gallery index (blim_amd/gallery.py) -- t2v VTG scores with the video prefixes read from the engine's prefix cache (blim.h: blim_prefix_cache_*,
blim_score_vtg_cached) are bit for bit those of PairScorer.vtg on the same pairs; stale slots are refused and refilled; rerank agrees with combine_and_rank's
t2v blend.  The host-side planning is tests/test_gallery_host.py."""
import os
import types

import numpy as np
import pytest
import torch

import lora_fixture as LF
import test_gpu_parity as P
from blim_amd import checkpoint as CK
from blim_amd import engine as eng
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd import training_utils as TU
from blim_amd.gallery import GalleryIndex
from blim_amd.modeling import BlimModel, DDPLike

pytestmark = pytest.mark.gpu


def _scorer(t, max_tokens=4096):
    prob = t.prob
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    return RU.PairScorer(DDPLike(t.model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video],
                         torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels), t.dims.num_clips, max_tokens=max_tokens)


def _t2v_pairs(t, queries=None, topk=None):
    q = queries or t.spec.get("queries", t.spec["n"])
    return RU._topk_pairs(torch.from_numpy(t.prob.t2v_sims)[:q], 0, topk or t.spec["topk"], False)


def _set_mode(t, mode):
    m = t.model
    if mode == "select":                  # a mixed mask: every form of the attention (plain, split, and the two mixed ones) is reached
        bits = np.array([[15, 1, 2, 0, 3, 14, 9, 6][li % 8] for li in range(t.dims.num_layers)], dtype=np.uint8)
        m.vtg_precise = "select"
        m.resolve_vtg("select", bits)
    else:
        m.vtg_precise = mode
    m.clear_cache()


def _same(t, mode, budget_slots=None, max_tokens=4096):
    _set_mode(t, mode)
    sc = _scorer(t, max_tokens)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = _t2v_pairs(t)
    ref = sc.vtg(pairs)
    gal = GalleryIndex(sc)
    if budget_slots is not None:
        gal.budget_bytes = budget_slots * sc.engine.prefix_cache_bytes(1, -(-gal.max_len() // 32) * 32, sc.vtg_mode in ("full", "select"))
    gal.build()
    got = gal.vtg_pairs(pairs)
    gal.close()
    return pairs, ref, got


@pytest.fixture(scope="module", params=["f16", "bf16"])
def tiny(request):
    t = P._build("tiny", dtype=request.param)
    yield t
    t.model.engine.close()


@pytest.mark.parametrize("mode", ["none", "full", "select"])
def test_cached_scores_are_bit_equal_to_pair_scorer(tiny, mode):
    pairs, ref, got = _same(tiny, mode)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(got, ref), (mode, np.max(np.abs(got - ref)))
    if mode == "full" or tiny.dtype == "f16":        # tied to the reference: the golden t2v VTG matrix of the tiny case
        g = np.load(os.path.join(P.GOLD, "tiny.npz"))["S_t2v_vtg"]
        S = np.full(g.shape, -100.0, np.float32)
        S[pairs[:, 1], pairs[:, 0]] = got
        m = g != -100
        assert np.array_equal(m, S != -100)
        assert np.max(np.abs(S[m] - g[m]) / np.abs(g[m])) <= 1e-3


@pytest.mark.parametrize("mode", ["none", "full"])
def test_gallery_over_budget_mixes_cached_and_in_batch_prefixes(tiny, mode):
    pairs, ref, got = _same(tiny, mode, budget_slots=tiny.spec["n"] // 2)
    assert np.array_equal(got, ref)
    pairs, ref, got = _same(tiny, mode, budget_slots=0)           # no slot at all: the in-batch path of the same call
    assert np.array_equal(got, ref)


def test_stale_slots_are_refused_and_refilled(tiny):
    t = tiny
    _set_mode(t, "none")
    sc = _scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = _t2v_pairs(t)
    gal = GalleryIndex(sc).build()
    assert np.array_equal(gal.vtg_pairs(pairs), sc.vtg(pairs))
    plans = list(gal.iter_plans(pairs))
    # a weight change: the C call refuses the slots, the index refills them once
    w2 = dict(t.w)
    w2["final_norm"] = t.w["final_norm"] * 1.01
    t.model.engine.load_weight("final_norm", w2["final_norm"])
    with pytest.raises(eng.BlimError, match="stale"):
        gal.run(plans[0])
    got = gal.vtg_pairs(pairs)
    assert np.array_equal(got, sc.vtg(pairs))
    # a mode change: refilled under the new mode (compensated slots)
    _set_mode(t, "full")
    got = gal.vtg_pairs(pairs)
    assert gal.cache.compensated
    sc.set_vtg_mode("full")
    assert np.array_equal(got, sc.vtg(pairs))
    # an option the slots recorded: refused by the engine itself
    plans = list(gal.iter_plans(pairs))
    t.model.engine.set_option("masked_query_zero", 1)
    try:
        with pytest.raises(eng.BlimError, match="masked_query_zero"):
            gal.run(plans[0])
    finally:
        t.model.engine.set_option("masked_query_zero", 0)
    t.model.engine.load_weight("final_norm", t.w["final_norm"])
    _set_mode(t, "none")
    gal.close()


def _combine_t2v(monkeypatch, ql, cand_l, prior, iv2, cpn, alpha, c, finetuned):
    """The blended t2v matrix training_utils.combine_and_rank builds from evaluation()'s matrices: captured where it hands it to get_recall for "blim"."""
    n = iv2.shape[0]
    seen = []
    monkeypatch.setattr(TU, "get_recall", lambda t2v, v2t, a, b: seen.append(np.array(t2v)) or {})
    t2v = {"internvideo2": iv2, "candidate_likelihood": cand_l, "query_likelihood": ql, "candidate_prior": prior}
    v2t = {k: np.zeros((n, n), np.float32) for k in t2v}
    args = types.SimpleNamespace(resume="finetuned.pth" if finetuned else "", eval=True, cpn=cpn, alpha=list(alpha), c=list(c))
    TU.combine_and_rank(t2v, v2t, args, n)
    monkeypatch.undo()
    return seen[-1]


def _rerank_case(t):
    n, k = t.spec["n"], t.spec["topk"]
    q = t.spec.get("queries", n)
    iv2 = t.prob.t2v_sims.astype(np.float32)
    cand = np.argsort(-iv2[:q], axis=1, kind="stable")[:, :k]
    texts = np.arange(q)
    pairs = np.stack([cand.reshape(-1), np.repeat(texts, k)], axis=1)
    return n, q, iv2, cand, texts, pairs


def _matrix(n, pairs, vals):
    M = np.full((n, n), -100.0, np.float32)
    M[pairs[:, 1], pairs[:, 0]] = vals
    return M


def test_rerank_zero_shot_matches_combine_and_rank_row(tiny, monkeypatch):
    t = tiny
    _set_mode(t, "none")
    sc = _scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    n, q, iv2, cand, texts, pairs = _rerank_case(t)
    ql = _matrix(n, pairs, sc.vtg(pairs))
    c = (0.6, 0.5, 0.7, 0.5)
    full = _combine_t2v(monkeypatch, ql, np.zeros((n, n), np.float32), None, iv2, False, (0.0, 0.0), c, False)
    gal = GalleryIndex(sc).build()
    order, blended = gal.rerank(texts, cand, first_stage=np.take_along_axis(iv2[:q], cand, 1), c=c)
    for i in range(q):
        want = full[i, cand[i]]
        o = np.argsort(-want, kind="stable")
        assert np.array_equal(order[i], cand[i][o])
        assert np.array_equal(blended[i], want[o])
    gal.close()


# ---- adapters kept apart (tests/golden/lora_tiny.npz: the reference's --eval --resume flow)
@pytest.fixture(scope="module", params=["f16", "bf16"])
def lora(request):
    spec, g, dims, prob = LF.load_case("lora_tiny")
    w = LF.base_weights_host(spec, dims)
    tr = LF.trainable_of(spec, dims)
    model = BlimModel(dims, max_positions=1024, dtype=request.param)
    model.engine.load_weights(w)
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    t = types.SimpleNamespace(spec=spec, dims=dims, model=model, w=w, tr=tr, prob=prob, dtype=request.param, case="lora_tiny")
    _load_adapters(t, 1.0)
    yield t
    model.engine.close()


def _load_adapters(t, scale):
    E = t.model.engine
    for nm in CK.expected_adapters(t.dims):
        E.load_adapter(nm, t.tr[nm + ":A"], (scale * t.tr[nm + ":B"]).astype(np.float32), LF.R, LF.ALPHA)
    E.load_weight("visual_head", t.tr["visual_head"])
    t.model.clear_cache()


@pytest.mark.parametrize("mode", ["none", "full", "select"])
def test_adapters_apart_bit_equal(lora, mode):
    assert lora.model.engine.num_adapters() == len(CK.expected_adapters(lora.dims))
    pairs, ref, got = _same(lora, mode)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(got, ref), (mode, np.max(np.abs(got - ref)))


def test_adapters_apart_invalidation(lora):
    t = lora
    _set_mode(t, "none")
    sc = _scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = _t2v_pairs(t)
    gal = GalleryIndex(sc).build()
    base = gal.vtg_pairs(pairs)
    assert np.array_equal(base, sc.vtg(pairs))
    try:
        for change in (lambda: _load_adapters(t, 0.5), lambda: t.model.engine.clear_adapters(), lambda: _load_adapters(t, 1.0)):
            plans = list(gal.iter_plans(pairs))
            change()
            with pytest.raises(eng.BlimError, match="stale"):              # blim_load_adapter / blim_clear_adapters make every slot stale
                gal.run(plans[0])
            got = gal.vtg_pairs(pairs)                                     # ... and the index refills
            assert np.array_equal(got, sc.vtg(pairs))
        assert np.array_equal(got, base)
    finally:
        gal.close()


def _finetuned_reference(t, sc, monkeypatch, alpha, c):
    n, q, iv2, cand, texts, pairs = _rerank_case(t)
    ql = _matrix(n, pairs, sc.vtg(pairs))
    cl = _matrix(n, pairs, sc.tvg(pairs))
    pr = _matrix(n, pairs, sc.tvg(pairs, cpn=True))
    return _combine_t2v(monkeypatch, ql, cl, pr, iv2, True, alpha, c, True)


def test_rerank_finetuned_matches_combine_and_rank_row(lora, monkeypatch):
    """Fine-tuned: candidate likelihood and CPN prior from the TVG path.  A TVG score depends at the 1e-6 level on which candidates share its merged sequence,
    so the blend agrees within 1e-5 and the order wherever neighbours are further apart.  An adapter reload in between: no prior of the old weights survives."""
    t = lora
    _set_mode(t, "none")
    sc = _scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    n, q, iv2, cand, texts, pairs = _rerank_case(t)
    alpha, c = (0.8, 0.3), (0.6, 0.5, 0.7, 0.5)
    gal = GalleryIndex(sc).build()
    try:
        for scale in (1.0, 0.5, 1.0):
            _load_adapters(t, scale)
            full = _finetuned_reference(t, sc, monkeypatch, alpha, c)
            order, blended = gal.rerank(texts, cand, first_stage=np.take_along_axis(iv2[:q], cand, 1), cpn=True, alpha=alpha, c=c, finetuned=True)
            for i in range(q):
                want = full[i, cand[i]]
                got = dict(zip(order[i].tolist(), blended[i].tolist()))
                for j, v in zip(cand[i].tolist(), want.tolist()):
                    assert abs(got[j] - v) <= 1e-5 * max(1.0, abs(v)), (scale, i, j, got[j], v)
                srt = np.sort(want)[::-1]
                if np.all(np.diff(-srt) > 1e-5):                          # order pinned only where neighbours are distinguishable
                    assert np.array_equal(order[i], cand[i][np.argsort(-want, kind="stable")])
                assert np.all(np.diff(blended[i]) <= 0)
    finally:
        _load_adapters(t, 1.0)
        gal.close()


# ---- a 64-video gallery at the full 7B dimensions: 28 layers (per-layer slot offsets), 7 query heads per KV head (the head-group split and the mixed
# select forms at G = 7), fills and scoring calls split over several packed calls
@pytest.fixture(scope="module")
def b7():
    dims = synth.ModelDims()
    model = BlimModel(dims, max_positions=1024, dtype="f16")
    model.engine.init_synthetic_weights(3)
    prob = synth.make_problem(4, 64, dims, tok_per_clip=64, text_len=(6, 30))
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    t = types.SimpleNamespace(spec={"n": 64, "topk": 16, "queries": 8}, dims=dims, model=model, w=None, prob=prob, dtype="f16", case="7b64")
    yield t
    model.engine.close()


@pytest.mark.parametrize("mode", ["none", "full", "select"])
def test_7b_gallery_64_videos(b7, mode):
    pairs, ref, got = _same(b7, mode, max_tokens=8192)
    assert len(pairs) == 8 * 16 and np.all(np.isfinite(ref))
    assert np.array_equal(got, ref), (mode, np.max(np.abs(got - ref)))
    pairs, ref, got = _same(b7, mode, budget_slots=40, max_tokens=8192)          # over budget: mixed slots
    assert np.array_equal(got, ref)


def test_fp8_engine_refuses_a_cache():
    t = P._build("tiny", dtype="f8")
    try:
        with pytest.raises(eng.BlimError):
            t.model.engine.prefix_cache(4, 64, False)
    finally:
        t.model.engine.close()


def test_cache_bytes_match_the_python_formula(tiny):
    from blim_amd.gallery import cache_bytes
    for comp in (False, True):
        assert tiny.model.engine.prefix_cache_bytes(7, 96, comp) == cache_bytes(tiny.dims, 7, 96, comp)


def test_search_cli_synthetic(tmp_path):
    import json
    import subprocess
    import sys
    out = tmp_path / "q.jsonl"
    r = subprocess.run([sys.executable, "-m", "blim_amd.search", "--synthetic", "64", "--query_ids", "0", "5", "--topk", "16", "--vtg_precise", "none",
                        "--c", "0.5", "0.5", "0.5", "0.5", "--output", str(out)], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    assert [x["query"] for x in lines] == ["caption:0", "caption:5"]
    for x in lines:
        assert len(x["videos"]) == 16 and all(np.isfinite(x["scores"]))
        assert x["scores"] == sorted(x["scores"], reverse=True)
