"""GPU: the shortlist -- PairScorer.tvg_gallery against PairScorer.tvg, its independence of how texts are grouped into calls,
GalleryIndex.shortlist / search_requests against rerank_requests over the shortlist's candidates, mixed batches over an eager and a lazy index, the v2t form over the
caption cache, and the command.  Every comparison is bit for bit, except where the whole-gallery planner and _plan_tvg cut a text's merged sequences at different
places: there section 11's rule holds, |got - want| <= 1e-5 x max(1, |want|) (tests/test_text_gallery_gpu.py: _close).  The host side is
tests/test_shortlist_host.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gallery_gpu as G
import test_lazy_gallery_gpu as LG
import test_text_gallery_gpu as TG
from blim_amd import synth
from blim_amd.gallery import GalleryIndex, TextGalleryIndex
from test_gallery_gpu import lora, tiny  # noqa: F401  (fixtures: the tiny case and its fine-tuned twin, 6 videos and 2 layers, in fp16 and bf16)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_BLEND = (0.6, 0.5, 0.7, 0.5)
ALPHA = (0.8, 0.3)


def _scorer(t, mode, max_tokens=4096):
    G._set_mode(t, "none")
    sc = G._scorer(t, max_tokens)
    sc.set_vtg_mode(t.model.vtg_mode())
    TG._set_tvg(t, sc, mode)
    return sc


def _counted(sc):
    """-> the list the scorer's engine calls are appended to."""
    calls, run = [], sc.run

    def counted(plan, cache=None):
        calls.append(plan)
        return run(plan, cache)
    sc.run = counted
    return calls


# ---- rules 1 and 2: the planner
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_tvg_gallery_equals_tvg_and_does_not_depend_on_the_grouping(lora, mode):
    _planner_rules(lora, mode)


def test_tvg_gallery_on_the_base_weights(tiny):
    _planner_rules(tiny, "full")


def _planner_rules(t, mode):
    n = t.spec["n"]
    sc = _scorer(t, mode)
    try:
        C = sc.num_clips
        assert sc.gallery_chunk() >= n
        # rule 1: one chunk, the text alone in its call -> the same call as PairScorer.tvg, bit for bit
        for i in (0, n - 1):
            want = sc.tvg(np.array([[j, i] for j in range(n)]))
            got = sc.tvg_gallery([i])
            assert got.shape == (1, n) and np.all(np.isfinite(want)) and np.array_equal(got[0], want), (i, float(np.max(np.abs(got[0] - want))))
        # ... chunks of 4 over 6 videos: the two planners cut differently -> section 11's rule
        texts = list(range(n))
        want = sc.tvg(np.array([[j, i] for i in texts for j in range(n)])).reshape(n, n)
        calls = _counted(sc)
        together = sc.tvg_gallery(texts, chunk=4)
        assert len(calls) == 1 and np.all(np.isfinite(together)) and TG._close(together, want), float(np.max(np.abs(together - want)))
        # rule 2: alone, reversed, and with call boundaries between the two chunks of a text -> bit-equal
        for i in texts:
            assert np.array_equal(sc.tvg_gallery([i], chunk=4)[0], together[i]), i
        assert np.array_equal(sc.tvg_gallery(texts[::-1], chunk=4), together[::-1])
        assert np.array_equal(sc.tvg_gallery([2, 0, 2], chunk=4), together[[2, 0, 2]])
        longest = max(len(sc.tvg_split[i]) for i in texts)
        sc.max_tokens = longest + 4 * (C - 1)                                    # the longest prompt and one chunk: that text's second chunk starts a new call
        del calls[:]
        split = sc.tvg_gallery(texts, chunk=4)
        at = texts.index(max(texts, key=lambda i: len(sc.tvg_split[i])))
        assert 2 <= len(calls) <= 2 * n and all(p.n_tokens <= sc.max_tokens for p in calls)      # several calls ...
        outs = [set((p.out_index[:, 0] // n).tolist()) for p in calls]
        assert sum(1 for o in outs if at in o) == 2                              # ... and a boundary between the two chunks of the longest text
        assert np.array_equal(split, together), float(np.max(np.abs(split - together)))
        sc.max_tokens = longest + 4 * (C - 1) - 1
        with pytest.raises(ValueError, match="max_tokens"):
            sc.tvg_gallery(texts, chunk=4)
    finally:
        sc.max_tokens = 4096
        TG._set_tvg(t, sc, "full")


# ---- rules 3, 4, 5: the index
def _check_against_rerank_requests(gal, sc, texts, K, cpn, bit_equal_tvg, chunk_note=""):
    """search_requests with shortlist K against rerank_requests over shortlist()'s candidates: the VTG term bit-equal always, the TVG term stage 1's value."""
    n = len(sc.video)
    more = dict(cpn=cpn, alpha=ALPHA, finetuned=True)
    cand, stage = gal.shortlist(texts, K, **{k: more[k] for k in ("cpn", "alpha")})
    assert cand.shape == stage.shape == (len(texts), min(K, n))
    # rule 3: the stable descending order of tvg_gallery (minus alpha[0] x the prior with cpn)
    full = sc.tvg_gallery(texts)
    if cpn:
        full = full - ALPHA[0] * gal._t2v_prior(texts, np.tile(np.arange(n), (len(texts), 1)))
    for q in range(len(texts)):
        o = np.argsort(-full[q], kind="stable")[:K]
        assert np.array_equal(cand[q], o) and np.array_equal(stage[q], full[q][o]) and np.all(np.isfinite(stage[q]))
    # the VTG term alone (c0 = 1): bit-equal, order included
    vtg_only = dict(more, c=(1.0, 0.0, 1.0, 0.0))
    got = gal.search_requests([(i, None, None, K) for i in texts], **vtg_only)
    want = gal.rerank_requests([(i, cand[q], None) for q, i in enumerate(texts)], **vtg_only)
    for (o1, b1), (o2, b2) in zip(got, want):
        assert np.array_equal(o1, o2) and np.array_equal(b1, b2)
    # the blend: the TVG term is stage 1's value
    blend = dict(more, c=C_BLEND)
    got = gal.search_requests([(i, None, None, K) for i in texts], **blend)
    want = gal.rerank_requests([(i, cand[q], None) for q, i in enumerate(texts)], **blend)
    for q, ((order, blended), (o2, b2)) in enumerate(zip(got, want)):
        ql = sc.vtg(np.stack([cand[q], np.full(len(cand[q]), texts[q])], axis=1))
        mine = C_BLEND[2] * (C_BLEND[0] * ql + (1 - C_BLEND[0]) * stage[q]) + (1 - C_BLEND[2]) * np.zeros(len(ql))
        o = np.argsort(-mine, kind="stable")
        assert np.array_equal(order, cand[q][o]) and np.array_equal(blended, mine[o])                   # exactly the blend of (VTG, stage 1, zero first stage)
        ref = dict(zip(o2.tolist(), b2.tolist()))
        assert sorted(order.tolist()) == sorted(o2.tolist())
        for j, v in zip(order.tolist(), blended.tolist()):
            assert abs(v - ref[j]) <= 1e-5 * max(1.0, abs(ref[j])), (q, j, v, ref[j])
        if bit_equal_tvg:
            assert np.array_equal(order, o2) and np.array_equal(blended, b2), q


@pytest.mark.parametrize("cpn", [False, True])
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_shortlist_and_search_requests_against_rerank_requests(lora, mode, cpn):
    t = lora
    n = t.spec["n"]
    sc = _scorer(t, mode)
    gal = GalleryIndex(sc).build()
    try:
        # one text per call and K = N: stage 1 and rerank_requests' TVG call are the same call (N fits one chunk) -> bit-equal throughout (rules 4 and 5)
        for i in (1, 4):
            _check_against_rerank_requests(gal, sc, [i], n, cpn, bit_equal_tvg=True)
            _check_against_rerank_requests(gal, sc, [i], n + 3, cpn, bit_equal_tvg=True)               # K clipped to N: candidates = the whole gallery
            order, blended = gal.search_requests([(i, None, None, n + 3)], cpn=cpn, alpha=ALPHA, c=C_BLEND, finetuned=True)[0]
            o2, b2 = gal.rerank_requests([(i, np.arange(n), None)], cpn=cpn, alpha=ALPHA, c=C_BLEND, finetuned=True)[0]
            assert np.array_equal(order, o2) and np.array_equal(blended, b2)                            # rule 5
        # several texts, K < N: rerank_requests scores K of the N videos per text, in other merged sequences -> section 11's rule on the TVG term
        _check_against_rerank_requests(gal, sc, [0, 3, 5], 3, cpn, bit_equal_tvg=False)
        _check_against_rerank_requests(gal, sc, [2], 1, cpn, bit_equal_tvg=False)
        with pytest.raises(ValueError, match="finetuned=False"):
            gal.search_requests([(0, None, None, 2)], finetuned=False)
    finally:
        gal.close(); TG._set_tvg(t, sc, "full")


# ---- rule 6: mixed batches, eager and lazy
@pytest.mark.parametrize("fill", ["eager", "lazy"])
def test_mixed_batches_behave_like_separate_calls(lora, fill):
    t = lora
    n = t.spec["n"]
    sc = _scorer(t, "full")
    gal = GalleryIndex(sc).build() if fill == "eager" else LG._lazy(sc, capacity=n // 2)      # fewer slots than videos
    try:
        rng = np.random.RandomState(11)
        iv2 = t.prob.t2v_sims.astype(np.float32)
        c5 = rng.permutation(n)[:4]
        batch = [(0, None, None, 3), (5, c5, iv2[5][c5], None), (2, None, None, n), (1, np.array([4, 1]), None, None), (3, None, None, 1), (4, np.array([2]), None, None)]
        explicit = [r[:3] for r in batch if r[3] is None]
        for more in (dict(cpn=True, alpha=ALPHA, c=C_BLEND, finetuned=True), dict(cpn=False, alpha=ALPHA, c=(1.0, 0.0, 1.0, 0.0), finetuned=True)):
            before = dict(gal.shortlist_stats)
            passes = gal._n_pass
            got = gal.search_requests(batch, **more)
            assert gal.shortlist_stats["passes"] == before["passes"] + 1 and gal.shortlist_stats["pairs"] == before["pairs"] + 3 * n      # ONE stage-1 pass
            assert gal._n_pass == passes + 1                                                                                           # ... and ONE VTG pass
            alone = [gal.search_requests([r], **more)[0] for r in batch]
            for r, (o1, b1), (o2, b2) in zip(batch, got, alone):
                # the shortlisted: stage 1 does not depend on the grouping and the VTG term never does; the explicit: their TVG call holds other texts when
                # batched (section 11's rule), unless that term has no weight
                if r[3] is not None or more["c"][0] == 1:
                    assert np.array_equal(o1, o2) and np.array_equal(b1, b2), r[0]
                else:
                    ref = dict(zip(o2.tolist(), b2.tolist()))
                    assert sorted(o1.tolist()) == sorted(o2.tolist()) and all(abs(v - ref[j]) <= 1e-5 * max(1.0, abs(ref[j])) for j, v in zip(o1.tolist(), b1.tolist()))
            want = gal.rerank_requests(explicit, **more)                            # the explicit requests: rerank_requests of them, exactly
            for (o1, b1), (o2, b2) in zip([g for g, r in zip(got, batch) if r[3] is None], want):
                assert np.array_equal(o1, o2) and np.array_equal(b1, b2)
            for (i, _, _, K), (order, blended) in zip(batch, got):
                assert np.all(np.isfinite(blended)) and np.all(np.diff(blended) <= 0) and (K is None or len(order) == min(K, n))
    finally:
        gal.close(); TG._set_tvg(t, sc, "full")


# ---- rule 7: v2t over the caption cache
@pytest.mark.parametrize("cpn", [False, True])
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_text_gallery_shortlist_and_its_rerank(lora, mode, cpn):
    t = lora
    n = t.spec["n"]
    sc = _scorer(t, mode)
    gal = GalleryIndex(sc).build()
    tg = TextGalleryIndex(sc, video_index=gal).build()
    try:
        for v in (0, n - 1):
            row = tg.tvg_pairs(np.stack([np.full(n, v), np.arange(n)], axis=1))
            assert np.all(np.isfinite(row))
            for K in (3, n + 2):
                cand, stage = tg.shortlist([v], K)
                o = np.argsort(-row, kind="stable")[:K]
                assert np.array_equal(cand[0], o) and np.array_equal(stage[0], row[o])
                order, blended = tg.rerank_shortlist([v], K, cpn=cpn, alpha=ALPHA, c=C_BLEND)
                o2, b2 = tg.rerank([v], cand, cpn=cpn, alpha=ALPHA, c=C_BLEND, finetuned=True)
                assert np.array_equal(order, o2) and np.array_equal(blended, b2) and blended.dtype == b2.dtype
        cand, stage = tg.shortlist([1, 4], 2)                                       # several query videos: one pass each
        for q, v in enumerate((1, 4)):
            c1, s1 = tg.shortlist([v], 2)
            assert np.array_equal(cand[q], c1[0]) and np.array_equal(stage[q], s1[0])
    finally:
        tg.close(); gal.close(); TG._set_tvg(t, sc, "full")


# ---- the command
def test_search_command_with_tvg_candidates_and_a_served_shortlist(tmp_path):
    base = [sys.executable, "-m", "blim_amd.search", "--synthetic", "24", "--topk", "5", "--vtg_precise", "none", "--resume", "x", "--cpn", "--alpha", "0.8", "0.3",
            "--c", "0.5", "0.5", "1", "0.5"]
    r = subprocess.run(base + ["--candidates", "tvg", "--query_ids", "0", "7", "--shortlist", "8"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = [json.loads(x) for x in r.stdout.splitlines()]
    assert [x["query"] for x in plain] == ["caption:0", "caption:7"]
    for x in plain:
        assert x["shortlisted"] == 8 and len(x["videos"]) == 5 and len(set(x["videos"])) == 5 and np.all(np.isfinite(x["scores"]))
        assert x["scores"] == sorted(x["scores"], reverse=True)
    assert json.loads(r.stderr.split("shortlist: ")[1].splitlines()[0]) == {"queries": 2, "stage1_passes": 2, "stage1_pairs": 48}
    # served: the same queries with the field, under --candidates all, in one batch with an explicit request and a bad one
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)
    prob = synth.make_problem(1, 24, dims, tok_per_clip=8, fast_video=False)        # the dry run's problem (blim_amd/search.py: --synthetic 24)
    cut = lambda a, m: [int(x) for x in np.asarray(a)[np.asarray(m) != 0]]
    rows7 = {"vtg_ids": cut(prob.vtg_ids[7], prob.vtg_masks[7]), "vtg_labels": cut(prob.vtg_labels[7], prob.vtg_masks[7]),
             "tvg_ids": cut(prob.tvg_ids[7], prob.tvg_masks[7]), "tvg_labels": cut(prob.tvg_labels[7], prob.tvg_masks[7])}
    lines = [json.dumps({"id": 0, "caption": 0, "shortlist": 8, "topk": 5}),
             json.dumps({"id": 1, "caption": 3, "candidate_idx": [2, 9, 4]}),
             json.dumps({"id": 2, "caption": 0, "shortlist": 0}),
             json.dumps({"id": 3, "rows": rows7, "shortlist": 8, "topk": 5})]
    src = tmp_path / "requests.jsonl"
    src.write_text("\n".join(lines) + "\n")
    outs = {}
    for B in (1, 4):
        with open(src) as stdin:
            s = subprocess.run(base + ["--candidates", "all", "--serve", "--batch_queries", str(B), "--batch_wait_ms", "50"], cwd=ROOT, stdin=stdin,
                               capture_output=True, text=True, timeout=300)
        assert s.returncode == 0, s.stderr[-2000:]
        outs[B] = [json.loads(x) for x in s.stdout.splitlines()]
        line = json.loads(s.stderr.split("shortlist: ")[1].splitlines()[0])
        assert line["queries"] == 2 and line["stage1_pairs"] == 48 and (line["stage1_passes"] == 2 if B == 1 else line["stage1_passes"] <= 2)
    out = outs[1]
    assert [x["id"] for x in out] == [0, 1, 2, 3] and "positive integer" in out[2]["error"] and sorted(out[1]["videos"]) == ["2", "4", "9"]
    strip = lambda x: {k: v for k, v in x.items() if k != "id"}
    assert strip(out[0]) == plain[0]                                                # a served shortlist is the command's
    assert out[3]["videos"] == plain[1]["videos"] and out[3]["scores"] == plain[1]["scores"] and out[3]["shortlisted"] == 8      # caption 7 sent as rows
    # batched: nothing moves (stage 1 and the VTG term do not depend on the grouping; the one explicit request's TVG call holds its own pairs either way)
    assert outs[4] == out
