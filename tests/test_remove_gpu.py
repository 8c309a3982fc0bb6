"""GPU: videos that leave a scorer at run time (PairScorer.remove_videos, _PrefixIndex._follow_removed, HostTier.forget, `python -m
blim_amd.search`: remove_video).  The reference of every test is a scorer -- and fresh indexes over it -- built from only the remaining videos, in the same order
(`fresh`); the scorer under test (`whole`) is built with all six and loses {1, 4}, so video KEEP[p] of `whole` is video p of `fresh`.  A projected row, a GEMM row
and an attention block do not depend on what else is in the scorer, the vocabulary registered again is the same split of the same float32 rows, and the whole-gallery
planner cuts its chunks over the live videos, so every comparison is np.array_equal: VTG scores, TVG scores with one video per text per call, tvg_gallery, tvg_first
(with and without a set), both priors and both blends, through eager, lazy and host-tier indexes.  Before the removal `whole`'s TVG scores differ from `fresh`'s --
the normaliser runs over 6 instead of 4 videos -- which is what makes the comparisons after it mean something.  The host side is tests/test_remove_host.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_grow_gpu as GW
import test_lazy_gallery_gpu as LG
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd.gallery import GalleryIndex, SearchRequest, TextGalleryIndex
from blim_amd.modeling import BlimModel
from test_gallery_gpu import lora, tiny  # noqa: F401  (fixtures: the tiny case and its fine-tuned twin, 6 videos and 2 layers, in fp16 and bf16)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_BLEND, ALPHA = GW.C_BLEND, GW.ALPHA
GONE, KEEP = [1, 4], np.array([0, 2, 3, 5])
_count_priors, _tiered = GW._count_priors, GW._tiered


def _scorer(t, videos, max_tokens=4096):
    """Every text of the problem over the videos `videos` of it, in that order, each with its own vocabulary row."""
    prob = t.prob
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    videos = list(videos)
    sc = RU.PairScorer(G.DDPLike(t.model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(prob.video[j]) for j in videos],
                       torch.from_numpy(prob.video_vocab[videos]), torch.arange(len(videos)), t.dims.num_clips, max_tokens=max_tokens)
    sc.set_vtg_mode(t.model.vtg_mode())
    return sc


def _pairs(videos, n):
    return np.array([[j, i] for j in videos for i in range(n)], np.int64)


def _eq(got, want):
    return np.all(np.isfinite(want)) and np.array_equal(got, want)


# ---- 1. the scorer
@pytest.mark.parametrize("mode", ["none", "full"])
def test_a_scorer_with_removals_scores_as_a_scorer_built_from_the_survivors(lora, mode):
    t = lora
    n = t.spec["n"]
    G._set_mode(t, mode)
    try:
        whole, fresh = _scorer(t, range(n)), _scorer(t, KEEP)
        texts = np.arange(n)
        # sensitivity, before the removal: the normaliser covers 6 instead of 4 videos
        for p, j in enumerate(KEEP):
            want, got = fresh.tvg(_pairs([p], n)), whole.tvg(_pairs([j], n))
            assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)) and not np.array_equal(got, want), j
        before = whole.tvg_gallery(texts, chunk=2)                               # (gallery_feats, _label_inverse memoised over six videos now)
        assert before.shape == (n, n) and not np.array_equal(before[:, KEEP], fresh.tvg_gallery(texts, chunk=2))
        whole.tvg_first(texts, 2)
        whole.remove_videos(GONE)
        assert whole.n_live == 4 and whole.n_vocab == 4 and whole.tvg_video_labels.tolist() == [0, -1, 1, 2, -1, 3]
        assert _eq(whole.vtg(_pairs(KEEP, n)), fresh.vtg(_pairs(range(4), n)))
        assert _eq(whole.vtg(_pairs(KEEP, n), cpn=True), fresh.vtg(_pairs(range(4), n), cpn=True))      # the v2t prior
        for p, j in enumerate(KEEP):                                             # one video per text: bit-equal (section 11), likelihood and prior
            for cpn in (False, True):
                want, got = fresh.tvg(_pairs([p], n), cpn=cpn), whole.tvg(_pairs([j], n), cpn=cpn)
                assert _eq(got, want), (j, cpn, float(np.max(np.abs(got - want))))
        for chunk in (2, 3, None):                                               # fixed chunks cut over the live videos: {0, 2}, {3, 5} -- not {0, 1}, {2, 3}, {4, 5}
            want, got = fresh.tvg_gallery(texts, chunk=chunk), whole.tvg_gallery(texts, chunk=chunk)
            assert got.shape == (n, n) and _eq(got[:, KEEP], want) and np.isnan(got[:, GONE]).all(), chunk
        for kw in (dict(), dict(cpn=True, alpha=ALPHA[0])):
            (i1, v1, l1), (i2, v2, l2) = whole.tvg_first(texts, 3, full=True, **kw), fresh.tvg_first(texts, 3, full=True, **kw)
            assert np.array_equal(i1, KEEP[i2]) and _eq(v1, v2) and l1.shape == (n, n) and _eq(l1[:, KEEP], l2) and np.isnan(l1[:, GONE]).all()
            sets = [[0, 1], [3], [2, 0, 1], [1, 2], [0, 1, 2, 3], [3, 0]]       # (in `fresh`'s indices)
            (i1, v1), (i2, v2) = whole.tvg_first(texts, 3, within=[KEEP[w] for w in sets], **kw), fresh.tvg_first(texts, 3, within=sets, **kw)
            assert np.array_equal(i1, np.where(i2 >= 0, KEEP[np.maximum(i2, 0)], -1)) and np.array_equal(np.isnan(v1), np.isnan(v2))
            assert np.array_equal(v1[~np.isnan(v1)], v2[~np.isnan(v2)]) and (i2 >= 0).sum() == sum(min(3, len(w)) for w in sets)
        with pytest.raises(ValueError, match="tvg_first: k = 5 outside 1 .. 4"):
            whole.tvg_first(texts, 5)
        for call in (lambda: whole.vtg(_pairs([4], 2)), lambda: whole.tvg(_pairs([0, 1], 2)), lambda: whole.tvg_first(texts[:1], 1, within=[[0, 4]])):
            with pytest.raises(ValueError, match="was removed"):
                call()
    finally:
        G._set_mode(t, "none")


def test_remove_then_add_back_equals_the_scorer_built_with_them_appended(lora):
    t = lora
    n = t.spec["n"]
    G._set_mode(t, "none")
    order = list(KEEP) + GONE
    whole, fresh = _scorer(t, range(n)), _scorer(t, order)
    whole.tvg_gallery(np.arange(n))
    whole.remove_videos(GONE)
    got = whole.add_videos([torch.from_numpy(t.prob.video[j]) for j in GONE], torch.from_numpy(t.prob.video_vocab[GONE]))
    assert got.tolist() == [6, 7] and whole.n_live == 6 and whole.tvg_video_labels.tolist() == [0, -1, 1, 2, -1, 3, 4, 5]
    at = np.array([0, 2, 3, 5, 6, 7])                                            # video p of `fresh` in `whole`
    assert _eq(whole.vtg(_pairs(at, n)), fresh.vtg(_pairs(range(6), n)))
    for p, j in enumerate(at):
        assert _eq(whole.tvg(_pairs([j], n)), fresh.tvg(_pairs([p], n))), j
    got, want = whole.tvg_gallery(np.arange(n), chunk=4), fresh.tvg_gallery(np.arange(n), chunk=4)      # the chunk {0, 2, 3, 5} | {6, 7}
    assert got.shape == (n, 8) and _eq(got[:, at], want) and np.isnan(got[:, GONE]).all()
    (i1, v1), (i2, v2) = whole.tvg_first(np.arange(n), 6), fresh.tvg_first(np.arange(n), 6)
    assert np.array_equal(i1, at[i2]) and _eq(v1, v2)


# ---- 2. the indexes: eager, lazy, host tier
def _index(sc, fill):
    if fill == "eager":
        return GalleryIndex(sc).build()
    if fill == "lazy":
        return LG._lazy(sc, 3)
    return _tiered(sc, 2, 6)


@pytest.mark.parametrize("fill", ["eager", "lazy", "host"])
def test_the_blends_through_an_index_after_a_removal(lora, fill):
    t = lora
    n = t.spec["n"]
    G._set_mode(t, "none")
    whole, fresh = _scorer(t, range(n)), _scorer(t, KEEP)
    gal, ref = _index(whole, fill), _index(fresh, fill)
    tg, tref = TextGalleryIndex(whole, video_index=gal).build(), TextGalleryIndex(fresh, video_index=ref).build()
    try:
        texts = np.arange(n)
        more = dict(cpn=True, alpha=ALPHA, c=C_BLEND, finetuned=True)
        o0, b0 = gal.rerank(texts, np.tile(np.arange(n), (n, 1)), **more)        # priors over six videos are memoised; every video has been through the cache
        tg.rerank([0, 2], np.tile(texts, (2, 1)), **more)
        assert len(gal._prior) > 0 and len(tg._prior) > 0
        v2t_prior = dict(tg._prior)
        whole.remove_videos(GONE)
        seen_whole, seen_fresh = _count_priors(whole), _count_priors(fresh)
        o1, b1 = gal.rerank(texts, np.tile(KEEP, (n, 1)), **more)
        o2, b2 = ref.rerank(texts, np.tile(np.arange(4), (n, 1)), **more)
        assert np.array_equal(o1, KEEP[o2]) and _eq(b1, b2), float(np.max(np.abs(b1 - b2)))      # a stale prior memo fails this
        assert seen_whole == seen_fresh and sum(seen_whole) > 0                   # every t2v prior was scored again, as on the fresh index
        assert not np.array_equal(b0[:, :4], b1)
        assert _eq(gal.vtg_pairs(_pairs(KEEP, n)), ref.vtg_pairs(_pairs(range(4), n)))
        assert {k[0] for k in gal.keys} == set(KEEP.tolist()) and {k[0] for k in gal.slot_of} <= set(KEEP.tolist()) and gal.removed_stats["videos"] == 2
        # the shortlist and the prefilter: a removed video is never returned, K and K0 are clipped to what is left
        kept0 = gal.prefilter_stats["kept"]
        reqs = [SearchRequest(0, shortlist=3), SearchRequest(1, shortlist=n + 2), SearchRequest(2, shortlist=2, prefilter=50), SearchRequest(3, shortlist=4, prefilter=4),
                SearchRequest(4, shortlist=2, prefilter=3, within=[5, 0, 3])]
        mapped = [r if r.within is None else r._replace(within=[int(np.nonzero(KEEP == j)[0][0]) for j in r.within]) for r in reqs]
        got, want = gal.search_requests(reqs, **more), ref.search_requests(mapped, **more)
        for (oa, ba), (ob, bb), k in zip(got, want, (3, 4, 2, 4, 2)):
            assert len(oa) == k and np.array_equal(oa, KEEP[ob]) and _eq(ba, bb) and not set(oa.tolist()) & set(GONE)
        assert gal.prefilter_stats["kept"] - kept0 == 4 + 4 + 3                   # K0 = 50 was clipped to the four live videos
        c1, s1 = gal.shortlist(texts, n, cpn=True, alpha=ALPHA)
        c2, s2 = ref.shortlist(texts, n, cpn=True, alpha=ALPHA)
        assert c1.shape == (n, 4) and np.array_equal(c1, KEEP[c2]) and _eq(s1, s2)
        # v2t: the query likelihood over the cached caption prompts, the VTG leg from the video cache, the (text, token count) prior memo kept
        for p, j in enumerate(KEEP):
            pairs_w, pairs_f = np.stack([np.full(n, j), texts], axis=1), np.stack([np.full(n, p), texts], axis=1)
            assert _eq(tg.tvg_pairs(pairs_w), tref.tvg_pairs(pairs_f)), j
            (oa, ba), (ob, bb) = tg.rerank([j], texts[None], **more), tref.rerank([p], texts[None], **more)
            assert np.array_equal(oa, ob) and _eq(ba, bb)
            (oa, ba), (ob, bb) = tg.rerank_shortlist([j], 3, cpn=True, alpha=ALPHA, c=C_BLEND), tref.rerank_shortlist([p], 3, cpn=True, alpha=ALPHA, c=C_BLEND)
            assert np.array_equal(oa, ob) and _eq(ba, bb)
        assert all(tg._prior[k] == v for k, v in v2t_prior.items())
        with pytest.raises(ValueError, match="video 4 was removed"):
            tg.rerank([4], texts[None], **more)
    finally:
        tg.close(); tref.close(); gal.close(); ref.close()


def test_an_eager_index_without_spare_slots_replaces_a_video(tiny):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, "none")
    whole, fresh = _scorer(t, range(n)), _scorer(t, [0, 2, 3, 4, 5, 1])
    gal = GalleryIndex(whole, spare_slots=0).build()
    try:
        assert len(gal.slot_of) == gal.n_slots == n
        (freed,) = [gal.slot_of[k] for k in gal.keys if k[0] == 1]
        cache = gal.cache
        whole.remove_videos([1])
        assert whole.add_videos([torch.from_numpy(t.prob.video[1])], torch.from_numpy(t.prob.video_vocab[1:2])).tolist() == [6]
        at = [0, 2, 3, 4, 5, 6]
        for _ in range(2):                                                       # the new video gets the freed slot before the first pass; the pass after it reads it too
            got, d = LG._delta(gal, lambda: gal.vtg_pairs(_pairs(at, n)))
            assert _eq(got, fresh.vtg(_pairs(range(6), n)))
            assert (d["hits"], d["misses"], d["admitted"], d["evicted"], d["prefix_tokens_packed"]) == (6, 0, 0, 0, 0)
        assert gal.cache is cache and cache.n_slots == n and gal.slot_of[gal.keys[-1]] == freed and gal.keys[-1][0] == 6      # no cache was resized or rebuilt
        assert gal.removed_stats == {"videos": 1, "slots_freed": 1, "records_forgotten": 0}
        for p, j in enumerate(at):
            assert _eq(whole.tvg(_pairs([j], n)), fresh.tvg(_pairs([p], n))), j
    finally:
        gal.close()


def test_a_lazy_index_frees_the_slot_and_refuses_a_pending_pass(tiny):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, "none")
    whole, twin = _scorer(t, range(n)), _scorer(t, range(n))
    gal, other = LG._lazy(whole, 3), LG._lazy(twin, 3)
    try:
        first = _pairs([0, 1, 2], n)
        ref = twin.vtg(_pairs(range(n), n)).reshape(n, n)
        for g in (gal, other):
            got, d = LG._delta(g, lambda: g.vtg_pairs(first))
            assert (d["misses"], d["admitted"]) == (3, 3) and _eq(got, ref[:3].reshape(-1))
        (freed,) = [gal.slot_of[k] for k in gal.keys if k[0] == 1]
        pending = list(gal.iter_plans(_pairs([1, 3], n)))                        # planned before the removal: video 3 would take video 0's slot
        ran = len(gal.ran)
        whole.remove_videos([1])
        with pytest.raises(RuntimeError, match="plan again"):
            gal.run(pending[0])
        assert len(gal.ran) == ran + 1 and sorted(k[0] for k in gal.slot_of) == [0, 2]      # (refused before the engine saw it: nothing was admitted or evicted)
        nxt = _pairs([0, 2, 3], n)
        got, d = LG._delta(gal, lambda: gal.vtg_pairs(nxt))
        _, d2 = LG._delta(other, lambda: other.vtg_pairs(nxt))
        assert _eq(got, ref[[0, 2, 3]].reshape(-1))
        assert d == {**d2, "evicted": 0} and d2["evicted"] == 1 and (d["hits"], d["misses"], d["admitted"]) == (2, 1, 1)      # as a run without it, but for the eviction
        assert gal.slot_of[[k for k in gal.keys if k[0] == 3][0]] == freed and gal.removed_stats == {"videos": 1, "slots_freed": 1, "records_forgotten": 0}
    finally:
        gal.close(); other.close()


def test_a_host_record_of_a_removed_video_is_neither_restored_nor_counted(tiny):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, "none")
    whole = _scorer(t, range(n))
    ref = whole.vtg(_pairs(range(n), n)).reshape(n, n)
    gal = _tiered(whole, 2, n)
    try:
        def pass_(videos):
            got, d = LG._delta(gal, lambda: gal.vtg_pairs(_pairs(videos, n)))
            assert _eq(got, ref[list(videos)].reshape(-1)), videos
            return d
        pass_((0, 1)); pass_((2, 3))                                             # videos 0 and 1 lose their slots: their records go to the host
        assert gal.host.stats.spilled == 2 and {k[0] for k in gal.host.rec_of} == {0, 1}
        whole.remove_videos([0])
        d = pass_((1, 4))                                                        # video 1 comes back by a copy; video 0's record is gone
        assert gal.host.stats.restored == 1 and (d["hits"], d["misses"], d["admitted"]) == (1, 1, 1)
        assert 0 not in {k[0] for k in gal.host.rec_of} and 0 not in {k[0] for k in gal.host._stamp}
        assert gal.removed_stats == {"videos": 1, "slots_freed": 0, "records_forgotten": 1}
        with pytest.raises(ValueError, match="video 0 was removed"):
            gal.vtg_pairs(_pairs((0, 5), n))
        restored = gal.host.stats.restored
        d = pass_((5, 2))
        assert gal.host.stats.restored in (restored, restored + 1) and d["hits"] + d["misses"] == 2      # (video 2 may come back; video 0 never does)
    finally:
        gal.close()


# ---- 3. the command
def test_the_command_removes_a_video_while_it_serves(tmp_path):
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)
    prob = synth.make_problem(1, 6, dims, tok_per_clip=8, fast_video=False)        # the dry run's problem (blim_amd/search.py: --synthetic 6)
    new = synth.tensor(1, "video.outside", (dims.num_clips, 8, dims.mm_hidden_size), std=1.0)
    feat = tmp_path / "outside.pth"
    torch.save(torch.from_numpy(new), str(feat))
    lines = [json.dumps({"id": 0, "caption": 0}),
             json.dumps({"id": 1, "remove_video": "2"}),
             json.dumps({"id": 2, "caption": 0}),
             json.dumps({"id": 3, "caption": 1, "candidates": ["0", "2"]}),
             json.dumps({"id": 4, "add_video": {"vid": "2", "features": str(feat)}}),
             json.dumps({"id": 5, "caption": 0}),
             json.dumps({"id": 6, "remove_video": "2", "topk": 1})]
    src = tmp_path / "requests.jsonl"
    src.write_text("\n".join(lines) + "\n")
    cmd = [sys.executable, "-m", "blim_amd.search", "--synthetic", "6", "--topk", "8", "--vtg_precise", "none", "--candidates", "all", "--c", "1", "0", "1", "0",
           "--serve", "--batch_queries", "4", "--batch_wait_ms", "50"]
    with open(src) as stdin:
        served = subprocess.run(cmd, cwd=ROOT, stdin=stdin, capture_output=True, text=True, timeout=300)
    assert served.returncode == 0, served.stderr[-2000:]
    out = [json.loads(x) for x in served.stdout.splitlines()]
    assert [x["id"] for x in out] == list(range(7))                                 # in arrival order
    assert out[1] == {"id": 1, "removed": "2", "index": 2, "videos": 5} and out[4] == {"id": 4, "added": "2", "index": 6, "videos": 6}
    assert "unknown video id '2'" in out[3]["error"] and "carries no query" in out[6]["error"]
    # three fresh runs, in this process: a scorer over the gallery as it was for each query
    model = BlimModel(dims, dtype=None)
    try:
        model.engine.init_synthetic_weights(0)
        model.set_tvg_prefix_length(prob.tvg_prefix_length)
        model.vtg_precise = None
        prob.video.append(new)
        prob.video_vocab = np.concatenate([prob.video_vocab, new.mean(axis=1, dtype=np.float32)[None]])
        t = types.SimpleNamespace(prob=prob, model=model, dims=dims)
        for x, videos, names in ((out[0], [0, 1, 2, 3, 4, 5], "012345"), (out[2], [0, 1, 3, 4, 5], "01345"), (out[5], [0, 1, 3, 4, 5, 6], "013452")):
            ql = _scorer(t, videos).vtg(_pairs(range(len(videos)), 1))
            o = np.argsort(-ql, kind="stable")
            assert x["videos"] == [names[k] for k in o] and x["scores"] == [float(v) for v in ql[o]] and x["query"] == "caption:0"
        summary = json.loads(served.stderr.split("serve: ")[1].splitlines()[0])
        assert (summary["requests"], summary["errors"], summary["videos_added"], summary["videos_removed"]) == (7, 2, 1, 1)
        removed = json.loads(served.stderr.split("removed: ")[1].splitlines()[0])
        assert removed == {"videos": 1, "slots_freed": 1, "records_forgotten": 0}
    finally:
        model.engine.close()
