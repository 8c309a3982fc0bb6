"""GPU: videos that join a scorer at run time (PairScorer.add_videos, _PrefixIndex._sync_videos, `python -m blim_amd.search`: add_video,
--query_video).  The reference of every test is a scorer built with all videos from the start (`whole`); the scorer under test (`late`) is built with the first half
and grown.  A projected row, a GEMM row and an attention block do not depend on what else is in the scorer, and the vocabulary registered again is the same split
of the same float32 rows, so every comparison is np.array_equal: VTG scores, TVG scores with one video per text per call, tvg_gallery's fixed chunks, the priors, the
blends.  Before the growth `late`'s TVG scores differ from `whole`'s -- the normaliser runs over 3 instead of 6 videos -- which is what makes the comparisons after it
mean something.  The host side is tests/test_grow_host.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_lazy_gallery_gpu as LG
import test_text_gallery_gpu as TG
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd.gallery import GalleryIndex, TextGalleryIndex
from blim_amd.modeling import BlimModel
from test_gallery_gpu import lora, tiny  # noqa: F401  (fixtures: the tiny case and its fine-tuned twin, 6 videos and 2 layers, in fp16 and bf16)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_BLEND = (0.6, 0.5, 0.7, 0.5)
ALPHA = (0.8, 0.3)


def _scorer(t, n_videos, vocab=None, max_tokens=4096):
    """Every text of the problem over its first n_videos videos (vocab: the vocabulary's rows, default the problem's)."""
    prob = t.prob
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    vocab = torch.from_numpy(prob.video_vocab) if vocab is None else vocab
    sc = RU.PairScorer(G.DDPLike(t.model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video[:n_videos]],
                       vocab[:n_videos], torch.from_numpy(prob.tvg_video_labels[:n_videos]), t.dims.num_clips, max_tokens=max_tokens)
    sc.set_vtg_mode(t.model.vtg_mode())
    return sc


def _join(t, late):
    """The second half of the problem's videos joins, with the problem's vocabulary rows."""
    n, h = t.spec["n"], t.spec["n"] // 2
    got = late.add_videos([torch.from_numpy(v) for v in t.prob.video[h:]], torch.from_numpy(t.prob.video_vocab[h:]))
    assert got.tolist() == list(range(h, n)) and late.n_vocab == n and late.tvg_video_labels.tolist() == list(range(n))


def _all_pairs(n):
    return np.array([[j, i] for j in range(n) for i in range(n)], np.int64)


# ---- 1. late videos
@pytest.mark.parametrize("mode", ["none", "full"])
def test_late_videos_score_as_videos_given_up_front(tiny, mode):
    t = tiny
    n, h = t.spec["n"], t.spec["n"] // 2
    G._set_mode(t, mode)
    try:
        whole, late = _scorer(t, n), _scorer(t, h)
        pairs = _all_pairs(n)
        # sensitivity, before the add: the normaliser covers 3 instead of 6 videos
        for j in range(h):
            block = pairs[pairs[:, 0] == j]
            want, got = whole.tvg(block), late.tvg(block)
            assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)) and not np.array_equal(got, want), j
        assert late.tvg_gallery(np.arange(n), chunk=2).shape == (n, h)          # (gallery_feats is memoised over three videos now)
        _join(t, late)
        ref = whole.vtg(pairs)
        got = late.vtg(pairs)
        assert np.all(np.isfinite(ref)) and np.array_equal(got, ref), float(np.max(np.abs(got - ref)))
        for j in range(n):                                                       # one video per text: bit-equal (section 11)
            block = pairs[pairs[:, 0] == j]
            want, got = whole.tvg(block), late.tvg(block)
            assert np.all(np.isfinite(want)) and np.array_equal(got, want), (j, float(np.max(np.abs(got - want))))
        want, got = whole.tvg_gallery(np.arange(n), chunk=2), late.tvg_gallery(np.arange(n), chunk=2)      # the chunk {2, 3} straddles old and new videos
        assert want.shape == (n, n) and np.all(np.isfinite(want)) and np.array_equal(got, want), float(np.max(np.abs(got - want)))
    finally:
        G._set_mode(t, "none")


def test_the_default_vocabulary_row_is_the_clip_mean(tiny):
    t = tiny
    n, h = t.spec["n"], t.spec["n"] // 2
    G._set_mode(t, "none")
    V = [torch.from_numpy(v) for v in t.prob.video]
    vocab = torch.stack([v.float().mean(1) for v in V])
    whole, late = _scorer(t, n, vocab), _scorer(t, h, vocab)
    assert late.add_videos(V[h:]).tolist() == list(range(h, n))
    for j in (0, n - 1):
        block = np.array([[j, i] for i in range(n)], np.int64)
        want, got = whole.tvg(block), late.tvg(block)
        assert np.all(np.isfinite(want)) and np.array_equal(got, want), j


# ---- 2. an eager index and its spare slots
@pytest.mark.parametrize("mode", ["none", "full"])
def test_an_eager_index_fills_new_videos_into_its_spare_slots(tiny, mode):
    t = tiny
    n, h = t.spec["n"], t.spec["n"] // 2
    G._set_mode(t, mode)
    try:
        whole = _scorer(t, n)
        pairs = _all_pairs(n)
        ref = whole.vtg(pairs)
        assert np.all(np.isfinite(ref))
        for spare in (3, 1, 0):
            late = _scorer(t, h)
            gal = GalleryIndex(late, spare_slots=spare).build()
            try:
                assert (len(gal.keys), len(gal.slot_of), gal.n_slots, gal.cache.n_slots) == (h, h, h + spare, h + spare)
                old = pairs[pairs[:, 0] < h]
                got, d = LG._delta(gal, lambda: gal.vtg_pairs(old))
                assert np.array_equal(got, ref[pairs[:, 0] < h]) and (d["hits"], d["misses"]) == (h, 0)
                cache = gal.cache
                _join(t, late)
                cached = min(spare, n - h)
                for _ in range(2):                                               # the new videos get their slots at the next pass; the pass after it reads them too
                    got, d = LG._delta(gal, lambda: gal.vtg_pairs(pairs))
                    assert np.array_equal(got, ref), (spare, float(np.max(np.abs(got - ref))))
                    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (h + cached, n - h - cached, 0, 0)
                    assert (d["prefix_tokens_packed"] == 0) == (cached == n - h)
                assert gal.cache is cache and cache.n_slots == h + spare           # no cache was resized or rebuilt
                assert (len(gal.keys), len(gal.slot_of)) == (n, h + cached) and sorted(gal.slot_of.values()) == list(range(h + cached))
                assert [k[0] for k in gal.keys if k in gal.slot_of] == list(range(h + cached))      # in key order
            finally:
                gal.close()
    finally:
        G._set_mode(t, "none")


# ---- 3. a lazy index and its host tier
def _tiered(sc, capacity, records):
    gal = GalleryIndex(sc, fill="lazy", host_budget_bytes=0)
    gal.budget_bytes = capacity * gal.per_slot_bytes()
    probe = sc.engine.prefix_cache(1, gal.slot_positions(), gal.compensated())
    gal.host_budget_bytes = records * probe.record_bytes(gal.slot_positions())
    probe.close()
    gal.build()
    assert gal.n_slots == capacity and gal.host is not None and gal.host.n_records == records
    return gal


@pytest.mark.parametrize("mode", ["none", "full"])
def test_a_lazy_index_admits_new_videos_and_restores_what_it_spilled_before(tiny, mode):
    t = tiny
    n, h = t.spec["n"], t.spec["n"] // 2
    G._set_mode(t, mode)
    try:
        whole, late = _scorer(t, n), _scorer(t, h)
        gal = _tiered(late, 2, n)
        try:
            def pass_(videos):
                pairs = np.array([[j, i] for j in videos for i in range(n)], np.int64)
                want = whole.vtg(pairs)
                got, d = LG._delta(gal, lambda: gal.vtg_pairs(pairs))
                assert np.all(np.isfinite(want)) and np.array_equal(got, want), (videos, float(np.max(np.abs(got - want))))
                return d
            d = pass_((0, 1))
            assert (d["hits"], d["misses"], d["admitted"]) == (0, 2, 2)
            d = pass_((2,))                                                      # video 0 loses its slot: its record goes to the host
            assert (d["misses"], d["admitted"], d["evicted"]) == (1, 1, 1) and gal.host.stats.spilled == 1
            records = dict(gal.host.rec_of)
            _join(t, late)
            d = pass_((3, 4))                                                    # new keys: admitted on demand, like any miss
            assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (0, 2, 2, 2) and len(gal.keys) == n
            assert all(gal.host.rec_of.get(k) == r for k, r in records.items()) and gal.host.stats.restored == 0
            d = pass_((0, 5))                                                    # video 0's record, spilled before the growth, comes back by a copy
            assert gal.host.stats.restored == 1 and (d["hits"], d["misses"], d["admitted"]) == (1, 1, 1)
            assert {k[0] for k in gal.slot_of} == {0, 5}
            d = pass_((0, 5))
            assert (d["hits"], d["misses"], d["prefix_tokens_packed"]) == (2, 0, 0)
        finally:
            gal.close()
    finally:
        G._set_mode(t, "none")


# ---- 4. the prior memo
def _count_priors(sc):
    """-> the list the pair counts of the scorer's prior passes (tvg(..., cpn=True)) are appended to."""
    seen, tvg = [], sc.tvg

    def counted(pairs, cpn=False):
        if cpn:
            seen.append(len(pairs))
        return tvg(pairs, cpn)
    sc.tvg = counted
    return seen


def test_the_prior_memo_is_dropped_when_the_vocabulary_grows(lora):
    t = lora
    n, h = t.spec["n"], t.spec["n"] // 2
    G._set_mode(t, "none")
    whole, late = _scorer(t, n), _scorer(t, h)
    gal, fresh = GalleryIndex(late).build(), None
    try:
        texts = np.arange(n)
        more = dict(cpn=True, alpha=ALPHA, c=C_BLEND, finetuned=True)
        gal.rerank(texts, np.tile(np.arange(h), (n, 1)), **more)                 # priors over three videos are memoised
        assert len(gal._prior) > 0
        _join(t, late)
        seen_late, seen_whole = _count_priors(late), _count_priors(whole)
        cand = np.tile(np.arange(n), (n, 1))
        order, blended = gal.rerank(texts, cand, **more)
        fresh = GalleryIndex(whole).build()
        o2, b2 = fresh.rerank(texts, cand, **more)
        assert np.all(np.isfinite(b2)) and np.array_equal(order, o2) and np.array_equal(blended, b2), float(np.max(np.abs(blended - b2)))      # a stale memo fails this
        assert seen_late == seen_whole and sum(seen_late) > 0                     # every prior was scored again, as on the fresh index
        assert np.array_equal(gal._t2v_prior(texts, cand), fresh._t2v_prior(texts, cand)) and seen_late == seen_whole
    finally:
        gal.close()
        if fresh is not None:
            fresh.close()


# ---- 5. the shortlist
def test_the_shortlist_after_growth(lora):
    t = lora
    n, h = t.spec["n"], t.spec["n"] // 2
    G._set_mode(t, "none")
    whole, late = _scorer(t, n), _scorer(t, h)
    gal, ref = GalleryIndex(late).build(), GalleryIndex(whole).build()
    try:
        texts = [0, 3, 5]
        cand, stage = gal.shortlist(texts, 2, cpn=True, alpha=ALPHA)             # (stage 1, gallery_feats and the priors over three videos)
        assert cand.shape == (3, 2) and cand.max() < h
        _join(t, late)
        for K in (4, n + 2):
            c1, s1 = gal.shortlist(texts, K, cpn=True, alpha=ALPHA)
            c2, s2 = ref.shortlist(texts, K, cpn=True, alpha=ALPHA)
            assert c1.shape == (3, min(K, n)) and np.all(np.isfinite(s2)) and np.array_equal(c1, c2) and np.array_equal(s1, s2)
        assert c2.max() >= h                                                      # (the new videos are ranked)
        iv2 = t.prob.t2v_sims.astype(np.float32)
        c5 = np.array([4, 1, 5, 0])
        batch = [(0, None, None, 3), (5, c5, iv2[5][c5], None), (2, None, None, n), (1, np.array([4, 1]), None, None), (3, None, None, 1), (4, np.array([5]), None, None)]
        for more in (dict(cpn=True, alpha=ALPHA, c=C_BLEND, finetuned=True), dict(cpn=False, alpha=ALPHA, c=(1.0, 0.0, 1.0, 0.0), finetuned=True)):
            got, want = gal.search_requests(batch, **more), ref.search_requests(batch, **more)
            for (o1, b1), (o2, b2) in zip(got, want):
                assert np.all(np.isfinite(b2)) and np.array_equal(o1, o2) and np.array_equal(b1, b2)
    finally:
        gal.close(); ref.close()


# ---- 6. v2t: a query video from outside
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_v2t_with_a_video_that_joined(lora, mode):
    t = lora
    n, h = t.spec["n"], t.spec["n"] // 2
    G._set_mode(t, "none")
    whole, late = _scorer(t, n), _scorer(t, h)
    TG._set_tvg(t, whole, mode); TG._set_tvg(t, late, mode)
    vg, vg_ref = GalleryIndex(late).build(), GalleryIndex(whole).build()
    tg, ref = TextGalleryIndex(late, video_index=vg).build(), TextGalleryIndex(whole, video_index=vg_ref).build()
    try:
        more = dict(cpn=True, alpha=ALPHA, c=C_BLEND)
        cand = np.arange(n)[None]
        tg.rerank([0], cand, finetuned=True, **more)                             # the v2t prior is memoised per (text, token count) ...
        slots, prior = dict(tg.slot_of), dict(tg._prior)
        _join(t, late)
        prior_passes = []
        vtg = late.vtg
        late.vtg = lambda pairs, cpn=False: (prior_passes.append(len(pairs)) if cpn else None) or vtg(pairs, cpn)
        for v in range(h, n):
            pairs = np.stack([np.full(n, v), np.arange(n)], axis=1)
            want = ref.tvg_pairs(pairs)
            assert np.all(np.isfinite(want)) and np.array_equal(tg.tvg_pairs(pairs), want), v
            assert np.array_equal(tg.vtg_pairs(pairs), ref.vtg_pairs(pairs))
            (o1, b1), (o2, b2) = tg.rerank([v], cand, finetuned=True, **more), ref.rerank([v], cand, finetuned=True, **more)
            assert np.all(np.isfinite(b2)) and np.array_equal(o1, o2) and np.array_equal(b1, b2)
            (o1, b1), (o2, b2) = tg.rerank_shortlist([v], 3, **more), ref.rerank_shortlist([v], 3, **more)
            assert np.array_equal(o1, o2) and np.array_equal(b1, b2)
        assert tg.slot_of == slots and tg._prior == prior and prior_passes == []    # ... and VTG-side state does not depend on the vocabulary: it stays
    finally:
        tg.close(); ref.close(); vg.close(); vg_ref.close(); TG._set_tvg(t, whole, "full")


# ---- 7. the command
def test_the_command_adds_a_video_while_it_serves_and_takes_one_as_a_query(tmp_path):
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)
    prob = synth.make_problem(1, 6, dims, tok_per_clip=8, fast_video=False)        # the dry run's problem (blim_amd/search.py: --synthetic 6)
    new = synth.tensor(1, "video.outside", (dims.num_clips, 8, dims.mm_hidden_size), std=1.0)
    feat = tmp_path / "outside.pth"
    torch.save(torch.from_numpy(new), str(feat))
    bad = tmp_path / "bad.pth"
    torch.save(torch.zeros((dims.num_clips + 1, 8, dims.mm_hidden_size)), str(bad))
    lines = [json.dumps({"id": 0, "caption": 0, "candidates": ["0", "2", "5"]}),
             json.dumps({"id": 1, "add_video": {"vid": "outside", "features": str(feat)}}),
             json.dumps({"id": 2, "caption": 0, "candidates": ["0", "outside", "5"]}),
             json.dumps({"id": 3, "add_video": {"vid": "another", "features": str(bad)}}),
             json.dumps({"id": 4, "add_video": {"vid": "copy", "features": str(feat)}}),
             json.dumps({"id": 5, "caption": 3, "candidates": ["outside"]})]
    src = tmp_path / "requests.jsonl"
    src.write_text("\n".join(lines) + "\n")
    base = [sys.executable, "-m", "blim_amd.search", "--synthetic", "6", "--topk", "3", "--vtg_precise", "none"]
    with open(src) as stdin:
        served = subprocess.run(base + ["--serve", "--batch_queries", "4", "--batch_wait_ms", "50", "--gallery_spare", "1"], cwd=ROOT, stdin=stdin, capture_output=True,
                                text=True, timeout=300)
    assert served.returncode == 0, served.stderr[-2000:]
    one_shot = subprocess.run(base + ["--direction", "v2t", "--query_video", str(feat), "--candidates", "all"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert one_shot.returncode == 0, one_shot.stderr[-2000:]
    # the reference: a scorer that had the video from the start, in this process
    model = BlimModel(dims, dtype=None)
    try:
        model.engine.init_synthetic_weights(0)
        model.set_tvg_prefix_length(prob.tvg_prefix_length)
        model.vtg_precise = None
        prob.video.append(new)
        t = types.SimpleNamespace(prob=prob, model=model, dims=dims)
        sc = _scorer(t, 7, torch.from_numpy(np.concatenate([prob.video_vocab, new.mean(axis=1, dtype=np.float32)[None]])))
        sc.tvg_video_labels = np.arange(7, dtype=np.int32)

        def ranked(pairs, names):
            ql = sc.vtg(np.asarray(pairs, np.int64))
            o = np.argsort(-ql, kind="stable")
            return [names[k] for k in o], [float(x) for x in ql[o]]
        out = [json.loads(x) for x in served.stdout.splitlines()]
        assert [x["id"] for x in out] == [0, 1, 2, 3, 4, 5]                         # in arrival order
        assert out[1] == {"id": 1, "added": "outside", "index": 6, "videos": 7}
        assert set(out[3]) == set(out[4]) == {"id", "error"} and "clips" in out[3]["error"] and "'outside'" in out[4]["error"]      # ... and the process went on
        for x, (text, cand) in ((out[0], (0, [0, 2, 5])), (out[2], (0, [0, 6, 5])), (out[5], (3, [6]))):
            videos, scores = ranked([[j, text] for j in cand], ["outside" if j == 6 else str(j) for j in cand])
            assert (x["videos"], x["scores"]) == (videos, scores) and x["query"] == f"caption:{text}"
        summary = json.loads(served.stderr.split("serve: ")[1].splitlines()[0])
        assert (summary["requests"], summary["errors"], summary["videos_added"]) == (6, 2, 1)
        stats = json.loads(served.stderr.split("gallery stats: ")[1].splitlines()[0])
        # the added video was filled into the spare slot: no pass packed a prefix (requests 2 and 5 are one pass of 3 keys or two of 3 + 1, as the lines arrive)
        assert stats["misses"] == 0 and stats["prefix_tokens_packed"] == 0 and stats["hits"] in (3 + 3, 3 + 3 + 1)
        line, = [json.loads(x) for x in one_shot.stdout.splitlines()]
        texts, scores = ranked([[6, i] for i in range(6)], list(range(6)))
        assert line == {"query": "video:outside.pth", "texts": texts, "scores": scores}
    finally:
        model.engine.close()
