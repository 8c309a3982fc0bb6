"""GPU: searching inside a caller's set of videos -- PairScorer.tvg_first(within=) / Engine.score_tvg_first_within against the whole-gallery
order of tvg_first(k = N) filtered to the set (indices exactly, values bit for bit), two texts on one packed prompt with different sets, and GalleryIndex.search_requests
with `within` against the same request without it (within = every video), against the composition of the public calls, over an eager and a lazy index, and after a
video joined.  The small synthetic model of tests/test_prefilter_gpu.py: N = 37 videos, 5 texts, fp16 and bf16.  The host side is tests/test_within_host.py."""
import numpy as np
import pytest
import torch

import test_prefilter_gpu as PG
from blim_amd.engine import TVG_RANK_MAX_K
from blim_amd.gallery import GalleryIndex, SearchRequest

pytestmark = pytest.mark.gpu
N, ALPHA, C_BLEND = PG.N, PG.ALPHA, PG.C_BLEND
four_clips = PG.four_clips
_bits = PG._bits


def _sets(seed, n_texts, n=N):
    """One set per text: sizes 1, n, and random ones between; given unsorted."""
    rs = np.random.RandomState(seed)
    sizes = [1, n] + [int(rs.randint(2, n)) for _ in range(n_texts - 2)]
    return [rs.permutation(n)[:m] for m in sizes]


@pytest.mark.parametrize("cpn", [False, True])
def test_within_is_the_whole_gallery_order_filtered_to_the_set(four_clips, cpn):
    t = four_clips
    sc, texts = PG._scorer(t)
    kw = dict(cpn=cpn, alpha=ALPHA[0])
    idx_all, val_all = sc.tvg_first(texts, N, **kw)
    calls = PG._counted(sc)
    sets = _sets(11 + cpn, len(texts))
    assert set(sets[0].tolist()) != set(sets[2].tolist())                          # texts[0] and its twin: one packed prompt, two sets
    for k in (1, 8, N, 64):
        del calls[:]
        idx, val = sc.tvg_first(texts, k, within=sets, **kw)
        assert len(calls) == 1 and calls[0].n_pairs == 4                           # each distinct prompt packed once: row_of carries the fan-out
        assert idx.dtype == np.int64 and val.dtype == np.float32 and idx.shape == val.shape == (len(texts), k)
        for q, w in enumerate(sets):
            inside = np.isin(idx_all[q], w)
            want_i, want_v = idx_all[q][inside][:k], val_all[q][inside][:k]
            kk = min(k, len(w))
            assert len(want_i) == kk and np.array_equal(idx[q, :kk], want_i) and np.array_equal(_bits(val[q, :kk]), _bits(want_v))
            assert (idx[q, kk:] == -1).all() and np.isnan(val[q, kk:]).all()
    # a set given with repeats is made unique; the answer does not depend on what shares the call
    i1, v1 = sc.tvg_first([texts[3]], 8, within=[np.concatenate([sets[3], sets[3][:2]])], **kw)
    i2, v2 = sc.tvg_first(texts, 8, within=sets, **kw)
    assert np.array_equal(i1[0], i2[3]) and np.array_equal(_bits(v1[0]), _bits(v2[3]))
    for bad, msg in ((dict(k=4, full=True), "full=True"), (dict(k=0), "outside 1"), (dict(k=TVG_RANK_MAX_K + 1), "TVG_RANK_MAX_K"), (dict(k=4, within=sets[:2]), "2 sets for 5 texts"),
                     (dict(k=4, within=[np.array([0, N])] * 5), "outside 0")):
        with pytest.raises(ValueError, match=msg):
            sc.tvg_first(texts, **{**dict(within=sets), **bad})


def _lazy(sc, capacity):
    gal = GalleryIndex(sc, fill="lazy")
    gal.budget_bytes = capacity * gal.per_slot_bytes()
    return gal.build()


@pytest.mark.parametrize("cpn", [False, True])
def test_requests_inside_a_set_are_the_composition_of_the_public_calls(four_clips, cpn):
    t = four_clips
    sc, texts = PG._scorer(t)
    a, b, twin, c, d = texts
    more = dict(cpn=cpn, alpha=ALPHA, c=C_BLEND, finetuned=True)
    vtg_only = dict(more, c=(1.0, 0.0, 1.0, 0.0))
    rs = np.random.RandomState(3)
    sub_a, sub_c, sub_d = rs.permutation(N)[:20], rs.permutation(N)[:9], rs.permutation(N)[:5]
    for lazy in (False, True):
        gal = _lazy(sc, 12) if lazy else GalleryIndex(sc).build()
        try:
            # within = every video: the same request without it
            plain = gal.search_requests([(a, None, None, 3, 8), (c, None, None, 4, 12)], **more)
            whole = gal.search_requests([SearchRequest(a, shortlist=3, prefilter=8, within=np.arange(N)), SearchRequest(c, shortlist=4, prefilter=12, within=rs.permutation(N))], **more)
            for (o1, b1), (o2, b2) in zip(plain, whole):
                assert np.array_equal(o1, o2) and np.array_equal(b1, b2)
            # proper subsets, in one batch with a plain request: one pass, every answer inside its set
            passes, before = gal._n_pass, dict(gal.within_stats)
            batch = [SearchRequest(a, shortlist=3, prefilter=8, within=sub_a), (b, np.array([4, 1, 30]), None, None), SearchRequest(c, shortlist=4, prefilter=6, within=sub_c),
                     SearchRequest(d, shortlist=9, within=sub_d)]
            got = gal.search_requests(batch, **more)
            assert gal._n_pass == passes + 1
            assert gal.within_stats == {"queries": before["queries"] + 3, "candidates": before["candidates"] + 20 + 9 + 5}
            for n, w in ((0, sub_a), (2, sub_c), (3, sub_d)):
                assert set(got[n][0].tolist()) <= set(w.tolist()) and len(got[n][0]) == min(batch[n].shortlist, len(w)) and np.all(np.isfinite(got[n][1]))
            assert sorted(got[3][0].tolist()) == sorted(sub_d.tolist())             # K above the set's size: the whole set
            # the composition by hand: tvg_first(within=) -> ONE PairScorer.tvg call over the kept pairs -> _best -> vtg_pairs -> _blend
            first, _ = sc.tvg_first([a, c], 8, cpn=cpn, alpha=ALPHA[0], within=[sub_a, sub_c])
            kept = [np.sort(first[0][:8]), np.sort(first[1][:6]), np.sort(sub_d)]
            assert np.array_equal(kept[0], gal.prefilter([a], 8, cpn=cpn, alpha=ALPHA, within=[sub_a])[0])
            ts = (a, c, d)
            term = sc.tvg(np.concatenate([np.stack([row, np.full(len(row), i)], axis=1) for row, i in zip(kept, ts)]))
            if cpn:
                term = term - ALPHA[0] * gal._t2v_prior(list(ts), kept)
            for (order, blended), row, tm, i, K in zip((got[0], got[2], got[3]), kept, np.split(term, [8, 14]), ts, (3, 4, 9)):
                keep, stage = gal._best(tm, K)
                cand = row[keep]
                ql = gal.vtg_pairs(np.stack([cand, np.full(len(cand), i)], axis=1))
                o, bl = gal._blend(cand[None], ql[None], stage[None], np.zeros((1, len(cand))), C_BLEND)
                assert np.array_equal(order, o[0]) and np.array_equal(blended, bl[0])
                # ... and, on the VTG term, the explicit-candidates request over what the set's stages chose
                (o1, b1), = gal.search_requests([SearchRequest(i, shortlist=K, prefilter=None if i == d else len(row), within=row)], **vtg_only)
                (o2, b2), = gal.search_requests([(i, o1, None)], **vtg_only)
                assert set(o1.tolist()) <= set(row.tolist()) and len(o1) == len(cand) and np.array_equal(o1, o2) and np.array_equal(b1, b2)
        finally:
            gal.close()


def test_a_lazy_index_moves_its_counters_only_by_the_rerank(four_clips):
    t = four_clips
    sc, texts = PG._scorer(t)
    a = texts[0]
    more = dict(cpn=False, alpha=ALPHA, c=C_BLEND, finetuned=True)
    sub = np.random.RandomState(8).permutation(N)[:25]
    one, two = _lazy(sc, 12), _lazy(sc, 12)
    try:
        (order, blended), = one.search_requests([SearchRequest(a, shortlist=4, prefilter=10, within=sub)], **more)
        (o2, b2), = two.search_requests([(a, order, None)], **more)                 # the parent's form over the four survivors
        d1, d2 = one.stats.as_dict(), two.stats.as_dict()
        assert d1 == d2 and d1["hits"] + d1["misses"] > 0, (d1, d2)                # 25 videos in the set, 10 through stage 0: only the 4 reranked touch the cache
        assert set(o2.tolist()) == set(order.tolist())
    finally:
        one.close(); two.close()


def test_a_set_may_name_a_video_that_joined(four_clips):
    t = four_clips
    sc, texts = PG._scorer(t)
    gal = GalleryIndex(sc).build()
    try:
        a = texts[0]
        with pytest.raises(ValueError, match=f"within: video index {N} outside"):
            gal.search_requests([SearchRequest(a, shortlist=2, prefilter=3, within=[1, N])], cpn=False, alpha=ALPHA, c=C_BLEND, finetuned=True)
        new, = sc.add_videos([torch.from_numpy(t.prob.video[3] * 0.5 + t.prob.video[11] * 0.5)]).tolist()
        assert new == N
        whole, wv = sc.tvg_first([a], N + 1)
        idx, val = sc.tvg_first([a], 3, within=[[new, 5, 20, 1]])
        inside = np.isin(whole[0], [new, 5, 20, 1])
        assert np.array_equal(idx[0], whole[0][inside][:3]) and np.array_equal(_bits(val[0]), _bits(wv[0][inside][:3]))
        (order, blended), = gal.search_requests([SearchRequest(a, shortlist=4, prefilter=4, within=[new, 5, 20, 1])], cpn=False, alpha=ALPHA, c=C_BLEND, finetuned=True)
        assert sorted(order.tolist()) == sorted([new, 5, 20, 1]) and np.all(np.isfinite(blended))
    finally:
        gal.close()
