"""CPU: videos that leave a scorer at run time (blim_amd/pair_scorer.py: PairScorer.remove_videos, live / n_live; blim_amd/gallery.py:
_PrefixIndex._follow_removed, HostTier.forget, removed_stats; blim_amd/search.py: the remove_video request) -- the checks are all-or-nothing, a removed index is a
tombstone and no other index moves, a vocabulary entry leaves with its last live video and the labels are compacted, every entry that takes video indices refuses
a removed one by name, the whole-gallery planner cuts its chunks over the live videos (the calls of a scorer built from the survivors), the indexes drop the keys,
stamps, reservations and host records of what left and hand the freed slot to the next video that joins, and a removal is a barrier in the serve loop.  Fakes as
in tests/test_grow_host.py and tests/test_within_host.py: no engine.  The GPU side is tests/test_remove_gpu.py."""
import json
import types

import numpy as np
import pytest
import torch

import test_gallery_host as GH
import test_grow_host as GW
import test_host_logic as HL
import test_host_tier_host as HT
import test_lazy_gallery_host as LZ
import test_serve_host as SH
import test_text_gallery_host as TH
from blim_amd import gallery as GL
from blim_amd import retrieval_utils as RU
from blim_amd import search as SR
from blim_amd import synth
from blim_amd.gallery import SearchRequest
from blim_amd.pair_scorer import _clip_major_vocab

NV, H = GH.NV, GH.H


# ---- remove_videos on a real PairScorer (planning only: tests/test_host_logic.py's fake model)
def _scorer(dims, prob, videos, labels=None, vocab=True, engine=None, max_tokens=4096):
    """All of the problem's texts over the videos `videos` of it, in that order, each with its own vocabulary row (labels: others, over the rows of range(max + 1))."""
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    T = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(T(prob.vtg_ids), T(prob.vtg_labels), T(prob.vtg_masks), tok)
    tvg = RU.padding_ids(T(prob.tvg_ids), T(prob.tvg_labels), T(prob.tvg_masks), tok)
    fake = HL._FakeModel(dims, prob.tvg_prefix_length)
    fake.engine = engine
    if labels is None:
        rows, labels = torch.from_numpy(prob.video_vocab[list(videos)]), np.arange(len(videos))
    else:
        rows = torch.from_numpy(prob.video_vocab[: int(max(labels)) + 1])
    return RU.PairScorer(fake, vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(prob.video[j]) for j in videos], rows if vocab else None,
                         torch.from_numpy(np.asarray(labels, np.int64)), dims.num_clips, max_tokens=max_tokens)


def _state(sc):
    return ([v is None for v in sc.video], sc.tvg_video_labels.tolist(), sc.n_vocab, sc.vocab_version, sc.live.tolist(), sc.n_live, sorted(sc._vfeat),
            None if sc.vocab_cm is None else sc.vocab_cm.clone())


def _same_state(a, b):
    return a[:7] == b[:7] and ((a[7] is None and b[7] is None) or torch.equal(a[7], b[7]))


def test_remove_videos_is_all_or_nothing_and_names_each_broken_rule():
    dims, prob = SH._problem()
    sc = _scorer(dims, prob, range(6))
    sc.video_feat(2, True)
    before = _state(sc)
    assert sc.live.tolist() == [True] * 6 and sc.live.dtype == bool and sc.n_live == 6
    for bad, words in (([6], "outside 0 .. 5"), ([-1], "outside 0 .. 5"), ([1, 3, 1], "video index 1 named twice"), ([1.5], "integer video indices"),
                       (["a"], "integer video indices"), ([True], "integer video indices"), (list(range(6)), "at least one video must remain")):
        with pytest.raises(ValueError, match="remove_videos: .*" + words):
            sc.remove_videos([2] + bad if bad != list(range(6)) else bad)          # the good index in front of it is not removed either
        assert _same_state(_state(sc), before), bad
    sc.remove_videos([])
    assert _same_state(_state(sc), before)                                          # nothing named: nothing changes, no version either
    sc.remove_videos([4])
    with pytest.raises(ValueError, match="remove_videos: video 4 was removed already"):
        sc.remove_videos([2, 4])
    assert sc.n_live == 5 and sc.video[2] is not None
    sc.remove_videos([0, 1, 2, 3])
    with pytest.raises(ValueError, match="at least one video must remain"):
        sc.remove_videos([5])
    assert sc.live.tolist() == [False] * 5 + [True] and sc.n_vocab == 1 and sc.tvg_video_labels.tolist() == [-1] * 5 + [0]


def test_tombstones_compacted_labels_and_the_vocabulary_registered_whole():
    dims, prob = SH._problem()
    sc, fresh = _scorer(dims, prob, range(6)), _scorer(dims, prob, [0, 2, 3, 5])
    V = list(sc.video)
    for j in range(6):
        sc.video_feat(j, True); sc.video_feat(j, False)
    sc.gallery_feats(); sc._label_inverse()
    version = sc.vocab_version
    assert sc.remove_videos([4, 1]) is None
    assert len(sc.video) == 6 and [v is None for v in sc.video] == [False, True, False, False, True, False]
    assert all(sc.video[j] is V[j] for j in (0, 2, 3, 5))                           # no other index moves
    assert sc.live.tolist() == [True, False, True, True, False, True] and sc.n_live == 4
    assert sc.tvg_video_labels.tolist() == [0, -1, 1, 2, -1, 3] and sc.tvg_video_labels.dtype == np.int32
    assert sorted(sc._vfeat) == sorted((j, t) for j in (0, 2, 3, 5) for t in (False, True))      # the removed videos' projected rows are dropped, the rest stay
    assert sc.vocab_version == version + 1 and sc.n_vocab == 4
    assert torch.equal(sc._vocab_src, fresh._vocab_src) and sc._vocab_src.dtype == torch.float32
    assert torch.equal(sc.vocab_cm, fresh.vocab_cm) and torch.equal(sc.vocab_cm, _clip_major_vocab(torch.from_numpy(prob.video_vocab[[0, 2, 3, 5]]), "cpu", torch.float16))
    # the memos keyed by the version are made again, over what is left
    assert sc.gallery_feats().shape[0] == 4 * dims.num_clips and sc._gfeat[0][2] == sc.vocab_version
    inv, lab = sc._label_inverse_host()
    assert inv.tolist() == [0, 2, 3, 5] and lab.tolist() == [0, -1, 1, 2, -1, 3] and sc._label_inverse()[1].tolist() == [0, 1, 2, 3]
    # a video that joins afterwards takes the next index and the next label: nothing is reused
    assert sc.add_videos([V[1]], torch.from_numpy(prob.video_vocab[1:2])).tolist() == [6]
    assert sc.tvg_video_labels.tolist() == [0, -1, 1, 2, -1, 3, 4] and sc.n_vocab == 5 and sc.n_live == 5 and sc.live.tolist()[-1]
    assert torch.equal(sc._vocab_src, torch.from_numpy(prob.video_vocab[[0, 2, 3, 5, 1]]))


def test_an_entry_leaves_with_its_last_live_video():
    dims, prob = SH._problem()
    sc = _scorer(dims, prob, range(6), labels=[0, 1, 1, 2, 3, 3])                   # videos 1, 2 and videos 4, 5 share an entry
    rows = torch.from_numpy(prob.video_vocab[:4])
    cm = sc.vocab_cm.clone()
    sc.remove_videos([1])                                                           # video 2 still has entry 1: the vocabulary is what it was
    assert sc.n_vocab == 4 and sc.tvg_video_labels.tolist() == [0, -1, 1, 2, 3, 3] and torch.equal(sc.vocab_cm, cm) and sc.vocab_version == 2
    sc.remove_videos([2, 4])                                                        # entry 1 leaves with video 2; entry 3 stays for video 5
    assert sc.n_vocab == 3 and sc.tvg_video_labels.tolist() == [0, -1, -1, 1, -1, 2] and sc.vocab_version == 3
    assert torch.equal(sc._vocab_src, rows[[0, 2, 3]]) and torch.equal(sc.vocab_cm, _clip_major_vocab(rows[[0, 2, 3]], "cpu", torch.float16))
    with pytest.raises(ValueError, match="permutation"):                            # (two live videos of one entry: the rank kernels cannot name them)
        _scorer(dims, prob, range(6), labels=[0, 1, 1, 2, 3, 3])._label_inverse()
    sc._label_inverse()                                                             # ... and here each live video has its own entry now


def test_the_vocabulary_goes_to_the_engine_whole_and_a_scorer_without_one_touches_none():
    dims, prob = SH._problem()
    seen = []
    engine = types.SimpleNamespace(can_precise=True, _vocab_key=None)

    def set_video_vocab(v):
        seen.append(v.clone())
        engine._vocab_key = ("key", len(seen))
    engine.set_video_vocab = set_video_vocab
    sc = _scorer(dims, prob, range(5), engine=engine)
    sc.remove_videos([0, 3])
    assert len(seen) == 2 and torch.equal(seen[1], torch.from_numpy(prob.video_vocab[[1, 2, 4]])) and seen[1].dtype == torch.float32
    assert sc._vocab_key == ("key", 2) and sc.vocab_cm is None and sc.n_vocab == 3
    plain = _scorer(dims, prob, range(4), vocab=False)
    plain.remove_videos([2])
    assert plain.n_vocab == 0 and plain._vocab_src is None and plain.vocab_cm is None and plain.vocab_version == 2
    assert plain.tvg_video_labels.tolist() == [0, 1, -1, 3] and plain.live.tolist() == [True, True, False, True]
    for a, b in zip(plain.plan_vtg(np.array([[3, 0], [0, 2]])), _scorer(dims, prob, [0, 1, 3], vocab=False).plan_vtg(np.array([[2, 0], [0, 2]]))):
        assert GH.plan_difference(a, b) is None


def test_a_scorer_that_never_removed_anything_keeps_the_words_of_its_label_rule():
    dims, prob = SH._problem()
    sc = _scorer(dims, prob, range(4), labels=[0, 1, 1, 2])
    with pytest.raises(ValueError, match=r"tvg_first: tvg_video_labels must be a permutation of arange\(4\) -- one vocabulary entry per video \(3 entries, 3 distinct labels\)"):
        sc._label_inverse()


def test_every_entry_that_takes_video_indices_refuses_a_removed_one_by_name():
    dims, prob = SH._problem()
    sc = _scorer(dims, prob, range(6))
    sc.remove_videos([1, 4])
    bad, good = np.array([[0, 0], [4, 2]]), np.array([[0, 0], [5, 2]])
    calls = {
        "vtg": lambda: sc.vtg(bad), "tvg": lambda: sc.tvg(bad), "vtg prior": lambda: sc.vtg(bad, cpn=True), "tvg prior": lambda: sc.tvg(bad, cpn=True),
        "plan_vtg": lambda: sc.plan_vtg(bad), "plan_tvg": lambda: sc.plan_tvg(bad), "iter_vtg_jobs": lambda: list(sc.iter_vtg_jobs([(good, False), (bad, True)])),
        "iter_tvg_jobs": lambda: list(sc.iter_tvg_jobs([(good, False), (bad, False)])),
        "_pack_vtg": lambda: list(sc._pack_vtg([(4, None, [0], [np.array([0])])])),
        "tvg_first within": lambda: sc.tvg_first([0, 1], 2, within=[[0, 2], [3, 4]]),
        "expect": lambda: sc.expect([0, 4], True), "video_feat": lambda: sc.video_feat(4, False),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="video 4 was removed"):
            call()
    assert len(sc.plan_vtg(good)) == 1 and len(sc.plan_tvg(good)) == 1              # ... and the live ones are planned as ever
    for p in sc.plan_tvg(np.array([[j, i] for j in (0, 2, 3, 5) for i in range(3)])):
        assert p.labels.min() >= 0                                                  # a tombstone's -1 never reaches the engine
    g = GL.GalleryIndex(sc)
    assert sorted({k[0] for k in g.keys}) == [0, 2, 3, 5]                           # an index made now has no key of a tombstone
    with pytest.raises(ValueError, match="video 4 was removed"):
        list(g.iter_plans(bad))
    for req in ((0, [0, 4], None), SearchRequest(0, shortlist=2, within=[4, 5])):
        with pytest.raises(ValueError, match="video 4 was removed"):
            g._checked([req], True)
    with pytest.raises(ValueError, match="video 1 was removed"):
        g.prefilter([0], 2, within=[[1, 2]])


# ---- the whole-gallery planner
@pytest.mark.parametrize("chunk, max_tokens", [(2, 4096), (3, 64), (None, 4096)])
def test_the_gallery_plans_of_a_scorer_with_removals_are_those_of_the_survivors(chunk, max_tokens):
    dims, prob = SH._problem()
    keep = [0, 2, 3, 5]
    sc, fresh = _scorer(dims, prob, range(6), max_tokens=max_tokens), _scorer(dims, prob, keep, max_tokens=max_tokens)
    texts = [4, 0, 2]
    before = list(sc.iter_tvg_gallery(texts, chunk))
    sc.remove_videos([1, 4])
    got, want = list(sc.iter_tvg_gallery(texts, chunk)), list(fresh.iter_tvg_gallery(texts, chunk))
    assert len(got) == len(want) and (chunk is None or len(before) >= len(got))
    if max_tokens == 64:
        assert len(want) > 1                                                        # more than one call: the cuts fall where the survivors' fall
    for a, b in zip(got, want):
        slots = b.out_index[:, 0]
        b.out_index = ((slots // 4) * 6 + np.asarray(keep)[slots % 4])[:, None]     # the output slots through the index map
        assert GH.plan_difference(a, b) is None                                     # tokens, positions, own_start, rows, labels, feature rows
    assert sorted(int(o) for p in got for o in p.out_index[:, 0]) == sorted(q * 6 + j for q in range(3) for j in keep)
    assert sc.gallery_feats().shape == fresh.gallery_feats().shape


# ---- K and K0, and what ranks
def test_k_and_k0_are_clipped_to_the_live_videos_and_a_removed_column_is_never_ranked():
    s = SH._fake(GH._random_texts(3), n_videos=6, tvg=True)
    s._dead = frozenset({1, 4}); s.video[1] = s.video[4] = None
    g = GL.GalleryIndex(s)
    (r,) = g._checked([SearchRequest(0, shortlist=3, prefilter=50)], True)
    assert (r.shortlist, r.prefilter) == (3, 4)                                     # K0 through check_shortlist's one rule, over n_live
    assert GL.check_shortlist(3, 50, s.n_live) == (3, 4)
    row = np.array([0.5, np.nan, 0.75, 0.5, np.nan, -1.0], np.float32)
    order, val = GL.GalleryIndex._best(row, 6)
    assert order.tolist() == [2, 0, 3, 5] and val.tolist() == [0.75, 0.5, 0.5, -1.0]
    assert GL.GalleryIndex._best(row, 2)[0].tolist() == [2, 0]
    s.tvg_gallery = lambda texts: np.tile(row, (len(texts), 1))
    s.tvg = lambda pairs, cpn=False: np.array([0.25 * j for j, _ in pairs], np.float32)
    cand, stage = g.shortlist([0, 2], 9)
    assert cand.tolist() == [[2, 0, 3, 5]] * 2 and g.shortlist_stats["pairs"] == 2 * 4
    cand, stage = g.shortlist([0], 9, cpn=True, alpha=(1.0, 0.0))                   # the prior is looked up for the live videos alone
    assert sorted(cand[0].tolist()) == [0, 2, 3, 5] and np.all(np.isfinite(stage)) and sorted(k[3] for k in g._prior) == [0, 2, 3, 5]


def test_the_calibration_sample_draws_live_videos_only():
    s = SH._fake(GH._random_texts(5), n_videos=8)
    g = GL.GalleryIndex(s)
    whole = g._calibration_sample(None, 0, 5)
    s._dead = frozenset({2, 7}); s.video[2] = s.video[7] = None
    for first_stage in (None, np.random.RandomState(0).rand(7, 5).astype(np.float32)):      # (the last video joined at run time: no first-stage row)
        pairs, confirm, n_eval = g._calibration_sample(first_stage, 0, 5)
        assert not set(confirm[:, 0].tolist()) & {2, 7} and not set(pairs[:, 0].tolist()) & {2, 7} and len(pairs) and n_eval == 6 * 5
        assert confirm[:, 0].max() < 8 and confirm[:, 1].max() < 5
    assert set(whole[1][:, 0].tolist()) == set(range(8))


# ---- the indexes follow
def _shrink(s, gone):
    """Videos leave a fake scorer, as remove_videos would leave it."""
    s.video = [None if j in gone else v for j, v in enumerate(s.video)]
    s._dead = frozenset(s._dead | set(gone))
    s.vocab_version = s.vocab_version + 1


def test_follow_removed_drops_keys_stamps_slots_and_the_pending_reservations():
    s = SH._fake(LZ.TEXTS, n_videos=4)
    g = LZ._lazy(s, 3)
    _, d = LZ._pass(g, [[0, 0], [1, 0]])
    assert d["admitted"] == 2 and sorted(g.slot_of.values()) == [0, 1]
    pending = list(g.iter_plans(np.array([[1, 1], [2, 0]])))                       # planned, not run: video 2 has the free slot reserved
    assert g._pass is not None and [k[0] for k in g._pass.reserved] == [2]
    keys, stats = list(g.keys), g.stats.as_dict()
    _shrink(s, {1, 2})
    with pytest.raises(RuntimeError, match="plan again"):                           # the pending pass names what left: refused, not run
        g.run(pending[0])
    assert g.ran[-1] is not pending[0] and g._pass is None
    assert g.keys == [k for k in keys if k[0] in (0, 3)] and [k[0] for k in g.slot_of] == [0] and [k[0] for k in g._stamp] == [0]
    assert g.removed_stats == {"videos": 2, "slots_freed": 1, "records_forgotten": 0} and g.stats.as_dict() == stats
    plans, d = LZ._pass(g, [[0, 0], [3, 0]])                                       # the freed slot is there for the next miss
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (1, 1, 1, 0) and g.slot_of[g.keys[1]] == 1
    g._sync_videos()
    assert g.removed_stats["videos"] == 2                                           # nothing new: nothing counted twice
    # a text with a new split joins: the tombstones get no key under it either
    s.add_texts([SH._vtg_row([1, 2, 2], [3], [4, 4])])
    list(g.iter_plans(np.array([[0, 3]])))
    assert sorted({k[0] for k in g.keys}) == [0, 3] and len(g.keys) == 4


def test_an_eager_plan_from_before_a_removal_is_refused_too():
    s = SH._fake(LZ.TEXTS, n_videos=3)
    g = GH._gallery(s, {0: 0, 1: 1})
    SH._scoring(g)
    old = list(g.iter_plans(np.array([[1, 0]])))
    _shrink(s, {1})
    with pytest.raises(RuntimeError, match="plan again"):
        g.run(old[0])
    assert g._scores(np.array([[0, 1], [2, 0]])).tolist() == [float(SH._score(0, 1)), float(SH._score(2, 0))]


def test_a_freed_eager_slot_is_filled_with_the_next_video_that_joins_without_spare_slots():
    plen = 2 + NV + 1
    s = SH._fake(GH._random_texts(1), n_videos=3)
    g = GW._eager(s, 0)
    assert (len(g.slot_of), g.n_slots, g.fills) == (3, 3, [([0, 1, 2], 3 * plen)])
    cache = g.cache
    _shrink(s, {1})
    GW._grow(s, 1)
    p, = g.iter_plans(np.array([[0, 0], [2, 0], [3, 0]]))
    assert g.fills[1:] == [([1], plen)] and g.slot_of[g.keys[-1]] == 1 and g.keys[-1][0] == 3      # the new prefix went into the freed slot
    assert sorted(p.slots_used.tolist()) == [0, 1, 2] and p.prefix_tokens == 0 and g.cache is cache and cache.n_slots == 3
    assert g.removed_stats == {"videos": 1, "slots_freed": 1, "records_forgotten": 0}
    GW._grow(s, 1)                                                                  # one more: no slot is free, it stays in the batch
    p, = g.iter_plans(np.array([[4, 0]]))
    assert p.prefix_tokens == plen and len(g.fills) == 2


def test_host_tier_forget_returns_the_arena_space():
    cache = HT._Cache()
    cache.lens = {0: 8, 1: 8}
    tier = GL.HostTier(cache, 64, 1 * HT.RB, arena=HT._Mem(HT.RB), staging=HT._Mem(HT.RB), sync=lambda: None)
    assert tier.n_records == 1
    tier.spill(cache, [("a", 0, 0, None, (1, 0))])
    assert tier.has("a") and tier.plan_spills(["b"], {"a", "b"}) == []              # one record, held by a key the pass protects: "b" does not fit
    assert tier.forget("a") is True and not tier.has("a") and tier.forget("a") is False
    assert (tier.rec_of, tier.key_of, tier.len_of, tier.tickets, tier._stamp) == ({}, {}, {}, {}, {}) and tier.stats.dropped == 1
    assert tier.plan_spills(["b"], {"a", "b"}) == [("b", 0, None)]                  # ... and now it does, in the same place
    tier.spill(cache, [("b", 1, 0, None, (2, 0))])
    assert tier.has("b") and tier.rec_of == {"b": 0} and tier.stats.as_dict()["spilled"] == 2
    with pytest.raises(KeyError):
        tier.restore(cache, [("a", 0, (3, 0))])                                     # a forgotten key cannot be restored


def test_a_removed_videos_host_record_is_forgotten_and_never_restored():
    s = GH._fake_scorer(HT.TEXTS, n_videos=5)
    g = HT._tiered(s, 2, 4)
    HT._pass(g, [0, 1]); d = HT._pass(g, [2, 3])                                   # videos 0 and 1 are spilled
    assert d["spilled"] == 2 and {k[0] for k in g.host.rec_of} == {0, 1}
    _shrink(s, {0})
    d = HT._pass(g, [1, 4])                                                         # video 1 comes back by a copy; video 0's record is gone
    assert d["restored"] == 1 and {k[0] for k in g.host.rec_of} >= {1} and 0 not in {k[0] for k in g.host.rec_of}
    assert g.removed_stats == {"videos": 1, "slots_freed": 0, "records_forgotten": 1}
    with pytest.raises(ValueError, match="video 0 was removed"):
        HT._pass(g, [0])
    assert set(g.host.stats.as_dict()) == {"restored", "spilled", "dropped", "bytes_to_host", "bytes_from_host"}


def test_a_text_gallery_passes_the_call_on_and_refuses_a_removed_query_video():
    s = TH._fake_scorer([[9, 8, 7, 6, 5], [9, 8, 7]], n_videos=4)
    vg = GL.GalleryIndex(s)
    tg = TH._index(s, [0])
    tg.video_index = vg
    s.vtg_mode = None
    calls = []
    s.vtg = lambda pairs, cpn=False: calls.append(len(pairs)) or np.zeros(len(pairs), np.float32)
    tg.v2t_prior([0], [[0, 1]])
    keys, slots, prior = list(tg.keys), dict(tg.slot_of), dict(tg._prior)
    _shrink(s, {2})
    list(tg.iter_plans(np.array([[3, 0], [3, 1]])))
    assert tg.keys == keys and tg.slot_of == slots and 2 not in {k[0] for k in vg.keys} and vg.removed_stats["videos"] == 1
    tg.v2t_prior([3], [[0, 1]])
    assert tg._prior == prior and calls == [2]                                      # the (text, token count) memo stays valid
    for call in (lambda: tg.prefilter([2], 1), lambda: tg.shortlist([0, 2], 1), lambda: tg.rerank([2], [[0, 1]]), lambda: tg.rerank_shortlist([2], 1),
                 lambda: tg.v2t_prior([2], [[0]]), lambda: list(tg.iter_plans(np.array([[2, 0]])))):
        with pytest.raises(ValueError, match="video 2 was removed"):
            call()


# ---- the serve loop
def _server(tmp_path, argv=(), n_videos=4, content_hash=None):
    srv, passes, feats = GW._server(tmp_path, argv, n_videos=n_videos, content_hash=content_hash)
    srv.s._vfeat = {}
    return srv, passes, feats


_serve = GW._serve


@pytest.mark.parametrize("B", [1, 8])
def test_a_removal_is_a_barrier_and_replies_stay_in_arrival_order(tmp_path, B):
    srv, passes, feats = _server(tmp_path, content_hash=lambda t: t.numpy().tobytes())
    lines = [json.dumps({"id": 0, "caption": 1}),
             json.dumps({"id": 1, "caption": 2, "candidates": ["v0", "v1"]}),                      # in front of the removal: the old gallery
             json.dumps({"id": 2, "remove_video": "v1"}),
             json.dumps({"id": 3, "caption": 2, "candidates": ["v0", "v1"]}),                      # behind it: the id is gone
             json.dumps({"id": 4, "caption": 0}),
             json.dumps({"id": 5, "caption": 0, "candidate_idx": [0, 1]}),
             json.dumps({"id": 6, "add_video": {"vid": "v1", "features": feats("a.pth", 1.0)}}),   # the same id again: a new index
             json.dumps({"id": 7, "caption": 2, "candidates": ["v1", "v0"]}),
             json.dumps({"id": 8, "remove_video": "v1"}),
             json.dumps({"id": 9, "add_video": {"vid": "other", "features": feats("b.pth", 1.0)}}),   # the same content under another id: its digest left too
             json.dumps({"id": 10, "caption": 3})]
    out, summary = _serve(srv, lines, B)
    assert [x["id"] for x in out] == list(range(11))
    assert sorted(out[0]["videos"]) == ["v0", "v1", "v2", "v3"] and sorted(out[1]["videos"]) == ["v0", "v1"]
    assert out[2] == {"id": 2, "removed": "v1", "index": 1, "videos": 3}
    assert "unknown video id 'v1'" in out[3]["error"] and sorted(out[4]["videos"]) == ["v0", "v2", "v3"]
    assert out[5]["error"] == "video 1 was removed"
    assert out[6] == {"id": 6, "added": "v1", "index": 4, "videos": 4}                          # (the live count, as the removal answers)
    assert sorted(out[7]["videos"]) == ["v0", "v1"] and sorted(out[7]["scores"]) == sorted(float(SH._score(j, 2)) for j in (0, 4))
    assert out[8] == {"id": 8, "removed": "v1", "index": 4, "videos": 3}
    assert out[9] == {"id": 9, "added": "other", "index": 5, "videos": 4}
    assert sorted(out[10]["videos"]) == ["other", "v0", "v2", "v3"]
    assert summary == {"requests": 11, "batches": 11 if B == 1 else 2, "mean_batch": 1.0 if B == 1 else 5.5, "errors": 2, "texts_added": 0, "videos_added": 2,
                       "videos_removed": 2}
    assert srv.s.live.tolist() == [True, False, True, True, False, True] and "v1" not in srv.vid_at and srv.vid_at["other"] == 5
    assert srv.n_vid.tolist() == [NV, 0, NV, NV, 0, NV] and list(srv.content_of.values()) == ["other"]
    assert all(k[0] != 1 for p in passes[2:] for k in p) and {k[0] for k in passes[-1]} == {0, 2, 3, 5} and srv.gal.removed_stats["videos"] == 2
    if B == 8:
        assert len(passes) == 4                                                     # one pass on each side of every barrier that has queries: a batch never spans one


def test_every_bad_remove_video_request_gets_its_error_line_and_removes_nothing(tmp_path):
    srv, passes, feats = _server(tmp_path, n_videos=2)
    bad = [({"remove_video": "v9"}, "unknown video id 'v9'"), ({"remove_video": ["v0"]}, "remove_video takes the id"), ({"remove_video": {"vid": "v0"}}, "remove_video takes the id"),
           ({"remove_video": None}, "remove_video takes the id"), ({"remove_video": True}, "remove_video takes the id"), ({"remove_video": ""}, "remove_video takes the id"),
           ({"id": [1], "remove_video": "v0"}, "id must be a JSON scalar")]
    bad += [({"remove_video": "v0", k: 1}, "a remove_video request carries no query") for k in SR.Server.QUERY_KEYS]
    bad += [({"remove_video": "v0", "add_video": {"vid": "x", "features": "f"}}, "an add_video request carries no query")]
    lines = [json.dumps({"id": n, **a}) for n, (a, _) in enumerate(bad)]
    out, summary = _serve(srv, lines, 4)
    for x, (_, msg) in zip(out, bad):
        assert set(x) == {"id", "error"} and msg in x["error"], x
    assert srv.s.n_live == 2 and srv.s.vocab_version == 0 and "videos_removed" not in summary and summary["errors"] == len(lines) and passes == []
    out, summary = _serve(srv, [json.dumps({"id": 0, "remove_video": "v0"}), json.dumps({"id": 1, "remove_video": "v0"}), json.dumps({"id": 2, "remove_video": "v1"}),
                                json.dumps({"id": 3, "caption": 0})], 4)
    assert out[0] == {"id": 0, "removed": "v0", "index": 0, "videos": 1}
    assert "'v0' was removed already" in out[1]["error"] and "last video" in out[2]["error"] and out[3]["videos"] == ["v1"]      # ... and the process goes on
    assert summary["videos_removed"] == 1 and srv.s.n_live == 1


def test_the_length_check_does_not_read_a_tombstone(tmp_path):
    srv, _, _ = _server(tmp_path)
    srv.s.max_row_len = 2 + NV + 1 + 4
    srv.n_vid[1] = 100                                                              # video 1's prefix alone leaves no response token
    out, _ = _serve(srv, [json.dumps({"id": 0, "caption": 0}), json.dumps({"id": 1, "remove_video": "v1"}), json.dumps({"id": 2, "caption": 0})], 1)
    assert "tokenizer_model_max_length" in out[0]["error"] and sorted(out[2]["videos"]) == ["v0", "v2", "v3"]


def test_within_and_shortlist_requests_behind_a_removal(tmp_path):
    import test_within_host as WH
    srv, passes = WH._server(["--candidates", "tvg", "--shortlist", "3", "--prefilter", "40", "--resume", "x"])
    srv.s._vfeat, srv.s.tvg_video_labels, srv.s._upcoming, srv.s._upcoming_pos = {}, np.arange(len(srv.vids), dtype=np.int32), {}, {}
    N = len(srv.vids)
    out, _ = _serve(srv, [json.dumps({"id": 0, "remove_video": "v2"}), json.dumps({"id": 1, "caption": 0, "within": ["v1", "v2"]}),
                          json.dumps({"id": 2, "caption": 0, "within_idx": [1, 2]}), json.dumps({"id": 3, "caption": 0, "shortlist": 2, "within_idx": [1, 3]})], 8)
    assert out[0]["videos"] == N - 1 and "within: unknown video id 'v2'" in out[1]["error"] and out[2]["error"] == "video 2 was removed"
    assert sorted(out[3]["videos"]) == ["v1", "v3"] and out[3]["within"] == 2
    r = srv.parse(json.dumps({"id": 4, "caption": 1}))
    assert r["shortlist"] == 3 and r["prefilter"] == 40                             # (the request keeps what it asked for; the index clips K0 to the live videos)
    (c,) = srv.gal._checked([SearchRequest(r["text"], None, None, r["shortlist"], r["prefilter"])], True)
    assert c.prefilter == N - 1


def test_a_stream_without_removals_prints_the_lines_it_always_did(tmp_path):
    srv, _, feats = _server(tmp_path)
    out, summary = _serve(srv, [json.dumps({"id": 0, "caption": 1}), json.dumps({"id": 1, "add_video": {"vid": "n", "features": feats("a.pth")}})], 1)
    assert summary == {"requests": 2, "batches": 2, "mean_batch": 1.0, "errors": 0, "texts_added": 0, "videos_added": 1}
    g = srv.gal
    indexes = [("gallery", g)]
    stats = json.dumps(g.stats.as_dict())
    want = [f"gallery stats: {stats}", f"serve: {json.dumps(summary)}"]
    assert set(g.stats.as_dict()) == {"hits", "misses", "admitted", "evicted", "prefix_tokens_packed"}
    assert SR.report_lines(indexes, summary, g.shortlist_stats, g.prefilter_stats, g.within_stats, g.removed_stats) == want
    assert SR.report_lines(indexes, summary, g.shortlist_stats, g.prefilter_stats, g.within_stats) == want
    out, summary = _serve(srv, [json.dumps({"id": 2, "remove_video": "n"})], 1)
    assert summary["videos_removed"] == 1
    g._follow_removed()
    lines = SR.report_lines(indexes, summary, g.shortlist_stats, g.prefilter_stats, g.within_stats, g.removed_stats)
    assert lines[:1] == want[:1] and lines[1] == f"serve: {json.dumps(summary)}" and lines[2] == 'removed: {"videos": 1, "slots_freed": 0, "records_forgotten": 0}'
    assert len(lines) == 3


def test_default_candidates_with_and_without_live():
    row = np.array([0.1, 0.9, 0.5, 0.9, 0.2], np.float32)
    live = np.array([True, False, True, True, True, True])
    cand, fs = SR.default_candidates("iv2", row, 6, 3)
    assert cand.tolist() == [1, 3, 2] and fs.tolist() == row[[1, 3, 2]].tolist()
    cand, fs = SR.default_candidates("iv2", row, 6, 3, live=live)
    assert cand.tolist() == [3, 2, 4] and fs.tolist() == row[[3, 2, 4]].tolist()   # the top-k of the row among the live videos
    cand, fs = SR.default_candidates("all", row, 6, 3)
    assert cand.tolist() == list(range(6)) and fs.tolist() == row.tolist() + [0.0]
    cand, fs = SR.default_candidates("all", row, 6, 3, live=live)
    assert cand.tolist() == [0, 2, 3, 4, 5] and fs.tolist() == row[[0, 2, 3, 4]].tolist() + [0.0]
    cand, fs = SR.default_candidates("all", None, 6, 3, live=live)
    assert cand.tolist() == [0, 2, 3, 4, 5] and fs is None
    cand, fs = SR.default_candidates("all", None, 6, 3, live=np.ones(6, bool))
    assert cand.tolist() == list(range(6))
