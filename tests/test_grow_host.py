"""CPU: videos that join a scorer at run time (blim_amd/pair_scorer.py: PairScorer.add_videos; blim_amd/gallery.py: _PrefixIndex._sync_videos,
spare_slots, the vocabulary in the prior memo's state; blim_amd/search.py: the add_video request, --query_video, --gallery_spare) -- a video added later has the state
of a video given up front, the checks are all-or-nothing, indices and labels never move, the vocabulary is registered whole, the indexes append keys and leave their
slots and stats alone, the spare slots are handed out in key order, the prior memo is dropped, and an add is a barrier in the serve loop.  Fakes as in
tests/test_serve_host.py: no engine.  The GPU side is tests/test_grow_gpu.py."""
import json
import types

import numpy as np
import pytest
import torch

import test_gallery_host as GH
import test_host_logic as HL
import test_serve_host as SH
import test_text_gallery_host as TH
from blim_amd import gallery as GL
from blim_amd import retrieval_utils as RU
from blim_amd import search as SR
from blim_amd import synth
from blim_amd.pair_scorer import _clip_major_vocab

NV, H = GH.NV, GH.H


# ---- add_videos on a real PairScorer (planning only: tests/test_host_logic.py's fake model)
def _scorer(dims, prob, n_videos, vocab=True, engine=None):
    """All of the problem's texts over its first n_videos videos."""
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    T = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(T(prob.vtg_ids), T(prob.vtg_labels), T(prob.vtg_masks), tok)
    tvg = RU.padding_ids(T(prob.tvg_ids), T(prob.tvg_labels), T(prob.tvg_masks), tok)
    fake = HL._FakeModel(dims, prob.tvg_prefix_length)
    fake.engine = engine
    return RU.PairScorer(fake, vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video[:n_videos]],
                         torch.from_numpy(prob.video_vocab[:n_videos]) if vocab else None, torch.from_numpy(prob.tvg_video_labels[:n_videos]), dims.num_clips,
                         max_tokens=4096)


def _state(sc):
    return (len(sc.video), sc.tvg_video_labels.tolist(), sc.n_vocab, sc.vocab_version, None if sc.vocab_cm is None else sc.vocab_cm.clone())


def _same_state(a, b):
    return a[:4] == b[:4] and ((a[4] is None and b[4] is None) or torch.equal(a[4], b[4]))


def test_videos_added_later_have_the_state_of_videos_given_up_front():
    dims, prob = SH._problem()
    V = [torch.from_numpy(v) for v in prob.video]
    rows = torch.from_numpy(prob.video_vocab)
    whole = _scorer(dims, prob, 6)
    given = V[:3]
    late = _scorer(dims, prob, 3)
    late.video[:] = given                                                        # (the same objects: identity is checked below)
    assert late.vocab_version == whole.vocab_version == 1
    assert late.add_videos(V[3:5], rows[3:5]).tolist() == [3, 4] and late.vocab_version == 2
    assert late.add_videos(V[5:], rows[5:]).tolist() == [5] and late.vocab_version == 3
    assert len(given) == 3 and all(a is b for a, b in zip(late.video, V))        # the caller's list is left alone; existing indices never move
    assert late.tvg_video_labels.tolist() == whole.tvg_video_labels.tolist() == list(range(6)) and late.tvg_video_labels.dtype == np.int32
    assert late.n_vocab == whole.n_vocab == 6 and late.has_vocab
    assert late.vocab_cm.dtype == whole.vocab_cm.dtype and torch.equal(late.vocab_cm, whole.vocab_cm)
    assert torch.equal(late.vocab_cm, _clip_major_vocab(rows, "cpu", torch.float16))
    pairs = np.array([[j, i] for j in range(6) for i in (0, 3, 5)])
    for plan in ("plan_vtg", "plan_tvg"):
        got, want = getattr(late, plan)(pairs), getattr(whole, plan)(pairs)
        assert [GH.plan_difference(a, b) for a, b in zip(got, want)] == [None] * len(want) and len(got) == len(want)
    assert late.add_videos([]).tolist() == [] and late.vocab_version == 4 and late.n_vocab == 6


def test_the_default_vocabulary_row_is_the_clip_mean_in_float32():
    dims, prob = SH._problem()
    V = [torch.from_numpy(v).to(torch.float16) for v in prob.video]              # 16-bit features, as blim_amd.extract writes them
    late = _scorer(dims, prob, 3)
    late.add_videos(V[3:])
    want = torch.cat([torch.from_numpy(prob.video_vocab[:3]), torch.stack([v.float().mean(1) for v in V[3:]])])
    assert want.dtype == torch.float32 and torch.equal(late._vocab_src, want)
    assert torch.equal(late.vocab_cm, _clip_major_vocab(want, "cpu", torch.float16)) and late.tvg_video_labels.tolist() == list(range(6))


def test_the_vocabulary_is_registered_whole_with_the_engine():
    dims, prob = SH._problem()
    seen = []
    engine = types.SimpleNamespace(can_precise=True, _vocab_key=None)

    def set_video_vocab(v):
        seen.append(v.clone())
        engine._vocab_key = ("key", len(seen))
    engine.set_video_vocab = set_video_vocab
    late = _scorer(dims, prob, 4, engine=engine)
    assert late.split_tvg and late.vocab_cm is None and late._vocab_key == ("key", 1)
    rows = torch.from_numpy(prob.video_vocab)
    late.add_videos([torch.from_numpy(v) for v in prob.video[4:]], rows[4:])
    assert len(seen) == 2 and torch.equal(seen[0], rows[:4]) and torch.equal(seen[1], rows) and seen[1].dtype == torch.float32
    assert late._vocab_key == ("key", 2) and late.n_vocab == 6 and late.vocab_cm is None


def test_add_videos_is_all_or_nothing_and_raises_on_each_broken_rule():
    dims, prob = SH._problem()
    C, M = dims.num_clips, dims.mm_hidden_size
    sc = _scorer(dims, prob, 3)
    good, row = torch.from_numpy(prob.video[3]), torch.from_numpy(prob.video_vocab[3:4])
    before = _state(sc)
    bad = {
        "rank": torch.zeros((C, M)),
        "rank 4": torch.zeros((1, C, 8, M)),
        "clips": torch.zeros((C + 1, 8, M)),
        "width": torch.zeros((C, 8, M + 1)),
        "empty": torch.zeros((C, 0, M)),
        "not a tensor": [1.0, 2.0],
    }
    for name, v in bad.items():
        with pytest.raises(ValueError, match="add_videos"):
            sc.add_videos([good, v])                                            # the good video in front of it is not added either
        assert _same_state(_state(sc), before), name
    for name, r in {"count": torch.cat([row, row]), "clips": row[:, :-1], "width": row[:, :, :-1], "rank": row[0]}.items():
        with pytest.raises(ValueError, match="vocab_rows"):
            sc.add_videos([good], r)
        assert _same_state(_state(sc), before), name
    assert sc.add_videos([good], row).tolist() == [3]                            # ... and the good one alone joins
    # a scorer without a vocabulary (no TVG): no vocab_rows, no entry
    plain = _scorer(dims, prob, 3, vocab=False)
    with pytest.raises(ValueError, match="without a video vocabulary"):
        plain.add_videos([good], row)
    assert len(plain.video) == 3 and plain.vocab_version == 1
    assert plain.add_videos([good]).tolist() == [3] and plain.vocab_version == 2
    assert plain.n_vocab == 0 and plain.vocab_cm is None and plain._vocab_src is None and plain.tvg_video_labels.tolist() == [0, 1, 2, -1]
    # the clip-mean rule needs features of the vocabulary's width
    narrow = _scorer(dims, prob, 3)
    narrow._vocab_src = narrow._vocab_src[:, :, : M // 2]
    with pytest.raises(ValueError, match="clip-mean"):
        narrow.add_videos([good])
    assert len(narrow.video) == 3


# ---- the indexes follow the scorer (fake scorers)
def _grow(s, k):
    """k videos join a fake scorer, as add_videos would leave it."""
    s.video_feat = lambda j, tvg: torch.full((NV, H), float(j))
    s.video = s.video + [np.zeros((1, NV, 8), np.float32) for _ in range(k)]
    s.vocab_version = s.vocab_version + 1


def _key(j, pre, post):
    return (j, np.array(pre, np.int64).tobytes(), np.array(post, np.int64).tobytes())


def test_sync_videos_appends_one_key_per_new_video_and_known_split():
    s = SH._fake(GH._random_texts(4), n_videos=3)                                # two splits: ([1, 0], [2]) and ([1, 1], [2])
    g = GH._gallery(s, {0: 0, 3: 1})
    keys, slot_of, stats = list(g.keys), dict(g.slot_of), g.stats.as_dict()
    assert len(keys) == 6 and keys[:2] == [_key(0, [1, 0], [2]), _key(0, [1, 1], [2])]      # video-major for what the index was made over
    _grow(s, 2)
    p, = g.iter_plans(np.array([[3, 2], [1, 1]]))                                # a pass is planned: the keys follow first
    assert g.keys[:6] == keys and g.keys[6:] == [_key(3, [1, 0], [2]), _key(3, [1, 1], [2]), _key(4, [1, 0], [2]), _key(4, [1, 1], [2])]      # new videos outermost
    assert g.slot_of == slot_of and g.stats.as_dict() == stats and g._n_videos == 5
    assert p.pfx_slot.numpy().tolist() == [1, -1, -1]                            # (video 1, split 1) reads its slot; the new video's prefix is in the batch
    assert g._needs(np.array([[4, 1], [0, 0], [3, 2]])) == [keys[0], g.keys[6], g.keys[9]]
    g._sync_videos()
    assert len(g.keys) == 10                                                     # nothing new: nothing appended
    # a text with a new split AND a video join before the next pass: the split meets the videos the keys covered, the video every split -- each key once
    s.add_texts([SH._vtg_row([1, 2, 2], [3], [4, 4])])
    _grow(s, 1)
    list(g.iter_plans(np.array([[5, 4]])))
    new = g.keys[10:]
    assert new[:5] == [_key(j, [1, 2, 2], [3]) for j in range(5)] and new[5:] == [_key(5, [1, 0], [2]), _key(5, [1, 1], [2]), _key(5, [1, 2, 2], [3])]
    assert len(set(g.keys)) == len(g.keys) == 18 and g.slot_of == slot_of
    fresh = GL.GalleryIndex(s)                                                   # an index made now: the same keys, video-major
    assert sorted(fresh.keys) == sorted(g.keys) and list(fresh.splits) == list(g.splits)


def test_a_text_gallery_has_no_key_per_video_and_its_video_index_follows():
    s = TH._fake_scorer([[9, 8, 7, 6, 5], [9, 8, 7]], n_videos=3)
    vg = GL.GalleryIndex(s)
    tg = TH._index(s, [0])
    tg.video_index = vg
    keys, n = list(tg.keys), len(vg.keys)
    s.video = s.video + [np.zeros((1, 5, 8), np.float32)]
    s.tvg_video_labels = np.append(s.tvg_video_labels, 103).astype(np.int32)
    s.video_feat = lambda j, tvg: torch.full((3, TH.H), float(j))
    p, = tg.iter_plans(np.array([[3, 0], [3, 1]]))
    assert tg.keys == keys and tg._n_videos == 4 and len(vg.keys) == n + 1 and vg.keys[-1][0] == 3
    assert p.labels.numpy().tolist() == [103, 103] and list(p.slots_used) == [0]


# ---- spare slots (an eager index, built over fakes)
class _Cache:
    def __init__(self, n_slots, max_len):
        self.n_slots, self.max_len, self.lens = n_slots, max_len, {}

    def slot_len(self, slot):
        return self.lens[slot]

    def close(self):
        pass


def _eager(s, spare, budget=None):
    """A GalleryIndex built through build() over a fake engine: 100 bytes a slot; the fill's packed calls are recorded, not run."""
    s.engine = types.SimpleNamespace(dtype="f16", weights_version=0, prefix_cache_bytes=lambda n, L, comp: 100 * n, prefix_cache=lambda n, L, comp: _Cache(n, L))
    g = GL.GalleryIndex(s, budget_bytes=budget, spare_slots=spare, log=lambda msg: None)
    g.fills = []

    def fill_call(st, slots):
        g.fills.append((list(slots), st.n_tok))
        for sl, ln in zip(slots, st.seq_len):
            g.cache.lens[sl] = ln
    g._fill_call = fill_call
    return g.build()


def test_spare_slots_are_filled_in_key_order_and_the_rest_stay_in_the_batch():
    plen = 2 + NV + 1
    pairs = np.array([[j, 0] for j in range(6)])
    for spare, cached in ((3, [3, 4, 5]), (1, [3]), (0, [])):
        s = SH._fake(GH._random_texts(1), n_videos=3)                            # one split
        g = _eager(s, spare)
        assert (len(g.keys), len(g.slot_of), g.n_slots, g.cache.n_slots) == (3, 3, 3 + spare, 3 + spare) and g.fills == [([0, 1, 2], 3 * plen)]
        stats = g.stats.as_dict()
        _grow(s, 3)
        p, = g.iter_plans(pairs)
        assert len(g.keys) == 6 and len(g.slot_of) == 3 + len(cached) and g.stats.as_dict() == stats
        assert g.fills[1:] == ([(list(range(3, 3 + len(cached))), len(cached) * plen)] if cached else [])      # ONE packed fill per sync
        assert [g.slot_of.get(g.keys[j], -1) for j in range(6)] == [0, 1, 2] + [j if j in cached else -1 for j in (3, 4, 5)]
        assert sorted(p.slots_used.tolist()) == [0, 1, 2] + cached and p.prefix_tokens == (3 - len(cached)) * plen
        _grow(s, 1)                                                              # one more: no slot is free any more, nothing is filled, no cache is resized
        list(g.iter_plans(pairs))
        assert len(g.keys) == 7 and len(g.slot_of) == 3 + len(cached) and g.cache.n_slots == 3 + spare and len(g.fills) == 1 + (1 if cached else 0)


def test_spare_slots_count_against_the_budget_and_a_longer_prefix_is_not_filled():
    s = SH._fake(GH._random_texts(1), n_videos=6)
    g = _eager(s, 3, budget=1000)
    assert (len(g.slot_of), g.n_slots) == (6, 9)
    g = _eager(s, 3, budget=700)                                                 # seven slots: three stay free, four videos are planned
    assert (len(g.slot_of), g.n_slots) == (4, 7) and sorted(g.slot_of.values()) == [0, 1, 2, 3]
    g = _eager(s, 3, budget=250)                                                 # two slots in all: both spare
    assert (len(g.slot_of), g.n_slots, g.cache.n_slots) == (0, 2, 2)
    g = _eager(s, 2)
    s.video_feat = lambda j, tvg: torch.full((int(np.prod(s.video[int(j)].shape[:2])), H), float(j))
    s.video = s.video + [np.zeros((1, NV + 40, 8), np.float32), np.zeros((1, NV, 8), np.float32)]      # the first is longer than a slot (32-aligned)
    s.vocab_version += 1
    list(g.iter_plans(np.array([[6, 0], [7, 0]])))
    assert g.keys[6] not in g.slot_of and g.slot_of[g.keys[7]] == 6 and g.fills[-1] == ([6], 2 + NV + 1)
    with pytest.raises(ValueError, match="spare_slots"):
        GL.GalleryIndex(s, fill="lazy", spare_slots=1)
    with pytest.raises(ValueError, match="spare_slots"):
        GL.GalleryIndex(s, spare_slots=-1)


def test_a_lazy_index_admits_an_added_videos_prefix_on_demand():
    import test_lazy_gallery_host as LZ
    s = SH._fake(LZ.TEXTS, n_videos=2)
    g = LZ._lazy(s, 2)
    _, d = LZ._pass(g, [[0, 0]])
    assert d["admitted"] == 1
    slot_of = dict(g.slot_of)
    _grow(s, 2)
    plans, d = LZ._pass(g, [[2, 0], [0, 1]])                                     # video 0 hits; the new video is a miss, admitted into the free slot
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (1, 1, 1, 0) and g.slot_of == {**slot_of, g.keys[2]: 1}
    _, d = LZ._pass(g, [[3, 0], [2, 2]])                                         # the next one takes the least recently used slot the pass does not need
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (1, 1, 1, 1) and {k[0] for k in g.slot_of} == {2, 3}


# ---- staleness: the vocabulary is part of what a TVG value was computed under
def test_prior_memo_is_dropped_when_the_vocabulary_grows():
    s = GH._fake_scorer([([1, 2], [3], [5, 6])], n_videos=2)
    s.tvg_split = [np.array([9, 8, 7], np.int64)]
    s.m.tvg_prefix_length = 2
    s.engine.weights_version = 0
    s.tvg_mode = "full"
    calls = []

    def tvg(pairs, cpn=False):
        calls.append(len(pairs))
        return np.full(len(pairs), float(len(s.video)), np.float32)
    s.tvg = tvg
    g = GL.GalleryIndex(s)
    cand = np.array([[0, 1]])
    before = g._tvg_state()
    assert g._t2v_prior([0], cand).tolist() == [[2.0, 2.0]]
    assert g._t2v_prior([0], cand).tolist() == [[2.0, 2.0]] and calls == [2] and g._prior_state == before      # memoised
    _grow(s, 1)
    assert g._tvg_state() != before and g._tvg_state()[:3] == before[:3]
    assert g._t2v_prior([0], cand).tolist() == [[3.0, 3.0]] and calls == [2, 2] and g._prior_state == g._tvg_state()
    assert g._t2v_prior([0], np.array([[2, 0]])).tolist() == [[3.0, 3.0]] and calls == [2, 2, 1]               # the new video: one pair more, the rest memoised


def test_the_v2t_prior_survives_the_growth():
    s = TH._fake_scorer([[9, 8, 7, 6, 5], [9, 8, 7]], n_videos=3)
    s.vtg_mode = None
    calls = []
    s.vtg = lambda pairs, cpn=False: calls.append(len(pairs)) or np.zeros(len(pairs), np.float32)
    tg = GL.TextGalleryIndex(s)
    tg.v2t_prior([0], [[0, 1]])
    s.video = s.video + [np.zeros((1, 5, 8), np.float32)]
    s.vocab_version = 1
    tg.v2t_prior([3], [[0, 1]])                                                  # the same token count: the (text, count) entries answer
    assert calls == [2] and len(tg._prior) == 2


# ---- the serve loop
def _server(tmp_path, argv=(), n_videos=4, content_hash=None):
    srv, passes = SH._server(argv, n_videos=n_videos)
    s = srv.s
    s.num_clips, s.tvg_video_labels, s.vocab_version = 1, np.arange(n_videos, dtype=np.int32), 0
    s.video_feat = lambda j, tvg: torch.full((NV, H), float(j))
    srv.content_hash = content_hash

    def feats(name, value=0.0, shape=(1, NV, 8)):
        path = tmp_path / name
        torch.save(torch.full(shape, float(value)), str(path))
        return str(path)
    return srv, passes, feats


def _serve(srv, lines, B):
    out = []
    summary = SR.serve(iter(lines), out.append, srv, batch_queries=B, batch_wait_ms=60000.0)
    return [json.loads(x) for x in out], summary


@pytest.mark.parametrize("B", [1, 5])
def test_an_add_is_a_barrier_and_replies_stay_in_arrival_order(tmp_path, B):
    srv, passes, feats = _server(tmp_path)
    lines = [json.dumps({"id": 0, "caption": 1}),
             json.dumps({"id": 1, "caption": 2, "candidates": ["v0", "new"]}),                     # in front of the add: the id is not known yet
             json.dumps({"id": 2, "add_video": {"vid": "new", "features": feats("a.pth", 1.0)}}),
             json.dumps({"id": 3, "caption": 2, "candidates": ["v0", "new"]}),
             json.dumps({"id": 4, "caption": 0})]
    out, summary = _serve(srv, lines, B)
    assert [x["id"] for x in out] == [0, 1, 2, 3, 4]
    assert "unknown video id" in out[1]["error"]
    assert out[2] == {"id": 2, "added": "new", "index": 4, "videos": 5}
    assert sorted(out[0]["videos"]) == ["v0", "v1", "v2", "v3"]                                    # scored against the old gallery ...
    assert sorted(out[3]["videos"]) == ["new", "v0"] and sorted(out[4]["videos"]) == ["new", "v0", "v1", "v2", "v3"]      # ... and against the new
    assert sorted(out[3]["scores"]) == sorted(float(SH._score(j, 2)) for j in (0, 4))
    assert len(passes) == (3 if B == 1 else 2)                                                      # five lines at once: two passes, one on each side of the add
    assert summary == {"requests": 5, "batches": 5 if B == 1 else 1, "mean_batch": 1.0 if B == 1 else 5.0, "errors": 1, "texts_added": 0, "videos_added": 1}
    assert len(srv.s.video) == 5 and srv.vids[-1] == "new" and srv.vid_at["new"] == 4 and srv.n_vid.tolist() == [NV] * 5
    assert srv.s.vocab_version == 1 and len(srv.gal.keys) == 2 * 5


def test_a_bad_add_video_request_gets_its_error_line_and_adds_nothing(tmp_path):
    srv, passes, feats = _server(tmp_path, content_hash=lambda t: t.numpy().tobytes())
    garbage = tmp_path / "garbage.pth"
    garbage.write_bytes(b"not a tensor file")
    listed = tmp_path / "list.pth"
    torch.save([1, 2, 3], str(listed))
    good = feats("good.pth", 2.0)
    bad = [
        ({"vid": "v1", "features": good}, "already in the gallery"),
        ({"vid": "x", "features": str(tmp_path / "missing.pth")}, "cannot read"),
        ({"vid": "x", "features": str(garbage)}, "cannot read"),
        ({"vid": "x", "features": str(listed)}, "floating-point tensor"),
        ({"vid": "x", "features": feats("rank.pth", shape=(NV, 8))}, "rank"),
        ({"vid": "x", "features": feats("clips.pth", shape=(2, NV, 8))}, "clips"),
        ({"vid": "x", "features": feats("width.pth", shape=(1, NV, 9))}, "width"),
        ({"vid": "x", "features": 7}, "path"),
        ({"vid": ["x"], "features": good}, "vid must be"),
        ({"vid": "x"}, "add_video takes"),
        ("x", "add_video takes"),
    ]
    lines = [json.dumps({"id": n, "add_video": a}) for n, (a, _) in enumerate(bad)]
    lines.append(json.dumps({"id": "q", "add_video": {"vid": "x", "features": good}, "caption": 0}))
    out, summary = _serve(srv, lines, 4)
    for x, (_, msg) in zip(out, bad):
        assert set(x) == {"id", "error"} and msg in x["error"], x
    assert "carries no query" in out[-1]["error"]
    assert len(srv.s.video) == 4 and len(srv.vids) == 4 and srv.s.vocab_version == 0 and "videos_added" not in summary and passes == []
    assert summary["errors"] == summary["requests"] == len(lines)
    # the process goes on: the good file joins, its content does not join twice under another name, another content does
    out, summary = _serve(srv, [json.dumps({"id": 0, "add_video": {"vid": "x", "features": good}}),
                                json.dumps({"id": 1, "add_video": {"vid": "y", "features": feats("copy.pth", 2.0)}}),
                                json.dumps({"id": 2, "add_video": {"vid": 7, "features": feats("other.pth", 3.0)}}),
                                json.dumps({"id": 3, "caption": 0, "candidates": [7, "x"]})], 4)
    assert out[0] == {"id": 0, "added": "x", "index": 4, "videos": 5} and "those of video 'x'" in out[1]["error"]
    assert out[2] == {"id": 2, "added": "7", "index": 5, "videos": 6} and sorted(out[3]["videos"]) == ["7", "x"]
    assert summary["videos_added"] == 2 and srv.s.vocab_version == 2


def test_a_run_time_video_has_a_zero_first_stage_term(tmp_path):
    srv, _, feats = _server(tmp_path, ["--c", "0.5", "0", "0.5", "0"])
    out, _ = _serve(srv, [json.dumps({"id": 0, "add_video": {"vid": "new", "features": feats("a.pth")}}), json.dumps({"id": 1, "caption": 2})], 1)
    row = srv.t2v_iv2[2]
    blended = 0.5 * (0.5 * np.array([SH._score(j, 2) for j in range(5)]) + 0.5 * np.zeros(5)) + 0.5 * np.concatenate([row, [0.0]]).astype(np.float32)
    o = np.argsort(-blended, kind="stable")
    assert out[1]["videos"] == [srv.vids[j] for j in o] and out[1]["scores"] == [float(x) for x in blended[o]]


# ---- the command's refusals
def test_check_args_for_outside_videos_and_spare_slots():
    p = SR.get_args_parser()
    with pytest.raises(SystemExit, match="--direction v2t"):
        SR.check_args(p.parse_args(["--query_ids", "0", "--query_video", "a.pth"]))
    with pytest.raises(SystemExit, match="iv2"):                                  # refused by name: no first-stage row
        SR.check_args(p.parse_args(["--direction", "v2t", "--query_video", "a.pth"]))
    with pytest.raises(SystemExit, match="--query_video"):
        SR.check_args(p.parse_args(["--serve", "--query_video", "a.pth"]))
    with pytest.raises(SystemExit, match="t2v"):                                  # as before
        SR.check_args(p.parse_args(["--serve", "--direction", "v2t", "--query_video", "a.pth", "--candidates", "all"]))
    with pytest.raises(SystemExit, match="needs --video_ids"):                    # as before
        SR.check_args(p.parse_args(["--direction", "v2t"]))
    with pytest.raises(SystemExit, match="--resume"):
        SR.check_args(p.parse_args(["--direction", "v2t", "--query_video", "a.pth", "--candidates", "tvg"]))
    a = p.parse_args(["--direction", "v2t", "--query_video", "a.pth", "b.pth", "--candidates", "all"])
    SR.check_args(a)
    assert a.query_video == ["a.pth", "b.pth"] and a.video_ids == [] and a.gallery_spare == 0
    SR.check_args(p.parse_args(["--direction", "v2t", "--query_video", "a.pth", "--video_ids", "1", "--candidates", "tvg", "--resume", "ft.pth"]))
    with pytest.raises(SystemExit, match="gallery_spare"):
        SR.check_args(p.parse_args(["--serve", "--gallery_spare", "-1"]))
    with pytest.raises(SystemExit, match="gallery_spare"):
        SR.check_args(p.parse_args(["--serve", "--gallery_spare", "4", "--gallery_fill", "lazy"]))
    SR.check_args(p.parse_args(["--serve", "--gallery_spare", "4"]))
    for argv, msg in ((["--dtype", "f8", "--serve"], "f8"), (["--shard", "2", "0", "--serve"], "shard")):
        with pytest.raises(SystemExit, match=msg):
            SR.check_args(p.parse_args(argv))
