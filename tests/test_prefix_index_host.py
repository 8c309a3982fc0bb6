"""CPU: the split of cache residency (blim_amd/prefix_index.py) from search policy (blim_amd/gallery.py), and the rules it states once -- the liveness reads of
PairScorer (`live_videos()`, `removed`) behind the one-armed `_calibration_sample` and `_stage1`, `_PrefixIndex._take` in its two callers (an admission and a
restore), the id-list rule of the serve loop by table, and the import surface of blim_amd.gallery.  The pinned numbers and error lines are those of the commit
before the split.  Fakes as in tests/test_lazy_gallery_host.py, tests/test_host_tier_host.py and tests/test_serve_host.py: no engine."""
import ast
import json

import numpy as np
import pytest

import test_gallery_host as GH
import test_host_tier_host as HT
import test_remove_host as RM
import test_serve_host as SH
from blim_amd import gallery as GL
from blim_amd import prefix_index as PI
from blim_amd import search as SR
from blim_amd.calibration import calibration_pairs


# ---- 1. the unified arms with nothing removed
@pytest.fixture(scope="module")
def whole():
    """A gallery of 8 videos and 5 texts, every video live."""
    s = SH._fake(GH._random_texts(5), n_videos=8, tvg=True)
    return s, GL.GalleryIndex(s)


def test_liveness_has_one_statement_on_the_scorer(whole):
    s, _ = whole
    assert s.live_videos().tolist() == list(range(8)) and s.live_videos().dtype == np.int64 and s.removed == frozenset()
    t = SH._fake(GH._random_texts(1), n_videos=5)
    RM._shrink(t, {3, 1})                                                           # (the storage the existing tests set: both reads derive from it)
    assert t.live_videos().tolist() == [0, 2, 4] and t.removed == frozenset({1, 3}) and isinstance(t.removed, frozenset)
    assert t.live.tolist() == [True, False, True, False, True] and t.n_live == 3


@pytest.mark.parametrize("rows", [None, 8, 6])
def test_the_calibration_sample_over_the_live_videos_is_the_plain_formula_when_all_are_live(whole, rows):
    _, g = whole
    fs = None if rows is None else np.random.RandomState(rows).rand(rows, 5).astype(np.float32)     # (6 rows: two videos joined at run time)
    pairs, confirm, n_eval = g._calibration_sample(fs, 3, 5)
    if fs is None:
        flat = np.random.RandomState(3).choice(8 * 5, size=min(2048, 8 * 5), replace=False)
        both = np.stack([flat // 5, flat % 5], axis=1).astype(np.int64)
        want = both[:256], both
    else:
        want = calibration_pairs(fs, 16, n_queries=32, per_query=8), calibration_pairs(fs, 16, n_queries=256, per_query=8)
    assert np.array_equal(pairs, want[0]) and np.array_equal(confirm, want[1]) and pairs.dtype == want[0].dtype and confirm.dtype == want[1].dtype
    assert n_eval == 8 * 5


def test_stage1_over_the_live_videos_is_the_plain_expression_when_all_are_live(whole):
    s, g = whole
    row = np.array([0.5, -2.0, 0.75, 0.5, 1.25, -1.0, 0.0, 3.5], np.float32)
    s.tvg_gallery = lambda texts: np.tile(row, (len(texts), 1))
    s.tvg = lambda pairs, cpn=False: np.array([0.25 * j for j, _ in pairs], np.float32)
    texts, alpha = [0, 2, 0], (0.5, 0.0)
    stage = np.tile(row, (3, 1))
    before = dict(g.shortlist_stats)
    got = g._stage1(texts, True, alpha)
    want = stage - alpha[0] * np.tile(0.25 * np.arange(8), (3, 1))                  # the prior of (text, video j) is the canned 0.25 j, a float64 memo
    assert np.array_equal(got, want) and got.dtype == want.dtype == np.float64
    assert {k: g.shortlist_stats[k] - before[k] for k in before} == {"queries": 3, "passes": 1, "pairs": 2 * 8}
    plain = g._stage1(texts, False, alpha)                                          # without cpn: the stage as tvg_gallery gave it
    assert np.array_equal(plain, stage) and plain.dtype == np.float32
    assert g.shortlist_stats["passes"] == before["passes"] + 2


# ---- 2. _take in its two callers
def test_take_serves_an_admission_and_a_restore_and_only_the_admission_counts_as_one():
    g = HT._tiered(GH._fake_scorer(HT.TEXTS, n_videos=3), 2, 1)                     # 2 slots over 3 videos, a host tier of one record

    def state():
        return ({k[0]: sl for k, sl in g.slot_of.items()}, {k[0]: st for k, st in g._stamp.items()}, g.stats.evicted, g.stats.admitted, g.host.stats.restored)
    HT._pass(g, [0, 1])                                                             # two free slots
    assert state() == ({0: 0, 1: 1}, {0: (1, 0), 1: (1, 1)}, 0, 2, 0)
    HT._pass(g, [2])                                                                # an admission that evicts: video 0, the least recently used, is spilled
    assert state() == ({1: 1, 2: 0}, {1: (1, 1), 2: (2, 0)}, 1, 3, 0) and {k[0] for k in g.host.rec_of} == {0}
    HT._pass(g, [0])                                                                # a restore that evicts: video 1 finds no record to take and is lost
    assert state() == ({2: 0, 0: 1}, {2: (2, 0), 0: (3, 0)}, 2, 3, 1)
    assert g.stats.as_dict() == {"hits": 1, "misses": 3, "admitted": 3, "evicted": 2, "prefix_tokens_packed": 3 * HT.PLEN}


def test_free_slots_and_fits():
    g = HT._tiered(GH._fake_scorer(HT.TEXTS, n_videos=3), 3, 0)
    assert g._free_slots() == [0, 1, 2] and all(g._fits(k) for k in g.keys)         # (a cache that names no length takes every key)
    HT._pass(g, [1])
    g.slot_of[g.keys[2]] = 2
    assert g._free_slots() == [1]
    g.cache.max_len = HT.PLEN
    assert g._fits(g.keys[0])
    g.cache.max_len = HT.PLEN - 1
    assert not g._fits(g.keys[0])


# ---- 3. the id-list rule, by table
@pytest.fixture(scope="module")
def server():
    srv, _ = SH._server(n_videos=6, finetuned=True)
    RM._shrink(srv.s, {1, 4})
    return srv


@pytest.mark.parametrize("ids, idx, word, opens", [("candidates", "candidate_idx", "candidate", ""), ("within", "within_idx", "within", "within: ")])
def test_each_broken_rule_of_an_id_list_gets_the_error_line_it_always_got(server, ids, idx, word, opens):
    more = {} if ids == "candidates" else {"shortlist": 2}
    table = [({ids: ["v0", "nope", "v2"]}, f"{opens}unknown video id 'nope'"),
             ({idx: [0, 6]}, f"{idx} must hold indices in 0 .. 5"), ({idx: [0, -1]}, f"{idx} must hold indices in 0 .. 5"),
             ({idx: [0, True]}, f"{idx} must hold indices in 0 .. 5"), ({idx: [0, 1.0]}, f"{idx} must hold indices in 0 .. 5"),
             ({idx: [0, 1, 2]}, "video 1 was removed"),
             ({idx: [4, 0, 1]}, "video 4 was removed"),                             # two removed indices, descending: the first in the request's order
             ({ids: ["v0", "v2", "v0"]}, f"the {word} list names a video twice"), ({idx: [2, 0, 2]}, f"the {word} list names a video twice")]
    for req, line in table:
        with pytest.raises(SR.BadRequest) as e:
            server.parse(json.dumps({"id": 7, "caption": 0, **more, **req}))
        assert str(e.value) == line and e.value.id == 7, req
    with pytest.raises(ValueError, match="video 1 was removed"):                    # ... while the scorer's own rule names the lowest
        server.s._need_live([4, 0, 1])
    good = server.parse(json.dumps({"id": 7, "caption": 0, **more, idx: [5, 0, 2]}))
    assert (good["cand"].tolist() == [5, 0, 2]) if ids == "candidates" else (good["within"].tolist() == [0, 2, 5])


def test_the_id_map_names_the_first_video_of_an_id(tmp_path):
    assert SR.video_index_of(["a", 7, "a", "7", "b"]) == {"a": 0, "7": 1, "b": 4}
    f = tmp_path / "ids.txt"
    f.write_text("b\n\na\n")
    assert SR.read_within_ids(str(f), ["a", 7, "a", "7", "b"]).tolist() == [0, 4]


# ---- 4. the import surface
MOVED = ("SLOT_ALIGN", "slot_plan", "cache_bytes", "GalleryStats", "HostStats", "_pinned_bytes", "_device_bytes", "_device_sync", "HostTier", "_Pass", "_PrefixIndex")
STAYED = ("check_shortlist", "check_within", "TVG_RANK_MAX_K", "SearchRequest", "request_pairs", "grid_pairs", "GalleryIndex", "TextGalleryIndex", "SEG_MAX")


def test_gallery_still_offers_every_name_and_the_moved_ones_are_the_same_objects():
    for name in MOVED:
        assert getattr(GL, name) is getattr(PI, name), name
    for name in STAYED:                                                             # with MOVED: every name tests/ and tools/ take from blim_amd.gallery
        assert hasattr(GL, name), name
    for name in ("check_shortlist", "check_within", "SearchRequest", "request_pairs", "grid_pairs", "GalleryIndex", "TextGalleryIndex"):
        assert getattr(GL, name).__module__ == "blim_amd.gallery" and not hasattr(PI, name), name
    assert issubclass(GL.GalleryIndex, PI._PrefixIndex) and issubclass(GL.TextGalleryIndex, PI._PrefixIndex)


def test_the_dependency_runs_one_way():
    tree = ast.parse(open(PI.__file__).read())
    froms = [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)] + [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    assert froms and not [m for m in froms if "gallery" in m or "search" in m]


def test_an_index_sees_a_replaced_rule_of_the_gallery_module(whole, monkeypatch):
    s, g = whole
    s.tvg_gallery = lambda texts: np.zeros((len(texts), 8), np.float32)
    asked, rule = [], GL.check_shortlist
    monkeypatch.setattr(GL, "check_shortlist", lambda K, K0, n: asked.append((K, K0, n)) or rule(K, K0, n))
    assert g.shortlist([0], 2)[0].tolist() == [[0, 1]] and asked == [(2, None, 8)]
    monkeypatch.setattr(GL, "TVG_RANK_MAX_K", 4)
    with pytest.raises(ValueError, match="above the rank kernel's limit of 4"):
        g._checked([GL.SearchRequest(0, shortlist=2, prefilter=5)], True)
