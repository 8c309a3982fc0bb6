"""CPU: the caption prefilter's host side (blim_amd/gallery.py: TextGalleryIndex.prefilter and the K0 of shortlist / rerank_shortlist; blim_amd/search.py:
--caption_prefilter) -- ONE stage-0 pass for all query videos, the resident keys through PairScorer.tvg_first_cached (their slots in key order, cols = the videos'
vocabulary entries), exactly the keys without a slot through PairScorer.tvg_first(..., k=1, full=True), the per-key values fanned out over texts that share a
prompt, Engine.rank_rows over the result; K0 clipped and refused by check_shortlist; nothing counted as a hit or a miss; prefilter=None leaves shortlist's calls as
they were.  Fakes as in tests/test_prefilter_host.py: no engine.  The GPU side is tests/test_caption_prefilter_gpu.py."""
import json
import types

import numpy as np
import pytest
import torch

import test_serve_host as SH
import test_shortlist_host as SL
from blim_amd import gallery as GL
from blim_amd import search as SR

N = SL.N                 # videos
T = 7                    # texts; 5 has text 1's caption prompt
LABELS = np.array([3, 0, 5, 1, 4, 2], np.int32)        # video j is vocabulary entry LABELS[j]


def _val(entry, prompt):
    """The fake's clip-0 value of (vocabulary entry, caption prompt): ties between prompts on purpose."""
    return np.float32(-((int(entry) * 3 + int(prompt[-1]) * 5) % 7) / 4.0)


def _fake(resident=(0, 2, 3), cache=True):
    """-> (scorer, index): `resident` = the keys (by position) that have a slot -- key n in slot 10 + n."""
    s = SL._fake(n_videos=N, n_texts=T)
    s.tvg_split[5] = s.tvg_split[1].copy()
    s.tvg_video_labels = LABELS
    s.first_calls, s.cached_calls, s.rank_calls = [], [], []
    tg = GL.TextGalleryIndex(s)
    assert len(tg.keys) == T - 1
    tg._state = tg._mode_state()                       # built: nothing to fill
    tg.slot_of = {tg.keys[n]: 10 + n for n in resident}
    tg.cache = object() if cache else None

    def tvg_first(texts, k, cpn=False, alpha=0.0, full=False):
        texts = np.asarray(texts, np.int64).reshape(-1)
        s._need_tvg(texts)
        s.first_calls.append((texts.tolist(), int(k), bool(cpn), bool(full)))
        lp = np.array([[_val(LABELS[j], s.tvg_split[i]) for j in range(N)] for i in texts], np.float32).reshape(len(texts), N)      # by VIDEO index
        idx = np.stack([np.argsort(-r, kind="stable")[:k] for r in lp]).astype(np.int64)
        return idx, np.take_along_axis(lp, idx, 1), lp

    def tvg_first_cached(cache_, slots, cols, chunk_rows=0):
        assert cache_ is tg.cache and cols.dtype == torch.int32
        s.cached_calls.append((list(slots), cols.tolist(), chunk_rows))
        key_of = {sl: k for k, sl in tg.slot_of.items()}
        return torch.tensor([[_val(c, np.frombuffer(key_of[sl], np.int64)) for sl in slots] for c in cols.tolist()], dtype=torch.float32).reshape(len(cols), len(slots))

    def rank_rows(values, k):
        s.rank_calls.append((tuple(values.shape), int(k)))
        v = values.numpy()
        idx = np.stack([np.argsort(-r, kind="stable")[:k] for r in v])
        return torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(np.take_along_axis(v, idx, 1))
    s.tvg_first, s.tvg_first_cached, s.engine.rank_rows = tvg_first, tvg_first_cached, rank_rows
    return s, tg


def _want(s, videos, k0):
    rows = np.array([[_val(LABELS[v], s.tvg_split[i]) for i in range(len(s.tvg_split))] for v in videos], np.float32)
    idx = np.stack([np.argsort(-r, kind="stable")[:k0] for r in rows])
    return idx, np.take_along_axis(rows, idx, 1)


def test_one_stage_0_pass_serves_all_videos_and_the_fallback_takes_exactly_the_keys_without_a_slot():
    s, tg = _fake(resident=(0, 2, 3))
    videos = [4, 1, 4]
    cand, val = tg.prefilter(videos, 4)
    assert s.cached_calls == [([10, 12, 13], LABELS[videos].tolist(), 0)]          # ONE cached call: the resident keys' slots in key order, the videos' entries
    assert s.first_calls == [([1, 4, 6], 1, False, True)]                          # ONE decoded call: the first text of each key without a slot (keys 1, 4, 5)
    assert s.rank_calls == [((3, T), 4)]
    idx, v = _want(s, videos, 4)
    assert cand.dtype == np.int64 and val.dtype == np.float32 and np.array_equal(cand, idx) and np.array_equal(val, v)
    assert tg.prefilter_stats == {"queries": 3, "passes": 1, "rows": T - 1, "kept": 12}
    assert tg.stats.as_dict() == dict.fromkeys(tg.stats.as_dict(), 0) and tg._stamp == {} and tg._n_pass == 0      # no hit, no miss, no admission, no stamp, no pass
    tg.prefilter([2], 3, chunk_rows=256)
    assert s.cached_calls[-1] == ([10, 12, 13], [int(LABELS[2])], 256)


def test_every_key_resident_or_none():
    s, tg = _fake(resident=range(T - 1))
    cand, val = tg.prefilter([0, 5], T)
    assert s.first_calls == [] and len(s.cached_calls) == 1 and s.cached_calls[0][0] == [10 + n for n in range(T - 1)]
    assert np.array_equal(cand, _want(s, [0, 5], T)[0])
    for s, tg in (_fake(resident=()), _fake(resident=(), cache=False)):
        cand, val = tg.prefilter([0, 5], T)
        assert s.cached_calls == [] and s.first_calls == [([0, 1, 2, 3, 4, 6], 1, False, True)]
        idx, v = _want(s, [0, 5], T)
        assert np.array_equal(cand, idx) and np.array_equal(val, v)


def test_texts_that_share_a_prompt_share_a_value_and_the_lower_index_goes_first():
    for resident in ((1,), ()):                                                    # the shared key from its slot, and from the decoded path
        s, tg = _fake(resident=resident)
        cand, val = tg.prefilter([3, 0], T)
        for q in range(2):
            row = dict(zip(cand[q].tolist(), val[q].tolist()))
            assert row[1] == row[5] and cand[q].tolist().index(1) < cand[q].tolist().index(5)
            assert np.array_equal(cand[q], _want(s, [3, 0], T)[0][q])


def test_k0_is_clipped_and_refused_by_the_one_rule(monkeypatch):
    s, tg = _fake()
    asked = []
    rule = GL.check_shortlist
    monkeypatch.setattr(GL, "check_shortlist", lambda K, K0, n: asked.append((K, K0, n)) or rule(K, K0, n))
    cand, val = tg.prefilter([2], 100)
    assert cand.shape == val.shape == (1, T) and s.rank_calls[-1] == ((1, T), T) and asked == [(None, 100, T)]          # clipped to the texts
    assert tg.prefilter([], 3)[0].shape == (0, 3) and tg.prefilter([], 3)[1].dtype == np.float32 and len(s.rank_calls) == 1
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="positive integer"):
            tg.prefilter([1], bad)
    with pytest.raises(ValueError, match="below the shortlist's K = 3"):
        tg.shortlist([1], 3, prefilter=2)
    passes = tg.prefilter_stats["passes"]
    monkeypatch.setattr(GL, "TVG_RANK_MAX_K", 4)
    with pytest.raises(ValueError, match="BLIM_TVG_RANK_MAX_K"):
        tg.prefilter([1], 100)                                                     # clipped to 7 texts, still above
    with pytest.raises(ValueError, match="BLIM_TVG_RANK_MAX_K"):
        tg.shortlist([1], 2, prefilter=5)
    monkeypatch.undo()
    no_tvg, = s.add_texts([SH._vtg_row([1, 1], [2, 2], [3])]).tolist()
    with pytest.raises(ValueError, match=f"text {no_tvg} "):                       # _need_tvg's error: every text is ranked
        tg.prefilter([0], 2)
    assert tg.prefilter_stats["passes"] == passes                                  # a refused call counts nothing


def test_shortlist_with_a_k0_scores_the_survivors_only_and_none_leaves_its_calls_as_they_were(monkeypatch):
    s, tg = _fake()
    asked = []

    def tvg_pairs(pairs):
        asked.append(np.asarray(pairs).tolist())
        return np.array([SL._stage(j, i) for j, i in pairs], np.float32)
    tg.tvg_pairs = tvg_pairs
    tg.vtg_pairs = lambda pairs: np.array([SH._score(j, i) for j, i in pairs], np.float32)
    rules = []
    rule = GL.check_shortlist
    monkeypatch.setattr(GL, "check_shortlist", lambda K, K0, n: rules.append((K, K0, n)) or rule(K, K0, n))
    # prefilter=None: one pass per video over every text, no stage 0, the rule asked as before
    cand, stage = tg.shortlist([4, 1], 3)
    assert asked == [[[4, i] for i in range(T)], [[1, i] for i in range(T)]] and rules == [(3, None, T)]
    assert s.cached_calls == [] and s.first_calls == [] and s.rank_calls == [] and tg.prefilter_stats["passes"] == 0
    for q, v in enumerate((4, 1)):
        row = np.array([SL._stage(v, i) for i in range(T)])
        o = np.argsort(-row, kind="stable")[:3]
        assert cand[q].tolist() == o.tolist() and stage[q].tolist() == row[o].tolist()
    # with K0: ONE stage-0 pass for both videos, then each video's pass over its survivors, ascending
    del asked[:], rules[:]
    cand, stage = tg.shortlist([4, 1], 2, prefilter=4)
    kept = _want(s, [4, 1], 4)[0]
    assert len(s.cached_calls) == 1 and len(s.first_calls) == 1 and tg.prefilter_stats == {"queries": 2, "passes": 1, "rows": T - 1, "kept": 8}
    assert asked == [[[4, i] for i in sorted(kept[0].tolist())], [[1, i] for i in sorted(kept[1].tolist())]] and rules[0] == (2, 4, T)
    for q, v in enumerate((4, 1)):
        texts = np.sort(kept[q])
        row = np.array([SL._stage(v, i) for i in texts])
        o = np.argsort(-row, kind="stable")[:2]
        assert cand[q].tolist() == texts[o].tolist() and stage[q].tolist() == row[o].tolist()
    # K0 = every text: the unprefiltered shortlist
    a, b = tg.shortlist([4, 1], 3, prefilter=T + 3), tg.shortlist([4, 1], 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # rerank_shortlist hands the K0 on, and without one calls shortlist as it did
    seen = []
    short = tg.shortlist
    tg.shortlist = lambda *a, **k: seen.append((a[1:], k)) or short(*a, **k)
    c = (0.6, 0.5, 0.7, 0.5)
    o1, b1 = tg.rerank_shortlist([4], 2, c=c, prefilter=4)
    o2, b2 = tg.rerank_shortlist([4], 2, c=c)
    assert seen == [((2, 4), {}), ((2,), {})]
    want_o, want_b = tg.rerank([4], cand[:1], c=c, finetuned=True)                 # the fake's tvg_pairs is deterministic: the reused term is the recomputed one
    assert np.array_equal(o1, want_o) and np.array_equal(b1, want_b) and o2.shape == (1, 2)


# ---- the command
@pytest.mark.parametrize("argv,msg", [
    (["--query_ids", "0", "--candidates", "tvg", "--caption_prefilter", "8", "--resume", "x"], "--caption_prefilter narrows the captions a query video ranks"),
    (["--direction", "v2t", "--video_ids", "0", "--caption_prefilter", "8", "--resume", "x"], "--caption_prefilter narrows the captions before --candidates tvg"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "all", "--caption_prefilter", "8", "--resume", "x"], "--caption_prefilter narrows the captions before"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--caption_prefilter", "0", "--resume", "x"], "--caption_prefilter must be at least --shortlist"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--shortlist", "16", "--caption_prefilter", "8", "--resume", "x"], "--caption_prefilter must be at least --shortlist"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--topk", "12", "--caption_prefilter", "8", "--resume", "x"], "--caption_prefilter must be at least --shortlist"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--caption_prefilter", "8"], "--candidates tvg needs a fine-tuned checkpoint"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--prefilter", "8", "--resume", "x"], "v2t has no prefilter"),       # the existing refusal ...
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--prefilter", "8", "--resume", "x"], "--caption_prefilter K0"),     # ... now points at the flag
])
def test_check_args_refusals(argv, msg):
    with pytest.raises(SystemExit, match=msg):
        SR.check_args(SR.get_args_parser().parse_args(argv))


def test_check_args_accepts_the_flag():
    p = SR.get_args_parser()
    assert p.parse_args(["--query_ids", "0"]).caption_prefilter is None
    for argv in (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--resume", "x", "--caption_prefilter", "64"],
                 ["--direction", "v2t", "--video_ids", "0", "3", "--candidates", "tvg", "--resume", "x", "--shortlist", "16", "--caption_prefilter", "16"],
                 ["--direction", "v2t", "--query_video", "a.pt", "--candidates", "tvg", "--resume", "x", "--topk", "4", "--caption_prefilter", "128"]):
        SR.check_args(p.parse_args(argv))


def test_the_command_prints_the_k0_and_the_closing_line():
    vids = [f"v{j}" for j in range(N)]
    runs = {}
    for K0 in (None, 4):
        s, tg = _fake()
        tg.tvg_pairs = lambda pairs: np.array([SL._stage(j, i) for j, i in pairs], np.float32)
        tg.vtg_pairs = lambda pairs: np.array([SH._score(j, i) for j, i in pairs], np.float32)
        args = SR.get_args_parser().parse_args(["--direction", "v2t", "--video_ids", "4", "1", "--candidates", "tvg", "--resume", "x", "--topk", "2", "--shortlist", "3"]
                                               + ([] if K0 is None else ["--caption_prefilter", str(K0)]))
        SR.check_args(args)
        got = []
        short = SR.run_v2t(tg, vids, None, args, got.append)
        runs[K0] = ([json.loads(x) for x in got], short, SR.report_lines([("text gallery", tg)], None, short, tg.prefilter_stats), s, tg)
    plain, short, lines, s, _ = runs[None]
    assert all(set(x) == {"query", "texts", "scores", "shortlisted"} for x in plain) and short == {"queries": 2, "passes": 2, "pairs": 2 * T}
    assert not any(line.startswith("prefilter:") for line in lines) and s.cached_calls == [] and s.first_calls == []
    out, short, lines, s, tg = runs[4]
    assert [x["query"] for x in out] == ["video:v4", "video:v1"] and all(x["prefiltered"] == 4 and x["shortlisted"] == 3 and len(x["texts"]) == 2 for x in out)
    assert short == {"queries": 2, "passes": 2, "pairs": 8}
    assert json.loads([line for line in lines if line.startswith("prefilter: ")][0][len("prefilter: "):]) == {"queries": 2, "stage0_passes": 2, "stage0_rows": 2 * (T - 1), "kept": 8}
    for x, v in zip(out, (4, 1)):
        order, blended = tg.rerank_shortlist([v], 3, c=SR.get_args_parser().parse_args([]).c or [1.0, 0.0, 1.0, 1.0], prefilter=4)
        assert x["texts"] == order[0, :2].tolist() and x["scores"] == [float(b) for b in blended[0, :2]]
