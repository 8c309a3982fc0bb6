"""CPU: texts that join a scorer at run time, and the serve loop (blim_amd/pair_scorer.py: PairScorer.add_texts; blim_amd/gallery.py: the index follows its scorer,
GalleryIndex.rerank_requests; blim_amd/search.py: --serve) -- a text added later has the state of a text given up front, the checks are all-or-nothing, the index
appends keys and leaves its slots and stats alone, ragged requests are one pass with rerank()'s results per request, a lazy index counts that pass exactly, and the
serve loop answers in arrival order, one error line per bad request, whatever the batch size.  Fakes as in tests/test_gallery_host.py and
tests/test_lazy_gallery_host.py: no engine.  The GPU side is tests/test_serve_gpu.py."""
import json
import types

import numpy as np
import pytest
import torch

import test_gallery_host as GH
import test_host_logic as HL
import test_lazy_gallery_host as LZ
from blim_amd import gallery as GL
from blim_amd import retrieval_utils as RU
from blim_amd import search as SR
from blim_amd import synth
from blim_amd.synth import IGNORE_INDEX, IMAGE_TOKEN_INDEX

NV, PLEN = GH.NV, LZ.PLEN
IMG = IMAGE_TOKEN_INDEX


# ---- add_texts on a real PairScorer (planning only: tests/test_host_logic.py's fake model)
def _problem(n=6):
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)
    return dims, synth.make_problem(5, n, dims, tok_per_clip=8, text_len=(3, 9))


def _unpadded(ids, labels, masks):
    return [(np.asarray(i)[np.asarray(m) != 0], np.asarray(l)[np.asarray(m) != 0]) for i, l, m in zip(ids, labels, masks)]


def _scorer(dims, prob, texts, limit=None):
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    T = lambda rows: [torch.from_numpy(rows[i]) for i in texts]
    vtg = RU.padding_ids(T(prob.vtg_ids), T(prob.vtg_labels), T(prob.vtg_masks), tok)
    tvg = RU.padding_ids(T(prob.tvg_ids), T(prob.tvg_labels), T(prob.tvg_masks), tok)
    fake = HL._FakeModel(dims, prob.tvg_prefix_length)
    fake.tokenizer_model_max_length = limit
    return RU.PairScorer(fake, vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video], None,
                         torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=4096)


def _same_texts(a, b):
    assert len(a.vtg_split) == len(b.vtg_split) == len(a.tvg_split) == len(b.tvg_split) == len(a.vtg_rows) == len(b.vtg_rows) == len(a.tvg_rows) == len(b.tvg_rows)
    for x, y in zip(a.vtg_split, b.vtg_split):
        assert all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(x, y))
    for x, y in zip(a.tvg_split, b.tvg_split):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    for rows_a, rows_b in ((a.vtg_rows, b.vtg_rows), (a.tvg_rows, b.tvg_rows)):
        for x, y in zip(rows_a, rows_b):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_texts_added_later_have_the_state_of_texts_given_up_front():
    dims, prob = _problem()
    whole = _scorer(dims, prob, range(6))
    late = _scorer(dims, prob, range(3))
    vtg_rows = _unpadded(prob.vtg_ids, prob.vtg_labels, prob.vtg_masks)
    tvg_rows = _unpadded(prob.tvg_ids, prob.tvg_labels, prob.tvg_masks)
    old = [tuple(a.copy() for a in s) for s in late.vtg_split]
    assert late.add_texts(vtg_rows[3:5], tvg_rows[3:5]).tolist() == [3, 4]
    assert late.add_texts(vtg_rows[5:], tvg_rows[5:]).tolist() == [5]
    assert late.add_texts([], []).tolist() == []
    _same_texts(late, whole)
    assert all(np.array_equal(p, q) for x, y in zip(old, late.vtg_split) for p, q in zip(x, y))       # existing indices never move
    pairs = np.array([[j, i] for j in range(6) for i in (0, 3, 5)])
    for plan in ("plan_vtg", "plan_tvg"):
        got, want = getattr(late, plan)(pairs), getattr(whole, plan)(pairs)
        assert [GH.plan_difference(a, b) for a, b in zip(got, want)] == [None] * len(want) and len(got) == len(want)


def _broken(vtg_row, tvg_row):
    ids, lab = vtg_row
    at = int(np.nonzero(ids == IMG)[0][0])
    tids, tlab = tvg_row
    first = int(np.argmax(tlab != IGNORE_INDEX))
    swapped = tids.copy(); swapped[first] = 17
    swapped_lab = tlab.copy(); swapped_lab[first] = 17
    return {
        "no placeholder": ((np.delete(ids, at), np.delete(lab, at)), tvg_row),
        "two placeholders": ((np.insert(ids, at, IMG), np.insert(lab, at, IGNORE_INDEX)), tvg_row),
        "TVG response": (vtg_row, (swapped, swapped_lab)),
        "lengths": ((ids, lab[:-1]), tvg_row),
    }


def test_add_texts_is_all_or_nothing_and_raises_on_each_broken_rule():
    dims, prob = _problem()
    sc = _scorer(dims, prob, range(3))
    vtg_rows = _unpadded(prob.vtg_ids, prob.vtg_labels, prob.vtg_masks)
    tvg_rows = _unpadded(prob.tvg_ids, prob.tvg_labels, prob.tvg_masks)
    for name, (bad_v, bad_t) in _broken(vtg_rows[4], tvg_rows[4]).items():
        with pytest.raises(ValueError):
            sc.add_texts([vtg_rows[3], bad_v], [tvg_rows[3], bad_t])                # the good row in front of it is not added either
        assert len(sc.vtg_split) == len(sc.tvg_split) == len(sc.vtg_rows) == len(sc.tvg_rows) == 3, name
    with pytest.raises(ValueError, match="TVG rows"):
        sc.add_texts(vtg_rows[3:5], tvg_rows[3:4])
    longest = max(len(r[0]) for r in tvg_rows)
    lim = _scorer(dims, prob, range(3), limit=longest - 1 + dims.num_clips)          # every TVG row fits ...
    lim.add_texts(vtg_rows[3:], tvg_rows[3:])
    lim = _scorer(dims, prob, [i for i in range(6) if len(tvg_rows[i][0]) < longest], limit=longest - 2 + dims.num_clips)
    n = len(lim.vtg_split)
    i_long = [i for i in range(6) if len(tvg_rows[i][0]) == longest][0]
    with pytest.raises(ValueError, match="tokenizer_model_max_length"):             # ... and one token less cuts the longest
        lim.add_texts([vtg_rows[i_long]], [tvg_rows[i_long]])
    assert len(lim.vtg_split) == len(lim.tvg_rows) == n
    assert lim.add_texts([vtg_rows[i_long]]).tolist() == [n]                         # without its TVG row the rule does not apply


def test_a_text_without_a_tvg_row_has_no_tvg_score():
    dims, prob = _problem()
    sc = _scorer(dims, prob, range(3))
    vtg_rows = _unpadded(prob.vtg_ids, prob.vtg_labels, prob.vtg_masks)
    i, = sc.add_texts([vtg_rows[4]]).tolist()
    assert i == 3 and sc.tvg_split[3] is None and sc.tvg_rows[3] is None
    assert len(sc.plan_vtg(np.array([[0, 3], [1, 0]]))) == 1
    for cpn in (False, True):
        with pytest.raises(ValueError, match="text 3 "):
            sc.plan_tvg(np.array([[0, 0], [1, 3]]), cpn)
    assert len(sc.plan_tvg(np.array([[0, 0], [1, 2]]))) == 1
    with pytest.raises(ValueError, match="text 3 "):
        list(GL.TextGalleryIndex(sc).iter_plans(np.array([[1, 3]])))


# ---- the index follows the scorer (fake scorers: texts = [(pre, post, response)])
def _vtg_row(pre, post, resp):
    ids = np.array(list(pre) + [IMG] + list(post) + list(resp), np.int64)
    lab = np.array([IGNORE_INDEX] * (len(pre) + 1 + len(post)) + list(resp), np.int64)
    return ids, lab


def _tvg_row(prompt):
    return np.array(list(prompt) + [IMG, 9], np.int64), np.array([IGNORE_INDEX] * len(prompt) + [IMG, 9], np.int64)


def _fake(texts, n_videos=4, max_row_len=None, tvg=False):
    """tests/test_gallery_host.py's fake scorer with what add_texts and rerank_requests read besides: rows, caption prompts, a TVG score per pair."""
    s = GH._fake_scorer(texts, n_videos=n_videos, max_row_len=max_row_len)
    s.vtg_rows = [_vtg_row(*t) for t in texts]
    s.tvg_rows = [_tvg_row([5, 6, i]) for i in range(len(texts))]
    s.tvg_split = [np.array([5, 6, i], np.int64) for i in range(len(texts))]
    s.num_clips = 4
    s.engine.weights_version = 0
    s.m.tvg_prefix_length = 2
    s.tvg_mode = "full"
    s.tvg_calls = []

    def tvg_scores(pairs, cpn=False):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        s._need_tvg(pairs[:, 1])
        s.tvg_calls.append((len(pairs), bool(cpn)))
        return np.array([_score(j, i) / (3.0 if cpn else 2.0) for j, i in pairs], np.float32)
    s.tvg = tvg_scores
    return s


def _score(j, i):
    return np.float32(-(((int(j) * 7 + int(i) * 3) % 11) + 0.25 * int(i)) / 3.0)


def _scoring(g):
    """The index scores through a fake engine call: pair (video j, text i) -> _score(j, i).  -> the list of the passes' key lists (one per _begin_pass)."""
    passes, now = [], {}
    begin, scores = g._begin_pass, g._scores

    def begin_pass(need):
        passes.append(list(need))
        return begin(need)

    def scores_(pairs):
        now["pairs"] = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        return scores(pairs)

    def run(plan, cache):
        for _, slot, _, ln, _ in ([] if plan.admits is None else plan.admits.tolist()):
            cache.lens[slot] = ln
        return torch.tensor([_score(*now["pairs"][int(o[0])]) for o in plan.out_index])
    g._begin_pass, g._scores, g.s.run = begin_pass, scores_, run
    g._state = g._mode_state()                     # built: nothing to refill
    return passes


def test_an_eager_index_appends_keys_and_serves_a_new_split_in_the_batch():
    s = _fake(LZ.TEXTS, n_videos=3)
    g = GH._gallery(s, {0: 0, 1: 1})                                             # videos 0 and 1 cached
    keys, slot_of, stats, split_id = list(g.keys), dict(g.slot_of), g.stats.as_dict(), g._split_id.copy()
    known, = s.add_texts([_vtg_row([1, 2], [3], [4, 4, 4])], [_tvg_row([5, 6, 7])]).tolist()
    p, = g.iter_plans(np.array([[0, known], [2, known]]))
    assert g.keys == keys and len(g.splits) == 1                                  # a known (pre, post): no new key
    assert p.pfx_slot.numpy().tolist() == [0, -1, -1] and list(p.slots_used) == [0]      # video 0 from its slot, video 2 in the batch
    new, = s.add_texts([_vtg_row([1, 2, 2], [3], [4, 4])]).tolist()
    p, = g.iter_plans(np.array([[0, new], [1, 0]]))
    assert g.keys[:len(keys)] == keys and len(g.keys) == len(keys) + 3 and len(g.splits) == 2
    assert g.keys[len(keys):] == [(j, np.array([1, 2, 2], np.int64).tobytes(), np.array([3], np.int64).tobytes()) for j in range(3)]
    assert p.pfx_slot.numpy().tolist() == [-1, -1, 1]                             # the new split's prefix is packed; text 0 over video 1 still reads slot 1
    assert g.slot_of == slot_of and g.stats.as_dict() == stats and g.admit is None
    assert g._split_id.tolist() == split_id.tolist() + [0, 1]
    assert g._needs(np.array([[1, new], [1, 0], [0, known]])) == [keys[0], keys[1], g.keys[len(keys) + 1]]
    fresh = GL.GalleryIndex(s)                                                    # an index made now: the same splits, video-major keys
    assert list(fresh.splits) == list(g.splits) and sorted(fresh.keys) == sorted(g.keys) and fresh._split_id.tolist() == g._split_id.tolist()


def test_a_lazy_index_admits_an_added_texts_prefix_on_demand():
    s = _fake(LZ.TEXTS, n_videos=3)
    g = LZ._lazy(s, 3)
    _, d = LZ._pass(g, [[0, 0]])
    assert d["admitted"] == 1
    slot_of, stamp = dict(g.slot_of), dict(g._stamp)
    new, = s.add_texts([_vtg_row([1, 2, 2], [3], [4, 4])]).tolist()
    plans, d = LZ._pass(g, [[0, new], [0, 1]])                                    # video 0 under the old split hits; under the new one it is a miss, admitted
    key = (0, np.array([1, 2, 2], np.int64).tobytes(), np.array([3], np.int64).tobytes())
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (1, 1, 1, 0)
    assert plans[0].admits[:, 1].tolist() == [1] and plans[0].admits[0, 3] == PLEN + 1
    assert g.slot_of == {**slot_of, key: 1} and set(stamp) < set(g._stamp)
    _, d = LZ._pass(g, [[0, new]])
    assert (d["hits"], d["misses"]) == (1, 0)
    g.cache.max_len = PLEN + 1                                                    # a split whose prefix is longer than a slot stays in the batch
    longer, = s.add_texts([_vtg_row([1, 2, 2, 2], [3], [4, 4])]).tolist()
    plans, d = LZ._pass(g, [[1, longer], [1, 0]])
    assert (d["misses"], d["admitted"]) == (2, 1) and plans[0].admits[0, 3] == PLEN


# ---- rerank_requests
C_BLEND = (0.6, 0.5, 0.7, 0.5)


def _requests(rng, texts, n_videos, ks):
    out = []
    for n, k in enumerate(ks):
        cand = rng.permutation(n_videos)[:k]
        out.append((int(texts[n % len(texts)]), cand, rng.rand(k).astype(np.float32) if n % 2 else None))
    return out


@pytest.mark.parametrize("finetuned", [False, True])
def test_ragged_requests_are_one_pass_with_reranks_results(finetuned):
    s = _fake(GH._random_texts(5), n_videos=6)
    g = GH._gallery(s, {0: 0, 2: 1, 5: 2})
    passes = _scoring(g)
    late, = s.add_texts([_vtg_row([1, 1], [2, 2], [3, 4])], [_tvg_row([5, 6, 9])]).tolist()
    reqs = _requests(np.random.RandomState(3), [0, 3, late, 4], 6, [1, 3, 6, 2, 1, 5])
    more = dict(cpn=True, alpha=(0.8, 0.3), c=C_BLEND, finetuned=finetuned)
    got = g.rerank_requests(reqs, **more)
    assert len(passes) == 1 and len(got) == len(reqs)                            # ONE pass over the concatenated pairs
    assert s.tvg_calls == ([(sum(len(c) for _, c, _ in reqs), False), (s.tvg_calls[1][0], True)] if finetuned else [])
    for (t, cand, fs), (order, blended) in zip(reqs, got):
        o1, b1 = g.rerank([t], cand[None], first_stage=None if fs is None else fs[None], **more)
        assert order.shape == blended.shape == (len(cand),)
        assert np.array_equal(order, o1[0]) and np.array_equal(blended, b1[0]) and blended.dtype == b1.dtype
        ql = np.array([_score(j, t) for j in cand])
        want = C_BLEND[2] * (C_BLEND[0] * ql + (1 - C_BLEND[0]) * (np.array([(_score(j, t) / np.float32(2.0)) - 0.8 * float(_score(j, t) / np.float32(3.0)) for j in cand])
                                                                     if finetuned else 0.0)) + (1 - C_BLEND[2]) * (0.0 if fs is None else fs)
        assert np.allclose(np.sort(want)[::-1], blended, rtol=1e-6, atol=0) and sorted(order.tolist()) == sorted(cand.tolist())
    assert g.rerank_requests([]) == []
    with pytest.raises(ValueError, match="no candidates"):
        g.rerank_requests([(0, np.zeros(0, np.int64), None)])
    if finetuned:
        no_tvg, = s.add_texts([_vtg_row([1, 1], [2, 2], [3])]).tolist()
        with pytest.raises(ValueError, match=f"text {no_tvg} "):
            g.rerank_requests([(0, [1, 2], None), (no_tvg, [3], None)], **more)


def test_a_lazy_index_counts_a_batch_of_requests_as_one_pass():
    s = _fake(LZ.TEXTS, n_videos=5)
    g = LZ._lazy(s, 2)
    passes = _scoring(g)
    delta = lambda reqs: LZ_delta(g, lambda: g.rerank_requests(reqs))
    batch = [(0, [0, 1], None), (2, [1, 2], None), (1, [2], None)]                # three keys, two slots
    got, d = delta(batch)
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"], d["prefix_tokens_packed"]) == (0, 3, 2, 0, 3 * PLEN)
    assert LZ._resident(g) == {0, 1} and len(passes) == 1
    again, d = delta(batch)                                                       # both slots pinned by the pass: video 2 stays in the batch
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"], d["prefix_tokens_packed"]) == (2, 1, 0, 0, PLEN)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, again))
    _, d = delta([(0, [3], None), (1, [1, 4], None)])                             # video 0 is the least recently used key the pass does not need
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (1, 2, 1, 1) and LZ._resident(g) == {1, 3}
    assert len(passes) == 3
    for (t, cand, _), (order, blended) in zip(batch, got):
        assert sorted(blended.tolist(), reverse=True) == blended.tolist() and sorted(blended.tolist()) == sorted(float(_score(j, t)) for j in cand)


def LZ_delta(g, fn):
    before = g.stats.as_dict()
    out = fn()
    return out, {k: v - before[k] for k, v in g.stats.as_dict().items()}


# ---- the serve loop
def _server(argv=(), n_videos=6, finetuned=False, max_row_len=None, build_rows=None):
    s = _fake(GH._random_texts(4), n_videos=n_videos, max_row_len=max_row_len)
    g = GH._gallery(s, {0: 0, 3: 1})
    passes = _scoring(g)
    args = SR.get_args_parser().parse_args(["--serve", "--candidates", "all"] + list(argv))
    SR.check_args(args)
    iv2 = np.random.RandomState(1).rand(4, n_videos).astype(np.float32)
    srv = SR.Server(g, [f"v{j}" for j in range(n_videos)], 4, iv2, args, finetuned=finetuned, build_rows=build_rows)
    return srv, passes


ROWS_A = {"vtg_ids": [1, 1, IMG, 2, 3, 4], "vtg_labels": [IGNORE_INDEX] * 4 + [3, 4], "tvg_ids": [5, 6, IMG, 9], "tvg_labels": [IGNORE_INDEX] * 2 + [IMG, 9]}
ROWS_B = {"vtg_ids": [1, 0, IMG, 2, 7], "vtg_labels": [IGNORE_INDEX] * 4 + [7]}                              # no TVG row
LINES = [
    json.dumps({"id": 0, "caption": 1}),
    json.dumps({"id": "a", "rows": ROWS_A, "candidate_idx": [4, 0, 2], "first_stage": [0.1, 0.9, 0.5]}),
    "{\"id\": 2, \"caption\": ",                                                                                 # malformed
    json.dumps({"id": 3, "caption": 2, "candidates": ["v1", "v9"]}),                                              # unknown id
    json.dumps({"id": 4, "rows": ROWS_B, "candidates": ["v5"]}),
    json.dumps({"id": 5, "caption": 0, "candidate_idx": []}),                                                     # empty
    json.dumps({"id": 6, "caption": 0, "candidate_idx": [1, 2, 1]}),                                              # duplicate
    json.dumps({"id": 7, "rows": ROWS_A, "topk": 2}),                                                             # the same text again
    json.dumps({"id": 8, "text": "a dog runs"}),                                                                  # no tokenizer here
    json.dumps({"id": 9.5, "caption": 3, "candidates": ["v2", "v0", "v4", "v1"], "topk": 3}),
    json.dumps({"id": 10, "rows": dict(ROWS_B, vtg_ids=[1, 0, 2, 7], vtg_labels=[IGNORE_INDEX] * 3 + [7])}),      # add_texts' check: no placeholder
    json.dumps({"id": 11, "caption": 1, "rows": ROWS_A}),                                                         # two query forms
    json.dumps({"id": 12, "caption": 4}),                                                                         # not a caption
]
ERRORS = {2: "malformed", 3: "unknown video id", 5: "empty", 6: "twice", 8: "tokenizer", 10: "placeholder", 11: "exactly one", 12: "caption must be"}


def _run(lines, B, **kw):
    srv, passes = _server(**kw)
    out = []
    summary = SR.serve(iter(lines), out.append, srv, batch_queries=B, batch_wait_ms=60000.0)       # (the end of the lines ends the wait: nothing sleeps)
    return [json.loads(x) for x in out], summary, srv, passes


@pytest.mark.parametrize("B", [1, 4, 64])
def test_serve_answers_in_arrival_order_whatever_the_batch(B):
    out, summary, srv, passes = _run(LINES, B)
    assert [x["id"] for x in out] == [0, "a", None, 3, 4, 5, 6, 7, 8, 9.5, 10, 11, 12]       # (the malformed line's id could not be read)
    for n, x in enumerate(out):
        if n in ERRORS:
            assert set(x) == {"id", "error"} and ERRORS[n] in x["error"], x
        else:
            assert set(x) == {"id", "query", "videos", "scores"} and x["scores"] == sorted(x["scores"], reverse=True)
    ref, _, _, _ = _run(LINES, 1)
    assert out == ref                                                            # a bad request costs its neighbours nothing
    assert out[0]["query"] == "caption:1" and sorted(out[0]["videos"]) == [f"v{j}" for j in range(6)]
    assert out[1]["query"] == "rows:4" and sorted(out[1]["videos"]) == ["v0", "v2", "v4"]
    want = 1.0 * np.array([_score(j, 4) for j in (4, 0, 2)])                      # the default blend: the query likelihood alone
    assert out[1]["scores"] == sorted((float(x) for x in want), reverse=True)
    assert out[4]["query"] == "rows:5" and out[4]["videos"] == ["v5"]
    assert out[7]["query"] == "rows:4" and len(out[7]["videos"]) == 2             # deduplicated: the first occurrence's text index
    assert len(out[9]["videos"]) == 3 and set(out[9]["videos"]) <= {"v2", "v0", "v4", "v1"}
    n_batches = -(-len(LINES) // B)
    assert summary == {"requests": 13, "batches": n_batches, "mean_batch": 13 / n_batches, "errors": 8, "texts_added": 2}
    assert len(srv.s.vtg_split) == 4 + 2 and len(srv.text_of) == 2
    assert len(passes) == sum(1 for a in range(0, len(LINES), B) if any(n not in ERRORS for n in range(a, min(a + B, len(LINES)))))


def test_serve_iv2_candidates_and_blank_lines():
    lines = [json.dumps({"id": 0, "caption": 2}), "", json.dumps({"id": 1, "rows": ROWS_A}), "  \n", json.dumps({"id": 2, "rows": ROWS_A, "candidates": ["v3"]})]
    for B in (1, 4):
        srv, _ = _server(["--candidates", "iv2", "--topk", "3", "--c", "0.5", "0", "0.5", "0"])
        out = []
        summary = SR.serve(iter(lines), out.append, srv, batch_queries=B, batch_wait_ms=60000.0)
        out = [json.loads(x) for x in out]
        row = srv.t2v_iv2[2]
        top = np.argsort(-row, kind="stable")[:3]
        blended = 0.5 * (0.5 * np.array([_score(j, 2) for j in top]) + 0.5 * np.zeros(3)) + 0.5 * row[top]
        o = np.argsort(-blended, kind="stable")
        assert out[0] == {"id": 0, "query": "caption:2", "videos": [f"v{j}" for j in top[o]], "scores": [float(x) for x in blended[o]]}
        assert "first-stage" in out[1]["error"] and out[2]["videos"] == ["v3"]
        assert summary["requests"] == 3 and summary["errors"] == 1 and summary["texts_added"] == 1


def test_serve_refuses_a_row_over_the_length_limit_and_a_blend_without_its_tvg_row():
    limit = 2 + NV + 1 + 1                                                        # [1, x] + video + [2]: one response token fits
    srv, _ = _server(max_row_len=limit)
    long_pre = {"vtg_ids": [1, 1, 1, IMG, 2, 7], "vtg_labels": [IGNORE_INDEX] * 5 + [7]}
    out = []
    SR.serve(iter([json.dumps({"id": 0, "rows": long_pre}), json.dumps({"id": 1, "rows": ROWS_B})]), out.append, srv, 4, 60000.0)
    out = [json.loads(x) for x in out]
    assert "tokenizer_model_max_length" in out[0]["error"] and out[1]["query"] == "rows:5"
    long_tvg = dict(ROWS_A, tvg_ids=[5] * limit + [IMG, 9], tvg_labels=[IGNORE_INDEX] * limit + [IMG, 9])
    n = len(srv.s.vtg_split)
    out = []
    SR.serve(iter([json.dumps({"id": 2, "rows": long_tvg})]), out.append, srv, 1, 0.0)
    assert "tokenizer_model_max_length" in json.loads(out[0])["error"] and len(srv.s.vtg_split) == n
    srv, _ = _server(["--c", "0.5", "0", "1", "0"], finetuned=True)
    out = []
    summary = SR.serve(iter([json.dumps({"id": 0, "rows": ROWS_B}), json.dumps({"id": 1, "rows": ROWS_A, "candidate_idx": [1, 2]})]), out.append, srv, 4, 60000.0)
    out = [json.loads(x) for x in out]
    assert "TVG row" in out[0]["error"] and out[1]["query"] == "rows:5" and summary["errors"] == 1
    srv, _ = _server(finetuned=True)                                              # c0 = 1: the TVG term has no weight, the text needs no TVG row
    out = []
    SR.serve(iter([json.dumps({"id": 0, "rows": ROWS_B, "candidate_idx": [1]})]), out.append, srv, 1, 0.0)
    assert json.loads(out[0])["videos"] == ["v1"]


def test_serve_text_requests_go_through_the_prompt_builder():
    built = []

    def build_rows(q):
        built.append(q)
        resp = [10 + len(w) for w in q.split()]
        return _vtg_row([1, 1], [2], resp), _tvg_row([5, 6] + resp)
    srv, _ = _server(build_rows=build_rows)
    out = []
    summary = SR.serve(iter([json.dumps({"id": n, "text": q, "candidate_idx": [0, 1, 2]}) for n, q in enumerate(["a dog runs", "a cat", "a dog runs"])]), out.append, srv, 2, 60000.0)
    out = [json.loads(x) for x in out]
    assert [x["query"] for x in out] == ["query:a dog runs", "query:a cat", "query:a dog runs"] and out[0]["scores"] == out[2]["scores"]
    assert summary["texts_added"] == 2 and len(srv.s.vtg_split) == 4 + 2 and built == ["a dog runs", "a cat", "a dog runs"]


def test_check_args_with_and_without_serve():
    p = SR.get_args_parser()
    with pytest.raises(SystemExit, match="t2v"):
        SR.check_args(p.parse_args(["--serve", "--direction", "v2t", "--video_ids", "0"]))
    with pytest.raises(SystemExit, match="stdin"):
        SR.check_args(p.parse_args(["--serve", "--query_ids", "0"]))
    with pytest.raises(SystemExit, match="batch_queries"):
        SR.check_args(p.parse_args(["--serve", "--batch_queries", "0"]))
    with pytest.raises(SystemExit, match="--serve"):
        SR.check_args(p.parse_args(["--query_ids", "0", "--batch_queries", "4"]))
    SR.check_args(p.parse_args(["--serve", "--batch_queries", "8", "--batch_wait_ms", "2.5", "--gallery_fill", "lazy"]))
    with pytest.raises(SystemExit, match="query"):                                # without --serve: as before
        SR.check_args(p.parse_args([]))
    a = p.parse_args(["--query_ids", "0"])
    assert (a.serve, a.batch_queries, a.batch_wait_ms) == (False, 1, 0.0)
    assert (a.candidates, a.topk, a.direction, a.gallery_fill, a.query, a.query_ids, a.video_ids, a.c, a.alpha, a.cpn, a.max_tokens, a.output) == \
        ("iv2", 10, "t2v", "eager", [], [0], [], None, [0.0, 0.0], False, 24576, None)
    assert (a.narrow_gemm, a.narrow_lo6, a.narrow_qkv, a.gallery_gb, a.gallery_host_gb, a.vtg_precise, a.tvg_precise, a.synthetic) == \
        ("off", "off", "off", None, None, "auto", "auto", 0)
    SR.check_args(a)
    assert a.c == [1.0, 0.0, 1.0, 0.0]
