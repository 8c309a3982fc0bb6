"""CPU: the one request type, the one K / K0 rule, the one candidate rule, the one report and the one-shot loops of the search command (blim_amd/gallery.py:
SearchRequest, check_shortlist, search_requests; blim_amd/search.py: default_candidates, answer_line, report_lines, gallery_banner, run_t2v, run_v2t) -- a request
given as a tuple and as a SearchRequest is the same request with the same scorer calls, every refusal of the rule comes from one function, the candidate rule is the
three rules the command had, the closing lines keep their text in one order, and the one-shot loops print what the index calls give.
Fakes as in tests/test_shortlist_host.py and tests/test_prefilter_host.py: no engine."""
import json
import types

import numpy as np
import pytest

import test_gallery_host as GH
import test_lazy_gallery_host as LZ
import test_prefilter_host as PF
import test_serve_host as SH
import test_shortlist_host as SL
from blim_amd import gallery as GL
from blim_amd import search as SR
from blim_amd.gallery import SearchRequest

N = PF.N


# ---- 1. tuples and SearchRequest
def test_a_search_request_is_a_tuple_of_three_four_or_five_fields():
    assert SearchRequest(*(2, [1, 4], None)) == (2, [1, 4], None, None, None)
    assert SearchRequest(*(2, None, None, 3)) == SearchRequest(2, shortlist=3) == (2, None, None, 3, None)
    r = SearchRequest(*(2, None, None, 3, 5))
    assert (r.text, r.cand, r.first_stage, r.shortlist, r.prefilter) == (2, None, None, 3, 5)
    with pytest.raises(TypeError):
        SearchRequest(*(2, None, None, 3, 5, 6))


@pytest.mark.parametrize("cpn", [False, True])
def test_tuples_and_search_requests_are_the_same_requests_with_the_same_calls(cpn):
    more = dict(cpn=cpn, alpha=(0.8, 0.3), c=SH.C_BLEND, finetuned=True)
    rng = np.random.RandomState(5)
    batch = [(0, None, None, 2, 4), (2, rng.permutation(N)[:4], rng.rand(4).astype(np.float32), None), (3, None, None, 3), (1, None, None, 3, 5), (4, None, None, 1, N + 9),
             (1, [4, 1], None, None, None), (2, None, None, 2, None), (3, [0, 5, 2], None)]
    for lazy in (False, True):
        runs = []
        for reqs in (batch, [SearchRequest(*r) for r in batch]):
            s = PF._fake()
            g = LZ._lazy(s, 3) if lazy else GH._gallery(s, {0: 0, 3: 1})
            passes = SH._scoring(g)
            kept = [tuple(r) for r in reqs]
            runs.append((g.search_requests(reqs, **more), s.first_calls, s.gallery_calls, s.tvg_calls, passes, g.stats.as_dict()))
            assert all(a is b or a == b for r, k in zip(reqs, kept) for a, b in zip(r, k) if not isinstance(a, np.ndarray))        # the requests are not written to
        SL._same_results(runs[0][0], runs[1][0])
        assert runs[0][1:] == runs[1][1:]
        assert runs[0][1] == [([0, 1, 4], N, cpn, 0.8)] and runs[0][2] == [[3, 2]] and len(runs[0][4]) == 1                         # one stage 0, one stage 1, one VTG pass
        assert sorted(call for call in runs[0][3] if not call[1]) == sorted([(4 + 5 + N, False), (4 + 2 + 3, False)])


# ---- 2. the K / K0 rule
@pytest.mark.parametrize("K,K0,n,limit,want", [
    (3, None, 6, 1024, (3, None)), (3, 5, 6, 1024, (3, 5)), (3, 100, 6, 1024, (3, 6)), (3, 3, 6, 1024, (3, 3)), (100, None, 6, 1024, (100, None)),
    (None, 4, 6, 1024, (None, 4)), (None, 100, 6, 1024, (None, 6)), (np.int64(2), np.int64(4), 6, 1024, (2, 4)), (2, 4, 6, 4, (2, 4)), (2, 100, 3, 4, (2, 3)),
    (True, None, 6, 1024, "positive integer"), (2.5, None, 6, 1024, "positive integer"), (0, None, 6, 1024, "k = 0"), (0, None, 6, 1024, "positive integer"),
    (-1, 4, 6, 1024, "positive integer"), (2, True, 6, 1024, "positive integer"), (2, 2.5, 6, 1024, "positive integer"), (2, 0, 6, 1024, "positive integer"),
    (None, 0, 6, 1024, "positive integer"), (3, 2, 6, 1024, "below the shortlist's K = 3"), (3, 2, 6, 1024, "at least the shortlist's K = 3"),
    (2, 5, 6, 4, "BLIM_TVG_RANK_MAX_K"), (2, 100, 6, 4, "limit of 4"), (None, 100, 6, 4, "BLIM_TVG_RANK_MAX_K"),
])
def test_check_shortlist_is_the_rule(monkeypatch, K, K0, n, limit, want):
    monkeypatch.setattr(GL, "TVG_RANK_MAX_K", limit)
    if isinstance(want, str):
        with pytest.raises(ValueError, match=want):
            GL.check_shortlist(K, K0, n)
    else:
        got = GL.check_shortlist(K, K0, n)
        assert got == want and all(x is None or type(x) is int for x in got)


def test_every_caller_refuses_through_check_shortlist(monkeypatch):
    s = PF._fake(n_texts=4)
    g = GH._gallery(s, {})
    SH._scoring(g)
    tg = GL.TextGalleryIndex(s)
    args = SR.get_args_parser().parse_args(["--serve", "--candidates", "all", "--resume", "x"])
    SR.check_args(args)
    srv =SR.Server(g, [f"v{j}" for j in range(N)], 4, None, args, finetuned=True)
    asked = []
    rule = GL.check_shortlist
    monkeypatch.setattr(GL, "check_shortlist", lambda K, K0, n: asked.append((K, K0, n)) or rule(K, K0, n))
    g.shortlist([1], 2); g.prefilter([1], 4); tg_refused = pytest.raises(ValueError, tg.shortlist, [1], 0)
    g.search_requests([(0, None, None, 2, 9)], finetuned=True)
    assert asked == [(2, None, N), (None, 4, N), (0, None, 4), (2, 9, N)] and "positive integer" in str(tg_refused.value)
    del asked[:]
    assert srv.parse(json.dumps({"caption": 0, "shortlist": 2, "prefilter": 9}))["prefilter"] == 9                  # (as given: the answer echoes it)
    assert asked == [(2, 9, N)]
    monkeypatch.setattr(GL, "TVG_RANK_MAX_K", 4)
    with pytest.raises(SR.BadRequest, match="BLIM_TVG_RANK_MAX_K"):                                                # the gallery's wording, as a bad request
        srv.parse(json.dumps({"caption": 0, "shortlist": 2, "prefilter": 5}))
    for K in ("4", 4.0):                                                                                           # the JSON types are the server's own check
        del asked[:]
        with pytest.raises(SR.BadRequest, match="positive integer"):
            srv.parse(json.dumps({"caption": 0, "shortlist": K}))
        assert asked == []


# ---- 3. the candidates of a query that names none
def test_default_candidates_is_the_three_rules_the_command_had():
    n, topk = 6, 4
    row = np.array([0.5, 1.0, 0.5, 1.0, -1.0, 0.5], np.float64)                     # ties
    # iv2, as the serve path and both one-shot loops had it
    r = np.asarray(row, dtype=np.float32)
    want = np.argsort(-r, kind="stable")[:min(topk, n)]
    cand, fs = SR.default_candidates("iv2", row, n, topk)
    assert cand.tolist() == want.tolist() == [1, 3, 0, 2] and fs.dtype == np.float32 and np.array_equal(fs, r[want])
    cand, fs = SR.default_candidates("iv2", row, n, 100)                           # k > N
    assert cand.tolist() == [1, 3, 0, 2, 5, 4] and np.array_equal(fs, r[cand])
    cand, fs = SR.default_candidates("iv2", row[:4], n, 100)                       # run-time videos have no score to be ranked by
    assert cand.tolist() == [1, 3, 0, 2]
    # all, as the serve path had it: a row shorter than the gallery is padded with zeros
    short = np.asarray(row[:n - 2], dtype=np.float32)
    want = np.concatenate([short, np.zeros(max(n - len(short), 0), np.float32)])[np.arange(n)]
    cand, fs = SR.default_candidates("all", row[:n - 2], n, topk)
    assert cand.tolist() == list(range(n)) and fs.dtype == np.float32 and np.array_equal(fs, want) and fs[-2:].tolist() == [0.0, 0.0]
    # all, as the one-shot loops had it: the row, or no first-stage term for a query without one
    cand, fs = SR.default_candidates("all", row, n, topk)
    assert cand.tolist() == list(range(n)) and np.array_equal(fs, np.asarray(row, dtype=np.float32)[np.arange(n)])
    cand, fs = SR.default_candidates("all", None, n, 100)
    assert cand.tolist() == list(range(n)) and fs is None


def test_answer_line_keeps_the_key_order():
    assert SR.answer_line("caption:1", "videos", ["v2", "v0"], np.array([0.5, -1.0], np.float32), head={"id": None}) == \
        '{"id": null, "query": "caption:1", "videos": ["v2", "v0"], "scores": [0.5, -1.0]}'
    assert SR.answer_line("rows:4", "videos", ["v2"], [0.25], 3, 5, head={"id": "a"}) == \
        '{"id": "a", "query": "rows:4", "videos": ["v2"], "scores": [0.25], "shortlisted": 3, "prefiltered": 5}'
    assert SR.answer_line("video:7", "texts", [3, 1], [0.5, 0.25], 2) == '{"query": "video:7", "texts": [3, 1], "scores": [0.5, 0.25], "shortlisted": 2}'


# ---- 4. the closing report and the banner
def _index(hits, host=None, **more):
    stats = types.SimpleNamespace(as_dict=lambda: {"hits": hits, "misses": 1, "admitted": 0, "evicted": 0, "prefix_tokens_packed": 58})
    tier = None if host is None else types.SimpleNamespace(stats=types.SimpleNamespace(as_dict=lambda: {"restored": host, "spilled": 2, "dropped": 0, "bytes_to_host": 64,
                                                                                                           "bytes_from_host": 32}), n_records=8, record_bytes=66080)
    return types.SimpleNamespace(stats=stats, host=tier, **more)


STATS = '{"hits": %d, "misses": 1, "admitted": 0, "evicted": 0, "prefix_tokens_packed": 58}'
TIER = '{"restored": %d, "spilled": 2, "dropped": 0, "bytes_to_host": 64, "bytes_from_host": 32, "records": 8, "record_bytes": 66080}'


def test_report_lines_keep_their_text_in_one_order():
    short, pre = {"queries": 3, "passes": 2, "pairs": 18}, {"queries": 2, "passes": 1, "rows": 2, "kept": 10}
    none = {"queries": 0, "passes": 0, "pairs": 0}
    summary = {"requests": 7, "batches": 3, "mean_batch": 7 / 3, "errors": 1, "texts_added": 2}
    assert SR.report_lines([("gallery", _index(4))]) == ["gallery stats: " + STATS % 4]
    assert SR.report_lines([("gallery", _index(4))], None, none, {"queries": 0, "passes": 0, "rows": 0, "kept": 0}) == ["gallery stats: " + STATS % 4]
    assert SR.report_lines([("gallery", _index(4, host=1))], summary, short, pre) == [
        "gallery stats: " + STATS % 4,
        "gallery host tier: " + TIER % 1,
        'serve: {"requests": 7, "batches": 3, "mean_batch": 2.3333333333333335, "errors": 1, "texts_added": 2}',
        'shortlist: {"queries": 3, "stage1_passes": 2, "stage1_pairs": 18}',
        'prefilter: {"queries": 2, "stage0_passes": 1, "stage0_rows": 2, "kept": 10}']
    assert SR.report_lines([("gallery", _index(4))], shortlist_stats=short) == ["gallery stats: " + STATS % 4, 'shortlist: {"queries": 3, "stage1_passes": 2, "stage1_pairs": 18}']
    two = lambda a, b: [("gallery", _index(4, host=a)), ("text gallery", _index(9, host=b))]
    both = "gallery stats: " + STATS % 4 + "; text gallery stats: " + STATS % 9
    assert SR.report_lines(two(None, None)) == [both]
    assert SR.report_lines(two(1, 5), shortlist_stats=short) == [both, "gallery host tier: " + TIER % 1 + "; text gallery host tier: " + TIER % 5,
                                                                 'shortlist: {"queries": 3, "stage1_passes": 2, "stage1_pairs": 18}']
    assert SR.report_lines(two(None, 5)) == [both, "text gallery host tier: " + TIER % 5]
    assert SR.report_lines(two(1, None), shortlist_stats=none) == [both, "gallery host tier: " + TIER % 1]


def test_the_gallery_banner_is_one_function_for_both_directions():
    args = SR.get_args_parser().parse_args(["--query_ids", "0", "--narrow_lo6", "auto"])
    s = types.SimpleNamespace(video=[0] * 24, tvg_split=[0] * 20, vtg_mode=None, tvg_mode="full")
    gal = types.SimpleNamespace(s=s, fill="eager", n_slots=6, cache=types.SimpleNamespace(bytes=6 * 66048), build_seconds=0.256)
    assert SR.gallery_banner(args, [("gallery", gal)], 3.14159) == \
        "gallery: 24 videos, fill eager, 6 cached slots of 66048 bytes, mode none, narrow_gemm off, narrow_lo6 auto, narrow_qkv off, built in 0.26s (ready 3.1s after start)"
    gal.fill, gal.cache, gal.n_slots, s.vtg_mode = "lazy", None, 0, "full"
    assert SR.gallery_banner(args, [("gallery", gal)], 3.0).startswith("gallery: 24 videos, fill lazy, 0 slots of 0 bytes, mode full, narrow_gemm off")
    tg = types.SimpleNamespace(n_slots=20, per_slot_bytes=lambda: 4352, build_seconds=0.5)
    assert SR.gallery_banner(args, [("gallery", gal), ("text gallery", tg)], 7.0) == \
        ("gallery: 24 videos, fill lazy, 0 slots, mode full, built in 0.26s; 20 texts, 20 caption slots of 4352 bytes, tvg mode full, narrow_gemm off, narrow_lo6 auto, "
         "narrow_qkv off, built in 0.50s (ready 7.0s after start)")


# ---- 5. the one-shot loops, on the fake indexes
VIDS = [f"v{j}" for j in range(N)]
IV2 = np.random.RandomState(1).rand(5, N).astype(np.float32)
BLEND = ["--cpn", "--alpha", "0.8", "0.3", "--c", "0.6", "0.5", "0.7", "0.5"]


def _gallery():
    s = PF._fake()
    g = GH._gallery(s, {0: 0, 3: 1})
    SH._scoring(g)
    return g


def _args(argv):
    args = SR.get_args_parser().parse_args(list(argv) + BLEND)
    SR.check_args(args)
    return args


@pytest.mark.parametrize("mode", [["--candidates", "iv2"], ["--candidates", "all"], ["--candidates", "all", "--resume", "x"], ["--candidates", "tvg", "--resume", "x", "--shortlist", "4"],
                                  ["--candidates", "tvg", "--resume", "x", "--shortlist", "4", "--prefilter", "5"], ["--candidates", "tvg", "--resume", "x"]])
def test_run_t2v_prints_what_the_index_calls_give(mode):
    args = _args(["--query_ids", "1", "4", "1", "--topk", "3"] + mode)
    got = []
    g = _gallery()
    SR.run_t2v(g, VIDS, IV2, args, got.append)
    # the loop the command had, on a fresh index
    g2, want = _gallery(), []
    k, finetuned = min(args.topk, N), bool(args.resume)
    for t in args.query_ids:
        more = {}
        if args.candidates == "tvg":
            K, K0 = SR.shortlist_k(args), args.prefilter
            (o, b), = g2.search_requests([(t, None, None, K) + (() if K0 is None else (K0,))], cpn=args.cpn, alpha=args.alpha, c=args.c, finetuned=finetuned)
            order, blended, more = o[None, :k], b[None, :k], {"shortlisted": K, **({} if K0 is None else {"prefiltered": K0})}
        else:
            if args.candidates == "iv2":
                row = np.asarray(IV2[t], dtype=np.float32)
                cand = np.argsort(-row, kind="stable")[:k][None]
                fs = row[cand]
            else:
                cand = np.arange(N)[None]
                fs = np.asarray(IV2[t], dtype=np.float32)[cand]
            order, blended = g2.rerank([t], cand, first_stage=fs, cpn=args.cpn, alpha=args.alpha, c=args.c, finetuned=finetuned)
        want.append(json.dumps({"query": f"caption:{t}", "videos": [VIDS[int(j)] for j in order[0]], "scores": [float(x) for x in blended[0]], **more}))
    assert got == want and len(got) == 3
    assert (g.s.first_calls, g.s.gallery_calls, g.s.tvg_calls) == (g2.s.first_calls, g2.s.gallery_calls, g2.s.tvg_calls)
    assert g.shortlist_stats == g2.shortlist_stats and g.prefilter_stats == g2.prefilter_stats and g.stats.as_dict() == g2.stats.as_dict()
    out = [json.loads(x) for x in got]
    if args.candidates == "tvg":
        assert all(x["shortlisted"] == SR.shortlist_k(args) and len(x["videos"]) == 3 for x in out)                # K kept, --topk printed
        assert all(("prefiltered" in x) == (args.prefilter is not None) for x in out) and list(out[0])[:3] == ["query", "videos", "scores"]
    else:
        assert all(set(x) == {"query", "videos", "scores"} and len(x["videos"]) == (3 if args.candidates == "iv2" else N) for x in out)


def test_run_t2v_gives_a_query_without_a_row_no_first_stage_term():
    args = _args(["--query_ids", "1", "--candidates", "all"])
    args.query = ["a dog runs"]                                                      # (the last text of the scorer is this query: no first-stage row)
    got, g, g2 = [], _gallery(), _gallery()
    SR.run_t2v(g, VIDS, IV2, args, got.append)
    more = dict(cpn=args.cpn, alpha=args.alpha, c=args.c, finetuned=False)
    o1, b1 = g2.rerank([1], np.arange(N)[None], first_stage=np.asarray(IV2[1], dtype=np.float32)[np.arange(N)[None]], **more)
    o2, b2 = g2.rerank([4], np.arange(N)[None], first_stage=None, **more)
    assert got == [json.dumps({"query": "caption:1", "videos": [VIDS[int(j)] for j in o1[0]], "scores": [float(x) for x in b1[0]]}),
                   json.dumps({"query": "query:a dog runs", "videos": [VIDS[int(j)] for j in o2[0]], "scores": [float(x) for x in b2[0]]})]


def _text_gallery():
    s = SL._fake()
    tg = GL.TextGalleryIndex(s)
    tg.tvg_pairs = lambda pairs: np.array([SL._stage(j, i) for j, i in pairs], np.float32)
    tg.vtg_pairs = lambda pairs: np.array([SH._score(j, i) for j, i in pairs], np.float32)
    return tg


@pytest.mark.parametrize("mode", [["--candidates", "iv2"], ["--candidates", "all"], ["--candidates", "all", "--resume", "x"], ["--candidates", "tvg", "--resume", "x", "--shortlist", "3"],
                                  ["--candidates", "tvg", "--resume", "x"]])
def test_run_v2t_prints_what_the_index_calls_give(mode):
    args = SR.get_args_parser().parse_args(["--direction", "v2t", "--video_ids", "4", "1", "5", "--topk", "2", "--c", "0.6", "0.5", "0.7", "0.5"] + mode)
    SR.check_args(args)
    v2t_iv2 = np.random.RandomState(2).rand(N - 1, 5).astype(np.float32)             # video 5 joined from outside: no first-stage row
    if args.candidates == "iv2":
        args.video_ids = [4, 1]
    got = []
    stats = SR.run_v2t(_text_gallery(), VIDS, v2t_iv2, args, got.append)
    # the loop the command had
    tg, want, n_texts = _text_gallery(), [], 5
    k, finetuned = min(args.topk, n_texts), bool(args.resume)
    for v in args.video_ids:
        more = {}
        if args.candidates == "tvg":
            K = SR.shortlist_k(args)
            order, blended = tg.rerank_shortlist([v], K, cpn=args.cpn, alpha=args.alpha, c=args.c)
            order, blended, more = order[:, :k], blended[:, :k], {"shortlisted": K}
        else:
            if args.candidates == "iv2":
                row = np.asarray(v2t_iv2[v], dtype=np.float32)
                cand = np.argsort(-row, kind="stable")[:k][None]
                fs = row[cand]
            else:
                cand = np.arange(n_texts)[None]
                fs = None if v >= len(v2t_iv2) else np.asarray(v2t_iv2[v], dtype=np.float32)[cand]
            order, blended = tg.rerank([v], cand, first_stage=fs, cpn=args.cpn, alpha=args.alpha, c=args.c, finetuned=finetuned)
        want.append(json.dumps({"query": f"video:{VIDS[v]}", "texts": [int(i) for i in order[0]], "scores": [float(x) for x in blended[0]], **more}))
    assert got == want and len(got) == len(args.video_ids)
    n = len(args.video_ids) if args.candidates == "tvg" else 0
    assert stats == {"queries": n, "passes": n, "pairs": n * n_texts}
    out = [json.loads(x) for x in got]
    assert all(len(x["texts"]) == (n_texts if args.candidates == "all" else 2) and ("shortlisted" in x) == (args.candidates == "tvg") for x in out)
