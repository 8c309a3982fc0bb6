"""CPU: the host side of searching inside a caller's set of videos (blim_amd/gallery.py: SearchRequest.within, GalleryIndex._checked / _chosen /
prefilter(within=); blim_amd/search.py: the serve fields `within` / `within_idx`, `"within": M` in the answer, --within_ids, the `within:` stderr line).  The fakes of
tests/test_shortlist_host.py / test_prefilter_host.py with a stage 0 that takes a set: no engine.  The GPU side is tests/test_within_gpu.py."""
import copy
import json
import pickle

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


def _fake(n_videos=N, n_texts=5):
    """test_prefilter_host's fake scorer, its stage 0 taking `within`: the whole-gallery order filtered to each text's set, -1 / NaN behind it."""
    s = PF._fake(n_videos=n_videos, n_texts=n_texts)
    whole = s.tvg_first
    s.within_calls = []

    def tvg_first(texts, k, cpn=False, alpha=0.0, full=False, within=None):
        if within is None:
            return whole(texts, k, cpn=cpn, alpha=alpha, full=full)
        texts = np.asarray(texts, np.int64).reshape(-1)
        s._need_tvg(texts)
        s.within_calls.append((texts.tolist(), int(k), bool(cpn), float(alpha), [np.asarray(w).tolist() for w in within]))
        idx, val = np.full((len(texts), k), -1, np.int64), np.full((len(texts), k), np.nan, np.float32)
        for q, (i, w) in enumerate(zip(texts, within)):
            row = np.array([PF._first(j, i) - (np.float32(alpha) * PF._first(j, 0) if cpn else 0) for j in range(n_videos)], np.float32)
            order = [j for j in np.argsort(-row, kind="stable") if j in set(np.asarray(w).tolist())][:k]
            idx[q, :len(order)], val[q, :len(order)] = order, row[order]
        return idx, val
    s.tvg_first = tvg_first
    return s


def _kept(t, K0, cpn, alpha, within):
    row = np.array([PF._first(j, t) - (np.float32(alpha[0]) * PF._first(j, 0) if cpn else 0) for j in range(N)], np.float32)
    return np.sort([j for j in np.argsort(-row, kind="stable") if j in set(within)][:K0])


def _gallery():
    s = _fake()
    g = GH._gallery(s, {0: 0, 3: 1})
    return s, g, SH._scoring(g)


# ---- 1. the request
def test_tuples_of_three_four_and_five_fields_are_unchanged_and_within_rides_beside_them():
    assert SearchRequest(*(2, [1, 4], None)) == (2, [1, 4], None, None, None) and SearchRequest(2, [1, 4]).within is None
    r = SearchRequest(2, shortlist=3, prefilter=5, within=[4, 1])
    assert r == (2, None, None, 3, 5) and r.within == [4, 1] and len(r) == 5 and "within=[4, 1]" in repr(r)
    assert "within" not in repr(SearchRequest(2, shortlist=3))
    batch = [(0, None, None, 2, 4), (2, [3, 1, 0], [0.5, 0.25, 0.125], None), (3, None, None, 3), (1, [4, 1], None)]
    more = dict(cpn=True, alpha=(0.8, 0.3), c=SH.C_BLEND, finetuned=True)
    s, g, _ = _gallery()
    got = g.search_requests(batch, **more)
    s1, g1, _ = _gallery()
    SL._same_results(got, g1.search_requests([SearchRequest(*r) for r in batch], **more))
    assert s.within_calls == [] and g.within_stats == {"queries": 0, "candidates": 0} and s.first_calls == s1.first_calls


def test_replace_make_and_repr_leave_a_valid_request_and_carry_the_set():
    """The NamedTuple API builds through tuple.__new__: every such request has `within`, None without a set, and search_requests takes it."""
    plain = SearchRequest(1, shortlist=3)
    r = plain._replace(shortlist=2)
    assert r.within is None and r == (1, None, None, 2, None) and "within" not in repr(r) and type(r) is SearchRequest
    m = SearchRequest._make((1, None, None, 2, 4))
    assert m.within is None and repr(m) == "SearchRequest(text=1, cand=None, first_stage=None, shortlist=2, prefilter=4)"
    assert tuple.__new__(SearchRequest, (1, None, None, 2, None)).within is None
    w = SearchRequest(1, shortlist=3, within=[4, 1])
    assert w._replace(prefilter=5).within == [4, 1] and w._replace(prefilter=5).prefilter == 5 and w._replace(within=None).within is None
    assert w._replace(within=[2]).within == [2] and w.within == [4, 1]
    assert SearchRequest._make((1, None, None, 2, None), within=[3]).within == [3] and "within=[3]" in repr(SearchRequest._make((1, None, None, 2, None), within=[3]))
    assert copy.copy(w).within == [4, 1] and pickle.loads(pickle.dumps(w)).within == [4, 1]
    # what the five-field tuple costs: == / hash / _fields / _asdict do not see the set
    assert w == plain and hash(w) == hash(plain) and "within" not in SearchRequest._fields and "within" not in w._asdict()
    more = dict(cpn=False, alpha=(0.8, 0.3), c=SH.C_BLEND, finetuned=True)
    s, g, _ = _gallery()
    s1, g1, _ = _gallery()
    SL._same_results(g.search_requests([r, m, w._replace(shortlist=2)], **more),
                     g1.search_requests([(1, None, None, 2), (1, None, None, 2, 4), SearchRequest(1, shortlist=2, within=[4, 1])], **more))
    assert g.within_stats == {"queries": 1, "candidates": 2}


def test_every_refusal_of_checked_names_its_rule():
    s, g, _ = _gallery()
    W = lambda *a, **k: SearchRequest(*a, **k)
    for bad, msg in ((W(0, [1, 2], within=[1, 2]), "names its candidates takes no within"), (W(0, [1, 2], None, 2, within=[1, 2]), "takes no within"),
                     (W(0, None, [0.5], 2, within=[1]), "first stage takes no within"), (W(0, within=[1, 2]), "within confines a shortlist: the request needs its K"),
                     (W(0, shortlist=2, within=[]), "within: an empty set"), (W(0, shortlist=2, within=[1, N]), f"within: video index {N} outside 0 .. {N - 1}"),
                     (W(0, shortlist=2, within=[-1, 2]), "within: video index -1 outside"), (W(0, shortlist=2, within=[3, 1, 3]), "within: video index 3 named twice"),
                     (W(0, shortlist=2, within=[1.5]), "within: a list of integer video indices"), (W(0, shortlist=2, within="ab"), "integer video indices"),
                     (W(0, shortlist=0, within=[1]), "positive integer"), (W(0, shortlist=3, prefilter=2, within=[0, 1, 2, 3]), "below the shortlist's K = 3"),
                     (W(0, None, None, None, 3, within=[1]), "needs its K")):
        with pytest.raises(ValueError, match=msg):
            g.search_requests([(1, [0], None, None), bad], finetuned=True)
    with pytest.raises(ValueError, match="finetuned=False"):
        g.search_requests([W(0, shortlist=2, within=[1, 2])], finetuned=False)
    assert s.within_calls == [] and s.first_calls == [] and g.within_stats == {"queries": 0, "candidates": 0}
    # the existing refusals keep their words
    for bad, msg in (((0, [1], None, 2, 4), "one of the two"), ((0, None, None, None, 3), "needs its K"), ((0, None, None), "one of the two")):
        with pytest.raises(ValueError, match=msg):
            g.search_requests([bad], finetuned=True)


def test_k_and_k0_are_clipped_to_the_set(monkeypatch):
    s, g, _ = _gallery()
    reqs = g._checked([SearchRequest(0, shortlist=5, prefilter=9, within=[4, 0, 2]), SearchRequest(1, shortlist=2, within=[5, 3, 1, 0])], True)
    assert reqs[0].prefilter == 3 and reqs[0].shortlist == 5 and reqs[0].within.tolist() == [0, 2, 4] and reqs[0].within.dtype == np.int64
    assert reqs[1].prefilter is None and reqs[1].within.tolist() == [0, 1, 3, 5]
    (order, blended), (o1, _) = g.search_requests([SearchRequest(0, shortlist=5, prefilter=9, within=[4, 0, 2]), SearchRequest(1, shortlist=2, within=[5, 3, 1, 0])],
                                                  finetuned=True, c=SH.C_BLEND)
    assert sorted(order.tolist()) == [0, 2, 4] and len(blended) == 3             # a K above the set's size keeps the whole set
    assert len(o1) == 2 and set(o1.tolist()) <= {0, 1, 3, 5}
    assert s.within_calls == [([0], 3, False, 0.0, [[0, 2, 4]])]                  # K0 clipped to the set before stage 0
    monkeypatch.setattr(GL, "TVG_RANK_MAX_K", 4)                                   # the kernel's limit binds the CLIPPED K0
    g.search_requests([SearchRequest(0, shortlist=2, prefilter=100, within=[0, 1, 2, 3])], finetuned=True)
    with pytest.raises(ValueError, match="BLIM_TVG_RANK_MAX_K"):
        g.search_requests([SearchRequest(0, shortlist=2, prefilter=100, within=[0, 1, 2, 3, 4])], finetuned=True)


# ---- 2. the passes
@pytest.mark.parametrize("cpn", [False, True])
def test_one_stage0_pass_for_the_within_requests_one_vtg_pass_for_all(cpn):
    alpha, c = (0.8, 0.3), SH.C_BLEND
    more = dict(cpn=cpn, alpha=alpha, c=c, finetuned=True)
    W = SearchRequest
    batch = [W(0, shortlist=2, prefilter=4, within=[5, 0, 3, 1, 2]), (2, [3, 1, 0, 4], [0.5, 0.25, 0.125, 1.0], None), (3, None, None, 3), W(1, shortlist=2, prefilter=3, within=[4, 2, 1, 0]),
             (4, None, None, 1, N + 9), W(2, shortlist=3, within=[1, 5, 4, 0]), W(0, shortlist=1, prefilter=N + 9, within=[2, 3])]
    sets = {0: [0, 1, 2, 3, 5], 3: [0, 1, 2, 4], 5: [0, 1, 4, 5], 6: [2, 3]}

    def fresh(lazy):
        s = _fake()
        g = LZ._lazy(s, 3) if lazy else GH._gallery(s, {0: 0, 3: 1})
        return s, g, SH._scoring(g)
    for lazy in (False, True):
        s, g, passes = fresh(lazy)
        got = g.search_requests(batch, **more)
        assert len(passes) == 1                                                    # ONE vtg_pairs pass for the whole batch
        assert s.within_calls == [([0, 1, 0], 4, cpn, 0.8, [sets[0], sets[3], sets[6]])]     # ONE stage-0 pass of their own, at the largest (clipped) K0
        assert s.first_calls == [([4], N, cpn, 0.8)] and s.gallery_calls == [[3]]  # the plain prefilter and the plain shortlist: as they were
        likelihood = sorted(call for call in s.tvg_calls if not call[1])
        assert likelihood == sorted([(4 + 3 + 4 + 2, False), (N, False), (4, False)])       # ONE TVG call over what the within requests kept (the set itself without a K0)
        assert g.within_stats == {"queries": 4, "candidates": 5 + 4 + 4 + 2}
        assert g.prefilter_stats == {"queries": 1 + 3, "passes": 2, "rows": 1 + 2, "kept": N + 4 + 3 + 2}
        assert g.shortlist_stats == {"queries": 1, "passes": 1, "pairs": N}
        for n, ws in sets.items():
            assert set(got[n][0].tolist()) <= set(ws) and len(got[n][0]) == min(batch[n].shortlist, len(ws))
        # each request alone: the same answer, bit for bit
        s1, g1, _ = fresh(lazy)
        SL._same_results(got, [g1.search_requests([r], **more)[0] for r in batch])
        # the composition by hand: prefilter(within=) -> PairScorer.tvg over the kept pairs (- alpha x prior) -> _best K -> vtg_pairs -> _blend
        for n, ws in sets.items():
            r = batch[n]
            s3, g3, _ = fresh(lazy)
            cand0 = np.asarray(ws) if r.prefilter is None else g3.prefilter([r.text], r.prefilter, cpn=cpn, alpha=alpha, within=[r.within])[0]
            if r.prefilter is not None:
                assert cand0.tolist() == _kept(r.text, min(r.prefilter, len(ws)), cpn, alpha, ws).tolist()
            term = s3.tvg(np.stack([cand0, np.full(len(cand0), r.text)], axis=1))
            if cpn:
                term = term - alpha[0] * g3._t2v_prior([r.text], [cand0])
            keep, stage = g3._best(term, r.shortlist)
            cand = cand0[keep]
            ql = g3.vtg_pairs(np.stack([cand, np.full(len(cand), r.text)], axis=1))
            o, b = g3._blend(cand[None], ql[None], stage[None], np.zeros((1, len(cand))), c)
            assert np.array_equal(got[n][0], o[0]) and np.array_equal(got[n][1], b[0])
    # within = every video: the request without within
    s, g, _ = fresh(False)
    s2, g2, _ = fresh(False)
    SL._same_results(g.search_requests([W(1, shortlist=2, prefilter=4, within=list(range(N)))], **more), g2.search_requests([(1, None, None, 2, 4)], **more))


def test_public_prefilter_takes_one_set_per_text():
    s, g, _ = _gallery()
    kept = g.prefilter([1, 3], 2, within=[[5, 0, 3], [2]])
    assert [k.tolist() for k in kept] == [_kept(1, 2, False, (0, 0), [0, 3, 5]).tolist(), [2]]
    assert s.within_calls == [([1, 3], 2, False, 0.0, [[0, 3, 5], [2]])] and g.within_stats == {"queries": 2, "candidates": 4}
    for bad, msg in (([[1]], "1 sets for 2 texts"), ([[1], []], "empty set"), ([[1], [7]], "outside"), ([[1, 1], [2]], "named twice")):
        with pytest.raises(ValueError, match=msg):
            g.prefilter([1, 3], 2, within=bad)


# ---- 3. serve
def _server(argv, finetuned=True, limit=None):
    s = _fake(n_texts=4)
    g = GH._gallery(s, {0: 0, 3: 1})
    passes = SH._scoring(g)
    args = SR.get_args_parser().parse_args(["--serve"] + list(argv))
    SR.check_args(args)
    iv2 = np.random.RandomState(1).rand(4, N).astype(np.float32)
    return SR.Server(g, [f"v{j}" for j in range(N)], 4, iv2, args, finetuned=finetuned), passes


ALL = ["--candidates", "all", "--resume", "x", "--c", "0.5", "0", "1", "0"]


def test_parse_reads_the_within_fields_and_every_error_line():
    srv, _ = _server(ALL)
    r = srv.parse(json.dumps({"id": 1, "caption": 2, "shortlist": 3, "within": ["v4", "v1", "v5"]}))
    assert r["within"].tolist() == [1, 4, 5] and r["shortlist"] == 3 and r["prefilter"] is None and r["cand"] is None
    r = srv.parse(json.dumps({"id": 1, "caption": 2, "shortlist": 3, "prefilter": 9, "within_idx": [4, 0]}))
    assert r["within"].tolist() == [0, 4] and r["prefilter"] == 9
    assert "within" not in srv.parse(json.dumps({"id": 1, "caption": 2, "shortlist": 3}))             # a request without the field: the dict it was
    for req, msg in (({"caption": 0, "shortlist": 2, "within": ["v1"], "within_idx": [1]}, "one form of the set"),
                     ({"caption": 0, "within": ["v1"], "candidates": ["v1", "v2"]}, "with candidates names its own candidates and takes no within"),
                     ({"caption": 0, "within_idx": [1], "candidate_idx": [1, 2]}, "with candidate_idx names its own"),
                     ({"caption": 0, "shortlist": 2, "within": ["v1"], "first_stage": [0.5]}, "first_stage"),
                     ({"caption": 0, "within": ["v1", "v2"]}, "within confines a shortlist: give shortlist"),
                     ({"caption": 0, "shortlist": 2, "within": []}, "the within list is empty"), ({"caption": 0, "shortlist": 2, "within_idx": "x"}, "within / within_idx must be a list"),
                     ({"caption": 0, "shortlist": 2, "within": {"v1": 1}}, "must be a list"),
                     ({"caption": 0, "shortlist": 2, "within": ["v1", "nope"]}, "within: unknown video id 'nope'"),
                     ({"caption": 0, "shortlist": 2, "within_idx": [1, N]}, f"within_idx must hold indices in 0 .. {N - 1}"),
                     ({"caption": 0, "shortlist": 2, "within_idx": [1, True]}, "within_idx must hold indices"),
                     ({"caption": 0, "shortlist": 2, "within": ["v1", "v3", "v1"]}, "within list names a video twice"),
                     ({"caption": 0, "shortlist": 3, "prefilter": 2, "within": ["v1", "v2", "v3"]}, "at least the shortlist's K = 3"),
                     ({"add_video": {"vid": "x", "features": "f.pt"}, "within": ["v1"]}, "carries no query"),
                     ({"add_video": {"vid": "x", "features": "f.pt"}, "within_idx": [1]}, "carries no query"),
                     # the existing messages, for their own cases
                     ({"caption": 0, "shortlist": 2, "candidates": ["v1"]}, "shortlist or candidates / candidate_idx, not both"),
                     ({"caption": 0, "candidates": ["v1"], "candidate_idx": [1]}, r"candidates \(video ids\) or candidate_idx \(indices\), not both"),
                     ({"caption": 0, "prefilter": 4}, "narrows a shortlist")):
        with pytest.raises(SR.BadRequest, match=msg) as e:
            srv.parse(json.dumps(dict(req, id=7)))
        assert e.value.id == 7
    tvg, _ = _server(["--candidates", "tvg", "--resume", "x", "--topk", "2", "--prefilter", "5"])
    r = tvg.parse(json.dumps({"caption": 1, "within": ["v0", "v2", "v3"]}))       # next to the default K, under the --prefilter default
    assert r["shortlist"] == 2 and r["prefilter"] == 5 and r["within"].tolist() == [0, 2, 3]


def test_the_length_check_uses_the_sets_videos():
    srv, _ = _server(ALL)
    srv.n_vid = np.array([4, 4, 4, 4, 4, 400])
    pre, post, _ = srv.s.vtg_split[2]
    srv.s.max_row_len = len(pre) + len(post) + 100
    with pytest.raises(SR.BadRequest, match="tokenizer_model_max_length"):
        srv.parse(json.dumps({"caption": 2, "shortlist": 2}))
    with pytest.raises(SR.BadRequest, match="tokenizer_model_max_length"):
        srv.parse(json.dumps({"caption": 2, "shortlist": 2, "within_idx": [1, 5]}))
    assert srv.parse(json.dumps({"caption": 2, "shortlist": 2, "within_idx": [1, 4]}))["within"].tolist() == [1, 4]


@pytest.mark.parametrize("B", [1, 3, 64])
def test_serve_answers_within_requests_whatever_the_batch(B):
    lines = [json.dumps({"id": 0, "caption": 1, "shortlist": 2, "prefilter": 3, "within": ["v5", "v0", "v2", "v3"]}),
             json.dumps({"id": 1, "rows": SH.ROWS_A, "candidate_idx": [4, 0, 2], "first_stage": [0.1, 0.9, 0.5]}),
             json.dumps({"id": 2, "caption": 0, "shortlist": 3, "within": ["v1", "v9"]}),
             json.dumps({"id": 3, "rows": SH.ROWS_A, "shortlist": 4, "within_idx": [2, 4], "topk": 1}),
             json.dumps({"id": 4, "caption": 3, "shortlist": 2, "prefilter": 4}),
             json.dumps({"id": 5, "caption": 2, "within": ["v1"]})]
    runs = {}
    for b in (1, B):
        srv, passes = _server(ALL)
        out = []
        summary = SR.serve(iter(lines), out.append, srv, batch_queries=b, batch_wait_ms=60000.0)
        runs[b] = ([json.loads(x) for x in out], summary, len(passes), srv)
    out, summary, n_passes, srv = runs[B]
    assert out == runs[1][0]                                                       # whatever the batch
    assert [x["id"] for x in out] == list(range(6)) and [n for n, x in enumerate(out) if "error" in x] == [2, 5] and summary["errors"] == 2
    assert "unknown video id 'v9'" in out[2]["error"] and "within confines a shortlist" in out[5]["error"]
    assert list(out[0]) == ["id", "query", "videos", "scores", "shortlisted", "prefiltered", "within"]
    assert out[0]["within"] == 4 and out[0]["shortlisted"] == 2 and out[0]["prefiltered"] == 3
    assert len(out[0]["videos"]) == 2 and set(out[0]["videos"]) <= {f"v{j}" for j in _kept(1, 3, False, (0, 0), [0, 2, 3, 5])}
    assert out[3]["within"] == 2 and out[3]["shortlisted"] == 4 and out[3]["videos"][0] in ("v2", "v4") and len(out[3]["videos"]) == 1 and "prefiltered" not in out[3]
    assert set(out[4]) == {"id", "query", "videos", "scores", "shortlisted", "prefiltered"} and set(out[1]) == {"id", "query", "videos", "scores"}
    assert srv.gal.within_stats == {"queries": 2, "candidates": 6}
    assert SR.report_lines([("gallery", srv.gal)], summary, srv.gal.shortlist_stats, srv.gal.prefilter_stats, srv.gal.within_stats)[-1] == \
        'within: {"queries": 2, "candidates": 6}'
    # a run whose requests carry no set: the lines it always had
    plain, _ = _server(ALL)
    SR.serve(iter([lines[1], lines[4]]), [].append, plain, batch_queries=B)
    assert not any(ln.startswith("within:") for ln in SR.report_lines([("gallery", plain.gal)], None, plain.gal.shortlist_stats, plain.gal.prefilter_stats, plain.gal.within_stats))
    assert SR.report_lines([("gallery", plain.gal)], None, plain.gal.shortlist_stats, plain.gal.prefilter_stats) == \
        SR.report_lines([("gallery", plain.gal)], None, plain.gal.shortlist_stats, plain.gal.prefilter_stats, plain.gal.within_stats)


# ---- 4. the command's arguments
@pytest.mark.parametrize("argv,msg", [
    (["--query_ids", "0", "--within_ids", "f.txt", "--resume", "x"], "--within_ids confines the shortlist --candidates tvg takes"),
    (["--query_ids", "0", "--candidates", "all", "--within_ids", "f.txt", "--resume", "x"], "--within_ids confines the shortlist"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--within_ids", "f.txt", "--resume", "x"], "--within_ids confines the t2v shortlist"),
    (["--serve", "--candidates", "tvg", "--within_ids", "f.txt", "--resume", "x"], "a --serve request carries its own set"),
    (["--query_ids", "0", "--candidates", "tvg", "--within_ids", "f.txt"], "--candidates tvg needs a fine-tuned checkpoint"),
])
def test_check_args_refusals(argv, msg):
    with pytest.raises(SystemExit, match=msg):
        SR.check_args(SR.get_args_parser().parse_args(argv))


def test_check_args_accepts_within_ids_and_the_file_is_read(tmp_path):
    p = SR.get_args_parser()
    assert p.parse_args(["--query_ids", "0"]).within_ids is None
    SR.check_args(p.parse_args(["--query_ids", "0", "--candidates", "tvg", "--resume", "x", "--prefilter", "64", "--within_ids", "f.txt"]))
    f = tmp_path / "ids.txt"
    f.write_text("v4\n\nv1 \nv5\n")
    vids = [f"v{j}" for j in range(N)]
    assert SR.read_within_ids(str(f), vids).tolist() == [1, 4, 5]
    for text, msg in (("", "an empty set"), ("v1\nzz\n", "unknown video id 'zz'"), ("v1\nv2\nv1\n", "names video 'v1' twice")):
        f.write_text(text)
        with pytest.raises(SystemExit, match=msg):
            SR.read_within_ids(str(f), vids)
    with pytest.raises(SystemExit, match="--within_ids"):
        SR.read_within_ids(str(tmp_path / "missing.txt"), vids)
    assert SR._within_line({"queries": 3, "candidates": 17}) == {"queries": 3, "candidates": 17}
    assert json.loads(SR.answer_line("q", "videos", ["a"], [0.5], 2, 4, within=3)) == {"query": "q", "videos": ["a"], "scores": [0.5], "shortlisted": 2, "prefiltered": 4, "within": 3}
    assert "within" not in json.loads(SR.answer_line("q", "videos", ["a"], [0.5], 2, 4))


# ---- 5. the add_video barrier
def test_a_set_may_name_a_video_added_earlier_in_the_stream_behind_the_barrier(tmp_path):
    import test_grow_host as GR
    srv, _, feats = GR._server(tmp_path, ["--candidates", "all", "--resume", "x"])
    srv.finetuned = True
    srv.s.tvg_split = [np.array([1, 2, 3])] * len(srv.s.vtg_split)                 # (every caption has its TVG row)
    scored = []

    def score(reqs):
        scored.append([(r["text"], r["shortlist"], r["prefilter"], None if r.get("within") is None else r["within"].tolist()) for r in reqs])
        return [(r["within"][:r["shortlist"]], np.zeros(min(r["shortlist"], len(r["within"])))) for r in reqs]
    srv._score = score
    lines = [json.dumps({"id": 0, "caption": 1, "shortlist": 2, "within": ["v0", "new"]}),              # in front of the add: the id is not known yet
             json.dumps({"id": 1, "caption": 1, "shortlist": 2, "within_idx": [0, 4]}),
             json.dumps({"id": 2, "add_video": {"vid": "new", "features": feats("a.pth", 1.0)}}),
             json.dumps({"id": 3, "caption": 1, "shortlist": 2, "within": ["new", "v0"]}),
             json.dumps({"id": 4, "caption": 2, "shortlist": 1, "prefilter": 2, "within_idx": [4, 3, 1]})]
    out, summary = GR._serve(srv, lines, 5)
    assert [x["id"] for x in out] == [0, 1, 2, 3, 4]
    assert "within: unknown video id 'new'" in out[0]["error"] and "within_idx must hold indices in 0 .. 3" in out[1]["error"]
    assert out[2] == {"id": 2, "added": "new", "index": 4, "videos": 5}
    assert scored == [[(1, 2, None, [0, 4]), (2, 1, 2, [1, 3, 4])]]                # one pass behind the barrier, the new video in both sets
    assert out[3]["videos"] == ["v0", "new"] and out[3]["within"] == 2 and out[4]["within"] == 3 and out[4]["prefiltered"] == 2
    assert summary["errors"] == 2 and summary["videos_added"] == 1


# ---- 6. the one-shot command
def test_run_t2v_confines_every_query_to_the_set_and_reports_it():
    args = SR.get_args_parser().parse_args(["--query_ids", "1", "3", "--candidates", "tvg", "--resume", "x", "--topk", "2", "--shortlist", "3", "--prefilter", "4", "--within_ids", "f.txt",
                                            "--c"] + [str(x) for x in SH.C_BLEND])
    SR.check_args(args)
    vids = [f"v{j}" for j in range(N)]
    within = np.array([0, 2, 3, 5])
    s, g, passes = _gallery()
    out = []
    SR.run_t2v(g, vids, None, args, out.append, within)
    out = [json.loads(x) for x in out]
    assert [x["query"] for x in out] == ["caption:1", "caption:3"]
    assert s.within_calls == [([1], 4, False, 0.0, [[0, 2, 3, 5]]), ([3], 4, False, 0.0, [[0, 2, 3, 5]])] and s.first_calls == [] and s.gallery_calls == []
    s1, g1, _ = _gallery()
    for x, t in zip(out, (1, 3)):
        assert list(x) == ["query", "videos", "scores", "shortlisted", "prefiltered", "within"] and (x["shortlisted"], x["prefiltered"], x["within"]) == (3, 4, 4)
        (order, blended), = g1.search_requests([SearchRequest(t, shortlist=3, prefilter=4, within=within)], cpn=False, alpha=args.alpha, c=args.c, finetuned=True)
        assert x["videos"] == [vids[j] for j in order[:2]] and x["scores"] == [float(b) for b in blended[:2]] and set(x["videos"]) <= {"v0", "v2", "v3", "v5"}
    assert g.within_stats == {"queries": 2, "candidates": 8}
    assert SR.report_lines([("gallery", g)], None, g.shortlist_stats, g.prefilter_stats, g.within_stats)[-1] == 'within: {"queries": 2, "candidates": 8}'
    # without a set the run is what it was: no "within" in the answer, the whole-gallery stage 0
    s2, g2, _ = _gallery()
    plain = []
    SR.run_t2v(g2, vids, None, args, plain.append)
    assert all("within" not in json.loads(x) for x in plain) and s2.within_calls == [] and len(s2.first_calls) == 2 and g2.within_stats == {"queries": 0, "candidates": 0}
