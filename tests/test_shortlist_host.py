"""CPU: the shortlist's host side (blim_amd/pair_scorer.py: PairScorer.iter_tvg_gallery / tvg_gallery; blim_amd/gallery.py: GalleryIndex.shortlist /
search_requests, TextGalleryIndex.shortlist / rerank_shortlist; blim_amd/search.py: --candidates tvg, --shortlist, the serve field) -- the whole-gallery planner cuts a
text's videos at fixed places whatever shares the call, never splits a chunk over two calls, names one feature block per call and is _plan_tvg's plan where the cuts
coincide; the block's memo follows the weights version; the order is stable; mixed batches are one stage-1 pass and one VTG pass; rerank_requests gives what it gave.
Fakes as in tests/test_serve_host.py: no engine.  The GPU side is tests/test_shortlist_gpu.py."""
import json
import types

import numpy as np
import pytest
import torch

import test_gallery_host as GH
import test_host_logic as HL
import test_lazy_gallery_host as LZ
import test_serve_host as SH
from blim_amd import gallery as GL
from blim_amd import search as SR
from blim_amd.pair_scorer import SEG_MAX

N = 6


# ---- 1. the planner, on a real PairScorer over a model that records its projections
class _Model(HL._FakeModel):
    """tests/test_host_logic.py's planning model with feature rows that tell the videos and their clips apart, and a count of the projections."""

    def __init__(self, dims, tp):
        super().__init__(dims, tp)
        self.projected = 0

    def project(self, feat, tvg, cache=True):
        self.projected += 1
        clips, T, _ = feat.shape
        n = clips if tvg else clips * T
        return (float(feat.float().mean()) + torch.arange(n, dtype=torch.float32)[:, None] * torch.ones((1, self.dims.hidden_size))).to(torch.float16)


def _scorer(max_tokens=4096):
    dims, prob = SH._problem(N)
    sc = SH._scorer(dims, prob, range(N))
    sc.m = _Model(dims, prob.tvg_prefix_length)
    sc.engine = types.SimpleNamespace(weights_version=0, set_precise=lambda *a, **k: None)
    sc.max_tokens = max_tokens
    return sc


def _chunks(sc, plans):
    """[(position of the text, the videos of one merged sequence)] of a list of plans, and per plan the set of text positions it holds."""
    C = sc.num_clips
    out, per_plan = [], []
    for p in plans:
        outs = p.out_index[:, 0]
        lens = [n // (C - 1) for n, pl in zip(p.batch.seq_len.tolist(), p.batch.pfx_len.tolist()) if pl]
        assert sum(lens) == p.n_pairs == len(outs)
        at, mine = 0, set()
        for n in lens:
            part = outs[at:at + n]
            assert len({int(o) // N for o in part}) == 1                        # a merged sequence holds one text's videos
            out.append((int(part[0]) // N, [int(o) % N for o in part])); mine.add(int(part[0]) // N)
            at += n
        per_plan.append(mine)
    return out, per_plan


def test_a_text_alone_and_several_texts_are_plan_tvgs_plans_where_the_cuts_coincide():
    sc = _scorer()
    assert sc.gallery_chunk() == SEG_MAX // (sc.num_clips - 1) and sc.gallery_chunk() >= N
    for texts in ([2], [0, 2, 5], list(range(N))):
        got = list(sc.iter_tvg_gallery(texts))
        want = sc.plan_tvg(np.array([[j, i] for i in texts for j in range(N)]))
        assert len(got) == len(want) == 1
        assert GH.plan_difference(got[0], want[0]) is None                      # batch, tokens, rows, labels, feature rows, output slots: array for array
        assert got[0].out_index[:, 0].tolist() == list(range(len(texts) * N))
    assert list(sc.iter_tvg_gallery([])) == []


@pytest.mark.parametrize("max_tokens", [4096, 80, 60, 46])
def test_cuts_are_fixed_and_no_chunk_is_split_by_a_call_boundary(max_tokens):
    sc = _scorer(max_tokens)
    C = sc.num_clips
    texts = [0, 2, 5, 3]
    plens = [len(sc.tvg_split[i]) for i in texts]
    assert max(plens) + 4 * (C - 1) <= 46                                        # (46: one prompt and one chunk, nothing more)
    plans = list(sc.iter_tvg_gallery(texts, chunk=4))
    chunks, per_plan = _chunks(sc, plans)
    assert chunks == [(q, v) for q in range(len(texts)) for v in ([0, 1, 2, 3], [4, 5])]      # the same cuts whatever the calls hold
    assert (len(plans) == 1) == (max_tokens == 4096) and (max_tokens != 46 or len(plans) == 2 * len(texts))
    feats = sc.gallery_feats()
    for p, mine in zip(plans, per_plan):
        assert p.n_tokens <= max_tokens and p.feats is feats                     # ONE feature block, the same tensor in every call
        n_prompts = sum(1 for pl in p.batch.pfx_len.tolist() if pl == 0)
        assert n_prompts == len(mine)                                            # the prompt once per call and text
        assert p.kind == "tvg" and p.row_start is None and p.pfx_slot is None and p.n_rows == p.n_pairs * C
    # every pair's rows and tokens, whatever call it fell into: the prompt's last row, then its own C - 1 clip tokens naming rows j * C .. of the block
    for p in plans:
        rows, src, start, plen = p.rows.numpy().reshape(-1, C), p.src_index.numpy(), p.batch.seq_start.numpy(), p.batch.seq_len.numpy()
        pos, own = p.batch.positions.numpy(), (p.batch.own_start.numpy() if p.batch.own_start is not None else np.zeros(p.n_tokens, np.int32))
        last = {int(s + n - 1): int(n) for s, n, pl in zip(start, plen, p.batch.pfx_len.numpy()) if pl == 0}
        seq_of = np.repeat(np.arange(len(start)), plen)
        for r, o, lab in zip(rows, p.out_index[:, 0], p.labels.numpy()):
            q, j = int(o) // N, int(o) % N
            assert last[int(r[0])] == plens[q] and lab == sc.tvg_video_labels[j]
            assert r[1:].tolist() == list(range(r[1], r[1] + C - 1)) and src[r[1:]].tolist() == [-(1 + j * C + m) for m in range(C - 1)]
            assert pos[r[1:]].tolist() == [plens[q] + m for m in range(C - 1)]
            s = seq_of[r[1]]
            assert len(set(own[r[1:]].tolist())) == 1 and own[r[1]] == r[1] - start[s] and p.batch.pfx_len.numpy()[s] == plens[q]
            assert p.batch.pfx_start.numpy()[s] + plens[q] - 1 == r[0]
    # the same texts one by one and in another order: the same chunks per text
    for q, i in enumerate(texts):
        alone, _ = _chunks(sc, list(sc.iter_tvg_gallery([i], chunk=4)))
        assert alone == [(0, [0, 1, 2, 3]), (0, [4, 5])]


def test_the_planner_refuses_what_it_cannot_plan():
    sc = _scorer()
    longest = max(len(sc.tvg_split[i]) for i in range(N))
    sc.max_tokens = longest + 4 * (sc.num_clips - 1) - 1                         # one token short of the longest prompt and one chunk
    with pytest.raises(ValueError, match=f"max_tokens = {sc.max_tokens}"):
        list(sc.iter_tvg_gallery(range(N), chunk=4))
    sc.max_tokens += 1
    plans = list(sc.iter_tvg_gallery(range(N), chunk=4))
    assert N < len(plans) <= 2 * N and all(p.n_tokens <= sc.max_tokens for p in plans)
    assert _chunks(sc, plans)[0] == [(q, v) for q in range(N) for v in ([0, 1, 2, 3], [4, 5])]
    with pytest.raises(ValueError, match="chunk"):
        list(sc.iter_tvg_gallery([0], chunk=0))
    vtg_rows = SH._unpadded(*[getattr(SH._problem(N)[1], k) for k in ("vtg_ids", "vtg_labels", "vtg_masks")])
    late, = sc.add_texts([vtg_rows[1]]).tolist()
    with pytest.raises(ValueError, match=f"text {late} "):
        list(sc.iter_tvg_gallery([0, late]))


def test_the_feature_block_is_built_once_and_dropped_on_a_weights_or_layout_change():
    sc = _scorer()
    C = sc.num_clips
    f = sc.gallery_feats()
    n_proj = sc.m.projected
    assert tuple(f.shape) == (N * C, sc.m.dims.hidden_size) and n_proj == N
    for j in range(N):
        assert torch.equal(f[j * C:(j + 1) * C], sc.video_feat(j, True))        # laid out as video_feat lays out one video
    assert len({float(f[j * C, 0]) for j in range(N)}) == N
    list(sc.iter_tvg_gallery([0, 1])); list(sc.iter_tvg_gallery([3], chunk=4))
    assert sc.gallery_feats() is f and sc.m.projected == n_proj                  # planning projects nothing and builds nothing
    sc.engine.weights_version += 1
    g = sc.gallery_feats()
    assert g is not f and sc.gallery_feats() is g and next(iter(sc.iter_tvg_gallery([0]))).feats is g
    sc.split_tvg = True
    assert sc.gallery_feats() is not g
    sc.split_tvg = False


def test_tvg_gallery_returns_video_order_rows_per_asked_text():
    sc = _scorer(46)
    ran = []

    def run(plan):
        ran.append(plan)
        return torch.tensor([100.0 * (int(o) // N) + int(o) % N for o in plan.out_index[:, 0]])
    sc.run = run
    got = sc.tvg_gallery([5, 0, 5], chunk=4)
    assert got.dtype == np.float32 and got.shape == (3, N) and len(ran) == 4     # texts 0 and 5 planned once each, two calls each
    assert got.tolist() == [[100.0 + j for j in range(N)], [float(j) for j in range(N)], [100.0 + j for j in range(N)]]
    assert sc.tvg_gallery([], chunk=4).shape == (0, N)


# ---- 2. the index (tests/test_serve_host.py's fakes; a fake stage 1)
def _stage(j, i):
    """The fake's TVG score of (video j, text i): ties between videos on purpose."""
    return np.float32(-((int(j) * 5 + int(i)) % 4) / 2.0)


def _fake(n_videos=N, n_texts=5):
    s = SH._fake(GH._random_texts(n_texts), n_videos=n_videos)
    s.gallery_calls = []

    def tvg_gallery(texts, chunk=None):
        texts = np.asarray(texts, np.int64).reshape(-1)
        s._need_tvg(texts)
        s.gallery_calls.append(texts.tolist())
        return np.array([[_stage(j, i) for j in range(n_videos)] for i in texts], np.float32).reshape(len(texts), n_videos)
    s.tvg_gallery = tvg_gallery
    return s


def _parent_rerank_requests(g, requests, cpn=False, alpha=(0.0, 0.0), c=(1.0, 1.0, 1.0, 1.0), finetuned=False):
    """GalleryIndex.rerank_requests as it stood before the shortlist (one vtg_pairs pass, one PairScorer.tvg call, one prior lookup, _blend per request)."""
    reqs = [(int(t), np.asarray(cand, dtype=np.int64).reshape(-1), fs) for t, cand, fs in requests]
    pairs = np.concatenate([np.stack([cand, np.full(len(cand), t, dtype=np.int64)], axis=1) for t, cand, _ in reqs])
    ends = np.cumsum([len(cand) for _, cand, _ in reqs])
    ql = np.split(g.vtg_pairs(pairs), ends[:-1])
    t2v_cand = None
    if finetuned:
        g._tvg_state()
        has = np.array([g.s.tvg_split[t] is not None for t, _, _ in reqs])
        if c[0] != 1:
            g.s._need_tvg([t for t, _, _ in reqs])
        of = np.repeat(has, [len(cand) for _, cand, _ in reqs])
        t2v_cand = np.zeros(len(pairs), dtype=np.float32)
        if of.any():
            t2v_cand[of] = g.s.tvg(pairs[of])
        if cpn and of.any():
            prior = np.zeros(len(pairs))
            prior[of] = g._t2v_prior([t for (t, _, _), h in zip(reqs, has) if h], [cand for (_, cand, _), h in zip(reqs, has) if h])
            t2v_cand = t2v_cand - alpha[0] * prior
        t2v_cand = np.split(t2v_cand, ends[:-1])
    out = []
    for n, (t, cand, fs) in enumerate(reqs):
        fs = np.zeros(cand.shape) if fs is None else np.asarray(fs).reshape(cand.shape)
        order, blended = g._blend(cand[None], ql[n][None], np.zeros((1, len(cand))) if t2v_cand is None else t2v_cand[n][None], fs[None], c)
        out.append((order[0], blended[0]))
    return out


def _same_results(a, b):
    assert len(a) == len(b)
    for (o1, b1), (o2, b2) in zip(a, b):
        assert o1.dtype == o2.dtype and b1.dtype == b2.dtype and np.array_equal(o1, o2) and np.array_equal(b1, b2)


@pytest.mark.parametrize("finetuned", [False, True])
@pytest.mark.parametrize("cpn", [False, True])
def test_rerank_requests_gives_what_it_gave(finetuned, cpn):
    more = dict(cpn=cpn, alpha=(0.8, 0.3), c=SH.C_BLEND, finetuned=finetuned)

    def run(fn):
        s = _fake()
        g = GH._gallery(s, {0: 0, 2: 1, 5: 2})
        passes = SH._scoring(g)
        no_tvg, = s.add_texts([SH._vtg_row([1, 1], [2, 2], [3])]).tolist()
        reqs = SH._requests(np.random.RandomState(3), [0, 3, 4, 1], N, [1, 3, 6, 2, 1, 5])
        res = fn(g, reqs, **more)
        res += fn(g, reqs[:2] + [(no_tvg, [1, 4], None)], **dict(more, c=(1.0, 0.5, 0.7, 0.5)))      # c0 = 1: a text without a TVG row keeps a zero term
        return res, list(s.tvg_calls), len(passes), s.gallery_calls
    new, old = run(lambda g, r, **kw: g.rerank_requests(r, **kw)), run(_parent_rerank_requests)
    _same_results(new[0], old[0])
    assert new[1:] == old[1:] and new[2] == 2 and new[3] == []                   # the same scorer calls, the same passes, no stage 1
    s = _fake()
    g = GH._gallery(s, {})
    SH._scoring(g)
    assert g.rerank_requests([]) == [] and g.search_requests([]) == []
    with pytest.raises(ValueError, match="no candidates"):
        g.rerank_requests([(0, np.zeros(0, np.int64), None)])


def test_ties_go_to_the_lower_video_index_and_k_is_clipped():
    s = _fake()
    g = GH._gallery(s, {})
    SH._scoring(g)
    row = np.array([_stage(j, 1) for j in range(N)])
    assert len(set(row.tolist())) < N                                            # the fake ties
    want = sorted(range(N), key=lambda j: (-row[j], j))
    cand, stage = g.shortlist([1, 3], 4)
    assert cand.shape == stage.shape == (2, 4) and cand[0].tolist() == want[:4] and stage[0].tolist() == row[want[:4]].tolist()
    cand, stage = g.shortlist([1], 100)
    assert cand.shape == (1, N) and cand[0].tolist() == want                     # k clipped to N
    assert g._best(np.array([0.5, 1.0, 0.5, 1.0, -1.0]), 3)[0].tolist() == [1, 3, 0]
    cand, stage = g.shortlist([1], 3, cpn=True, alpha=(0.8, 0.0))                # with cpn: minus alpha[0] x the prior, the term of rerank()'s blend
    full = row - 0.8 * g._t2v_prior([1], np.arange(N)[None])[0]
    o = np.argsort(-full, kind="stable")[:3]
    assert cand[0].tolist() == o.tolist() and np.array_equal(stage[0], full[o])
    with pytest.raises(ValueError, match="k = 0"):
        g.shortlist([1], 0)
    no_tvg, = s.add_texts([SH._vtg_row([1, 1], [2, 2], [3])]).tolist()
    with pytest.raises(ValueError, match=f"text {no_tvg} "):
        g.shortlist([0, no_tvg], 2)
    assert g.shortlist_stats == {"queries": 4, "passes": 3, "pairs": 4 * N}      # ([1, 3], [1], [1]; a refused call counts nothing)


@pytest.mark.parametrize("cpn", [False, True])
def test_a_mixed_batch_is_one_stage_1_pass_and_one_vtg_pass_and_equals_separate_calls(cpn):
    more = dict(cpn=cpn, alpha=(0.8, 0.3), c=SH.C_BLEND, finetuned=True)
    rng = np.random.RandomState(5)
    batch = [(0, None, None, 3), (2, rng.permutation(N)[:4], rng.rand(4).astype(np.float32), None), (3, None, None, N + 5), (1, [4, 1], None, None), (4, None, None, 1)]

    def fresh(lazy):
        s = _fake()
        g = LZ._lazy(s, 3) if lazy else GH._gallery(s, {0: 0, 3: 1})             # (a lazy index with fewer slots than the pass has keys)
        return s, g, SH._scoring(g)
    for lazy in (False, True):
        b = batch
        s, g, passes = fresh(lazy)
        got = g.search_requests(b, **more)
        assert len(passes) == 1 and s.gallery_calls == [[t for t, _, _, K in b if K is not None]]      # ONE stage-1 pass, ONE vtg_pairs pass
        assert [call for call in s.tvg_calls if not call[1]] == [(6, False)]                           # the TVG term of the explicit requests' six pairs only
        s1, g1, _ = fresh(lazy)
        alone = [g1.search_requests([r], **more)[0] for r in b]
        _same_results(got, alone)
        s2, g2, _ = fresh(lazy)
        _same_results([got[1], got[3]], g2.rerank_requests([b[1][:3], b[3][:3]], **more))             # the explicit requests: rerank_requests, exactly
        for (t, _, _, K), (order, blended) in zip(b, got):
            if K is None:
                continue
            s3, g3, _ = fresh(lazy)
            cand, stage = g3.shortlist([t], K, cpn=cpn, alpha=more["alpha"])
            assert sorted(order.tolist()) == sorted(cand[0].tolist()) and len(order) == min(K, N)
            ql = np.array([SH._score(j, t) for j in cand[0]])
            want = SH.C_BLEND[2] * (SH.C_BLEND[0] * ql + (1 - SH.C_BLEND[0]) * stage[0]) + (1 - SH.C_BLEND[2]) * np.zeros(len(ql))
            o = np.argsort(-want, kind="stable")
            assert np.array_equal(order, cand[0][o]) and np.array_equal(blended, want[o])              # stage 1's value IS the TVG term; the first stage is zero


def test_search_requests_refuses_what_it_cannot_score():
    s = _fake()
    g = GH._gallery(s, {})
    SH._scoring(g)
    for bad, msg in (((0, [1], None, 2), "one of the two"), ((0, None, None, None), "one of the two"), ((0, None, None, 0), "positive integer"),
                     ((0, None, None, 2.5), "positive integer"), ((0, None, None, True), "positive integer"), ((0, None, [0.5, 0.1], 2), "first stage"),
                     ((0, [], None, None), "no candidates")):
        with pytest.raises(ValueError, match=msg):
            g.search_requests([(1, [0], None, None), bad], finetuned=True)
    with pytest.raises(ValueError, match="finetuned=False"):
        g.search_requests([(0, None, None, 2)], finetuned=False)
    assert s.gallery_calls == [] and s.tvg_calls == []


def test_text_gallery_shortlist_is_one_pass_per_query_video_in_stable_order():
    s = _fake()
    tg = GL.TextGalleryIndex(s)
    asked = []

    def tvg_pairs(pairs):
        asked.append(np.asarray(pairs).tolist())
        return np.array([_stage(j, i) for j, i in pairs], np.float32)
    tg.tvg_pairs = tvg_pairs
    tg.vtg_pairs = lambda pairs: np.array([SH._score(j, i) for j, i in pairs], np.float32)
    cand, stage = tg.shortlist([4, 1], 3)
    assert asked == [[[4, i] for i in range(5)], [[1, i] for i in range(5)]]     # every text has one video in each pass
    for q, v in enumerate((4, 1)):
        row = np.array([_stage(v, i) for i in range(5)])
        o = np.argsort(-row, kind="stable")[:3]
        assert cand[q].tolist() == o.tolist() and stage[q].tolist() == row[o].tolist()
    assert tg.shortlist([0], 99)[0].shape == (1, 5)
    c = (0.6, 0.5, 0.7, 0.5)
    order, blended = tg.rerank_shortlist([4], 3, c=c)
    o1, b1 = tg.rerank([4], cand[:1], c=c, finetuned=True)                        # the fake's tvg_pairs is deterministic: the reused term is the recomputed one
    assert np.array_equal(order, o1) and np.array_equal(blended, b1) and blended.dtype == b1.dtype


# ---- 3. the command's arguments
@pytest.mark.parametrize("argv,msg", [
    (["--query_ids", "0", "--candidates", "tvg"], "--candidates tvg"),
    (["--query_ids", "0", "--shortlist", "8", "--resume", "x"], "--shortlist"),
    (["--query_ids", "0", "--candidates", "all", "--shortlist", "8", "--resume", "x"], "--shortlist"),
    (["--query_ids", "0", "--candidates", "tvg", "--shortlist", "0", "--resume", "x"], "--shortlist"),
    (["--query_ids", "0", "--candidates", "tvg", "--topk", "0", "--resume", "x"], "--shortlist"),
    (["--serve", "--candidates", "tvg"], "--candidates tvg"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg"], "--candidates tvg"),
    (["--query", "a dog runs", "--resume", "x"], "candidates all"),               # the existing refusal, word for word
])
def test_check_args_refusals(argv, msg):
    with pytest.raises(SystemExit, match=msg):
        SR.check_args(SR.get_args_parser().parse_args(argv))


def test_check_args_accepts_the_shortlist():
    p = SR.get_args_parser()
    assert p.parse_args(["--query_ids", "0"]).shortlist is None
    for argv in (["--query_ids", "0", "--candidates", "tvg", "--resume", "x"], ["--query", "a dog", "--candidates", "tvg", "--resume", "x", "--shortlist", "64"],
                 ["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--resume", "x"], ["--serve", "--candidates", "tvg", "--resume", "x", "--shortlist", "4"],
                 ["--serve", "--candidates", "all"]):
        SR.check_args(p.parse_args(argv))
    a = p.parse_args(["--query_ids", "0", "--candidates", "tvg", "--resume", "x", "--topk", "7"])
    assert SR.shortlist_k(a) == 7
    a.shortlist = 64
    assert SR.shortlist_k(a) == 64
    with pytest.raises(SystemExit, match="free-text queries have no first-stage row: use --candidates all"):
        SR.check_args(p.parse_args(["--query", "a dog runs"]))


# ---- 4. serve
def _server(argv, finetuned=True):
    s = _fake(n_texts=4)
    g = GH._gallery(s, {0: 0, 3: 1})
    passes = SH._scoring(g)
    args = SR.get_args_parser().parse_args(["--serve"] + list(argv))
    SR.check_args(args)
    iv2 = np.random.RandomState(1).rand(4, N).astype(np.float32)
    return SR.Server(g, [f"v{j}" for j in range(N)], 4, iv2, args, finetuned=finetuned), passes


def test_parse_reads_the_shortlist_field():
    srv, _ = _server(["--candidates", "all", "--resume", "x", "--c", "0.5", "0", "1", "0"])
    r = srv.parse(json.dumps({"id": 1, "caption": 2, "shortlist": 3}))
    assert r["shortlist"] == 3 and r["cand"] is None and r["fs"] is None and r["text"] == 2
    r = srv.parse(json.dumps({"id": 2, "rows": SH.ROWS_A}))                      # under `all`: the whole gallery, as before
    assert r["shortlist"] is None and r["cand"].tolist() == list(range(N))
    for req, msg in (({"caption": 0, "shortlist": 2, "candidates": ["v1"]}, "not both"), ({"caption": 0, "shortlist": 2, "candidate_idx": [1]}, "not both"),
                     ({"caption": 0, "shortlist": 0}, "positive integer"), ({"caption": 0, "shortlist": "4"}, "positive integer"),
                     ({"caption": 0, "shortlist": 2.0}, "positive integer"), ({"caption": 0, "shortlist": True}, "positive integer"),
                     ({"rows": SH.ROWS_B, "shortlist": 2}, "TVG row"), ({"caption": 0, "shortlist": 2, "first_stage": [0.1, 0.2]}, "first_stage")):
        with pytest.raises(SR.BadRequest, match=msg) as e:
            srv.parse(json.dumps(dict(req, id=7)))
        assert e.value.id == 7
    zero, _ = _server(["--candidates", "all"], finetuned=False)
    with pytest.raises(SR.BadRequest, match="fine-tuned"):
        zero.parse(json.dumps({"caption": 0, "shortlist": 2}))
    tvg, _ = _server(["--candidates", "tvg", "--resume", "x", "--topk", "2"])
    assert tvg.parse(json.dumps({"rows": SH.ROWS_A}))["shortlist"] == 2          # --candidates tvg: a query without candidates takes the shortlist
    assert tvg.parse(json.dumps({"caption": 1}))["shortlist"] == 2
    assert tvg.parse(json.dumps({"caption": 1, "shortlist": 5}))["shortlist"] == 5
    r = tvg.parse(json.dumps({"caption": 1, "candidate_idx": [3, 1]}))
    assert r["shortlist"] is None and r["cand"].tolist() == [3, 1]
    iv2, _ = _server(["--candidates", "iv2", "--resume", "x"])
    with pytest.raises(SR.BadRequest, match="first-stage"):                       # under iv2: as before
        iv2.parse(json.dumps({"rows": SH.ROWS_A}))


@pytest.mark.parametrize("B", [1, 3, 64])
def test_serve_hands_mixed_batches_to_search_requests(B):
    lines = [json.dumps({"id": 0, "caption": 1, "shortlist": 3}),
             json.dumps({"id": 1, "rows": SH.ROWS_A, "candidate_idx": [4, 0, 2], "first_stage": [0.1, 0.9, 0.5]}),
             json.dumps({"id": 2, "caption": 0, "shortlist": 2, "candidates": ["v1"]}),
             json.dumps({"id": 3, "rows": SH.ROWS_A, "shortlist": 4, "topk": 2}),
             json.dumps({"id": 4, "rows": SH.ROWS_B, "shortlist": 2}),
             json.dumps({"id": 5, "caption": 3}),
             json.dumps({"id": 6, "caption": 2, "shortlist": 100})]
    runs = {}
    for b in (1, B):
        srv, passes = _server(["--candidates", "all", "--resume", "x", "--c", "0.5", "0", "1", "0"])
        out = []
        summary = SR.serve(iter(lines), out.append, srv, batch_queries=b, batch_wait_ms=60000.0)
        runs[b] = ([json.loads(x) for x in out], summary, len(passes), srv)
    out, summary, n_passes, srv = runs[B]
    assert out == runs[1][0]                                                      # whatever the batch
    assert [x["id"] for x in out] == list(range(7)) and [n for n, x in enumerate(out) if "error" in x] == [2, 4]
    assert "not both" in out[2]["error"] and "TVG row" in out[4]["error"] and summary["errors"] == 2
    assert set(out[0]) == {"id", "query", "videos", "scores", "shortlisted"} and out[0]["shortlisted"] == 3 and len(out[0]["videos"]) == 3
    assert set(out[1]) == set(out[5]) == {"id", "query", "videos", "scores"} and len(out[5]["videos"]) == N
    assert out[3]["shortlisted"] == 4 and len(out[3]["videos"]) == 2 and out[6]["shortlisted"] == 100 and len(out[6]["videos"]) == N
    for x in out:
        assert "error" in x or x["scores"] == sorted(x["scores"], reverse=True)
    row = np.array([_stage(j, 1) for j in range(N)])
    assert sorted(out[0]["videos"]) == sorted(f"v{j}" for j in np.argsort(-row, kind="stable")[:3])
    batches_with = lambda which: sum(1 for a in range(0, 7, B) if any(n in which for n in range(a, min(a + B, 7))))
    assert n_passes == batches_with((0, 1, 3, 5, 6)) and len(srv.s.gallery_calls) == batches_with((0, 3, 6))      # one VTG pass and at most one stage-1 pass per batch
    assert srv.gal.shortlist_stats["queries"] == 3 and srv.gal.shortlist_stats["pairs"] == 3 * N
    assert SR._shortlist_line(srv.gal.shortlist_stats) == {"queries": 3, "stage1_passes": len(srv.s.gallery_calls), "stage1_pairs": 3 * N}
