"""CPU: the prefilter's host side (blim_amd/pair_scorer.py: PairScorer.iter_tvg_first / tvg_first; blim_amd/gallery.py: GalleryIndex.prefilter and the fifth request
field of search_requests; blim_amd/search.py: --prefilter, the serve field) -- the planner packs each distinct caption prompt once and, with cpn, each prior head once
per call and each prior key as the one token _plan_tvg's prior segment opens with; calls are cut at max_tokens with a prompt and its prior in one call; vocabulary
entries go back to videos through the inverse of the labels; prefiltered requests share one stage-0 pass, one PairScorer.tvg call and the batch's one VTG pass;
4-tuples give what they gave.  Fakes as in tests/test_shortlist_host.py: no engine.  The GPU side is tests/test_prefilter_gpu.py."""
import json

import numpy as np
import pytest
import torch

import test_gallery_host as GH
import test_lazy_gallery_host as LZ
import test_serve_host as SH
import test_shortlist_host as SL
from blim_amd import gallery as GL
from blim_amd import search as SR

N = SL.N


# ---- 1. the planner, on a real PairScorer
def _seqs(p):
    """[(tokens, positions, key_visible, pfx_start, pfx_len)] of a plan's sequences."""
    src, pos, vis = p.src_index.numpy(), p.batch.positions.numpy(), p.batch.key_visible.numpy()
    out = []
    for s0, n, ps, pl in zip(p.batch.seq_start.tolist(), p.batch.seq_len.tolist(), p.batch.pfx_start.tolist(), p.batch.pfx_len.tolist()):
        out.append((src[s0:s0 + n].tolist(), pos[s0:s0 + n].tolist(), vis[s0:s0 + n].tolist(), ps, pl))
    return out


def _with_twin(sc):
    """The scorer with one more text whose caption prompt is text 2's, byte for byte (another VTG row)."""
    twin, = sc.add_texts([sc.vtg_rows[4]], [sc.tvg_rows[2]]).tolist()
    assert np.array_equal(sc.tvg_split[twin], sc.tvg_split[2])
    return twin


def test_each_distinct_prompt_is_packed_once_and_its_row_is_its_last_token():
    sc = SL._scorer()
    twin = _with_twin(sc)
    texts = [2, 0, twin, 5, 0]
    plan, = sc.iter_tvg_first(texts)
    assert plan.kind == "tvg_first" and plan.prior_rows is None and plan.row_start is None and plan.pfx_slot is None
    seqs = _seqs(plan)
    distinct = [2, 0, 5]                                                           # in order of first appearance
    assert len(seqs) == 3 and plan.n_pairs == plan.n_rows == 3 and plan.n_tokens == sum(len(sc.tvg_split[i]) for i in distinct)
    rows = plan.rows.numpy().tolist()
    for (toks, pos, vis, ps, pl), i, row, s0 in zip(seqs, distinct, rows, plan.batch.seq_start.tolist()):
        pr = sc.tvg_split[i]
        assert toks == pr.tolist() and pos == list(range(len(pr))) and vis == [1] * len(pr) and pl == 0 and row == s0 + len(pr) - 1
    assert [o.tolist() for o in plan.out_index] == [[0, 2], [1, 4], [3]]           # the twin rides on text 2's row, the repeated text on its own
    assert plan.labels.numpy().tolist() == [-1, -1, -1]
    assert list(sc.iter_tvg_first([])) == []
    vtg_rows = SH._unpadded(*[getattr(SH._problem(N)[1], k) for k in ("vtg_ids", "vtg_labels", "vtg_masks")])
    late, = sc.add_texts([vtg_rows[1]]).tolist()
    with pytest.raises(ValueError, match=f"text {late} "):
        list(sc.iter_tvg_first([0, late]))


@pytest.mark.parametrize("tp_more", [0, 100])
def test_the_prior_is_the_first_token_of_plan_tvgs_prior_segment(tp_more):
    """tp as the problem has it (the prompts' last tokens lie at or beyond it: hidden as keys) and tp beyond every prompt (the last token lies inside the head: visible)."""
    sc = SL._scorer()
    sc.m.tvg_prefix_length += tp_more
    tp = sc.m.tvg_prefix_length
    twin = _with_twin(sc)
    texts = [2, 0, twin, 5, 3]
    plan, = sc.iter_tvg_first(texts, cpn=True)
    seqs = _seqs(plan)
    keys = list(dict.fromkeys((sc.tvg_split[i][:tp].tobytes(), len(sc.tvg_split[i]), int(sc.tvg_split[i][-1])) for i in texts))
    heads = list(dict.fromkeys(k[0] for k in keys))
    prompts = list(dict.fromkeys(sc.tvg_split[i].tobytes() for i in texts))
    assert len(seqs) == len(heads) + len(keys) + len(prompts) and len(prompts) == 4
    assert plan.n_rows == len(prompts) + len(keys) and plan.n_pairs == len(prompts) and len(plan.prior_rows) == len(keys)
    start = plan.batch.seq_start.tolist()
    seq_at = {s0: q for q, s0 in enumerate(start)}
    side = set()
    for row, key in zip(plan.prior_rows.numpy().tolist(), keys):
        toks, pos, vis, ps, pl = seqs[seq_at[row]]
        hb, plen, last = key
        assert toks == [last] and pos == [plen - 1] and vis == [1 if plen - 1 < tp else 0]
        side.add(vis[0])
        assert pl == len(np.frombuffer(hb, np.int64)) and seqs[seq_at[ps]][0] == np.frombuffer(hb, np.int64).tolist() and seqs[seq_at[ps]][4] == 0
    assert side == ({1} if tp_more else {0})
    # each prompt row names its prior row
    po = plan.labels.numpy().tolist()
    for row, at, outs in zip(plan.rows.numpy().tolist(), po, plan.out_index):
        i = texts[int(outs[0])]
        pr = sc.tvg_split[i]
        assert keys[at] == (pr[:tp].tobytes(), len(pr), int(pr[-1]))
    # the same token, position, visibility and prefix as the first token of _plan_tvg's prior segment of any pair of the text
    for i in (0, 3):
        ref, = sc.plan_tvg(np.array([[1, i]]), cpn=True)
        rs = _seqs(ref)
        assert len(rs) == 2 and rs[0][4] == 0
        pr = sc.tvg_split[i]
        at = keys.index((pr[:tp].tobytes(), len(pr), int(pr[-1])))
        mine = seqs[seq_at[plan.prior_rows.numpy().tolist()[at]]]
        assert (rs[1][0][0], rs[1][1][0], rs[1][2][0], rs[1][4]) == (mine[0][0], mine[1][0], mine[2][0], mine[4])
        assert rs[0][0] == seqs[seq_at[mine[3]]][0] and ref.rows.numpy()[0] == ref.batch.seq_start.numpy()[1]


@pytest.mark.parametrize("cpn", [False, True])
def test_calls_are_cut_at_max_tokens_and_a_prompt_shares_its_priors_call(cpn):
    sc = SL._scorer()
    tp = sc.m.tvg_prefix_length
    texts = list(range(N))
    longest = max(len(sc.tvg_split[i]) for i in texts)
    whole, = sc.iter_tvg_first(texts, cpn=cpn)
    sc.max_tokens = 2 * longest + tp + 2                                           # two prompts with their priors at the most
    plans = list(sc.iter_tvg_first(texts, cpn=cpn))
    assert 1 < len(plans) <= N and all(p.n_tokens <= sc.max_tokens for p in plans)
    assert sorted(int(o) for p in plans for outs in p.out_index for o in outs) == texts
    for p in plans:
        seqs = _seqs(p)
        start = {s0: q for q, s0 in enumerate(p.batch.seq_start.tolist())}
        if cpn:
            heads = [s for s in seqs if s[4] == 0 and len(s[0]) == tp and not any(len(sc.tvg_split[i]) == tp for i in texts)]
            assert len(heads) == 1                                                 # the shared head once per call
            for row, at, outs in zip(p.rows.numpy().tolist(), p.labels.numpy().tolist(), p.out_index):
                pr = sc.tvg_split[texts[int(outs[0])]]
                prior = seqs[start[p.prior_rows.numpy().tolist()[at]]]
                assert prior[0] == [int(pr[-1])] and prior[1] == [len(pr) - 1]     # ... and a prompt's prior row lies in the prompt's own call
        else:
            assert p.prior_rows is None
    assert sum(p.n_pairs for p in plans) == whole.n_pairs == N


def test_vocabulary_entries_go_back_to_videos_through_the_inverse_of_the_labels():
    sc = SL._scorer()
    sc.n_vocab = N
    perm = np.array([3, 0, 5, 1, 4, 2], np.int32)
    sc.tvg_video_labels = perm                                                     # video j is vocabulary entry perm[j]
    ran = []

    def run(plan, k=1, alpha=0.0, full=False):
        ran.append((plan, k, alpha, full))
        n = plan.n_pairs
        idx = torch.stack([(torch.arange(k) + r) % N for r in range(n)]).to(torch.int32)          # vocabulary entries
        val = torch.stack([-(torch.arange(k, dtype=torch.float32) + 10 * r) for r in range(n)])
        lp = torch.stack([torch.arange(N, dtype=torch.float32) + 100 * r for r in range(n)])       # by vocabulary entry
        return (idx, val, lp) if full else (idx, val)
    sc.run = run
    twin = _with_twin(sc)
    idx, val, lp = sc.tvg_first([2, 0, twin], 3, full=True)
    inv = np.argsort(perm)
    assert idx.dtype == np.int64 and val.dtype == np.float32 and idx.shape == val.shape == (3, 3) and lp.shape == (3, N)
    assert idx.tolist() == [inv[[0, 1, 2]].tolist(), inv[[1, 2, 3]].tolist(), inv[[0, 1, 2]].tolist()]      # rows 0 (texts 2 and its twin) and 1
    assert val[1].tolist() == [-10.0, -11.0, -12.0] and np.array_equal(val[0], val[2])
    assert lp[0].tolist() == [float(perm[j]) for j in range(N)] and lp[1].tolist() == [100.0 + perm[j] for j in range(N)]     # by VIDEO index
    assert len(ran) == 1 and ran[0][1:] == (3, 0.0, True)
    idx2, val2 = sc.tvg_first([0], 2, cpn=True, alpha=0.4)
    assert ran[-1][1:] == (2, 0.4, False) and ran[-1][0].prior_rows is not None and idx2.shape == (1, 2)
    for k in (0, N + 1):
        with pytest.raises(ValueError, match="outside 1"):
            sc.tvg_first([0], k)
    sc.vocab_version += 1                                                          # (the memo follows the vocabulary)
    sc.tvg_video_labels = np.array([0, 1, 2, 3, 4, 4], np.int32)
    with pytest.raises(ValueError, match="permutation"):
        sc.tvg_first([0], 2)
    sc.vocab_version += 1
    sc.tvg_video_labels = np.arange(N, dtype=np.int32)
    sc.n_vocab = N + 1                                                             # an entry no video names
    with pytest.raises(ValueError, match="permutation"):
        sc.tvg_first([0], 2)


# ---- 2. the index (tests/test_shortlist_host.py's fakes and a fake stage 0)
def _first(j, i):
    """The fake's clip-0 value of (video j, text i): ties between videos on purpose."""
    return np.float32(-((int(j) * 3 + int(i) * 5) % 7) / 4.0)


def _fake(n_videos=N, n_texts=5):
    s = SL._fake(n_videos=n_videos, n_texts=n_texts)
    s.first_calls = []

    def tvg_first(texts, k, cpn=False, alpha=0.0, full=False):
        texts = np.asarray(texts, np.int64).reshape(-1)
        s._need_tvg(texts)
        s.first_calls.append((texts.tolist(), int(k), bool(cpn), float(alpha)))
        rows = np.array([[_first(j, i) - (np.float32(alpha) * _first(j, 0) if cpn else 0) for j in range(n_videos)] for i in texts], np.float32).reshape(len(texts), n_videos)
        idx = np.stack([np.argsort(-r, kind="stable")[:k] for r in rows]).astype(np.int64)
        return idx, np.take_along_axis(rows, idx, 1)
    s.tvg_first = tvg_first
    return s


def _kept(t, K0, cpn, alpha):
    row = np.array([_first(j, t) - (np.float32(alpha[0]) * _first(j, 0) if cpn else 0) for j in range(N)], np.float32)
    return np.sort(np.argsort(-row, kind="stable")[:min(K0, N)])


def test_prefilter_keeps_the_first_k0_sorted_ascending_and_counts():
    s = _fake()
    g = GH._gallery(s, {})
    SH._scoring(g)
    kept = g.prefilter([1, 3, 1], 4)
    assert kept.dtype == np.int64 and kept.shape == (3, 4) and s.first_calls == [([1, 3, 1], 4, False, 0.0)]
    for row, t in zip(kept, (1, 3, 1)):
        assert row.tolist() == _kept(t, 4, False, (0, 0)).tolist()
    assert g.prefilter([2], 100, cpn=True, alpha=(0.8, 0.3)).tolist() == [list(range(N))]           # K0 clipped to N
    assert s.first_calls[-1] == ([2], N, True, 0.8)
    assert g.prefilter_stats == {"queries": 4, "passes": 2, "rows": 3, "kept": 3 * 4 + N}
    assert g.shortlist_stats == {"queries": 0, "passes": 0, "pairs": 0}
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="positive integer"):
            g.prefilter([1], bad)
    no_tvg, = s.add_texts([SH._vtg_row([1, 1], [2, 2], [3])]).tolist()
    with pytest.raises(ValueError, match=f"text {no_tvg} "):
        g.prefilter([0, no_tvg], 2)
    assert g.prefilter_stats["passes"] == 2                                        # a refused call counts nothing


@pytest.mark.parametrize("cpn", [False, True])
def test_a_prefiltered_request_is_the_composition_of_the_public_calls_with_exact_call_counts(cpn):
    alpha, c = (0.8, 0.3), SH.C_BLEND
    more = dict(cpn=cpn, alpha=alpha, c=c, finetuned=True)
    rng = np.random.RandomState(5)
    batch = [(0, None, None, 2, 4), (2, rng.permutation(N)[:4], rng.rand(4).astype(np.float32), None), (3, None, None, 3), (1, None, None, 3, 5), (4, None, None, 1, N + 9),
             (1, [4, 1], None, None, None), (2, None, None, 2, None)]

    def fresh(lazy):
        s = _fake()
        g = LZ._lazy(s, 3) if lazy else GH._gallery(s, {0: 0, 3: 1})
        return s, g, SH._scoring(g)
    for lazy in (False, True):
        s, g, passes = fresh(lazy)
        got = g.search_requests(batch, **more)
        assert len(passes) == 1                                                    # ONE vtg_pairs pass for the whole batch
        assert s.first_calls == [([0, 1, 4], N, cpn, 0.8)]                         # ONE stage-0 pass, at the largest K0 (clipped to N)
        assert s.gallery_calls == [[3, 2]]                                         # the plain shortlist requests: their own whole-gallery stage 1, once
        likelihood = [call for call in s.tvg_calls if not call[1]]
        assert sorted(likelihood) == sorted([(4 + 5 + N, False), (4 + 2, False)])  # ONE TVG call over the kept pairs; one over the explicit requests' pairs
        assert g.prefilter_stats == {"queries": 3, "passes": 1, "rows": 3, "kept": 4 + 5 + N}
        assert g.shortlist_stats == {"queries": 2, "passes": 1, "pairs": 2 * N}
        # each request alone: the same answer, bit for bit
        s1, g1, _ = fresh(lazy)
        SL._same_results(got, [g1.search_requests([r], **more)[0] for r in batch])
        # 4-tuples (and a fifth field of None) give what they gave
        s2, g2, _ = fresh(lazy)
        four = [r[:4] for r in batch if len(r) == 4 or r[4] is None]
        SL._same_results([x for x, r in zip(got, batch) if len(r) == 4 or r[4] is None], g2.search_requests(four, **more))
        assert s2.first_calls == []
        # the composition: prefilter -> PairScorer.tvg over the kept pairs (- alpha x prior) -> _best K -> vtg_pairs -> _blend
        for (t, _, _, K, K0), (order, blended) in [(r, x) for r, x in zip(batch, got) if len(r) == 5 and r[4] is not None]:
            s3, g3, _ = fresh(lazy)
            cand0 = g3.prefilter([t], K0, cpn=cpn, alpha=alpha)[0]
            assert cand0.tolist() == _kept(t, K0, cpn, alpha).tolist()
            pairs = np.stack([cand0, np.full(len(cand0), t)], axis=1)
            term = s3.tvg(pairs)
            if cpn:
                term = term - alpha[0] * g3._t2v_prior([t], [cand0])
            keep, stage = g3._best(term, K)
            cand = cand0[keep]
            ql = g3.vtg_pairs(np.stack([cand, np.full(len(cand), t)], axis=1))
            o, b = g3._blend(cand[None], ql[None], stage[None], np.zeros((1, len(cand))), c)
            assert np.array_equal(order, o[0]) and np.array_equal(blended, b[0]) and len(order) == min(K, N)
    # with K0 = N the kept set is the best K of PairScorer.tvg over all N
    s, g, _ = fresh(False)
    (order, _), = g.search_requests([(3, None, None, 3, N)], **more)
    full = s.tvg(np.stack([np.arange(N), np.full(N, 3)], axis=1))
    if cpn:
        full = full - alpha[0] * g._t2v_prior([3], [np.arange(N)])
    assert sorted(order.tolist()) == sorted(np.argsort(-full, kind="stable")[:3].tolist())


def test_search_requests_refuses_bad_prefilters_and_keeps_its_refusals(monkeypatch):
    s = _fake()
    g = GH._gallery(s, {})
    SH._scoring(g)
    for bad, msg in (((0, None, None, 3, 2), "below the shortlist's K = 3"), ((0, None, None, 2, 0), "positive integer"), ((0, None, None, 2, 2.5), "positive integer"),
                     ((0, None, None, 2, True), "positive integer"), ((0, [1, 2], None, None, 3), "needs its K"), ((0, None, None, None, 3), "needs its K"),
                     ((0, [1], None, 2, 4), "one of the two"), ((0, None, None, 0, 4), "positive integer"), ((0, None, [0.5], 2, 4), "first stage"),
                     ((0, [1], None, 2), "one of the two"), ((0, [], None, None), "no candidates")):
        with pytest.raises(ValueError, match=msg):
            g.search_requests([(1, [0], None, None), bad], finetuned=True)
    with pytest.raises(ValueError, match="finetuned=False"):
        g.search_requests([(0, None, None, 2, 4)], finetuned=False)
    monkeypatch.setattr(GL, "TVG_RANK_MAX_K", 4)                                   # (a gallery of more than 1024 videos, in small)
    with pytest.raises(ValueError, match="BLIM_TVG_RANK_MAX_K"):
        g.search_requests([(0, None, None, 2, 5)], finetuned=True)
    with pytest.raises(ValueError, match="BLIM_TVG_RANK_MAX_K"):
        g.prefilter([0], 100)                                                      # clipped to N = 6, still above
    g.search_requests([(0, None, None, 2, 4)], finetuned=True)
    assert s.first_calls == [([0], 4, False, 0.0)] and s.gallery_calls == []


# ---- 3. the command's arguments
@pytest.mark.parametrize("argv,msg", [
    (["--query_ids", "0", "--prefilter", "8", "--resume", "x"], "--prefilter"),
    (["--query_ids", "0", "--candidates", "all", "--prefilter", "8", "--resume", "x"], "--prefilter"),
    (["--query_ids", "0", "--candidates", "tvg", "--prefilter", "0", "--resume", "x"], "--prefilter"),
    (["--query_ids", "0", "--candidates", "tvg", "--shortlist", "16", "--prefilter", "8", "--resume", "x"], "--prefilter must be at least --shortlist"),
    (["--query_ids", "0", "--candidates", "tvg", "--topk", "12", "--prefilter", "8", "--resume", "x"], "--prefilter must be at least --shortlist"),
    (["--direction", "v2t", "--video_ids", "0", "--candidates", "tvg", "--prefilter", "8", "--resume", "x"], "v2t has no prefilter"),
    (["--query_ids", "0", "--candidates", "tvg", "--prefilter", "8"], "--candidates tvg needs a fine-tuned checkpoint"),      # the existing refusal, word for word
    (["--query_ids", "0", "--shortlist", "8", "--resume", "x"], "--shortlist is the number of candidates"),
])
def test_check_args_refusals(argv, msg):
    with pytest.raises(SystemExit, match=msg):
        SR.check_args(SR.get_args_parser().parse_args(argv))


def test_check_args_accepts_the_prefilter():
    p = SR.get_args_parser()
    assert p.parse_args(["--query_ids", "0"]).prefilter is None
    for argv in (["--query_ids", "0", "--candidates", "tvg", "--resume", "x", "--prefilter", "64"], ["--query", "a dog", "--candidates", "tvg", "--resume", "x", "--shortlist", "16", "--prefilter", "16"],
                 ["--serve", "--candidates", "tvg", "--resume", "x", "--shortlist", "4", "--prefilter", "128"]):
        SR.check_args(p.parse_args(argv))
    assert SR._prefilter_line({"queries": 3, "passes": 2, "rows": 3, "kept": 17}) == {"queries": 3, "stage0_passes": 2, "stage0_rows": 3, "kept": 17}


# ---- 4. serve
def _server(argv, finetuned=True):
    s = _fake(n_texts=4)
    g = GH._gallery(s, {0: 0, 3: 1})
    passes = SH._scoring(g)
    args = SR.get_args_parser().parse_args(["--serve"] + list(argv))
    SR.check_args(args)
    iv2 = np.random.RandomState(1).rand(4, N).astype(np.float32)
    return SR.Server(g, [f"v{j}" for j in range(N)], 4, iv2, args, finetuned=finetuned), passes


def test_parse_reads_the_prefilter_field():
    srv, _ = _server(["--candidates", "all", "--resume", "x", "--c", "0.5", "0", "1", "0"])
    r = srv.parse(json.dumps({"id": 1, "caption": 2, "shortlist": 3, "prefilter": 5}))
    assert r["shortlist"] == 3 and r["prefilter"] == 5 and r["cand"] is None
    assert srv.parse(json.dumps({"id": 1, "caption": 2, "shortlist": 3}))["prefilter"] is None
    assert srv.parse(json.dumps({"id": 2, "rows": SH.ROWS_A}))["prefilter"] is None
    for req, msg in (({"caption": 0, "prefilter": 4}, "narrows a shortlist"), ({"caption": 0, "candidate_idx": [1, 2], "prefilter": 4}, "narrows a shortlist"),
                     ({"caption": 0, "shortlist": 3, "prefilter": 2}, "at least the shortlist's K = 3"), ({"caption": 0, "shortlist": 2, "prefilter": 0}, "positive integer"),
                     ({"caption": 0, "shortlist": 2, "prefilter": "4"}, "positive integer"), ({"caption": 0, "shortlist": 2, "prefilter": 4.0}, "positive integer"),
                     ({"caption": 0, "shortlist": 2, "prefilter": True}, "positive integer"), ({"rows": SH.ROWS_B, "shortlist": 2, "prefilter": 4}, "TVG row"),
                     ({"caption": 0, "shortlist": 2, "prefilter": 4, "candidates": ["v1"]}, "not both"),
                     ({"add_video": {"vid": "x", "features": "f.pt"}, "prefilter": 4}, "carries no query")):
        with pytest.raises(SR.BadRequest, match=msg) as e:
            srv.parse(json.dumps(dict(req, id=7)))
        assert e.value.id == 7
    zero, _ = _server(["--candidates", "all"], finetuned=False)
    with pytest.raises(SR.BadRequest, match="fine-tuned"):
        zero.parse(json.dumps({"caption": 0, "shortlist": 2, "prefilter": 4}))
    tvg, _ = _server(["--candidates", "tvg", "--resume", "x", "--topk", "2"])
    r = tvg.parse(json.dumps({"caption": 1, "prefilter": 4}))                      # next to the default K under --candidates tvg
    assert r["shortlist"] == 2 and r["prefilter"] == 4
    assert tvg.parse(json.dumps({"caption": 1}))["prefilter"] is None
    flag, _ = _server(["--candidates", "tvg", "--resume", "x", "--topk", "2", "--prefilter", "5"])
    assert flag.parse(json.dumps({"caption": 1}))["prefilter"] == 5                # --prefilter: the default K's requests are prefiltered
    assert flag.parse(json.dumps({"caption": 1, "prefilter": 3}))["prefilter"] == 3
    assert flag.parse(json.dumps({"caption": 1, "shortlist": 6}))["prefilter"] is None and flag.parse(json.dumps({"caption": 1, "candidate_idx": [3, 1]}))["prefilter"] is None


@pytest.mark.parametrize("B", [1, 3, 64])
def test_serve_answers_prefiltered_requests_whatever_the_batch(B):
    lines = [json.dumps({"id": 0, "caption": 1, "shortlist": 3, "prefilter": 4}),
             json.dumps({"id": 1, "rows": SH.ROWS_A, "candidate_idx": [4, 0, 2], "first_stage": [0.1, 0.9, 0.5]}),
             json.dumps({"id": 2, "caption": 0, "shortlist": 3, "prefilter": 2}),
             json.dumps({"id": 3, "rows": SH.ROWS_A, "shortlist": 2, "prefilter": 100, "topk": 1}),
             json.dumps({"id": 4, "caption": 3, "shortlist": 2}),
             json.dumps({"id": 5, "caption": 2, "prefilter": 3})]
    runs = {}
    for b in (1, B):
        srv, passes = _server(["--candidates", "all", "--resume", "x", "--c", "0.5", "0", "1", "0"])
        out = []
        summary = SR.serve(iter(lines), out.append, srv, batch_queries=b, batch_wait_ms=60000.0)
        runs[b] = ([json.loads(x) for x in out], summary, len(passes), srv)
    out, summary, n_passes, srv = runs[B]
    assert out == runs[1][0]                                                       # whatever the batch
    assert [x["id"] for x in out] == list(range(6)) and [n for n, x in enumerate(out) if "error" in x] == [2, 5]
    assert "at least the shortlist" in out[2]["error"] and "narrows a shortlist" in out[5]["error"]
    assert set(out[0]) == {"id", "query", "videos", "scores", "shortlisted", "prefiltered"} and out[0]["shortlisted"] == 3 and out[0]["prefiltered"] == 4
    assert len(out[0]["videos"]) == 3 and set(out[0]["videos"]) <= {f"v{j}" for j in _kept(1, 4, False, (0, 0))}
    assert out[3]["prefiltered"] == 100 and len(out[3]["videos"]) == 1
    assert set(out[4]) == {"id", "query", "videos", "scores", "shortlisted"} and set(out[1]) == {"id", "query", "videos", "scores"}
    batches_with = lambda which: sum(1 for a in range(0, 6, B) if any(n in which for n in range(a, min(a + B, 6))))
    assert len(srv.s.first_calls) == batches_with((0, 3)) and len(srv.s.gallery_calls) == batches_with((4,))
    assert srv.gal.prefilter_stats["queries"] == 2 and srv.gal.prefilter_stats["kept"] == 4 + N
    assert SR._prefilter_line(srv.gal.prefilter_stats)["stage0_passes"] == len(srv.s.first_calls)
