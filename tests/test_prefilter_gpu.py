"""GPU: the prefilter -- PairScorer.tvg_first / Engine.score_tvg_first against PairScorer.tvg where a TVG score IS its clip-0 term
(num_clips = 1: equal as floats, the candidate prior's rows included), against the literal surface at num_clips = 4 (the tolerance of the fused-vs-literal parity
tests, tests/test_gpu_parity.py: score_rtol), its independence of what shares a call and of where max_tokens cuts, the order against the stable argsort of its own
rows, and GalleryIndex.prefilter / the five-field request of search_requests / the serve field against the composition of the public calls.  Tiny dims, N = 37
videos, 5 texts: two with one caption prompt, two with prompts of one length (one prior key).  fp16 and bf16.  The host side is tests/test_prefilter_host.py."""
import copy
import json
import types

import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_gpu_parity as P
from blim_amd import retrieval_utils as RU
from blim_amd import search as SR
from blim_amd import synth
from blim_amd.gallery import GalleryIndex
from blim_amd.modeling import BlimModel, DDPLike

pytestmark = pytest.mark.gpu
N = 37
ALPHA = (0.8, 0.3)
C_BLEND = (0.6, 0.5, 0.7, 0.5)
f32 = np.float32


def _build(dtype, clips):
    spec = dict(P.CASES["tiny"], n=N)
    dims = synth.ModelDims(**dict(spec["dims"], num_clips=clips))
    model = BlimModel(dims, max_positions=1024, dtype=dtype)
    model.engine.load_weights(synth.synthetic_weights(dims, spec["wseed"]))
    prob = synth.make_problem(spec["pseed"], N, dims, tok_per_clip=spec["tok_per_clip"], text_len=spec["text_len"])
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    return types.SimpleNamespace(spec=spec, dims=dims, model=model, prob=prob, dtype=dtype)


@pytest.fixture(scope="module", params=["f16", "bf16"])
def one_clip(request):
    t = _build(request.param, 1)
    yield t
    t.model.engine.close()


@pytest.fixture(scope="module", params=["f16", "bf16"])
def four_clips(request):
    t = _build(request.param, 4)
    yield t
    t.model.engine.close()


def _scorer(t):
    """-> (the scorer, the 5 texts): a, b, a's twin (another VTG row, a's caption prompt byte for byte), c with b's prompt length, d."""
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    lens = [len(p) for p in sc.tvg_split]
    b, c = next((x, y) for x in range(N) for y in range(x + 1, N) if lens[x] == lens[y])
    a = next(i for i in range(N) if lens[i] != lens[b])
    d = next(i for i in range(N) if lens[i] not in (lens[a], lens[b]))
    twin, = sc.add_texts([sc.vtg_rows[d]], [sc.tvg_rows[a]]).tolist()
    return sc, [a, b, twin, c, d]


def _counted(sc):
    calls, run = [], sc.run

    def counted(plan, cache=None, **kw):
        calls.append(plan)
        return run(plan, cache, **kw)
    sc.run = counted
    return calls


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.int32)


def _prior_lp(sc, texts):
    """The prior rows' own log-probabilities [Q, N]: the plan of tvg_first(cpn=True) run with its prior rows as the scored rows."""
    out = np.zeros((len(texts), sc.n_vocab), f32)
    for plan in sc.iter_tvg_first(texts, cpn=True):
        p2 = copy.copy(plan)
        p2.rows, p2.prior_rows, p2.n_pairs = plan.prior_rows, None, len(plan.prior_rows)
        lp = sc.run(p2, k=1, full=True)[2].cpu().numpy()
        for at, outs in zip(plan.labels.cpu().numpy().tolist(), plan.out_index):
            out[outs] = lp[at]
    return out


def test_with_one_clip_a_tvg_score_is_its_clip_0_term(one_clip):
    t = one_clip
    sc, texts = _scorer(t)
    pairs = np.array([[j, i] for i in texts for j in range(N)])
    want = sc.tvg(pairs).reshape(len(texts), N)
    idx, val, lp = sc.tvg_first(texts, 8, full=True)
    assert np.all(np.isfinite(want)) and np.array_equal(lp, want), float(np.max(np.abs(lp - want)))
    assert np.array_equal(_bits(lp[0]), _bits(lp[2]))                              # the twin rides on its caption's row
    for q in range(len(texts)):
        o = np.argsort(-lp[q], kind="stable")[:8]
        assert np.array_equal(idx[q], o) and np.array_equal(_bits(val[q]), _bits(lp[q][o]))
    # the prior rows: PairScorer.tvg(cpn = True), and the term in numpy f32 arithmetic
    prior = sc.tvg(pairs, cpn=True).reshape(len(texts), N)
    pl = _prior_lp(sc, texts)
    assert np.array_equal(pl, prior), float(np.max(np.abs(pl - prior)))
    assert np.array_equal(_bits(pl[1]), _bits(pl[3]))                              # one prior key for the two prompts of one length
    idx, val, lp2 = sc.tvg_first(texts, N, cpn=True, alpha=ALPHA[0], full=True)
    assert np.array_equal(_bits(lp2), _bits(lp))
    term = lp - (f32(ALPHA[0]) * pl).astype(f32)
    for q in range(len(texts)):
        o = np.argsort(-term[q], kind="stable")
        assert np.array_equal(idx[q], o) and np.array_equal(_bits(val[q]), _bits(term[q][o]))


def test_clip_0_against_the_literal_surface(four_clips):
    t = four_clips
    sc, texts = _scorer(t)
    model, prob, dev = t.model, t.prob, t.model.device
    ddp = DDPLike(model)
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    ids, lab, msk = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    vocab = torch.from_numpy(prob.video_vocab)
    _, _, lp = sc.tvg_first(texts, 4, full=True)
    rtol = P.score_rtol(t.dtype, "t2v_tvg", literal=True)
    for q, i in enumerate(texts[:2] + texts[3:]):                                  # (the twin is its caption's row)
        r = model.prepare_inputs_labels_for_multimodal(ids[[i]].to(dev), None, msk[[i]].to(dev), None, lab[[i]].to(dev), [torch.from_numpy(prob.video[0]).to(dev)],
                                                       ["video"], image_sizes=[(448, 448)], video_feature=True, tvg=True, cpn=True)
        out = ddp(inputs_embeds=r[4], attention_mask=r[2][0])
        lg = RU._tvg_logits_literal(ddp, out.hidden_states, r[5], vocab, t.dims.num_clips, dev)[0, 0].double().cpu().numpy()      # clip 0: the prompt's last row
        ref = lg - (lg.max() + np.log(np.exp(lg - lg.max()).sum()))
        got = lp[texts.index(i)]
        np.testing.assert_allclose(got, ref, rtol=rtol)
    # the summand of the score itself: the mean over clips of PairScorer.tvg holds it (clip 0's share of a pair's score, a loose sanity bound)
    assert np.all(lp <= 0)


@pytest.mark.parametrize("cpn", [False, True])
def test_values_do_not_depend_on_what_shares_a_call_or_on_the_cut(four_clips, cpn):
    t = four_clips
    sc, texts = _scorer(t)
    calls = _counted(sc)
    kw = dict(cpn=cpn, alpha=ALPHA[0], full=True)
    idx, val, lp = sc.tvg_first(texts, 16, **kw)
    assert len(calls) == 1 and calls[0].n_pairs == 4 and np.all(np.isfinite(lp)) and np.all(np.isfinite(val))       # 5 texts, 4 distinct prompts, ONE call
    if cpn:
        assert len(calls[0].prior_rows) == 3                                       # three prompt lengths: three prior keys
    for q, i in enumerate(texts):                                                  # alone
        del calls[:]
        i1, v1, l1 = sc.tvg_first([i], 16, **kw)
        assert len(calls) == 1 and np.array_equal(i1[0], idx[q]) and np.array_equal(_bits(v1[0]), _bits(val[q])) and np.array_equal(_bits(l1[0]), _bits(lp[q]))
    del calls[:]
    i2, v2, l2 = sc.tvg_first(texts[::-1], 16, **kw)                               # among others, in another order
    assert np.array_equal(i2, idx[::-1]) and np.array_equal(_bits(v2), _bits(val[::-1])) and np.array_equal(_bits(l2), _bits(lp[::-1]))
    longest = max(len(sc.tvg_split[i]) for i in texts)
    sc.max_tokens = 2 * longest + (sc.m.tvg_prefix_length + 2 if cpn else 0)       # two prompts (and their priors) per call at the most
    try:
        want_calls = len(list(sc.iter_tvg_first(texts, cpn)))
        del calls[:]
        i3, v3, l3 = sc.tvg_first(texts, 16, **kw)
        assert len(calls) == want_calls and 2 <= want_calls <= 4 and all(p.n_tokens <= sc.max_tokens for p in calls)
        assert np.array_equal(i3, idx) and np.array_equal(_bits(v3), _bits(val)) and np.array_equal(_bits(l3), _bits(lp))
    finally:
        sc.max_tokens = 4096
    term = lp
    if cpn:
        term = lp - (f32(ALPHA[0]) * _prior_lp(sc, texts)).astype(f32)
    for q in range(len(texts)):                                                    # the order: the stable argsort of its own rows
        o = np.argsort(-term[q], kind="stable")[:16]
        assert np.array_equal(idx[q], o) and np.array_equal(_bits(val[q]), _bits(term[q][o]))
    with pytest.raises(ValueError, match="outside 1"):
        sc.tvg_first(texts, N + 1)


@pytest.mark.parametrize("cpn", [False, True])
def test_prefiltered_requests_are_the_composition_of_the_public_calls(four_clips, cpn):
    t = four_clips
    sc, texts = _scorer(t)
    gal = GalleryIndex(sc).build()
    try:
        a, b, twin, c, d = texts
        more = dict(cpn=cpn, alpha=ALPHA, c=C_BLEND, finetuned=True)
        before = dict(gal.prefilter_stats)
        passes = gal._n_pass
        batch = [(a, None, None, 3, 8), (b, np.array([4, 1, 30]), None, None), (c, None, None, 4, 12), (d, None, None, 2)]
        got = gal.search_requests(batch, **more)
        assert gal._n_pass == passes + 1 and gal.prefilter_stats["passes"] == before["passes"] + 1 and gal.prefilter_stats["kept"] == before["kept"] + 20
        # the composition, per prefiltered request: prefilter -> ONE PairScorer.tvg call over both requests' kept pairs -> _best -> vtg_pairs -> _blend
        kept = gal._stage0([a, c], [8, 12], cpn, ALPHA)
        for row, i, K0 in zip(kept, (a, c), (8, 12)):
            assert np.array_equal(row, gal.prefilter([i], K0, cpn=cpn, alpha=ALPHA)[0]) and np.array_equal(row, np.sort(row)) and len(set(row.tolist())) == K0
        term = sc.tvg(np.concatenate([np.stack([row, np.full(len(row), i)], axis=1) for row, i in zip(kept, (a, c))]))
        if cpn:
            term = term - ALPHA[0] * gal._t2v_prior([a, c], kept)
        for (order, blended), row, tm, i, K in zip((got[0], got[2]), kept, np.split(term, [8]), (a, c), (3, 4)):
            keep, stage = gal._best(tm, K)
            cand = row[keep]
            ql = gal.vtg_pairs(np.stack([cand, np.full(K, i)], axis=1))
            o, bl = gal._blend(cand[None], ql[None], stage[None], np.zeros((1, K)), C_BLEND)
            assert np.array_equal(order, o[0]) and np.array_equal(blended, bl[0]) and np.all(np.isfinite(blended))
        # mixed batches against each request alone: bit for bit on the VTG term (a TVG value moves with its neighbours in a merged sequence, section 11's rule)
        vtg_only = dict(more, c=(1.0, 0.0, 1.0, 0.0))
        together = gal.search_requests(batch, **vtg_only)
        for r, (o1, b1) in zip(batch, together):
            o2, b2 = gal.search_requests([r], **vtg_only)[0]
            if set(o1.tolist()) == set(o2.tolist()):
                assert np.array_equal(o1, o2) and np.array_equal(b1, b2)
            want = sc.vtg(np.stack([o1, np.full(len(o1), r[0])], axis=1))
            assert np.array_equal(b1, want.astype(b1.dtype))
        # K0 = N: the kept set is the best K of PairScorer.tvg over all N
        (order, _), = gal.search_requests([(d, None, None, 5, N)], **more)
        full = sc.tvg(np.stack([np.arange(N), np.full(N, d)], axis=1))
        if cpn:
            full = full - ALPHA[0] * gal._t2v_prior([d], [np.arange(N)])
        assert sorted(order.tolist()) == sorted(np.argsort(-full, kind="stable")[:5].tolist())
        with pytest.raises(ValueError, match="below the shortlist"):
            gal.search_requests([(a, None, None, 5, 4)], **more)
        # a served request
        args = SR.get_args_parser().parse_args(["--serve", "--candidates", "all", "--resume", "x", "--alpha", str(ALPHA[0]), str(ALPHA[1]), "--c"] + [str(x) for x in C_BLEND]
                                               + (["--cpn"] if cpn else []))
        SR.check_args(args)
        srv = SR.Server(gal, [f"v{j}" for j in range(N)], N, None, args, finetuned=True)
        out = []
        srv.handle([json.dumps({"id": 9, "caption": int(a), "shortlist": 3, "prefilter": 8})], out.append)
        ans = json.loads(out[0])
        assert ans["prefiltered"] == 8 and ans["shortlisted"] == 3 and ans["videos"] == [f"v{j}" for j in got[0][0]] and ans["scores"] == [float(x) for x in got[0][1]]
    finally:
        gal.close()


def test_a_video_that_joins_can_be_ranked(four_clips):
    t = four_clips
    sc, texts = _scorer(t)
    gal = GalleryIndex(sc).build()
    try:
        a = texts[0]
        before, _ = sc.tvg_first([a], N)
        assert sorted(before[0].tolist()) == list(range(N))
        new, = sc.add_videos([torch.from_numpy(t.prob.video[3] * 0.5 + t.prob.video[11] * 0.5)]).tolist()
        assert new == N
        idx, val, lp = sc.tvg_first([a], N + 1, full=True)                          # the next call ranks over the new vocabulary
        assert sorted(idx[0].tolist()) == list(range(N + 1)) and lp.shape == (1, N + 1) and np.all(np.isfinite(lp))
        assert np.array_equal(idx[0], np.argsort(-lp[0], kind="stable"))
        kept = gal.prefilter([a], N + 1)
        assert kept.tolist() == [list(range(N + 1))]
        (order, blended), = gal.search_requests([(a, None, None, N + 1, N + 1)], cpn=False, alpha=ALPHA, c=C_BLEND, finetuned=True)
        assert new in order.tolist() and np.all(np.isfinite(blended))
    finally:
        gal.close()
