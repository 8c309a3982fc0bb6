"""GPU: the caption prefilter -- TextGalleryIndex.prefilter / PrefixCache.tvg_first_cols (blim.h: blim_tvg_first_cached) against
PairScorer.tvg where a TVG score IS its clip-0 term (num_clips = 1: equal as floats, plain and compensated), bit for bit against PairScorer.tvg_first(full=True)'s
lp[text, video] at num_clips = 4 (a cached hidden row and a decoded one are the same row) over an eager full cache, a budget that leaves prompts without a slot, a
lazy index with part of its keys resident (whose counters must not move) and chunk_rows = 256 over more than 256 slots against the default chunking; the ties of
texts that share a prompt; shortlist / rerank_shortlist with a K0 against the composition of the public calls; a stale cache; a video that joined; the command.
Tiny dims; 37 videos and 38 texts (two with one caption prompt), 320 for the chunking.  The host side is tests/test_caption_prefilter_host.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_gpu_parity as P
import test_text_gallery_gpu as TG
from blim_amd import engine as eng
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd.gallery import GalleryIndex, TextGalleryIndex
from blim_amd.modeling import BlimModel, DDPLike
from test_gallery_gpu import lora  # noqa: F401  (fixture: lora_tiny with adapters apart, a fine-tuned model's blend)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 37
ALPHA = (0.8, 0.3)
C_BLEND = (0.6, 0.5, 0.7, 0.5)
f32 = np.float32


def _build(dtype, clips, n=N):
    spec = dict(P.CASES["tiny"], n=n)
    dims = synth.ModelDims(**dict(spec["dims"], num_clips=clips))
    model = BlimModel(dims, max_positions=1024, dtype=dtype)
    model.engine.load_weights(synth.synthetic_weights(dims, spec["wseed"]))
    prob = synth.make_problem(spec["pseed"], n, dims, tok_per_clip=spec["tok_per_clip"], text_len=spec["text_len"])
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


@pytest.fixture(scope="module")
def many():
    t = _build("f16", 4, 320)
    yield t
    t.model.engine.close()


def _scorer(t, mode="full", precise=True, twin=True):
    """-> the scorer under TVG mode `mode` (precise False: plain TVG calls), with one more text whose caption prompt is text 3's, byte for byte."""
    prob = t.prob
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    G._set_mode(t, "none")
    sc = RU.PairScorer(DDPLike(t.model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video],
                       torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels), t.dims.num_clips, precise_tvg=precise)
    sc.set_vtg_mode(t.model.vtg_mode())
    TG._set_tvg(t, sc, mode)
    assert bool(sc.split_tvg) == bool(precise)
    if twin:
        new, = sc.add_texts([sc.vtg_rows[7]], [sc.tvg_rows[3]]).tolist()
        assert new == len(prob.tvg_ids) and np.array_equal(sc.tvg_split[new], sc.tvg_split[3])
    return sc


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.int32)


def _matrix(tg, videos, **kw):
    """prefilter at K0 = every text -> (the values by text index [Q, texts], cand, val); checks the order on the way: descending, ties to the lower text index."""
    n = len(tg.s.tvg_split)
    cand, val = tg.prefilter(videos, n, **kw)
    assert cand.shape == val.shape == (len(videos), n) and cand.dtype == np.int64 and val.dtype == f32
    M = np.zeros((len(videos), n), f32)
    for q in range(len(videos)):
        assert sorted(cand[q].tolist()) == list(range(n))
        M[q, cand[q]] = val[q]
        assert np.array_equal(cand[q], np.argsort(-M[q], kind="stable"))
    return M, cand, val


def _first_lp(sc, videos):
    """PairScorer.tvg_first(full=True)'s lp[text, video] for every text -> [Q, texts]."""
    lp = sc.tvg_first(np.arange(len(sc.tvg_split)), 1, full=True)[2]
    return np.ascontiguousarray(lp[:, np.asarray(videos)].T)


# ---- 1. num_clips = 1: the stage-0 value is the TVG score
@pytest.mark.parametrize("precise", [False, True], ids=["plain", "compensated"])
def test_with_one_clip_a_stage_0_value_is_the_tvg_score(one_clip, precise):
    t = one_clip
    sc = _scorer(t, precise=precise)
    tg = TextGalleryIndex(sc).build()
    try:
        assert bool(tg.cache.compensated) == precise and len(tg.slot_of) == len(tg.keys) == N
        videos = [0, 5, N - 1, 5]
        M, _, _ = _matrix(tg, videos)
        n = len(sc.tvg_split)
        for q, v in enumerate(videos):
            want = sc.tvg(np.stack([np.full(n, v), np.arange(n)], axis=1))
            assert np.all(np.isfinite(want)) and np.array_equal(M[q], want), (v, float(np.max(np.abs(M[q] - want))))
        assert np.array_equal(_bits(M[1]), _bits(M[3]))
    finally:
        tg.close(); TG._set_tvg(t, sc, "full")


# ---- 2. num_clips = 4: the cached row is the decoded row
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_a_stage_0_value_is_tvg_firsts_lp_bit_for_bit(four_clips, mode):
    t = four_clips
    sc = _scorer(t, mode)
    videos = [3, 0, N - 1]
    want = _first_lp(sc, videos)
    assert np.all(np.isfinite(want)) and np.all(want <= 0)
    n_keys = len(TextGalleryIndex(sc).keys)
    assert n_keys == N                                                             # 38 texts, 37 prompts
    for slots in (None, n_keys // 2, 0):                                           # an eager full cache; a budget that leaves prompts without a slot; no slot at all
        tg = TextGalleryIndex(sc)
        if slots is not None:
            tg.budget_bytes = slots * tg.per_slot_bytes()
        try:
            before = sc.exec_tokens
            M, cand, val = _matrix(tg, videos)
            assert len(tg.slot_of) == (n_keys if slots is None else slots)
            assert np.array_equal(_bits(M), _bits(want)), (slots, float(np.max(np.abs(M - want))))
            assert (sc.exec_tokens > before) == (slots is not None)                 # the keys without a slot went through the decoded path, the others through no call of the scorer's
            assert tg.prefilter_stats == {"queries": 3, "passes": 1, "rows": n_keys, "kept": 3 * (N + 1)} and tg.stats.as_dict() == dict.fromkeys(tg.stats.as_dict(), 0)
            c8, v8 = tg.prefilter(videos, 8)                                       # a smaller K0 keeps the first K0 of the same order
            assert np.array_equal(c8, cand[:, :8]) and np.array_equal(_bits(v8), _bits(val[:, :8]))
        finally:
            tg.close()
    TG._set_tvg(t, sc, "full")


def test_a_lazy_index_with_part_of_its_keys_resident_keeps_its_counters(four_clips):
    t = four_clips
    sc = _scorer(t)
    videos = [2, 9]
    want = _first_lp(sc, videos)
    tg = TextGalleryIndex(sc, fill="lazy")
    tg.budget_bytes = 12 * tg.per_slot_bytes()
    tg.build()
    try:
        M, _, _ = _matrix(tg, videos)                                              # nothing resident
        assert tg.slot_of == {} and np.array_equal(_bits(M), _bits(want))
        tg.tvg_pairs(np.stack([np.full(9, 4), np.arange(9)], axis=1))              # a pass admits nine prompts
        assert len(tg.slot_of) == 9 and tg.stats.admitted == 9
        state = (tg.stats.as_dict(), dict(tg.slot_of), dict(tg._stamp), tg._n_pass)
        M, _, _ = _matrix(tg, videos)
        assert np.array_equal(_bits(M), _bits(want))
        assert (tg.stats.as_dict(), dict(tg.slot_of), dict(tg._stamp), tg._n_pass) == state       # no hit, no miss, no admission, no stamp, no pass
    finally:
        tg.close()


def test_a_value_does_not_depend_on_the_chunking(many):
    t = many
    sc = _scorer(t, twin=False)
    tg = TextGalleryIndex(sc).build()
    try:
        n = len(sc.tvg_split)
        assert len(tg.slot_of) == len(tg.keys) > 256
        videos = [0, 17, 319]
        c0, v0 = tg.prefilter(videos, 64)                                          # the default chunk: every slot in one
        c1, v1 = tg.prefilter(videos, 64, chunk_rows=256)                          # two chunks, the second partly filled
        assert np.array_equal(c0, c1) and np.array_equal(_bits(v0), _bits(v1)) and np.all(np.isfinite(v0))
        M, _, _ = _matrix(tg, videos, chunk_rows=256)
        assert np.array_equal(_bits(M), _bits(_first_lp(sc, videos)))
        slots = [tg.slot_of[k] for k in tg.keys]
        cols = torch.from_numpy(np.asarray(sc.tvg_video_labels, np.int32)[videos]).cuda()
        with pytest.raises(eng.BlimError, match="chunk_rows"):
            sc.tvg_first_cached(tg.cache, slots, cols, chunk_rows=100)
        with pytest.raises(eng.BlimError, match="outside 0"):
            sc.tvg_first_cached(tg.cache, slots + [tg.cache.n_slots], cols)
    finally:
        tg.close()


# ---- 3. texts that share a prompt
def test_texts_that_share_a_prompt_tie_and_the_lower_index_goes_first(four_clips):
    t = four_clips
    sc = _scorer(t)
    tg = TextGalleryIndex(sc).build()
    try:
        twin = len(sc.tvg_split) - 1
        M, cand, _ = _matrix(tg, [1, 8, 30])
        assert np.array_equal(_bits(M[:, 3]), _bits(M[:, twin]))
        for row in cand.tolist():
            assert row.index(3) < row.index(twin)
    finally:
        tg.close()


# ---- 4. the composition
@pytest.mark.parametrize("cpn", [False, True])
def test_a_prefiltered_shortlist_is_the_composition_of_the_public_calls(lora, cpn):
    t = lora
    n = t.spec["n"]
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    TG._set_tvg(t, sc, "full")
    gal = GalleryIndex(sc).build()
    tg = TextGalleryIndex(sc, video_index=gal).build()
    more = dict(cpn=cpn, alpha=ALPHA, c=C_BLEND)
    try:
        videos, k, K0 = [0, n - 1, 2], 2, 4
        kept, _ = tg.prefilter(videos, K0)
        cand, stage = tg.shortlist(videos, k, prefilter=K0)
        for q, v in enumerate(videos):
            texts = np.sort(kept[q])
            row = tg.tvg_pairs(np.stack([np.full(K0, v), texts], axis=1))
            o = np.argsort(-row, kind="stable")[:k]
            assert np.array_equal(cand[q], texts[o]) and np.array_equal(_bits(stage[q]), _bits(row[o])) and np.all(np.isfinite(row))
        order, blended = tg.rerank_shortlist(videos, k, prefilter=K0, **more)
        pairs = np.stack([np.repeat(videos, k), cand.reshape(-1)], axis=1)
        v2t = tg.vtg_pairs(pairs).reshape(cand.shape)
        if cpn:
            v2t = v2t - ALPHA[1] * tg.v2t_prior(videos, cand)
        o2, b2 = tg._blend(cand, stage, v2t, np.zeros(cand.shape), C_BLEND)       # rerank over that shortlist, the stage-1 term reused
        assert np.array_equal(order, o2) and np.array_equal(blended, b2) and np.all(np.isfinite(blended))
        for q, v in enumerate(videos):                                             # ... which, one video per text, is the recomputed one
            o3, b3 = tg.rerank([v], cand[q:q + 1], finetuned=True, **more)
            assert np.array_equal(order[q], o3[0]) and np.array_equal(blended[q], b3[0])
        # K0 = every text: the unprefiltered results exactly
        for K in (3, n + 2):
            a, b = tg.shortlist(videos, K, prefilter=n + 5), tg.shortlist(videos, K)
            assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
            a, b = tg.rerank_shortlist(videos, K, prefilter=n + 5, **more), tg.rerank_shortlist(videos, K, **more)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype
        with pytest.raises(ValueError, match="below the shortlist"):
            tg.shortlist(videos, 3, prefilter=2)
    finally:
        tg.close(); gal.close(); TG._set_tvg(t, sc, "full")


# ---- 5. a stale cache
def test_a_stale_cache_is_refilled_by_the_index_and_refused_by_the_engine(four_clips):
    t = four_clips
    sc = _scorer(t, "full")
    tg = TextGalleryIndex(sc).build()
    videos = [6, 1]
    try:
        slots = [tg.slot_of[k] for k in tg.keys]
        cols = torch.from_numpy(np.asarray(sc.tvg_video_labels, np.int32)[videos]).cuda()
        for mode in ("attn", "full"):
            TG._set_tvg(t, sc, mode)
            with pytest.raises(eng.BlimError, match="stale.*precise_mlp"):         # read directly: the engine's own refusal
                sc.tvg_first_cached(tg.cache, slots, cols)
            M, _, _ = _matrix(tg, videos)                                          # the index follows the mode and refills first
            assert tg._state[1] == mode and np.array_equal(_bits(M), _bits(_first_lp(sc, videos)))
            slots = [tg.slot_of[k] for k in tg.keys]
            got = sc.tvg_first_cached(tg.cache, slots, cols).cpu().numpy()
            assert np.array_equal(_bits(got[:, [tg.keys.index(p.tobytes()) for p in sc.tvg_split]]), _bits(M))
    finally:
        tg.close(); TG._set_tvg(t, sc, "full")


# ---- 6. a video that joined
def test_a_video_that_joined_can_be_the_query(four_clips):
    t = four_clips
    sc = _scorer(t)
    tg = TextGalleryIndex(sc).build()
    try:
        before, _, _ = _matrix(tg, [4])
        new, = sc.add_videos([torch.from_numpy(t.prob.video[3] * 0.5 + t.prob.video[11] * 0.5)]).tolist()
        assert new == N and sc.n_vocab == N + 1
        M, _, _ = _matrix(tg, [new, 4])
        want = _first_lp(sc, [new, 4])                                             # lp over the N + 1 entries
        assert np.array_equal(_bits(M), _bits(want)) and np.all(np.isfinite(M))
        assert not np.array_equal(_bits(M[1]), _bits(before[0])) and np.all(M[1] <= before[0] + 1e-6)      # the grown vocabulary moved the normaliser of an old video's values
        cand, stage = tg.shortlist([new], 3, prefilter=10)
        assert len(set(cand[0].tolist())) == 3 and np.all(np.isfinite(stage))
    finally:
        tg.close()


# ---- 7. the command
def test_the_command_prefilters_the_captions():
    base = [sys.executable, "-m", "blim_amd.search", "--synthetic", "24", "--direction", "v2t", "--video_ids", "0", "5", "--topk", "4", "--resume", "x", "--candidates", "tvg",
            "--shortlist", "6", "--vtg_precise", "none", "--c", "0.5", "0.5", "0.5", "0.5"]
    runs = {}
    for K0 in (None, 8):
        r = subprocess.run(base + ([] if K0 is None else ["--caption_prefilter", str(K0)]), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[K0] = ([json.loads(x) for x in r.stdout.splitlines()], r.stderr)
    plain, err = runs[None]
    assert [x["query"] for x in plain] == ["video:0", "video:5"] and all(set(x) == {"query", "texts", "scores", "shortlisted"} for x in plain) and "prefilter:" not in err
    for K0 in (8,):
        lines, err = runs[K0]
        for x in lines:
            assert x["prefiltered"] == K0 and x["shortlisted"] == 6 and len(x["texts"]) == 4 and len(set(x["texts"])) == 4 and np.all(np.isfinite(x["scores"]))
            assert x["scores"] == sorted(x["scores"], reverse=True)
        assert json.loads(err.split("prefilter: ")[1].splitlines()[0]) == {"queries": 2, "stage0_passes": 2, "stage0_rows": 2 * 24, "kept": 2 * K0}
        assert json.loads(err.split("shortlist: ")[1].splitlines()[0]) == {"queries": 2, "stage1_passes": 2, "stage1_pairs": 2 * K0}
    assert all(x["shortlisted"] == 6 and len(x["texts"]) == 4 for x in plain)                         # without the flag: the answer lines as they were
