"""GPU: the lazy gallery (blim_amd/gallery.py `fill="lazy"`; blim.h: blim_score_vtg_admit / blim_score_tvg_admit) -- a scoring call captures the in-batch
prefixes it had to compute into slots on the way through, and the calls after it read them.  Every pass -- all misses, all hits, mixed, after an eviction, after a
re-admission of a shorter prompt into a slot that held a longer one -- gives bit for bit the scores of PairScorer.vtg / .tvg on the same pairs (TVG sets where
several videos share a text: within 1e-5, DESIGN.md section 11's rule).  The refusals of the admit calls are host-side checks: nothing is provoked on the device.
The host-side policy and planning are tests/test_lazy_gallery_host.py."""
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
from blim_amd import gallery as GL
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd.gallery import GalleryIndex, TextGalleryIndex
from blim_amd.synth import IGNORE_INDEX
from test_gallery_gpu import tiny  # noqa: F401  (fixture: the tiny case, 6 videos and 2 layers, in fp16 and bf16)

pytestmark = pytest.mark.gpu


def _scorer(t, max_tokens=4096, one_token=(), second_split=()):
    """G._scorer on the test's own copy of the rows.  one_token: texts whose response is cut to its first token (such a pair's score reads the prefix's last row
    alone); second_split: texts whose instruction differs in one token, so that their prefixes are keys of their own."""
    prob = t.prob
    ids, lab, msk = [r.copy() for r in prob.vtg_ids], [r.copy() for r in prob.vtg_labels], [r.copy() for r in prob.vtg_masks]
    for i in one_token:
        n_prompt = int(np.argmax(lab[i] != IGNORE_INDEX))
        ids[i], lab[i], msk[i] = ids[i][:n_prompt + 1], lab[i][:n_prompt + 1], msk[i][:n_prompt + 1]
    for i in second_split:
        at = int(np.argmax(lab[i] != IGNORE_INDEX)) - 6          # a token of the instruction between the video and the response
        ids[i][at] = ids[i][at] + 1
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(ids), Tt(lab), Tt(msk), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    return RU.PairScorer(G.DDPLike(t.model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video],
                         torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels), t.dims.num_clips, max_tokens=max_tokens)


def _lazy(sc, capacity=None, cls=GalleryIndex):
    gal = cls(sc, fill="lazy")
    if capacity is not None:
        gal.budget_bytes = capacity * gal.per_slot_bytes()
    gal.build()
    assert gal.slot_of == {} and gal.n_slots == (len(gal.keys) if capacity is None else capacity)
    gal.ran = []
    run = gal.run
    gal.run = lambda plan: gal.ran.append(plan) or run(plan)          # (the passes' plans, as they ran)
    return gal


def _delta(gal, pass_):
    before = gal.stats.as_dict()
    out = pass_()
    return out, {k: v - before[k] for k, v in gal.stats.as_dict().items()}


# ---- 1. miss, hit, and the eager index
@pytest.mark.parametrize("mode", ["none", "full", "select"])
def test_bit_equal_through_miss_and_hit(tiny, mode):
    t = tiny
    G._set_mode(t, mode)
    sc = _scorer(t, one_token=(2,))                                    # 4. text 2 answers in one token: on the second pass its scores read a slot's hidden row alone
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = G._t2v_pairs(t)
    ref = sc.vtg(pairs)
    assert np.all(np.isfinite(ref))
    n_vid = len(np.unique(pairs[:, 0]))
    gal = _lazy(sc)
    eager = GalleryIndex(sc).build()
    try:
        assert gal.cache.compensated == (mode != "none")
        got, d = _delta(gal, lambda: gal.vtg_pairs(pairs))             # pass 1: all misses, every one admitted
        assert np.array_equal(got, ref), (mode, np.max(np.abs(got - ref)))
        assert d["hits"] == 0 and d["misses"] == d["admitted"] == n_vid and d["evicted"] == 0 and d["prefix_tokens_packed"] > 0
        assert all(p.admits is not None and np.all(p.pfx_slot.cpu().numpy() == -1) for p in gal.ran)
        n1 = len(gal.ran)
        got, d = _delta(gal, lambda: gal.vtg_pairs(pairs))             # pass 2: all hits
        assert np.array_equal(got, ref), (mode, np.max(np.abs(got - ref)))
        assert d["hits"] == n_vid and d["misses"] == d["admitted"] == 0 and d["prefix_tokens_packed"] == 0
        assert np.array_equal(eager.vtg_pairs(pairs), got)
        assert sum(p.n_tokens for p in gal.ran[n1:]) == sum(p.n_tokens for p in eager.iter_plans(pairs))
        single = pairs[:, 1] == 2                                      # 4. the one-token text: the admitted hidden row, bit for bit
        assert single.any() and all(p.admits is None for p in gal.ran[n1:])
        assert np.array_equal(got[single], ref[single])
    finally:
        gal.close(); eager.close(); G._set_mode(t, "none")


# ---- 2. eviction, and a slot read in the call after the one that admitted it
@pytest.mark.parametrize("mode", ["none", "full"])
def test_eviction_and_slot_reuse_over_several_calls(tiny, mode):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, mode)
    # texts 1, 3, 5 under a second prompt split: a video's groups alternate between two keys, so a key admitted by one call is needed again by a later call of the pass
    sc = _scorer(t, max_tokens=96, second_split=(1, 3, 5))
    sc.set_vtg_mode(t.model.vtg_mode())
    gal = _lazy(sc, capacity=n // 2)
    try:
        assert len(gal.keys) == 2 * n and gal.max_len() < 96
        read_after_admit = 0
        for videos in ((0, 1), (2, 3, 0), (4, 5), (1, 2, 5)):
            pairs = np.array([[j, i] for j in videos for i in range(n)], np.int64)
            first = len(gal.ran)
            got = gal.vtg_pairs(pairs)
            want = sc.vtg(pairs)
            assert np.all(np.isfinite(want)) and np.array_equal(got, want), (videos, np.max(np.abs(got - want)))
            ran = gal.ran[first:]
            assert len(ran) > len(videos)                              # the pass spans several calls
            admitted = set()
            for p in ran:
                read_after_admit += len(admitted & set(p.slots_used.tolist()))
                admitted |= set() if p.admits is None else set(p.admits[:, 1].tolist())
        assert read_after_admit > 0 and gal.stats.evicted > 0 and gal.stats.hits > 0
        assert len(gal.slot_of) == n // 2 and sorted(gal.slot_of.values()) == list(range(n // 2))
    finally:
        gal.close(); G._set_mode(t, "none")


# ---- 3. the text gallery: caption prompts of unequal lengths
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_text_gallery_shorter_prompt_into_a_longer_prompts_slot(tiny, mode):
    t = tiny
    sc = G._scorer(t)
    TG._set_tvg(t, sc, mode)
    tg = _lazy(sc, capacity=1, cls=TextGalleryIndex)
    try:
        lens = [len(p) for p in sc.tvg_split]
        long_, short = int(np.argmax(lens)), int(np.argmin(lens))
        assert lens[long_] > lens[short]
        for i, want_d in ((long_, (0, 1, 1, 0)), (long_, (1, 0, 0, 0)), (short, (0, 1, 1, 1)), (short, (1, 0, 0, 0))):
            pairs = np.array([[1, i]], np.int64)
            got, d = _delta(tg, lambda: tg.tvg_pairs(pairs))
            want = sc.tvg(pairs)
            assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == want_d
            assert np.all(np.isfinite(want)) and np.array_equal(got, want), (i, got, want)     # positions beyond the short prompt hold the long one's K / V
        assert tg.cache.slot_len(0) == lens[short]
    finally:
        tg.close(); TG._set_tvg(t, sc, "full")


@pytest.mark.parametrize("mode", ["attn", "full"])
def test_text_gallery_passes_of_query_videos(tiny, mode):
    t = tiny
    sc = G._scorer(t)
    TG._set_tvg(t, sc, mode)
    tg = _lazy(sc, capacity=3, cls=TextGalleryIndex)
    try:
        pairs = TG._v2t_pairs(t)
        for _ in range(2):                                             # one video per text: bit for bit, through misses, hits and evictions
            TG._assert_bit_equal_per_video(sc, tg, pairs)
        assert tg.stats.hits > 0 and tg.stats.admitted > 3 and tg.stats.evicted > 0
        assert np.max(np.bincount(pairs[:, 1])) >= 2                   # several videos share a text: section 11's rule
        want = sc.tvg(pairs)
        got = tg.tvg_pairs(pairs)
        assert np.all(np.isfinite(got)) and TG._close(got, want), float(np.max(np.abs(got - want)))
    finally:
        tg.close(); TG._set_tvg(t, sc, "full")


# ---- 5. 7B width
def test_7b_width_miss_then_hit():
    t = P._build("wide", device_synth=True)
    try:
        G._set_mode(t, "none")
        sc = G._scorer(t)
        sc.set_vtg_mode(t.model.vtg_mode())
        pairs = G._t2v_pairs(t)
        ref = sc.vtg(pairs)
        gal = _lazy(sc)
        for want_hits in (0, len(np.unique(pairs[:, 0]))):
            got, d = _delta(gal, lambda: gal.vtg_pairs(pairs))
            assert d["hits"] == want_hits
            assert np.all(np.isfinite(ref)) and np.array_equal(got, ref), float(np.max(np.abs(got - ref)))
        gal.close()
    finally:
        t.model.engine.close()


# ---- 6. staleness
def test_stale_slots_are_refused_dropped_and_admitted_again(tiny):
    t = tiny
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = G._t2v_pairs(t)
    gal = _lazy(sc)
    try:
        assert np.array_equal(gal.vtg_pairs(pairs), sc.vtg(pairs))
        plans = list(gal.iter_plans(pairs))
        assert len(plans[0].slots_used) > 0
        t.model.engine.load_weight("final_norm", t.w["final_norm"] * 1.01)
        with pytest.raises(eng.BlimError, match="stale"):              # the engine's own refusal: the backstop
            gal.run(plans[0])
        cache = gal.cache
        got, d = _delta(gal, lambda: gal.vtg_pairs(pairs))             # the index drops its slots and admits again, into the same cache
        assert gal.cache is cache and d["hits"] == 0 and d["admitted"] == len(np.unique(pairs[:, 0]))
        assert np.array_equal(got, sc.vtg(pairs))
        G._set_mode(t, "full")                                         # none -> full: the cache is recreated with the lo parts
        got, d = _delta(gal, lambda: gal.vtg_pairs(pairs))
        assert gal.cache is not cache and gal.cache.compensated and d["hits"] == 0 and d["admitted"] > 0
        sc.set_vtg_mode("full")
        assert np.array_equal(got, sc.vtg(pairs))
        got, d = _delta(gal, lambda: gal.vtg_pairs(pairs))
        assert d["misses"] == 0 and np.array_equal(got, sc.vtg(pairs))
    finally:
        t.model.engine.load_weight("final_norm", t.w["final_norm"])
        G._set_mode(t, "none")
        gal.close()


# ---- 7. refusals of the admit call itself
def test_admit_call_refusals_are_host_side(tiny):
    t = tiny
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = G._t2v_pairs(t)
    ref = sc.vtg(pairs)
    gal = _lazy(sc)
    try:
        half = pairs[pairs[:, 0] < 3]
        gal.vtg_pairs(half)                                            # videos 0 .. 2 hold slots 0 .. 2; 3 .. 5 do not
        plan, = list(gal.iter_plans(pairs))
        a = plan.admits
        assert len(a) >= 2 and len(plan.slots_used) >= 1
        E, cache = t.model.engine, gal.cache

        def call(admits, slots_used=plan.slots_used):
            with sc._call_options("vtg"):
                return cache.score_vtg(plan.batch, plan.pfx_slot, slots_used, E.assemble(plan.src_index, plan.feats), plan.rows, plan.labels, plan.row_start,
                                       admits=admits)
        twice = a.copy(); twice[1, 1] = twice[0, 1]
        with pytest.raises(eng.BlimError, match="twice"):
            call(twice)
        both = a.copy(); both[0, 1] = plan.slots_used[0]
        with pytest.raises(eng.BlimError, match="read by this call"):
            call(both)
        long_ = a.copy(); long_[0, 3] = cache.max_len + 1
        with pytest.raises(eng.BlimError, match="len"):
            call(long_)
        row = a.copy(); row[0, 4] = plan.n_rows
        with pytest.raises(eng.BlimError, match="row"):
            call(row)
        outside = a.copy(); outside[0, 1] = cache.n_slots
        with pytest.raises(eng.BlimError, match="outside"):
            call(outside)
        beyond = a.copy(); beyond[0, 2] = plan.n_tokens - 1
        with pytest.raises(eng.BlimError, match="does not fit"):
            call(beyond)
        assert all(cache.slot_len(int(s)) > 0 for s in plan.slots_used)
        got = gal.run(plan).float().cpu().numpy()                      # the plan as planned still runs, and admits
        out = np.full(len(pairs), np.nan, np.float32)
        for k, o in enumerate(plan.out_index):
            out[o] = got[k]
        assert np.array_equal(out, ref)
        assert np.array_equal(gal.vtg_pairs(pairs), ref) and len(gal.slot_of) == len(np.unique(pairs[:, 0]))
    finally:
        gal.close()


# ---- 8. the CLI
def test_search_cli_lazy_prints_the_eager_runs_lines():
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)
    gb = 4.5 * GL.cache_bytes(dims, 1, 64, False) / 2**30             # about 4 slots of the dry run's 58-token prefixes
    base = [sys.executable, "-m", "blim_amd.search", "--synthetic", "12", "--query_ids", "0", "1", "2", "3", "--topk", "4", "--vtg_precise", "none"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    for fill, more in (("eager", []), ("lazy", ["--gallery_gb", repr(gb)])):
        r = subprocess.run(base + ["--gallery_fill", fill] + more, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[fill] = r
        assert f"fill {fill}" in r.stderr
    assert runs["lazy"].stdout == runs["eager"].stdout and len(runs["eager"].stdout.splitlines()) == 4
    assert "4 slots" in runs["lazy"].stderr
    stats = json.loads(runs["lazy"].stderr.split("gallery stats: ")[1].splitlines()[0])
    assert stats["hits"] >= 1 and stats["admitted"] >= 4 and stats["evicted"] >= 1
    assert stats["hits"] + stats["misses"] == 16
