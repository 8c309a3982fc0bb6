"""GPU: the text gallery (blim_amd/gallery.py: TextGalleryIndex) -- v2t TVG scores with the caption prompts read from the engine's prefix cache (blim.h:
blim_score_tvg_cached) against PairScorer.tvg on the same pairs: bit for bit where every text of the set has one video (each merged sequence is then a single
segment), within 1e-5 where several videos share a text (the cached and uncached planners may cut merged sequences at different places, and a TVG score moves at
the 1e-6 level with its neighbours in the merged sequence: tests/test_gallery_gpu.py::test_rerank_finetuned_matches_combine_and_rank_row).  Stale slots are refused
and refilled; rerank agrees with combine_and_rank's v2t blend.  The host-side planning is tests/test_text_gallery_host.py."""
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
from blim_amd import checkpoint as CK
from blim_amd import engine as eng
from blim_amd import retrieval_utils as RU
from blim_amd import training_utils as TU
from blim_amd.gallery import GalleryIndex, TextGalleryIndex
from test_gallery_gpu import b7, lora, tiny  # noqa: F401  (fixtures: the tiny case, lora_tiny with adapters apart, 64 items at the 7B dimensions)

pytestmark = pytest.mark.gpu


def _v2t_pairs(t, queries=None, topk=None):
    """(video, text) pairs of the evaluation's v2t passes: each query video's top-k texts of the first stage."""
    q = queries or t.spec.get("queries", t.spec["n"])
    return RU._topk_pairs(torch.from_numpy(t.prob.v2t_sims)[:q], 0, topk or t.spec["topk"], True)


def _per_video(pairs):
    return [pairs[pairs[:, 0] == v] for v in np.unique(pairs[:, 0])]


def _set_tvg(t, sc, mode):
    t.model.tvg_precise = mode
    sc.set_tvg_mode(t.model.tvg_mode())


def _close(got, want):
    return np.all(np.abs(got - want) <= 1e-5 * np.maximum(1.0, np.abs(want)))


def _assert_bit_equal_per_video(sc, tg, pairs):
    """One query video against its candidates: every text has one video, so every sequence is a single segment -- bit-equality."""
    for block in _per_video(pairs):
        assert len(np.unique(block[:, 1])) == len(block)
        want = sc.tvg(block)
        got = tg.tvg_pairs(block)
        assert np.all(np.isfinite(want))
        assert np.array_equal(got, want), (int(block[0, 0]), float(np.max(np.abs(got - want))))


def _index(t, mode, budget_slots=None, max_tokens=4096):
    sc = G._scorer(t, max_tokens)
    _set_tvg(t, sc, mode)
    tg = TextGalleryIndex(sc)
    if budget_slots is not None:
        tg.budget_bytes = budget_slots * tg.per_slot_bytes()
    tg.build()
    assert len(tg.slot_of) == (len(tg.keys) if budget_slots is None else min(budget_slots, len(tg.keys)))
    return sc, tg


# ---- 1. bit-equality, one video per text
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_cached_tvg_is_bit_equal_one_video_per_text(tiny, mode):
    sc, tg = _index(tiny, mode)
    try:
        assert tg.cache.compensated == sc.split_tvg
        _assert_bit_equal_per_video(sc, tg, _v2t_pairs(tiny))
    finally:
        tg.close(); _set_tvg(tiny, sc, "full")


@pytest.mark.parametrize("mode", ["attn", "full"])
def test_adapters_apart_bit_equal(lora, mode):
    assert lora.model.engine.num_adapters() == len(CK.expected_adapters(lora.dims))      # tvg_mlp and visual_head adapters are on this path
    sc, tg = _index(lora, mode)
    try:
        _assert_bit_equal_per_video(sc, tg, _v2t_pairs(lora))
    finally:
        tg.close(); _set_tvg(lora, sc, "full")


@pytest.mark.parametrize("mode", ["attn", "full"])
def test_7b_text_gallery_64_texts(b7, mode):
    """28 layers (per-layer slot offsets), G = 7; the 64 prompts fill in several calls of 1,024 tokens."""
    sc, tg = _index(b7, mode, max_tokens=1024)
    try:
        assert tg.slot_positions() % 32 == 0 and 0 <= tg.slot_positions() - tg.max_len() < 32
        assert sum(len(p) for p in tg.prompts.values()) > 2 * 1024
        pairs = _v2t_pairs(b7)
        assert len(pairs) == 8 * 16
        _assert_bit_equal_per_video(sc, tg, pairs)
    finally:
        tg.close(); _set_tvg(b7, sc, "full")
    # one video per text over all 64 texts, calls of 128 tokens: the cached scoring (192 tokens) splits too, the fill runs one or two prompts per call
    sc, tg = _index(b7, mode, max_tokens=128)
    try:
        pairs = np.stack([np.arange(64) % 8, np.arange(64)], axis=1)
        plans = list(tg.iter_plans(pairs))
        assert len(plans) >= 2 and sum(p.n_tokens for p in plans) == 3 * 64
        want = sc.tvg(pairs)
        got = tg.tvg_pairs(pairs)
        assert np.all(np.isfinite(want)) and np.array_equal(got, want), float(np.max(np.abs(got - want)))
    finally:
        tg.close(); _set_tvg(b7, sc, "full")


# ---- 2. tied to the reference
def _golden_v2t_tvg(t, g):
    sc, tg = _index(t, "full")
    try:
        pairs = _v2t_pairs(t)
        S = np.full(g.shape, -100.0, np.float32)
        S[pairs[:, 0], pairs[:, 1]] = tg.tvg_pairs(pairs)
        m = g != -100
        assert np.array_equal(m, S != -100)
        assert np.max(np.abs(S[m] - g[m]) / np.abs(g[m])) <= 1e-3
    finally:
        tg.close()


@pytest.mark.parametrize("tiny", ["f16"], indirect=True)
def test_cached_tvg_matches_the_golden_v2t_matrix(tiny):
    _golden_v2t_tvg(tiny, np.load(os.path.join(P.GOLD, "tiny.npz"))["S_v2t_tvg"])


@pytest.mark.parametrize("lora", ["f16"], indirect=True)
def test_cached_tvg_matches_the_golden_v2t_matrix_adapters_apart(lora):
    _golden_v2t_tvg(lora, np.load(os.path.join(P.GOLD, "lora_tiny.npz"))["S_v2t_tvg"])


# ---- 3. several videos per text: merged segments over cached slots
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_several_videos_per_text_in_one_call(tiny, mode):
    sc, tg = _index(tiny, mode)
    try:
        pairs = _v2t_pairs(tiny)
        assert np.max(np.bincount(pairs[:, 1])) >= 2
        plans = list(tg.iter_plans(pairs))
        assert len(plans) == 1 and plans[0].batch.own_start is not None and np.all(plans[0].pfx_slot.cpu().numpy() >= 0)
        want = sc.tvg(pairs)
        got = tg.tvg_pairs(pairs)
        assert np.all(np.isfinite(got)) and _close(got, want), float(np.max(np.abs(got - want)))
    finally:
        tg.close(); _set_tvg(tiny, sc, "full")


def test_several_videos_per_text_7b(b7):
    sc, tg = _index(b7, "full", max_tokens=1024)
    try:
        pairs = _v2t_pairs(b7)
        assert np.max(np.bincount(pairs[:, 1])) >= 2
        want = sc.tvg(pairs)
        got = tg.tvg_pairs(pairs)
        assert np.all(np.isfinite(got)) and _close(got, want), float(np.max(np.abs(got - want)))
    finally:
        tg.close()


# ---- 4. over budget
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_over_budget_mixes_cached_and_in_batch_prompts(tiny, mode):
    n_keys = len(TextGalleryIndex(G._scorer(tiny)).keys)
    for slots in (n_keys // 2, 0):
        sc, tg = _index(tiny, mode, budget_slots=slots)
        try:
            pairs = _v2t_pairs(tiny)
            if slots:                                              # cached and in-batch prompts in one call, for at least one query video
                mixed = 0
                for block in _per_video(pairs):
                    plans = list(tg.iter_plans(block))
                    sl = plans[0].pfx_slot.cpu().numpy()
                    mixed += len(plans) == 1 and bool((sl >= 0).any()) and plans[0].n_tokens > 3 * int((sl >= 0).sum())
                assert mixed >= 1
            _assert_bit_equal_per_video(sc, tg, pairs)
        finally:
            tg.close(); _set_tvg(tiny, sc, "full")


# ---- 5. staleness
def test_stale_slots_are_refused_and_refilled(tiny):
    t = tiny
    sc, tg = _index(t, "full")
    E = t.model.engine
    pairs = _v2t_pairs(t)
    try:
        _assert_bit_equal_per_video(sc, tg, pairs)
        # a weight change: the C call refuses the slots, the index refills them once
        plans = list(tg.iter_plans(pairs))
        E.load_weight("final_norm", t.w["final_norm"] * 1.01)
        with pytest.raises(eng.BlimError, match="stale"):
            tg.run(plans[0])
        _assert_bit_equal_per_video(sc, tg, pairs)
        # --tvg_precise full -> attn -> full: the slots recorded the MLP branch's compensation
        for mode in ("attn", "full"):
            plans = list(tg.iter_plans(pairs))
            _set_tvg(t, sc, mode)
            if sc.split_tvg:
                with pytest.raises(eng.BlimError, match="stale.*precise_mlp"):
                    tg.run(plans[0])
            _assert_bit_equal_per_video(sc, tg, pairs)
            assert tg._state[1] == mode
        # an option the slots recorded: refused by the engine itself
        plans = list(tg.iter_plans(pairs))
        E.set_option("masked_query_zero", 1)
        try:
            with pytest.raises(eng.BlimError, match="masked_query_zero"):
                tg.run(plans[0])
        finally:
            E.set_option("masked_query_zero", 0)
    finally:
        E.load_weight("final_norm", t.w["final_norm"])
        _set_tvg(t, sc, "full")
        tg.close()


def test_adapters_apart_invalidation(lora):
    t = lora
    sc, tg = _index(t, "full")
    pairs = _v2t_pairs(t)
    try:
        base = tg.tvg_pairs(pairs)
        for change in (lambda: G._load_adapters(t, 0.5), lambda: t.model.engine.clear_adapters(), lambda: G._load_adapters(t, 1.0)):
            plans = list(tg.iter_plans(pairs))
            change()
            with pytest.raises(eng.BlimError, match="stale"):              # blim_load_adapter / blim_clear_adapters make every slot stale
                tg.run(plans[0])
            _assert_bit_equal_per_video(sc, tg, pairs)                     # ... and the index refills
        assert np.array_equal(tg.tvg_pairs(pairs), base)
    finally:
        G._load_adapters(t, 1.0)
        tg.close()


# ---- 6. blend
def _combine_v2t(monkeypatch, ql, cand_l, prior, iv2, cpn, alpha, c, finetuned):
    """The blended v2t matrix training_utils.combine_and_rank builds from evaluation()'s matrices: captured where it hands it to get_recall for "blim"."""
    n = iv2.shape[0]
    seen = []
    monkeypatch.setattr(TU, "get_recall", lambda t2v, v2t, a, b: seen.append(np.array(v2t)) or {})
    v2t = {"internvideo2": iv2, "candidate_likelihood": cand_l, "query_likelihood": ql, "candidate_prior": prior}
    t2v = {k: np.zeros((n, n), np.float32) for k in v2t}
    args = types.SimpleNamespace(resume="finetuned.pth" if finetuned else "", eval=True, cpn=cpn, alpha=list(alpha), c=list(c))
    TU.combine_and_rank(t2v, v2t, args, n)
    monkeypatch.undo()
    return seen[-1]


def _rerank_case(t):
    n, k = t.spec["n"], t.spec["topk"]
    q = t.spec.get("queries", n)
    iv2 = t.prob.v2t_sims.astype(np.float32)
    cand = np.argsort(-iv2[:q], axis=1, kind="stable")[:, :k]
    videos = np.arange(q)
    pairs = np.stack([np.repeat(videos, k), cand.reshape(-1)], axis=1)
    return n, q, iv2, cand, videos, pairs


def _matrix(n, pairs, vals):
    M = np.full((n, n), -100.0, np.float32)
    M[pairs[:, 0], pairs[:, 1]] = vals
    return M


@pytest.mark.parametrize("cpn", [False, True])
def test_rerank_zero_shot_matches_combine_and_rank_row(tiny, monkeypatch, cpn):
    t = tiny
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    n, q, iv2, cand, videos, pairs = _rerank_case(t)
    cl = _matrix(n, pairs, sc.vtg(pairs))
    pr = _matrix(n, pairs, sc.vtg(pairs, cpn=True))
    alpha, c = (0.8, 0.3), (0.6, 0.5, 0.7, 0.5)
    full = _combine_v2t(monkeypatch, np.zeros((n, n), np.float32), cl, pr, iv2, cpn, alpha, c, False)
    gal = GalleryIndex(sc).build() if cpn else None                   # the VTG leg from cached video slots, or from PairScorer.vtg: the same bits
    tg = TextGalleryIndex(sc, video_index=gal)
    try:
        order, blended = tg.rerank(videos, cand, first_stage=np.take_along_axis(iv2[:q], cand, 1), cpn=cpn, alpha=alpha, c=c)
        assert tg.cache is None and tg._state is None                 # zero-shot: no TVG term, the caption cache is never filled
        for v in range(q):
            want = full[v, cand[v]]
            o = np.argsort(-want, kind="stable")
            assert np.array_equal(order[v], cand[v][o])
            assert np.array_equal(blended[v], want[o])
    finally:
        tg.close()
        if gal is not None:
            gal.close()


def test_rerank_finetuned_matches_combine_and_rank_row(lora, monkeypatch):
    """Fine-tuned: candidate likelihood and prior from the VTG path, query likelihood from the cached TVG path; several videos share a text here, so the blend
    agrees within 1e-5 and the order wherever neighbours are further apart.  An adapter reload in between: no prior or slot of the old weights survives."""
    t = lora
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    _set_tvg(t, sc, "full")
    n, q, iv2, cand, videos, pairs = _rerank_case(t)
    alpha, c = (0.8, 0.3), (0.6, 0.5, 0.7, 0.5)
    gal = GalleryIndex(sc).build()
    tg = TextGalleryIndex(sc, video_index=gal)
    seen = []
    try:
        for scale in (1.0, 0.5, 1.0):
            G._load_adapters(t, scale)
            cl = _matrix(n, pairs, sc.vtg(pairs))
            pr = _matrix(n, pairs, sc.vtg(pairs, cpn=True))
            ql = _matrix(n, pairs, sc.tvg(pairs))
            full = _combine_v2t(monkeypatch, ql, cl, pr, iv2, True, alpha, c, True)
            order, blended = tg.rerank(videos, cand, first_stage=np.take_along_axis(iv2[:q], cand, 1), cpn=True, alpha=alpha, c=c, finetuned=True)
            seen.append(blended.copy())
            for v in range(q):
                want = full[v, cand[v]]
                got = dict(zip(order[v].tolist(), blended[v].tolist()))
                for i, x in zip(cand[v].tolist(), want.tolist()):
                    assert abs(got[i] - x) <= 1e-5 * max(1.0, abs(x)), (scale, v, i, got[i], x)
                srt = np.sort(want)[::-1]
                if np.all(np.diff(-srt) > 1e-5):                          # order pinned only where neighbours are distinguishable
                    assert np.array_equal(order[v], cand[v][np.argsort(-want, kind="stable")])
                assert np.all(np.diff(blended[v]) <= 0)
        assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])      # the cached path is deterministic across refills
    finally:
        G._load_adapters(t, 1.0)
        tg.close(); gal.close()


# ---- 7. fp8
def test_fp8_engine_is_refused():
    t = P._build("tiny", dtype="f8")
    try:
        with pytest.raises(ValueError, match="fp8"):
            TextGalleryIndex(G._scorer(t))
    finally:
        t.model.engine.close()


# ---- 8. CLI
def test_search_cli_v2t_synthetic(tmp_path):
    out = tmp_path / "v.jsonl"
    r = subprocess.run([sys.executable, "-m", "blim_amd.search", "--synthetic", "64", "--direction", "v2t", "--video_ids", "0", "5", "--topk", "16", "--resume", "x",
                        "--cpn", "--c", "0.5", "0.5", "0.5", "0.5", "--output", str(out)], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    assert [x["query"] for x in lines] == ["video:0", "video:5"]
    for x in lines:
        assert len(x["texts"]) == 16 and len(set(x["texts"])) == 16 and all(np.isfinite(x["scores"]))
        assert x["scores"] == sorted(x["scores"], reverse=True)
