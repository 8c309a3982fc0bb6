"""GPU: run-time texts and micro-batched requests (PairScorer.add_texts, GalleryIndex.rerank_requests, `python -m blim_amd.search --serve`).  A text that joins
a scorer later scores bit for bit as a text given up front -- through PairScorer.vtg, an eager index built before it joined (a new prompt split is served in the
batch) and a lazy one (admitted on demand); VTG scores are bit-equal however requests are grouped (a GEMM row does not depend on its batch's composition, a
continuation reads the same prefix tiles in the same order: DESIGN.md sections 10 and 12); TVG scores follow section 11's rule (bit-equal when every text of the
call has one candidate, else within 1e-5 x max(1, |score|)).  The host side is tests/test_serve_host.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_lazy_gallery_gpu as LG
import test_text_gallery_gpu as TG
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd.gallery import GalleryIndex
from blim_amd.synth import IGNORE_INDEX
from test_gallery_gpu import lora, tiny  # noqa: F401  (fixtures: the tiny case and its fine-tuned twin, 6 videos and 2 layers, in fp16 and bf16)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_BLEND = (0.6, 0.5, 0.7, 0.5)


def _rows(t, second_split=()):
    """The problem's rows, unpadded: ([(ids, labels)] VTG, [(ids, labels)] TVG).  second_split: texts whose instruction differs in one token (a key of their own)."""
    prob = t.prob
    ids = [r.copy() for r in prob.vtg_ids]
    for i in second_split:
        at = int(np.argmax(prob.vtg_labels[i] != IGNORE_INDEX)) - 6
        ids[i][at] = ids[i][at] + 1
    cut = lambda a, m: np.asarray(a)[np.asarray(m) != 0]
    return ([(cut(ids[i], prob.vtg_masks[i]), cut(prob.vtg_labels[i], prob.vtg_masks[i])) for i in range(len(ids))],
            [(cut(prob.tvg_ids[i], prob.tvg_masks[i]), cut(prob.tvg_labels[i], prob.tvg_masks[i])) for i in range(len(ids))])


def _scorer(t, vtg_rows, tvg_rows, max_tokens=4096):
    """A scorer of the given unpadded rows over the problem's videos."""
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    T = lambda rows, k: [torch.from_numpy(r[k]) for r in rows]
    ones = lambda rows: [torch.ones(len(r[0]), dtype=torch.int64) for r in rows]
    vtg = RU.padding_ids(T(vtg_rows, 0), T(vtg_rows, 1), ones(vtg_rows), tok)
    tvg = RU.padding_ids(T(tvg_rows, 0), T(tvg_rows, 1), ones(tvg_rows), tok)
    prob = t.prob
    sc = RU.PairScorer(G.DDPLike(t.model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video],
                       torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels), t.dims.num_clips, max_tokens=max_tokens)
    sc.set_vtg_mode(t.model.vtg_mode())
    return sc


# ---- 1. late texts
@pytest.mark.parametrize("mode", ["none", "full"])
def test_late_texts_score_as_texts_given_up_front(tiny, mode):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, mode)
    vtg_rows, tvg_rows = _rows(t, second_split=(4,))                   # text 4 joins late AND brings a prompt split the indexes have not seen
    whole = _scorer(t, vtg_rows, tvg_rows)
    late = _scorer(t, vtg_rows[:n // 2], tvg_rows[:n // 2])
    eager = GalleryIndex(late).build()                                  # both indexes exist before the texts join
    lazy = LG._lazy(late)
    try:
        n_keys = len(eager.keys)
        assert late.add_texts(vtg_rows[n // 2:], tvg_rows[n // 2:]).tolist() == list(range(n // 2, n))
        pairs = np.array([[j, i] for j in range(n) for i in range(n)], np.int64)
        ref = whole.vtg(pairs)
        assert np.all(np.isfinite(ref))
        got = late.vtg(pairs)
        assert np.array_equal(got, ref), float(np.max(np.abs(got - ref)))
        got = eager.vtg_pairs(pairs)
        assert np.array_equal(got, ref), float(np.max(np.abs(got - ref)))
        assert len(eager.keys) == 2 * n_keys and len(eager.slot_of) == n_keys and eager.stats.misses == n      # the new split: one in-batch prefix per video
        half = pairs[pairs[:, 0] < n // 2]                              # n / 2 videos under two splits: as many keys as the lazy index has slots
        got, d = LG._delta(lazy, lambda: lazy.vtg_pairs(half))
        assert np.array_equal(got, ref[pairs[:, 0] < n // 2])
        assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (0, n, n, 0)
        got, d = LG._delta(lazy, lambda: lazy.vtg_pairs(half))
        assert np.array_equal(got, ref[pairs[:, 0] < n // 2])
        assert (d["hits"], d["misses"], d["prefix_tokens_packed"]) == (n, 0, 0)
        # TVG: one video per text -> bit-equal; the whole set -> section 11's rule
        for j in range(n):
            block = pairs[pairs[:, 0] == j]
            want = whole.tvg(block)
            assert np.all(np.isfinite(want)) and np.array_equal(late.tvg(block), want), j
        want, got = whole.tvg(pairs), late.tvg(pairs)
        assert TG._close(got, want), float(np.max(np.abs(got - want)))
    finally:
        eager.close(); lazy.close(); G._set_mode(t, "none")


# ---- 2. grouping
def _requests(t, n_texts):
    """8 requests, k_q in {1, 3, 5, N}, over every text; every other one with a first-stage row."""
    n = t.spec["n"]
    rng = np.random.RandomState(7)
    iv2 = t.prob.t2v_sims.astype(np.float32)
    out = []
    for q, k in enumerate([1, 3, 5, n, 3, 1, n, 5]):
        text = q % n_texts
        cand = rng.permutation(n)[:k]
        out.append((text, cand, iv2[text % n][cand] if q % 2 else None))
    return out


def _grouped(gal, reqs, size, **more):
    return [r for a in range(0, len(reqs), size) for r in gal.rerank_requests(reqs[a:a + size], **more)]


def test_grouping_leaves_zero_shot_results_bit_equal(tiny):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, "none")
    vtg_rows, tvg_rows = _rows(t)
    sc = _scorer(t, vtg_rows[:4], tvg_rows[:4])
    gal = GalleryIndex(sc).build()
    try:
        sc.add_texts(vtg_rows[4:], tvg_rows[4:])
        reqs = _requests(t, n)
        whole = _grouped(gal, reqs, len(reqs), c=C_BLEND)
        for size in (3, 1):
            for (o1, b1), (o2, b2) in zip(whole, _grouped(gal, reqs, size, c=C_BLEND)):
                assert np.array_equal(o1, o2) and np.array_equal(b1, b2), size
        for (text, cand, fs), (order, blended) in zip(reqs, whole):
            o, b = gal.rerank([text], cand[None], first_stage=None if fs is None else fs[None], c=C_BLEND)
            assert np.array_equal(order, o[0]) and np.array_equal(blended, b[0]) and np.all(np.isfinite(blended))
            ql = sc.vtg(np.stack([cand, np.full(len(cand), text)], axis=1))
            want = C_BLEND[2] * (C_BLEND[0] * ql + (1 - C_BLEND[0]) * np.zeros(len(cand))) + (1 - C_BLEND[2]) * (np.zeros(len(cand)) if fs is None else fs)
            assert np.array_equal(blended, want[np.argsort(-want, kind="stable")])
    finally:
        gal.close()


def test_grouping_on_the_fine_tuned_blend(lora):
    t = lora
    n = t.spec["n"]
    G._set_mode(t, "none")
    vtg_rows, tvg_rows = _rows(t)
    sc = _scorer(t, vtg_rows[:4], tvg_rows[:4])
    gal = GalleryIndex(sc).build()
    try:
        sc.add_texts(vtg_rows[4:], tvg_rows[4:])
        reqs = _requests(t, n)
        # the VTG term alone (c0 = c2 = 1: the blend is the query likelihood): bit-equal however the requests are grouped
        vtg_only = dict(cpn=True, alpha=(0.8, 0.3), c=(1.0, 0.0, 1.0, 0.0), finetuned=True)
        whole = _grouped(gal, reqs, len(reqs), **vtg_only)
        for size in (3, 1):
            for (o1, b1), (o2, b2) in zip(whole, _grouped(gal, reqs, size, **vtg_only)):
                assert np.array_equal(o1, o2) and np.array_equal(b1, b2), size
        for (text, cand, _), (order, blended) in zip(reqs, whole):
            ql = sc.vtg(np.stack([cand, np.full(len(cand), text)], axis=1))
            assert np.array_equal(blended, ql[np.argsort(-ql, kind="stable")]) and np.array_equal(order, cand[np.argsort(-ql, kind="stable")])
        # the blend: merged TVG sequences may be cut elsewhere -> section 11's rule, per candidate
        more = dict(cpn=True, alpha=(0.8, 0.3), c=C_BLEND, finetuned=True)
        per = [gal.rerank([text], cand[None], first_stage=None if fs is None else fs[None], **more) for text, cand, fs in reqs]
        for size in (len(reqs), 3, 1):
            for (text, cand, _), (order, blended), (o, b) in zip(reqs, _grouped(gal, reqs, size, **more), per):
                want = dict(zip(o[0].tolist(), b[0].tolist()))
                assert sorted(order.tolist()) == sorted(cand.tolist()) and np.all(np.diff(blended) <= 0)
                for j, v in zip(order.tolist(), blended.tolist()):
                    assert abs(v - want[j]) <= 1e-5 * max(1.0, abs(want[j])), (size, text, j, v, want[j])
                if len(cand) == 1 and size == 1:                          # one text with one candidate: the same call
                    assert np.array_equal(blended, b[0])
    finally:
        gal.close()


# ---- 3. a lazy index under pressure
def test_a_lazy_index_under_pressure_counts_a_batch_as_one_pass(tiny):
    t = tiny
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    gal = LG._lazy(sc, capacity=4)
    try:
        batch = [(0, [0, 1, 2], None), (1, [2, 3], None), (2, [4, 5, 0], None), (5, [1], None)]       # six keys, four slots

        def check(reqs, got):
            for (text, cand, _), (order, blended) in zip(reqs, got):
                want = sc.vtg(np.stack([order, np.full(len(order), text)], axis=1))
                assert sorted(order.tolist()) == sorted(cand) and np.all(np.isfinite(want))
                assert np.array_equal(blended, want), (text, float(np.max(np.abs(blended - want))))  # (c = 1 1 1 1: the blend is the likelihood)
        n_ran = len(gal.ran)
        got, d = LG._delta(gal, lambda: gal.rerank_requests(batch))
        check(batch, got)
        assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (0, 6, 4, 0) and len(gal.ran) == n_ran + 1
        assert {k[0] for k in gal.slot_of} == {0, 1, 2, 3}                 # the first four keys the planner met took the free slots
        got, d = LG._delta(gal, lambda: gal.rerank_requests(batch))        # every slot is needed by the pass: videos 4 and 5 stay in the batch
        check(batch, got)
        assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (4, 2, 0, 0)
        other = [(3, [4], None), (4, [5, 3], None)]                        # video 3 pinned; 4 and 5 take the slots of the least recently used: videos 0 and 1
        got, d = LG._delta(gal, lambda: gal.rerank_requests(other))
        check(other, got)
        assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (1, 2, 2, 2) and {k[0] for k in gal.slot_of} == {2, 3, 4, 5}
    finally:
        gal.close()


# ---- 4. the command
def test_serve_command_answers_alike_whatever_the_batch(tmp_path):
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)
    prob = synth.make_problem(1, 24, dims, tok_per_clip=8, fast_video=False)        # the dry run's problem (blim_amd/search.py: --synthetic 24)
    cut = lambda a, m: [int(x) for x in np.asarray(a)[np.asarray(m) != 0]]
    rows = lambda i: {"vtg_ids": cut(prob.vtg_ids[i], prob.vtg_masks[i]), "vtg_labels": cut(prob.vtg_labels[i], prob.vtg_masks[i]),
                      "tvg_ids": cut(prob.tvg_ids[i], prob.tvg_masks[i]), "tvg_labels": cut(prob.tvg_labels[i], prob.tvg_masks[i])}
    row5 = np.asarray(prob.t2v_sims[5], dtype=np.float32)
    top5 = np.argsort(-row5, kind="stable")[:5]
    lines = [json.dumps({"id": 0, "caption": 0}),
             json.dumps({"id": 1, "rows": rows(5), "candidate_idx": [int(j) for j in top5], "first_stage": [float(x) for x in row5[top5]]}),
             json.dumps({"id": 2, "caption": 5}),
             "{\"id\": 3, \"caption\"",
             json.dumps({"id": 4, "caption": 7, "candidates": ["3", "no such video"]}),
             json.dumps({"id": 5, "rows": rows(9), "candidate_idx": [4, 20, 11], "topk": 2}),
             json.dumps({"id": 6, "caption": 7}),
             json.dumps({"id": 7, "rows": rows(5), "candidate_idx": [2]}),
             json.dumps({"id": 8, "caption": 23}),
             json.dumps({"id": 9, "rows": rows(9)})]                                 # no first-stage row under --candidates iv2
    src = tmp_path / "requests.jsonl"
    src.write_text("\n".join(lines) + "\n")
    base = [sys.executable, "-m", "blim_amd.search", "--synthetic", "24", "--topk", "5", "--vtg_precise", "none", "--c", "0.5", "0.5", "0.5", "0.5"]
    runs = {}
    for B, more in ((1, []), (4, ["--batch_wait_ms", "50"])):
        with open(src) as stdin:
            r = subprocess.run(base + ["--serve", "--batch_queries", str(B)] + more, cwd=ROOT, stdin=stdin, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "gallery:" in r.stderr and "gallery stats:" in r.stderr
        runs[B] = r
    assert runs[1].stdout == runs[4].stdout
    out = [json.loads(x) for x in runs[1].stdout.splitlines()]
    assert [x["id"] for x in out] == [0, 1, 2, None, 4, 5, 6, 7, 8, 9]
    assert [n for n, x in enumerate(out) if "error" in x] == [3, 4, 9]
    assert "malformed" in out[3]["error"] and "unknown video id" in out[4]["error"] and "first-stage" in out[9]["error"]
    assert out[1]["videos"] == out[2]["videos"] and out[1]["scores"] == out[2]["scores"]          # caption 5 sent as rows: the same tokens, the same scores
    assert len(out[5]["videos"]) == 2 and set(out[5]["videos"]) <= {"4", "20", "11"} and out[7]["videos"] == ["2"] and out[7]["query"] == out[1]["query"]
    for B in (1, 4):
        summary = json.loads(runs[B].stderr.split("serve: ")[1].splitlines()[0])
        assert (summary["requests"], summary["errors"], summary["texts_added"]) == (10, 3, 2)
        assert summary["batches"] == 10 if B == 1 else summary["batches"] < 10
    r = subprocess.run(base + ["--query_ids", "0", "5", "7", "23"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = [json.loads(x) for x in r.stdout.splitlines()]
    served = [{k: v for k, v in out[n].items() if k != "id"} for n in (0, 2, 6, 8)]
    assert plain == served and [x["query"] for x in plain] == ["caption:0", "caption:5", "caption:7", "caption:23"]
