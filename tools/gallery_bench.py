"""Gallery index throughput (blim_amd/gallery.py): t2v VTG pairs/s of Q queries x top-k over N synthetic videos, the cached path (GalleryIndex.vtg_scores)
against the uncached PairScorer.vtg on the SAME pairs, alternated `--reps` times each in one process; the build time and bytes per slot; single-query latency
for k = 16 and k = N; in the plain and the fully compensated VTG mode.  Scores of the two paths are checked bit-equal on every repetition.

    python tools/gallery_bench.py --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r09_gallery.json

`--direction v2t`: the text gallery (TextGalleryIndex).  Per TVG mode (`--tvg_modes`): the TVG leg alone -- TextGalleryIndex.tvg_pairs against PairScorer.tvg on the
same Q x top-k (video, text) pairs, alternated -- with packed tokens, build time and bytes per slot; the whole fine-tuned v2t blend (VTG from cached video slots +
cached TVG + memoised prior against PairScorer.vtg + .tvg + .vtg(cpn=True)); single-query latency for k = 16 and k = N; the engine's timing classes of one cached
and one uncached TVG pass.  Several videos share a text in the Q x top-k set, so its scores are checked within 1e-5 x max(1, |score|) on every repetition; the
single-query sets (one video per text) are checked bit-equal.

    python tools/gallery_bench.py --direction v2t --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r10_text_gallery.json

`--fill lazy` (t2v): the lazy gallery (GalleryIndex(fill="lazy")) on the same protocol -- alternating repetitions in one process, medians.
(a) time to first result: eager = build() + the first query's top-k, lazy = allocation + the same query, all misses; (b) a pass of all misses with admission
against PairScorer.vtg on the same pairs (the price of the capture), with the host time of the calls alone; (c) the all-hit pass, lazy against eager; (d) a stream of
queries, one pass each, under a budget of a quarter of the gallery: hit rate and pairs/s, lazy against the static slot plan -- every query once, the same again,
and `--stream_draws` draws with a Zipf popularity over the queries.  Scores are checked bit-equal to PairScorer.vtg throughout.

    python tools/gallery_bench.py --fill lazy --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r11_lazy_gallery.json

`--host_gb G` (t2v): the lazy gallery's host tier (GalleryIndex(fill="lazy", host_budget_bytes=G GB)).  (a) the transfers alone, 16 slots at a
time: the export and import kernels (slot <-> device staging) and the whole spill and restore (with the copy to and from pinned host memory), ms per record and GB/s;
(b) the query streams of `--fill lazy` (d) under a quarter of the gallery, a lazy index without a tier against one with it, alternated in one process: hit rate,
pairs/s, time per query, and what the tier moved.  Scores are checked bit-equal to PairScorer.vtg throughout.

    python tools/gallery_bench.py --host_gb 10 --n 1000 --queries 55 --k 16 --reps 3 --synthetic_7b --out profiles/r15_host_tier.json

`--narrow_gemm` (t2v): engine option "narrow_gemm"  off (0) against auto (1), alternated `--reps` times in one process on ONE eager index: the
single-query latency table above (k = 16 and k = N, per mode), a stream of the Q queries one cached pass of k pairs each, and the engine's timing classes of one cached
k = 16 query under each value.  Option 0 launches the kernels the library launched before the option existed.  Scores are checked bit-equal between the two values
on every repetition.

    python tools/gallery_bench.py --narrow_gemm --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r16_narrow_gemm_gallery.json

`--narrow_lo6`: the same measurements for engine option "narrow_lo6" (the compensated o_proj and down launches that carry the e2m3 second
pass), in the compensated modes: t2v under `--modes full,select` (select: layers 0 - 3 compensated in every unit, the others plain), and with `--direction v2t` the
cached TVG leg of one k = 16 query under `--tvg_modes attn,full`.

    python tools/gallery_bench.py --narrow_lo6 --modes full,select --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r18_narrow_lo6_gallery.json
    python tools/gallery_bench.py --narrow_lo6 --direction v2t --n 1000 --k 16 --synthetic_7b --out profiles/r18_narrow_lo6_v2t.json

`--narrow_qkv`: the same measurements for engine option "narrow_qkv" (the QKV launch in all of its 16-bit forms), t2v under `--modes none,full` and
the v2t TVG leg.  The two older options stay on auto under BOTH values, so that 0 is the library as it ran with them before this option existed.

    python tools/gallery_bench.py --narrow_qkv --modes none,full --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r19_narrow_qkv_gallery.json
    python tools/gallery_bench.py --narrow_qkv --direction v2t --n 1000 --k 16 --synthetic_7b --out profiles/r19_narrow_qkv_v2t.json

`--serve_batch B [B ...]` (t2v): the stream of Q queries x top-k through GalleryIndex.rerank_requests in groups of B, against the per-query loop
of `python -m blim_amd.search` (one rerank() per query), the three narrow options on auto throughout, alternated `--reps` times in one process on ONE eager all-hit index:
ms per query, pairs/s, the latency of each request when all Q are queued at once (the time its group's call returned; median and worst), the narrow kernels' launch
counters and the packed tokens per pass.  Then a lazy index of a quarter of the gallery under `--fill lazy`'s Zipf stream: the loop, B = 1 and B = 8, a fresh index per
repetition.  Results are checked bit-equal to the per-query loop's on every repetition.

    python tools/gallery_bench.py --serve_batch 1 2 4 8 16 55 --modes none --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r20_serve.json

`--shortlist K [K ...]` (t2v): whole-gallery queries on the fine-tuned blend (c0 = 0.5, no first stage, no cpn) through
GalleryIndex.search_requests, the three narrow options on auto: `all` (every video a candidate: N VTG pairs and N TVG pairs per query) against `tvg` (the gallery
ranked by PairScorer.tvg_gallery, the best K reranked) at each K, per request and in groups of `--shortlist_batches`, alternated `--reps` times in one process on ONE
eager index: ms per query with stage 1's and stage 2's shares; stage 1 taken apart into host planning and engine calls; for `--recall_k` the share of queries whose
`all` top-1 / top-10 lie inside the shortlist -- on random weights, which says nothing about a trained checkpoint.  Every repetition is checked bit-equal to the
leg's first run, and the shortlisted answers bit-equal across the group sizes.

    python tools/gallery_bench.py --shortlist 16 64 256 --modes none --tvg_modes attn --n 1000 --queries 55 --synthetic_7b --out profiles/r21_shortlist.json

`--grow K` (t2v): videos that join a running gallery.  Scorers over the first N - K videos, with an eager index (spare_slots = K) and a lazy one
built, are grown through PairScorer.add_videos -- one video per call on one scorer, all K in one call on another -- and timed per added video: add_videos (the checks,
the clip means, the vocabulary registered again), the re-registration alone (Engine.set_video_vocab over all rows), the gallery_feats() rebuild, the eager index's
spare-slot fill (_sync_videos: the projection of the new videos and one packed fill), and the lazy index's first query of a new video (miss and admission) against the
same query again (hit).  Then the stream of Q queries x top-k over the grown eager index against an index built over all N from the start, alternated `--reps` times
in one process and checked bit-equal (a tvg_gallery query too), with the engine's timing classes of one stream each: the same classes with the same call counts.

    python tools/gallery_bench.py --grow 8 --modes none --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r24_gallery_grow.json

`--grow K --remove` (t2v): videos that leave a running gallery, with r24's protocol.  Scorers over all N videos, with an eager index (no spare
slot) and gallery_feats() made, lose K videos spread over the gallery through PairScorer.remove_videos -- one video per call on one scorer, all K in one call on
another -- timed per removed video: remove_videos (the checks, the tombstones, the vocabulary registered again), the re-registration alone (Engine.set_video_vocab over
the surviving rows), the gallery_feats() rebuild and the index sync (_sync_videos: keys, stamps and slots dropped).  Then a REPLACEMENT on the eager index with no spare
slot -- remove one video, add one, sync: the new prefix is filled into the freed slot -- against the only alternative without removal, measured in the same script: the
model loaded again and the index built again over the new set.  Then the stream of Q queries x top-k (candidates among the survivors) over the index after K removals
against an index built from the survivors, alternated `--reps` times in one process and checked bit-equal through the index map (a tvg_gallery query too), with the
engine's timing classes of one stream each.

    python tools/gallery_bench.py --grow 8 --remove --modes none --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r29_gallery_remove.json

`--shortlist K --prefilter K0 [K0 ...]` (t2v): `--shortlist`'s protocol (the fine-tuned blend, the narrow options on auto, one eager index,
`--gallery_gb` caps it) for the shortlist of K alone -- the parent's `--candidates tvg`, stage 1 over the whole gallery -- against the cascade at each K0: stage 0
(GalleryIndex._stage0: one logits row per query, ranked on the device), stage 1 (PairScorer.tvg over the K0 survivors), stage 2 (the cached VTG rerank of the best K),
per request and in groups of `--shortlist_batches`, alternated `--reps` times in one process; every repetition is checked bit-equal to the leg's first run.  Stage 0
is taken apart into host planning, the engine call (HIP events) and the rank kernel alone (HIP events, blim_tvg_rank on logits of the call's shape).  The share of
the parent shortlist's K videos that lie inside the K0 is reported -- on random weights, which says nothing about a trained checkpoint.  `--rank_kernel`: the rank
kernel alone at N = 1,000 and 100,000, 1 and 8 rows, k = 128, against what it replaces on the parent: the [rows, N] copy to the host plus np.argsort(kind="stable").

    python tools/gallery_bench.py --shortlist 16 --prefilter 64 128 256 --rank_kernel --modes none --tvg_modes attn --n 1000 --queries 55 --synthetic_7b --out profiles/r26_prefilter.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blim_amd import retrieval_utils as RU  # noqa: E402
from blim_amd import synth  # noqa: E402
from blim_amd.gallery import GalleryIndex, TextGalleryIndex  # noqa: E402
from blim_amd.modeling import BlimModel, DDPLike  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=55)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--synthetic_7b", action="store_true")
    ap.add_argument("--tok_per_clip", type=int, default=None, help="video tokens per clip (default: 64 for 7B rows, 8 otherwise)")
    ap.add_argument("--modes", default="none,full")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--max_tokens", type=int, default=24576)
    ap.add_argument("--direction", default="t2v", choices=["t2v", "v2t"])
    ap.add_argument("--tvg_modes", default="attn,full", help="v2t: the TVG calls' modes to measure")
    ap.add_argument("--fill", default="eager", choices=["eager", "lazy"], help="lazy: the lazy gallery's measurements (t2v)")
    ap.add_argument("--stream_draws", type=int, default=165, help="--fill lazy: queries of the Zipf stream")
    ap.add_argument("--host_gb", type=float, default=None, help="the host tier's measurements (t2v): pinned host memory of the tier, GB")
    ap.add_argument("--narrow_gemm", action="store_true", help="engine option narrow_gemm 0 against 1 (t2v, eager index): single-query latency, query stream, timing classes")
    ap.add_argument("--narrow_lo6", action="store_true", help="engine option narrow_lo6 0 against 1 in the compensated modes (t2v: --modes full,select; v2t: the TVG leg)")
    ap.add_argument("--narrow_qkv", action="store_true", help="engine option narrow_qkv 0 against 1, narrow_gemm and narrow_lo6 on auto throughout (t2v: --modes none,full; v2t: the TVG leg)")
    ap.add_argument("--serve_batch", type=int, nargs="+", default=None, metavar="B",
                    help="the query stream through GalleryIndex.rerank_requests in groups of B against the per-query loop, the three narrow options on auto (t2v)")
    ap.add_argument("--shortlist", type=int, nargs="+", default=None, metavar="K",
                    help="whole-gallery queries on the fine-tuned blend: --candidates all against --candidates tvg with a shortlist of K, per request and in batches (t2v)")
    ap.add_argument("--shortlist_batches", type=int, nargs="+", default=[1, 8], metavar="B", help="--shortlist: requests per pass")
    ap.add_argument("--recall_k", type=int, nargs="+", default=[16, 64, 256], metavar="K", help="--shortlist: the shortlist sizes whose cover of the `all` top-1 / top-10 is reported")
    ap.add_argument("--prefilter", type=int, nargs="+", default=None, metavar="K0", help="--shortlist K: the shortlist alone against the cascade with a prefilter of K0 (t2v)")
    ap.add_argument("--rank_kernel", action="store_true", help="--prefilter: also the rank kernel alone against the copy to the host plus np.argsort")
    ap.add_argument("--gallery_gb", type=float, default=None, help="--prefilter: device memory for the prefix cache (default: every video)")
    ap.add_argument("--grow", type=int, default=None, metavar="K", help="the index built over N - K videos and grown by K (PairScorer.add_videos) against one built over all N (t2v)")
    ap.add_argument("--remove", action="store_true", help="--grow K: the other way round -- K videos leave an index built over all N (PairScorer.remove_videos) against one built from the survivors")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = synth.ModelDims() if a.synthetic_7b else synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                                                                     num_kv_heads=1, mm_hidden_size=64)
    tpc = a.tok_per_clip or (64 if a.synthetic_7b else 8)
    model = BlimModel(dims, dtype=a.dtype)
    model.engine.init_synthetic_weights(0)
    prob = synth.make_problem(1, a.n, dims, tok_per_clip=tpc, fast_video=a.n > 256)
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    tok = type("T", (), {"pad_token_id": synth.PAD_ID})()
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    video = [torch.from_numpy(v) for v in prob.video]
    q = np.linspace(0, a.n - 1, a.queries).round().astype(np.int64)
    if (a.narrow_lo6 or a.narrow_qkv) and a.direction == "v2t":
        return main_narrow_v2t(a, dims, model, prob, vtg, tvg, video, q, tpc, option="narrow_qkv" if a.narrow_qkv else "narrow_lo6")
    if a.direction == "v2t":
        return main_v2t(a, dims, model, prob, vtg, tvg, video, q, tpc)
    if a.grow and a.remove:
        return main_remove(a, dims, model, prob, vtg, tvg, video, q, tpc)
    if a.grow:
        return main_grow(a, dims, model, prob, vtg, tvg, video, q, tpc)
    if a.shortlist and a.prefilter:
        return main_prefilter(a, dims, model, prob, vtg, tvg, video, q, tpc)
    if a.shortlist:
        return main_shortlist(a, dims, model, prob, vtg, tvg, video, q, tpc)
    if a.serve_batch:
        return main_serve(a, dims, model, prob, vtg, tvg, video, q, tpc)
    if a.narrow_gemm or a.narrow_lo6 or a.narrow_qkv:
        return main_narrow(a, dims, model, prob, vtg, tvg, video, q, tpc, option="narrow_qkv" if a.narrow_qkv else "narrow_lo6" if a.narrow_lo6 else "narrow_gemm")
    if a.host_gb is not None:
        return main_host(a, dims, model, prob, vtg, tvg, video, q, tpc)
    if a.fill == "lazy":
        return main_lazy(a, dims, model, prob, vtg, tvg, video, q, tpc)
    cand = np.argsort(-prob.t2v_sims[q], axis=1, kind="stable")[:, :a.k]
    pairs = np.stack([cand.reshape(-1), np.repeat(q, a.k)], axis=1)
    res = {"n": a.n, "queries": a.queries, "k": a.k, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc, "modes": {}}
    for mode in a.modes.split(","):
        model.vtg_precise = None if mode == "none" else mode
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode())
        sc.vtg(pairs[:8])                                                  # warm-up: features projected, workspaces sized
        gal = GalleryIndex(sc)
        t_build, _ = timed(gal.build)
        gal.vtg_pairs(pairs[:8])
        tok_unc = sum(p.n_tokens for p in sc.iter_vtg(pairs))
        tok_cac = sum(p.n_tokens for p in gal.iter_plans(pairs))
        t_unc, t_cac = [], []
        for _ in range(a.reps):
            dt, ref = timed(lambda: sc.vtg(pairs)); t_unc.append(dt)
            dt, got = timed(lambda: gal.vtg_pairs(pairs)); t_cac.append(dt)
            assert np.array_equal(ref, got), "cached scores differ from PairScorer.vtg"
        lat = {}
        for kk in (16, a.n):
            c1 = np.argsort(-prob.t2v_sims[q[0]], kind="stable")[:kk][None]
            gal.vtg_scores([q[0]], c1)
            ts = [timed(lambda: gal.vtg_scores([q[0]], c1))[0] for _ in range(3)]
            p1 = np.stack([c1[0], np.full(kk, q[0])], axis=1)
            tu = [timed(lambda: sc.vtg(p1))[0] for _ in range(3)]
            lat[f"k{kk}"] = {"cached_ms": 1e3 * float(np.median(ts)), "uncached_ms": 1e3 * float(np.median(tu))}
        P = len(pairs)
        r = {"build_s": t_build, "slots": len(gal.slot_of), "bytes_per_slot": gal.cache.bytes // len(gal.slot_of), "tokens_uncached": tok_unc,
             "tokens_cached": tok_cac, "uncached_s": t_unc, "cached_s": t_cac, "uncached_pairs_per_s": P / float(np.median(t_unc)),
             "cached_pairs_per_s": P / float(np.median(t_cac)), "speedup": float(np.median(t_unc) / np.median(t_cac)), "latency": lat, "bit_equal": True}
        res["modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        gal.close()
        del sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_narrow(a, dims, model, prob, vtg, tvg, video, q, tpc, option="narrow_gemm"):
    """Option "narrow_gemm" (or "narrow_lo6", "narrow_qkv") 0 against 1 on one eager index (see the module text)."""
    from blim_amd import engine as eng
    e = model.engine
    launches_of, threshold = {"narrow_qkv": (eng.gemm_narrow_qkv_launches, eng.gemm_narrow_qkv_threshold), "narrow_lo6": (eng.gemm_narrow_lo6_launches, eng.gemm_narrow_lo6_threshold),
                              "narrow_gemm": (eng.gemm_narrow_launches, eng.gemm_narrow_threshold)}[option]
    if option == "narrow_qkv":                                             # the background of both values: the older options on auto
        e.set_option("narrow_gemm", 1); e.set_option("narrow_lo6", 1)
    res = {"n": a.n, "queries": a.queries, "k": a.k, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc, "reps": a.reps,
           "threshold_tiles": threshold(), "modes": {}}
    if option != "narrow_gemm":
        res["option"] = option
    if option == "narrow_qkv":
        res["background"] = {"narrow_gemm": 1, "narrow_lo6": 1}
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x))
    for mode in a.modes.split(","):
        model.vtg_precise = None if mode == "none" else mode
        if mode == "select":                                               # a fixed mask instead of a calibration: the first four layers compensated in every unit
            model.resolve_vtg("select", np.array([15 if li < 4 else 0 for li in range(dims.num_layers)], dtype=np.uint8))
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode())
        sc.vtg(np.stack([np.arange(8), np.full(8, q[0])], axis=1))
        gal = GalleryIndex(sc)
        gal.build()
        r = {"latency": {}}

        def latency(tq, c1):
            ts, launches, ref = {0: [], 1: []}, {}, None
            for v in (0, 1):                                               # warm-up of both kernels' paths
                e.set_option(option, v); gal.vtg_scores([tq], c1)
            for _ in range(a.reps):
                for v in (0, 1):
                    e.set_option(option, v)
                    n0 = launches_of()
                    dt, got = timed(lambda: gal.vtg_scores([tq], c1))
                    ts[v].append(dt); launches[v] = launches_of() - n0
                    ref = got if ref is None else ref
                    assert np.array_equal(np.asarray(ref), np.asarray(got)), "scores differ between the option's values 0 and 1"
            return {"off_ms": 1e3 * med(ts[0]), "auto_ms": 1e3 * med(ts[1]), "off_spread": spread(ts[0]), "auto_spread": spread(ts[1]),
                    "off_all_ms": [1e3 * t for t in ts[0]], "auto_all_ms": [1e3 * t for t in ts[1]], "narrow_launches": launches}
        for kk in (a.k, a.n):
            r["latency"][f"k{kk}"] = latency(q[0], np.argsort(-prob.t2v_sims[q[0]], kind="stable")[:kk][None])
        cand = np.argsort(-prob.t2v_sims[q], axis=1, kind="stable")[:, :a.k]
        ts = {0: [], 1: []}

        def stream():
            return [np.asarray(gal.vtg_scores([int(t)], cand[i][None])) for i, t in enumerate(q)]
        ref = None
        for _ in range(a.reps):
            for v in (0, 1):
                e.set_option(option, v)
                dt, got = timed(stream); ts[v].append(dt)
                ref = got if ref is None else ref
                assert all(np.array_equal(x, y) for x, y in zip(ref, got)), "stream scores differ between the option's values 0 and 1"
        r["stream"] = {"queries": len(q), "k": a.k, "off_s": med(ts[0]), "auto_s": med(ts[1]), "off_spread": spread(ts[0]), "auto_spread": spread(ts[1]),
                       "off_ms_per_query": 1e3 * med(ts[0]) / len(q), "auto_ms_per_query": 1e3 * med(ts[1]) / len(q)}

        def classes(tq, c1):
            out = {}
            for v in (0, 1):
                e.set_option(option, v)
                e.timing_enable(True); e.timing_report()
                gal.vtg_scores([tq], c1)
                out["auto" if v else "off"] = {k: x for k, x in e.timing_report().items() if x["calls"]}
                e.timing_enable(False)
            return out
        r["classes"] = classes(q[0], np.argsort(-prob.t2v_sims[q[0]], kind="stable")[:a.k][None])
        if option == "narrow_qkv":
            # QKV's N has 18 column tiles where the residual GEMMs' has 14: the same query can sit on the other side of this option's threshold.  The packed tokens of
            # every query of the stream, how many narrow launches one stream makes, and the same two measurements for the stream's median query (by packed tokens)
            toks = [int(sum(p.n_tokens for p in gal.iter_plans(np.stack([cand[i], np.full(a.k, t)], axis=1)))) for i, t in enumerate(q)]
            e.set_option(option, 1)
            n0 = launches_of(); stream(); r["stream"]["narrow_launches"] = launches_of() - n0
            r["stream"]["tokens_per_query"] = toks
            r["stream"]["tokens_first_query"] = toks[0]
            im = int(np.argsort(toks, kind="stable")[len(toks) // 2])
            r["median_query"] = {"index": im, "tokens": toks[im], "latency": latency(int(q[im]), cand[im][None]), "classes": classes(int(q[im]), cand[im][None])}
        e.set_option(option, 0)
        res["modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        gal.close()
        del sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_narrow_v2t(a, dims, model, prob, vtg, tvg, video, q, tpc, option="narrow_lo6"):
    """Option "narrow_lo6" (or "narrow_qkv") 0 against 1 on the cached TVG leg of one v2t query of k candidates, per TVG mode (see the module text)."""
    from blim_amd import engine as eng
    e = model.engine
    launches_of, threshold = ((eng.gemm_narrow_qkv_launches, eng.gemm_narrow_qkv_threshold) if option == "narrow_qkv" else
                              (eng.gemm_narrow_lo6_launches, eng.gemm_narrow_lo6_threshold))
    if option == "narrow_qkv":                                             # the background of both values: the older options on auto
        e.set_option("narrow_gemm", 1); e.set_option("narrow_lo6", 1)
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x))
    res = {"direction": "v2t", "option": option, "n": a.n, "k": a.k, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc,
           "reps": a.reps, "threshold_tiles": threshold(), "tvg_modes": {}}
    model.vtg_precise = None
    c1 = np.argsort(-prob.v2t_sims[q[0]], kind="stable")[:a.k]
    p1 = np.stack([np.full(a.k, q[0]), c1], axis=1)
    for mode in a.tvg_modes.split(","):
        model.tvg_precise = mode
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode()); sc.set_tvg_mode(model.tvg_mode())
        sc.tvg(p1[:8])
        gal = GalleryIndex(sc)
        gal.build()
        tg = TextGalleryIndex(sc, video_index=gal)
        tg.build()
        ts, launches, ref = {0: [], 1: []}, {}, None
        for v in (0, 1):
            e.set_option(option, v); tg.tvg_pairs(p1)
        for _ in range(a.reps):
            for v in (0, 1):
                e.set_option(option, v)
                n0 = launches_of()
                dt, got = timed(lambda: tg.tvg_pairs(p1))
                ts[v].append(dt); launches[v] = launches_of() - n0
                ref = got if ref is None else ref
                assert np.array_equal(ref, got), "TVG scores differ between the option's values 0 and 1"
        r = {"off_ms": 1e3 * med(ts[0]), "auto_ms": 1e3 * med(ts[1]), "off_spread": spread(ts[0]), "auto_spread": spread(ts[1]),
             "off_all_ms": [1e3 * t for t in ts[0]], "auto_all_ms": [1e3 * t for t in ts[1]], "narrow_launches": launches,
             "tokens_cached": sum(p.n_tokens for p in tg.iter_plans(p1)), "classes": {}}
        for v in (0, 1):
            e.set_option(option, v)
            e.timing_enable(True); e.timing_report()
            tg.tvg_pairs(p1)
            r["classes"]["auto" if v else "off"] = {k: x for k, x in e.timing_report().items() if x["calls"]}
            e.timing_enable(False)
        e.set_option(option, 0)
        res["tvg_modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        tg.close(); gal.close()
        del sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_serve(a, dims, model, prob, vtg, tvg, video, q, tpc):
    """`--serve_batch`: the stream of Q queries x top-k through GalleryIndex.rerank_requests in groups of B against the per-query loop (see the module text)."""
    from blim_amd import engine as eng
    e = model.engine
    counters = {"narrow_gemm": eng.gemm_narrow_launches, "narrow_lo6": eng.gemm_narrow_lo6_launches, "narrow_qkv": eng.gemm_narrow_qkv_launches}
    for o in counters:
        e.set_option(o, 1)
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x))
    Q = len(q)
    sizes = sorted(set(min(int(b), Q) for b in a.serve_batch))
    cand = np.argsort(-prob.t2v_sims[q], axis=1, kind="stable")[:, :a.k]
    reqs = [(int(t), cand[i], None) for i, t in enumerate(q)]
    res = {"serve_batch": sizes, "n": a.n, "queries": a.queries, "k": a.k, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc, "reps": a.reps,
           "options": {o: 1 for o in counters}, "thresholds_tiles": {"narrow_gemm": eng.gemm_narrow_threshold(), "narrow_lo6": eng.gemm_narrow_lo6_threshold(),
                                                                     "narrow_qkv": eng.gemm_narrow_qkv_threshold()}, "modes": {}}

    def grouped(gal, items, B, stamps=None):
        out, t0 = [], time.perf_counter()
        for lo in range(0, len(items), B):
            out += gal.rerank_requests(items[lo:lo + B])              # (the scores come back to the host: the call has finished when it returns)
            if stamps is not None:
                stamps += [time.perf_counter() - t0] * len(items[lo:lo + B])
        return out

    for mode in a.modes.split(","):
        model.vtg_precise = None if mode == "none" else mode
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode())
        sc.vtg(np.stack([np.arange(8), np.full(8, q[0])], axis=1))
        gal = GalleryIndex(sc)
        gal.build()

        def loop():                                                      # the per-query loop of `python -m blim_amd.search` without --serve: one rerank() per query
            return [gal.rerank([t], c[None]) for t, c, _ in reqs]
        ref = [(o[0], b[0]) for o, b in loop()]
        legs = ["loop"] + [f"B{B}" for B in sizes]
        ts = {leg: [] for leg in legs}
        lat = {leg: [] for leg in legs}
        for B in sizes:                                                  # warm-up of every batch size's workspaces
            grouped(gal, reqs, B)
        for _ in range(a.reps):
            for leg in legs:
                stamps = []
                if leg == "loop":
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = []
                    for t, c, _ in reqs:
                        o, b = gal.rerank([t], c[None]); got.append((o[0], b[0])); stamps.append(time.perf_counter() - t0)
                    dt = time.perf_counter() - t0
                else:
                    dt, got = timed(lambda: grouped(gal, reqs, int(leg[1:]), stamps))
                ts[leg].append(dt); lat[leg].append(stamps)
                assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(got, ref)), f"{leg}: results differ from the per-query loop"
        r = {"eager": {}}
        for leg in legs:
            B = 1 if leg == "loop" else int(leg[1:])
            n0 = {o: f() for o, f in counters.items()}
            if leg == "loop":
                loop()
            else:
                grouped(gal, reqs, B)
            launches = {o: f() - n0[o] for o, f in counters.items()}
            tokens = [int(sum(p.n_tokens for p in gal.iter_plans(np.concatenate([np.stack([c, np.full(len(c), t)], axis=1) for t, c, _ in reqs[lo:lo + B]]))))
                      for lo in range(0, Q, B)]
            worst = [max(s) for s in lat[leg]]
            mid = [float(np.median(s)) for s in lat[leg]]
            r["eager"][leg] = {"s": ts[leg], "ms_per_query": 1e3 * med(ts[leg]) / Q, "pairs_per_s": Q * a.k / med(ts[leg]), "spread": spread(ts[leg]),
                               "ratio_to_loop": med(ts["loop"]) / med(ts[leg]), "latency_median_ms": 1e3 * med(mid), "latency_worst_ms": 1e3 * med(worst),
                               "narrow_launches": launches, "passes": len(tokens), "tokens_per_pass_median": float(np.median(tokens)), "tokens_per_pass_max": int(max(tokens))}
        # the lazy index under a quarter of the gallery, r11's Zipf stream: the per-query loop, B = 1 and B = 8; a fresh index per repetition and leg
        per = gal.per_slot_bytes()
        gal.close()
        rng = np.random.RandomState(0)
        w = 1.0 / np.arange(1, Q + 1); w /= w.sum()
        order = rng.choice(Q, size=a.stream_draws, p=w)
        zreqs = [reqs[i] for i in order]
        zlegs = ["loop"] + [f"B{B}" for B in (1, 8) if B <= Q]
        zt, zs = {leg: [] for leg in zlegs}, {}
        for _ in range(a.reps):
            for leg in zlegs:
                g = GalleryIndex(sc, budget_bytes=(a.n // 4) * per, fill="lazy").build()
                if leg == "loop":
                    dt, got = timed(lambda: [(o[0], b[0]) for o, b in (g.rerank([t], c[None]) for t, c, _ in zreqs)])
                else:
                    dt, got = timed(lambda: grouped(g, zreqs, int(leg[1:])))
                assert all(np.array_equal(o, ref[i][0]) and np.array_equal(b, ref[i][1]) for (o, b), i in zip(got, order)), f"lazy {leg}: results differ from the eager per-query loop"
                st = g.stats.as_dict()
                zt[leg].append(dt); zs[leg] = dict(st, hit_rate=st["hits"] / max(st["hits"] + st["misses"], 1))
                g.close()
        r["lazy_zipf"] = {"slots": a.n // 4, "draws": int(a.stream_draws),
                          **{leg: dict(zs[leg], s=zt[leg], ms_per_query=1e3 * med(zt[leg]) / len(order), pairs_per_s=len(order) * a.k / med(zt[leg]), spread=spread(zt[leg]),
                                       ratio_to_loop=med(zt["loop"]) / med(zt[leg])) for leg in zlegs}}
        res["modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        del sc
        torch.cuda.empty_cache()
    for o in counters:
        e.set_option(o, 0)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_grow(a, dims, model, prob, vtg, tvg, video, q, tpc):
    """`--grow K`: a gallery built over N - K videos and grown by K against one built over all N (see the module text)."""
    e = model.engine
    N, K = a.n, int(a.grow)
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x)) if len(x) > 1 else 0.0
    ms = lambda x: [1e3 * float(t) for t in x]
    vocab, labels = torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels)
    cand = np.argsort(-prob.t2v_sims[q], axis=1, kind="stable")[:, :a.k]
    res = {"grow": K, "n": N, "queries": a.queries, "k": a.k, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc, "reps": a.reps, "modes": {}}

    def scorer(n):
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video[:n], vocab[:n], labels[:n], dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode())
        return sc

    for mode in a.modes.split(","):
        model.vtg_precise = None if mode == "none" else mode
        model.tvg_precise = a.tvg_modes.split(",")[0]
        model.clear_cache()
        whole = scorer(N)
        whole.set_tvg_mode(model.tvg_mode())
        whole.vtg(np.stack([np.arange(8), np.full(8, q[0])], axis=1))      # warm-up: workspaces sized
        ref_gal = GalleryIndex(whole)
        t_build, _ = timed(ref_gal.build)
        t_feats_whole, _ = timed(whole.gallery_feats)
        r = {"from_start": {"build_s": t_build, "slots": len(ref_gal.slot_of), "gallery_feats_s": t_feats_whole}}

        def grown(batch):
            """A scorer over N - K videos with its indexes built and gallery_feats() made, grown by K videos one at a time or in one call."""
            sc = scorer(N - K)
            sc.set_tvg_mode(model.tvg_mode())
            eager = GalleryIndex(sc, spare_slots=K)
            tb, _ = timed(eager.build)
            lazy = GalleryIndex(sc, fill="lazy").build()
            sc.gallery_feats()
            steps = [list(range(N - K, N))] if batch else [[j] for j in range(N - K, N)]
            t = {"add_videos": [], "gallery_feats": [], "spare_fill": [], "lazy_first": [], "lazy_again": []}
            for js in steps:
                dt, got = timed(lambda: sc.add_videos([video[j] for j in js], vocab[js])); t["add_videos"].append(dt / len(js))
                assert got.tolist() == js
                dt, _ = timed(sc.gallery_feats); t["gallery_feats"].append(dt / len(js))
                dt, _ = timed(eager._sync_videos); t["spare_fill"].append(dt / len(js))
                assert all(eager.keys[j] in eager.slot_of for j in js)
                pairs = np.stack([np.asarray(js), np.full(len(js), q[0])], axis=1)
                dt, first = timed(lambda: lazy.vtg_pairs(pairs)); t["lazy_first"].append(dt / len(js))
                dt, again = timed(lambda: lazy.vtg_pairs(pairs)); t["lazy_again"].append(dt / len(js))
                assert np.array_equal(first, again) and np.array_equal(first, ref_gal.vtg_pairs(pairs)), "a grown lazy index's scores differ from the from-start index's"
            assert lazy.stats.admitted == K and lazy.stats.hits == K
            lazy.close()
            out = {"build_s": tb, "calls": len(steps), **{k + "_ms_per_video": {"median": med(ms(v)), "min": min(ms(v)), "max": max(ms(v)), "first_call": ms(v)[0]} for k, v in t.items()}}
            return sc, eager, out

        sc1, gal1, r["one_at_a_time"] = grown(False)
        sc2, gal2, r["one_batch"] = grown(True)
        gal2.close()
        # the re-registration alone: all N rows through the engine's split
        t_reg = [timed(lambda: e.set_video_vocab(sc1._vocab_src))[0] for _ in range(max(a.reps, 3))]
        r["set_video_vocab_ms"] = {"rows": int(sc1.n_vocab), "bytes": int(sc1._vocab_src.numel() * 4), "median": med(ms(t_reg)), "min": min(ms(t_reg)), "spread": spread(t_reg)}
        on_device = sc1._vocab_src.to(model.device)
        t_reg = [timed(lambda: e.set_video_vocab(on_device))[0] for _ in range(max(a.reps, 3))]
        r["set_video_vocab_device_rows_ms"] = {"median": med(ms(t_reg)), "min": min(ms(t_reg)), "spread": spread(t_reg)}
        # the same stream after the growth and from the start
        stream = lambda gal: [gal.rerank([int(t)], cand[i][None]) for i, t in enumerate(q)]
        ref = stream(ref_gal); stream(gal1)
        ts = {"grown": [], "from_start": []}
        for _ in range(a.reps):
            for leg, gal in (("grown", gal1), ("from_start", ref_gal)):
                dt, got = timed(lambda: stream(gal)); ts[leg].append(dt)
                assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(got, ref)), f"{leg}: the stream's results differ"
        classes = {}
        for leg, gal in (("grown", gal1), ("from_start", ref_gal)):
            e.timing_enable(True); e.timing_report()
            stream(gal)
            classes[leg] = {k: x for k, x in e.timing_report().items() if x["calls"]}
            e.timing_enable(False)
        same = {k: x["calls"] for k, x in classes["grown"].items()} == {k: x["calls"] for k, x in classes["from_start"].items()}
        tokens = {leg: int(sum(p.n_tokens for i, t in enumerate(q) for p in gal.iter_plans(np.stack([cand[i], np.full(a.k, t)], axis=1))))
                  for leg, gal in (("grown", gal1), ("from_start", ref_gal))}
        r["stream"] = {leg: {"s": ts[leg], "ms_per_query": 1e3 * med(ts[leg]) / len(q), "spread": spread(ts[leg]), "packed_tokens": tokens[leg]} for leg in ts}
        r["stream"].update(ratio_grown_to_from_start=med(ts["grown"]) / med(ts["from_start"]), same_classes_and_calls=bool(same), classes=classes,
                           new_videos_among_candidates=int(np.sum(cand >= N - K)), stats_grown=gal1.stats.as_dict(), stats_from_start=ref_gal.stats.as_dict())
        texts = [int(q[0]), int(q[-1])]
        dt1, g1 = timed(lambda: sc1.tvg_gallery(texts)); dt2, g2 = timed(lambda: whole.tvg_gallery(texts))
        assert np.array_equal(g1, g2), "tvg_gallery over the grown scorer differs from the from-start scorer's"
        r["tvg_gallery_two_texts_ms"] = {"grown": 1e3 * dt1, "from_start": 1e3 * dt2, "bit_equal": True}
        res["modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        gal1.close(); ref_gal.close()
        del sc1, sc2, whole
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_remove(a, dims, model, prob, vtg, tvg, video, q, tpc):
    """`--grow K --remove`: K videos leave a gallery built over all N, against one built from the survivors (see the module text)."""
    e = model.engine
    N, K = a.n, int(a.grow)
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x)) if len(x) > 1 else 0.0
    ms = lambda x: [1e3 * float(t) for t in x]
    vocab = torch.from_numpy(prob.video_vocab)
    gone = np.unique(np.linspace(1, N - 2, K).round().astype(np.int64))            # the videos that leave: spread over the gallery, never a query's own
    gone = np.array([j for j in gone if j not in set(q.tolist())], dtype=np.int64)
    K = len(gone)
    keep = np.array([j for j in range(N) if j not in set(gone.tolist())], dtype=np.int64)
    place = -np.ones(N, dtype=np.int64); place[keep] = np.arange(len(keep))         # a survivor's index in the gallery built from the survivors
    sims = prob.t2v_sims[q].copy(); sims[:, gone] = -np.inf
    cand = np.argsort(-sims, axis=1, kind="stable")[:, :a.k]                        # candidates among the survivors
    res = {"remove": K, "removed": gone.tolist(), "n": N, "queries": a.queries, "k": a.k, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc,
           "reps": a.reps, "modes": {}}

    def scorer(ids):
        ids = [int(j) for j in ids]
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [video[j] for j in ids], vocab[ids], torch.arange(len(ids)), dims.num_clips,
                           max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode())
        sc.set_tvg_mode(model.tvg_mode())
        return sc

    for mode in a.modes.split(","):
        model.vtg_precise = None if mode == "none" else mode
        model.tvg_precise = a.tvg_modes.split(",")[0]
        model.clear_cache()
        fresh = scorer(keep)
        fresh.vtg(np.stack([np.arange(8), np.full(8, q[0])], axis=1))               # warm-up: workspaces sized
        ref_gal = GalleryIndex(fresh)
        t_build, _ = timed(ref_gal.build)
        t_feats, _ = timed(fresh.gallery_feats)
        r = {"from_survivors": {"build_s": t_build, "slots": len(ref_gal.slot_of), "gallery_feats_s": t_feats}}

        def shrunk(batch):
            """A scorer over all N videos with its eager index built and gallery_feats() made, losing K videos one at a time or in one call."""
            sc = scorer(range(N))
            eager = GalleryIndex(sc, spare_slots=0)
            tb, _ = timed(eager.build)
            sc.gallery_feats()
            steps = [gone.tolist()] if batch else [[int(j)] for j in gone]
            t = {"remove_videos": [], "gallery_feats": [], "index_sync": []}
            for js in steps:
                dt, _ = timed(lambda: sc.remove_videos(js)); t["remove_videos"].append(dt / len(js))
                dt, _ = timed(sc.gallery_feats); t["gallery_feats"].append(dt / len(js))
                dt, _ = timed(eager._sync_videos); t["index_sync"].append(dt / len(js))
                assert not any(k[0] in js for k in eager.keys) and not any(k[0] in js for k in eager.slot_of)
            assert eager.removed_stats == {"videos": K, "slots_freed": K, "records_forgotten": 0} and sc.n_live == N - K
            out = {"build_s": tb, "calls": len(steps), **{k + "_ms_per_video": {"median": med(ms(v)), "min": min(ms(v)), "max": max(ms(v)), "first_call": ms(v)[0]} for k, v in t.items()}}
            return sc, eager, out

        sc1, gal1, r["one_at_a_time"] = shrunk(False)
        sc2, gal2, r["one_batch"] = shrunk(True)
        gal2.close()
        # the re-registration alone: the surviving rows through the engine's split
        t_reg = [timed(lambda: e.set_video_vocab(sc1._vocab_src))[0] for _ in range(max(a.reps, 3))]
        r["set_video_vocab_ms"] = {"rows": int(sc1.n_vocab), "bytes": int(sc1._vocab_src.numel() * 4), "median": med(ms(t_reg)), "min": min(ms(t_reg)), "spread": spread(t_reg)}
        # the same stream after the removals and from the survivors
        stream = lambda gal, at: [gal.rerank([int(t)], at[cand[i]][None]) for i, t in enumerate(q)]
        ident = np.arange(N)
        ref = stream(ref_gal, place); stream(gal1, ident)
        ts = {"removed": [], "from_survivors": []}
        for _ in range(a.reps):
            for leg, gal, at in (("removed", gal1, ident), ("from_survivors", ref_gal, place)):
                dt, got = timed(lambda: stream(gal, at)); ts[leg].append(dt)
                back = ident if leg == "removed" else keep
                assert all(np.array_equal(back[o], keep[o1]) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(got, ref)), f"{leg}: the stream's results differ"
        classes = {}
        for leg, gal, at in (("removed", gal1, ident), ("from_survivors", ref_gal, place)):
            e.timing_enable(True); e.timing_report()
            stream(gal, at)
            classes[leg] = {k: x for k, x in e.timing_report().items() if x["calls"]}
            e.timing_enable(False)
        same = {k: x["calls"] for k, x in classes["removed"].items()} == {k: x["calls"] for k, x in classes["from_survivors"].items()}
        tokens = {leg: int(sum(p.n_tokens for i, t in enumerate(q) for p in gal.iter_plans(np.stack([at[cand[i]], np.full(a.k, t)], axis=1))))
                  for leg, gal, at in (("removed", gal1, ident), ("from_survivors", ref_gal, place))}
        r["stream"] = {leg: {"s": ts[leg], "ms_per_query": 1e3 * med(ts[leg]) / len(q), "spread": spread(ts[leg]), "packed_tokens": tokens[leg]} for leg in ts}
        r["stream"].update(ratio_removed_to_from_survivors=med(ts["removed"]) / med(ts["from_survivors"]), same_classes_and_calls=bool(same), classes=classes,
                           stats_removed=gal1.stats.as_dict(), stats_from_survivors=ref_gal.stats.as_dict())
        texts = [int(q[0]), int(q[-1])]
        dt1, g1 = timed(lambda: sc1.tvg_gallery(texts)); dt2, g2 = timed(lambda: fresh.tvg_gallery(texts))
        assert np.array_equal(g1[:, keep], g2) and np.isnan(g1[:, gone]).all(), "tvg_gallery over the scorer with removals differs from the survivors' scorer's"
        r["tvg_gallery_two_texts_ms"] = {"removed": 1e3 * dt1, "from_survivors": 1e3 * dt2, "bit_equal": True}
        # a replacement on the eager index with no spare slot, against the model loaded and the index built again over the new set
        out_j = int(keep[len(keep) // 2])
        t_rep = {}
        t_rep["remove_videos"], _ = timed(lambda: sc1.remove_videos([out_j]))
        t_rep["add_videos"], new = timed(lambda: sc1.add_videos([video[int(gone[0])]], vocab[[int(gone[0])]]))
        t_rep["index_sync_and_fill"], _ = timed(gal1._sync_videos)
        new_key = [k for k in gal1.keys if k[0] == int(new[0])]
        assert new_key and all(k in gal1.slot_of for k in new_key), "the new video's prefix was not filled into the freed slot"
        pairs = np.stack([np.full(4, int(new[0])), q[:4]], axis=1)
        before = gal1.stats.as_dict()
        t_rep["first_query_of_the_new_video"], got = timed(lambda: gal1.vtg_pairs(pairs))
        assert gal1.stats.hits - before["hits"] == len(new_key) and gal1.stats.misses == before["misses"], "the new video was not served from a cached slot"
        after = [j for j in keep if j != out_j] + [int(gone[0])]

        def rebuild():
            """-> (seconds of the model load, seconds of the scorer and the index build, the new video's scores)."""
            torch.cuda.synchronize()
            t_start = time.perf_counter()
            m2 = BlimModel(dims, dtype=a.dtype)
            m2.engine.init_synthetic_weights(0)
            m2.set_tvg_prefix_length(prob.tvg_prefix_length)
            m2.vtg_precise, m2.tvg_precise = model.vtg_precise, model.tvg_precise
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s2 = RU.PairScorer(DDPLike(m2), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [video[j] for j in after], vocab[[int(j) for j in after]], torch.arange(len(after)),
                               dims.num_clips, max_tokens=a.max_tokens)
            s2.set_vtg_mode(m2.vtg_mode())
            g2_ = GalleryIndex(s2).build()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            want = g2_.vtg_pairs(np.stack([np.full(4, len(after) - 1), q[:4]], axis=1))
            g2_.close(); m2.engine.close()
            return t0 - t_start, dt, want
        t_load, t_index, want = rebuild()
        assert np.array_equal(got, want), "the replaced video's scores differ from a rebuilt gallery's"
        r["replacement"] = {"removed": out_j, "added_as": int(new[0]), **{k + "_ms": 1e3 * v for k, v in t_rep.items()},
                            "total_ms": 1e3 * (t_rep["remove_videos"] + t_rep["add_videos"] + t_rep["index_sync_and_fill"]),
                            "rebuild": {"model_load_s": t_load, "scorer_and_index_build_s": t_index, "total_s": t_load + t_index}, "bit_equal": True}
        res["modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        gal1.close(); ref_gal.close()
        del sc1, sc2, fresh
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_shortlist(a, dims, model, prob, vtg, tvg, video, q, tpc):
    """`--shortlist`: whole-gallery queries on the fine-tuned blend, `all` (every video a candidate) against `tvg` (the best K of the TVG ranking), see the module text."""
    e = model.engine
    for o in ("narrow_gemm", "narrow_lo6", "narrow_qkv"):
        e.set_option(o, 1)
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x))
    Q, N = len(q), a.n
    Ks = sorted(set(min(int(K), N) for K in a.shortlist))
    Bs = sorted(set(min(int(B), Q) for B in a.shortlist_batches))
    more = dict(cpn=False, alpha=(0.0, 0.0), c=(0.5, 0.5, 1.0, 0.5), finetuned=True)
    res = {"shortlist": Ks, "batches": Bs, "n": N, "queries": Q, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc, "reps": a.reps,
           "blend": {"c": list(more["c"]), "cpn": False}, "options": {"narrow_gemm": 1, "narrow_lo6": 1, "narrow_qkv": 1}, "runs": {}}
    for mode in a.modes.split(","):
        for tmode in a.tvg_modes.split(","):
            model.vtg_precise = None if mode == "none" else mode
            model.tvg_precise = tmode
            model.clear_cache()
            sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                               torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
            sc.set_vtg_mode(model.vtg_mode()); sc.set_tvg_mode(model.tvg_mode())
            warm = np.stack([np.arange(8), np.full(8, q[0])], axis=1)
            sc.vtg(warm); sc.tvg(warm)
            gal = GalleryIndex(sc)
            t_build, _ = timed(gal.build)
            t_feats, _ = timed(sc.gallery_feats)                         # once per weights version: the TVG rows of all N videos as one tensor
            stage1_s, inner = [0.0], gal._stage1

            def stage1(texts, cpn, alpha):                               # stage 1's share of a leg's wall time (its result is on the host when it returns)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = inner(texts, cpn, alpha)
                stage1_s[0] += time.perf_counter() - t0
                return out
            gal._stage1 = stage1

            def run(K, B):
                reqs = [(int(t), np.arange(N), None, None) if K is None else (int(t), None, None, K) for t in q]
                return [r for lo in range(0, Q, B) for r in gal.search_requests(reqs[lo:lo + B], **more)]
            legs = [(K, B) for K in [None] + Ks for B in Bs]
            name = lambda K, B: f"{'all' if K is None else f'tvg{K}'}_B{B}"
            ref = {leg: run(*leg) for leg in legs}                       # warm-up of every leg's workspaces; the results every repetition is held to
            for K in Ks:                                                 # the shortlisted answers do not depend on the batch: bit-equal
                for B in Bs[1:]:
                    assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(ref[(K, B)], ref[(K, Bs[0])])), f"tvg{K}: B = {B} differs from B = {Bs[0]}"
            ts, s1 = {leg: [] for leg in legs}, {leg: [] for leg in legs}
            for rep in range(a.reps):
                for leg in legs:
                    stage1_s[0] = 0.0
                    dt, got = timed(lambda: run(*leg))
                    ts[leg].append(dt); s1[leg].append(stage1_s[0])
                    print(f"repetition {rep}: {name(*leg)} {dt:.3f} s", file=sys.stderr, flush=True)
                    assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(got, ref[leg])), f"{name(*leg)}: results differ between repetitions"
            # stage 1 taken apart: planning on the host (array expressions and the uploads), then the engine calls alone
            parts = {}
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for B in Bs:
                plan_ms, gpu_ms, calls, tokens = [], [], 0, 0
                for _ in range(a.reps):
                    tp = tg_ = 0.0
                    calls = tokens = 0
                    for lo in range(0, Q, B):
                        texts = np.unique(q[lo:lo + B])
                        dt, plans = timed(lambda: list(sc.iter_tvg_gallery(texts)))
                        tp += dt
                        ev0.record()
                        outs = [sc.run(p) for p in plans]
                        ev1.record()
                        torch.cuda.synchronize()
                        tg_ += ev0.elapsed_time(ev1)
                        calls += len(plans); tokens += sum(p.n_tokens for p in plans)
                        del outs
                    plan_ms.append(1e3 * tp / Q); gpu_ms.append(tg_ / Q)
                parts[B] = {"host_planning_ms_per_query": med(plan_ms), "gpu_ms_per_query": med(gpu_ms), "engine_calls": calls, "tokens": tokens,
                            "chunk": sc.gallery_chunk(), "spread_planning": spread(plan_ms), "spread_gpu": spread(gpu_ms)}
            # how much of the `all` answer a shortlist of K keeps -- on RANDOM weights: it says nothing about a trained checkpoint
            stage = inner(q, False, (0.0, 0.0))
            rank = np.argsort(-stage, axis=1, kind="stable")
            top = [o for o, _ in ref[(None, Bs[0])]]
            cover = {}
            for K in sorted(set(min(int(K), N) for K in a.recall_k)):
                kept = [set(rank[i, :K].tolist()) for i in range(Q)]
                cover[f"K{K}"] = {"all_top1_inside": float(np.mean([int(top[i][0]) in kept[i] for i in range(Q)])),
                                  "all_top10_inside": float(np.mean([set(top[i][:10].tolist()) <= kept[i] for i in range(Q)]))}
            r = {"build_s": t_build, "gallery_feats_s": t_feats, "legs": {}, "stage1": {f"B{B}": v for B, v in parts.items()}, "cover_random_weights": cover}
            for leg in legs:
                K, B = leg
                base = med(ts[(None, B)])
                r["legs"][name(*leg)] = {"s": ts[leg], "ms_per_query": 1e3 * med(ts[leg]) / Q, "spread": spread(ts[leg]), "stage1_ms_per_query": 1e3 * med(s1[leg]) / Q,
                                         "stage2_ms_per_query": 1e3 * med([t - s for t, s in zip(ts[leg], s1[leg])]) / Q, "ratio_to_all": base / med(ts[leg]),
                                         "vtg_pairs_per_query": N if K is None else K}
            res["runs"][f"vtg_{mode}/tvg_{tmode}"] = r
            print(json.dumps({f"vtg_{mode}/tvg_{tmode}": r}), flush=True)
            gal.close()
            del sc
            torch.cuda.empty_cache()
    for o in ("narrow_gemm", "narrow_lo6", "narrow_qkv"):
        e.set_option(o, 0)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def rank_kernel_alone(shapes, k, reps=20):
    """blim_tvg_rank alone (HIP events) against the [rows, N] copy to the host plus np.argsort(kind="stable") of every row, on Gaussian logits."""
    from blim_amd import engine as eng
    out = {}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rows, N in shapes:
        kk = min(k, N)
        lg = torch.randn((rows, N), dtype=torch.float32, device="cuda")
        idx, val = torch.empty((rows, kk), dtype=torch.int32, device="cuda"), torch.empty((rows, kk), dtype=torch.float32, device="cuda")
        lp = torch.empty((rows, N), dtype=torch.float32, device="cuda")
        for _ in range(3):
            eng.tvg_rank(lg, N, kk, idx, val)
        ms = {"select": [], "select_and_lp": []}
        for name, more in (("select", {}), ("select_and_lp", {"logprob_out": lp})):
            for _ in range(reps):
                ev0.record(); eng.tvg_rank(lg, N, kk, idx, val, **more); ev1.record()
                torch.cuda.synchronize()
                ms[name].append(ev0.elapsed_time(ev1))
        host = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = torch.log_softmax(lg, dim=1).cpu().numpy()
            order = np.stack([np.argsort(-r, kind="stable")[:kk] for r in h])
            host.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(order[:, 0], idx.cpu().numpy()[:, 0])
        out[f"rows{rows}_N{N}"] = {"k": kk, "kernel_ms": float(np.median(ms["select"])), "kernel_with_logprob_out_ms": float(np.median(ms["select_and_lp"])),
                                   "copy_back_and_argsort_ms": float(np.median(host))}
    return out


def main_prefilter(a, dims, model, prob, vtg, tvg, video, q, tpc):
    """`--shortlist K --prefilter K0 ...`: the parent's shortlist against the cascade, see the module text."""
    from blim_amd import engine as eng
    e = model.engine
    for o in ("narrow_gemm", "narrow_lo6", "narrow_qkv"):
        e.set_option(o, 1)
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x))
    Q, N = len(q), a.n
    K = min(int(a.shortlist[0]), N)
    K0s = sorted(set(min(int(k0), N) for k0 in a.prefilter))
    Bs = sorted(set(min(int(B), Q) for B in a.shortlist_batches))
    more = dict(cpn=False, alpha=(0.0, 0.0), c=(0.5, 0.5, 1.0, 0.5), finetuned=True)
    res = {"shortlist": K, "prefilter": K0s, "batches": Bs, "n": N, "queries": Q, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc,
           "reps": a.reps, "blend": {"c": list(more["c"]), "cpn": False}, "options": {"narrow_gemm": 1, "narrow_lo6": 1, "narrow_qkv": 1}, "gallery_gb": a.gallery_gb, "runs": {}}
    for mode in a.modes.split(","):
        for tmode in a.tvg_modes.split(","):
            model.vtg_precise = None if mode == "none" else mode
            model.tvg_precise = tmode
            model.clear_cache()
            sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                               torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
            sc.set_vtg_mode(model.vtg_mode()); sc.set_tvg_mode(model.tvg_mode())
            warm = np.stack([np.arange(8), np.full(8, q[0])], axis=1)
            sc.vtg(warm); sc.tvg(warm)
            gal = GalleryIndex(sc, budget_bytes=None if a.gallery_gb is None else int(a.gallery_gb * 2**30))
            t_build, _ = timed(gal.build)
            sc.gallery_feats()
            clock = {"s0": 0.0, "s1": 0.0}

            def wrap(obj, name, key):
                inner = getattr(obj, name)

                def f(*args, **kw):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = inner(*args, **kw)
                    clock[key] += time.perf_counter() - t0
                    return out
                setattr(obj, name, f)
            wrap(gal, "_stage0", "s0"); wrap(gal, "_stage1", "s1"); wrap(sc, "tvg", "s1")

            def run(K0, B):
                reqs = [(int(t), None, None, K) + (() if K0 is None else (K0,)) for t in q]
                return [r for lo in range(0, Q, B) for r in gal.search_requests(reqs[lo:lo + B], **more)]
            legs = [(K0, B) for K0 in [None] + K0s for B in Bs]
            name = lambda K0, B: f"{'parent' if K0 is None else f'pre{K0}'}_tvg{K}_B{B}"
            ref = {leg: run(*leg) for leg in legs}
            ts, s0, s1 = ({leg: [] for leg in legs} for _ in range(3))
            for rep_ in range(a.reps):
                for leg in legs:
                    clock["s0"] = clock["s1"] = 0.0
                    dt, got = timed(lambda: run(*leg))
                    ts[leg].append(dt); s0[leg].append(clock["s0"]); s1[leg].append(clock["s1"])
                    print(f"repetition {rep_}: {name(*leg)} {dt:.3f} s", file=sys.stderr, flush=True)
                    assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(got, ref[leg])), f"{name(*leg)}: results differ between repetitions"
            # stage 0 taken apart: planning on the host, the engine call, the rank kernel alone on logits of the call's shape
            parts = {}
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for B in Bs:
                for K0 in K0s:
                    plan_ms, gpu_ms, rank_ms = [], [], []
                    for _ in range(a.reps):
                        tp = tg_ = tr = 0.0
                        for lo in range(0, Q, B):
                            texts = q[lo:lo + B]
                            dt, plans = timed(lambda: list(sc.iter_tvg_first(texts)))
                            tp += dt
                            ev0.record()
                            outs = [sc.run(p, k=K0) for p in plans]
                            ev1.record()
                            torch.cuda.synchronize()
                            tg_ += ev0.elapsed_time(ev1)
                            rows = sum(p.n_pairs for p in plans)
                            lg = torch.randn((rows, N), dtype=torch.float32, device="cuda")
                            ev0.record(); eng.tvg_rank(lg, N, K0, outs[0][0].new_empty((rows, K0)), outs[0][1].new_empty((rows, K0))); ev1.record()
                            torch.cuda.synchronize()
                            tr += ev0.elapsed_time(ev1)
                        plan_ms.append(1e3 * tp / Q); gpu_ms.append(tg_ / Q); rank_ms.append(tr / Q)
                    parts[f"pre{K0}_B{B}"] = {"host_planning_ms_per_query": med(plan_ms), "engine_call_ms_per_query": med(gpu_ms), "rank_kernel_ms_per_query": med(rank_ms)}
            # how much of the parent shortlist a prefilter of K0 keeps -- on RANDOM weights: it says nothing about a trained checkpoint
            cover = {}
            parent = [set(o.tolist()) for o, _ in ref[(None, Bs[0])]]
            for K0 in K0s:
                kept = gal.prefilter(q, K0)
                cover[f"K0_{K0}"] = {"parent_topK_inside": float(np.mean([len(parent[i] & set(kept[i].tolist())) / len(parent[i]) for i in range(Q)]))}
            r = {"build_s": t_build, "legs": {}, "stage0": parts, "cover_random_weights": cover}
            for leg in legs:
                K0, B = leg
                base = med(ts[(None, B)])
                r["legs"][name(*leg)] = {"s": ts[leg], "ms_per_query": 1e3 * med(ts[leg]) / Q, "spread": spread(ts[leg]), "stage0_ms_per_query": 1e3 * med(s0[leg]) / Q,
                                         "stage1_ms_per_query": 1e3 * med(s1[leg]) / Q,
                                         "stage2_ms_per_query": 1e3 * med([t - x - y for t, x, y in zip(ts[leg], s0[leg], s1[leg])]) / Q, "ratio_to_parent": base / med(ts[leg])}
            res["runs"][f"vtg_{mode}/tvg_{tmode}"] = r
            print(json.dumps({f"vtg_{mode}/tvg_{tmode}": r}), flush=True)
            gal.close()
            del sc
            torch.cuda.empty_cache()
    if a.rank_kernel:
        res["rank_kernel"] = rank_kernel_alone([(1, 1000), (8, 1000), (1, 100000), (8, 100000)], 128)
        print(json.dumps({"rank_kernel": res["rank_kernel"]}), flush=True)
    for o in ("narrow_gemm", "narrow_lo6", "narrow_qkv"):
        e.set_option(o, 0)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_lazy(a, dims, model, prob, vtg, tvg, video, q, tpc):
    cand = np.argsort(-prob.t2v_sims[q], axis=1, kind="stable")[:, :a.k]
    pairs = np.stack([cand.reshape(-1), np.repeat(q, a.k)], axis=1)
    P = len(pairs)
    med = lambda t: float(np.median(t))
    res = {"fill": "lazy", "n": a.n, "queries": a.queries, "k": a.k, "reps": a.reps, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc,
           "pairs": P, "distinct_videos": int(len(np.unique(pairs[:, 0]))), "modes": {}}
    for mode in a.modes.split(","):
        model.vtg_precise = None if mode == "none" else mode
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode())
        ref = sc.vtg(pairs)                                               # warm-up: every feature projected, workspaces sized
        first = pairs[:a.k]
        # (a) time to first result, a fresh index each time
        ttfr = {"eager": [], "lazy": [], "eager_build_s": [], "lazy_build_s": []}
        for _ in range(a.reps):
            for fill in ("eager", "lazy"):
                g = GalleryIndex(sc, fill=fill)
                dt, got = timed(lambda: (g.build(), g.vtg_pairs(first))[1])
                assert np.array_equal(got, ref[:a.k]), f"{fill}: first query differs from PairScorer.vtg"
                ttfr[fill].append(dt); ttfr[fill + "_build_s"].append(g.build_seconds)
                g.close()
        # (b) a pass of all misses with admission against PairScorer.vtg; (c) the all-hit pass against an eager index
        eager = GalleryIndex(sc).build()
        lazy = GalleryIndex(sc, fill="lazy").build()
        t_unc, t_miss, t_hit, t_eager, host_miss, host_unc = [], [], [], [], [], []
        for _ in range(a.reps):
            lazy._drop()
            dt, want = timed(lambda: sc.vtg(pairs)); t_unc.append(dt)
            dt, got = timed(lambda: lazy.vtg_pairs(pairs)); t_miss.append(dt)
            assert np.array_equal(got, want), "a pass of misses differs from PairScorer.vtg"
            dt, got = timed(lambda: eager.vtg_pairs(pairs)); t_eager.append(dt)
            assert np.array_equal(got, want)
            dt, got = timed(lambda: lazy.vtg_pairs(pairs)); t_hit.append(dt)
            assert np.array_equal(got, want), "a pass of hits differs from PairScorer.vtg"
            # the host's time in the engine calls alone (plans made beforehand, the device idle at the start): a call that waited for the device would show here
            lazy._drop()
            plans = list(lazy.iter_plans(pairs)); torch.cuda.synchronize()
            t0 = time.perf_counter(); outs = [lazy.run(p) for p in plans]; host_miss.append(time.perf_counter() - t0); torch.cuda.synchronize()
            plans = list(sc.iter_vtg(pairs)); torch.cuda.synchronize()
            t0 = time.perf_counter(); outs = [sc.run(p) for p in plans]; host_unc.append(time.perf_counter() - t0); torch.cuda.synchronize()
        tok = {"uncached": sum(p.n_tokens for p in sc.iter_vtg(pairs)), "hit": sum(p.n_tokens for p in lazy.iter_plans(pairs)),
               "eager": sum(p.n_tokens for p in eager.iter_plans(pairs))}
        lazy.close()
        # (d) a query stream, one pass per query, under a quarter of the gallery
        per = eager.per_slot_bytes()
        eager.close()
        budget = (a.n // 4) * per
        rng = np.random.RandomState(0)
        w = 1.0 / np.arange(1, a.queries + 1); w /= w.sum()
        streams = {"each_query_once": np.arange(a.queries), "the_same_again": np.arange(a.queries), "zipf": rng.choice(a.queries, size=a.stream_draws, p=w)}
        stream = {name: {"eager_s": [], "lazy_s": []} for name in streams}
        for _ in range(a.reps):
            idx = {"eager": GalleryIndex(sc, budget_bytes=budget).build(), "lazy": GalleryIndex(sc, budget_bytes=budget, fill="lazy").build()}
            for name, order in streams.items():
                for fill, g in idx.items():
                    g.stats.reset()
                    def run_stream():
                        return [g.vtg_scores([q[i]], cand[i][None]) for i in order]
                    dt, outs = timed(run_stream)
                    for i, o in zip(order, outs):
                        assert np.array_equal(o[0], ref[i * a.k:(i + 1) * a.k]), f"{fill} stream differs from PairScorer.vtg"
                    st = g.stats.as_dict()
                    stream[name][fill + "_s"].append(dt)
                    stream[name][fill] = dict(st, hit_rate=st["hits"] / max(st["hits"] + st["misses"], 1))
            for g in idx.values():
                g.close()
        for name, order in streams.items():
            for fill in ("eager", "lazy"):
                stream[name][fill + "_pairs_per_s"] = len(order) * a.k / med(stream[name][fill + "_s"])
        r = {"time_to_first_result": dict(ttfr, eager_median_s=med(ttfr["eager"]), lazy_median_s=med(ttfr["lazy"])),
             "miss_pass": {"uncached_s": t_unc, "lazy_all_misses_s": t_miss, "overhead": med(t_miss) / med(t_unc) - 1.0,
                           "host_in_calls_lazy_s": host_miss, "host_in_calls_uncached_s": host_unc,
                           "uncached_pairs_per_s": P / med(t_unc), "lazy_pairs_per_s": P / med(t_miss)},
             "steady_state": {"eager_s": t_eager, "lazy_all_hits_s": t_hit, "eager_pairs_per_s": P / med(t_eager), "lazy_pairs_per_s": P / med(t_hit), "tokens": tok},
             "stream": dict(stream, slots=a.n // 4, bytes_per_slot=per), "bit_equal": True}
        res["modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        del sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_host(a, dims, model, prob, vtg, tvg, video, q, tpc):
    cand = np.argsort(-prob.t2v_sims[q], axis=1, kind="stable")[:, :a.k]
    pairs = np.stack([cand.reshape(-1), np.repeat(q, a.k)], axis=1)
    med = lambda t: float(np.median(t))
    host_bytes = int(a.host_gb * 2**30)
    res = {"host_gb": a.host_gb, "n": a.n, "queries": a.queries, "k": a.k, "reps": a.reps, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc,
           "pairs": len(pairs), "distinct_videos": int(len(np.unique(pairs[:, 0]))), "modes": {}}
    for mode in a.modes.split(","):
        model.vtg_precise = None if mode == "none" else mode
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode())
        ref = sc.vtg(pairs)                                               # warm-up: every feature projected, workspaces sized
        per = GalleryIndex(sc, fill="lazy").per_slot_bytes()
        budget = (a.n // 4) * per
        # (a) the transfers alone: the first query's k slots, admitted by its own call, out and back in
        g = GalleryIndex(sc, budget_bytes=budget, fill="lazy", host_budget_bytes=host_bytes).build()
        assert np.array_equal(g.vtg_pairs(pairs[:a.k]), ref[:a.k])
        keys = list(g.slot_of)[:g.host.stage_records]
        ln = g.cache.slot_len(g.slot_of[keys[0]])
        nb = g.cache.record_bytes(ln)
        moves = [(g.slot_of[k], ln, n * g.host.record_bytes) for n, k in enumerate(keys)]
        items_out = [(k, g.slot_of[k], n, None, (0, n)) for n, k in enumerate(keys)]
        items_in = [(k, g.slot_of[k], (0, n)) for n, k in enumerate(keys)]
        tr = {"pack_s": [], "spill_s": [], "unpack_s": [], "restore_s": []}
        for _ in range(a.reps + 1):                                       # (the first round warms the copies up and is dropped)
            dt, tickets = timed(lambda: g.cache.export_slots(moves, g.host.staging)); tr["pack_s"].append(dt)
            dt, _ = timed(lambda: g.cache.import_slots(moves, g.host.staging, tickets)); tr["unpack_s"].append(dt)
            dt, _ = timed(lambda: g.host.spill(g.cache, items_out)); tr["spill_s"].append(dt)
            dt, _ = timed(lambda: g.host.restore(g.cache, items_in)); tr["restore_s"].append(dt)
        assert np.array_equal(g.vtg_pairs(pairs[:a.k]), ref[:a.k]), "scores differ after the slots went out and came back"
        transfers = {"records": len(keys), "record_bytes": nb, "slot_positions": ln}
        for name, t in tr.items():
            m = med(t[1:])
            transfers[name] = t[1:]
            transfers[name[:-2] + "_ms_per_record"] = 1e3 * m / len(keys)
            transfers[name[:-2] + "_GB_per_s"] = len(keys) * nb / m / 1e9
        n_records, pinned = g.host.n_records, g.host.n_records * g.host.record_bytes
        g.close()
        # (b) the query streams under a quarter of the gallery: lazy without a tier against lazy with it
        rng = np.random.RandomState(0)
        w = 1.0 / np.arange(1, a.queries + 1); w /= w.sum()
        streams = {"each_query_once": np.arange(a.queries), "the_same_again": np.arange(a.queries), "zipf": rng.choice(a.queries, size=a.stream_draws, p=w)}
        stream = {name: {"lazy_s": [], "tier_s": []} for name in streams}
        for _ in range(a.reps):
            idx = {"lazy": GalleryIndex(sc, budget_bytes=budget, fill="lazy").build(),
                   "tier": GalleryIndex(sc, budget_bytes=budget, fill="lazy", host_budget_bytes=host_bytes).build()}
            for name, order in streams.items():
                for form, g in idx.items():
                    g.stats.reset()
                    h0 = g.host.stats.as_dict() if g.host is not None else None
                    def run_stream():
                        return [g.vtg_scores([q[i]], cand[i][None]) for i in order]
                    dt, outs = timed(run_stream)
                    for i, o in zip(order, outs):
                        assert np.array_equal(o[0], ref[i * a.k:(i + 1) * a.k]), f"{form} stream differs from PairScorer.vtg"
                    st = g.stats.as_dict()
                    stream[name][form + "_s"].append(dt)
                    stream[name][form] = dict(st, hit_rate=st["hits"] / max(st["hits"] + st["misses"], 1))
                    if h0 is not None:
                        stream[name]["host"] = {k: v - h0[k] for k, v in g.host.stats.as_dict().items()}
            for g in idx.values():
                g.close()
        for name, order in streams.items():
            for form in ("lazy", "tier"):
                stream[name][form + "_pairs_per_s"] = len(order) * a.k / med(stream[name][form + "_s"])
                stream[name][form + "_ms_per_query"] = 1e3 * med(stream[name][form + "_s"]) / len(order)
        r = {"transfers": transfers, "stream": dict(stream, slots=a.n // 4, bytes_per_slot=per, host_records=n_records, pinned_bytes=pinned), "bit_equal": True}
        res["modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        del sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


def main_v2t(a, dims, model, prob, vtg, tvg, video, q, tpc):
    cand = np.argsort(-prob.v2t_sims[q], axis=1, kind="stable")[:, :a.k]
    fs = np.take_along_axis(prob.v2t_sims[q].astype(np.float32), cand, 1)
    pairs = np.stack([np.repeat(q, a.k), cand.reshape(-1)], axis=1)
    P = len(pairs)
    close = lambda got, want: bool(np.all(np.abs(got - want) <= 1e-5 * np.maximum(1.0, np.abs(want))))
    alpha, c = (0.8, 0.3), (0.5, 0.5, 0.5, 0.5)
    res = {"direction": "v2t", "n": a.n, "queries": a.queries, "k": a.k, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc,
           "pairs": P, "distinct_texts": int(len(np.unique(pairs[:, 1]))), "vtg_mode": "none", "tvg_modes": {}}
    model.vtg_precise = None
    for mode in a.tvg_modes.split(","):
        model.tvg_precise = mode
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode()); sc.set_tvg_mode(model.tvg_mode())
        sc.tvg(pairs[:8]); sc.vtg(pairs[:8])                              # warm-up: features projected, workspaces sized
        gal = GalleryIndex(sc)
        t_vbuild, _ = timed(gal.build)
        tg = TextGalleryIndex(sc, video_index=gal)
        t_build, _ = timed(tg.build)
        tg.tvg_pairs(pairs[:8])
        tok_unc = sum(p.n_tokens for p in sc.iter_tvg(pairs))
        tok_cac = sum(p.n_tokens for p in tg.iter_plans(pairs))
        # 1. the TVG leg alone
        t_unc, t_cac, dmax, biteq = [], [], 0.0, True
        for _ in range(a.reps):
            dt, ref = timed(lambda: sc.tvg(pairs)); t_unc.append(dt)
            dt, got = timed(lambda: tg.tvg_pairs(pairs)); t_cac.append(dt)
            assert close(got, ref), "cached TVG scores differ from PairScorer.tvg by more than 1e-5"
            dmax = max(dmax, float(np.max(np.abs(got - ref)))); biteq = biteq and bool(np.array_equal(got, ref))
        # 2. the whole fine-tuned blend
        def uncached_blend():
            cl, ql, pr = sc.vtg(pairs), sc.tvg(pairs), sc.vtg(pairs, cpn=True)
            return 0.5 * (0.5 * ql + 0.5 * (cl - alpha[1] * pr)).reshape(cand.shape) + 0.5 * fs
        rr = lambda: tg.rerank(q, cand, first_stage=fs, cpn=True, alpha=alpha, c=c, finetuned=True)
        t_cold, _ = timed(rr)                                             # the prior memo is empty on this call
        b_unc, b_cac = [], []
        for _ in range(a.reps):
            dt, want = timed(uncached_blend); b_unc.append(dt)
            dt, (order, blended) = timed(rr); b_cac.append(dt)
            assert close(blended, -np.sort(-want, axis=1)), "cached blend differs from the uncached one by more than 1e-5"
        # 3. single-query latency: one video per text, bit-equal
        lat = {}
        for kk in (16, a.n):
            c1 = np.argsort(-prob.v2t_sims[q[0]], kind="stable")[:kk]
            p1 = np.stack([np.full(kk, q[0]), c1], axis=1)
            f1 = prob.v2t_sims[q[0]].astype(np.float32)[c1][None]
            assert np.array_equal(tg.tvg_pairs(p1), sc.tvg(p1)), "single-query cached TVG scores are not bit-equal"
            r1 = lambda: tg.rerank([q[0]], c1[None], first_stage=f1, cpn=True, alpha=alpha, c=c, finetuned=True)
            r1()
            med = lambda fn: 1e3 * float(np.median([timed(fn)[0] for _ in range(3)]))
            lat[f"k{kk}"] = {"tvg_cached_ms": med(lambda: tg.tvg_pairs(p1)), "tvg_uncached_ms": med(lambda: sc.tvg(p1)), "blend_cached_ms": med(r1),
                             "blend_uncached_ms": med(lambda: (sc.vtg(p1), sc.tvg(p1), sc.vtg(p1, cpn=True))),
                             "tokens_cached": sum(p.n_tokens for p in tg.iter_plans(p1)), "tokens_uncached": sum(p.n_tokens for p in sc.iter_tvg(p1))}
        # where the time goes: the engine's timing classes of one pass each
        cls = {}
        for name, fn in (("cached", lambda: tg.tvg_pairs(pairs)), ("uncached", lambda: sc.tvg(pairs))):
            model.engine.timing_enable(True)
            model.engine.timing_report()
            wall, _ = timed(fn)
            rep = model.engine.timing_report()
            model.engine.timing_enable(False)
            cls[name] = {"wall_ms": 1e3 * wall, "classes_ms": {k: round(v["ms"], 3) for k, v in rep.items() if v["calls"]}, "launches": int(sum(v["calls"] for v in rep.values()))}
        spread = lambda t: float((max(t) - min(t)) / np.median(t))
        r = {"build_s": t_build, "video_build_s": t_vbuild, "slots": len(tg.slot_of), "slot_positions": tg.slot_positions(), "bytes_per_slot": tg.cache.bytes // len(tg.slot_of),
             "tokens_uncached": tok_unc, "tokens_cached": tok_cac, "uncached_s": t_unc, "cached_s": t_cac, "uncached_pairs_per_s": P / float(np.median(t_unc)),
             "cached_pairs_per_s": P / float(np.median(t_cac)), "speedup": float(np.median(t_unc) / np.median(t_cac)), "spread_uncached": spread(t_unc),
             "spread_cached": spread(t_cac), "max_abs_diff": dmax, "bit_equal_every_rep": biteq, "within_1e-5_every_rep": True,
             "blend": {"uncached_s": b_unc, "cached_s": b_cac, "cached_cold_prior_s": t_cold, "speedup": float(np.median(b_unc) / np.median(b_cac)),
                       "uncached_pairs_per_s": P / float(np.median(b_unc)), "cached_pairs_per_s": P / float(np.median(b_cac))},
             "latency": lat, "timing": cls}
        res["tvg_modes"][mode] = r
        print(json.dumps({mode: r}), flush=True)
        tg.close(); gal.close()
        del sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


if __name__ == "__main__":
    main()
