"""The caption prefilter measured: v2t `--candidates tvg` with and without `--caption_prefilter K0`, on the same indexes in one process.

Per TVG mode (`--tvg_modes`): the parent's whole-caption shortlist -- TextGalleryIndex.rerank_shortlist(video, K), one tvg_pairs pass over all N captions per query
video -- against the same call with prefilter = K0 for each `--prefilter K0`, one query video per call as the command runs them (`per_query`), and all query
videos in one call, which shares one stage-0 pass (`batched`).  `--reps` alternating repetitions of every leg, medians, the spread, the time inside
TextGalleryIndex.prefilter (stage 0) and the rest; each repetition's answers are compared with the first run's.  Then the parts of stage 0 alone by HIP events: the
engine entry (PrefixCache.tvg_first_cols) for 1 and Q columns over every slot, tvg_cols over [N, N] logits, rank_rows over [Q, N] values.  How much of the parent's
K a K0 keeps is reported on RANDOM weights: it says nothing about a trained checkpoint.

    python tools/caption_prefilter_bench.py --n 1000 --queries 55 --shortlist 16 --prefilter 64 128 256 --synthetic_7b --tvg_modes attn --out profiles/r27_caption_prefilter.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blim_amd import engine as eng  # noqa: E402
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


def events_ms(fn, reps=20, warm=3):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        ev0.record(); fn(); ev1.record()
        torch.cuda.synchronize()
        out.append(ev0.elapsed_time(ev1))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=55)
    ap.add_argument("--shortlist", type=int, default=16, metavar="K")
    ap.add_argument("--prefilter", type=int, nargs="+", default=[64, 128, 256], metavar="K0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--synthetic_7b", action="store_true")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--tvg_modes", default="attn")
    ap.add_argument("--max_tokens", type=int, default=24576)
    ap.add_argument("--no_video_index", action="store_true", help="the VTG leg of the rerank from PairScorer.vtg instead of cached video slots (a large N: no video cache is built)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = synth.ModelDims() if a.synthetic_7b else synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                                                                     num_kv_heads=1, mm_hidden_size=64)
    tpc = 64 if a.synthetic_7b else 8
    model = BlimModel(dims, dtype=a.dtype)
    e = model.engine
    e.init_synthetic_weights(0)
    prob = synth.make_problem(1, a.n, dims, tok_per_clip=tpc, fast_video=a.n > 256)
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    tok = type("T", (), {"pad_token_id": synth.PAD_ID})()
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    video = [torch.from_numpy(v) for v in prob.video]
    q = np.linspace(0, a.n - 1, a.queries).round().astype(np.int64)
    for o in ("narrow_gemm", "narrow_lo6", "narrow_qkv"):
        e.set_option(o, 1)
    med = lambda x: float(np.median(x))
    spread = lambda x: float((max(x) - min(x)) / np.median(x))
    Q, N = len(q), a.n
    K = min(a.shortlist, N)
    K0s = sorted(set(min(int(k0), N) for k0 in a.prefilter))
    more = dict(cpn=False, alpha=(0.0, 0.0), c=(0.5, 0.5, 1.0, 0.5))
    res = {"direction": "v2t", "shortlist": K, "prefilter": K0s, "n": N, "queries": Q, "dtype": a.dtype, "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc,
           "reps": a.reps, "blend": {"c": list(more["c"]), "cpn": False}, "options": {"narrow_gemm": 1, "narrow_lo6": 1, "narrow_qkv": 1},
           "video_index": not a.no_video_index, "runs": {}}
    for tmode in a.tvg_modes.split(","):
        model.vtg_precise, model.tvg_precise = None, tmode
        model.clear_cache()
        sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab),
                           torch.from_numpy(prob.tvg_video_labels), dims.num_clips, max_tokens=a.max_tokens)
        sc.set_vtg_mode(model.vtg_mode()); sc.set_tvg_mode(model.tvg_mode())
        warm = np.stack([np.full(8, q[0]), np.arange(8)], axis=1)
        sc.vtg(warm); sc.tvg(warm)
        gal = None if a.no_video_index else GalleryIndex(sc)
        t_gal = 0.0 if gal is None else timed(gal.build)[0]
        tg = TextGalleryIndex(sc, video_index=gal)
        t_build, _ = timed(tg.build)
        clock = {"s0": 0.0}
        inner = tg.prefilter

        def stage0(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(*args, **kw)
            torch.cuda.synchronize()
            clock["s0"] += time.perf_counter() - t0
            return out
        tg.prefilter = stage0

        def run(K0, batched):
            kw = {} if K0 is None else {"prefilter": K0}
            if batched:
                o, b = tg.rerank_shortlist(q, K, **more, **kw)
                return list(zip(o, b))
            return [tuple(x[0] for x in tg.rerank_shortlist([v], K, **more, **kw)) for v in q]
        legs = [(K0, batched) for batched in (False, True) for K0 in [None] + K0s]
        name = lambda K0, batched: f"{'parent' if K0 is None else f'pre{K0}'}_tvg{K}_{'batched' if batched else 'per_query'}"
        ref = {leg: run(*leg) for leg in legs}                                     # (also the warm-up of every leg)
        ts, s0 = ({leg: [] for leg in legs} for _ in range(2))
        for rep_ in range(a.reps):
            for leg in legs:
                clock["s0"] = 0.0
                dt, got = timed(lambda: run(*leg))
                ts[leg].append(dt); s0[leg].append(clock["s0"])
                print(f"repetition {rep_}: {name(*leg)} {dt:.3f} s", file=sys.stderr, flush=True)
                assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(got, ref[leg])), f"{name(*leg)}: results differ between repetitions"
        # the parts of stage 0 alone, by HIP events
        slots = [tg.slot_of[k] for k in tg.keys]
        parts = {"slots": len(slots)}
        for n_cols in (1, Q):
            cols = torch.from_numpy(np.asarray(sc.tvg_video_labels, np.int32)[q[:n_cols]]).cuda()
            parts[f"engine_entry_cols{n_cols}_ms"] = events_ms(lambda: sc.tvg_first_cached(tg.cache, slots, cols))
            lg = torch.randn((len(slots), N), dtype=torch.float32, device="cuda")
            out = torch.empty((n_cols, len(slots)), dtype=torch.float32, device="cuda")
            parts[f"tvg_cols_rows{len(slots)}_cols{n_cols}_ms"] = events_ms(lambda: eng.tvg_cols(lg, N, cols, out))
        vals = torch.randn((Q, N), dtype=torch.float32, device="cuda")
        for K0 in K0s:
            idx, val = torch.empty((Q, K0), dtype=torch.int32, device="cuda"), torch.empty((Q, K0), dtype=torch.float32, device="cuda")
            parts[f"rank_rows_rows{Q}_n{N}_k{K0}_ms"] = events_ms(lambda: eng.rank_rows(vals, N, K0, idx, val))
            parts[f"rank_rows_rows1_n{N}_k{K0}_ms"] = events_ms(lambda: eng.rank_rows(vals, N, K0, idx, val, n_rows=1))
        # how much of the parent's K a prefilter of K0 keeps -- on RANDOM weights: it says nothing about a trained checkpoint
        cover = {}
        parent = [set(o.tolist()) for o, _ in ref[(None, False)]]
        for K0 in K0s:
            kept, _ = inner(q, K0)
            cover[f"K0_{K0}"] = {"parent_topK_inside": float(np.mean([len(parent[i] & set(kept[i].tolist())) / len(parent[i]) for i in range(Q)]))}
        r = {"video_index_build_s": t_gal, "caption_cache_build_s": t_build, "caption_slots": len(tg.slot_of), "legs": {}, "stage0_parts": parts, "cover_random_weights": cover,
             "prefilter_stats": dict(tg.prefilter_stats)}
        for leg in legs:
            K0, batched = leg
            base = med(ts[(None, batched)])
            r["legs"][name(*leg)] = {"s": ts[leg], "ms_per_query": 1e3 * med(ts[leg]) / Q, "spread": spread(ts[leg]), "stage0_ms_per_query": 1e3 * med(s0[leg]) / Q,
                                     "rest_ms_per_query": 1e3 * med([t - x for t, x in zip(ts[leg], s0[leg])]) / Q, "ratio_to_parent": base / med(ts[leg])}
        res["runs"][f"tvg_{tmode}"] = r
        print(json.dumps({f"tvg_{tmode}": r}), flush=True)
        tg.close()
        if gal is not None:
            gal.close()
        del sc
        torch.cuda.empty_cache()
    for o in ("narrow_gemm", "narrow_lo6", "narrow_qkv"):
        e.set_option(o, 0)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    e.close()


if __name__ == "__main__":
    main()
