"""Gallery index throughput (blim_amd/gallery.py): t2v VTG pairs/s of Q queries x top-k over N synthetic videos, the cached path (GalleryIndex.vtg_scores)
against the uncached PairScorer.vtg on the SAME pairs, alternated `--reps` times each in one process; the build time and bytes per slot; single-query latency
for k = 16 and k = N; in the plain and the fully compensated VTG mode.  Scores of the two paths are checked bit-equal on every repetition.

    python tools/gallery_bench.py --n 1000 --queries 55 --k 16 --synthetic_7b --out profiles/r09_gallery.json"""
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
from blim_amd.gallery import GalleryIndex  # noqa: E402
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


if __name__ == "__main__":
    main()
