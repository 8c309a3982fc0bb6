"""Searching inside a caller's set of videos, measured on tools/gallery_bench.py's --prefilter protocol: one process, 7B rows with synthetic
weights, whole-gallery queries on the fine-tuned blend, K = --shortlist, K0 = --prefilter, the three narrow options on auto, legs alternating, --reps repetitions.

    python tools/within_bench.py --n 1000 --synthetic_7b --out profiles/r28_within.json

Sets of M videos (--sets, and N itself) are drawn once per M from --seed and shared by every query.  Legs, per M and per B (requests per search_requests call):
  explicit_M   the only filtered form there was: a request that names the M videos as its candidates, all M reranked (over --explicit_queries of the queries: the
               leg costs about 0.4 ms per video and query);
  within_M     SearchRequest(t, shortlist=K, prefilter=K0, within=set);
  pre          the plain prefiltered request (t, None, None, K, K0), to set beside within_N.
Then tvg_rank_within_kernel alone beside tvg_rank_kernel (HIP events, Gaussian logits, k = 64), and how many of the unfiltered K0 survivors fall inside a 5 % set."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from blim_amd import engine as eng  # noqa: E402
from blim_amd import retrieval_utils as RU  # noqa: E402
from blim_amd import synth  # noqa: E402
from blim_amd.gallery import GalleryIndex, SearchRequest  # noqa: E402
from blim_amd.modeling import BlimModel, DDPLike  # noqa: E402

med = lambda x: float(np.median(x))
spread = lambda x: float((max(x) - min(x)) / np.median(x))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def kernels_alone(shapes, k=64, reps=20):
    """blim_tvg_rank_within over one list of M columns of one row of N, beside blim_tvg_rank on the same row: HIP events, medians."""
    out = {}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for N, M in shapes:
        lg = torch.randn((1, N), dtype=torch.float32, device="cuda")
        wi = torch.from_numpy(np.sort(np.random.RandomState(M).permutation(N)[:M]).astype(np.int32)).cuda()
        off = torch.tensor([0, M], dtype=torch.int32, device="cuda")
        kk = min(k, N)
        idx, val = torch.empty((1, k), dtype=torch.int32, device="cuda"), torch.empty((1, k), dtype=torch.float32, device="cuda")
        ms = {"within": [], "whole": []}
        for name, call in (("within", lambda: eng.tvg_rank_within(lg, N, k, wi, off, idx, val)), ("whole", lambda: eng.tvg_rank(lg, N, kk, idx, val))):
            for _ in range(3):
                call()
            for _ in range(reps):
                ev0.record(); call(); ev1.record()
                torch.cuda.synchronize()
                ms[name].append(ev0.elapsed_time(ev1))
        out[f"N{N}_M{M}"] = {"k": k, "tvg_rank_within_ms": med(ms["within"]), "tvg_rank_ms": med(ms["whole"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=55)
    ap.add_argument("--explicit_queries", type=int, default=11, help="queries of the explicit-candidates legs (evenly spaced among --queries)")
    ap.add_argument("--shortlist", type=int, default=16)
    ap.add_argument("--prefilter", type=int, default=64)
    ap.add_argument("--sets", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=28)
    ap.add_argument("--synthetic_7b", action="store_true")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--max_tokens", type=int, default=24576)
    ap.add_argument("--kernel_shapes", type=int, nargs="*", default=[1000, 50, 1000, 500, 5000, 50, 5000, 500, 5000, 5000, 100000, 50, 100000, 500, 100000, 5000, 100000, 100000],
                    metavar="N M", help="pairs N M for the kernels alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = synth.ModelDims() if a.synthetic_7b else synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                                                                     num_kv_heads=1, mm_hidden_size=64)
    tpc = 64 if a.synthetic_7b else 8
    model = BlimModel(dims, dtype=a.dtype)
    model.engine.init_synthetic_weights(0)
    prob = synth.make_problem(1, a.n, dims, tok_per_clip=tpc, fast_video=a.n > 256)
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    tok = type("T", (), {"pad_token_id": synth.PAD_ID})()
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    video = [torch.from_numpy(v) for v in prob.video]
    N, Q = a.n, a.queries
    q = np.linspace(0, N - 1, Q).round().astype(np.int64)
    qe = q[np.linspace(0, Q - 1, min(a.explicit_queries, Q)).round().astype(np.int64)]
    for o in ("narrow_gemm", "narrow_lo6", "narrow_qkv"):
        model.engine.set_option(o, 1)
    model.vtg_precise, model.tvg_precise = None, "attn"
    model.clear_cache()
    sc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels),
                       dims.num_clips, max_tokens=a.max_tokens)
    sc.set_vtg_mode(model.vtg_mode()); sc.set_tvg_mode(model.tvg_mode())
    warm = np.stack([np.arange(8), np.full(8, q[0])], axis=1)
    sc.vtg(warm); sc.tvg(warm)
    gal = GalleryIndex(sc)
    t_build, _ = timed(gal.build)
    K, K0 = min(a.shortlist, N), min(a.prefilter, N)
    more = dict(cpn=False, alpha=(0.0, 0.0), c=(0.5, 0.5, 1.0, 0.5), finetuned=True)
    Ms = sorted(set(min(m, N) for m in a.sets) | {N})
    rs = np.random.RandomState(a.seed)
    sets = {M: np.sort(rs.permutation(N)[:M]) for M in Ms}
    Bs = sorted(set(min(B, Q) for B in a.batches))

    def run(kind, M, B):
        if kind == "explicit":
            reqs, qs = [(int(t), sets[M], None) for t in qe], len(qe)
        elif kind == "within":
            reqs, qs = [SearchRequest(int(t), shortlist=K, prefilter=K0, within=sets[M]) for t in q], Q
        else:
            reqs, qs = [(int(t), None, None, K, K0) for t in q], Q
        return [r for lo in range(0, qs, B) for r in gal.search_requests(reqs[lo:lo + B], **more)]
    legs = [(kind, M, B) for B in Bs for kind, M in [("pre", N)] + [(k_, M) for M in Ms for k_ in ("within", "explicit")]]
    name = lambda kind, M, B: f"{kind}{'' if kind == 'pre' else f'_M{M}'}_B{B}"
    ref = {leg: run(*leg) for leg in legs}
    for B in Bs:                                                      # within = every video IS the plain prefiltered request
        assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(ref[("within", N, B)], ref[("pre", N, B)])), "within = all differs from the plain request"
    for M in Ms:
        assert all(set(o.tolist()) <= set(sets[M].tolist()) for o, _ in ref[("within", M, Bs[0])])
    ts = {leg: [] for leg in legs}
    for rep_ in range(a.reps):
        for leg in legs:
            dt, got = timed(lambda: run(*leg))
            ts[leg].append(dt)
            print(f"repetition {rep_}: {name(*leg)} {dt:.3f} s", file=sys.stderr, flush=True)
            assert all(np.array_equal(o, o1) and np.array_equal(b, b1) for (o, b), (o1, b1) in zip(got, ref[leg])), f"{name(*leg)}: results differ between repetitions"
    res = {"n": N, "queries": Q, "explicit_queries": len(qe), "shortlist": K, "prefilter": K0, "sets": Ms, "seed": a.seed, "batches": Bs, "reps": a.reps, "dtype": a.dtype,
           "dims": "7B" if a.synthetic_7b else "tiny", "video_tokens": 4 * tpc, "build_s": t_build, "legs": {}}
    for leg in legs:
        n_q = len(qe) if leg[0] == "explicit" else Q
        res["legs"][name(*leg)] = {"s": ts[leg], "queries": n_q, "ms_per_query": 1e3 * med(ts[leg]) / n_q, "spread": spread(ts[leg])}
    # post-filtering: how many of the unfiltered K0 survivors lie inside a 5 % set (RANDOM weights: a count, not a recall claim)
    five = np.sort(np.random.RandomState(a.seed + 1).permutation(N)[:max(N // 20, 1)])
    kept = gal.prefilter(q, K0)
    inside = [int(np.isin(row, five).sum()) for row in kept]
    res["postfilter_5pct"] = {"set": len(five), "K0": K0, "inside_mean": float(np.mean(inside)), "inside_min": int(min(inside)), "inside_max": int(max(inside)),
                              "queries_with_fewer_than_K": int(sum(x < K for x in inside))}
    res["within_stats"] = dict(gal.within_stats)
    print(json.dumps({k_: v for k_, v in res.items() if k_ != "legs"}), flush=True)
    print(json.dumps({k_: {"ms_per_query": round(v["ms_per_query"], 3), "spread": round(v["spread"], 4)} for k_, v in res["legs"].items()}), flush=True)
    gal.close()
    ks = a.kernel_shapes
    res["kernels"] = kernels_alone(list(zip(ks[0::2], ks[1::2])))
    print(json.dumps({"kernels": res["kernels"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    model.engine.close()


if __name__ == "__main__":
    main()
