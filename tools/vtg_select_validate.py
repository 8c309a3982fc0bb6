"""Does `--vtg_precise select` hold the 1e-3 bar over a WHOLE evaluation, and what does it save?  Runs one six-pass evaluation (N videos x N texts, top-16, real 7B
configuration) twice -- VTG calls fully compensated, then with the per-layer mask calibrate_vtg_select measures on the evaluation's own pairs -- and compares every
computed entry of all six matrices (the TVG calls run fully compensated in both: their three matrices must be bit-equal).  Then times bench.py's headline-shaped step
(880 pairs: 96 video + 32 text tokens, top-16) plain, fully compensated and under the chosen mask.

    python tools/vtg_select_validate.py [--n 1000] [--weights gaussian|sink7b|heavy7b] [--dtype f16]
"""
import argparse, json, os, sys, time, types
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from blim_amd import retrieval_utils as RU, synth
from blim_amd.modeling import BlimModel, DDPLike

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000)
ap.add_argument("--topk", type=int, default=16)
ap.add_argument("--weights", default="heavy7b", choices=["gaussian", "sink7b", "heavy7b"])
ap.add_argument("--dtype", default="f16")
ap.add_argument("--seed", type=int, default=1, help="seed of the synthetic problem (videos, texts, similarity matrices)")
ap.add_argument("--no_step", action="store_true", help="skip the headline-step timing")
a = ap.parse_args()

dims = synth.ModelDims()
model = BlimModel(dims, max_positions=1024, dtype=a.dtype)
wseed = 0
if a.weights != "gaussian":
    from oracle.gen_golden_heavy import CASES, heavy_items          # (the reshaped tensors of the trained-like fixtures)
    spec = CASES[a.weights]
    wseed = spec["wseed"]
model.engine.init_synthetic_weights(wseed)
if a.weights != "gaussian":
    for name, arr in heavy_items(dims, wseed, only_changed=True, sink=bool(spec.get("sink", False))):
        model.engine.load_weight(name, arr)
prob = synth.make_problem(a.seed, a.n, dims, tok_per_clip=64, fast_video=True)
loader = synth.ProblemLoader(prob, 64, video_dtype=torch.float16)
tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
nz = lambda x: np.where(x == 0, np.float32(1e-6), x)
dev = torch.device("cuda", 0)
out = {}
for mode in ("full", "select"):
    args = types.SimpleNamespace(topk=a.topk, num_clips=dims.num_clips, cpn=True, resume="x", eval=True, dataset="MSRVTT", batch_size_eval=16,
                                 iv2_scores={"v2t": torch.from_numpy(nz(prob.v2t_sims)), "t2v": torch.from_numpy(nz(prob.t2v_sims))}, max_tokens=32768, dedup=True)
    model.clear_cache()
    model.tvg_precise = "full"
    model.vtg_precise = mode
    torch.cuda.synchronize()
    t0 = time.time()
    t2v, v2t = RU.evaluation(DDPLike(model), loader, dev, tok, args)
    torch.cuda.synchronize()
    out[mode] = (t2v, v2t, time.time() - t0, args._eval_stats)
(t2v_f, v2t_f, s_f, _), (t2v_s, v2t_s, s_s, st) = out["full"], out["select"]
table = st.get("vtg_precise_table", {})
rep = {"weights": a.weights, "dtype": a.dtype, "n": a.n, "seed": a.seed, "vtg_chosen": st.get("vtg_precise"), "mask": table.get("mask"), "k": table.get("k"),
       "calibration_seconds": round(float(table.get("seconds", 0.0)), 3), "seconds_full": round(s_f, 2), "seconds_select": round(s_s, 2),
       "units": table.get("units"), "order": table.get("order"), "probes": table.get("probes"), "confirm": table.get("confirm"), "none": table.get("none")}
for name, F, S in (("t2v query_likelihood (VTG)", t2v_f["query_likelihood"], t2v_s["query_likelihood"]),
                   ("v2t candidate_likelihood (VTG)", v2t_f["candidate_likelihood"], v2t_s["candidate_likelihood"]),
                   ("v2t candidate_prior (VTG, CPN)", v2t_f["candidate_prior"], v2t_s["candidate_prior"]),
                   ("t2v candidate_likelihood (TVG)", t2v_f["candidate_likelihood"], t2v_s["candidate_likelihood"]),
                   ("t2v candidate_prior (TVG, CPN)", t2v_f["candidate_prior"], t2v_s["candidate_prior"]),
                   ("v2t query_likelihood (TVG)", v2t_f["query_likelihood"], v2t_s["query_likelihood"])):
    m = F != -100.0
    assert np.array_equal(m, S != -100.0)
    d = np.abs(S[m].astype(np.float64) - F[m]) / np.abs(F[m])
    rep[name] = {"entries": int(m.sum()), "max": float(d.max()), "rms": float(np.sqrt(np.mean(d ** 2))), "over_1e-3": int((d > 1e-3).sum()),
                 "bit_equal": bool(np.array_equal(F, S))}

if not a.no_step and st.get("vtg_precise") == "select":
    import bench
    mask = np.array(table["mask"], dtype=np.uint8)
    step = {}
    for mode in ("none", "full", "select"):
        model.vtg_precise = mode
        if mode == "select":
            model.resolve_vtg("select", mask)
        (sc, pl, _, _), = bench.build_step_plans(model, 0, 1, 55, 16)
        model.engine.reserve(pl.n_tokens, pl.n_rows, compensated=mode != "none")
        sc.run(pl)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(5):
            r = sc.run(pl)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
        step[mode] = {"pairs": pl.n_pairs, "ms_per_step": round(dt * 1e3, 3), "pairs_per_s": round(pl.n_pairs / dt, 1), "finite": bool(torch.isfinite(r).all())}
    rep["headline_step"] = step
    saved = s_f - (s_s - rep["calibration_seconds"])                  # what the evaluation's passes gained by running under the mask
    rep["calibration_over_time_saved"] = round(rep["calibration_seconds"] / saved, 3) if saved > 0 else None
model.engine.close()
print(json.dumps(rep, indent=1))
