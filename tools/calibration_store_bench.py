"""What `--calibration_store` saves: the weights fingerprint's cost, then whole evaluations (N videos x N texts, top-k, real 7B configuration) per weight set -- VTG + TVG
fully compensated (the yardstick), and for each requested mode a COLD run (empty store for these weights: measured, record written) and a WARM run (the record
verified on the evaluation's own sample) -- with calibration and end-to-end seconds, the calibration source, the select mask, and whether the warm run's six score
matrices are bit-equal to the cold run's.  The weight sets share one store directory, so every cold run after the first is also offered the other sets' records
(a miss: another fingerprint).  Cold and warm run in one process, the model's in-process resolution reset in between (what a new process starts from).

    python tools/calibration_store_bench.py [--n 1000] [--weights gaussian,sink7b,heavy7b] [--modes select,auto] [--no_full] [--fingerprint]
"""
import argparse, json, os, shutil, sys, tempfile, time, types
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from blim_amd import retrieval_utils as RU, synth
from blim_amd import engine as E
from blim_amd import training_utils as TU
from blim_amd.modeling import BlimModel, DDPLike

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000)
ap.add_argument("--topk", type=int, default=16)
ap.add_argument("--weights", default="gaussian,sink7b,heavy7b")
ap.add_argument("--modes", default="select,auto")
ap.add_argument("--dtype", default="f16")
ap.add_argument("--seed", type=int, default=1, help="seed of the synthetic problem (videos, texts, similarity matrices)")
ap.add_argument("--no_full", action="store_true", help="skip the fully compensated yardstick runs")
ap.add_argument("--fingerprint", action="store_true", help="time the weights fingerprint of fp16 and bf16 7B engines and the hash of one 4 GiB buffer")
ap.add_argument("--store", default=None, help="store directory (default: a fresh temporary one, removed at the end)")
a = ap.parse_args()

dims = synth.ModelDims()
dev = torch.device("cuda", 0)
rep = {"n": a.n, "topk": a.topk, "dtype": a.dtype, "seed": a.seed}


def fingerprint_bytes(d):
    """Bytes blim_weights_fingerprint reads (csrc/engine.hip: the placed tensors + the visual head's hi | lo | hi rows; no adapters here)."""
    H, I, V, M, L = d.hidden_size, d.intermediate_size, d.vocab_size, d.mm_hidden_size, d.num_layers
    qkv = (d.num_heads + 2 * d.num_kv_heads) * 128
    b = 2 * (2 * V * H + M * H + 3 * M * H) + 4 * H + 2 * (2 * (H * M + H * H) + 4 * 2 * H)
    return b + L * (4 * 2 * H + 2 * qkv * H + 4 * qkv + 2 * (H * H + 2 * I * H + H * I))


def time_fingerprint(model, reps=5):
    eng = model.engine
    eng.fingerprint()                                                   # (first call: allocations, code objects)
    ts = []
    for _ in range(reps):
        eng.weights_version += 1                                        # defeat the per-version cache
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fp = eng.fingerprint()
        ts.append(time.perf_counter() - t0)
    eng.weights_version -= reps
    s = float(np.median(ts))
    return {"fingerprint": fp, "ms": round(s * 1e3, 3), "gb": round(fingerprint_bytes(dims) / 1e9, 3), "gb_per_s": round(fingerprint_bytes(dims) / s / 1e9, 1)}


if a.fingerprint:
    fpr = {}
    for dt in ("f16", "bf16"):
        m = BlimModel(dims, max_positions=1024, dtype=dt)
        m.engine.init_synthetic_weights(0)
        fpr[dt] = time_fingerprint(m)
        m.engine.close()
        del m
        torch.cuda.empty_cache()
    buf = torch.empty(4 * 2**30 + 24, dtype=torch.uint8, device=dev)
    buf.fill_(7)
    E.hash_device(buf)
    ts = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        E.hash_device(buf)
        ts.append(time.perf_counter() - t0)
    s = float(np.median(ts))
    fpr["hash_4GiB"] = {"ms": round(s * 1e3, 3), "gb_per_s": round(buf.numel() / s / 1e9, 1)}
    del buf
    torch.cuda.empty_cache()
    rep["fingerprint"] = fpr

store = a.store or tempfile.mkdtemp(prefix="calstore-")
model = BlimModel(dims, max_positions=1024, dtype=a.dtype)
prob = synth.make_problem(a.seed, a.n, dims, tok_per_clip=64, fast_video=True)
loader = synth.ProblemLoader(prob, 64, video_dtype=torch.float16)
tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
nz = lambda x: np.where(x == 0, np.float32(1e-6), x)
ids = {i: i for i in range(a.n)}


def evaluate(vtg, tvg, use_store):
    args = types.SimpleNamespace(topk=a.topk, num_clips=dims.num_clips, cpn=True, resume="x", eval=True, dataset="MSRVTT", batch_size_eval=16,
                                 iv2_scores={"v2t": torch.from_numpy(nz(prob.v2t_sims)), "t2v": torch.from_numpy(nz(prob.t2v_sims))}, max_tokens=32768, dedup=True,
                                 calibration_store=store if use_store else None)
    model.clear_cache()
    model.tvg_precise = tvg
    model.vtg_precise = vtg                                             # (a new request: the in-process resolution starts over)
    torch.cuda.synchronize()
    t0 = time.time()
    t2v, v2t = RU.evaluation(DDPLike(model), loader, dev, tok, args)
    torch.cuda.synchronize()
    st = args._eval_stats
    return {"t2v": t2v, "v2t": v2t, "seconds": round(time.time() - t0, 3), "calibration_seconds": st.get("calibration_seconds"),
            "source": st.get("calibration_source"), "fingerprint": st.get("weights_fingerprint"), "vtg": st.get("vtg_precise"), "tvg": st.get("tvg_precise"),
            "mask": st.get("vtg_select_mask")}


def bit_equal(r1, r2):
    return all(np.array_equal(r1[d][k], r2[d][k]) for d in ("t2v", "v2t") for k in r1[d] if k != "internvideo2")


def recall(r):
    return TU.get_recall(r["t2v"]["query_likelihood"], r["v2t"]["candidate_likelihood"], ids, ids)


def brief(r):
    return {k: r[k] for k in ("seconds", "calibration_seconds", "source", "vtg", "tvg", "mask")}


requests = {"select": ("select", "full"), "auto": ("auto", "auto")}
try:
    for wname in a.weights.split(","):
        wseed = 0
        if wname != "gaussian":
            from oracle.gen_golden_heavy import CASES, heavy_items          # (the reshaped tensors of the trained-like fixtures)
            spec = CASES[wname]
            wseed = spec["wseed"]
        model.engine.init_synthetic_weights(wseed)
        if wname != "gaussian":
            for name, arr in heavy_items(dims, wseed, only_changed=True, sink=bool(spec.get("sink", False))):
                model.engine.load_weight(name, arr)
        out = {"fingerprint": model.engine.fingerprint()}
        if not a.no_full:
            out["full"] = brief(evaluate("full", "full", False))
        for mode in a.modes.split(","):
            vtg, tvg = requests[mode]
            plain = evaluate(vtg, tvg, False) if mode == "auto" else None      # `auto` without the store: what a warm run must reproduce bit for bit
            cold = evaluate(vtg, tvg, True)
            warm = evaluate(vtg, tvg, True)
            out[mode] = {"cold": brief(cold), "warm": brief(warm), "warm_bit_equal_cold": bit_equal(cold, warm),
                         "recall_equal": recall(cold) == recall(warm), "same_mask": cold["mask"] == warm["mask"]}
            if plain is not None:
                out[mode]["without_store"] = brief(plain)
                out[mode]["warm_bit_equal_without_store"] = bit_equal(plain, warm)
        rep[wname] = out
        print(json.dumps({wname: out}), file=sys.stderr, flush=True)
finally:
    model.engine.close()
    if a.store is None:
        shutil.rmtree(store, ignore_errors=True)
print(json.dumps(rep, indent=1))
