"""Development aid: attention class time on the SYN step and on reference-shaped VTG / TVG plans, optionally with another build of the library (BLIM_LIB=path)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from blim_amd import engine as eng
if os.environ.get("BLIM_LIB"):
    eng.load_library(os.path.join(ROOT, os.environ["BLIM_LIB"]))
import bench
from blim_amd import retrieval_utils as RU, synth
from blim_amd.modeling import BlimModel, DDPLike
dims = synth.ModelDims()
model = BlimModel(dims, max_positions=1024, dtype="f16")
model.engine.init_synthetic_weights(0)
((sc, plan, prob, pairs),) = bench.build_step_plans(model, 0, 1, 55, 16)
rprob = synth.make_problem(1, 96, dims, tok_per_clip=64, fast_video=True)
model.set_tvg_prefix_length(rprob.tvg_prefix_length)
tok = type("T", (), {"pad_token_id": synth.PAD_ID})()
Tt = lambda rows: [torch.from_numpy(r) for r in rows]
vtg = RU.padding_ids(Tt(rprob.vtg_ids), Tt(rprob.vtg_labels), Tt(rprob.vtg_masks), tok)
tvg = RU.padding_ids(Tt(rprob.tvg_ids), Tt(rprob.tvg_labels), Tt(rprob.tvg_masks), tok)
rsc = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in rprob.video], torch.from_numpy(rprob.video_vocab),
                    torch.from_numpy(rprob.tvg_video_labels), dims.num_clips, max_tokens=32768)
rpairs = RU._topk_pairs(torch.from_numpy(rprob.v2t_sims), 0, 28, True)
for name, scorer, pl in (("SYN VTG", sc, plan), ("REF VTG", rsc, rsc.plan_vtg(rpairs)[0]), ("REF TVG", rsc, rsc.plan_tvg(rpairs)[0])):
    scorer.run(pl); torch.cuda.synchronize()
    model.engine.timing_enable(True)
    scorer.run(pl); torch.cuda.synchronize()
    rep = model.engine.timing_report()
    model.engine.timing_enable(False)
    tot = sum(v["ms"] for v in rep.values())
    print(f"{os.environ.get('BLIM_LIB', 'product')}: {name}: attention {rep['attention']['ms']:.2f} ms of {tot:.1f} ms ({pl.batch.n_blocks} blocks, {pl.n_tokens} tokens)", flush=True)
