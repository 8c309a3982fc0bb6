"""`python -m blim_amd.search`: rerank text queries over a dataset's test videos with the gallery index (blim_amd/gallery.py).

The gallery is the dataset's test videos; their VTG prefixes are computed once (GalleryIndex.build) and every query is scored on its own response tokens.  Queries
are test captions (`--query_ids`) and / or free text (`--query TEXT`, tokenised by the dataset's own prompt builder: needs the real tokenizer).  `--candidates iv2`
takes each dataset query's top-k of the first-stage t2v row, `--candidates all` scores the whole gallery.  One JSON line per query: the ranked video ids and their
blended t2v scores (training_utils.combine_and_rank's t2v half: `--cpn --alpha --c`; zero-shot runs blend the query likelihood with the first stage only).
`--synthetic N [--synthetic_7b]`: a dry run on synth.make_problem, as main.py's.  `--gallery_fill lazy` computes no prefix up front: the first query runs at once, its
calls leave their videos' prefixes in the cache, and `--gallery_gb` is the cache's capacity.  The `gallery stats:` stderr line reports the hits
and misses.  `--gallery_host_gb` / `--text_gallery_host_gb` (lazy fill) keep the evicted slots in pinned host memory; one more stderr line
reports what that tier did.

`--direction v2t` is the other half: the gallery is the dataset's test captions and the queries are test videos (`--video_ids`).  The candidate likelihood (VTG) is
served from the same video cache; a fine-tuned checkpoint's query likelihood (TVG) reads the captions' prompts from a second cache (TextGalleryIndex,
`--text_gallery_gb`), and the CPN prior is kept per text.  One JSON line per query video: the ranked text indices and their blended v2t scores.
"""
from __future__ import annotations

import argparse
import json
import sys
import time


def get_args_parser():
    p = argparse.ArgumentParser("BLiM gallery search", add_help=True)
    p.add_argument("--model_path", default="./pretrained/VideoChat-Flash-Qwen2-7B_res448", type=str)
    p.add_argument("--dataset", default="DiDeMo", type=str, choices=["DiDeMo", "ActivityNet", "LSMDC", "MSRVTT"])
    p.add_argument("--resume", default="", type=str, help="fine-tuned LoRA / visual_head checkpoint (empty = zero-shot)")
    p.add_argument("--num_clips", default=4, type=int)
    p.add_argument("--dtype", default=None, choices=["f16", "bf16", "f8"])
    p.add_argument("--vtg_precise", default="auto", choices=["auto", "none", "full", "select"])
    p.add_argument("--tvg_precise", default="auto", choices=["auto", "attn", "full"])
    p.add_argument("--second_pass", default=None, choices=["e2m3", "16bit", "auto"], help="auto is refused here (it is measured inside evaluation() only)")
    p.add_argument("--calibration_store", default=None, type=str, metavar="DIR", help="refused: the index's mode resolution does not use the store")
    p.add_argument("--cpn", action="store_true")
    p.add_argument("--alpha", default=[0.0, 0.0], type=float, nargs="+")
    p.add_argument("--c", default=None, type=float, nargs="+",
                   help="ensemble weights as main.py's; only c0 (query vs candidate likelihood) and c2 (likelihood vs first stage) act on t2v, only c1 and c3 (likewise) "
                        "on v2t.  Default: t2v 1 0 1 0 (the query likelihood alone), v2t 1 0 1 1 (c1 = 0, c3 = 1: the VTG likelihood alone)")
    p.add_argument("--topk", default=10, type=int)
    p.add_argument("--lora_r", default=8, type=int)
    p.add_argument("--lora_alpha", default=32, type=int)
    p.add_argument("--query_ids", default=[], type=int, nargs="*", help="test captions (indices) used as queries")
    p.add_argument("--query", default=[], type=str, action="append", help="a free-text query (repeatable)")
    p.add_argument("--direction", default="t2v", choices=["t2v", "v2t"], help="t2v: text queries over the videos; v2t: video queries (--video_ids) over the captions")
    p.add_argument("--video_ids", default=[], type=int, nargs="*", help="test videos (indices) used as queries (--direction v2t)")
    p.add_argument("--candidates", default="iv2", choices=["iv2", "all"])
    p.add_argument("--gallery_gb", default=None, type=float, help="device memory for the prefix cache (default: every video)")
    p.add_argument("--text_gallery_gb", default=None, type=float, help="v2t: device memory for the caption-prompt cache (default: every distinct prompt)")
    p.add_argument("--gallery_fill", default="eager", choices=["eager", "lazy"],
                   help="eager: every prefix under the budget is computed before the first query; lazy: nothing is, --gallery_gb / --text_gallery_gb are capacities, a "
                        "query's own calls capture the prefixes they had to pack and the least recently used slots make room")
    p.add_argument("--gallery_host_gb", default=None, type=float,
                   help="--gallery_fill lazy: pinned host memory that keeps the video slots the cache evicts; a video with a record there is copied back instead of decoded again")
    p.add_argument("--text_gallery_host_gb", default=None, type=float, help="v2t, --gallery_fill lazy: the same for the caption-prompt cache")
    p.add_argument("--narrow_gemm", default="off", choices=["off", "auto"],
                   help="auto: o_proj and down of small scoring calls run on the narrow-tile residual GEMM (engine option \"narrow_gemm\" = 1): the same scores bit for bit, "
                        "spread over the whole chip.  Refused with --dtype f8")
    p.add_argument("--narrow_lo6", default="off", choices=["off", "auto"],
                   help="auto: the same for the compensated o_proj and down launches that carry the e2m3 second pass (fp16 engines; bf16 under --second_pass e2m3): engine "
                        "option \"narrow_lo6\" = 1, the same scores bit for bit.  Does nothing where the compensated calls walk K twice in 16 bits (those are "
                        "--narrow_gemm's).  Refused with --dtype f8")
    p.add_argument("--narrow_qkv", default="off", choices=["off", "auto"],
                   help="auto: the QKV projection of small scoring calls runs on the narrow-tile QKV GEMM (engine option \"narrow_qkv\" = 1), in the plain, compensated and "
                        "e2m3 second-pass forms alike: the same scores bit for bit.  Refused with --dtype f8")
    p.add_argument("--max_tokens", default=24576, type=int)
    p.add_argument("--shard", default=None, type=int, nargs=2, metavar=("W", "RANK"))
    p.add_argument("--synthetic", default=0, type=int)
    p.add_argument("--synthetic_7b", action="store_true")
    p.add_argument("--output", default=None, type=str, help="write the JSON lines here too")
    return p


def check_args(args, world: int = 1) -> None:
    """Refusals (SystemExit with the reason): what the gallery index does not cover."""
    if getattr(args, "narrow_gemm", "off") == "auto" and args.dtype == "f8":
        raise SystemExit("search: --narrow_gemm auto needs a 16-bit engine (--dtype f16 | bf16): the narrow residual GEMM takes fp16 / bf16 operands")
    if getattr(args, "narrow_lo6", "off") == "auto" and args.dtype == "f8":
        raise SystemExit("search: --narrow_lo6 auto needs a 16-bit engine (--dtype f16 | bf16): the narrow residual GEMM with the e2m3 second pass takes fp16 / bf16 operands")
    if getattr(args, "narrow_qkv", "off") == "auto" and args.dtype == "f8":
        raise SystemExit("search: --narrow_qkv auto needs a 16-bit engine (--dtype f16 | bf16): the narrow QKV GEMM takes fp16 / bf16 operands")
    if args.dtype == "f8":
        raise SystemExit("search: --dtype f8 is not supported (the prefix cache needs a 16-bit engine: --dtype f16 | bf16)")
    if args.shard is not None:
        raise SystemExit("search: --shard is not supported (a gallery is not sharded over ranks)")
    if world > 1:
        raise SystemExit(f"search: world size {world} > 1 is not supported (run one process)")
    for flag in ("gallery_host_gb", "text_gallery_host_gb"):
        if getattr(args, flag, None) is not None and args.gallery_fill != "lazy":
            raise SystemExit(f"search: --{flag} needs --gallery_fill lazy (the host tier keeps the slots a lazy cache evicts; an eager cache is filled once and evicts none)")
        if getattr(args, flag, None) is not None and getattr(args, flag) < 0:
            raise SystemExit(f"search: --{flag} must not be negative")
    v2t = getattr(args, "direction", "t2v") == "v2t"
    if args.c is None:                        # the likelihood of the direction alone: t2v c0 = c2 = 1; v2t c1 = 0, c3 = 1
        args.c = [1.0, 0.0, 1.0, 1.0] if v2t else [1.0, 0.0, 1.0, 0.0]
    if v2t:
        if args.query or args.query_ids:
            raise SystemExit("search: --direction v2t takes video queries (--video_ids), not --query / --query_ids")
        if not args.video_ids:
            raise SystemExit("search: --direction v2t needs --video_ids")
    else:
        if getattr(args, "video_ids", None):
            raise SystemExit("search: --video_ids are the queries of --direction v2t (t2v takes --query_ids and / or --query)")
        if not args.query_ids and not args.query:
            raise SystemExit("search: give --query_ids and / or --query")
    if args.query and args.candidates == "iv2":
        raise SystemExit("search: free-text queries have no first-stage row: use --candidates all")
    if args.query and args.synthetic:
        raise SystemExit("search: free-text queries need the dataset's tokenizer (not --synthetic)")
    if len(args.c) != 4 or len(args.alpha) != 2:
        raise SystemExit("search: --c takes 4 values, --alpha 2")
    if v2t and args.c[3] == 0:
        raise SystemExit("search: --c with c3 = 0 ranks by the first-stage scores alone (the likelihood would have no effect): give c3 > 0, e.g. the v2t default 1 0 1 1")
    if not v2t and args.c[2] == 0:
        raise SystemExit("search: --c with c2 = 0 ranks by the first-stage scores alone (the likelihood would have no effect): give c2 > 0, e.g. the default 1 0 1 0")
    if args.calibration_store:
        raise SystemExit("search: --calibration_store is not supported: the gallery resolves --vtg_precise auto | select on its own sample without the store; "
                         "pass the mode a stored evaluation resolved (--vtg_precise none | full) instead")
    if args.second_pass == "auto":
        raise SystemExit("search: --second_pass auto is not supported (it is measured by evaluation()): give e2m3 or 16bit")


def main(args):
    import os
    import types

    import numpy as np
    import torch

    from . import distributed as D
    from . import retrieval_utils as RU
    from . import synth
    from .gallery import GalleryIndex
    from .modeling import BlimModel, DDPLike

    check_args(args, int(os.environ.get("WORLD_SIZE", "1")))
    t0 = time.time()
    T = torch.from_numpy
    if args.synthetic > 0:
        dims = synth.ModelDims(num_clips=args.num_clips) if args.synthetic_7b else synth.ModelDims(
            vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64, num_clips=args.num_clips)
        model = BlimModel(dims, dtype=args.dtype)
        model.engine.init_synthetic_weights(0)
        prob = synth.make_problem(1, args.synthetic, dims, tok_per_clip=64 if args.synthetic_7b else 8, fast_video=args.synthetic > 256)
        tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
        rows = lambda a: [T(r) for r in a]
        vtg_ids, vtg_lab, vtg_msk = prob.vtg_ids, prob.vtg_labels, prob.vtg_masks
        tvg_ids, tvg_lab, tvg_msk = prob.tvg_ids, prob.tvg_labels, prob.tvg_masks
        video, vocab, vlab = [T(v) for v in prob.video], T(prob.video_vocab), T(prob.tvg_video_labels)
        t2v_iv2, v2t_iv2 = prob.t2v_sims, prob.v2t_sims
        vids = [str(j) for j in range(len(video))]
        model.set_tvg_prefix_length(prob.tvg_prefix_length)
        vtg_ids, vtg_lab, vtg_msk, tvg_ids, tvg_lab, tvg_msk = (rows(x) for x in (vtg_ids, vtg_lab, vtg_msk, tvg_ids, tvg_lab, tvg_msk))
    else:
        from .checkpoint import load_checkpoint
        from .dataloader import RetrievalDataset
        from .main import dims_from_config, load_tokenizer
        tok = load_tokenizer(args.model_path)
        dims = dims_from_config(args.model_path, args.num_clips)
        cfg_json = json.load(open(os.path.join(args.model_path, "config.json")))
        model = BlimModel(dims, dtype=args.dtype, tokenizer_model_max_length=cfg_json.get("tokenizer_model_max_length"))
        load_checkpoint(model.engine, dims, args.model_path, args.resume or None, lora_r=args.lora_r, lora_alpha=args.lora_alpha)
        args.eval = True
        ds = RetrievalDataset(args, tokenizer=tok, split="test")
        items = [ds[i] for i in range(len(ds))]
        video = [it["video"] for it in items]
        vids = [it["vid"] for it in items]
        vtg_ids, vtg_lab, vtg_msk = [it["vtg_ids"] for it in items], [it["vtg_labels"] for it in items], [it["vtg_masks"] for it in items]
        tvg_ids, tvg_lab, tvg_msk = [it["tvg_ids"] for it in items], [it["tvg_labels"] for it in items], [it["tvg_masks"] for it in items]
        from .dataloader import DEFAULT_IMAGE_TOKEN, TVG_PROMPT, VTG_PROMPTS
        for q in args.query:                      # free text: the dataset's own prompt builder
            a = ds._ids_labels(f"{DEFAULT_IMAGE_TOKEN}\n{VTG_PROMPTS[ds.dataset]}", q)
            b = ds._ids_labels(f"{TVG_PROMPT}\nCaption: {q}", DEFAULT_IMAGE_TOKEN)
            vtg_ids.append(a[0]); vtg_lab.append(a[1]); vtg_msk.append(a[2]); tvg_ids.append(b[0]); tvg_lab.append(b[1]); tvg_msk.append(b[2])
        vocab, vlab = ds.video_vocab, torch.tensor([it["tvg_video_labels"] for it in items])
        model.set_tvg_prefix_length(ds.tvg_prefix_length)
        finetuned_ = bool(args.resume)
        first = torch.load(f"./scores/{args.dataset.lower()}{'' if finetuned_ else '_zeroshot'}.pth", weights_only=True) if args.candidates == "iv2" else None
        t2v_iv2 = None if first is None else first["t2v"].numpy()
        v2t_iv2 = None if first is None else first["v2t"].numpy()
    if getattr(args, "narrow_gemm", "off") == "auto":
        model.engine.set_option("narrow_gemm", 1)
    if getattr(args, "narrow_lo6", "off") == "auto":
        model.engine.set_option("narrow_lo6", 1)
    if getattr(args, "narrow_qkv", "off") == "auto":
        model.engine.set_option("narrow_qkv", 1)
    if model.engine.can_precise:
        model.tvg_precise = args.tvg_precise
        model.vtg_precise = None if args.vtg_precise == "none" else args.vtg_precise
        if args.second_pass:
            model.second_pass = args.second_pass
    vtg = RU.padding_ids(vtg_ids, vtg_lab, vtg_msk, tok)
    tvg = RU.padding_ids(tvg_ids, tvg_lab, tvg_msk, tok)
    scorer = RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], video, vocab, vlab, args.num_clips, max_tokens=args.max_tokens)
    budget = None if args.gallery_gb is None else int(args.gallery_gb * 2**30)
    host = None if args.gallery_host_gb is None else int(args.gallery_host_gb * 2**30)
    gal = GalleryIndex(scorer, budget_bytes=budget, fill=args.gallery_fill, host_budget_bytes=host)
    if args.direction == "v2t":
        return _main_v2t(args, model, scorer, gal, v2t_iv2, vids, len(tvg_ids), t0)
    gal.build(first_stage=None if t2v_iv2 is None else np.ascontiguousarray(np.asarray(t2v_iv2, dtype=np.float32).T))     # v2t first stage: calibration sample
    print(f"gallery: {len(video)} videos, fill {gal.fill}, {gal.n_slots} {'slots' if gal.fill == 'lazy' else 'cached slots'} of {gal.cache.bytes // max(gal.n_slots, 1) if gal.cache else 0} bytes, "
          f"mode {scorer.vtg_mode or 'none'}, narrow_gemm {getattr(args, 'narrow_gemm', 'off')}, narrow_lo6 {getattr(args, 'narrow_lo6', 'off')}, narrow_qkv {getattr(args, 'narrow_qkv', 'off')}, built in {gal.build_seconds:.2f}s (ready {time.time() - t0:.1f}s after start)", file=sys.stderr, flush=True)
    n_ds = len(vtg_ids) - len(args.query)
    texts = list(args.query_ids) + list(range(n_ds, len(vtg_ids)))
    names = [f"caption:{i}" for i in args.query_ids] + [f"query:{q}" for q in args.query]
    N = len(video)
    k = min(args.topk, N)
    finetuned = bool(args.resume)
    out = open(args.output, "w") if args.output else None
    for t, name in zip(texts, names):
        if args.candidates == "iv2":
            row = np.asarray(t2v_iv2[t], dtype=np.float32)
            cand = np.argsort(-row, kind="stable")[:k][None]
            fs = row[cand]
        else:
            cand = np.arange(N)[None]
            fs = None if t2v_iv2 is None else np.asarray(t2v_iv2[t], dtype=np.float32)[cand] if t < n_ds else None
        order, blended = gal.rerank([t], cand, first_stage=fs, cpn=args.cpn, alpha=args.alpha, c=args.c, finetuned=finetuned)
        line = json.dumps({"query": name, "videos": [vids[int(j)] for j in order[0]], "scores": [float(x) for x in blended[0]]})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()
    print(f"gallery stats: {json.dumps(gal.stats.as_dict())}", file=sys.stderr, flush=True)
    if gal.host is not None:
        print(f"gallery host tier: {json.dumps(dict(gal.host.stats.as_dict(), records=gal.host.n_records, record_bytes=gal.host.record_bytes))}", file=sys.stderr, flush=True)
    gal.close()
    model.engine.close()
    return 0


def _main_v2t(args, model, scorer, gal, v2t_iv2, vids, n_texts: int, t0: float) -> int:
    """Video queries over the captions: the VTG leg from the video cache, the fine-tuned TVG leg from the caption-prompt cache."""
    import numpy as np

    from .gallery import TextGalleryIndex
    n_videos = len(vids)
    first = None if v2t_iv2 is None else np.ascontiguousarray(np.asarray(v2t_iv2, dtype=np.float32))
    gal.build(first_stage=first)
    finetuned = bool(args.resume)
    tbudget = None if args.text_gallery_gb is None else int(args.text_gallery_gb * 2**30)
    thost = None if args.text_gallery_host_gb is None else int(args.text_gallery_host_gb * 2**30)
    tg = TextGalleryIndex(scorer, budget_bytes=tbudget, video_index=gal, fill=args.gallery_fill, host_budget_bytes=thost)
    if finetuned:                                     # a zero-shot blend has no TVG term: no caption cache
        tg.build(first_stage=first)
    print(f"gallery: {n_videos} videos, fill {gal.fill}, {gal.n_slots} {'slots' if gal.fill == 'lazy' else 'cached slots'}, mode {scorer.vtg_mode or 'none'}, built in {gal.build_seconds:.2f}s; "
          f"{n_texts} texts, {tg.n_slots} caption slots of {tg.per_slot_bytes()} bytes, tvg mode {scorer.tvg_mode}, narrow_gemm {getattr(args, 'narrow_gemm', 'off')}, narrow_lo6 {getattr(args, 'narrow_lo6', 'off')}, narrow_qkv {getattr(args, 'narrow_qkv', 'off')}, built in {tg.build_seconds:.2f}s "
          f"(ready {time.time() - t0:.1f}s after start)", file=sys.stderr, flush=True)
    bad = [v for v in args.video_ids if not 0 <= v < n_videos]
    if bad:
        raise SystemExit(f"search: --video_ids {bad} outside 0 .. {n_videos - 1}")
    k = min(args.topk, n_texts)
    out = open(args.output, "w") if args.output else None
    for v in args.video_ids:
        if args.candidates == "iv2":
            row = np.asarray(v2t_iv2[v], dtype=np.float32)
            cand = np.argsort(-row, kind="stable")[:k][None]
            fs = row[cand]
        else:
            cand = np.arange(n_texts)[None]
            fs = None if v2t_iv2 is None else np.asarray(v2t_iv2[v], dtype=np.float32)[cand]
        order, blended = tg.rerank([v], cand, first_stage=fs, cpn=args.cpn, alpha=args.alpha, c=args.c, finetuned=finetuned)
        line = json.dumps({"query": f"video:{vids[v]}", "texts": [int(i) for i in order[0]], "scores": [float(x) for x in blended[0]]})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()
    print(f"gallery stats: {json.dumps(gal.stats.as_dict())}; text gallery stats: {json.dumps(tg.stats.as_dict())}", file=sys.stderr, flush=True)
    tiers = [(name, ix.host) for name, ix in (("gallery", gal), ("text gallery", tg)) if ix.host is not None]
    if tiers:
        print("; ".join(f"{name} host tier: {json.dumps(dict(h.stats.as_dict(), records=h.n_records, record_bytes=h.record_bytes))}" for name, h in tiers), file=sys.stderr, flush=True)
    tg.close()
    gal.close()
    model.engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(get_args_parser().parse_args()))
