"""`python -m blim_amd.search`: rerank text queries over a dataset's test videos with the gallery index (blim_amd/gallery.py).

The gallery is the dataset's test videos; their VTG prefixes are computed once (GalleryIndex.build) and every query is scored on its own response tokens.  Queries
are test captions (`--query_ids`) and / or free text (`--query TEXT`, tokenised by the dataset's own prompt builder: needs the real tokenizer).  `--candidates iv2`
takes each dataset query's top-k of the first-stage t2v row, `--candidates all` scores the whole gallery.  `--candidates tvg` (fine-tuned checkpoints: `--resume`;
DESIGN.md section 18) needs no first stage: the whole gallery is ranked by the TVG candidate term of the blend, log P(video | text) (minus alpha[0] x its prior with
`--cpn`; PairScorer.tvg_gallery, the caption prompt once and num_clips - 1 clip tokens per video), the best `--shortlist K` (default `--topk`) are reranked with that
term reused and a zero first-stage term, the best `--topk` of them are printed, the JSON line gains `"shortlisted": K`, and a `shortlist:` stderr line at the end
counts the queries, the stage-1 passes and their pairs.  It serves `--query`, `--query_ids` and, under `--direction v2t`, `--video_ids` (there the captions are
ranked by the query likelihood over the cached prompts: TextGalleryIndex.shortlist).  `--prefilter K0` (t2v) puts a stage in front of that: the
whole gallery is ranked ON THE DEVICE by the clip-0 term of the TVG likelihood -- one logits row per query, whatever the gallery's size -- and the TVG ranking runs on
the best K0 only; the JSON line gains `"prefiltered": K0` and a `prefilter:` stderr line is printed at the end.  `--caption_prefilter K0` (v2t, DESIGN.md section
22) is the other direction's stage: every caption's clip-0 term for the query video comes from the cached prompts' stored rows with no decode
(TextGalleryIndex.prefilter), the per-video TVG pass runs over the best K0 captions, and the answer line and the `prefilter:` line are the same.  One JSON line per query: the ranked video ids and their
blended t2v scores (training_utils.combine_and_rank's t2v half: `--cpn --alpha --c`; zero-shot runs blend the query likelihood with the first stage only).
`--synthetic N [--synthetic_7b]`: a dry run on synth.make_problem, as main.py's.  `--gallery_fill lazy` computes no prefix up front: the first query runs at once, its
calls leave their videos' prefixes in the cache, and `--gallery_gb` is the cache's capacity.  The `gallery stats:` stderr line reports the hits
and misses.  `--gallery_host_gb` / `--text_gallery_host_gb` (lazy fill) keep the evicted slots in pinned host memory; one more stderr line
reports what that tier did.

`--direction v2t` is the other half: the gallery is the dataset's test captions and the queries are test videos (`--video_ids`).  The candidate likelihood (VTG) is
served from the same video cache; a fine-tuned checkpoint's query likelihood (TVG) reads the captions' prompts from a second cache (TextGalleryIndex,
`--text_gallery_gb`), and the CPN prior is kept per text.  One JSON line per query video: the ranked text indices and their blended v2t scores.

`--serve` (t2v): the model is loaded and the gallery built as above, then the command reads one JSON request per line from stdin until EOF and
writes one JSON line per request to stdout, in arrival order.  A request: `id` (any JSON scalar, echoed); exactly one of `caption` (a test caption's index), `text`
(free text through the dataset's prompt builder, as `--query`; refused per request under `--synthetic`) and `rows` ({"vtg_ids", "vtg_labels"[, "tvg_ids",
"tvg_labels"]}, raw token rows); optionally `candidates` (video ids as printed in `videos`) or `candidate_idx` (indices), `first_stage` (floats, parallel to the
candidates) and `topk` (truncates the answer).  Without candidates a `caption` request takes `--candidates` (`iv2`: its top-`--topk` of the first stage; `all`: the
gallery; `tvg`: the shortlist); a `text` / `rows` request takes the whole gallery under `all`, the shortlist under `tvg`, and gets an error line under `iv2`.  A
request may carry `"shortlist": K` itself, under any `--candidates`: its candidates are the best K of the gallery's TVG ranking and its answer gains
`"shortlisted": K`; next to it (or next to the default K under `--candidates tvg`) `"prefilter": K0` narrows the gallery to K0 >= K videos first and the answer gains
`"prefiltered": K0`; with `candidates` / `candidate_idx` or `first_stage`, a K that is no positive integer, a query without a TVG row, or a model without `--resume` it
gets an error line.  The answer is {"id", "query", "videos", "scores"} or
{"id", "error"}: a bad request (malformed JSON, an unknown video id, an empty or duplicate candidate list, a row that fails PairScorer.add_texts' checks or leaves no
response token under tokenizer_model_max_length, a fine-tuned blend with c0 < 1 for rows without a TVG row) gets its error line and the process goes on.
`--batch_queries B` / `--batch_wait_ms W`: a reader thread queues the lines; the loop takes what is waiting, up to B requests, waits at most W ms for more only while
fewer are there, and scores the batch as ONE pass (GalleryIndex.search_requests, one gallery.SearchRequest per request: the shortlist requests of a batch share one
stage-1 pass, all requests one VTG pass)
-- the same scores as one pass per request, bit for bit on the VTG term and on a shortlist's stage 1.  Texts join the
scorer at run time (PairScorer.add_texts); identical `text` / `rows` queries share one text index.  At EOF a `serve:` stderr line counts requests, batches, the mean
batch size, errors and texts added (and, once a video was added, `videos_added`).

Videos join a running gallery too.  A request `{"id", "add_video": {"vid": NAME, "features": PATH}}` -- PATH a feature file as blim_amd.extract
writes it, read with torch.load(weights_only=True) -- is answered with {"id", "added": NAME, "index": j, "videos": N}; it is validated in full first (the file, the
tensor's shape, a `vid` the gallery does not know yet, features whose content no video added at run time has: engine.hash_device) and a bad one gets its error line.
An add is a barrier in the stream: a micro-batch never spans it, the requests in front of it are scored against the old gallery and those behind it against the new,
where `candidates` may name NAME; answers stay in arrival order.  The video's vocabulary row is its clip mean (dataloader.py's rule) and the whole vocabulary is
registered again, so every later TVG score is normalised over the grown gallery; a run-time video has no first-stage score (a zero term under `--candidates all`).
`--gallery_spare S` (eager fill) keeps S free slots, counted against `--gallery_gb`, that such videos' prefixes are filled into; beyond them, and always under
`--gallery_fill lazy`, they are served as any miss.  `--direction v2t --query_video FILE [FILE ...]`: the files' videos join before the indexes are built and the
captions are ranked for each (`"query": "video:<basename>"`; `--candidates all | tvg`, `iv2` is refused: no first-stage row).  All outside videos of one run share one
vocabulary, so a TVG term depends on which others were given.

Raw frames.  `{"id", "add_video": {"vid": NAME, "frames": PATH}}` -- PATH a .npy of uint8 [n, H, W, 3], read with allow_pickle=False -- is the
same request with the features computed here: the frames are sampled to 16 by blim_amd.extract's rule for frame stacks, resized and normalised on the GPU
(vision.preprocess_device), run through the vision tower, and the fp16 tensor enters the `features` path above (its checks, the duplicate-content digest, the barrier,
the `added` reply), so a video added from frames and the same video added from its extracted feature file are duplicates and score alike.  Exactly one of `features`
and `frames`.  An unreadable or non-uint8 file, a wrong rank or channel count, no frame, or a tower that cannot be loaded gets its error line.  A `--query_video` FILE
ending in `.npy` is such a frame stack too.  The tower is created at the first use of frames, from `--vision_model_path` (default `--model_path`) or, for dry runs,
`--vision_synthetic SEED`.

Inside a set of the caller's.  A request may carry `"within": [video ids]` or `"within_idx": [indices]` next to `"shortlist": K` (or next to the
default K under `--candidates tvg`), with `"prefilter": K0` or the `--prefilter` default optional: the shortlist -- and the prefilter in front of it -- rank the
videos of the set alone, K and K0 clipped to its size M, and the answer gains `"within": M`.  The clip-0 values are the whole gallery's (the normaliser still runs
over every registered video, which keeps a score equal to the evaluation's), so the result is the unfiltered order filtered to the set, at the cost of the unfiltered
request.  A caller can hide a video this way without changing any score; a video that is gone for good is removed (below).  Both forms at once, `within` with `candidates` /
`candidate_idx` / `first_stage`, `within` with neither a shortlist nor `--candidates tvg`, an empty list, an unknown id and a repeated id each get an error line;
an `add_video` request refuses the keys as it refuses other query keys, and a set behind the barrier may name the new video.  One-shot: `--within_ids FILE` (one
video id per line; t2v, `--candidates tvg`) confines every query of the run.  A `within:` stderr line counts the requests that carried a set and the videos named.

Videos leave a running gallery.  A request `{"id", "remove_video": VID}` is answered with {"id", "removed": VID, "index": j, "videos": <live
count>}; it is validated in full first (an unknown id, an id removed already, the last video of the gallery, a request that also carries query keys and a value that
is no JSON scalar each get an error line) and it is a barrier exactly as `add_video` is: the requests in front of it are scored against the old gallery and answered
first, those behind it see the new one, a micro-batch never spans it.  Indices never move: the removed index stays a tombstone, its id and its content digest are
forgotten -- the same features may join again, under the same or another id, at a new index --, `candidates` / `within` that name it get the "unknown video id"
words and `candidate_idx` / `within_idx` "video j was removed"; `--candidates all` means the videos that are left, `iv2` the top-k of the first-stage row among
them.  The vocabulary is registered again without the video's entry, so every later TVG score is that of an evaluation over the gallery as it now is; the cache slot
of its prefix is free at once, and under `--gallery_fill eager` the next `add_video` is filled into it even with `--gallery_spare 0`.  The EOF `serve:` line gains
`videos_removed`, and a `removed:` stderr line counts the videos, the slots freed and the host records forgotten -- both only when a removal happened.  There is no
one-shot flag: a one-shot run simply does not load the video.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

from .main import NARROW_GEMMS


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
    p.add_argument("--candidates", default="iv2", choices=["iv2", "all", "tvg"],
                   help="iv2: the first stage's top --topk; all: the whole gallery; tvg (fine-tuned checkpoints, --resume): the whole gallery ranked by the TVG likelihood, "
                        "the best --shortlist reranked")
    p.add_argument("--shortlist", default=None, type=int, metavar="K", help="--candidates tvg: candidates kept from the TVG ranking of the gallery (default: --topk)")
    p.add_argument("--prefilter", default=None, type=int, metavar="K0",
                   help="--candidates tvg, t2v: the whole gallery is first ranked on the device by the clip-0 term of the TVG likelihood (one logits row per query, "
                        "whatever the gallery's size), the TVG ranking runs on the best K0 >= --shortlist only")
    p.add_argument("--within_ids", default=None, type=str, metavar="FILE",
                   help="--candidates tvg, t2v one-shot: one video id per line; every query of the run is shortlisted (and, with --prefilter, prefiltered) inside this "
                        "set of videos alone, K and K0 clipped to its size")
    p.add_argument("--caption_prefilter", default=None, type=int, metavar="K0",
                   help="--candidates tvg, v2t: every caption is first ranked on the device by the clip-0 term of the query likelihood, read from the cached prompts' "
                        "stored rows (no decode, one pass for all query videos), the TVG ranking runs on the best K0 >= --shortlist captions only")
    p.add_argument("--query_video", default=[], type=str, nargs="*", metavar="FILE",
                   help="--direction v2t: feature files of videos outside the dataset ([num_clips, tokens, width] tensors as blim_amd.extract writes them) used as queries; "
                        "they join the scorer (PairScorer.add_videos) before the indexes are built.  --candidates all | tvg")
    p.add_argument("--vision_model_path", default=None, type=str,
                   help="raw frames (--serve: add_video frames; --direction v2t: a --query_video FILE ending in .npy): the checkpoint the vision tower is loaded from "
                        "at the first use of frames (default: --model_path)")
    p.add_argument("--vision_synthetic", default=None, type=int, metavar="SEED", help="raw frames: seeded random tower weights instead of the checkpoint (dry run)")
    p.add_argument("--gallery_gb", default=None, type=float, help="device memory for the prefix cache (default: every video)")
    p.add_argument("--gallery_spare", default=0, type=int, metavar="S",
                   help="--gallery_fill eager: S free slots beyond the planned ones, for the videos that join at run time (--serve: add_video).  They count against --gallery_gb")
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
    p.add_argument("--serve", action="store_true",
                   help="t2v: after the gallery is built, read one JSON request per line from stdin until EOF and answer each with one JSON line on stdout, in arrival "
                        "order (see the module text)")
    p.add_argument("--batch_queries", default=1, type=int, help="--serve: up to this many waiting requests are scored in one pass")
    p.add_argument("--batch_wait_ms", default=0.0, type=float, help="--serve: with fewer than --batch_queries requests waiting, wait at most this long for more")
    return p


def shortlist_k(args) -> int:
    """--candidates tvg: the candidates kept from the TVG ranking (--shortlist, default --topk)."""
    return int(args.topk if args.shortlist is None else args.shortlist)


def check_args(args, world: int = 1) -> None:
    """Refusals (SystemExit with the reason): what the gallery index does not cover."""
    for flag, gemm in NARROW_GEMMS.items():
        if getattr(args, flag) == "auto" and args.dtype == "f8":
            raise SystemExit(f"search: --{flag} auto needs a 16-bit engine (--dtype f16 | bf16): {gemm} takes fp16 / bf16 operands")
    if args.dtype == "f8":
        raise SystemExit("search: --dtype f8 is not supported (the prefix cache needs a 16-bit engine: --dtype f16 | bf16)")
    if args.shard is not None:
        raise SystemExit("search: --shard is not supported (a gallery is not sharded over ranks)")
    if world > 1:
        raise SystemExit(f"search: world size {world} > 1 is not supported (run one process)")
    for flag in ("gallery_host_gb", "text_gallery_host_gb"):
        if getattr(args, flag) is not None and args.gallery_fill != "lazy":
            raise SystemExit(f"search: --{flag} needs --gallery_fill lazy (the host tier keeps the slots a lazy cache evicts; an eager cache is filled once and evicts none)")
        if getattr(args, flag) is not None and getattr(args, flag) < 0:
            raise SystemExit(f"search: --{flag} must not be negative")
    spare = args.gallery_spare
    if spare < 0:
        raise SystemExit("search: --gallery_spare must not be negative")
    if spare and args.gallery_fill != "eager":
        raise SystemExit("search: --gallery_spare keeps free slots in an eager cache (--gallery_fill eager); a lazy cache admits a video that joins on demand, under --gallery_gb")
    v2t = args.direction == "v2t"
    if args.c is None:                        # the likelihood of the direction alone: t2v c0 = c2 = 1; v2t c1 = 0, c3 = 1
        args.c = [1.0, 0.0, 1.0, 1.0] if v2t else [1.0, 0.0, 1.0, 0.0]
    serve = bool(args.serve)
    if serve:
        if v2t:
            raise SystemExit("search: --serve answers text queries over the videos only (--direction t2v); v2t is not served")
        if args.query or args.query_ids or args.video_ids:
            raise SystemExit("search: --serve reads its queries from stdin, one JSON request per line (not --query / --query_ids / --video_ids)")
        if args.batch_queries < 1 or args.batch_wait_ms < 0:
            raise SystemExit("search: --batch_queries must be at least 1 and --batch_wait_ms must not be negative")
    elif args.batch_queries != 1 or args.batch_wait_ms != 0:
        raise SystemExit("search: --batch_queries / --batch_wait_ms batch the requests of --serve")
    if v2t:
        if args.query or args.query_ids:
            raise SystemExit("search: --direction v2t takes video queries (--video_ids), not --query / --query_ids")
        outside = args.query_video
        if not args.video_ids and not outside:
            raise SystemExit("search: --direction v2t needs --video_ids")
        if outside and args.candidates == "iv2":
            raise SystemExit("search: --query_video: a video outside the dataset has no first-stage row (--candidates iv2): use --candidates all, or tvg with --resume")
    else:
        if args.query_video:
            raise SystemExit("search: --query_video files are the queries of --direction v2t (t2v takes --query_ids and / or --query)")
        if args.video_ids:
            raise SystemExit("search: --video_ids are the queries of --direction v2t (t2v takes --query_ids and / or --query)")
        if not args.query_ids and not args.query and not serve:
            raise SystemExit("search: give --query_ids and / or --query")
    if args.query and args.candidates == "iv2":
        raise SystemExit("search: free-text queries have no first-stage row: use --candidates all")
    if args.query and args.synthetic:
        raise SystemExit("search: free-text queries need the dataset's tokenizer (not --synthetic)")
    if args.candidates == "tvg" and not args.resume:
        raise SystemExit("search: --candidates tvg needs a fine-tuned checkpoint (--resume): a zero-shot model's visual head is untrained, so it has no TVG likelihood to "
                         "rank the gallery by")
    if args.shortlist is not None and args.candidates != "tvg":
        raise SystemExit("search: --shortlist is the number of candidates --candidates tvg keeps (give --candidates tvg)")
    if args.candidates == "tvg" and shortlist_k(args) < 1:
        raise SystemExit("search: --shortlist must be at least 1 (it defaults to --topk)")
    K0 = args.prefilter
    if K0 is not None:
        if v2t:
            raise SystemExit("search: --prefilter narrows the t2v TVG ranking (--direction t2v): v2t has no prefilter of the videos.  Its captions are narrowed by "
                             "--caption_prefilter K0")
        if args.candidates != "tvg":
            raise SystemExit("search: --prefilter narrows the gallery before --candidates tvg ranks it (give --candidates tvg)")
        if K0 < 1 or K0 < shortlist_k(args):
            raise SystemExit(f"search: --prefilter must be at least --shortlist ({shortlist_k(args)}): the shortlist is taken from the videos it keeps")
    if getattr(args, "within_ids", None) is not None:
        if v2t:
            raise SystemExit("search: --within_ids confines the t2v shortlist to a set of videos (--direction t2v): a set of captions for v2t is not built")
        if serve:
            raise SystemExit("search: --within_ids applies to the one-shot queries; a --serve request carries its own set (\"within\" / \"within_idx\")")
        if args.candidates != "tvg":
            raise SystemExit("search: --within_ids confines the shortlist --candidates tvg takes (give --candidates tvg)")
    K0 = args.caption_prefilter
    if K0 is not None:
        if not v2t:
            raise SystemExit("search: --caption_prefilter narrows the captions a query video ranks (--direction v2t): t2v narrows its videos with --prefilter")
        if args.candidates != "tvg":
            raise SystemExit("search: --caption_prefilter narrows the captions before --candidates tvg ranks them (give --candidates tvg)")
        if K0 < 1 or K0 < shortlist_k(args):
            raise SystemExit(f"search: --caption_prefilter must be at least --shortlist ({shortlist_k(args)}): the shortlist is taken from the captions it keeps")
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
    tower_path, tower_seed = args.vision_model_path, args.vision_synthetic
    if tower_path is not None and tower_seed is not None:
        raise SystemExit("search: give --vision_model_path or --vision_synthetic, not both (the tower has one set of weights)")
    takes_frames = serve or (v2t and any(is_frame_stack(f) for f in (args.query_video or [])))
    if (tower_path is not None or tower_seed is not None) and not takes_frames:
        raise SystemExit("search: --vision_model_path / --vision_synthetic load the vision tower for raw frames: they act under --serve (add_video frames) and with a "
                         "--query_video FILE ending in .npy (--direction v2t)")


def is_frame_stack(path) -> bool:
    """--query_video: a FILE ending in .npy is a stack of raw frames, anything else a feature file."""
    return isinstance(path, str) and path.endswith(".npy")


def load_frame_stack(path, num_frames: int):
    """A video's raw frames (a .npy of uint8 [n, H, W, 3], n >= 1, read with allow_pickle=False) -> uint8 [num_frames, H, W, 3], sampled by blim_amd.extract's
    rule for frame stacks.  ValueError when the file cannot be read as one."""
    import numpy as np

    from .extract import sample_stack
    if not isinstance(path, str) or not path:
        raise ValueError("frames must be the path of a .npy frame stack")
    try:
        a = np.load(path, allow_pickle=False)
    except (OSError, ValueError, EOFError) as e:
        raise ValueError(f"cannot read the frame stack {path!r} ({type(e).__name__})") from None
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise ValueError(f"the frame stack {path!r} does not hold one uint8 array")
    if a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"the frame stack {path!r} has shape {tuple(a.shape)}: rank 4 with 3 channels, [n, H, W, 3], is needed")
    if a.shape[0] < 1 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"the frame stack {path!r} holds no frame (shape {tuple(a.shape)})")
    return np.ascontiguousarray(sample_stack(a, num_frames))


class FrameFeaturiser:
    """Raw frames -> the feature tensor blim_amd.extract would have written for them: the vision tower, created at the first call
    (`--vision_synthetic SEED`: seeded weights; else the checkpoint at `--vision_model_path`, default `--model_path`), with the resize and the normalisation
    on the GPU (VisionEncoder.video_feature_u8).  fp16, as the extractor's default: the features equal an extracted file's bit for bit.  ValueError when the
    tower cannot be loaded or refuses the frames."""

    def __init__(self, args, dims=None):
        from .vision import VisionDims
        self.args, self.dims, self.enc = args, dims or VisionDims(), None
        self.num_frames = int(args.num_clips) * self.dims.num_frames          # 16: the frames a video is sampled to

    def __call__(self, frames_u8):
        if self.enc is None:
            import pickle

            from .vision import VisionEncoder
            enc = None
            try:
                enc = VisionEncoder(self.dims, dtype="f16")
                seed = self.args.vision_synthetic
                if seed is not None:
                    enc.init_synthetic_weights(seed)
                else:
                    enc.load_checkpoint(self.args.vision_model_path or self.args.model_path)
            except (RuntimeError, OSError, KeyError, ValueError, ImportError, EOFError, pickle.UnpicklingError) as e:      # (engine.BlimError is a RuntimeError)
                if enc is not None:
                    enc.close()
                raise ValueError(f"the vision tower cannot be loaded ({type(e).__name__}: {e})") from None
            self.enc = enc
        return self.enc.video_feature_u8(frames_u8)

    def close(self):
        if self.enc is not None:
            self.enc.close()
            self.enc = None


def load_video_features(path):
    """A video's feature file (blim_amd.extract's output: one tensor [num_clips, tokens, width]) -> the tensor, on the host.  ValueError when it cannot be read as one."""
    import pickle

    import torch
    if not isinstance(path, str) or not path:
        raise ValueError("features must be the path of a feature file")
    try:
        t = torch.load(path, map_location="cpu", weights_only=True)
    except (OSError, RuntimeError, ValueError, EOFError, pickle.UnpicklingError) as e:
        raise ValueError(f"cannot read the feature file {path!r} ({type(e).__name__})") from None
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise ValueError(f"the feature file {path!r} does not hold one floating-point tensor")
    return t


def query_video_features(files, args, featuriser=None):
    """--query_video: each FILE's feature tensor -- read from a feature file, or computed from a .npy frame stack by the vision tower (one tower for the run,
    created only when a frame stack is there, closed before the indexes are built).  ValueError as load_video_features / load_frame_stack / FrameFeaturiser."""
    own = None
    try:
        feats = []
        for f in files:
            if is_frame_stack(f):
                if featuriser is None:
                    featuriser = own = FrameFeaturiser(args)
                feats.append(featuriser(load_frame_stack(f, getattr(featuriser, "num_frames", None) or 16)))
            else:
                feats.append(load_video_features(f))
        return feats
    finally:
        if own is not None:
            own.close()


def default_candidates(mode: str, row, n: int, k: int, live=None):
    """The candidates of a query that names none, under `--candidates iv2 | all` -> (candidate indices, their first-stage scores or None).  row: the query's
    first-stage row, or None for a query that has none (free text, raw rows, a video outside the dataset): then `all` has no first-stage term, and `iv2` is the
    caller's refusal.  iv2: the stable top-k of the row.  all: the whole gallery of n, the row padded with zeros for the entries that joined at run time.
    live (bool [n]): the videos that are left -- `all` is those, `iv2` the top-k of the row among them."""
    import numpy as np
    if row is not None:
        row = np.asarray(row, dtype=np.float32)
    if live is not None:
        live = np.asarray(live, dtype=bool).reshape(-1)
    if mode == "iv2":
        order = np.argsort(-row, kind="stable")
        if live is not None:
            order = order[live[order]]
        cand = order[:min(k, n)]
    else:
        cand = np.arange(n) if live is None else np.nonzero(live)[0]
        if row is not None:
            row = np.concatenate([row, np.zeros(max(n - len(row), 0), np.float32)])
    return cand, None if row is None else row[cand]


def answer_line(query: str, ranked_as: str, ranked, scores, shortlisted=None, prefiltered=None, head=None, within=None) -> str:
    """One stdout answer: {**head (serve: the request's id), "query", ranked_as ("videos" | "texts"): the ranked ids, "scores", then "shortlisted": K and
    "prefiltered": K0 where the candidates came from the shortlist / through the prefilter, and "within": M, the size of the set the request was confined to}."""
    more = {} if shortlisted is None else {"shortlisted": shortlisted}
    if prefiltered is not None:
        more["prefiltered"] = prefiltered
    if within is not None:
        more["within"] = int(within)
    return json.dumps({**(head or {}), "query": query, ranked_as: list(ranked), "scores": [float(x) for x in scores], **more})


def video_index_of(vids) -> dict:
    """The id map, stated once: {str(id): video index}; an id that appears twice names its first video."""
    at = {}
    for j, v in enumerate(vids):
        at.setdefault(str(v), j)
    return at


class BadRequest(ValueError):
    """A request that gets an error line; the process goes on."""


class Server:
    """`--serve`: turns request lines into rerank requests of one GalleryIndex and the results into answer lines.  A request is validated in full -- its JSON, its
    query (a `text` / `rows` query joins the scorer through PairScorer.add_texts, with its checks), its candidates -- before it enters a batch, so a bad request
    cannot fail the pass its neighbours are scored in.  Identical `text` / `rows` queries share the text index of the first one (a dict from row bytes to index)."""

    def __init__(self, gal, vids, n_captions: int, t2v_iv2, args, finetuned: bool = False, build_rows=None, content_hash=None, featuriser=None):
        import numpy as np
        self.np = np
        self.gal, self.s = gal, gal.s
        self.vids = [v for v in vids]
        self.vid_at = video_index_of(self.vids)
        self.n_captions, self.t2v_iv2, self.args, self.finetuned, self.build_rows = int(n_captions), t2v_iv2, args, bool(finetuned), build_rows
        self.n_vid = np.array([int(np.prod(v.shape[-3:-1])) for v in self.s.video], dtype=np.int64)      # video tokens of each prefix, as the planner counts them
        self.text_of = {}                          # row bytes -> text index
        self.content_hash = content_hash           # feature tensor -> a digest of its content (engine.hash_device on the device copy), or None: contents are not compared
        self.content_of = {}                       # digest -> the id of the run-time video that has this content
        self.featuriser = featuriser               # raw frames uint8 [num_frames, H, W, 3] -> the video's feature tensor (FrameFeaturiser), or None: `frames` is refused
        self.requests = self.batches = self.errors = self.texts_added = self.videos_added = self.videos_removed = 0
        self.removed_ids = set()                   # ids that left and have not joined again: a second removal is refused by name

    # ---- one request
    def _rows(self, req):
        """-> ((vtg ids, labels), (tvg ids, labels) or None) of a `text` / `rows` request."""
        np = self.np
        if "text" in req:
            if self.build_rows is None:
                raise BadRequest("a text query needs the dataset's tokenizer (not --synthetic): send rows")
            if not isinstance(req["text"], str):
                raise BadRequest("text must be a string")
            return self.build_rows(req["text"])
        rows = req["rows"]
        if not isinstance(rows, dict) or "vtg_ids" not in rows or "vtg_labels" not in rows or ("tvg_ids" in rows) != ("tvg_labels" in rows):
            raise BadRequest("rows takes vtg_ids and vtg_labels, and tvg_ids with tvg_labels or neither")
        try:
            get = lambda k: np.asarray(rows[k], dtype=np.int64).reshape(-1) if len(rows[k]) else np.zeros(0, np.int64)
            return (get("vtg_ids"), get("vtg_labels")), ((get("tvg_ids"), get("tvg_labels")) if "tvg_ids" in rows else None)
        except (TypeError, ValueError, OverflowError):
            raise BadRequest("rows must hold lists of integers") from None

    def _text(self, req):
        """-> (text index, the answer's `query` field)."""
        kinds = [k for k in ("caption", "text", "rows") if k in req]
        if len(kinds) != 1:
            raise BadRequest("give exactly one of caption, text, rows")
        if kinds[0] == "caption":
            i = req["caption"]
            if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < self.n_captions:
                raise BadRequest(f"caption must be an index in 0 .. {self.n_captions - 1}")
            return i, f"caption:{i}"
        vtg_row, tvg_row = self._rows(req)
        key = tuple(self.np.asarray(a).astype(self.np.int64).tobytes() for r in (vtg_row, tvg_row) if r is not None for a in r)
        t = self.text_of.get(key)
        if t is None:
            try:
                t = int(self.s.add_texts([vtg_row], None if tvg_row is None else [tvg_row])[0])
            except ValueError as e:
                raise BadRequest(str(e)) from None
            self.text_of[key] = t
            self.texts_added += 1
        return t, (f"query:{req['text']}" if "text" in req else f"rows:{t}")

    def _refuse_removed(self, idx) -> None:
        """Names the first removed index in the request's own order (PairScorer._need_live names the lowest)."""
        removed = self.s.removed
        gone = [int(j) for j in idx if int(j) in removed]
        if gone:
            raise BadRequest(f"video {gone[0]} was removed")

    def _named(self, req, ids_key: str, idx_key: str, word: str, opens: str = ""):
        """The id-list rule, stated once: req[ids_key] (video ids as printed in `videos`) or req[idx_key] (indices) -> video indices in the request's order, a
        list.  An unknown id, an index that is no integer of 0 .. N - 1, a removed index and a video named twice are refused; `word` names the list in the
        messages and `opens` opens the unknown-id one."""
        given = req.get(ids_key, req.get(idx_key))
        if ids_key in req:
            unknown = [v for v in given if str(v) not in self.vid_at]
            if unknown:
                raise BadRequest(f"{opens}unknown video id {unknown[0]!r}")
            idx = [self.vid_at[str(v)] for v in given]
        else:
            N = len(self.vids)
            if any(isinstance(j, bool) or not isinstance(j, int) or not 0 <= j < N for j in given):
                raise BadRequest(f"{idx_key} must hold indices in 0 .. {N - 1}")
            self._refuse_removed(given)
            idx = given
        if len(set(idx)) != len(idx):
            raise BadRequest(f"the {word} list names a video twice")
        return idx

    def _candidates(self, req, t: int, is_caption: bool):
        """-> (candidate video indices, first-stage scores or None, None), or (None, None, K): the candidates are the best K of the gallery's TVG ranking."""
        np = self.np
        N = len(self.vids)
        fs = None
        if "shortlist" in req:
            K = req["shortlist"]
            if "candidates" in req or "candidate_idx" in req:
                raise BadRequest("shortlist ranks the whole gallery: give shortlist or candidates / candidate_idx, not both")
            if isinstance(K, bool) or not isinstance(K, int):
                raise BadRequest("shortlist must be a positive integer")
            return self._shortlisted(req, t, K)
        if "candidates" in req and "candidate_idx" in req:
            raise BadRequest("give candidates (video ids) or candidate_idx (indices), not both")
        if "candidates" in req or "candidate_idx" in req:
            given = req.get("candidates", req.get("candidate_idx"))
            if not isinstance(given, list) or not given:
                raise BadRequest("the candidate list is empty")
            cand = np.asarray(self._named(req, "candidates", "candidate_idx", "candidate"), dtype=np.int64)
        elif self.args.candidates == "tvg":
            return self._shortlisted(req, t, shortlist_k(self.args))
        else:
            row = self.t2v_iv2[t] if self.t2v_iv2 is not None and is_caption else None
            if row is None and self.args.candidates == "iv2":
                raise BadRequest("a text / rows query has no first-stage row (--candidates iv2): send candidates")
            cand, fs = default_candidates(self.args.candidates, row, N, self.args.topk, live=self.s.live)
        if "first_stage" in req:
            try:
                fs = np.asarray(req["first_stage"], dtype=np.float32).reshape(-1)
            except (TypeError, ValueError):
                raise BadRequest("first_stage must hold numbers") from None
            if len(fs) != len(cand) or not np.all(np.isfinite(fs)):
                raise BadRequest("first_stage must hold one finite number per candidate")
        return cand, fs, None

    def _shortlisted(self, req, t: int, K: int):
        """A request whose candidates are the best K videos of the gallery's TVG ranking (GalleryIndex.search_requests): what that needs, checked here."""
        if not self.finetuned:
            raise BadRequest("a shortlist ranks the gallery by the TVG likelihood of a fine-tuned checkpoint (--resume): this model has none")
        if self.s.tvg_split[t] is None:
            raise BadRequest("a shortlist needs the query's TVG row (rows without tvg_ids / tvg_labels have none)")
        if "first_stage" in req:
            raise BadRequest("first_stage is parallel to the candidates: a shortlist request names none")
        return None, None, int(K)

    def _within(self, req, shortlist):
        """-> the set of a request that carries `"within"` (video ids) or `"within_idx"` (indices), as ascending video indices; None: it carries neither."""
        np = self.np
        if "within" not in req and "within_idx" not in req:
            return None
        if "within" in req and "within_idx" in req:
            raise BadRequest("give within (video ids) or within_idx (indices), one form of the set")
        other = [k for k in ("candidates", "candidate_idx", "first_stage") if k in req]
        if other:
            raise BadRequest(f"within confines a shortlist to a set of videos: a request with {other[0]} names its own candidates and takes no within")
        if shortlist is None:
            raise BadRequest("within confines a shortlist: give shortlist (or run --candidates tvg)")
        given = req.get("within", req.get("within_idx"))
        if not isinstance(given, list):
            raise BadRequest("within / within_idx must be a list")
        if not given:
            raise BadRequest("the within list is empty")
        if "within" in req and any(isinstance(v, (dict, list)) for v in given):
            raise BadRequest("within must hold video ids")
        return np.sort(np.asarray(self._named(req, "within", "within_idx", "within", opens="within: "), dtype=np.int64))

    def _prefilter(self, req, shortlist, n_videos=None):
        """-> the K0 of a shortlisted request: its own `"prefilter"`, else --prefilter for a request that takes the default K; None: not prefiltered.  The
        shortlist's K and this K0 are held to gallery.check_shortlist here, before the request enters a batch."""
        from .gallery import check_shortlist
        K0 = self.args.prefilter if "shortlist" not in req else None
        if "prefilter" in req:
            K0 = req["prefilter"]
            if isinstance(K0, bool) or not isinstance(K0, int):
                raise BadRequest("prefilter must be a positive integer")
            if shortlist is None:
                raise BadRequest("prefilter narrows a shortlist: give shortlist (or run --candidates tvg), not candidates / candidate_idx")
        if shortlist is None:
            return None
        try:
            check_shortlist(shortlist, K0, (len(self.vids) - len(self.s.removed)) if n_videos is None else n_videos)
        except ValueError as e:
            raise BadRequest(str(e)) from None
        return K0

    def parse(self, line: str):
        """One request line -> a dict(id, query, text, cand, fs, topk, shortlist: K with cand None, or None); BadRequest (with .id, as far as it was read) for a request that gets an error line."""
        rid = None
        try:
            try:
                req = json.loads(line)
            except ValueError:
                raise BadRequest("malformed JSON") from None
            if not isinstance(req, dict):
                raise BadRequest("a request is a JSON object")
            rid = req.get("id")
            if isinstance(rid, (dict, list)):
                rid = None
                raise BadRequest("id must be a JSON scalar")
            if "add_video" in req:
                return self._add_request(rid, req)
            if "remove_video" in req:
                return self._remove_request(rid, req)
            topk = req.get("topk")
            if topk is not None and (isinstance(topk, bool) or not isinstance(topk, int) or topk < 1):
                raise BadRequest("topk must be a positive integer")
            t, name = self._text(req)
            cand, fs, shortlist = self._candidates(req, t, "caption" in req)
            within = self._within(req, shortlist)
            prefilter = self._prefilter(req, shortlist, None if within is None else len(within))
            pre, post, resp = self.s.vtg_split[t]
            limit = getattr(self.s, "max_row_len", None)
            seen = within if within is not None else cand                   # the videos the request may rerank
            if limit is not None and len(pre) + int((self.n_vid if seen is None else self.n_vid[seen]).max()) + len(post) >= limit:
                raise BadRequest(f"tokenizer_model_max_length = {limit} leaves no response token of this query after a candidate's video tokens")
            if self.finetuned and self.args.c[0] < 1 and self.s.tvg_split[t] is None:
                raise BadRequest("a fine-tuned blend with c0 < 1 needs the query's TVG row (rows without tvg_ids / tvg_labels have none)")
            more = {} if within is None else {"within": within}             # (a request without the field: the dict it always was)
            return {"id": rid, "query": name, "text": t, "cand": cand, "fs": fs, "topk": topk, "shortlist": shortlist, "prefilter": prefilter, **more}
        except BadRequest as e:
            e.id = rid
            raise

    QUERY_KEYS = ("caption", "text", "rows", "candidates", "candidate_idx", "first_stage", "shortlist", "prefilter", "topk", "within", "within_idx")

    # ---- a video that joins
    def _add_request(self, rid, req):
        """`{"id", "add_video": {"vid", "features" | "frames"}}`, validated in full before anything changes -> dict(id, add: (vid, tensor, digest)).  `frames` (a
        .npy stack of raw frames) goes through the vision tower first and is a `features` request from there on."""
        if any(k in req for k in self.QUERY_KEYS + ("remove_video",)):
            raise BadRequest("an add_video request carries no query")
        a = req["add_video"]
        if not isinstance(a, dict) or set(a) not in ({"vid", "features"}, {"vid", "frames"}):
            raise BadRequest("add_video takes vid (the new video's id) and features (the path of its feature file)")
        vid = a["vid"]
        if isinstance(vid, (bool, dict, list)) or vid is None or str(vid) == "":
            raise BadRequest("vid must be a non-empty string or a number")
        if str(vid) in self.vid_at:
            raise BadRequest(f"video id {vid!r} is already in the gallery")
        try:
            if "frames" in a:
                if self.featuriser is None:
                    raise ValueError("this server has no vision tower for raw frames: send features")
                feat = self.featuriser(load_frame_stack(a["frames"], getattr(self.featuriser, "num_frames", None) or 16))
            else:
                feat = load_video_features(a["features"])
            self.s.check_videos([feat])
        except ValueError as e:
            raise BadRequest(str(e)) from None
        digest = None
        if self.content_hash is not None:
            digest = self.content_hash(feat)
            if digest in self.content_of:
                raise BadRequest(f"these features are those of video {self.content_of[digest]!r}, added earlier")
        return {"id": rid, "add": (vid, feat, digest)}

    def _add(self, item, write) -> None:
        """The video joins: the scorer (its vocabulary registered again), the id map; the index follows before its next pass (GalleryIndex._sync_videos)."""
        vid, feat, digest = item["add"]
        try:
            j = int(self.s.add_videos([feat])[0])
        except ValueError as e:                    # (parse checked it already: what it did not foresee)
            self.errors += 1
            write(json.dumps({"id": item["id"], "error": str(e)}))
            return
        self.vids.append(vid if isinstance(vid, str) else str(vid))
        self.vid_at[str(vid)] = j
        self.removed_ids.discard(str(vid))
        self.n_vid = self.np.append(self.n_vid, int(self.np.prod(feat.shape[-3:-1])))
        if digest is not None:
            self.content_of[digest] = self.vids[-1]
        self.videos_added += 1
        write(json.dumps({"id": item["id"], "added": self.vids[-1], "index": j, "videos": int(self.s.n_live)}))      # (the videos the gallery holds: the index space less the removed ones)

    # ---- a video that leaves
    def _remove_request(self, rid, req):
        """`{"id", "remove_video": VID}`, validated in full before anything changes -> dict(id, remove: (VID as the gallery names it, its index))."""
        if any(k in req for k in self.QUERY_KEYS):
            raise BadRequest("a remove_video request carries no query")
        vid = req["remove_video"]
        if isinstance(vid, (bool, dict, list)) or vid is None or str(vid) == "":
            raise BadRequest("remove_video takes the id of a video of the gallery: a non-empty string or a number")
        key = str(vid)
        if key not in self.vid_at:
            raise BadRequest(f"video id {vid!r} was removed already" if key in self.removed_ids else f"unknown video id {vid!r}")
        if self.s.n_live <= 1:
            raise BadRequest(f"video id {vid!r} is the last video of the gallery: at least one video must remain")
        j = self.vid_at[key]
        try:
            self.s.check_removal([j])
        except ValueError as e:
            raise BadRequest(str(e)) from None
        return {"id": rid, "remove": (key, j)}

    def _remove(self, item, write) -> None:
        """The video leaves: the scorer (a tombstone; its vocabulary registered again without the entry), the id map and the content digests -- the same features
        may join again, under the same or another id, at a new index; the index follows before its next pass (_PrefixIndex._follow_removed)."""
        key, j = item["remove"]
        try:
            self.s.remove_videos([j])
        except ValueError as e:                    # (parse checked it already: what it did not foresee)
            self.errors += 1
            write(json.dumps({"id": item["id"], "error": str(e)}))
            return
        del self.vid_at[key]
        self.removed_ids.add(key)
        for j2, v in enumerate(self.vids):         # (an id that appears twice names its first video: now the next one that is left)
            if str(v) == key and j2 not in self.s.removed:
                self.vid_at[key] = j2
                self.removed_ids.discard(key)
                break
        self.n_vid[j] = 0                          # (a tombstone adds nothing to the longest prefix a request may meet)
        self.content_of = {d: v for d, v in self.content_of.items() if str(v) != key or key in self.vid_at}
        self.videos_removed += 1
        write(json.dumps({"id": item["id"], "removed": self.vids[j], "index": j, "videos": int(self.s.n_live)}))

    # ---- one batch
    def _score(self, reqs):
        from .gallery import SearchRequest
        a = self.args
        return self.gal.search_requests([SearchRequest(r["text"], r["cand"], r["fs"], r["shortlist"], r["prefilter"], within=r.get("within")) for r in reqs],
                                        cpn=a.cpn, alpha=a.alpha, c=a.c, finetuned=self.finetuned)

    def handle(self, lines, write) -> None:
        """The requests that arrived together: every good one is scored in ONE search_requests pass; one answer line per request, in arrival order.  An add_video
        request is a barrier: the requests in front of it are parsed, scored against the gallery as it is and answered, then the video joins and is answered, and only
        then are the requests behind it read -- they may name the new video, and their passes see the new gallery."""
        lines = [ln for ln in lines if ln.strip()]
        if not lines:
            return
        self.batches += 1
        items = []
        for ln in lines:
            try:
                item = self.parse(ln)
            except BadRequest as e:
                item = e
            if isinstance(item, dict) and ("add" in item or "remove" in item):
                self._answer(items, write)
                items = []
                self.requests += 1
                (self._add if "add" in item else self._remove)(item, write)
            else:
                items.append(item)
        self._answer(items, write)

    def _answer(self, items, write) -> None:
        """The parsed requests of one stretch without an add: one pass, one line each."""
        if not items:
            return
        good = [r for r in items if isinstance(r, dict)]
        if good:
            try:
                results = self._score(good)
            except ValueError as e:                # what validation did not foresee: each request alone, so that only the one at fault gets the error
                results = [BadRequest(str(e))] if len(good) == 1 else []
                for r in good if len(good) > 1 else []:
                    try:
                        results += self._score([r])
                    except ValueError as e1:
                        results.append(BadRequest(str(e1)))
            for r, res in zip(good, results):
                r["result"] = res
        self.requests += len(items)
        for r in items:
            res = r if isinstance(r, BadRequest) else r["result"]
            if isinstance(res, BadRequest):
                self.errors += 1
                write(json.dumps({"id": getattr(r, "id", None) if isinstance(r, BadRequest) else r["id"], "error": str(res)}))
                continue
            order, blended = res
            k = len(order) if r["topk"] is None else min(r["topk"], len(order))
            write(answer_line(r["query"], "videos", [self.vids[int(j)] for j in order[:k]], blended[:k], r["shortlist"], r["prefilter"], head={"id": r["id"]},
                              within=None if r.get("within") is None else len(r["within"])))

    def summary(self):
        more = {"videos_added": self.videos_added} if self.videos_added else {}             # (a stream without an add_video request: the line it always was)
        if self.videos_removed:                                                             # (likewise without a remove_video request)
            more["videos_removed"] = self.videos_removed
        return {"requests": self.requests, "batches": self.batches, "mean_batch": self.requests / self.batches if self.batches else 0.0, "errors": self.errors,
                "texts_added": self.texts_added, **more}


def serve(lines, write, server, batch_queries: int = 1, batch_wait_ms: float = 0.0):
    """The serve loop.  A reader thread moves `lines` (any iterable: stdin) into a queue; this loop takes what is waiting, up to batch_queries requests, waits at most
    batch_wait_ms for more only while fewer are there, and hands the batch to server.handle(batch, write).  Ends at the end of `lines`.  -> server.summary()."""
    import queue
    import threading
    q, eof = queue.Queue(), object()

    def reader():
        try:
            for line in lines:
                q.put(line)
        finally:
            q.put(eof)
    th = threading.Thread(target=reader, name="serve-reader", daemon=True)
    th.start()
    ended = False
    while not ended:
        item = q.get()
        if item is eof:
            break
        batch = [item]
        deadline = time.monotonic() + batch_wait_ms / 1e3
        while len(batch) < batch_queries:
            try:
                item = q.get_nowait()
            except queue.Empty:
                left = deadline - time.monotonic()
                if left <= 0:
                    break
                try:
                    item = q.get(timeout=left)
                except queue.Empty:
                    break
            if item is eof:
                ended = True
                break
            batch.append(item)
        server.handle(batch, write)
    th.join()
    return server.summary()


def build_problem(args):
    """What the run scores over -> a namespace: model (weights loaded, the TVG prefix length set), tok, vtg and tvg ([ids, labels, masks] rows of the texts: the test
    captions, then one per --query), video, vocab, vlab, vids, the first-stage matrices t2v_iv2 / v2t_iv2 (None: not loaded) and build_rows (--serve: free text ->
    its unpadded (vtg, tvg) rows; None under --synthetic, which has no tokenizer)."""
    import os
    import types

    import numpy as np
    import torch

    from . import synth
    from .modeling import BlimModel
    T = torch.from_numpy
    p = types.SimpleNamespace(build_rows=None)
    if args.synthetic > 0:
        dims = synth.ModelDims(num_clips=args.num_clips) if args.synthetic_7b else synth.ModelDims(
            vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64, num_clips=args.num_clips)
        p.model = BlimModel(dims, dtype=args.dtype)
        p.model.engine.init_synthetic_weights(0)
        prob = synth.make_problem(1, args.synthetic, dims, tok_per_clip=64 if args.synthetic_7b else 8, fast_video=args.synthetic > 256)
        p.tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
        p.vtg = [[T(r) for r in x] for x in (prob.vtg_ids, prob.vtg_labels, prob.vtg_masks)]
        p.tvg = [[T(r) for r in x] for x in (prob.tvg_ids, prob.tvg_labels, prob.tvg_masks)]
        p.video, p.vocab, p.vlab = [T(v) for v in prob.video], T(prob.video_vocab), T(prob.tvg_video_labels)
        p.t2v_iv2, p.v2t_iv2 = prob.t2v_sims, prob.v2t_sims
        p.vids = [str(j) for j in range(len(p.video))]
        p.model.set_tvg_prefix_length(prob.tvg_prefix_length)
        return p
    from .checkpoint import load_checkpoint
    from .dataloader import DEFAULT_IMAGE_TOKEN, TVG_PROMPT, VTG_PROMPTS, RetrievalDataset
    from .main import dims_from_config, load_tokenizer
    p.tok = load_tokenizer(args.model_path)
    dims = dims_from_config(args.model_path, args.num_clips)
    cfg_json = json.load(open(os.path.join(args.model_path, "config.json")))
    p.model = BlimModel(dims, dtype=args.dtype, tokenizer_model_max_length=cfg_json.get("tokenizer_model_max_length"))
    load_checkpoint(p.model.engine, dims, args.model_path, args.resume or None, lora_r=args.lora_r, lora_alpha=args.lora_alpha)
    args.eval = True
    ds = RetrievalDataset(args, tokenizer=p.tok, split="test")
    items = [ds[i] for i in range(len(ds))]
    p.video, p.vids = [it["video"] for it in items], [it["vid"] for it in items]
    p.vtg = [[it[k] for it in items] for k in ("vtg_ids", "vtg_labels", "vtg_masks")]
    p.tvg = [[it[k] for it in items] for k in ("tvg_ids", "tvg_labels", "tvg_masks")]
    # free text: the dataset's own prompt builder -> its (vtg, tvg) rows, (ids, labels, masks) each
    prompts = lambda q: (ds._ids_labels(f"{DEFAULT_IMAGE_TOKEN}\n{VTG_PROMPTS[ds.dataset]}", q), ds._ids_labels(f"{TVG_PROMPT}\nCaption: {q}", DEFAULT_IMAGE_TOKEN))
    for q in args.query:
        for rows, row in zip((p.vtg, p.tvg), prompts(q)):
            for column, x in zip(rows, row):
                column.append(x)
    unpad = lambda r: (np.asarray(r[0])[np.asarray(r[2]) != 0], np.asarray(r[1])[np.asarray(r[2]) != 0])
    p.build_rows = lambda q: tuple(unpad(r) for r in prompts(q))
    p.vocab, p.vlab = ds.video_vocab, torch.tensor([it["tvg_video_labels"] for it in items])
    p.model.set_tvg_prefix_length(ds.tvg_prefix_length)
    first = torch.load(f"./scores/{args.dataset.lower()}{'' if args.resume else '_zeroshot'}.pth", weights_only=True) if args.candidates == "iv2" else None
    p.t2v_iv2 = None if first is None else first["t2v"].numpy()
    p.v2t_iv2 = None if first is None else first["v2t"].numpy()
    return p


def build_scorer(args, p):
    """The command's numeric options on p.model, p's rows padded -> the PairScorer over p's videos and texts."""
    from . import retrieval_utils as RU
    from .modeling import DDPLike
    model = p.model
    for flag in NARROW_GEMMS:
        if getattr(args, flag) == "auto":
            model.engine.set_option(flag, 1)
    if model.engine.can_precise:
        model.tvg_precise = args.tvg_precise
        model.vtg_precise = None if args.vtg_precise == "none" else args.vtg_precise
        if args.second_pass:
            model.second_pass = args.second_pass
    vtg, tvg = RU.padding_ids(*p.vtg, p.tok), RU.padding_ids(*p.tvg, p.tok)
    return RU.PairScorer(DDPLike(model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], p.video, p.vocab, p.vlab, args.num_clips, max_tokens=args.max_tokens)


def build_indexes(args, scorer, p):
    """-> [("gallery", GalleryIndex)], built; under --direction v2t followed by ("text gallery", TextGalleryIndex) over the same video cache."""
    import numpy as np

    from .gallery import GalleryIndex, TextGalleryIndex
    gb = lambda x: None if x is None else int(x * 2**30)
    gal = GalleryIndex(scorer, budget_bytes=gb(args.gallery_gb), fill=args.gallery_fill, host_budget_bytes=gb(args.gallery_host_gb), spare_slots=args.gallery_spare)
    if args.direction == "t2v":
        gal.build(first_stage=None if p.t2v_iv2 is None else np.ascontiguousarray(np.asarray(p.t2v_iv2, dtype=np.float32).T))     # v2t first stage: calibration sample
        return [("gallery", gal)]
    first = None if p.v2t_iv2 is None else np.ascontiguousarray(np.asarray(p.v2t_iv2, dtype=np.float32))
    gal.build(first_stage=first)
    tg = TextGalleryIndex(scorer, budget_bytes=gb(args.text_gallery_gb), video_index=gal, fill=args.gallery_fill, host_budget_bytes=gb(args.text_gallery_host_gb))
    if args.resume:                                   # a zero-shot blend has no TVG term: no caption cache
        tg.build(first_stage=first)
    return [("gallery", gal), ("text gallery", tg)]


def gallery_banner(args, indexes, ready: float) -> str:
    """The `gallery:` stderr line, once the indexes are built: the video cache, under v2t the caption cache too."""
    gal, s = indexes[0][1], indexes[0][1].s
    narrow = ", ".join(f"{flag} {getattr(args, flag)}" for flag in NARROW_GEMMS)
    head = f"gallery: {len(s.video)} videos, fill {gal.fill}, {gal.n_slots} {'slots' if gal.fill == 'lazy' else 'cached slots'}"
    ready = f"(ready {ready:.1f}s after start)"
    if len(indexes) == 1:
        return (f"{head} of {gal.cache.bytes // max(gal.n_slots, 1) if gal.cache else 0} bytes, mode {s.vtg_mode or 'none'}, {narrow}, "
                f"built in {gal.build_seconds:.2f}s {ready}")
    tg = indexes[1][1]
    return (f"{head}, mode {s.vtg_mode or 'none'}, built in {gal.build_seconds:.2f}s; {len(s.tvg_split)} texts, {tg.n_slots} caption slots of {tg.per_slot_bytes()} bytes, "
            f"tvg mode {s.tvg_mode}, {narrow}, built in {tg.build_seconds:.2f}s {ready}")


def report_lines(indexes, serve_summary=None, shortlist_stats=None, prefilter_stats=None, within_stats=None, removed_stats=None):
    """The closing stderr lines of a run over `indexes` ([(name, index)]: "gallery", and "text gallery" under v2t), in one order: what the caches did, what their
    host tiers did (where there is one), `serve:`, `shortlist:` and `prefilter:` (where a pass of theirs ran), `within:` (where a request carried a set), `removed:` (where a video left the gallery)."""
    tier = lambda h: json.dumps(dict(h.stats.as_dict(), records=h.n_records, record_bytes=h.record_bytes))
    lines = ["; ".join(f"{name} stats: {json.dumps(ix.stats.as_dict())}" for name, ix in indexes)]
    if any(ix.host is not None for _, ix in indexes):
        lines.append("; ".join(f"{name} host tier: {tier(ix.host)}" for name, ix in indexes if ix.host is not None))
    if serve_summary is not None:
        lines.append(f"serve: {json.dumps(serve_summary)}")
    if shortlist_stats is not None and shortlist_stats["passes"]:
        lines.append(f"shortlist: {json.dumps(_shortlist_line(shortlist_stats))}")
    if prefilter_stats is not None and prefilter_stats["passes"]:
        lines.append(f"prefilter: {json.dumps(_prefilter_line(prefilter_stats))}")
    if within_stats is not None and within_stats["queries"]:
        lines.append(f"within: {json.dumps(_within_line(within_stats))}")
    if removed_stats is not None and removed_stats["videos"]:
        lines.append(f"removed: {json.dumps(_removed_line(removed_stats))}")
    return lines


def _shortlist_line(stats):
    """The `shortlist:` stderr line: queries shortlisted, stage-1 passes and the pairs those scored."""
    return {"queries": int(stats["queries"]), "stage1_passes": int(stats["passes"]), "stage1_pairs": int(stats["pairs"])}


def _prefilter_line(stats):
    """The `prefilter:` stderr line: queries prefiltered, stage-0 passes, the logits rows those ranked and the videos kept for stage 1."""
    return {"queries": int(stats["queries"]), "stage0_passes": int(stats["passes"]), "stage0_rows": int(stats["rows"]), "kept": int(stats["kept"])}


def _within_line(stats):
    """The `within:` stderr line: queries confined to a set of the caller's, and the videos those sets held."""
    return {"queries": int(stats["queries"]), "candidates": int(stats["candidates"])}


def _removed_line(stats):
    """The `removed:` stderr line: videos that left the gallery, the cache slots their prefixes gave back and the host records forgotten with them."""
    return {"videos": int(stats["videos"]), "slots_freed": int(stats["slots_freed"]), "records_forgotten": int(stats["records_forgotten"])}


def read_within_ids(path, vids):
    """--within_ids FILE, one video id per line (blank lines skipped) -> ascending video indices; SystemExit names an empty file, an unknown or a repeated id."""
    import numpy as np
    try:
        with open(path) as f:
            ids = [ln.strip() for ln in f if ln.strip()]
    except OSError as e:
        raise SystemExit(f"search: --within_ids: {e}") from None
    at = video_index_of(vids)
    if not ids:
        raise SystemExit(f"search: --within_ids {path}: an empty set of videos")
    unknown = [v for v in ids if v not in at]
    if unknown:
        raise SystemExit(f"search: --within_ids: unknown video id {unknown[0]!r}")
    idx = [at[v] for v in ids]
    if len(set(idx)) != len(idx):
        raise SystemExit(f"search: --within_ids names video {ids[[i for i, j in enumerate(idx) if j in idx[:i]][0]]!r} twice")
    return np.sort(np.asarray(idx, dtype=np.int64))


def output_writer(path):
    """-> (write(line): the line to stdout, flushed, and to the --output file when there is one; close())."""
    out = open(path, "w") if path else None

    def write(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    return write, (out.close if out else lambda: None)


def run_serve(gal, vids, t2v_iv2, args, write, lines, build_rows=None, content_hash=None):
    """--serve: the request lines answered through `write` until they end -> the counts of the `serve:` line."""
    featuriser = FrameFeaturiser(args)             # (the tower is created when the first add_video request brings frames)
    server = Server(gal, vids, len(gal.s.vtg_split), t2v_iv2, args, finetuned=bool(args.resume), build_rows=build_rows, content_hash=content_hash, featuriser=featuriser)
    summary = serve(lines, write, server, args.batch_queries, args.batch_wait_ms)
    if server.videos_removed:                      # (a removal no pass came after: the index follows it now, so that the `removed:` line counts it)
        gal._follow_removed()
    featuriser.close()
    return summary


def run_t2v(gal, vids, t2v_iv2, args, write, within=None) -> None:
    """The one-shot text queries (--query_ids, then one text per --query at the end of the scorer's texts), one answer line each.  within (--within_ids): the
    video indices every query's shortlist is confined to."""
    from .gallery import SearchRequest
    n_texts, N = len(gal.s.vtg_split), len(vids)
    n_ds = n_texts - len(args.query)
    names = [f"caption:{i}" for i in args.query_ids] + [f"query:{q}" for q in args.query]
    blend = dict(cpn=args.cpn, alpha=args.alpha, c=args.c, finetuned=bool(args.resume))
    for t, name in zip(list(args.query_ids) + list(range(n_ds, n_texts)), names):
        K = K0 = None
        if args.candidates == "tvg":              # the gallery ranked by the TVG candidate term, the best K reranked; the answer is the best --topk of those
            K, K0 = shortlist_k(args), args.prefilter
            (order, blended), = gal.search_requests([SearchRequest(t, shortlist=K, prefilter=K0, within=within)], **blend)
            order, blended = order[:min(args.topk, N)], blended[:min(args.topk, N)]
        else:
            cand, fs = default_candidates(args.candidates, t2v_iv2[t] if t2v_iv2 is not None and t < n_ds else None, N, args.topk)
            order, blended = (x[0] for x in gal.rerank([t], cand[None], first_stage=None if fs is None else fs[None], **blend))
        write(answer_line(name, "videos", [vids[int(j)] for j in order], blended, K, K0, within=None if within is None else len(within)))


def run_v2t(tg, vids, v2t_iv2, args, write):
    """The one-shot video queries (--video_ids) over the captions: the VTG leg from the video cache, the fine-tuned TVG leg from the caption-prompt cache; one
    answer line each -> the shortlist's counts, as GalleryIndex.shortlist_stats keeps them."""
    n_texts = len(tg.s.tvg_split)
    k = min(args.topk, n_texts)
    blend = dict(cpn=args.cpn, alpha=args.alpha, c=args.c)
    shortlisted = {"queries": 0, "passes": 0, "pairs": 0}
    K0 = getattr(args, "caption_prefilter", None)
    narrow = {} if K0 is None else {"prefilter": K0}    # (section 22: stage 1 runs over the K0 captions the cached clip-0 rows rank first)
    for v in args.video_ids:
        K = None
        if args.candidates == "tvg":              # the captions ranked by the query likelihood over the cached prompts, the best K reranked
            K = shortlist_k(args)
            order, blended = (x[0, :k] for x in tg.rerank_shortlist([v], K, **blend, **narrow))
            shortlisted = {"queries": shortlisted["queries"] + 1, "passes": shortlisted["passes"] + 1,
                           "pairs": shortlisted["pairs"] + (n_texts if K0 is None else min(K0, n_texts))}
        else:                                     # (--query_video: no first-stage row)
            cand, fs = default_candidates(args.candidates, v2t_iv2[v] if v2t_iv2 is not None and v < len(v2t_iv2) else None, n_texts, args.topk)
            order, blended = (x[0] for x in tg.rerank([v], cand[None], first_stage=None if fs is None else fs[None], finetuned=bool(args.resume), **blend))
        write(answer_line(f"video:{vids[v]}", "texts", [int(i) for i in order], blended, K, K0 if K is not None else None))
    return shortlisted


def main(args):
    import os

    import torch                                  # noqa: F401  (with the package's modules, loaded before the clock starts: `ready ...s after start` counts the work)

    from . import gallery, modeling, retrieval_utils, synth      # noqa: F401

    check_args(args, int(os.environ.get("WORLD_SIZE", "1")))
    t0 = time.time()
    p = build_problem(args)
    # --within_ids names videos of the dataset (t2v, one-shot: check_args): a bad file ends the run here, before the scorer and the gallery are built
    within = None if getattr(args, "within_ids", None) is None else read_within_ids(args.within_ids, p.vids)
    scorer = build_scorer(args, p)
    vids, n_dataset, v2t = p.vids, len(p.video), args.direction == "v2t"
    if args.query_video:                          # v2t: videos outside the dataset join the scorer before the indexes are built; they share one vocabulary
        try:
            scorer.add_videos(query_video_features(args.query_video, args))
        except ValueError as e:
            raise SystemExit(f"search: --query_video: {e}") from None
        vids = list(vids) + [os.path.basename(f) for f in args.query_video]
    indexes = build_indexes(args, scorer, p)
    gal = indexes[0][1]
    print(gallery_banner(args, indexes, time.time() - t0), file=sys.stderr, flush=True)
    if v2t:
        args.video_ids = list(args.video_ids) + list(range(n_dataset, len(vids)))
        bad = [v for v in args.video_ids if not 0 <= v < len(vids)]
        if bad:
            raise SystemExit(f"search: --video_ids {bad} outside 0 .. {len(vids) - 1}")
    write, close_output = output_writer(args.output)
    summary, shortlisted, prefiltered = None, gal.shortlist_stats, gal.prefilter_stats
    if args.serve:
        from .engine import hash_device
        content_hash = lambda feat: hash_device(feat.contiguous().to(p.model.device))      # (one upload and one pass over a feature tensor: a fraction of the projection that follows)
        summary = run_serve(gal, vids, p.t2v_iv2, args, write, sys.stdin, p.build_rows, content_hash)
    elif v2t:
        shortlisted, prefiltered = run_v2t(indexes[1][1], vids, p.v2t_iv2, args, write), getattr(indexes[1][1], "prefilter_stats", None)
    else:
        run_t2v(gal, vids, p.t2v_iv2, args, write, within)
    close_output()
    for line in report_lines(indexes, summary, shortlisted, prefiltered, getattr(gal, "within_stats", None), getattr(gal, "removed_stats", None)):
        print(line, file=sys.stderr, flush=True)
    for _, ix in reversed(indexes):
        ix.close()
    p.model.engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(get_args_parser().parse_args()))

