"""`PairScorer` -- the fused scoring path `retrieval_utils.evaluation` runs by default -- and its planner (split out of retrieval_utils.py in round 6, VERDICT r5 item 7;
retrieval_utils re-exports every name).

A likelihood is a function of the (video, text) pair only, so pairs from many queries are packed into large token batches; tokens that are identical for every
candidate of a query (the video + prompt prefix for VTG, the caption prompt for TVG) are computed once and their K/V reused (SURVEY.md section 7 "prefix-KV reuse");
hidden states that no score reads (tail tokens) are not computed; priors that do not depend on the query (v2t VTG-CPN) are computed once per
candidate.  Replaces the per-query / per-batch loops of /root/reference/retrieval_utils.py:48-153 (which `retrieval_utils.compute_*_scores_x` keep literally).
"""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import distributed as dist_utils
from .calibration import TVG_MODES, VTG_MODES, VTG_SPLIT_MODES, CalibrationMixin
from .engine import PackedBatch
from .synth import IGNORE_INDEX, IMAGE_TOKEN_INDEX

SEG_MAX = 256            # bound of a merged TVG sequence (PairScorer._plan_tvg: own-segment tiles below a query's segment are computed and masked)


def _clip_major_vocab(video_vocab, device, dtype):
    """[N, clips, M] -> 16-bit [clips, N, M] on device (layout blim_tvg_* expects)."""
    return video_vocab.to(device=device, dtype=dtype).permute(1, 0, 2).contiguous()


@dataclass
class Plan:
    """One engine call: packed batch + row bookkeeping, all device-resident."""
    kind: str                  # "vtg" | "tvg" | "tvg_first"
    batch: PackedBatch
    src_index: object          # int32 [n_tokens]  (assemble input)
    feats: object              # bf16 [n_feat_rows, H]
    rows: object               # int32
    labels: object             # int32 (vtg: [n_rows] token ids; tvg: [n_pairs] video labels)
    row_start: Optional[object]
    n_pairs: int
    out_index: np.ndarray      # host: which requested pair each scored pair answers (many-to-one allowed)
    n_tokens: int
    n_rows: int
    pfx_slot: Optional[object] = None            # planned over a prefix source (blim_amd/prefix_index.py): device int32 per sequence, the cache slot of its prefix (-1: in the batch)
    slots_used: Optional[np.ndarray] = None      # ... host int32: every slot the call reads
    admits: Optional[np.ndarray] = None          # ... host int32 [n, 5] = (seq, slot, start, len, row): in-batch prefixes the call also captures into slots (a source with `admit`)
    prefix_tokens: int = 0                       # ... of n_tokens, those of in-batch prefix sequences
    prior_rows: Optional[object] = None          # kind "tvg_first": device int32, the prior sequences' scored tokens (None without cpn); `labels` is then each row's prior row


def _split_prompt_response(ids: np.ndarray, labels: np.ndarray):
    """ids/labels of one row (left pad stripped) -> (prompt ids, response ids) with labels == -100 on the prompt."""
    resp = labels != IGNORE_INDEX
    n_prompt = int(np.argmax(resp)) if resp.any() else len(ids)
    assert resp[n_prompt:].all(), "response must be one trailing span"
    return ids[:n_prompt], ids[n_prompt:]


def _select_factors(layer_bits):
    """`--vtg_precise select`: the mean compensation factor (1 plain, 2 compensated) of the QKV, o_proj, gate|up and down GEMMs over the layers of a mask."""
    b = np.asarray(layer_bits, dtype=np.int64).reshape(-1)
    return tuple(1.0 + float(np.mean((b >> k) & 1)) for k in range(4))


def executed_flops(dims, n_tokens: int, n_rows: int, kind: str, mode=None, n_vocab: int = 0, prune: bool = True, layer_bits=None) -> float:
    """GEMM FLOPs one engine call EXECUTES (the per-token constants applied to the token counts actually launched; attention,
    < 1 - 3 %, excluded): decoder layers over n_tokens packed tokens + the head over n_rows scored rows.  `mode`: compensation of the call (None: plain;
    "attn": QKV, o_proj and the head take hi + lo inputs; "full": every GEMM -- a TVG call of a 16-bit engine runs in one of the last two, TVG_MODES; a VTG
    call plain, "full" or "select", VTG_MODES).  prune: the last layer's o_proj / MLP run on the scored rows only (engine option prune_last) when they are < 15/16 of
    the tokens.  "select" with its per-layer mask `layer_bits`: each GEMM class at its mean factor over the layers, the head compensated."""
    H, I = dims.hidden_size, dims.intermediate_size
    q = 2.0 * H * (dims.num_heads + 2 * dims.num_kv_heads) * dims.head_dim
    o, gu, d = 2.0 * H * H, 4.0 * H * I, 2.0 * H * I
    fq = fo = 2.0 if mode in ("attn", "full") else 1.0      # "attn" (TVG calls only): the attention branch and the scored rows compensated, the MLP branch plain
    fg = fd = 2.0 if mode == "full" else 1.0
    if mode == "select":
        fq, fo, fg, fd = _select_factors(layer_bits if layer_bits is not None else [15] * dims.num_layers)
    per_tok = fq * q + fo * o + fg * gu + fd * d
    total = dims.num_layers * per_tok * n_tokens
    if prune and n_rows <= n_tokens - n_tokens // 16:
        total -= (fo * o + fg * gu + fd * d) * (n_tokens - n_rows)
    if kind == "vtg":
        total += (2.0 if mode == "select" else fo) * 2.0 * H * dims.vocab_size * n_rows
    else:
        # the visual head and the product with the video vocabulary: three-term compensated products (one GEMM of depth 3 K each) on a compensated call
        total += (3.0 if fo == 2.0 else 1.0) * (2.0 * H * dims.mm_hidden_size + 2.0 * dims.mm_hidden_size * n_vocab) * n_rows
    return total


def lo6_pass_flops(dims, n_tokens: int, n_rows: int, kind: str, mode=None, prune: bool = True, layer_bits=None) -> float:
    """The part of executed_flops() that runs on the e2m3 MFMA when the engine's option "precise_lo6" is on (fp16 engines, default): the second walk over K of the
    decoder GEMMs and of lm_head in the compensated modes (the TVG head's three-term products are 16-bit GEMMs of depth 3 K).  A roofline for such a call prices
    these flops at the fp6 peak (4x the 16-bit one) and the rest at the 16-bit one."""
    if mode not in ("attn", "full", "select"):
        return 0.0
    H, I = dims.hidden_size, dims.intermediate_size
    q = 2.0 * H * (dims.num_heads + 2 * dims.num_kv_heads) * dims.head_dim
    o, gu, d = 2.0 * H * H, 4.0 * H * I, 2.0 * H * I
    g2 = gu if mode == "full" else 0.0
    d2 = d if mode == "full" else 0.0
    if mode == "select":
        fq, fo, fg, fd = _select_factors(layer_bits if layer_bits is not None else [15] * dims.num_layers)
        q, o, g2, d2 = (fq - 1.0) * q, (fo - 1.0) * o, (fg - 1.0) * gu, (fd - 1.0) * d
    total = dims.num_layers * (q + o + g2 + d2) * n_tokens
    if prune and n_rows <= n_tokens - n_tokens // 16:
        total -= (o + g2 + d2) * (n_tokens - n_rows)
    if kind == "vtg":
        total += 2.0 * H * dims.vocab_size * n_rows
    return total


class PairScorer(CalibrationMixin):
    """Fused scoring of arbitrary (video, text) pairs.  See the module docstring for what is shared."""
    vocab_version = 0        # (instance state, set by the constructor; here for the indexes' sake: a scorer that never grew reads as version 0)
    has_vocab = False
    _dead = frozenset()      # the indices remove_videos took out (video[j] is None there); empty for a scorer that never removed anything

    def __init__(self, model, vtg_ids, vtg_masks, vtg_labels, tvg_ids, tvg_masks, tvg_labels, video: Sequence, video_vocab,
                 tvg_video_labels, num_clips: int, max_tokens: int = 24576, precise_tvg: bool = True, feat_chunk: int = 64):
        import torch
        self.precise_tvg = bool(precise_tvg)
        eng_ = getattr(model.module if hasattr(model, "module") else model, "engine", None)
        self.split_tvg = self.precise_tvg and eng_ is not None and bool(getattr(eng_, "can_precise", False))   # TVG rows as [hi | lo]
        # VTG calls: plain 16-bit on fp16 engines; bf16 engines run them compensated too (modeling.py: vtg_precise), feature rows included --
        # with plain bf16 features the projector's 8-bit rounding alone left 1e-3 on the scores at 7B depth
        m_ = model.module if hasattr(model, "module") else model
        can = eng_ is not None and bool(getattr(eng_, "can_precise", False))
        vm = (m_.vtg_mode() if hasattr(m_, "vtg_mode") else getattr(m_, "vtg_precise", None)) if can else None
        self.vtg_mode = None if vm in ("auto", "none") else vm           # an unresolved "auto": plain until calibrate_vtg decides (evaluation() does it before the first pass)
        tm = m_.tvg_mode() if hasattr(m_, "tvg_mode") else getattr(m_, "tvg_precise", None)
        self.tvg_mode = tm if tm in TVG_MODES else "full"                # (an unresolved "auto": full until calibrate_tvg says otherwise)
        self.split_vtg = self.vtg_mode in VTG_SPLIT_MODES
        self.m = model.module if hasattr(model, "module") else model
        self.engine = self.m.engine
        self.device = self.m.device
        self.max_tokens = int(max_tokens)
        self.num_clips = int(num_clips)
        if self.num_clips != int(self.m.dims.num_clips):         # blim_score_tvg reads n_pairs * blim_config.num_clips rows
            raise ValueError(f"num_clips = {num_clips} but the engine was created with num_clips = {self.m.dims.num_clips}")
        strip = lambda ids, msk, lab: [(np.asarray(ids[i])[np.asarray(msk[i]) != 0], np.asarray(lab[i])[np.asarray(msk[i]) != 0])
                                       for i in range(len(ids))]
        vtg_rows = strip(vtg_ids, vtg_masks, vtg_labels)
        tvg_rows = strip(tvg_ids, tvg_masks, tvg_labels)
        # the videos given here and the videos that join later (add_videos) go through the same code: the list is the scorer's own, the caller's is left alone
        self.video: List = []
        self.tvg_video_labels = np.zeros(0, dtype=np.int32)
        self.vocab_cm, self.n_vocab, self._vocab_src, self._vocab_key = None, 0, None, None
        self.has_vocab = video_vocab is not None
        self.vocab_version = 0           # bumped whenever videos join: what a TVG normaliser, gallery_feats() and every memo of a TVG value were computed over
        self._join_videos(list(video), video_vocab, np.asarray(tvg_video_labels).astype(np.int32).reshape(-1))
        self.exec_flops = 0.0            # GEMM FLOPs of the engine calls run so far (executed_flops; bench.py's roofline fractions)
        self.exec_flops_lo6 = 0.0        # ... of which on the e2m3 MFMA (lo6_pass_flops: the compensated modes' second pass under the engine's "precise_lo6")
        self.exec_tokens = 0
        self._vfeat: Dict[Tuple[int, bool], object] = {}
        self._upcoming: Dict[bool, List[int]] = {}; self._upcoming_pos: Dict[bool, int] = {}
        self.feat_chunk = int(feat_chunk)
        # rows longer than config.tokenizer_model_max_length lose their tail after the splice (modeling_videochat_flash.py:452-457; None = no limit)
        self.max_row_len = getattr(self.m, "tokenizer_model_max_length", None)
        # per-text rows and splits: the texts given here and the texts that join later (add_texts) go through the same code
        self.vtg_rows, self.tvg_rows, self.vtg_split, self.tvg_split = [], [], [], []
        if len(vtg_rows) != len(tvg_rows):
            raise ValueError(f"{len(vtg_rows)} VTG rows but {len(tvg_rows)} TVG rows: one of each per text")
        self.add_texts(vtg_rows, tvg_rows)

    # ---- texts
    def _text_state(self, vtg_row, tvg_row):
        """One text's unpadded (ids, labels) rows -> ((pre, post, response) of its VTG row, the caption prompt of its TVG row or None without one), checked."""
        ids, lab = vtg_row
        prompt, resp = _split_prompt_response(ids, lab)
        w = np.nonzero(prompt == IMAGE_TOKEN_INDEX)[0]
        if len(w) != 1:
            raise ValueError(f"VTG prompt must hold exactly one <image> placeholder (found {len(w)})")
        vtg = (prompt[: w[0]].astype(np.int64), prompt[w[0] + 1:].astype(np.int64), resp.astype(np.int64))
        if tvg_row is None:
            return vtg, None
        ids, lab = tvg_row
        prompt, resp = _split_prompt_response(ids, lab)
        if not (len(resp) >= 1 and resp[0] == IMAGE_TOKEN_INDEX):
            raise ValueError("TVG response must start with the <image> placeholder")
        if self.max_row_len is not None and len(ids) - 1 + self.num_clips > self.max_row_len:
            # the reference reads the clip positions relative to the <|im_end|> label of the row's tail (retrieval_utils.py:99-107); a row cut
            # inside its clip tokens or tail has no such label any more
            raise ValueError(f"TVG row of {len(ids) - 1 + self.num_clips} tokens exceeds tokenizer_model_max_length = {self.max_row_len}")
        return vtg, prompt.astype(np.int64)

    def add_texts(self, vtg_rows, tvg_rows=None) -> np.ndarray:
        """Texts that join the scorer: unpadded (ids, labels) rows, one per text; tvg_rows None: the texts have no TVG row (plan_tvg / tvg refuse them).  Every row
        is checked before any is added: a bad one raises ValueError and adds nothing.  Existing indices never move.  -> the new texts' indices."""
        as_row = lambda r: (np.asarray(r[0]), np.asarray(r[1]))
        vtg_rows = [as_row(r) for r in vtg_rows]
        tvg_rows = [None] * len(vtg_rows) if tvg_rows is None else [as_row(r) for r in tvg_rows]
        if len(tvg_rows) != len(vtg_rows):
            raise ValueError(f"add_texts: {len(vtg_rows)} VTG rows but {len(tvg_rows)} TVG rows")
        for ids, lab in [r for r in vtg_rows + tvg_rows if r is not None]:
            if ids.ndim != 1 or ids.shape != lab.shape or len(ids) == 0:
                raise ValueError(f"add_texts: a row is (ids, labels) of one length, got shapes {ids.shape} and {lab.shape}")
        try:
            states = [self._text_state(v, t) for v, t in zip(vtg_rows, tvg_rows)]
        except AssertionError as e:                                      # (_split_prompt_response: a response that is not one trailing span)
            raise ValueError(str(e)) from None
        first = len(self.vtg_split)
        self.vtg_rows += vtg_rows; self.tvg_rows += tvg_rows
        self.vtg_split += [v for v, _ in states]; self.tvg_split += [t for _, t in states]
        return np.arange(first, first + len(states), dtype=np.int64)

    # ---- videos
    def add_videos(self, videos, vocab_rows=None) -> np.ndarray:
        """Videos that join the scorer: feature tensors as the constructor takes them ([num_clips, tokens, width], what blim_amd.extract writes).
        vocab_rows [n, num_clips, mm_hidden] float32: the videos' entries of the TVG vocabulary; None: each video's clip means in float32 (dataloader.py:
        load_video_feature(v).mean(1)).  Every video is checked before any is added: a bad one raises ValueError and adds nothing.  Existing indices and vocabulary
        labels never move; the new videos take the indices len(video) .. and the labels n_vocab .., one label each.  A TVG score is a softmax over the vocabulary, so
        the vocabulary is registered again, whole, and vocab_version is bumped: gallery_feats() and every memo of a TVG value keyed by it are computed again.  A
        scorer built without a vocabulary (no TVG) refuses vocab_rows and adds the videos without an entry (label -1).  -> the new videos' indices."""
        videos, rows, labels = self.check_videos(videos, vocab_rows)
        first = len(self.video)
        self._join_videos(videos, rows, labels)
        return np.arange(first, first + len(videos), dtype=np.int64)

    def check_videos(self, videos, vocab_rows=None):
        """add_videos' checks, changing nothing: -> (the videos, their float32 vocabulary rows or None without a vocabulary, their labels); ValueError for a bad one."""
        import torch
        videos = list(videos)
        C = self.num_clips
        ref = next((v for v in self.video if v is not None), None)       # (a removed video is a tombstone: the first live one gives the shapes)
        ndim = len(ref.shape) if ref is not None else 3
        width = int(ref.shape[-1]) if ref is not None else None
        for n, v in enumerate(videos):
            shape = tuple(getattr(v, "shape", ()))
            if len(shape) != ndim or len(shape) < 3:
                raise ValueError(f"add_videos: video {n} has shape {shape}: a feature tensor of rank {ndim}, [num_clips, tokens, width]")
            if int(shape[0]) != C:
                raise ValueError(f"add_videos: video {n} has {shape[0]} clips, the scorer was built with num_clips = {C}")
            if min(shape) < 1:
                raise ValueError(f"add_videos: video {n} has an empty dimension {shape}")
            if width is not None and int(shape[-1]) != width:
                raise ValueError(f"add_videos: video {n} has feature width {shape[-1]}, the scorer's videos have {width}")
            width = int(shape[-1])
        if not self.has_vocab:
            if vocab_rows is not None:
                raise ValueError("add_videos: this scorer was built without a video vocabulary (no TVG): it takes no vocab_rows")
            rows, labels = None, np.full(len(videos), -1, dtype=np.int32)
        else:
            M = int(self._vocab_src.shape[-1])
            if vocab_rows is None:
                if videos and (ndim != 3 or width != M):
                    raise ValueError(f"add_videos: the clip-mean rule needs [num_clips, tokens, {M}] features (got rank {ndim}, width {width}): pass vocab_rows")
                rows = torch.stack([torch.as_tensor(v).float().mean(1) for v in videos]) if videos else torch.zeros((0, C, M), dtype=torch.float32)
            else:
                rows = torch.as_tensor(vocab_rows)
                if tuple(rows.shape) != (len(videos), C, M):
                    raise ValueError(f"add_videos: vocab_rows has shape {tuple(rows.shape)}, {len(videos)} videos need {(len(videos), C, M)}")
                rows = rows.to(torch.float32)
            labels = np.arange(self.n_vocab, self.n_vocab + len(videos), dtype=np.int32)
        return videos, rows, labels

    def _join_videos(self, videos: List, vocab_rows, labels: np.ndarray) -> None:
        """The bookkeeping of the constructor's videos (vocab_rows: the dataset's vocabulary, labels: the dataset's, one per video, shared among the captions of a
        video) and of add_videos' (one row and one label of its own per video): the lists are appended to, the vocabulary is registered whole.  16-bit engines: as
        hi + lo operands with the engine (blim_set_video_vocab; the TVG calls name none); other engines take the plain 16-bit clip-major copy."""
        import torch
        self.video += videos
        self.tvg_video_labels = np.concatenate([self.tvg_video_labels, labels]).astype(np.int32)
        if vocab_rows is not None and (self._vocab_src is None or int(vocab_rows.shape[0])):
            self._register_vocab(vocab_rows if self._vocab_src is None else
                                 torch.cat([torch.as_tensor(self._vocab_src).to(torch.float32).cpu(), vocab_rows.to(torch.float32).cpu()], dim=0))
        self.vocab_version += 1

    def _register_vocab(self, src) -> None:
        """The whole vocabulary (float32 source rows [n, clips, M]) registered: with the engine as hi + lo operands, or as the clip-major 16-bit copy."""
        self._vocab_src, self.n_vocab = src, int(src.shape[0])
        if self.split_tvg and hasattr(self.engine, "set_video_vocab"):
            self.engine.set_video_vocab(src)
            self._vocab_key = self.engine._vocab_key
        else:
            self.vocab_cm = _clip_major_vocab(src, self.device, self.m.dtype)

    # ---- videos that leave
    @property
    def live(self) -> np.ndarray:
        """bool [len(video)]: False where remove_videos left a tombstone.  len(video) stays the index space."""
        out = np.ones(len(self.video), dtype=bool)
        if self._dead:
            out[sorted(self._dead)] = False
        return out

    @property
    def n_live(self) -> int:
        return len(self.video) - len(self._dead)

    @property
    def removed(self) -> frozenset:
        """The indices remove_videos took out: what other modules ask instead of the storage."""
        return frozenset(self._dead)

    def live_videos(self) -> np.ndarray:
        """int64, ascending: the indices of the videos that are left."""
        return np.nonzero(self.live)[0]

    def _need_live(self, videos) -> None:
        """ValueError that names the first removed video among `videos` (any array of video indices)."""
        if self._dead:
            for j in np.unique(np.asarray(videos, dtype=np.int64)):
                if int(j) in self._dead:
                    raise ValueError(f"video {int(j)} was removed")

    def check_removal(self, indices) -> np.ndarray:
        """remove_videos' checks, changing nothing: -> the indices, int64; ValueError names the rule."""
        items = list(indices.reshape(-1)) if isinstance(indices, np.ndarray) else list(indices) if isinstance(indices, (list, tuple, range)) else None
        if items is None or any(isinstance(j, (bool, np.bool_)) or not isinstance(j, (int, np.integer)) for j in items):
            raise ValueError("remove_videos: a list of integer video indices")
        idx = np.asarray(items, dtype=np.int64).reshape(-1)
        N = len(self.video)
        if len(idx) and (idx.min() < 0 or idx.max() >= N):
            raise ValueError(f"remove_videos: video index {int(idx.min() if idx.min() < 0 else idx.max())} outside 0 .. {N - 1}")
        srt = np.sort(idx)
        if (srt[1:] == srt[:-1]).any():
            raise ValueError(f"remove_videos: video index {int(srt[1:][srt[1:] == srt[:-1]][0])} named twice")
        gone = [int(j) for j in idx if int(j) in self._dead]
        if gone:
            raise ValueError(f"remove_videos: video {gone[0]} was removed already")
        if len(idx) >= self.n_live:
            raise ValueError(f"remove_videos: {len(idx)} of {self.n_live} videos: at least one video must remain")
        return idx

    def remove_videos(self, indices) -> None:
        """Videos that leave the scorer, the mirror image of add_videos.  Every index is checked before anything changes (check_removal).
        TOMBSTONES: a removed index is never reused and no other index moves -- video[j] becomes None, its cached projected rows are dropped, tvg_video_labels[j]
        becomes -1, `live` / `n_live` say what is left.  A vocabulary entry leaves with its last live video: the float32 source rows of the surviving entries, in
        their order, are registered again whole (the path _join_videos takes), the surviving labels are compacted to 0 .. n_vocab - 1 in their old order, and
        vocab_version is bumped -- gallery_feats(), _label_inverse and every memo of a TVG value keyed by it are computed again, over the gallery as it now is.  A
        scorer built without a vocabulary removes the videos without touching one.  Every entry that takes video indices refuses a removed one by name."""
        import torch
        idx = self.check_removal(indices)
        if not len(idx):
            return
        labels = np.asarray(self.tvg_video_labels, dtype=np.int32).copy()
        old = labels[idx]
        for j in idx:
            self.video[int(j)] = None
            self._vfeat.pop((int(j), True), None); self._vfeat.pop((int(j), False), None)
        labels[idx] = -1
        self._dead = self._dead | frozenset(int(j) for j in idx)
        self._upcoming, self._upcoming_pos = {}, {}                         # (a look-ahead order may name what just left)
        if self.has_vocab and self._vocab_src is not None:
            still = set(labels[labels >= 0].tolist())
            keep = np.ones(self.n_vocab, dtype=bool)
            keep[[int(l) for l in old if 0 <= int(l) < self.n_vocab and int(l) not in still]] = False
            if not keep.all():
                new_of = np.cumsum(keep) - 1                                 # old entry -> its place among the survivors
                at = (labels >= 0) & (labels < self.n_vocab)
                labels[at] = new_of[labels[at]]
                self._register_vocab(torch.as_tensor(self._vocab_src).to(torch.float32).cpu()[torch.from_numpy(np.nonzero(keep)[0])])
        self.tvg_video_labels = labels.astype(np.int32)
        self.vocab_version += 1

    def _need_tvg(self, texts) -> None:
        for i in np.unique(np.asarray(texts, dtype=np.int64)):
            if self.tvg_split[int(i)] is None:
                raise ValueError(f"text {int(i)} was added without a TVG row: it has no TVG score")

    # ---- projected video features, cached on device (K1 once per video instead of once per pair)
    def video_feat(self, j: int, tvg: bool):
        """Projected feature rows of video j, cached on device.  TVG rows (clip means) are produced in the compensated mode when the TVG
        calls run in it: [clips, 2H] rows of hi | lo -- at 7B depth the 16-bit rounding of the projector output was the largest remaining
        error of the TVG scores.

        A miss projects a CHUNK: video j together with the next videos the running pass will ask for (`expect`), one upload and one
        projector call per `feat_chunk` videos.  A projected row depends on its own input row only, so the values are those of a
        per-video call; what changes is the fixed cost -- one upload + six launches per video was 0.4 ms x N on EVERY rank of a sharded
        evaluation (every rank needs the clip features of nearly all videos), the part of the job that did not shrink with the world size."""
        key = (int(j), bool(tvg))
        if key[0] in self._dead:
            raise ValueError(f"video {key[0]} was removed")
        f = self._vfeat.get(key)
        if f is None:
            self._project_chunk(int(j), bool(tvg))
            f = self._vfeat[key]
        return f

    def expect(self, video_ids, tvg: bool) -> None:
        """Order in which the pass being planned will first ask for its videos (chunked projection looks ahead along it)."""
        ids = np.asarray(video_ids, dtype=np.int64)
        self._need_live(ids)
        _, first = np.unique(ids, return_index=True)
        self._upcoming[bool(tvg)] = [int(v) for v in ids[np.sort(first)]]
        self._upcoming_pos[bool(tvg)] = 0

    def share_tvg_feats(self, world: int, rank: int) -> bool:
        """Multi-GPU evaluations: every rank needs the TVG clip features (tvg_mlp projection + clip means, a few KB per video) of nearly ALL videos --
        its texts' candidates -- which left an upload + projection of N videos on every rank whatever the world size.  Instead each rank projects the
        videos of its own row block and ONE all-gather ([N / W + 1, clips, width] per rank; 57 MB in total at N = 1000) hands everyone the rest.  The
        values are those of a local projection (a projected row depends on its own input row only).  Returns False (nothing done) when the videos differ
        in shape or no process group is up; then video_feat() projects on demand as before."""
        import torch
        if (world <= 1 and not dist_utils.force_collective()) or not dist_utils.is_dist_avail_and_initialized() or not hasattr(self.m, "project_many"):
            return False
        if self._dead:                                                       # (row blocks are cut over index space: a scorer with tombstones projects on demand)
            return False
        N = len(self.video)
        if len({tuple(v.shape) for v in self.video}) != 1:
            return False
        s_, e_ = dist_utils.row_block(N, world, rank)
        step = N // world + 1
        self.expect(np.arange(s_, e_), True)
        mine = [self.video_feat(j, True) for j in range(s_, e_)]
        per, width = (int(mine[0].shape[0]), int(mine[0].shape[1])) if mine else (self.num_clips, self.m.dims.hidden_size * (2 if self.split_tvg else 1))
        buf = torch.zeros((step * per, width), dtype=self.m.dtype, device=self.device)
        if mine:
            buf[: (e_ - s_) * per] = torch.cat(mine, dim=0)
        parts = [torch.empty_like(buf) for _ in range(world)]
        torch.distributed.all_gather(parts, buf)
        for r in range(world):
            rs, re = dist_utils.row_block(N, world, r)
            for j in range(rs, re):
                self._vfeat[(j, True)] = parts[r][(j - rs) * per:(j - rs + 1) * per]
        return True

    def adopt_tvg_feats(self, world: int, rank: int, peers) -> bool:
        """Shard emulation's stand-in for share_tvg_feats (one process plays rank `rank` of `world`; there is nobody to gather from): the rank projects the
        videos of its OWN row block here, as share_tvg_feats would, and takes the other blocks' clip features from `peers` ({video index: [clips, width] device
        rows}, e.g. an earlier evaluation's, handed in by the caller) -- what the all-gather would have delivered; the all-gather's own time is NOT part of
        an emulated rank's clock.  Rows of another width (another TVG mode) are not adopted; such videos are projected on demand as before."""
        N = len(self.video)
        if world <= 1 or not peers or self._dead or len({tuple(v.shape) for v in self.video}) != 1:
            return False
        s_, e_ = dist_utils.row_block(N, world, rank)
        self.expect(np.arange(s_, e_), True)
        mine = [self.video_feat(j, True) for j in range(s_, e_)]
        width = int(mine[0].shape[1]) if mine else self.m.dims.hidden_size * (2 if self.split_tvg else 1)
        for j, f in peers.items():
            if not (s_ <= j < e_) and (int(j), True) not in self._vfeat and int(f.shape[1]) == width and f.dtype == self.m.dtype:
                self._vfeat[(int(j), True)] = f
        return True

    def _project_chunk(self, j: int, tvg: bool) -> None:
        shape = tuple(self.video[j].shape)
        chunk = [j]
        up, pos = self._upcoming.get(tvg, []), self._upcoming_pos.get(tvg, 0)
        while pos < len(up) and len(chunk) < self.feat_chunk:
            v = up[pos]; pos += 1
            if v != j and (v, tvg) not in self._vfeat and tuple(self.video[v].shape) == shape:
                chunk.append(v)
        self._upcoming_pos[tvg] = pos
        split = self.split_tvg if tvg else self.split_vtg
        many = getattr(self.m, "project_many", None)
        if split:
            self.engine.set_precise(True, embeds=True)
        try:
            if many is not None:
                outs = many([self.video[v] for v in chunk], tvg)
            else:                                                            # a model surface with the per-video projector only
                outs = [self.m.project(self.video[v].to(self.device), tvg, cache=False) for v in chunk]
        finally:
            if split:
                self.engine.set_precise(False)
        for v, y in zip(chunk, outs):
            self._vfeat[(v, tvg)] = y

    # ---- planning (host) ------------------------------------------------------------------------
    def plan_vtg(self, pairs: np.ndarray, cpn: bool = False) -> List[Plan]:
        return list(self.iter_vtg(pairs, cpn))

    def plan_tvg(self, pairs: np.ndarray, cpn: bool = False) -> List[Plan]:
        return list(self.iter_tvg(pairs, cpn))

    def iter_vtg(self, pairs: np.ndarray, cpn: bool = False):
        """pairs: [P, 2] (video j, text i).  cpn=True: video keys masked -> the score depends on the text only.
        Yields one Plan per engine call, so that packing call k+1 (host) overlaps call k (device)."""
        return self.iter_vtg_jobs([(pairs, cpn)])

    def iter_vtg_jobs(self, jobs, slots=None):
        """Several VTG passes -- [(pairs, cpn), ...] -- planned into the SAME engine calls (outputs concatenated in job order): a plan does not know which pass a
        sequence belongs to (a prior's prompt is its own sequence with the video's positions left out), so a rank's text-block prior rides in the last, partly
        filled call of its likelihood pass instead of being a latency-bound call of its own (iter_tvg_jobs: the TVG counterpart).  slots: a prefix source (_pack_vtg)."""
        items, base = [], 0
        for pairs, cpn in jobs:
            pairs = np.asarray(pairs, dtype=np.int64)
            items += self._vtg_items(pairs, bool(cpn), base)
            base += len(pairs)
        yield from self._pack_vtg(items, slots)

    def _vtg_items(self, pairs: np.ndarray, cpn: bool, base: int):
        """Groups of one VTG pass: (video j or None for a prior, its token count, texts, output slots per text), output slot of pair p = base + p."""
        if len(pairs):
            self._need_live(pairs[:, 0])
        if cpn:
            texts, inv = np.unique(pairs[:, 1], return_inverse=True)
            # the prior masks the video keys but keeps their positions: every video must contribute the same number of tokens,
            # else the reference's per-pair cpn forward would differ between queries too
            nvs = {int(np.prod(self.video[int(j)].shape[-3:-1])) for j in np.unique(pairs[:, 0])}
            if len(nvs) != 1:
                raise ValueError(f"VTG candidate prior: the videos of this pass have different token counts {sorted(nvs)}; score them per count")
            nv = nvs.pop()
            groups: Dict[Tuple, List[int]] = {}
            for ti, i in enumerate(texts):
                pre, post, _ = self.vtg_split[int(i)]
                groups.setdefault((pre.tobytes(), post.tobytes()), []).append(ti)
            return [(None, nv, [int(texts[t]) for t in g], [base + np.nonzero(inv == t)[0] for t in g]) for g in groups.values()]
        order = np.lexsort((pairs[:, 1], pairs[:, 0]))
        self.expect(pairs[order, 0], False)
        items = []
        j_prev, cur = None, None
        for idx in order:
            j, i = int(pairs[idx, 0]), int(pairs[idx, 1])
            pre, post, _ = self.vtg_split[i]
            key = (j, pre.tobytes(), post.tobytes())
            if key != j_prev:
                cur = (j, None, [], [])
                items.append(cur); j_prev = key
            cur[2].append(i); cur[3].append(np.array([base + idx]))
        return items

    def _pack_vtg(self, items, slots=None):
        """Packs groups into super-batches.  slots: a prefix source (blim_amd/prefix_index.py: `slot_of` {(video, pre, post): slot} and `cache.slot_len`) -- a group whose
        prefix it holds packs no prefix sequence: its sequences name the slot and each pair's first row is -(slot + 1).  A source with an `admit(key)` hook (a lazy
        index) is offered every prefix that had to be packed: when it returns a slot, the plan records the admission of that prefix sequence (Plan.admits; its row is
        the position of the prefix's last token in `rows`).  The group itself keeps the in-batch prefix: a slot is readable from the next call on."""
        st = _PackState(self, "vtg", slots)
        for (j, nv, texts_g, outs_g) in items:
            if j is not None and j in self._dead:
                raise ValueError(f"video {j} was removed")
            pre, post, _ = self.vtg_split[texts_g[0]]
            slot = -1 if slots is None or j is None else slots.slot_of.get((j, pre.tobytes(), post.tobytes()), -1)
            if j is None:
                n_vid = nv
            elif slot >= 0:                                                # a cached video is not projected at query time: its token count is its shape's
                n_vid = int(np.prod(self.video[j].shape[-3:-1]))
            else:
                n_vid = int(self.video_feat(j, False).shape[0])
            ppos_end = len(pre) + n_vid + len(post)
            need = (0 if slot >= 0 else ppos_end - (n_vid if j is None else 0)) + sum(max(len(self.vtg_split[i][2]) - 1, 0) for i in texts_g)
            if st.n_tok and st.n_tok + need > self.max_tokens:
                yield st.finish(); st = _PackState(self, "vtg", slots)
            # prefix sequence
            if slot >= 0:
                plen = slots.cache.slot_len(slot)
                if plen != ppos_end:
                    raise RuntimeError(f"gallery slot {slot} holds {plen} positions, the prefix of video {j} has {ppos_end}")
                st.used.add(slot)
                p0, last = 0, -(slot + 1)
            else:
                if j is None:
                    if len(pre) + len(post) == 0:
                        # the reference's rows always open with the ChatML header; with no visible token in front of the response the
                        # prior's first factor would be read from a fully masked video position (undefined attention row)
                        raise ValueError("VTG candidate prior (cpn=True) needs at least one prompt token besides the <image> placeholder")
                    ptoks = np.concatenate([pre, post]); ppos = np.concatenate([np.arange(len(pre)), len(pre) + n_vid + np.arange(len(post))])
                else:
                    fo = st.add_feat(self.video_feat(j, False))
                    ptoks = np.concatenate([pre, -(1 + fo + np.arange(n_vid)), post]); ppos = np.arange(len(ptoks))
                p0 = st.add_seq(ptoks, ppos, np.ones(len(ptoks), np.uint8), None)
                plen = len(ptoks); last = p0 + plen - 1
                if j is not None:
                    st.offer((j, pre.tobytes(), post.tobytes()), p0, plen)
            for i, outs in zip(texts_g, outs_g):
                resp = self.vtg_split[i][2]
                if self.max_row_len is not None and ppos_end + len(resp) > self.max_row_len:
                    if ppos_end >= self.max_row_len:                       # no label left: the reference's criterion divides 0 by 0 there
                        raise ValueError(f"tokenizer_model_max_length = {self.max_row_len} leaves no response token of text {i} ({ppos_end} prompt + video tokens)")
                    resp = resp[: self.max_row_len - ppos_end]             # :452-457: the row's tail is cut, the score averages the tokens that remain
                body = resp[:-1]                                           # the last response token predicts nothing
                rows = [last]
                if len(body):
                    s0 = st.add_seq(body, ppos_end + np.arange(len(body)), np.ones(len(body), np.uint8), (p0, plen), slot=slot)
                    rows += list(range(s0, s0 + len(body)))
                st.add_pair(rows, resp.astype(np.int32), outs)
        if st.n_pairs:
            yield st.finish()

    def iter_tvg(self, pairs: np.ndarray, cpn: bool = False):
        """pairs: [P, 2] (video j, text i); score = log P(video j | text i) (mean over clips)."""
        return self.iter_tvg_jobs([(pairs, cpn)])

    def iter_tvg_jobs(self, jobs, slots=None):
        """Several TVG passes -- [(pairs, cpn), ...] -- planned into the SAME engine calls: outputs are concatenated in job order.  A plan does not know which pass
        a sequence belongs to (visibility is per token, a prior's prefix is its own sequence), so a small likelihood pass and its prior fill one call instead of
        leaving two partly filled ones -- what a rank's share of a sharded evaluation and the calibration sample consist of.  slots: a prefix source (_plan_tvg)."""
        box, base = [_PackState(self, "tvg", slots)], 0
        for pairs, cpn in jobs:
            pairs = np.asarray(pairs, dtype=np.int64)
            yield from self._plan_tvg(pairs, bool(cpn), box, base, slots)
            base += len(pairs)
        if box[0].n_pairs:
            yield box[0].finish()

    def _plan_tvg(self, pairs: np.ndarray, cpn: bool, box, base: int, slots=None):
        """Plans one TVG pass into the pack state box[0] (replaced whenever a call is full and yielded); output slot of pair p = base + p.  slots: a prefix source
        (blim_amd/prefix_index.py: `slot_of` {caption prompt bytes: slot} and `cache.slot_len`) -- a text whose prompt it holds packs no prompt: its merged sequences name
        the slot and each pair's first row is -(slot + 1).  The priors (cpn) have no cached form."""
        C = self.num_clips
        st = box[0]
        if len(pairs):
            self._need_tvg(pairs[:, 1])
            self._need_live(pairs[:, 0])                                     # (a tombstone's label is -1: it never reaches the engine)
        # The continuations of one prefix -- the C - 1 clip tokens of every candidate video of a text (prior: last prompt token + clip tokens) -- are
        # packed into ONE sequence whose segments do not see each other (blim_batch.own_start): the 32-query attention blocks are dense instead of
        # holding 3 - 4 queries each (2,919 -> ~500 blocks per 13,700-token call at the reference's shapes) and the planner adds one sequence per
        # group instead of one per pair.  SEG_MAX bounds a merged sequence.
        if cpn:
            # prior depends on (prompt length, last prompt token, first tvg_prefix_length tokens, video) only
            tp = self.m.tvg_prefix_length
            keyed: Dict[Tuple, List[int]] = {}
            for idx, (j, i) in enumerate(pairs):
                pr = self.tvg_split[int(i)]
                keyed.setdefault((pr[:tp].tobytes(), len(pr), int(pr[-1]), int(j)), []).append(idx)
            by_prefix: Dict[bytes, List[Tuple]] = {}
            for k, v in keyed.items():
                by_prefix.setdefault(k[0], []).append((k, v))
            self.expect([k[3] for lst in by_prefix.values() for (k, _) in lst], True)
            for pbytes, lst in by_prefix.items():
                ptoks = np.frombuffer(pbytes, dtype=np.int64)
                pos_in, p0 = 0, None
                while pos_in < len(lst):
                    room = (self.max_tokens - st.n_tok - (len(ptoks) if p0 is None else 0)) // C
                    if st.n_tok and room < 1:
                        yield st.finish(); st = box[0] = _PackState(self, "tvg"); p0 = None
                        room = (self.max_tokens - len(ptoks)) // C
                    n = max(1, min(len(lst) - pos_in, room, SEG_MAX // C))
                    if p0 is None:                       # the prefix is packed once per engine call; every merged sequence of the group names it
                        p0 = st.add_seq(ptoks, np.arange(len(ptoks)), np.ones(len(ptoks), np.uint8), None)
                    toks, posn, vis, own = [], [], [], []
                    for m_, (k, outs) in enumerate(lst[pos_in:pos_in + n]):
                        _, plen_full, last_tok, j = k
                        fo = st.add_feat(self.video_feat(j, True))
                        toks.append(np.concatenate([[last_tok], -(1 + fo + np.arange(C - 1))]))
                        posn.append(plen_full - 1 + np.arange(C))
                        vis.append(np.concatenate([[1 if plen_full - 1 < tp else 0], np.ones(C - 1)]).astype(np.uint8))
                        own.append(np.full(C, m_ * C, np.int32))
                    s0 = st.add_seq(np.concatenate(toks), np.concatenate(posn), np.concatenate(vis), (p0, len(ptoks)), own_start=np.concatenate(own))
                    for m_, (k, outs) in enumerate(lst[pos_in:pos_in + n]):
                        st.add_pair(list(range(s0 + m_ * C, s0 + (m_ + 1) * C)), np.array([self.tvg_video_labels[k[3]]], np.int32), base + np.array(outs))
                    pos_in += n
        else:
            order = np.lexsort((pairs[:, 0], pairs[:, 1]))
            self.expect(pairs[order, 0], True)
            # candidates of each text, in order
            groups: List[Tuple[int, List[int]]] = []
            for idx in order:
                i = int(pairs[idx, 1])
                if not groups or groups[-1][0] != i:
                    groups.append((i, []))
                groups[-1][1].append(int(idx))
            per = max(C - 1, 1)
            for i, idxs in groups:
                pr = self.tvg_split[i]
                plen = len(pr)
                slot = -1 if slots is None else slots.slot_of.get(pr.tobytes(), -1)
                if slot >= 0:
                    held = slots.cache.slot_len(slot)
                    if held != plen:
                        raise RuntimeError(f"text gallery slot {slot} holds {held} positions, the caption prompt of text {i} has {plen}")
                pos_in, p0 = 0, None
                while pos_in < len(idxs):
                    own = plen if slot < 0 and p0 is None else 0          # prompt tokens this text still has to pack into the call (a cached text: none)
                    room = (self.max_tokens - st.n_tok - own) // per
                    # (num_clips == 1 over a prefix source: a cached text adds no token, so the rows alone fill a call)
                    if (st.n_tok and room < 1) or (slots is not None and C == 1 and st.n_pairs >= self.max_tokens):
                        yield st.finish(); st = box[0] = _PackState(self, "tvg", slots); p0 = None
                        room = (self.max_tokens - (plen if slot < 0 else 0)) // per
                    n = max(1, min(len(idxs) - pos_in, room, SEG_MAX // per))
                    if slot >= 0:
                        st.used.add(slot)
                        first, pfx = -(slot + 1), (0, plen)
                    else:
                        if p0 is None:                   # the prompt is packed once per engine call; every merged sequence of the text names it
                            p0 = st.add_seq(pr, np.arange(plen), np.ones(plen, np.uint8), None)
                            st.offer(pr.tobytes(), p0, plen)   # (a source with `admit`: the packed prompt may be captured into a slot, as in _pack_vtg)
                        first, pfx = p0 + plen - 1, (p0, plen)
                    chunk = idxs[pos_in:pos_in + n]
                    s0 = None
                    if C > 1:
                        toks, own_start = [], []
                        for m_, idx in enumerate(chunk):
                            fo = st.add_feat(self.video_feat(int(pairs[idx, 0]), True))
                            toks.append(-(1 + fo + np.arange(C - 1)))
                            own_start.append(np.full(C - 1, m_ * (C - 1), np.int32))
                        s0 = st.add_seq(np.concatenate(toks), np.tile(plen + np.arange(C - 1), n), np.ones(n * (C - 1), np.uint8), pfx,
                                        own_start=np.concatenate(own_start), slot=slot)
                    for m_, idx in enumerate(chunk):
                        rows = [first]
                        if C > 1:
                            rows += list(range(s0 + m_ * (C - 1), s0 + (m_ + 1) * (C - 1)))
                        else:
                            self.video_feat(int(pairs[idx, 0]), True)
                        st.add_pair(rows, np.array([self.tvg_video_labels[int(pairs[idx, 0])]], np.int32), np.array([base + idx]))
                    pos_in += n

    # ---- one text against the WHOLE gallery (the shortlist's stage 1)
    def gallery_chunk(self) -> int:
        """Videos per merged sequence of the whole-gallery planner: the bound of _plan_tvg's merged sequences."""
        return SEG_MAX // max(self.num_clips - 1, 1)

    def gallery_feats(self):
        """The TVG feature rows of every live video as ONE device tensor [n_live * C, Hw], the rows of the p-th live video (ascending index; video j itself in a
        scorer without tombstones) at p * C as video_feat(j, True) lays them out (its own values: a concatenation).  Built once per (weights version, split_tvg, vocab_version) and dropped when one changes (add_videos bumps the last: the cached per-video rows
        stay, the concatenation is made again); a call of iter_tvg_gallery names it as its feature rows."""
        import torch
        key = (getattr(self.engine, "weights_version", None), bool(self.split_tvg), self.vocab_version)
        memo = getattr(self, "_gfeat", None)
        if memo is None or memo[0] != key:
            C = self.num_clips
            lv = np.nonzero(self.live)[0]                                    # (the live videos, ascending: the p-th of them has its rows at p * C)
            self.expect(lv, True)
            rows = [self.video_feat(int(j), True) for j in lv]
            if any(int(r.shape[0]) != C for r in rows):
                raise ValueError(f"tvg_gallery: every video must project to num_clips = {C} TVG rows")
            memo = self._gfeat = (key, torch.cat(rows, dim=0))
        return memo[1]

    def iter_tvg_gallery(self, texts, chunk: Optional[int] = None):
        """texts [Q] (text indices) against every video of the scorer: the engine calls of log P(video j | text), output slot of (texts[q], video j) = q * N + j.
        The likelihood branch of _plan_tvg with two differences.  FIXED CHUNKS: a text's videos are cut into merged sequences of exactly `chunk` videos (default
        SEG_MAX // max(C - 1, 1); the last one shorter) whatever else shares the call, and a chunk that does not fit the call starts a new one -- a TVG score moves
        with its neighbours in the merged sequence, so with fixed cuts it depends on its text and the gallery alone.  NO PER-VIDEO PYTHON:
        the feature rows are gallery_feats(), added once per call, and a chunk's tokens, positions, own_start, rows, labels and output slots are array expressions
        -- the host cost of a text is O(chunks).  Row conventions are _plan_tvg's: the prompt packed once per call, each pair's first row the prompt's last row."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        C, N = self.num_clips, len(self.video)
        chunk = self.gallery_chunk() if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"tvg_gallery: chunk = {chunk}: at least one video per merged sequence")
        if not len(texts) or not N:
            return
        self._need_tvg(texts)
        # the fixed chunks are cut over the LIVE videos in ascending index order: a scorer with tombstones plans the calls of a scorer built
        # from the survivors, and only the output slots are index space
        lv = np.nonzero(self.live)[0] if self._dead else np.arange(N)
        L = len(lv)
        longest = max(len(self.tvg_split[int(i)]) for i in texts)
        if longest + min(chunk, L) * (C - 1) > self.max_tokens:
            raise ValueError(f"tvg_gallery: max_tokens = {self.max_tokens} cannot hold one caption prompt ({longest} tokens) and one chunk of {min(chunk, L)} videos "
                             f"({min(chunk, L) * (C - 1)} tokens)")
        feats = self.gallery_feats()
        clip = np.arange(C - 1)
        st = _GalleryCall(self, feats)
        for q, i in enumerate(texts):
            pr = self.tvg_split[int(i)]
            plen = len(pr)
            p0 = None
            for v0 in range(0, L, chunk):
                n = min(chunk, L - v0)
                if st.n_tok and st.n_tok + (plen if p0 is None else 0) + n * (C - 1) > self.max_tokens:
                    yield st.finish(); st = _GalleryCall(self, feats); p0 = None
                if p0 is None:                           # the prompt is packed once per engine call; every merged sequence of the text names it
                    p0 = st.add_seq(pr, np.arange(plen), None, (0, 0))
                at = np.arange(v0, v0 + n)                   # places among the live videos: where gallery_feats() holds their rows
                v = lv[at]
                rows = np.full((n, C), p0 + plen - 1, np.int64)
                if C > 1:
                    s0 = st.add_seq(-(1 + at[:, None] * C + clip[None, :]).reshape(-1), np.tile(plen + clip, n), np.repeat(np.arange(n) * (C - 1), C - 1), (p0, plen))
                    rows[:, 1:] = s0 + np.arange(n)[:, None] * (C - 1) + clip[None, :]
                st.add_pairs(rows, self.tvg_video_labels[v], q * N + v)
        if st.n_pairs:
            yield st.finish()

    def tvg_gallery(self, texts, chunk: Optional[int] = None) -> np.ndarray:
        """log P(video j | text) of each text against every live video -> f32 [Q, N] in video-index order, NaN in the column of a removed video.  Each distinct text
        is planned once, in ascending index order (iter_tvg_gallery); a value does not depend on which texts are asked for together, in which order, or on where
        max_tokens cuts the calls."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        N = len(self.video)
        uniq, inv = np.unique(texts, return_inverse=True)
        out = np.full(len(uniq) * N, np.nan, dtype=np.float32)
        done = [(p.out_index, self.run(p)) for p in self.iter_tvg_gallery(uniq, chunk)]
        for out_index, r in done:
            out[out_index[:, 0]] = r.float().cpu().numpy()
        return out.reshape(len(uniq), N)[inv.reshape(-1)]

    # ---- clip 0 of every video from the caption prompt alone (the prefilter's stage 0)
    def iter_tvg_first(self, texts, cpn: bool = False):
        """texts [Q] (text indices): the engine calls of log P(clip 0 of video j | text) for EVERY j at once -- a pair's first scored row is its prompt's last
        row (_plan_tvg), so one row per text carries the whole gallery.  Each distinct caption prompt (by bytes) is packed once, a sequence of its own; its scored
        row is its last token.  cpn: for each distinct video-independent prior key of _plan_tvg (pr[:tp] bytes, len(pr), pr[-1]) the head pr[:tp] is packed once
        per call and a one-token sequence [pr[-1]] follows it at position len(pr) - 1, visible as a key when len(pr) - 1 < tp, the head its prefix: the first
        token of _plan_tvg's prior segment, which predicts clip 0 and does not depend on the video.  Plans of kind "tvg_first": rows = the prompts' rows,
        prior_rows = the prior tokens' rows, labels = each prompt row's index into prior_rows, out_index = the positions in `texts` each row answers.  Calls are
        cut at max_tokens; a prompt and its prior share a call."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        if not len(texts):
            return
        self._need_tvg(texts)
        tp = self.m.tvg_prefix_length
        groups: Dict[bytes, List[int]] = {}
        for q, i in enumerate(texts):
            groups.setdefault(self.tvg_split[int(i)].tobytes(), []).append(q)
        st = _FirstCall(self, cpn)
        for pbytes, outs in groups.items():
            pr = np.frombuffer(pbytes, dtype=np.int64)
            if st.n_tok and st.n_tok + st.need(pr, tp) > self.max_tokens:
                yield st.finish(); st = _FirstCall(self, cpn)
            st.add(pr, tp, outs)
        if st.n_pairs:
            yield st.finish()

    def _label_inverse(self):
        """-> (device int64 [n_vocab]: the video of each vocabulary entry, device int64 [n_live]: the live videos' labels, ascending by video -- tvg_video_labels
        itself in a scorer without tombstones), memoised per vocab_version with their host copies (_label_inverse_host: the inverse, and tvg_video_labels in index
        space).  The rank kernel ranks VOCABULARY entries; they name videos only when the live videos' labels are a permutation of arange(n_vocab)."""
        import torch
        memo = getattr(self, "_label_inv", None)
        if memo is None or memo[0] != self.vocab_version:
            lab = np.asarray(self.tvg_video_labels, dtype=np.int64)
            N = len(self.video)
            if self._dead:                                                   #  the rule over what is left: inv names live videos only
                at = np.nonzero(self.live)[0]
                N = len(at)
                if len(lab) != len(self.video) or self.n_vocab != N or not np.array_equal(np.sort(lab[at]), np.arange(N)):
                    raise ValueError(f"tvg_first: the live videos' tvg_video_labels must be a permutation of arange({N}) -- one vocabulary entry per live video "
                                     f"({self.n_vocab} entries, {len(np.unique(lab[at]))} distinct labels)")
                inv = np.empty(N, dtype=np.int64)
                inv[lab[at]] = at
                dev_lab = lab[at]                                            # the labels of the live videos, ascending by video: the live columns of a `full` result
            else:
                dev_lab = lab
                if len(lab) != N or self.n_vocab != N or not np.array_equal(np.sort(lab), np.arange(N)):
                    raise ValueError(f"tvg_first: tvg_video_labels must be a permutation of arange({N}) -- one vocabulary entry per video ({self.n_vocab} entries, "
                                     f"{len(np.unique(lab))} distinct labels)")
                inv = np.empty(N, dtype=np.int64)
                inv[lab] = np.arange(N)
            memo = self._label_inv = (self.vocab_version, torch.from_numpy(inv).to(self.device), torch.from_numpy(dev_lab).to(self.device), inv, lab)
        return memo[1], memo[2]

    def _label_inverse_host(self):
        """_label_inverse's two arrays as numpy int64, from the same memo."""
        self._label_inverse()
        return self._label_inv[3], self._label_inv[4]

    def tvg_first(self, texts, k: int, cpn: bool = False, alpha: float = 0.0, full: bool = False, within=None):
        """The best k videos of each text by log P(clip 0 of the video | text) -- minus alpha x the candidate prior's clip-0 term with cpn -- ranked ON THE DEVICE
        (Engine.score_tvg_first): -> (idx int64 [Q, k] video indices, val f32 [Q, k], and with full lp f32 [Q, N], the log-probabilities by video index).  The order
        is descending with ties to the lower VOCABULARY entry.  Each distinct prompt is computed once; a value does not depend on what shares its call.
        within: one array of video indices per text -- text q is ranked inside its own set alone (Engine.score_tvg_first_within).  Each set is made unique and
        sorted by vocabulary entry, so the kernel's position order is the tie order above and the result is the whole-gallery order filtered to the set, every
        value the same bits (the normaliser stays over the whole vocabulary).  Text q gets min(k, len(within[q])) real places, the rest are -1 / NaN; k is then
        bounded by TVG_RANK_MAX_K alone.  Texts with one prompt still share one packed row.  After remove_videos nothing changes here: the kernels rank vocabulary
        entries, so a removed video cannot appear; lp keeps index-space columns [Q, len(video)], NaN in a removed one, and a set that names one is refused."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        N, k = self.n_vocab, int(k)
        if within is not None:
            return self._tvg_first_within(texts, k, cpn, alpha, full, within)
        inv, lab = self._label_inverse()
        if not 1 <= k <= N:
            raise ValueError(f"tvg_first: k = {k} outside 1 .. {N}")
        idx = np.zeros((len(texts), k), dtype=np.int64)
        val = np.zeros((len(texts), k), dtype=np.float32)
        lp = np.zeros((len(texts), N), dtype=np.float32) if full else None
        cols = None
        if full and self._dead:                                              # index-space columns, NaN where a video was removed
            lp, cols = np.full((len(texts), len(self.video)), np.nan, dtype=np.float32), np.nonzero(self.live)[0]
        done = [(p.out_index, self.run(p, k=k, alpha=float(alpha), full=full)) for p in self.iter_tvg_first(texts, cpn)]
        for out_index, res in done:
            vi, vv = inv[res[0].long()].cpu().numpy(), res[1].cpu().numpy()
            vl = res[2][:, lab].cpu().numpy() if full else None
            for r, outs in enumerate(out_index):
                idx[outs], val[outs] = vi[r], vv[r]
                if full and cols is None:
                    lp[outs] = vl[r]
                elif full:
                    lp[np.asarray(outs, dtype=np.int64)[:, None], cols[None, :]] = vl[r][None, :]
        return (idx, val, lp) if full else (idx, val)

    def _tvg_first_within(self, texts, k: int, cpn: bool, alpha: float, full: bool, within):
        """tvg_first(within=): per plan of iter_tvg_first one query per text -- row_of carries the fan-out that out_index carries for the whole-gallery form."""
        import torch
        from .engine import TVG_RANK_MAX_K
        if full:
            raise ValueError("tvg_first: full=True returns the whole gallery's rows and takes no within")
        if not 1 <= k <= TVG_RANK_MAX_K:
            raise ValueError(f"tvg_first: k = {k} outside 1 .. TVG_RANK_MAX_K = {TVG_RANK_MAX_K}")
        if len(within) != len(texts):
            raise ValueError(f"tvg_first: within holds {len(within)} sets for {len(texts)} texts")
        N = len(self.video) if self._dead else self.n_vocab                  # (the index space; without tombstones the permutation rule makes the two one number)
        inv, lab = self._label_inverse_host()
        entries = []                                                         # per text: its set as vocabulary entries, unique and ascending
        for q, w in enumerate(within):
            w = np.asarray(w, dtype=np.int64).reshape(-1)
            if len(w) and (w.min() < 0 or w.max() >= N):
                raise ValueError(f"tvg_first: within[{q}] names a video outside 0 .. {N - 1}")
            self._need_live(w)
            entries.append(np.unique(lab[w]))
        idx = np.full((len(texts), k), -1, dtype=np.int64)
        val = np.full((len(texts), k), np.nan, dtype=np.float32)
        done = []
        for p in self.iter_tvg_first(texts, cpn):
            qs = np.concatenate([np.asarray(outs, dtype=np.int64) for outs in p.out_index])
            row_of = np.concatenate([np.full(len(outs), r, dtype=np.int32) for r, outs in enumerate(p.out_index)])
            off = np.zeros(len(qs) + 1, dtype=np.int64)
            np.cumsum([len(entries[q]) for q in qs], out=off[1:])
            if off[-1] >= 2 ** 31:
                raise ValueError(f"tvg_first: the sets of one call hold {int(off[-1])} entries, more than an int32 offset reaches")
            flat = np.concatenate([entries[q] for q in qs] + [np.zeros(1, np.int64)]).astype(np.int32)          # (one entry of padding: never an empty tensor; n_within counts the real ones)
            dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
            done.append((qs, self.run(p, k=k, alpha=float(alpha), within=(dev(row_of, np.int32), dev(flat, np.int32), dev(off, np.int32), int(off[-1])))))
        for qs, res in done:
            pos, vv = res[0].cpu().numpy(), res[1].cpu().numpy()
            for i, q in enumerate(qs):
                kk = min(k, len(entries[q]))
                idx[q, :kk], val[q, :kk] = inv[entries[q][pos[i, :kk]]], vv[i, :kk]
        return idx, val

    # ---- execution (device) ---------------------------------------------------------------------
    @contextmanager
    def _call_options(self, kind: str):
        """The engine options every call of `kind` runs under, for the length of the call.  A prefix cache's fills run under it too (blim_amd/prefix_index.py): the
        engine refuses a slot whose fill ran under other options than the call that reads it."""
        if kind == "vtg":
            comp = self.vtg_mode in VTG_SPLIT_MODES                          # None | "full" | "select"
            self.engine.set_precise(comp, embeds=comp, mlp=True, layers=self.vtg_mode == "select")
        else:
            if self.vocab_cm is None and getattr(self.engine, "_vocab_key", None) != self._vocab_key:
                self.engine.set_video_vocab(self._vocab_src)                 # another scorer / the literal path registered its own vocabulary since
            # TVG calls: compensated (3-5 new tokens per pair: cheap); how much of the MLP branch is compensated follows tvg_mode (calibrate_tvg)
            self.engine.set_precise(self.split_tvg, embeds=self.split_tvg, mlp=self.tvg_mode != "attn", tvg=True)
        try:
            yield
        finally:
            self.engine.set_precise(False)

    def _count(self, plan: Plan) -> None:
        """exec_tokens / exec_flops / exec_flops_lo6 of one engine call."""
        self.exec_tokens += plan.n_tokens
        f8 = getattr(self.engine, "dtype", "") == "f8"
        lo6 = getattr(self.engine, "lo6", False)
        if plan.kind == "vtg":
            mode = self.vtg_mode
            bits = getattr(self.engine, "layer_mask", None) if mode == "select" else None
            self.exec_flops += executed_flops(self.m.dims, plan.n_tokens, plan.n_rows, "vtg", mode, prune=not f8, layer_bits=bits)
            if lo6:
                self.exec_flops_lo6 += lo6_pass_flops(self.m.dims, plan.n_tokens, plan.n_rows, "vtg", mode, prune=not f8, layer_bits=bits)
            return
        self.exec_flops += executed_flops(self.m.dims, plan.n_tokens, plan.n_rows, "tvg", self.tvg_mode if self.split_tvg else None,
                                          n_vocab=self.n_vocab, prune=not f8)
        if lo6 and self.split_tvg and getattr(self.engine, "dtype", "") != "bf16":      # (bf16 engines: TVG calls keep the bf16 second pass, Engine.set_precise)
            self.exec_flops_lo6 += lo6_pass_flops(self.m.dims, plan.n_tokens, plan.n_rows, "tvg", self.tvg_mode, prune=not f8)

    def _register_first_vocab(self) -> None:
        """Inside _call_options("tvg"): a scorer whose TVG calls name their vocabulary registers it, since the clip-0 entries run over the registered one."""
        if self.vocab_cm is not None and (getattr(self, "_first_vocab", None) != (self.vocab_version, getattr(self.engine, "_vocab_key", None))):
            self.engine.set_video_vocab(self._vocab_src)
            self._first_vocab = (self.vocab_version, self.engine._vocab_key)

    def tvg_first_cached(self, cache, slots, cols, chunk_rows: int = 0):
        """log P(clip 0 of vocabulary entry cols[c] | the caption prompt in slots[q]) from the cache's stored hidden rows, under the TVG calls' options
        (PrefixCache.tvg_first_cols: no decode) -> device f32 [n_cols, n_slots].  slots: host ints; cols: device int32."""
        with self._call_options("tvg"):
            self._register_first_vocab()
            return cache.tvg_first_cols(slots, cols, chunk_rows)

    def run(self, plan: Plan, cache=None, k: int = 1, alpha: float = 0.0, full: bool = False, within=None):
        """One engine call; returns a device f32 tensor [plan.n_pairs].  A plan made over a prefix source (plan.pfx_slot) goes through `cache`, the PrefixCache
        that holds its slots, and is not counted in exec_*: those count the scorer's own calls.  A plan of kind "tvg_first" (k, alpha, full are its arguments)
        returns Engine.score_tvg_first's tuple instead -- or, with within = (row_of, within, within_off on the device, n_within), one query per entry of row_of,
        Engine.score_tvg_first_within's."""
        if plan.kind == "tvg_first":
            self._count(plan)
            with self._call_options("tvg"):
                self._register_first_vocab()
                embeds = self.engine.assemble(plan.src_index, plan.feats)
                cpn = plan.prior_rows is not None
                if within is not None:
                    row_of, wi, off, n_within = within
                    return self.engine.score_tvg_first_within(plan.batch, embeds, plan.rows, k, row_of, wi, off, n_within=n_within, prior_rows=plan.prior_rows,
                                                              prior_of=plan.labels[row_of.long()].contiguous() if cpn else None, alpha=alpha if cpn else 0.0)
                return self.engine.score_tvg_first(plan.batch, embeds, plan.rows, k, prior_rows=plan.prior_rows, prior_of=plan.labels if cpn else None,
                                                   alpha=alpha if cpn else 0.0, full=full)
        if plan.pfx_slot is None:
            self._count(plan)
            via, slots = self.engine, ()
        else:
            via, slots = cache, (plan.pfx_slot, plan.slots_used)
        more = {} if plan.admits is None else {"admits": plan.admits}        # (plans of a source that admits: the call also captures the prefixes they name)
        with self._call_options(plan.kind):
            embeds = self.engine.assemble(plan.src_index, plan.feats)
            if plan.kind == "vtg":
                return via.score_vtg(plan.batch, *slots, embeds, plan.rows, plan.labels, plan.row_start, **more)
            return via.score_tvg(plan.batch, *slots, embeds, plan.rows, self.vocab_cm, plan.labels, **more)

    def score(self, plans, n_requested: int, run=None) -> np.ndarray:
        """plans: list or generator of Plan.  Engine calls are asynchronous, so with a generator the host packs plan k+1 while
        the device runs plan k; the scores are copied back once, at the end.  run: what executes a plan (default: self.run)."""
        run = run or self.run
        out = np.full(n_requested, np.nan, dtype=np.float32)
        done = [(p.out_index, run(p)) for p in plans]
        for out_index, r in done:
            sc = r.float().cpu().numpy()
            for k, outs in enumerate(out_index):
                out[outs] = sc[k]
        return out

    def score_device(self, plans, n_requested: int):
        """As score(), but the result stays on the device (f32 [n_requested], NaN where nothing was scored) and nothing
        synchronises: evaluation() scatters it into the score matrix on the device, so the host goes straight on to plan the next
        pass while the device is still running this one."""
        import torch
        out = torch.full((n_requested,), float("nan"), dtype=torch.float32, device=self.device)
        res, src, dst, base = [], [], [], 0
        for p in plans:                                           # every engine call of the pass is queued first ...
            res.append(self.run(p))
            src.append(base + np.repeat(np.arange(len(p.out_index)), [len(o) for o in p.out_index]))
            dst.append(np.concatenate(p.out_index) if len(p.out_index) else np.zeros(0, np.int64))
            base += p.n_pairs
        if res:                                                   # ... then one index upload and one device-side scatter
            idx = torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)).to(self.device)
            out[idx[1]] = torch.cat(res).float()[idx[0]]
        return out

    # ---- which compensation the VTG calls need (`--vtg_precise auto`) ---------------------------------------------------------------
    def set_vtg_mode(self, mode) -> None:
        """Compensation of this scorer's following VTG calls: None | "full" | "select" (the engine's per-layer mask: Engine.set_layer_mask).  The cached VTG feature rows are dropped when their layout changes ([hi | lo] rows in
        the compensated mode).  (The model's own record of what `auto` resolved to is BlimModel.resolve_vtg: calibrate_vtg and evaluation() write it.)"""
        mode = None if mode in (None, "none") else mode
        if mode not in (None,) + VTG_MODES[1:] + ("select",):
            raise ValueError(f"vtg mode {mode!r}: one of {VTG_MODES}")
        if not bool(getattr(self.engine, "can_precise", False)):
            mode = None
        split = mode in VTG_SPLIT_MODES
        if split != self.split_vtg:
            self._vfeat = {k: v for k, v in self._vfeat.items() if k[1]}
        self.vtg_mode, self.split_vtg = mode, split

    def set_tvg_mode(self, mode) -> None:
        if mode not in TVG_MODES:
            raise ValueError(f"tvg mode {mode!r}: one of {TVG_MODES}")
        self.tvg_mode = mode

    def vtg(self, pairs, cpn=False) -> np.ndarray:
        return self.score(self.iter_vtg(pairs, cpn), len(pairs))

    def tvg(self, pairs, cpn=False) -> np.ndarray:
        return self.score(self.iter_tvg(pairs, cpn), len(pairs))

    def vtg_device(self, pairs, cpn=False):
        return self.score_device(self.iter_vtg(pairs, cpn), len(pairs))

    def vtg_jobs_device(self, jobs):
        """Several VTG passes through shared engine calls (iter_vtg_jobs); scores concatenated in job order."""
        return self.score_device(self.iter_vtg_jobs(jobs), sum(len(p) for p, _ in jobs))

    def tvg_device(self, pairs, cpn=False):
        return self.score_device(self.iter_tvg(pairs, cpn), len(pairs))

    def tvg_jobs_device(self, jobs):
        """Several TVG passes through shared engine calls (iter_tvg_jobs); scores concatenated in job order."""
        return self.score_device(self.iter_tvg_jobs(jobs), sum(len(p) for p, _ in jobs))


class _PackState:
    """Accumulates sequences / rows of one super-batch on the host, then uploads once.  slots: the prefix source the call is planned over, if any -- the plan
    then carries the cache slot of every sequence (-1: in-batch prefix) and the slots the call reads."""

    def __init__(self, scorer: PairScorer, kind: str, slots=None):
        self.s, self.kind, self.slots = scorer, kind, slots
        self.tok: List[np.ndarray] = []; self.pos: List[np.ndarray] = []; self.vis: List[np.ndarray] = []
        self.seq_start: List[int] = []; self.seq_len: List[int] = []; self.pfx_start: List[int] = []; self.pfx_len: List[int] = []
        self.slot: List[int] = []; self.used = set()
        self.admit = getattr(slots, "admit", None)                        # the source's hook, if it admits prefixes inside scoring calls
        self.admits: List[Tuple[int, int, int, int]] = []                 # (seq, slot, start, len) of the in-batch prefixes this call captures
        self.n_prefix_tok = 0
        self.own: List[np.ndarray] = []; self.any_own = False             # per token: first own-segment index it attends to (segmented sequences)
        self.feats: List[object] = []; self.feat_key: Dict[int, int] = {}; self.n_feat = 0
        self.rows: List[int] = []; self.labels: List[np.ndarray] = []; self.row_start: List[int] = [0]
        self.out_index: List[np.ndarray] = []
        self.n_tok = 0; self.n_pairs = 0

    def add_feat(self, f) -> int:
        k = f.data_ptr()
        if k in self.feat_key:
            return self.feat_key[k]
        off = self.n_feat
        self.feats.append(f); self.feat_key[k] = off; self.n_feat += int(f.shape[0])
        return off

    def add_seq(self, toks, pos, vis, prefix, own_start=None, slot: int = -1) -> int:
        start = self.n_tok
        self.tok.append(np.asarray(toks, np.int64)); self.pos.append(np.asarray(pos, np.int64)); self.vis.append(np.asarray(vis, np.uint8))
        if own_start is None:
            self.own.append(np.zeros(len(toks), np.int32))
        else:
            self.own.append(np.asarray(own_start, np.int32)); self.any_own = True
        self.seq_start.append(start); self.seq_len.append(len(toks))
        self.pfx_start.append(prefix[0] if prefix else 0); self.pfx_len.append(prefix[1] if prefix else 0)
        self.slot.append(int(slot))
        self.n_tok += len(toks)
        if prefix is None:
            self.n_prefix_tok += len(toks)
        return start

    def offer(self, key, start: int, plen: int) -> None:
        """The prefix sequence just packed (the last one added) is offered to a source that admits: a slot back records the admission."""
        slot = None if self.admit is None else self.admit(key)
        if slot is not None:
            self.admits.append((len(self.seq_start) - 1, int(slot), int(start), int(plen)))

    def add_pair(self, rows, labels, outs):
        self.rows += rows
        self.labels.append(np.asarray(labels, np.int32))
        self.row_start.append(len(self.rows))
        self.out_index.append(np.asarray(outs))
        self.n_pairs += 1

    def upload(self):
        """-> (PackedBatch, assemble's src_index, feature rows) of the sequences so far, on the device."""
        import torch
        dev = self.s.device
        batch = PackedBatch(np.concatenate(self.pos), np.concatenate(self.vis), np.array(self.seq_start), np.array(self.seq_len),
                            np.array(self.pfx_start), np.array(self.pfx_len), device=dev, own_start=np.concatenate(self.own) if self.any_own else None)
        src = torch.from_numpy(np.concatenate(self.tok).astype(np.int32)).to(dev)
        H = self.s.m.dims.hidden_size
        wide = self.s.split_tvg if self.kind == "tvg" else self.s.split_vtg                   # feature rows are [hi | lo]
        feats = torch.cat(self.feats, dim=0) if self.feats else torch.zeros((1, H * (2 if wide else 1)), dtype=self.s.m.dtype, device=dev)
        return batch, src, feats

    def finish(self) -> Plan:
        import torch
        dev = self.s.device
        n_prefix_tok = self.n_prefix_tok
        if self.slots is not None and self.n_tok == 0:     # every pair reads a cached row only (one-token responses): one dummy token keeps the batch non-empty
            self.add_seq(np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, np.uint8), None)
        batch, src, feats = self.upload()
        admits = None
        if self.admits:                                    # the row of an admission: where its prefix's last token stands in `rows` (every pair of the prefix opens with it)
            at: Dict[int, int] = {}
            for r, t_ in enumerate(self.rows):
                at.setdefault(int(t_), r)
            admits = np.array([(q, sl, st_, ln, at[st_ + ln - 1]) for q, sl, st_, ln in self.admits], dtype=np.int32).reshape(-1, 5)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        cached = self.slots is not None
        return Plan(kind=self.kind, batch=batch, src_index=src, feats=feats, rows=t(np.array(self.rows)), labels=t(np.concatenate(self.labels)),
                    row_start=t(np.array(self.row_start)) if self.kind == "vtg" else None, n_pairs=self.n_pairs,
                    out_index=self.out_index, n_tokens=self.n_tok, n_rows=len(self.rows),
                    pfx_slot=t(self.slot) if cached else None, slots_used=np.array(sorted(self.used), dtype=np.int32) if cached else None,
                    admits=admits, prefix_tokens=n_prefix_tok if cached else 0)


class _FirstCall:
    """One engine call of PairScorer.iter_tvg_first: caption prompts, and with cpn the prior heads and one-token prior sequences, each packed once per call."""

    def __init__(self, scorer: PairScorer, cpn: bool):
        self.st, self.cpn = _PackState(scorer, "tvg"), bool(cpn)
        self.heads: Dict[bytes, int] = {}                                  # head bytes -> start of its sequence in this call
        self.priors: Dict[Tuple, int] = {}                                 # prior key -> index into prior_rows
        self.prior_rows: List[int] = []

    n_tok = property(lambda self: self.st.n_tok)
    n_pairs = property(lambda self: self.st.n_pairs)

    def _key(self, pr, tp):
        return (pr[:tp].tobytes(), len(pr), int(pr[-1]))

    def need(self, pr, tp) -> int:
        """Tokens the prompt would add to this call."""
        if not self.cpn:
            return len(pr)
        key = self._key(pr, tp)
        return len(pr) + (0 if key in self.priors else 1 + (0 if key[0] in self.heads else len(pr[:tp])))

    def add(self, pr, tp, outs) -> None:
        st, plen = self.st, len(pr)
        at = -1
        if self.cpn:
            key = self._key(pr, tp)
            at = self.priors.get(key, -1)
            if at < 0:
                head = pr[:tp]
                h0 = self.heads.get(key[0])
                if h0 is None:
                    h0 = self.heads[key[0]] = st.add_seq(head, np.arange(len(head)), np.ones(len(head), np.uint8), None)
                row = st.add_seq(pr[-1:], np.array([plen - 1]), np.array([1 if plen - 1 < tp else 0], np.uint8), (h0, len(head)))
                at = self.priors[key] = len(self.prior_rows)
                self.prior_rows.append(row)
        p0 = st.add_seq(pr, np.arange(plen), np.ones(plen, np.uint8), None)
        st.add_pair([p0 + plen - 1], np.array([at], np.int32), np.asarray(outs, dtype=np.int64))

    def finish(self) -> Plan:
        import torch
        plan = self.st.finish()
        plan.kind = "tvg_first"
        if self.cpn:
            plan.prior_rows = torch.from_numpy(np.asarray(self.prior_rows, dtype=np.int32)).to(self.st.s.device)
            plan.n_rows += len(self.prior_rows)
        return plan


class _GalleryCall:
    """One engine call of PairScorer.iter_tvg_gallery: whole sequences and whole chunks of pairs are added as arrays, then uploaded once.  The feature rows are the
    scorer's gallery_feats(), named by every call as they are (video j's rows at j * C), so nothing is gathered or copied per call."""

    def __init__(self, scorer: PairScorer, feats):
        self.s, self.feats = scorer, feats
        self.tok: List[np.ndarray] = []; self.pos: List[np.ndarray] = []; self.own: List[np.ndarray] = []
        self.seq_start: List[int] = []; self.seq_len: List[int] = []; self.pfx_start: List[int] = []; self.pfx_len: List[int] = []
        self.rows: List[np.ndarray] = []; self.labels: List[np.ndarray] = []; self.out: List[np.ndarray] = []
        self.n_tok = 0; self.n_pairs = 0

    def add_seq(self, toks, pos, own_start, prefix) -> int:
        start = self.n_tok
        self.tok.append(np.asarray(toks, np.int64)); self.pos.append(np.asarray(pos, np.int64))
        self.own.append(np.zeros(len(toks), np.int32) if own_start is None else np.asarray(own_start, np.int32))
        self.seq_start.append(start); self.seq_len.append(len(toks))
        self.pfx_start.append(prefix[0]); self.pfx_len.append(prefix[1])
        self.n_tok += len(toks)
        return start

    def add_pairs(self, rows, labels, outs) -> None:
        """A chunk's pairs: rows [n, C], labels [n], output slots [n]."""
        self.rows.append(rows.reshape(-1)); self.labels.append(np.asarray(labels, np.int32)); self.out.append(np.asarray(outs, np.int64))
        self.n_pairs += len(outs)

    def finish(self) -> Plan:
        import torch
        dev = self.s.device
        batch = PackedBatch(np.concatenate(self.pos), np.ones(self.n_tok, np.uint8), np.array(self.seq_start), np.array(self.seq_len),
                            np.array(self.pfx_start), np.array(self.pfx_len), device=dev, own_start=np.concatenate(self.own))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        rows = np.concatenate(self.rows)
        return Plan(kind="tvg", batch=batch, src_index=t(np.concatenate(self.tok)), feats=self.feats, rows=t(rows), labels=t(np.concatenate(self.labels)),
                    row_start=None, n_pairs=self.n_pairs, out_index=np.concatenate(self.out)[:, None], n_tokens=self.n_tok, n_rows=len(rows))
