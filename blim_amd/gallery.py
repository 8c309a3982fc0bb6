"""Gallery index: rerank new text queries over a gallery whose video prefixes are computed once (t2v `query_likelihood`, log P(text | video)).

A VTG likelihood runs the video's `[header][video][instruction]` prefix through every layer before the text's response tokens; the prefix does not depend on the
query.  `GalleryIndex.build()` fills one slot of the engine's prefix cache (blim.h: blim_prefix_cache_*) per (video j, pre, post) -- the grouping
`PairScorer._vtg_items` uses -- with the K / V of every layer and the last prefix row's final-norm hidden state (that row predicts the first response token).  A
query's pairs are then packed as their response tokens alone (`blim_score_vtg_cached`): 31 tokens per pair instead of ~300 at the 7B shapes.  The scores are bit
for bit those of `PairScorer.vtg` on the same pairs.  Videos beyond the memory budget keep the in-batch prefix, in the same calls.

`TextGalleryIndex` is the other direction (v2t): the gallery is the scorer's texts, a query is a video.  The v2t `query_likelihood` is TVG, log P(video | text); its
prefix is the text's caption prompt, which does not depend on the query video.  One slot per distinct prompt; a query's pairs are then packed as the video's
num_clips - 1 clip tokens alone (`blim_score_tvg_cached`).  DESIGN.md section 11.
"""
from __future__ import annotations

import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .calibration import VTG_SPLIT_MODES
from .pair_scorer import PairScorer, _PackState

SLOT_ALIGN = 32          # a slot's positions are padded to a multiple of the attention's key tile
SEG_MAX = 256            # bound of a merged TVG sequence (PairScorer._plan_tvg)


def slot_plan(keys: Sequence[Tuple], per_slot_bytes: int, budget_bytes: Optional[int], priority: Optional[Sequence[int]] = None) -> Dict[Tuple, int]:
    """Static slot assignment: keys (in gallery order) take slots in `priority` order (indices into keys; default: gallery order) until the budget is used.
    -> {key: slot}.  budget_bytes None: every key gets a slot."""
    order = list(range(len(keys))) if priority is None else [int(p) for p in priority]
    if sorted(order) != list(range(len(keys))):
        raise ValueError("priority must be a permutation of the gallery's prefixes")
    n = len(keys) if budget_bytes is None else min(len(keys), int(budget_bytes) // max(int(per_slot_bytes), 1))
    return {keys[k]: s for s, k in enumerate(order[:n])}


def cache_bytes(dims, n_slots: int, max_len: int, compensated: bool) -> int:
    """Device bytes of a prefix cache (blim.h: blim_prefix_cache_bytes): per slot, num_layers x max_len positions of K | V heads (and their lo parts when
    compensated) plus one hidden row (hi, and lo when compensated), 16-bit values."""
    f = 2 if compensated else 1
    return int(n_slots) * (dims.num_layers * int(max_len) * 2 * dims.num_kv_heads * dims.head_dim * f + dims.hidden_size * f) * 2


class GalleryIndex:
    """t2v VTG scores of arbitrary (video, text) pairs of a PairScorer's videos and texts, with the videos' prefixes cached on the device.

    scorer: the PairScorer whose videos form the gallery and whose texts are the queries (dataset captions and / or free-text queries packed by the same prompt
    builder); its prompt splits (vtg_split) and projected video features are reused.  budget_bytes: device memory for the cache (None: every prefix)."""

    def __init__(self, scorer: PairScorer, budget_bytes: Optional[int] = None, priority: Optional[Sequence[int]] = None, log=None):
        self.s = scorer
        self.m, self.engine = scorer.m, scorer.engine
        if getattr(self.engine, "dtype", "") == "f8":
            raise ValueError("GalleryIndex: fp8 engines are not supported (use --dtype f16 or bf16)")
        self.budget_bytes = budget_bytes
        self.priority = priority
        self.log = log if log is not None else (lambda msg: print(msg, file=sys.stderr, flush=True))
        # the prompt splits of the texts: (pre, post) pairs, in order of first appearance
        splits: Dict[Tuple[bytes, bytes], Tuple[np.ndarray, np.ndarray]] = {}
        for pre, post, _ in scorer.vtg_split:
            splits.setdefault((pre.tobytes(), post.tobytes()), (pre, post))
        self.splits = splits
        self.keys: List[Tuple[int, bytes, bytes]] = [(j, k[0], k[1]) for j in range(len(scorer.video)) for k in splits]
        self.cache = None
        self.slot_of: Dict[Tuple, int] = {}
        self._state = None
        self._prior: Dict[Tuple, float] = {}       # t2v candidate priors, valid for the (weights, TVG mode) state in _prior_state
        self._prior_state = None
        self.build_seconds = 0.0

    # ---- geometry
    def prefix_len(self, key) -> int:
        j, pre, post = key
        n_vid = int(np.prod(self.s.video[j].shape[-3:-1]))
        return len(np.frombuffer(pre, np.int64)) + n_vid + len(np.frombuffer(post, np.int64))

    def max_len(self) -> int:
        return max(self.prefix_len(k) for k in self.keys)

    def compensated(self) -> bool:
        return self.s.vtg_mode in VTG_SPLIT_MODES

    def slot_positions(self) -> int:
        return -(-self.max_len() // SLOT_ALIGN) * SLOT_ALIGN

    def per_slot_bytes(self) -> int:
        return self.engine.prefix_cache_bytes(1, self.slot_positions(), self.compensated())

    def _mode_state(self):
        mask = self.engine.layer_mask if self.s.vtg_mode == "select" else None
        return (self.engine.weights_version, self.s.vtg_mode, None if mask is None else tuple(int(b) for b in mask), bool(getattr(self.engine, "lo6", False)))

    # ---- numeric mode
    def resolve_mode(self, first_stage=None, seed: int = 0) -> Optional[str]:
        """`--vtg_precise auto` / `select` not yet measured on these weights: measured with the existing calibrator on the gallery's own (video, caption) pairs --
        calibration_pairs of the first-stage v2t scores when given ([N videos, N texts]), else a seeded sample of 256 pairs.  Returns the mode the VTG calls run in."""
        m = self.m
        mode = m.vtg_mode() if hasattr(m, "vtg_mode") else None
        if mode != "auto":
            self.s.set_vtg_mode(mode)
            return self.s.vtg_mode
        from .calibration import calibration_pairs
        Nv, Nt = len(self.s.video), len(self.s.vtg_split)
        if first_stage is not None:             # evaluation()'s sample and confirmation sample (retrieval_utils.evaluation)
            pairs = calibration_pairs(first_stage, 16, n_queries=32, per_query=8)
            confirm = calibration_pairs(first_stage, 16, n_queries=256, per_query=8)
        else:                                   # the same sizes, seeded
            rng = np.random.RandomState(seed)
            flat = rng.choice(Nv * Nt, size=min(2048, Nv * Nt), replace=False)
            both = np.stack([flat // Nt, flat % Nt], axis=1).astype(np.int64)
            pairs, confirm = both[:256], both
        n_eval = Nv * min(16, Nt)
        if getattr(m, "vtg_precise", None) == "select":
            chosen, table = self.s.calibrate_vtg_select(pairs, n_eval=n_eval, confirm_pairs=confirm)
            if chosen == "select":
                m.resolve_vtg("select", np.asarray(table["mask"], dtype=np.uint8))
            else:
                m.resolve_vtg(chosen)
        else:
            chosen, table = self.s.calibrate_vtg(pairs, n_eval=n_eval, confirm_pairs=confirm)
            m.resolve_vtg(chosen)
        self.s.set_vtg_mode(m.vtg_mode())
        return self.s.vtg_mode

    # ---- fill
    def build(self, first_stage=None) -> "GalleryIndex":
        """Resolves the numeric mode, assigns the slots under the budget and fills them in packed calls of up to max_tokens tokens."""
        import time
        import torch
        self.resolve_mode(first_stage)
        t0 = time.perf_counter()
        comp = self.compensated()
        L = self.slot_positions()
        per = self.engine.prefix_cache_bytes(1, L, comp)
        self.slot_of = slot_plan(self.keys, per, self.budget_bytes, self.priority)
        if self.cache is not None:
            self.cache.close(); self.cache = None
        if self.slot_of:
            self.cache = self.engine.prefix_cache(len(self.slot_of), L, comp)
            self._fill(sorted(self.slot_of.items(), key=lambda kv: kv[1]))
        torch.cuda.synchronize()
        self.build_seconds = time.perf_counter() - t0
        self._state = self._mode_state()
        return self

    def _fill(self, items):
        st = _PackState(self.s, "vtg")
        slots: List[int] = []
        self.s.expect([k[0] for k, _ in items], False)
        for key, slot in items:
            j, pre_b, post_b = key
            pre, post = np.frombuffer(pre_b, np.int64), np.frombuffer(post_b, np.int64)
            f = self.s.video_feat(j, False)
            plen = len(pre) + int(f.shape[0]) + len(post)
            if st.n_tok and st.n_tok + plen > self.s.max_tokens:
                self._fill_call(st, slots); st = _PackState(self.s, "vtg"); slots = []
            fo = st.add_feat(f)
            ptoks = np.concatenate([pre, -(1 + fo + np.arange(int(f.shape[0]))), post])
            st.add_seq(ptoks, np.arange(len(ptoks)), np.ones(len(ptoks), np.uint8), None)
            slots.append(slot)
        if slots:
            self._fill_call(st, slots)

    def _fill_call(self, st: _PackState, slots: List[int]):
        import torch
        from .engine import PackedBatch
        dev = self.s.device
        batch = PackedBatch(np.concatenate(st.pos), np.concatenate(st.vis), np.array(st.seq_start), np.array(st.seq_len), device=dev)
        src = torch.from_numpy(np.concatenate(st.tok).astype(np.int32)).to(dev)
        feats = torch.cat(st.feats, dim=0)
        comp = self.compensated()
        self.engine.set_precise(comp, embeds=comp, mlp=True, layers=self.s.vtg_mode == "select")
        try:
            embeds = self.engine.assemble(src, feats)
            self.cache.fill(batch, embeds, np.asarray(slots, np.int32))
        finally:
            self.engine.set_precise(False)

    def _fresh(self):
        """A weight / adapter / mode change since build(): the slots are refilled once (the engine would refuse them: BLIM_ERR_STATE)."""
        if self._state is None:
            self.build()
            return
        mode_before = self.s.vtg_mode
        if hasattr(self.m, "vtg_mode") and self.m.vtg_mode() != "auto":
            self.s.set_vtg_mode(self.m.vtg_mode())
        if self._mode_state() != self._state or self.s.vtg_mode != mode_before:
            self.log(f"gallery: weights or numeric mode changed since the fill ({self._state} -> {self._mode_state()}): refilling {len(self.slot_of)} slots")
            self.build()

    # ---- planning
    def iter_plans(self, pairs: np.ndarray):
        """pairs [P, 2] (video j, text i) -> engine calls; each plan carries pfx_slot (device) and the slots it reads."""
        pairs = np.asarray(pairs, dtype=np.int64)
        s = self.s
        items = s._vtg_items(pairs, False, 0)
        st = _CachedPack(s)
        for (j, _, texts_g, outs_g) in items:
            pre, post, _ = s.vtg_split[texts_g[0]]
            key = (j, pre.tobytes(), post.tobytes())
            slot = self.slot_of.get(key, -1)
            n_vid = int(np.prod(s.video[j].shape[-3:-1])) if slot >= 0 else int(s.video_feat(j, False).shape[0])
            body_tok = sum(max(len(s.vtg_split[i][2]) - 1, 0) for i in texts_g)
            need = body_tok + (0 if slot >= 0 else len(pre) + n_vid + len(post))
            if st.n_tok and st.n_tok + need > s.max_tokens:
                yield st.finish_cached(); st = _CachedPack(s)
            ppos_end = len(pre) + n_vid + len(post)
            if slot >= 0:
                plen = self.cache.slot_len(slot)
                if plen != ppos_end:
                    raise RuntimeError(f"gallery slot {slot} holds {plen} positions, the prefix of video {j} has {ppos_end}")
                st.used.add(slot)
                last, p0 = -(slot + 1), 0
            else:
                fo = st.add_feat(s.video_feat(j, False))
                ptoks = np.concatenate([pre, -(1 + fo + np.arange(n_vid)), post])
                p0 = st.add_seq(ptoks, np.arange(len(ptoks)), np.ones(len(ptoks), np.uint8), None)
                plen = len(ptoks); last = p0 + plen - 1
            for i, outs in zip(texts_g, outs_g):
                resp = s.vtg_split[i][2]
                if s.max_row_len is not None and ppos_end + len(resp) > s.max_row_len:
                    if ppos_end >= s.max_row_len:
                        raise ValueError(f"tokenizer_model_max_length = {s.max_row_len} leaves no response token of text {i} ({ppos_end} prompt + video tokens)")
                    resp = resp[: s.max_row_len - ppos_end]
                body = resp[:-1]
                rows = [last]
                if len(body):
                    s0 = st.add_seq(body, ppos_end + np.arange(len(body)), np.ones(len(body), np.uint8), (p0, plen), slot=slot)
                    rows += list(range(s0, s0 + len(body)))
                st.add_pair(rows, resp.astype(np.int32), outs)
        if st.n_pairs:
            yield st.finish_cached()

    def run(self, plan):
        comp = self.compensated()
        self.engine.set_precise(comp, embeds=comp, mlp=True, layers=self.s.vtg_mode == "select")
        try:
            embeds = self.engine.assemble(plan.src_index, plan.feats)
            return self.cache_or_none().score_vtg(plan.batch, plan.pfx_slot, plan.slots_used, embeds, plan.rows, plan.labels, plan.row_start)
        finally:
            self.engine.set_precise(False)

    def cache_or_none(self):
        if self.cache is None:                       # a budget of zero slots: a one-slot cache that no sequence names keeps the same call path
            self.cache = self.engine.prefix_cache(1, SLOT_ALIGN, self.compensated())
        return self.cache

    # ---- scores
    def vtg_pairs(self, pairs) -> np.ndarray:
        """log P(text i | video j) of arbitrary pairs [P, 2] (video j, text i): PairScorer.vtg, bit for bit, with the cached prefixes."""
        self._fresh()
        out = np.full(len(pairs), np.nan, dtype=np.float32)
        done = [(p.out_index, self.run(p)) for p in self.iter_plans(pairs)]
        for out_index, r in done:
            sc = r.float().cpu().numpy()
            for k, outs in enumerate(out_index):
                out[outs] = sc[k]
        return out

    def vtg_scores(self, texts, cand) -> np.ndarray:
        """t2v query_likelihood of queries `texts` (text indices of the scorer, [Q]) against candidates cand [Q, k] (video indices) -> [Q, k]."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        cand = np.asarray(cand, dtype=np.int64).reshape(len(texts), -1)
        pairs = np.stack([cand.reshape(-1), np.repeat(texts, cand.shape[1])], axis=1)
        return self.vtg_pairs(pairs).reshape(cand.shape)

    def _tvg_state(self):
        """What a TVG score was computed under: the engine's weights (and adapters) and the TVG calls' compensation."""
        m = self.m
        if hasattr(m, "tvg_mode"):
            self.s.set_tvg_mode(m.tvg_mode())               # as evaluation() does for a caller's scorer: follow what the model asks for / has resolved NOW
        return (self.engine.weights_version, self.s.tvg_mode, self.s.split_tvg)

    def _t2v_prior(self, texts, cand) -> np.ndarray:
        """The t2v candidate prior (TVG-CPN) of every (text, video) pair, memoised per the planner's prior key: it does not depend on the query's own tokens.
        The memo holds for one (weights, TVG mode) state: after a weight, adapter or mode change it is dropped and the priors are computed again."""
        s = self.s
        state = self._tvg_state()
        if state != self._prior_state:
            self._prior, self._prior_state = {}, state
        tp = s.m.tvg_prefix_length
        keys = []
        for i, row in zip(texts, cand):
            pr = s.tvg_split[int(i)]
            keys += [(pr[:tp].tobytes(), len(pr), int(pr[-1]), int(j)) for j in row]
        miss = [k for k in dict.fromkeys(keys) if k not in self._prior]
        if miss:
            pairs = np.array([[j, int(i)] for i, row in zip(texts, cand) for j in row], np.int64)
            first = {}
            for p_, k in zip(pairs, keys):
                first.setdefault(k, p_)
            todo = np.array([first[k] for k in miss], np.int64)
            for k, v in zip(miss, s.tvg(todo, cpn=True)):
                self._prior[k] = float(v)
        return np.array([self._prior[k] for k in keys]).reshape(cand.shape)

    def rerank(self, texts, cand, first_stage=None, cpn: bool = False, alpha=(0.0, 0.0), c=(1.0, 1.0, 1.0, 1.0), finetuned: bool = False):
        """The t2v half of training_utils.combine_and_rank for these queries' candidates: blended = c2 * (c0 * query_likelihood + (1 - c0) * candidate) + (1 - c2) *
        first_stage, candidate = the TVG candidate likelihood (minus alpha[0] x its prior with cpn) for fine-tuned checkpoints and zeros for zero-shot ones, as there.
        -> (order [Q, k] of candidate video ids, best first; blended scores in that order)."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        cand = np.asarray(cand, dtype=np.int64).reshape(len(texts), -1)
        ql = self.vtg_scores(texts, cand)
        fs = np.zeros(cand.shape) if first_stage is None else np.asarray(first_stage).reshape(cand.shape)
        if finetuned:
            self._tvg_state()
            pairs = np.stack([cand.reshape(-1), np.repeat(texts, cand.shape[1])], axis=1)
            t2v_cand = self.s.tvg(pairs).reshape(cand.shape)
            if cpn:
                t2v_cand = t2v_cand - alpha[0] * self._t2v_prior(texts, cand)
        else:
            t2v_cand = np.zeros(cand.shape)
        c0, _, c2, _ = c
        t2v_lm = c0 * ql + (1 - c0) * t2v_cand
        blended = c2 * t2v_lm + (1 - c2) * fs
        order = np.argsort(-blended, axis=1, kind="stable")
        return np.take_along_axis(cand, order, 1), np.take_along_axis(blended, order, 1)

    def close(self):
        if self.cache is not None:
            self.cache.close(); self.cache = None


class _CachedPack(_PackState):
    """_PackState plus the cache slot of every sequence (-1: in-batch prefix) and the slots a call reads."""

    def __init__(self, scorer: PairScorer, kind: str = "vtg"):
        super().__init__(scorer, kind)
        self.slot: List[int] = []
        self.used = set()

    def add_seq(self, toks, pos, vis, prefix, own_start=None, slot: int = -1) -> int:
        self.slot.append(int(slot))
        return super().add_seq(toks, pos, vis, prefix, own_start)

    def finish_cached(self):
        import torch
        if self.n_tok == 0:               # every pair of the call reads a cached row only (one-token responses): one dummy token keeps the batch non-empty
            self.add_seq(np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, np.uint8), None)
        plan = self.finish()
        plan.pfx_slot = torch.from_numpy(np.asarray(self.slot, dtype=np.int32)).to(self.s.device)
        plan.slots_used = np.array(sorted(self.used), dtype=np.int32)
        return plan


class TextGalleryIndex:
    """v2t scores of arbitrary (video, text) pairs of a PairScorer's videos and texts, with the texts' caption prompts (the TVG prefixes) cached on the device.

    scorer: the PairScorer whose texts form the gallery and whose videos are the queries.  budget_bytes: device memory for the caption cache (None: every distinct
    prompt).  video_index: a GalleryIndex on the same scorer that serves the VTG leg (log P(text | video)) from its video slots; without one that leg is PairScorer.vtg.
    The caption cache is filled on the first TVG use or by build(): a zero-shot blend has no TVG term and never fills it."""

    def __init__(self, scorer: PairScorer, budget_bytes: Optional[int] = None, video_index: Optional[GalleryIndex] = None, log=None):
        self.s = scorer
        self.m, self.engine = scorer.m, scorer.engine
        if getattr(self.engine, "dtype", "") == "f8":
            raise ValueError("TextGalleryIndex: fp8 engines are not supported (use --dtype f16 or bf16)")
        if video_index is not None and video_index.s is not scorer:
            raise ValueError("TextGalleryIndex: video_index must be built on the same scorer")
        self.budget_bytes = budget_bytes
        self.video_index = video_index
        self.log = log if log is not None else (lambda msg: print(msg, file=sys.stderr, flush=True))
        # one key per distinct caption prompt, in order of first appearance: texts with the same prompt share a slot
        prompts: Dict[bytes, np.ndarray] = {}
        for pr in scorer.tvg_split:
            prompts.setdefault(pr.tobytes(), pr)
        self.prompts = prompts
        self.keys: List[bytes] = list(prompts)
        self.cache = None
        self.slot_of: Dict[bytes, int] = {}
        self._state = None
        self._prior: Dict[Tuple[int, int], float] = {}      # v2t candidate priors (VTG-CPN), valid for the state in _prior_state
        self._prior_state = None
        self.build_seconds = 0.0
        self.exec_tokens = 0                                # packed tokens of the cached TVG calls run so far

    # ---- geometry
    def max_len(self) -> int:
        return max(len(p) for p in self.prompts.values())

    def compensated(self) -> bool:
        return bool(self.s.split_tvg)

    def slot_positions(self) -> int:
        return -(-self.max_len() // SLOT_ALIGN) * SLOT_ALIGN

    def per_slot_bytes(self) -> int:
        return self.engine.prefix_cache_bytes(1, self.slot_positions(), self.compensated())

    def _lo6_tvg(self) -> bool:
        """Whether the TVG calls' second pass runs in e2m3: bf16 engines keep the 16-bit pass for them (Engine.set_precise, tvg=True)."""
        return bool(getattr(self.engine, "lo6", False)) and self.compensated() and getattr(self.engine, "dtype", "") != "bf16"

    def _mode_state(self):
        return (self.engine.weights_version, self.s.tvg_mode, bool(self.s.split_tvg), self._lo6_tvg())

    def _follow_model(self) -> None:
        """As evaluation() does for a caller's scorer: the TVG calls follow what the model asks for / has resolved NOW."""
        if hasattr(self.m, "tvg_mode"):
            self.s.set_tvg_mode(self.m.tvg_mode())

    # ---- numeric mode
    def resolve_mode(self, first_stage=None, seed: int = 0) -> str:
        """`--tvg_precise auto` not yet measured on these weights: measured with PairScorer.calibrate_tvg on the gallery's own (video, text) pairs -- calibration_pairs
        of the first-stage v2t scores when given ([N videos, N texts]), else a seeded sample; the sizes are GalleryIndex.resolve_mode's.  Returns the TVG calls' mode."""
        m = self.m
        if self.compensated() and getattr(m, "tvg_precise", None) == "auto" and hasattr(m, "tvg_resolved") and not m.tvg_resolved():
            from .calibration import calibration_pairs
            Nv, Nt = len(self.s.video), len(self.s.tvg_split)
            if first_stage is not None:
                pairs = calibration_pairs(first_stage, 16, n_queries=32, per_query=8)
                confirm = calibration_pairs(first_stage, 16, n_queries=256, per_query=8)
            else:
                rng = np.random.RandomState(seed)
                flat = rng.choice(Nv * Nt, size=min(2048, Nv * Nt), replace=False)
                both = np.stack([flat // Nt, flat % Nt], axis=1).astype(np.int64)
                pairs, confirm = both[:256], both
            chosen, _ = self.s.calibrate_tvg(pairs, n_eval=Nv * min(16, Nt), confirm_pairs=confirm)
            m.resolve_tvg(chosen)
        self._follow_model()
        return self.s.tvg_mode

    # ---- fill
    def build(self, first_stage=None) -> "TextGalleryIndex":
        """Resolves the TVG calls' mode, assigns the slots under the budget and fills them in packed calls of up to max_tokens tokens."""
        import time
        import torch
        self.resolve_mode(first_stage)
        t0 = time.perf_counter()
        comp = self.compensated()
        L = self.slot_positions()
        per = self.engine.prefix_cache_bytes(1, L, comp)
        self.slot_of = slot_plan(self.keys, per, self.budget_bytes)
        if self.cache is not None:
            self.cache.close(); self.cache = None
        if self.slot_of:
            self.cache = self.engine.prefix_cache(len(self.slot_of), L, comp)
            self._fill(sorted(self.slot_of.items(), key=lambda kv: kv[1]))
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.build_seconds = time.perf_counter() - t0
        self._state = self._mode_state()
        return self

    def _fill(self, items):
        st = _PackState(self.s, "tvg")
        slots: List[int] = []
        for key, slot in items:
            pr = self.prompts[key]
            if st.n_tok and st.n_tok + len(pr) > self.s.max_tokens:
                self._fill_call(st, slots); st = _PackState(self.s, "tvg"); slots = []
            st.add_seq(pr, np.arange(len(pr)), np.ones(len(pr), np.uint8), None)
            slots.append(slot)
        if slots:
            self._fill_call(st, slots)

    def _tvg_options(self) -> None:
        """The options every TVG call of the scorer runs under (PairScorer.run): fill and scoring must agree, the slots record them."""
        s = self.s
        if s.vocab_cm is None and getattr(self.engine, "_vocab_key", None) != s._vocab_key:
            self.engine.set_video_vocab(s._vocab_src)
        self.engine.set_precise(s.split_tvg, embeds=s.split_tvg, mlp=s.tvg_mode != "attn", tvg=True)

    def _fill_call(self, st: _PackState, slots: List[int]):
        import torch
        from .engine import PackedBatch
        dev = self.s.device
        batch = PackedBatch(np.concatenate(st.pos), np.concatenate(st.vis), np.array(st.seq_start), np.array(st.seq_len), device=dev)
        src = torch.from_numpy(np.concatenate(st.tok).astype(np.int32)).to(dev)
        H = self.m.dims.hidden_size
        feats = torch.zeros((1, H * (2 if self.s.split_tvg else 1)), dtype=self.m.dtype, device=dev)          # a caption prompt holds no video token
        self._tvg_options()
        try:
            embeds = self.engine.assemble(src, feats)
            self.cache.fill(batch, embeds, np.asarray(slots, np.int32))
        finally:
            self.engine.set_precise(False)

    def _fresh(self):
        """A weight / adapter / TVG mode change since build(): the slots are refilled once (the engine would refuse them: BLIM_ERR_STATE)."""
        if self._state is None:
            self.build()
            return
        self._follow_model()
        if self._mode_state() != self._state:
            self.log(f"text gallery: weights or TVG mode changed since the fill ({self._state} -> {self._mode_state()}): refilling {len(self.slot_of)} slots")
            self.build()

    # ---- planning
    def iter_plans(self, pairs: np.ndarray):
        """pairs [P, 2] (video j, text i) -> engine calls, planned as PairScorer._plan_tvg's likelihood branch: the candidates of one text are merged sequences of up to
        SEG_MAX // (C - 1) videos' clip tokens (own_start).  A cached text packs no prompt: its sequences name the slot and each pair's first row is -(slot + 1)."""
        pairs = np.asarray(pairs, dtype=np.int64)
        s = self.s
        C = s.num_clips
        per = max(C - 1, 1)
        order = np.lexsort((pairs[:, 0], pairs[:, 1]))
        s.expect(pairs[order, 0], True)
        groups: List[Tuple[int, List[int]]] = []
        for idx in order:
            i = int(pairs[idx, 1])
            if not groups or groups[-1][0] != i:
                groups.append((i, []))
            groups[-1][1].append(int(idx))
        st = _CachedPack(s, "tvg")
        for i, idxs in groups:
            pr = s.tvg_split[i]
            plen = len(pr)
            slot = self.slot_of.get(pr.tobytes(), -1)
            if slot >= 0:
                held = self.cache.slot_len(slot)
                if held != plen:
                    raise RuntimeError(f"text gallery slot {slot} holds {held} positions, the caption prompt of text {i} has {plen}")
            pos_in, p0 = 0, None
            while pos_in < len(idxs):
                own = lambda: plen if (slot < 0 and p0 is None) else 0          # prompt tokens this text still has to pack into the call
                room = (s.max_tokens - st.n_tok - own()) // per
                if (st.n_tok and room < 1) or (C == 1 and st.n_pairs >= s.max_tokens):      # (C == 1, every text cached: rows alone fill a call)
                    yield st.finish_cached(); st = _CachedPack(s, "tvg"); p0 = None
                    room = (s.max_tokens - own()) // per
                n = max(1, min(len(idxs) - pos_in, room, SEG_MAX // per))
                if slot >= 0:
                    st.used.add(slot)
                    first, pfx = -(slot + 1), (0, plen)
                else:
                    if p0 is None:                       # the prompt is packed once per engine call; every merged sequence of the text names it
                        p0 = st.add_seq(pr, np.arange(plen), np.ones(plen, np.uint8), None)
                    first, pfx = p0 + plen - 1, (p0, plen)
                chunk = idxs[pos_in:pos_in + n]
                s0 = None
                if C > 1:
                    toks, own_start = [], []
                    for m_, idx in enumerate(chunk):
                        fo = st.add_feat(s.video_feat(int(pairs[idx, 0]), True))
                        toks.append(-(1 + fo + np.arange(C - 1)))
                        own_start.append(np.full(C - 1, m_ * (C - 1), np.int32))
                    s0 = st.add_seq(np.concatenate(toks), np.tile(plen + np.arange(C - 1), n), np.ones(n * (C - 1), np.uint8), pfx,
                                    own_start=np.concatenate(own_start), slot=slot)
                for m_, idx in enumerate(chunk):
                    rows = [first]
                    if C > 1:
                        rows += list(range(s0 + m_ * (C - 1), s0 + (m_ + 1) * (C - 1)))
                    else:
                        s.video_feat(int(pairs[idx, 0]), True)
                    st.add_pair(rows, np.array([s.tvg_video_labels[int(pairs[idx, 0])]], np.int32), np.array([idx]))
                pos_in += n
        if st.n_pairs:
            yield st.finish_cached()

    def run(self, plan):
        self.exec_tokens += plan.n_tokens
        self._tvg_options()
        try:
            embeds = self.engine.assemble(plan.src_index, plan.feats)
            return self.cache_or_none().score_tvg(plan.batch, plan.pfx_slot, plan.slots_used, embeds, plan.rows, self.s.vocab_cm, plan.labels)
        finally:
            self.engine.set_precise(False)

    def cache_or_none(self):
        if self.cache is None:                       # a budget of zero slots: a one-slot cache that no sequence names keeps the same call path
            self.cache = self.engine.prefix_cache(1, SLOT_ALIGN, self.compensated())
        return self.cache

    # ---- scores
    def tvg_pairs(self, pairs) -> np.ndarray:
        """log P(video j | text i) of arbitrary pairs [P, 2] (video j, text i): PairScorer.tvg with the caption prompts read from the cache."""
        self._fresh()
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        out = np.full(len(pairs), np.nan, dtype=np.float32)
        done = [(p.out_index, self.run(p)) for p in self.iter_plans(pairs)]
        for out_index, r in done:
            sc = r.float().cpu().numpy()
            for k, outs in enumerate(out_index):
                out[outs] = sc[k]
        return out

    def vtg_pairs(self, pairs) -> np.ndarray:
        """log P(text i | video j): from the video index's slots when there is one, else PairScorer.vtg."""
        if self.video_index is not None:
            return self.video_index.vtg_pairs(pairs)
        m = self.m
        if hasattr(m, "vtg_mode") and m.vtg_mode() != "auto":
            self.s.set_vtg_mode(m.vtg_mode())
        return self.s.vtg(pairs)

    def _vtg_state(self):
        """What a VTG prior was computed under: the weights (and adapters), the VTG calls' mode, its layer mask and the second pass."""
        m = self.m
        if hasattr(m, "vtg_mode") and m.vtg_mode() != "auto":
            self.s.set_vtg_mode(m.vtg_mode())
        mask = getattr(self.engine, "layer_mask", None) if self.s.vtg_mode == "select" else None
        return (self.engine.weights_version, self.s.vtg_mode, None if mask is None else tuple(int(b) for b in mask), bool(getattr(self.engine, "lo6", False)))

    def v2t_prior(self, videos, cand) -> np.ndarray:
        """The v2t candidate prior (VTG-CPN) of every (video, text) pair: it depends on the text and on the video's token count only, so it is memoised per
        (text, token count) for one (weights, VTG mode, layer mask, second pass) state; misses are scored with PairScorer.vtg(..., cpn=True)."""
        s = self.s
        state = self._vtg_state()
        if state != self._prior_state:
            self._prior, self._prior_state = {}, state
        n_vid = lambda j: int(np.prod(s.video[int(j)].shape[-3:-1]))
        videos = np.asarray(videos, dtype=np.int64).reshape(-1)
        cand = np.asarray(cand, dtype=np.int64).reshape(len(videos), -1)
        keys = [(int(i), n_vid(j)) for j, row in zip(videos, cand) for i in row]
        first: Dict[Tuple[int, int], int] = {}
        for (j, row) in zip(videos, cand):
            for i in row:
                first.setdefault((int(i), n_vid(j)), int(j))
        miss = [k for k in dict.fromkeys(keys) if k not in self._prior]
        for nv in sorted({k[1] for k in miss}):              # one pass per token count (PairScorer._vtg_items refuses a mixed one)
            part = [k for k in miss if k[1] == nv]
            todo = np.array([[first[k], k[0]] for k in part], np.int64)
            for k, v in zip(part, s.vtg(todo, cpn=True)):
                self._prior[k] = v
        return np.array([self._prior[k] for k in keys], dtype=np.float32).reshape(cand.shape)

    def rerank(self, videos, cand, first_stage=None, cpn: bool = False, alpha=(0.0, 0.0), c=(1.0, 1.0, 1.0, 1.0), finetuned: bool = False):
        """The v2t half of training_utils.combine_and_rank for these query videos' candidate texts: blended = c3 * (c1 * query_likelihood + (1 - c1) *
        (candidate_likelihood - alpha[1] * candidate_prior)) + (1 - c3) * first_stage; candidate_likelihood is VTG (log P(text | video)), query_likelihood TVG
        (log P(video | text)).  Zero-shot: the likelihood term is the (debiased) candidate likelihood alone and no TVG call is made, as there.
        -> (order [Q, k] of candidate text ids, best first; blended scores in that order)."""
        videos = np.asarray(videos, dtype=np.int64).reshape(-1)
        cand = np.asarray(cand, dtype=np.int64).reshape(len(videos), -1)
        pairs = np.stack([np.repeat(videos, cand.shape[1]), cand.reshape(-1)], axis=1)
        v2t_cand = self.vtg_pairs(pairs).reshape(cand.shape)
        fs = np.zeros(cand.shape) if first_stage is None else np.asarray(first_stage).reshape(cand.shape)
        if cpn:
            v2t_cand = v2t_cand - alpha[1] * self.v2t_prior(videos, cand)
        _, c1, _, c3 = c
        v2t_lm = c1 * self.tvg_pairs(pairs).reshape(cand.shape) + (1 - c1) * v2t_cand if finetuned else v2t_cand
        blended = c3 * v2t_lm + (1 - c3) * fs
        order = np.argsort(-blended, axis=1, kind="stable")
        return np.take_along_axis(cand, order, 1), np.take_along_axis(blended, order, 1)

    def close(self):
        if self.cache is not None:
            self.cache.close(); self.cache = None
