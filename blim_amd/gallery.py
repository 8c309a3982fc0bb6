"""Search policy over cached prefixes: what is ranked, by which stages, and how the terms are blended.  Which prefix holds a cache slot, and how slots are
filled, admitted, evicted, spilled and restored, is blim_amd/prefix_index.py (`_PrefixIndex`, imported here; it does not import this module).

The two directions.  `GalleryIndex` (t2v `query_likelihood`, log P(text | video)): a VTG likelihood runs the video's `[header][video][instruction]` prefix through
every layer before the text's response tokens, and the prefix does not depend on the query.  One slot per (video j, pre, post) -- the grouping
`PairScorer._vtg_items` uses -- holds the K / V of every layer and the last prefix row's final-norm hidden state; a query's pairs are then packed as their response
tokens alone (`blim_score_vtg_cached`), and the scores are bit for bit those of `PairScorer.vtg` on the same pairs.  `TextGalleryIndex` (v2t):
the gallery is the scorer's texts, a query is a video.  The v2t `query_likelihood` is TVG, log P(video | text); its prefix is the text's caption prompt.  One slot
per distinct prompt; a query's pairs are packed as the video's num_clips - 1 clip tokens alone (`blim_score_tvg_cached`).  DESIGN.md section 11.

The request type.  `SearchRequest`: a text over candidates it names, or over the best `shortlist` = K videos of the gallery's TVG ranking, which `prefilter` = K0
narrows first and `within` confines to a set of the caller's.  `check_shortlist` and `check_within` state the K / K0 rule and the set's rule
once; `GalleryIndex.search_requests` scores requests of unequal candidate counts as one pass.

The stages.  Stage 1, the shortlist, needs no first stage on a fine-tuned checkpoint: `GalleryIndex.shortlist` ranks the whole gallery by
the TVG candidate term of the blend (`PairScorer.tvg_gallery`: fixed chunks, so a value depends on its text and the gallery alone), and `search_requests` reranks
the best K with that term reused; `TextGalleryIndex.shortlist` / `rerank_shortlist` are the v2t form over the cached caption prompts.  Stage 0, the prefilter
(sections 21 and 22), narrows the gallery first: `GalleryIndex.prefilter` by the clip-0 term of the prompt's row, `TextGalleryIndex.prefilter` by the clip-0 term of
every caption for all query videos from the slots' stored hidden rows.  A removed video (section 24) is never ranked: its stage-1 column is NaN.

The blends.  `rerank` / `_blend` are the two halves of training_utils.combine_and_rank; every memo of a TVG value (`_t2v_prior`) is keyed by the scorer's
`vocab_version` -- a video that joins or leaves moves the softmax normaliser of every TVG score -- while the v2t prior is kept per (text, token count).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .calibration import VTG_SPLIT_MODES
from .engine import TVG_RANK_MAX_K
from .pair_scorer import SEG_MAX, PairScorer                   # noqa: F401  (SEG_MAX: the planner's bound, named here too)
from .prefix_index import (SLOT_ALIGN, GalleryStats, HostStats, HostTier, _Pass, _PrefixIndex, cache_bytes, slot_plan,      # noqa: F401  (the residency core, under
                           _device_bytes, _device_sync, _pinned_bytes)                                                      # the names it always had in this module)


class _RequestFields(NamedTuple):
    text: int
    cand: Optional[Sequence[int]] = None
    first_stage: Optional[Sequence[float]] = None
    shortlist: Optional[int] = None
    prefilter: Optional[int] = None


_KEEP = object()


class SearchRequest(_RequestFields):
    """One request of GalleryIndex.search_requests: a text over candidates it names (`cand`, with an optional `first_stage` parallel to them) or over the best
    `shortlist` = K videos of the gallery's TVG ranking, which `prefilter` = K0 >= K narrows first.  A plain tuple of the first three, four or five fields is the same
    request.  `within` (video indices, each once) confines a shortlist request to a set of the caller's: it is ranked inside the set alone, K and K0 clipped to
    the set's size.  It is the sixth field, given by keyword -- SearchRequest(t, shortlist=K, within=ids) --, and rides beside the five-field tuple, so a request
    still unpacks to, and compares as, the five fields it always had.  What follows from that: `==` and `hash` do not see `within` (two requests that differ in
    their sets alone compare equal), and `_fields` / `_asdict()` list the five fields without it.  `_replace` keeps the set unless `within=` is given; `_make`
    takes it as a keyword; a request built by either without one has `within` None, as every request had."""
    within = None                                  # (the default of every construction path, tuple.__new__ included)

    def __new__(cls, *fields, within=None, **named):
        self = super().__new__(cls, *fields, **named)
        self.within = within
        return self

    @classmethod
    def _make(cls, iterable, within=None):
        self = super()._make(iterable)
        self.within = within
        return self

    def _replace(self, within=_KEEP, **named):
        out = super()._replace(**named)
        out.within = self.within if within is _KEEP else within
        return out

    def __repr__(self):
        return super().__repr__() if self.within is None else f"{super().__repr__()[:-1]}, within={self.within!r})"


def check_within(within, n_videos: int) -> np.ndarray:
    """The rule of a request's set, stated once: non-empty, integer video indices in 0 .. n_videos - 1, none twice.  -> the set ASCENDING, int64 (position order is
    then the whole gallery's tie order); ValueError names the rule."""
    try:
        raw = np.asarray(within)
        w = raw.astype(np.int64).reshape(-1)
        whole = raw.dtype != bool and bool((w == raw.reshape(-1)).all())
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError("within: a list of integer video indices")
    if len(w) == 0:
        raise ValueError("within: an empty set of videos")
    if w.min() < 0 or w.max() >= n_videos:
        raise ValueError(f"within: video index {int(w.min() if w.min() < 0 else w.max())} outside 0 .. {int(n_videos) - 1}")
    w = np.sort(w)
    if (w[1:] == w[:-1]).any():
        raise ValueError(f"within: video index {int(w[1:][w[1:] == w[:-1]][0])} named twice")
    return w


def check_shortlist(K, K0, n_videos: int) -> Tuple[Optional[int], Optional[int]]:
    """The K / K0 rule, stated once: a shortlist keeps K candidates (None: GalleryIndex.prefilter, a stage 0 on its own), a prefilter keeps K0 videos for it (None:
    no prefilter); both are positive integers, K0 is at least K and, clipped to the gallery's n_videos, at most the rank kernel's BLIM_TVG_RANK_MAX_K.
    -> (K, K0 clipped to n_videos), None where None was given; ValueError."""
    positive = lambda x: not isinstance(x, bool) and int(x) == x and int(x) >= 1
    if K0 is not None and not positive(K0):
        raise ValueError(f"prefilter K0 = {K0!r}: a positive integer")
    if K is not None and not positive(K):
        raise ValueError(f"shortlist k = {K!r}: a positive integer")
    if K is not None and K0 is not None and K0 < K:
        raise ValueError(f"prefilter K0 = {K0} below the shortlist's K = {K}: K0 must be at least the shortlist's K = {K}")
    if K0 is not None and min(int(K0), int(n_videos)) > TVG_RANK_MAX_K:
        raise ValueError(f"prefilter K0 = {min(int(K0), int(n_videos))} above the rank kernel's limit of {TVG_RANK_MAX_K} (BLIM_TVG_RANK_MAX_K)")
    return None if K is None else int(K), None if K0 is None else min(int(K0), int(n_videos))


def request_pairs(queries, cands, query_col: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """One query index and one candidate list per request -> (the [P, 2] (video j, text i) pairs, request by request in candidate order; the points that split a [P]
    result back into the requests).  query_col: the column of the query -- 1, a text over candidate videos (t2v); 0, a video over candidate texts (v2t)."""
    cands = [np.asarray(cand, dtype=np.int64).reshape(-1) for cand in cands]
    lens = [len(cand) for cand in cands]
    query = np.repeat(np.asarray(queries, dtype=np.int64).reshape(-1), lens)
    flat = np.concatenate(cands) if cands else np.zeros(0, np.int64)
    return np.stack([flat, query] if query_col else [query, flat], axis=1), np.cumsum(lens)[:-1]


def grid_pairs(queries, cand, query_col: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """request_pairs for queries [Q] with k candidates each, cand [Q, k] -> (queries, cand, as int64 arrays; the [Q * k, 2] pairs, whose results reshape(cand.shape))."""
    queries = np.asarray(queries, dtype=np.int64).reshape(-1)
    cand = np.asarray(cand, dtype=np.int64).reshape(len(queries), -1)
    return queries, cand, request_pairs(queries, cand, query_col)[0]


def _follow_vtg(s: PairScorer) -> None:
    """As evaluation() does for a caller's scorer: the VTG calls follow what the model has resolved NOW (an unresolved `auto` leaves the scorer's mode)."""
    if hasattr(s.m, "vtg_mode") and s.m.vtg_mode() != "auto":
        s.set_vtg_mode(s.m.vtg_mode())


def _vtg_state(s: PairScorer):
    """What a VTG score is computed under: the weights (and adapters), the VTG calls' mode, its layer mask and the second pass."""
    mask = getattr(s.engine, "layer_mask", None) if s.vtg_mode == "select" else None
    return (s.engine.weights_version, s.vtg_mode, None if mask is None else tuple(int(b) for b in mask), bool(getattr(s.engine, "lo6", False)))


class GalleryIndex(_PrefixIndex):
    """t2v VTG scores of arbitrary (video, text) pairs of a PairScorer's videos and texts, with the videos' prefixes cached on the device.

    scorer: the PairScorer whose videos form the gallery and whose texts are the queries (dataset captions and / or free-text queries packed by the same prompt
    builder); its prompt splits (vtg_split) and projected video features are reused.  budget_bytes: device memory for the cache (None: every prefix)."""
    kind, _changed = "vtg", "gallery: weights or numeric mode"

    def __init__(self, scorer: PairScorer, budget_bytes: Optional[int] = None, priority: Optional[Sequence[int]] = None, log=None, fill: str = "eager",
                 host_budget_bytes: Optional[int] = None, spare_slots: int = 0):
        super().__init__(scorer, budget_bytes, priority, log, fill, host_budget_bytes, spare_slots)
        # the prompt splits of the texts: (pre, post) pairs, in order of first appearance; one key per (video, split), video-major for the texts given here
        self.splits: Dict[Tuple[bytes, bytes], Tuple[np.ndarray, np.ndarray]] = {}
        self.keys: List[Tuple[int, bytes, bytes]] = []
        self._split_id = np.zeros(0, dtype=np.int64)
        self._sync_texts()
        self.shortlist_stats = {"queries": 0, "passes": 0, "pairs": 0}      # texts shortlisted, stage-1 passes (one tvg_gallery each), the (text, video) pairs those scored
        self.prefilter_stats = {"queries": 0, "passes": 0, "rows": 0, "kept": 0}   # texts prefiltered, stage-0 passes (one tvg_first each), the logits rows those ranked, the videos kept
        self.within_stats = {"queries": 0, "candidates": 0}                  # texts searched inside a set of the caller's, the videos those sets held

    def _count_texts(self) -> int:
        return len(self.s.vtg_split)

    def _grow(self, lo: int, hi: int) -> None:
        """Texts lo .. hi - 1 joined: their split ids, and one key per video for every (pre, post) the index has not seen, appended."""
        at = {k: n for n, k in enumerate(self.splits)}
        new, ids = [], []
        for pre, post, _ in self.s.vtg_split[lo:hi]:
            k = (pre.tobytes(), post.tobytes())
            if k not in at:
                at[k] = len(at); self.splits[k] = (pre, post); new.append(k)
            ids.append(at[k])
        dead = self.s.removed                        # (a removed video has no key, under a new split either)
        videos = [j for j in range(self._n_videos) if j not in dead]     # (the videos the keys cover: one that joined since brings its keys in _sync_videos)
        self.keys += [(j, k[0], k[1]) for j in videos for k in new] if not self.keys else [(j, k[0], k[1]) for k in new for j in videos]
        self._split_id = np.concatenate([self._split_id, np.asarray(ids, dtype=np.int64)])

    def _video_keys(self, lo: int, hi: int) -> List:
        """Videos lo .. hi - 1 joined: one key per (new video, known split), new videos outermost."""
        dead = self.s.removed                        # (a video that joined and left again before the index looked brings none)
        return [(j, k[0], k[1]) for j in range(lo, hi) if j not in dead for k in self.splits]

    def _forget_videos(self, gone) -> None:
        """The keys of the videos `gone` leave the key list the planners walk, slot_of -- their slots are free at once: the eager fill of _sync_videos and the lazy
        admission of _begin_pass take any slot no key holds --, the recency stamps and the host tier (HostTier.forget: a later restore cannot resurrect them)."""
        mine = [k for k in self.keys if k[0] in gone]
        if not mine:
            return
        self.keys = [k for k in self.keys if k[0] not in gone]
        for k in mine:
            if self.slot_of.pop(k, None) is not None:
                self.removed_stats["slots_freed"] += 1
            self._stamp.pop(k, None)
            if self.host is not None and self.host.forget(k):
                self.removed_stats["records_forgotten"] += 1

    def prefix_len(self, key) -> int:
        j, pre, post = key
        n_vid = int(np.prod(self.s.video[j].shape[-3:-1]))
        return len(np.frombuffer(pre, np.int64)) + n_vid + len(np.frombuffer(post, np.int64))

    def _prefix(self, key):
        """-> (tokens before the video, the video's projected rows, tokens after it)."""
        j, pre, post = key
        return np.frombuffer(pre, np.int64), self.s.video_feat(j, False), np.frombuffer(post, np.int64)

    def _fill(self, items):
        self.s.expect([k[0] for k, _ in items], False)
        super()._fill(items)

    def compensated(self) -> bool:
        return self.s.vtg_mode in VTG_SPLIT_MODES

    def _mode_state(self):
        return _vtg_state(self.s)

    def _follow_model(self) -> bool:
        """-> whether following the model changed the scorer's mode under the index (then the slots are refilled whatever they recorded)."""
        before = self.s.vtg_mode
        _follow_vtg(self.s)
        return self.s.vtg_mode != before

    # ---- numeric mode
    def resolve_mode(self, first_stage=None, seed: int = 0) -> Optional[str]:
        """`--vtg_precise auto` / `select` not yet measured on these weights: measured with the existing calibrator on the gallery's own (video, caption) pairs --
        calibration_pairs of the first-stage v2t scores when given ([N videos, N texts]), else a seeded sample of 256 pairs.  Returns the mode the VTG calls run in."""
        m = self.m
        mode = m.vtg_mode() if hasattr(m, "vtg_mode") else None
        if mode != "auto":
            self.s.set_vtg_mode(mode)
            return self.s.vtg_mode
        pairs, confirm, n_eval = self._calibration_sample(first_stage, seed, len(self.s.vtg_split))
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

    # ---- planning
    def _needs(self, pairs: np.ndarray) -> List:
        """The (video, pre, post) keys of a pass, in the order _vtg_items forms their groups: by video, then by text."""
        if not len(pairs):
            return []
        order = np.lexsort((pairs[:, 1], pairs[:, 0]))
        S, split = len(self.splits), list(self.splits)
        code = (pairs[:, 0] * S + self._split_id[pairs[:, 1]])[order]
        _, first = np.unique(code, return_index=True)
        return [(int(c) // S,) + split[int(c) % S] for c in code[np.sort(first)]]

    def _plans(self, pairs: np.ndarray):
        """pairs [P, 2] (video j, text i) -> engine calls, planned by PairScorer._pack_vtg over this index's slots; each plan carries pfx_slot (device) and the
        slots it reads."""
        s = self.s
        yield from s._pack_vtg(s._vtg_items(np.asarray(pairs, dtype=np.int64), False, 0), slots=self)

    # ---- scores
    def vtg_pairs(self, pairs) -> np.ndarray:
        """log P(text i | video j) of arbitrary pairs [P, 2] (video j, text i): PairScorer.vtg, bit for bit, with the cached prefixes."""
        return self._scores(pairs)

    def vtg_scores(self, texts, cand) -> np.ndarray:
        """t2v query_likelihood of queries `texts` (text indices of the scorer, [Q]) against candidates cand [Q, k] (video indices) -> [Q, k]."""
        _, cand, pairs = grid_pairs(texts, cand)
        return self.vtg_pairs(pairs).reshape(cand.shape)

    def _tvg_state(self):
        """What a TVG score was computed under: the engine's weights (and adapters), the TVG calls' compensation and the video vocabulary its softmax runs over
        (PairScorer.vocab_version: a video that joins moves the normaliser of every TVG score, the priors included)."""
        m = self.m
        if hasattr(m, "tvg_mode"):
            self.s.set_tvg_mode(m.tvg_mode())               # as evaluation() does for a caller's scorer: follow what the model asks for / has resolved NOW
        return (self.engine.weights_version, self.s.tvg_mode, self.s.split_tvg, self.s.vocab_version)

    def _t2v_prior(self, texts, cand) -> np.ndarray:
        """The t2v candidate prior (TVG-CPN) of every (text, video) pair, memoised per the planner's prior key: it does not depend on the query's own tokens.
        The memo holds for one (weights, TVG mode, vocabulary) state: after a weight, adapter or mode change, or when videos join (add_videos), it is dropped and
        the priors are computed again."""
        s = self.s
        state = self._tvg_state()
        if state != self._prior_state:
            self._prior, self._prior_state = {}, state
        tp = s.m.tvg_prefix_length
        s._need_tvg(texts)
        keys = []
        for i, row in zip(texts, cand):                                 # (rows of any lengths: rerank_requests hands in ragged candidate lists)
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
        out = np.array([self._prior[k] for k in keys])
        return out.reshape(cand.shape) if isinstance(cand, np.ndarray) else out

    def rerank(self, texts, cand, first_stage=None, cpn: bool = False, alpha=(0.0, 0.0), c=(1.0, 1.0, 1.0, 1.0), finetuned: bool = False):
        """The t2v half of training_utils.combine_and_rank for these queries' candidates: blended = c2 * (c0 * query_likelihood + (1 - c0) * candidate) + (1 - c2) *
        first_stage, candidate = the TVG candidate likelihood (minus alpha[0] x its prior with cpn) for fine-tuned checkpoints and zeros for zero-shot ones, as there.
        -> (order [Q, k] of candidate video ids, best first; blended scores in that order)."""
        texts, cand, pairs = grid_pairs(texts, cand)
        ql = self.vtg_scores(texts, cand)
        fs = np.zeros(cand.shape) if first_stage is None else np.asarray(first_stage).reshape(cand.shape)
        if finetuned:
            self._tvg_state()
            t2v_cand = self.s.tvg(pairs).reshape(cand.shape)
            if cpn:
                t2v_cand = t2v_cand - alpha[0] * self._t2v_prior(texts, cand)
        else:
            t2v_cand = np.zeros(cand.shape)
        return self._blend(cand, ql, t2v_cand, fs, c)

    @staticmethod
    def _blend(cand, ql, t2v_cand, fs, c):
        """cand, query likelihood, candidate likelihood and first stage, [Q, k] each -> (candidates best first, their blended scores)."""
        c0, _, c2, _ = c
        t2v_lm = c0 * ql + (1 - c0) * t2v_cand
        blended = c2 * t2v_lm + (1 - c2) * fs
        order = np.argsort(-blended, axis=1, kind="stable")
        return np.take_along_axis(cand, order, 1), np.take_along_axis(blended, order, 1)

    def rerank_requests(self, requests, cpn: bool = False, alpha=(0.0, 0.0), c=(1.0, 1.0, 1.0, 1.0), finetuned: bool = False):
        """rerank() for requests of unequal sizes, scored together: requests = [(text index, candidate video indices [k_q], first_stage [k_q] or None)].  The pairs of
        all requests are ONE vtg_pairs pass (one pass of a lazy index: its needed keys pinned, its misses admitted under section 12's policy) and, for fine-tuned
        checkpoints, one PairScorer.tvg call and one prior lookup; the blend is rerank()'s, per request.  A VTG score does not depend on what shares its call, so the
        query likelihood is bit for bit that of rerank() per request.  -> [(order [k_q], blended [k_q])] in request order.  (search_requests with no shortlist request: a request without candidates is
        refused there.)"""
        return self.search_requests([(t, cand, fs) for t, cand, fs in requests], cpn=cpn, alpha=alpha, c=c, finetuned=finetuned)

    # ---- the shortlist: the gallery ranked by the TVG candidate term, the best K reranked
    def _stage1(self, texts, cpn: bool, alpha) -> np.ndarray:
        """-> [Q, N]: the candidate term of rerank()'s fine-tuned blend for every video of the gallery -- PairScorer.tvg_gallery (one pass for all texts), minus
        alpha[0] x the candidate prior with cpn.  A text without a TVG row is refused by name."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        self.s._need_tvg(texts)
        self._tvg_state()
        stage = self.s.tvg_gallery(texts)
        lv = self.s.live_videos()                    #  index-space columns, NaN in a removed one; the prior is looked up for live videos only
        st = self.shortlist_stats
        st["queries"] += len(texts); st["passes"] += 1; st["pairs"] += len(np.unique(texts)) * len(lv)
        if cpn:
            prior = self._t2v_prior(texts, np.tile(lv, (len(texts), 1)))
            out = np.full(stage.shape, np.nan, dtype=np.result_type(stage, prior))
            out[:, lv] = stage[:, lv] - alpha[0] * prior
            stage = out
        return stage

    @staticmethod
    def _best(stage: np.ndarray, k: int):
        """One text's stage-1 row [N] -> (the best min(k, N) videos, their values): descending, ties to the lower video index.  A removed video's column is NaN
        (section 24): it sorts behind every value and is cut off, so N counts the live columns and a removed index is never returned."""
        order = np.argsort(-stage, kind="stable")[:max(min(int(k), len(stage) - int(np.isnan(stage).sum())), 0)]
        return order.astype(np.int64), stage[order]

    def shortlist(self, texts, k: int, cpn: bool = False, alpha=(0.0, 0.0)):
        """The whole gallery ranked by the TVG candidate term of each text: -> (cand [Q, min(k, N)] video indices, best first; their stage-1 scores)."""
        k, _ = check_shortlist(k, None, self.s.n_live)
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        stage = self._stage1(texts, cpn, alpha)
        best = [self._best(row, k) for row in stage]
        k = min(int(k), self.s.n_live)
        return (np.stack([b[0] for b in best]) if best else np.zeros((0, k), np.int64),
                np.stack([b[1] for b in best]) if best else np.zeros((0, k), stage.dtype))

    # ---- the prefilter: the gallery ranked on the device by the clip-0 summand of the TVG score, the best K0 kept for the likelihood
    def prefilter(self, texts, k0: int, cpn: bool = False, alpha=(0.0, 0.0), within=None):
        """The K0 videos of each text that log P(clip 0 of the video | text) ranks first (minus alpha[0] x the candidate prior's clip-0 term with cpn): ONE
        PairScorer.tvg_first pass for all texts, one logits row per distinct prompt whatever the gallery's size.  -> cand [Q, min(k0, N)] video indices, ASCENDING
        (a set: what ranks it is stage 1).  ValueError as check_shortlist.
        within: one set of video indices per text (check_within's rule) -- text q keeps the min(k0, len(within[q])) videos OF ITS SET that the same values rank
        first, still one pass and one row per distinct prompt.  -> a list of Q ascending arrays, one per text."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        if within is not None:
            if len(within) != len(texts):
                raise ValueError(f"prefilter: within holds {len(within)} sets for {len(texts)} texts")
            sets = [check_within(w, len(self.s.video)) for w in within]
            for w in sets:
                self.s._need_live(w)
            k0s = [check_shortlist(None, k0, len(w))[1] for w in sets]
            self.within_stats["queries"] += len(texts); self.within_stats["candidates"] += int(sum(len(w) for w in sets))
            return self._stage0(texts, k0s, cpn, alpha, within=sets)
        _, k0 = check_shortlist(None, k0, self.s.n_live)
        kept = self._stage0(texts, [k0] * len(texts), cpn, alpha)
        return np.stack(kept) if kept else np.zeros((0, k0), np.int64)

    def _stage0(self, texts, k0s, cpn: bool, alpha, within=None) -> List[np.ndarray]:
        """ONE stage-0 pass at the largest K0 (checked and clipped by the caller): text q keeps the first k0s[q] of its own order -- a smaller K0's survivors are a
        prefix of a larger one's -- sorted ascending.  within: text q's own set (checked by the caller, k0s[q] <= its size): its order is then the set's alone."""
        texts = np.asarray(texts, dtype=np.int64).reshape(-1)
        if not len(texts):
            return []
        self.s._need_tvg(texts)
        self._tvg_state()
        more = {} if within is None else {"within": within}
        idx, _ = self.s.tvg_first(texts, max(k0s), cpn=cpn, alpha=float(alpha[0]), **more)
        st = self.prefilter_stats
        st["queries"] += len(texts); st["passes"] += 1; st["rows"] += len(np.unique(texts)); st["kept"] += int(sum(k0s))
        return [np.sort(row[:k]) for row, k in zip(idx, k0s)]

    def search_requests(self, requests, cpn: bool = False, alpha=(0.0, 0.0), c=(1.0, 1.0, 1.0, 1.0), finetuned: bool = False):
        """rerank_requests() with requests that may take their candidates from the shortlist: requests = SearchRequest objects or plain tuples of their first three,
        four or five fields (text index, candidate video indices [k_q] or None, first_stage [k_q] or None, shortlist K or None, prefilter K0 or None), exactly one of
        candidates and K per request.  A request with candidates is rerank_requests' (its TVG term one PairScorer.tvg call over the explicit requests' pairs).  The
        shortlist requests of the batch share ONE stage-1 pass (_stage1) over the whole gallery; each keeps its best K videos as candidates, its first-stage term is
        zero, and the TVG candidate term of its blend IS its stage-1 value: it is not computed a second time.  A shortlist request with a `prefilter` K0 >= K is
        narrowed first: the prefiltered requests of the batch share ONE stage-0 pass (prefilter, at the largest K0: a smaller K0's survivors are the first K0 of the
        same order); their stage-1 terms are ONE PairScorer.tvg call over their surviving pairs (minus alpha[0] x the prior over those K0 candidates with cpn), of
        which each keeps its best K as a shortlist request does.  A shortlist request with `within` (SearchRequest's keyword) is ranked inside
        that set alone: those with a K0 share ONE stage-0 pass of their own (PairScorer.tvg_first(within=), K0 clipped to the set), the others keep their whole set,
        and ONE PairScorer.tvg call scores what was kept.  All requests then share ONE vtg_pairs pass (one pass of a lazy index).
        -> [(order [k_q], blended [k_q])] in request order."""
        reqs = self._checked(requests, finetuned)
        if not reqs:
            return []
        cands, terms = self._chosen(reqs, cpn, alpha)
        if finetuned:
            self._given_terms(reqs, cands, terms, cpn, alpha, c)
        pairs, cuts = request_pairs([r.text for r in reqs], cands)
        out = []
        for r, cand, ql, term in zip(reqs, cands, np.split(self.vtg_pairs(pairs), cuts), terms):
            fs = np.zeros(cand.shape) if r.first_stage is None else np.asarray(r.first_stage).reshape(cand.shape)
            order, blended = self._blend(cand[None], ql[None], np.zeros((1, len(cand))) if term is None else term[None], fs[None], c)
            out.append((order[0], blended[0]))
        return out

    def _checked(self, requests, finetuned: bool) -> List[SearchRequest]:
        """Step 1 of search_requests: every request a SearchRequest -- its text an int, named candidates an int64 array, K and K0 through check_shortlist (K0
        clipped to the gallery) -- or the ValueError that names what it lacks."""
        N, reqs = len(self.s.video), []
        for r in requests:
            r = r if isinstance(r, SearchRequest) else SearchRequest(*r)
            if r.prefilter is not None and r.shortlist is None:
                raise ValueError("search_requests: a prefilter K0 narrows a shortlist: the request needs its K")
            if r.within is not None:
                if r.cand is not None or r.first_stage is not None:
                    raise ValueError("search_requests: within confines a shortlist to a set of videos; a request that names its candidates"
                                     f"{'' if r.cand is not None else ' first stage'} takes no within")
                if r.shortlist is None:
                    raise ValueError("search_requests: within confines a shortlist: the request needs its K")
                w = check_within(r.within, N)
                self.s._need_live(w)
                K, K0 = check_shortlist(r.shortlist, r.prefilter, len(w))
                reqs.append(SearchRequest(int(r.text), shortlist=K, prefilter=K0, within=w))
                continue
            if (r.cand is None) == (r.shortlist is None):
                raise ValueError("search_requests: a request takes candidates or a shortlist K, one of the two")
            if r.shortlist is not None:
                K, K0 = check_shortlist(r.shortlist, r.prefilter, self.s.n_live)     # (K0 clipped to the videos that are left)
                if r.first_stage is not None:
                    raise ValueError("search_requests: a first stage is parallel to a request's candidates; a shortlist request has none")
                reqs.append(SearchRequest(int(r.text), shortlist=K, prefilter=K0))
            else:
                cand = np.asarray(r.cand, dtype=np.int64).reshape(-1)
                if len(cand) == 0:
                    raise ValueError("search_requests: a request has no candidates")
                self.s._need_live(cand)
                reqs.append(SearchRequest(int(r.text), cand, r.first_stage))
        if not finetuned and any(r.shortlist is not None for r in reqs):
            raise ValueError("search_requests: a shortlist ranks by the TVG likelihood, which a zero-shot model does not have (finetuned=False)")
        return reqs

    def _chosen(self, reqs: List[SearchRequest], cpn: bool, alpha):
        """Step 2: -> (candidates, TVG candidate term) per request.  A request that names its candidates keeps them and has no term yet (None).  The plain shortlists
        take the best K of ONE stage-1 pass; the prefiltered ones the best K of ONE PairScorer.tvg call over what ONE stage-0 pass kept; the value they were ranked
        by is their term."""
        cands, terms = [r.cand for r in reqs], [None] * len(reqs)
        short = [n for n, r in enumerate(reqs) if r.shortlist is not None and r.prefilter is None and r.within is None]
        pre = [n for n, r in enumerate(reqs) if r.prefilter is not None and r.within is None]
        win = [n for n, r in enumerate(reqs) if r.within is not None]
        if short:
            for n, row in zip(short, self._stage1([reqs[n].text for n in short], cpn, alpha)):
                cands[n], terms[n] = self._best(row, reqs[n].shortlist)
        def keep_best(ns, texts, kept):                                  # ONE PairScorer.tvg call over what was kept; each request keeps its best K of it
            pairs, cuts = request_pairs(texts, kept)
            term = self.s.tvg(pairs)
            if cpn:
                term = term - alpha[0] * self._t2v_prior(texts, kept)
            for n, cand, row in zip(ns, kept, np.split(term, cuts)):
                order, terms[n] = self._best(row, reqs[n].shortlist)
                cands[n] = cand[order]
        if pre:
            texts = [reqs[n].text for n in pre]
            keep_best(pre, texts, self._stage0(texts, [reqs[n].prefilter for n in pre], cpn, alpha))
        if win:                                                         #  inside the caller's set: those with a K0 share a stage-0 pass of their own
            texts = [reqs[n].text for n in win]
            self.s._need_tvg(texts)
            self._tvg_state()
            st = self.within_stats
            st["queries"] += len(win); st["candidates"] += int(sum(len(reqs[n].within) for n in win))
            kept = [reqs[n].within for n in win]
            narrowed = [i for i, n in enumerate(win) if reqs[n].prefilter is not None]
            some = self._stage0([texts[i] for i in narrowed], [reqs[win[i]].prefilter for i in narrowed], cpn, alpha, within=[kept[i] for i in narrowed])
            for i, cand in zip(narrowed, some):
                kept[i] = cand
            keep_best(win, texts, kept)
        return cands, terms

    def _given_terms(self, reqs: List[SearchRequest], cands, terms, cpn: bool, alpha, c) -> None:
        """Step 3 (fine-tuned blends): the TVG candidate term of the requests that named their candidates, written into `terms`: ONE PairScorer.tvg call over their
        pairs, minus alpha[0] x the prior with cpn."""
        given = [n for n, r in enumerate(reqs) if r.shortlist is None]
        if not given:
            return
        self._tvg_state()
        texts, mine = [reqs[n].text for n in given], [cands[n] for n in given]
        pairs, cuts = request_pairs(texts, mine)
        has = np.array([self.s.tvg_split[t] is not None for t in texts])
        if c[0] != 1:                                                   # the candidate likelihood has a weight: every text needs its TVG row
            self.s._need_tvg(texts)
        of = np.repeat(has, [len(cand) for cand in mine])               # (a text added without a TVG row keeps a zero term under c0 = 1)
        term = np.zeros(len(pairs), dtype=np.float32)
        if of.any():
            term[of] = self.s.tvg(pairs[of])
        if cpn and of.any():
            prior = np.zeros(len(pairs))
            prior[of] = self._t2v_prior([t for t, h in zip(texts, has) if h], [cand for cand, h in zip(mine, has) if h])
            term = term - alpha[0] * prior
        for n, row in zip(given, np.split(term, cuts)):
            terms[n] = row


class TextGalleryIndex(_PrefixIndex):
    """v2t scores of arbitrary (video, text) pairs of a PairScorer's videos and texts, with the texts' caption prompts (the TVG prefixes) cached on the device.

    scorer: the PairScorer whose texts form the gallery and whose videos are the queries.  budget_bytes: device memory for the caption cache (None: every distinct
    prompt).  video_index: a GalleryIndex on the same scorer that serves the VTG leg (log P(text | video)) from its video slots; without one that leg is PairScorer.vtg.
    The caption cache is filled on the first TVG use or by build(): a zero-shot blend has no TVG term and never fills it."""
    kind, _changed = "tvg", "text gallery: weights or TVG mode"

    def __init__(self, scorer: PairScorer, budget_bytes: Optional[int] = None, video_index: Optional[GalleryIndex] = None, log=None, fill: str = "eager",
                 host_budget_bytes: Optional[int] = None, spare_slots: int = 0):
        super().__init__(scorer, budget_bytes, None, log, fill, host_budget_bytes, spare_slots)
        if video_index is not None and video_index.s is not scorer:
            raise ValueError("TextGalleryIndex: video_index must be built on the same scorer")
        self.video_index = video_index
        # one key per distinct caption prompt, in order of first appearance: texts with the same prompt share a slot
        self.prompts: Dict[bytes, np.ndarray] = {}
        self.keys: List[bytes] = []
        self._sync_texts()
        self.exec_tokens = 0                                # packed tokens of the cached TVG calls run so far
        self.prefilter_stats = {"queries": 0, "passes": 0, "rows": 0, "kept": 0}   # videos prefiltered, stage-0 passes, the caption rows those scored, the texts kept

    def _count_texts(self) -> int:
        return len(self.s.tvg_split)

    def _grow(self, lo: int, hi: int) -> None:
        """Texts lo .. hi - 1 joined: a key per caption prompt the index has not seen, appended (a text added without a TVG row has none)."""
        for pr in self.s.tvg_split[lo:hi]:
            if pr is not None and pr.tobytes() not in self.prompts:
                self.prompts[pr.tobytes()] = pr
                self.keys.append(pr.tobytes())

    def _sync_videos(self, fill: bool = True) -> None:
        """A caption prompt holds no video: a video that joins brings no key here, and the video index follows it.  (The v2t prior is kept per (text, token count),
        VTG-side: it does not depend on the vocabulary and is not dropped.)  A video that leaves takes no key either: the call is passed
        on, and the query entries refuse a removed video by name."""
        super()._sync_videos(fill)
        if fill and self.video_index is not None:
            self.video_index._sync_videos()

    def prefix_len(self, key) -> int:
        return len(self.prompts[key])

    def _prefix(self, key):
        """-> (the caption prompt, no feature rows, nothing after): a caption prompt holds no video token."""
        return self.prompts[key], None, ()

    def compensated(self) -> bool:
        return bool(self.s.split_tvg)

    def _lo6_tvg(self) -> bool:
        """Whether the TVG calls' second pass runs in e2m3: bf16 engines keep the 16-bit pass for them (Engine.set_precise, tvg=True)."""
        return bool(getattr(self.engine, "lo6", False)) and self.compensated() and getattr(self.engine, "dtype", "") != "bf16"

    def _mode_state(self):
        return (self.engine.weights_version, self.s.tvg_mode, bool(self.s.split_tvg), self._lo6_tvg())

    def _follow_model(self) -> bool:
        """As evaluation() does for a caller's scorer: the TVG calls follow what the model asks for / has resolved NOW.  -> False: _mode_state() tells a change."""
        if hasattr(self.m, "tvg_mode"):
            self.s.set_tvg_mode(self.m.tvg_mode())
        return False

    # ---- numeric mode
    def resolve_mode(self, first_stage=None, seed: int = 0) -> str:
        """`--tvg_precise auto` not yet measured on these weights: measured with PairScorer.calibrate_tvg on the gallery's own (video, text) pairs -- calibration_pairs
        of the first-stage v2t scores when given ([N videos, N texts]), else a seeded sample; the sizes are GalleryIndex.resolve_mode's.  Returns the TVG calls' mode."""
        m = self.m
        if self.compensated() and getattr(m, "tvg_precise", None) == "auto" and hasattr(m, "tvg_resolved") and not m.tvg_resolved():
            pairs, confirm, n_eval = self._calibration_sample(first_stage, seed, len(self.s.tvg_split))
            chosen, _ = self.s.calibrate_tvg(pairs, n_eval=n_eval, confirm_pairs=confirm)
            m.resolve_tvg(chosen)
        self._follow_model()
        return self.s.tvg_mode

    # ---- planning
    def _needs(self, pairs: np.ndarray) -> List:
        """The caption prompts of a pass, in the order _plan_tvg meets its texts."""
        self.s._need_tvg(pairs[:, 1])
        return list(dict.fromkeys(self.s.tvg_split[int(i)].tobytes() for i in np.unique(pairs[:, 1])))

    def _plans(self, pairs: np.ndarray):
        """pairs [P, 2] (video j, text i) -> engine calls, planned by PairScorer._plan_tvg's likelihood branch over this index's slots: the candidates of one text are
        merged sequences of up to SEG_MAX // (C - 1) videos' clip tokens (own_start).  A cached text packs no prompt: its sequences name the slot and each pair's first
        row is -(slot + 1)."""
        yield from self.s.iter_tvg_jobs([(pairs, False)], slots=self)

    def run(self, plan):
        self.exec_tokens += plan.n_tokens
        return super().run(plan)

    # ---- scores
    def tvg_pairs(self, pairs) -> np.ndarray:
        """log P(video j | text i) of arbitrary pairs [P, 2] (video j, text i): PairScorer.tvg with the caption prompts read from the cache."""
        return self._scores(pairs)

    def vtg_pairs(self, pairs) -> np.ndarray:
        """log P(text i | video j): from the video index's slots when there is one, else PairScorer.vtg."""
        if self.video_index is not None:
            return self.video_index.vtg_pairs(pairs)
        _follow_vtg(self.s)
        return self.s.vtg(pairs)

    def v2t_prior(self, videos, cand) -> np.ndarray:
        """The v2t candidate prior (VTG-CPN) of every (video, text) pair: it depends on the text and on the video's token count only, so it is memoised per
        (text, token count) for one (weights, VTG mode, layer mask, second pass) state; misses are scored with PairScorer.vtg(..., cpn=True)."""
        s = self.s
        _follow_vtg(s)
        state = _vtg_state(s)
        if state != self._prior_state:
            self._prior, self._prior_state = {}, state
        n_vid = lambda j: int(np.prod(s.video[int(j)].shape[-3:-1]))
        videos = np.asarray(videos, dtype=np.int64).reshape(-1)
        s._need_live(videos)                                 # (a miss is scored over its query video: never over a tombstone)
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
        videos, cand, pairs = grid_pairs(videos, cand, query_col=0)
        self.s._need_live(videos)
        v2t_cand = self.vtg_pairs(pairs).reshape(cand.shape)
        fs = np.zeros(cand.shape) if first_stage is None else np.asarray(first_stage).reshape(cand.shape)
        if cpn:
            v2t_cand = v2t_cand - alpha[1] * self.v2t_prior(videos, cand)
        return self._blend(cand, self.tvg_pairs(pairs).reshape(cand.shape) if finetuned else None, v2t_cand, fs, c)

    @staticmethod
    def _blend(cand, ql, v2t_cand, fs, c):
        """cand, query likelihood (None: zero-shot, the candidate likelihood alone), candidate likelihood and first stage, [Q, k] each -> (candidates best first,
        their blended scores)."""
        _, c1, _, c3 = c
        v2t_lm = v2t_cand if ql is None else c1 * ql + (1 - c1) * v2t_cand
        blended = c3 * v2t_lm + (1 - c3) * fs
        order = np.argsort(-blended, axis=1, kind="stable")
        return np.take_along_axis(cand, order, 1), np.take_along_axis(blended, order, 1)

    # ---- the caption prefilter: every caption ranked on the device by the clip-0 summand of the query likelihood, from the cached rows
    def _stage0(self, videos, chunk_rows: int = 0):
        """-> device f32 [Q, texts]: log P(clip 0 of video | text) for every text and every query video, ONE pass for all Q.  A pair's first scored row is the
        caption prompt's last row, whose hidden state a slot stores: the resident keys go through PairScorer.tvg_first_cached (no decode; cols = the videos'
        vocabulary entries); a key without a slot -- beyond the budget, or not resident in a lazy index -- is scored by the decoded path, PairScorer.tvg_first(...,
        full=True), column `video` of its lp: the same row, the same bits.  Nothing is admitted, counted as a hit or a miss, or stamped.  The per-key values are
        fanned out on the device: texts with the same prompt share a key."""
        import torch
        s = self.s
        dev = getattr(s, "device", "cpu")
        of_text = self._key_of_text(dev)
        have = [n for n, k in enumerate(self.keys) if k in self.slot_of] if self.cache is not None else []
        part = None
        if have:
            cols = torch.from_numpy(np.asarray(s.tvg_video_labels, dtype=np.int32)[videos]).to(dev)
            part = s.tvg_first_cached(self.cache, [self.slot_of[self.keys[n]] for n in have], cols, chunk_rows)
        if len(have) == len(self.keys):
            per_key = part
        else:
            resident = set(have)
            lack = [n for n in range(len(self.keys)) if n not in resident]
            first = {}
            for i, n in enumerate(of_text[0]):
                first.setdefault(n, i)
            lp = s.tvg_first([first[n] for n in lack], 1, full=True)[2]
            per_key = torch.empty((len(videos), len(self.keys)), dtype=torch.float32, device=dev)
            if have:
                per_key[:, torch.as_tensor(have, dtype=torch.int64, device=dev)] = part
            per_key[:, torch.as_tensor(lack, dtype=torch.int64, device=dev)] = torch.from_numpy(np.ascontiguousarray(lp[:, videos].T)).to(dev)
        return per_key[:, of_text[1]].contiguous()

    def _key_of_text(self, dev):
        """-> (every text's key position, the same as a device index), kept while the texts and the keys are the ones it was made for (both are appended only)."""
        import torch
        size = (len(self.s.tvg_split), len(self.keys))
        memo = getattr(self, "_fan", None)
        if memo is None or memo[0] != size:
            key_at = {k: n for n, k in enumerate(self.keys)}
            of_text = [key_at[pr.tobytes()] for pr in self.s.tvg_split]
            memo = self._fan = (size, of_text, torch.as_tensor(of_text, dtype=torch.int64, device=dev))
        return memo[1], memo[2]

    def prefilter(self, videos, k0: int, chunk_rows: int = 0):
        """The K0 captions of each query video that log P(clip 0 of the video | text) ranks first: ONE stage-0 pass for all videos (_stage0: two small GEMMs over
        the cached rows, no layer), ranked on the device (Engine.rank_rows).  The index follows the model's TVG mode and fills its cache first, as tvg_pairs does.
        -> (cand int64 [Q, min(k0, texts)] text indices, best first: descending, ties to the lower text index; val f32, their values).  ValueError as
        check_shortlist (K0 clipped to the texts); a text without a TVG row is refused by name."""
        videos = np.asarray(videos, dtype=np.int64).reshape(-1)
        self.s._need_live(videos)
        n = len(self.s.tvg_split)
        _, k0 = check_shortlist(None, k0, n)
        if not len(videos):
            return np.zeros((0, k0), np.int64), np.zeros((0, k0), np.float32)
        if any(pr is None for pr in self.s.tvg_split):
            self.s._need_tvg(np.arange(n))                     # (raises: every text is ranked)
        self._fresh()
        self._sync_texts()
        self._sync_videos()
        idx, val = self.engine.rank_rows(self._stage0(videos, chunk_rows), k0)
        st = self.prefilter_stats
        st["queries"] += len(videos); st["passes"] += 1; st["rows"] += len(self.keys); st["kept"] += len(videos) * k0
        return idx.cpu().numpy().astype(np.int64), val.cpu().numpy()

    # ---- the shortlist, v2t
    def shortlist(self, videos, k: int, prefilter: Optional[int] = None):
        """Every caption ranked by a query video's TVG likelihood, log P(video | text), over the cached prompts: one tvg_pairs pass per query video, so every text has
        one video and a value is that of any other pass that scores the pair so (section 11).  Descending, ties to the lower text index.  prefilter = K0 >= k
        (section 22): ONE prefilter() pass for all videos first, and each video's pass runs over its K0 survivors only, in ascending text order.
        -> (cand [Q, min(k, texts)] text indices, best first; their stage-1 scores)."""
        videos = np.asarray(videos, dtype=np.int64).reshape(-1)
        self.s._need_live(videos)
        n = len(self.s.tvg_split)
        k = min(check_shortlist(k, prefilter, n)[0], n)
        kept = None if prefilter is None else np.sort(self.prefilter(videos, prefilter)[0], axis=1)
        cand, stage = np.zeros((len(videos), k), np.int64), np.zeros((len(videos), k), np.float32)
        for q, v in enumerate(videos):
            texts = np.arange(n) if kept is None else kept[q]
            row = self.tvg_pairs(np.stack([np.full(len(texts), v, dtype=np.int64), texts], axis=1))
            order = np.argsort(-row, kind="stable")[:k]
            cand[q], stage[q] = texts[order], row[order]
        return cand, stage

    def rerank_shortlist(self, videos, k: int, cpn: bool = False, alpha=(0.0, 0.0), c=(1.0, 1.0, 1.0, 1.0), prefilter: Optional[int] = None):
        """rerank(videos, shortlist(videos, k), finetuned=True) without a first stage, the query likelihood of the blend being the shortlist's stage-1 value: the TVG
        term is not computed a second time.  prefilter = K0: shortlist's.  -> (order [Q, k] of text ids, best first; blended scores in that order)."""
        self.s._need_live(videos)
        cand, stage = self.shortlist(videos, k) if prefilter is None else self.shortlist(videos, k, prefilter)
        videos, cand, pairs = grid_pairs(videos, cand, query_col=0)
        v2t_cand = self.vtg_pairs(pairs).reshape(cand.shape)
        if cpn:
            v2t_cand = v2t_cand - alpha[1] * self.v2t_prior(videos, cand)
        return self._blend(cand, stage, v2t_cand, np.zeros(cand.shape), c)
