"""Cache residency: which prefix keys hold a slot of the engine's prefix cache (blim.h: blim_prefix_cache_*), and how they come and go.  What is searched, and how
a search is blended, is blim_amd/gallery.py; this module does not import it.

`_PrefixIndex` owns one cache slot per prefix key under a memory budget.  It neither plans nor runs a call of its own: the planners are PairScorer's (`_pack_vtg`,
`_plan_tvg`), handed the index as their prefix source -- a group whose prefix has a slot packs no prefix sequence -- and the calls, and the fills, run under
`PairScorer._call_options`, so a slot is read under the options it was filled under.

- The fill and the refill.  `fill="eager"`: `build()` assigns the slots (`slot_plan`) and fills them in packed calls; the keys beyond the budget keep the in-batch
  prefix.  A weight, adapter or mode change refills them once (`_fresh`).
- The per-pass admission policy (`fill="lazy"`).  Nothing is filled up front and the budget is a capacity: a prefix that a scoring call had to
  pack anyway (a miss) is captured into a slot by that very call (`blim_score_*_admit`).  Which slot is decided per pass -- one vtg_pairs / tvg_pairs call -- in
  `_begin_pass`: free slots first, then the least recently used slot whose key this pass does not need, else no admission.  `_commit` makes a call's admissions the
  index's state once the call has returned.
- The host tier (`HostTier`; lazy fill with `host_budget_bytes`).  A key that loses its slot is kept as a packed record in pinned host
  memory, and a key that has a record gets a slot back by a copy (blim.h: blim_prefix_cache_export / _import) instead of a decode.
- Following the scorer.  Texts that join (`PairScorer.add_texts`, section 17) and videos that join (`add_videos`, section 19) append keys before the next pass
  is planned; an eager index fills a new video into its `spare_slots`, a lazy one admits it on demand.  Videos leave as well (`remove_videos`, section 24):
  indices never move; before the next pass the keys of a removed video leave the key list, `slot_of`, the recency stamps, a pending pass's reservations and the
  host tier (`HostTier.forget`), their slots are free at once, a plan made before is refused, and `removed_stats` counts what left.
"""
from __future__ import annotations

import sys
from dataclasses import asdict, dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .pair_scorer import PairScorer, _PackState

SLOT_ALIGN = 32          # a slot's positions are padded to a multiple of the attention's key tile


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


@dataclass
class GalleryStats:
    """What an index's passes did, counted per prefix group (key) per pass and committed as the pass's calls return: keys found in a slot, keys packed in the batch,
    of those the ones captured into a slot, the keys that lost their slot to them, and the tokens of every in-batch prefix sequence."""
    hits: int = 0
    misses: int = 0
    admitted: int = 0
    evicted: int = 0
    prefix_tokens_packed: int = 0

    def reset(self) -> None:
        self.hits = self.misses = self.admitted = self.evicted = self.prefix_tokens_packed = 0

    def as_dict(self) -> Dict[str, int]:
        return asdict(self)


@dataclass
class HostStats:
    """What a host tier did: slots restored from a record, slots spilled into one, records given up (to make room, or because the weights or the mode changed),
    and the bytes copied each way."""
    restored: int = 0
    spilled: int = 0
    dropped: int = 0
    bytes_to_host: int = 0
    bytes_from_host: int = 0

    def as_dict(self) -> Dict[str, int]:
        return asdict(self)


def _pinned_bytes(n: int):
    import torch
    return torch.empty(int(n), dtype=torch.uint8, pin_memory=True)


def _device_bytes(n: int, device):
    import torch
    return torch.empty(int(n), dtype=torch.uint8, device=device)


def _device_sync():
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()


class HostTier:
    """The lazy index's second tier: slots that lose their place in the prefix cache are kept as packed records (blim.h:
    blim_prefix_cache_export) in pinned host memory, and a key with a record gets its slot back by a copy (blim_prefix_cache_import) instead of a decode.

    arena: pinned uint8, host_budget_bytes cut into fixed records of record_bytes(positions) -- a slot of any filled length fits one; only the bytes of the slot's own
    record are copied.  staging: device uint8 of stage_records records, what the two entry points write and read; a transfer of more slots goes in chunks.  Every copy
    is copy_(non_blocking=True) on the current stream -- the one the scoring calls run on -- so that the reuse of a record, of the staging buffer and the calls that read
    a restored slot are ordered by that stream alone, and the host never reads the arena.  One ticket per record.  The tier is inclusive: a record stays valid after
    its key was restored, and a slot that has one is not exported again."""

    def __init__(self, cache, positions: int, host_budget_bytes: int, stage_records: int = 16, arena=None, staging=None, sync=None):
        self.record_bytes = int(cache.record_bytes(int(positions)))
        if self.record_bytes <= 0:
            raise ValueError(f"HostTier: the cache has no record of {positions} positions")
        self.n_records = max(int(host_budget_bytes), 0) // self.record_bytes
        self.stage_records = max(1, min(int(stage_records), max(self.n_records, 1)))
        self.stats = HostStats()
        self.rec_of: Dict = {}           # key -> its record
        self.key_of: Dict[int, object] = {}
        self.len_of: Dict[int, int] = {}
        self.tickets: Dict[int, object] = {}
        self._stamp: Dict = {}           # key -> its last use, as the index stamps it
        self._sync = sync if sync is not None else _device_sync
        self.arena = self.staging = None
        if self.n_records:
            self.arena = arena if arena is not None else _pinned_bytes(self.n_records * self.record_bytes)
            if not self.arena.is_pinned():
                raise ValueError("HostTier: the arena must be pinned host memory (a pageable copy would make every transfer wait for the device)")
            if self.arena.numel() < self.n_records * self.record_bytes:
                raise ValueError(f"HostTier: the arena holds {self.arena.numel()} bytes, {self.n_records} records need {self.n_records * self.record_bytes}")
            self.staging = staging if staging is not None else _device_bytes(self.stage_records * self.record_bytes, cache.engine.device)

    def has(self, key) -> bool:
        return key in self.rec_of

    def touch(self, key, stamp) -> None:
        if key in self.rec_of:
            self._stamp[key] = stamp

    def plan_spills(self, victims: Sequence, protected) -> List[Tuple]:
        """-> [(victim, record, the key that gives the record up or None)] for the victims that get a record, in their order: a free record, else the least recently
        used record whose key is not in `protected`; a victim that finds neither is lost, as without a tier.  Nothing changes here."""
        free = [r for r in range(self.n_records) if r not in self.key_of]
        lru = sorted((k for k in self.rec_of if k not in protected), key=lambda k: self._stamp.get(k, (0, 0)))
        out = []
        for v in victims:
            if free:
                out.append((v, free.pop(0), None))
            elif lru:
                d = lru.pop(0)
                out.append((v, self.rec_of[d], d))
        return out

    def _chunks(self, items):
        for a in range(0, len(items), self.stage_records):
            yield items[a:a + self.stage_records]

    def spill(self, cache, items: Sequence[Tuple]) -> None:
        """items [(key, slot, record, dropped key or None, stamp)]: the slots' records go to the arena.  A chunk is committed when its export has returned."""
        rb = self.record_bytes
        for part in self._chunks(list(items)):
            moves = [(slot, cache.slot_len(slot), n * rb) for n, (_, slot, _, _, _) in enumerate(part)]
            tickets = cache.export_slots(moves, self.staging)
            for (key, slot, rec, dropped, stamp), (_, ln, off), t in zip(part, moves, tickets):
                nb = cache.record_bytes(ln)
                self.arena[rec * rb:rec * rb + nb].copy_(self.staging[off:off + nb], non_blocking=True)
                if dropped is not None and self.rec_of.get(dropped) == rec:
                    del self.rec_of[dropped]; self._stamp.pop(dropped, None)
                    self.stats.dropped += 1
                self.rec_of[key], self.key_of[rec], self.len_of[rec], self.tickets[rec], self._stamp[key] = rec, key, ln, t, stamp
                self.stats.spilled += 1; self.stats.bytes_to_host += nb

    def restore(self, cache, items: Sequence[Tuple], committed=None) -> None:
        """items [(key, slot, stamp)]: the keys' records become the slots.  committed(key, slot, stamp) is called per key once its chunk's import has returned; a
        failed import raises and commits nothing of its chunk."""
        rb = self.record_bytes
        for part in self._chunks(list(items)):
            moves, tickets = [], []
            for n, (key, slot, _) in enumerate(part):
                rec = self.rec_of[key]
                ln = self.len_of[rec]
                nb = cache.record_bytes(ln)
                self.staging[n * rb:n * rb + nb].copy_(self.arena[rec * rb:rec * rb + nb], non_blocking=True)
                moves.append((slot, ln, n * rb)); tickets.append(self.tickets[rec])
            cache.import_slots(moves, self.staging, tickets)
            for (key, slot, stamp), (_, ln, _) in zip(part, moves):
                self._stamp[key] = stamp
                self.stats.restored += 1; self.stats.bytes_from_host += cache.record_bytes(ln)
                if committed is not None:
                    committed(key, slot, stamp)

    def forget(self, key) -> bool:
        """forget_all for one key (its video was removed: DESIGN.md section 24): the record's arena space is free for the next spill, and no later restore can bring
        the key back.  -> whether the key had a record.  (A copy into the record that is still in flight is ordered before its next use by the stream, as ever.)"""
        rec = self.rec_of.pop(key, None)
        self._stamp.pop(key, None)
        if rec is None:
            return False
        self.key_of.pop(rec, None); self.len_of.pop(rec, None); self.tickets.pop(rec, None)
        self.stats.dropped += 1
        return True

    def forget_all(self) -> None:
        """A weight, adapter or mode change: no record is valid any more (the engine would refuse their slots as stale)."""
        self.stats.dropped += len(self.rec_of)
        self.rec_of, self.key_of, self.len_of, self.tickets, self._stamp = {}, {}, {}, {}, {}

    def close(self) -> None:
        """Copies into and out of the arena may still be in flight: the device is waited for before the memory goes."""
        if self.arena is not None:
            self._sync()
        self.arena = self.staging = None
        self.rec_of, self.key_of, self.len_of, self.tickets, self._stamp = {}, {}, {}, {}, {}


@dataclass
class _Pass:
    """One vtg_pairs / tvg_pairs call as the index sees it: the keys it needs in the order the planner meets them, and -- lazy fill -- the slot reserved for each
    miss that is admitted ({key: (slot, the key that loses it or None)}).  Nothing of it is part of the index's state until a call of the pass has returned."""
    no: int
    need: List
    hits: List
    misses: List
    reserved: Dict = field(default_factory=dict)
    offered: set = field(default_factory=set)
    counted: bool = False


class _PrefixIndex:
    """What the two indexes share: one cache slot per prefix key under a memory budget, filled in packed calls and refilled when the weights or the numeric mode
    change.  A subclass names its call kind, its keys (self.keys, in gallery order), a key's prefix (prefix_len, _prefix), compensated(), _mode_state(),
    _follow_model(), resolve_mode(), a pass's keys (_needs) and its plans (_plans); the planners read slot_of and cache (and, on a lazy index, call admit)."""
    kind = ""              # "vtg" | "tvg": the calls whose prefixes the slots hold
    _changed = ""          # the refill's log line opens with it

    def __init__(self, scorer: PairScorer, budget_bytes: Optional[int], priority: Optional[Sequence[int]], log, fill: str = "eager",
                 host_budget_bytes: Optional[int] = None, spare_slots: int = 0):
        if fill not in ("eager", "lazy"):
            raise ValueError(f"fill {fill!r}: 'eager' or 'lazy'")
        if int(spare_slots) < 0 or (int(spare_slots) and fill != "eager"):
            raise ValueError(f"{type(self).__name__}: spare_slots = {spare_slots}: free slots of an eager cache for the keys that join later, not negative; "
                             "a lazy index's budget is its capacity already")
        self.spare_slots = int(spare_slots)
        if host_budget_bytes is not None and fill != "lazy":
            raise ValueError(f"{type(self).__name__}: host_budget_bytes keeps the slots a lazy index evicts; an eager index ({fill!r}) evicts none: use fill='lazy'")
        self.host_budget_bytes = host_budget_bytes
        self.host: Optional[HostTier] = None         # lazy fill with host_budget_bytes: built with the cache
        if fill == "lazy" and priority is not None:
            raise ValueError(f"{type(self).__name__}: priority orders the eager fill; a lazy index follows the queries")
        self.fill = fill
        self.n_slots = 0                 # lazy: the capacity (eager: the planned slots and the spare ones)
        self.stats = GalleryStats()
        self._stamp: Dict = {}           # lazy: resident key -> (pass number, position among the pass's keys) of its last use
        self._pass: Optional[_Pass] = None
        self._n_pass = 0
        self._n_texts = 0                # the scorer's texts the keys cover (PairScorer.add_texts: texts join later; _sync_texts)
        self._n_videos = len(scorer.video)   # ... and its videos (PairScorer.add_videos; _sync_videos)
        self._gone = scorer.removed          # ... and the removed ones it has followed (PairScorer.remove_videos; _sync_videos)
        self._stale_before = 0               # passes numbered up to this were planned before a removal the index has followed since: run() refuses their plans
        self.removed_stats = {"videos": 0, "slots_freed": 0, "records_forgotten": 0}     # removed videos followed, the slots their keys gave back, their host records forgotten
        self.s = scorer
        self.m, self.engine = scorer.m, scorer.engine
        if getattr(self.engine, "dtype", "") == "f8":
            raise ValueError(f"{type(self).__name__}: fp8 engines are not supported (use --dtype f16 or bf16)")
        self.budget_bytes = budget_bytes
        self.priority = priority
        self.log = log if log is not None else (lambda msg: print(msg, file=sys.stderr, flush=True))
        self.keys: List = []
        self.cache = None
        self.slot_of: Dict = {}
        self._state = None
        self._prior: Dict[Tuple, float] = {}       # candidate priors of the other direction's calls, valid for the state in _prior_state
        self._prior_state = None
        self.build_seconds = 0.0

    # ---- geometry
    def max_len(self) -> int:
        return max(self.prefix_len(k) for k in self.keys)

    def slot_positions(self) -> int:
        return -(-self.max_len() // SLOT_ALIGN) * SLOT_ALIGN

    def per_slot_bytes(self) -> int:
        return self.engine.prefix_cache_bytes(1, self.slot_positions(), self.compensated())

    def _free_slots(self) -> List[int]:
        """The slots no key holds, ascending."""
        taken = set(self.slot_of.values())
        return [sl for sl in range(self.n_slots) if sl not in taken]

    def _fits(self, key) -> bool:
        """Whether the key's prefix fits a slot: a key that joined after build() may be longer than one, and then stays in the batch."""
        room = getattr(self.cache, "max_len", None)
        return room is None or self.prefix_len(key) <= room

    def _calibration_sample(self, first_stage, seed: int, n_texts: int):
        """-> (pairs, confirmation pairs, n_eval) for the scorer's calibrators: calibration_pairs of the first-stage v2t scores when given ([N videos, N texts];
        evaluation()'s sample and confirmation sample), else a seeded sample of the same sizes.  Live videos only: a refill after a weight
        change must not sample a tombstone."""
        from .calibration import calibration_pairs
        lv, Nt = self.s.live_videos(), n_texts
        if first_stage is not None:
            rows = lv[lv < len(first_stage)]         # (a video that joined at run time has no first-stage row)
            sub = np.asarray(first_stage)[rows]
            pairs, confirm = (calibration_pairs(sub, 16, n_queries=q, per_query=8) for q in (32, 256))
            pairs[:, 0], confirm[:, 0] = rows[pairs[:, 0]], rows[confirm[:, 0]]
        else:
            rng = np.random.RandomState(seed)
            flat = rng.choice(len(lv) * Nt, size=min(2048, len(lv) * Nt), replace=False)
            both = np.stack([lv[flat // Nt], flat % Nt], axis=1).astype(np.int64)
            pairs, confirm = both[:256], both
        return pairs, confirm, len(lv) * min(16, Nt)

    # ---- fill
    def build(self, first_stage=None):
        """Resolves the numeric mode, assigns the slots under the budget and fills them in packed calls of up to max_tokens tokens."""
        import time
        import torch
        self._sync_texts()
        self._sync_videos(fill=False)                # (the keys only: every key is planned below)
        self.resolve_mode(first_stage)
        t0 = time.perf_counter()
        comp = self.compensated()
        L = self.slot_positions()
        per = self.engine.prefix_cache_bytes(1, L, comp)
        self.close()
        self._drop()
        if self.fill == "lazy":                      # the budget is a capacity: nothing is filled, the scoring calls admit what they had to pack anyway
            self.n_slots = len(self.keys) if self.budget_bytes is None else min(len(self.keys), int(self.budget_bytes) // max(int(per), 1))
            if self.n_slots:
                self.cache = self.engine.prefix_cache(self.n_slots, L, comp)
                if self.host_budget_bytes is not None:
                    self.host = HostTier(self.cache, L, self.host_budget_bytes)
        else:                                        # the spare slots count against the budget: they are taken off it before the keys are planned
            spare = self.spare_slots if self.budget_bytes is None else min(self.spare_slots, int(self.budget_bytes) // max(int(per), 1))
            self.slot_of = slot_plan(self.keys, per, None if self.budget_bytes is None else int(self.budget_bytes) - spare * int(per), self.priority)
            self.n_slots = len(self.slot_of) + spare
            if self.n_slots:
                self.cache = self.engine.prefix_cache(self.n_slots, L, comp)
                self._fill(sorted(self.slot_of.items(), key=lambda kv: kv[1]))
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.build_seconds = time.perf_counter() - t0
        self._state = self._mode_state()
        return self

    def _fill(self, items):
        st, slots = _PackState(self.s, self.kind), []
        for key, slot in items:
            pre, f, post = self._prefix(key)
            n_feat = 0 if f is None else int(f.shape[0])
            plen = len(pre) + n_feat + len(post)
            if st.n_tok and st.n_tok + plen > self.s.max_tokens:
                self._fill_call(st, slots); st, slots = _PackState(self.s, self.kind), []
            ptoks = pre if f is None else np.concatenate([pre, -(1 + st.add_feat(f) + np.arange(n_feat)), post])
            st.add_seq(ptoks, np.arange(plen), np.ones(plen, np.uint8), None)
            slots.append(slot)
        if slots:
            self._fill_call(st, slots)

    def _fill_call(self, st: _PackState, slots: List[int]):
        batch, src, feats = st.upload()
        with self.s._call_options(self.kind):        # the options the scoring calls run under: the slots record them
            self.cache.fill(batch, self.engine.assemble(src, feats), np.asarray(slots, np.int32))

    def _fresh(self):
        """A weight / adapter / mode change since build(): the slots are refilled once (the engine would refuse them: BLIM_ERR_STATE)."""
        if self._state is None:
            self.build()
        elif self._follow_model() or self._mode_state() != self._state:
            if self.fill == "lazy":                  # the slots are dropped and admitted again on demand; the cache itself stays unless its layout changes
                self.log(f"{self._changed} changed since the slots were admitted ({self._state} -> {self._mode_state()}): dropping {len(self.slot_of)} slots")
                if self.cache is None or self.n_slots == 0 or bool(self.cache.compensated) != bool(self.compensated()):
                    self.build()
                else:
                    self._drop()
                    self._state = self._mode_state()
                return
            self.log(f"{self._changed} changed since the fill ({self._state} -> {self._mode_state()}): refilling {len(self.slot_of)} slots")
            self.build()

    def _drop(self):
        """Forgets every slot (and every reservation): the index holds nothing."""
        self.slot_of, self._stamp, self._pass = {}, {}, None
        if self.host is not None:
            self.host.forget_all()

    # ---- passes (lazy fill: the replacement policy)
    @property
    def admit(self):
        """The planners' hook (PairScorer._pack_vtg / _plan_tvg): present on a lazy index only."""
        return self._admit if self.fill == "lazy" else None

    def _begin_pass(self, need: List) -> _Pass:
        """A pass opens: `need` = its keys in the order the planner meets them.  Reservations of plans that were never run are dropped with the pass they belonged
        to.  Lazy fill, the policy: resident keys the pass needs are pinned; a miss takes a free slot, else the least recently used slot whose key the pass does not
        need, else it is not admitted -- so no slot is read and overwritten within a pass, and a scan over more keys than slots keeps its resident set.  Nothing the
        index holds changes here: run() commits.

        With a host tier the same rule hands out the slots, and a key that gets one and has a record is RESTORED instead of admitted: the
        tier's transfers run here, before the pass is planned (the planner reads slot_of and the cache's lengths) -- every export, then every import -- and a restore is
        part of the index's state as soon as its import has returned.  The keys that lose their slots are exported unless they have a record already; those of
        admissions stay resident until the admitting call commits."""
        self._n_pass += 1
        no = self._n_pass
        reserved: Dict = {}
        if self.fill == "lazy" and self.n_slots:
            needed = set(need)
            at = {k: n for n, k in enumerate(need)}
            free = self._free_slots()
            victims = sorted((k for k in self.slot_of if k not in needed), key=lambda k: self._stamp.get(k, (0, 0)))
            host = self.host if self.host is not None and self.host.n_records else None
            restores, losers = [], []
            for k in need:
                if k in self.slot_of or not self._fits(k):
                    continue
                if free:
                    sl, v = free.pop(0), None
                elif victims:
                    v = victims.pop(0)
                    sl = self.slot_of[v]
                else:
                    break
                if host is not None and host.has(k):
                    restores.append((k, sl, v))
                else:
                    reserved[k] = (sl, v)
                if v is not None:
                    losers.append(v)
            if host is not None and (restores or losers):
                spills = host.plan_spills([v for v in losers if not host.has(v)], needed | set(losers))
                host.spill(self.cache, [(v, self.slot_of[v], rec, dropped, self._stamp.get(v, (0, 0))) for v, rec, dropped in spills])
                loser_of = {sl: v for _, sl, v in restores}
                host.restore(self.cache, [(k, sl, (no, at[k])) for k, sl, _ in restores], lambda k, sl, stamp: self._take(k, sl, loser_of[sl], stamp))
        p = _Pass(no, need, [k for k in need if k in self.slot_of], [k for k in need if k not in self.slot_of], reserved)
        self._pass = p
        return p

    def _admit(self, key):
        """-> the slot reserved for `key` in the pass being planned (once per pass), or None: the prefix stays in the batch."""
        p = self._pass
        if p is None or key not in p.reserved or key in p.offered:
            return None
        p.offered.add(key)
        return p.reserved[key][0]

    def iter_plans(self, pairs):
        """pairs [P, 2] (video j, text i) -> the engine calls of one pass, planned by PairScorer's planner over this index's slots (the subclass's _plans)."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        self.s._need_live(pairs[:, 0])               # a removed video is refused by name before the pass opens
        self._sync_texts()
        self._sync_videos()
        p = self._begin_pass(self._needs(pairs))
        for plan in self._plans(pairs):
            plan.pass_ = p
            yield plan

    def _take(self, key, slot: int, loser, stamp) -> None:
        """Key `key` takes slot `slot` from `loser` (None: the slot was free), admitted or restored: the loser's slot and stamp go, counted as an eviction, when it
        still holds that slot; the slot and the stamp are the key's."""
        if loser is not None and self.slot_of.get(loser) == slot:
            del self.slot_of[loser]; self._stamp.pop(loser, None)
            self.stats.evicted += 1
        self.slot_of[key] = slot; self._stamp[key] = stamp

    def _commit(self, plan) -> None:
        """An engine call of the pass returned without error: what it did becomes the index's state -- the pass's hits and misses (once), the slots the call admitted,
        the keys that lost them, the recency of the keys used."""
        p = getattr(plan, "pass_", None)
        if p is None:
            return
        st = self.stats
        if not p.counted:
            p.counted = True
            st.hits += len(p.hits); st.misses += len(p.misses)
            at = {k: n for n, k in enumerate(p.need)}
            for k in p.hits:
                if k in self.slot_of:
                    self._stamp[k] = (p.no, at[k])
                    if self.host is not None:
                        self.host.touch(k, (p.no, at[k]))
        st.prefix_tokens_packed += int(plan.prefix_tokens)
        if plan.admits is not None and len(plan.admits):
            at = {k: n for n, k in enumerate(p.need)}
            by_slot = {sl: (k, v) for k, (sl, v) in p.reserved.items()}
            for sl in np.asarray(plan.admits)[:, 1]:
                k, v = by_slot[int(sl)]
                self._take(k, int(sl), v, (p.no, at[k]))
                st.admitted += 1                     # (a restore takes a slot too, and is no admission)

    def _sync_texts(self) -> None:
        """The index follows its scorer: texts that joined since the keys were last derived (PairScorer.add_texts) extend them.  Keys are appended only, so the
        slots, the recency stamps, the stats and the host tier's records stay valid; a new key has no slot until it is admitted (lazy) or the index is built again."""
        n = self._count_texts()
        if n != self._n_texts:
            self._grow(self._n_texts, n)
            self._n_texts = n

    def _sync_videos(self, fill: bool = True) -> None:
        """The index follows its scorer: videos that joined since the keys were last derived (PairScorer.add_videos) extend them -- after
        _sync_texts, so that a new video meets every known split once.  Keys are appended only, so the slots, the recency stamps, the stats and the host tier's
        records stay valid, and no cache is resized.  A lazy index admits a new key on demand like any miss.  An eager index that was built fills the new keys, in key
        order, into the slots it still has free (spare_slots) with the fill path of build(); the keys beyond them, and a key longer than a slot, keep the in-batch
        prefix, as a late text's new split does.  The numeric mode is not resolved again (resolve_mode ran on the gallery build() saw).
        Videos that left (PairScorer.remove_videos) are followed first (_follow_removed), so a slot they free is there for a video that joins."""
        self._follow_removed()
        n = len(self.s.video)
        if n == self._n_videos:
            return
        new = self._video_keys(self._n_videos, n)
        self.keys += new
        self._n_videos = n
        if not (fill and new and self.fill == "eager" and self._state is not None and self.cache is not None):
            return
        free = self._free_slots()
        items = []
        for k in new:
            if not free:
                break
            if self._fits(k):
                items.append((k, free.pop(0)))
        if items:
            self._fill(items)
            self.slot_of.update(items)

    def _video_keys(self, lo: int, hi: int) -> List:
        """The keys videos lo .. hi - 1 bring (none where the keys do not name a video)."""
        return []

    def _follow_removed(self) -> bool:
        """The index follows the videos that left its scorer since it last looked: what names them is dropped (_forget_videos) and nothing else -- indices never
        move, no cache is resized or rebuilt, the numeric mode is not resolved again.  A plan made before that may name a slot that is free now, or filled again:
        the pending pass is dropped and run() refuses every plan of an earlier pass.  -> whether anything left."""
        dead = self.s.removed
        if dead == self._gone:
            return False
        gone = dead - self._gone
        self._gone = dead
        self.removed_stats["videos"] += len(gone)
        self._forget_videos(gone)
        self._pass, self._stale_before = None, self._n_pass
        return True

    def _forget_videos(self, gone) -> None:
        """The index's state that names the videos `gone` (none where the keys do not name a video)."""

    # ---- scoring
    def run(self, plan):
        self._follow_removed()
        p = getattr(plan, "pass_", None)
        if (self.fill == "lazy" and p is not self._pass) or (p is not None and p.no <= self._stale_before):
            raise RuntimeError(f"{type(self).__name__}: this plan belongs to an earlier pass (its slots may have been admitted to other prefixes since): plan again")
        out = self.s.run(plan, self.cache_or_none())
        self._commit(plan)
        return out

    def cache_or_none(self):
        if self.cache is None:                       # a budget of zero slots: a one-slot cache that no sequence names keeps the same call path
            self.cache = self.engine.prefix_cache(1, SLOT_ALIGN, self.compensated())
        return self.cache

    def _scores(self, pairs) -> np.ndarray:
        self._fresh()
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        return self.s.score(self.iter_plans(pairs), len(pairs), self.run)

    def close(self):
        if self.host is not None:                    # first: its copies read and write the cache's staging partner on the stream; it waits for the device
            self.host.close(); self.host = None
        if self.cache is not None:
            self.cache.close(); self.cache = None
