"""GPU: slot export / import (blim.h: blim_prefix_cache_export / _import) and the lazy gallery's host tier (blim_amd/gallery.py: HostTier, `host_budget_bytes`;
DESIGN.md section 13).  The feature copies bytes, so every comparison is exact: records byte for byte, scores bit for bit (np.array_equal) against PairScorer on the
same pairs -- with one video per text on the TVG side, where section 11's 1e-5 rule does not come into play.  The refusals and the stale-ticket rule are host-side
checks: nothing is provoked on the device.  A few MB are pinned at most.  The policy's host side is tests/test_host_tier_host.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gallery_gpu as G
import test_gpu_parity as P
import test_lazy_gallery_gpu as LZ
import test_text_gallery_gpu as TG
from blim_amd import engine as eng
from blim_amd import gallery as GL
from blim_amd import synth
from blim_amd.gallery import GalleryIndex, HostTier, TextGalleryIndex
from blim_amd.pair_scorer import _PackState
from test_gallery_gpu import tiny  # noqa: F401  (fixture: the tiny case, 6 videos and 2 layers, in fp16 and bf16)

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _staging(nbytes):
    return torch.full((int(nbytes),), SENTINEL, dtype=torch.uint8, device="cuda")


def _raw_bytes(t, cache, ln):
    """A record's bytes before the rounding to 256: (num_layers * len * kv_w + hid_w) 16-bit values."""
    f = 2 if cache.compensated else 1
    return (t.dims.num_layers * ln * 2 * t.dims.num_kv_heads * t.dims.head_dim * f + t.dims.hidden_size * f) * 2


def _laid_out(cache, lens, gap=256):
    """-> (offsets, total bytes): records of the given lengths one after the other with `gap` untouched bytes before each."""
    offs, at = [], 0
    for ln in lens:
        at += gap
        offs.append(at)
        at += cache.record_bytes(ln)
    return offs, at + gap


def _assert_only_the_records_were_written(t, cache, host_bytes, lens, offs):
    """The records are written (little of them still reads as the sentinel); their padding and every byte between them keep it."""
    keep = np.ones(len(host_bytes), bool)
    for ln, off in zip(lens, offs):
        raw = _raw_bytes(t, cache, ln)
        assert raw <= cache.record_bytes(ln) < raw + 256 and cache.record_bytes(ln) % 256 == 0
        keep[off:off + raw] = False
        assert np.mean(host_bytes[off:off + raw] != SENTINEL) > 0.9
    assert np.all(host_bytes[keep] == SENTINEL)


def _eager_over(sc, cls, cache, slot_of):
    """An index of `cls` that reads `cache` through `slot_of` as an eager index reads the cache it filled."""
    g = cls(sc)
    g.cache, g.slot_of, g.n_slots = cache, dict(slot_of), len(slot_of)
    g._state = g._mode_state()
    return g


# ---- 1. round trip across layouts
@pytest.mark.parametrize("mode", ["none", "full"])
def test_round_trip_into_a_cache_of_another_layout(tiny, mode):
    t = tiny
    G._set_mode(t, mode)
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = G._t2v_pairs(t)
    ref = sc.vtg(pairs)
    a = GalleryIndex(sc).build()
    A = a.cache
    n = A.n_slots
    B = t.model.engine.prefix_cache(n + 2, A.max_len + 32, A.compensated)
    try:
        assert A.compensated == (mode == "full") and np.all(np.isfinite(ref))
        over_a = a.vtg_pairs(pairs)
        lens = [A.slot_len(s) for s in range(n)]
        offs, total = _laid_out(A, lens)
        st1, st2 = _staging(total), _staging(total)
        tickets = A.export_slots(list(zip(range(n), lens, offs)), st1)
        assert [tk.len for tk in tickets] == lens and [A.slot_len(s) for s in range(n)] == lens
        perm = [(3 * s + 1) % (n + 2) for s in range(n)]                   # n + 2 = 8 slots: 3 s + 1 mod 8 is a permutation
        assert len(set(perm)) == n and [B.record_bytes(ln) for ln in lens] == [A.record_bytes(ln) for ln in lens]
        B.import_slots(list(zip(perm, lens, offs)), st1, tickets)
        assert [B.slot_len(p) for p in perm] == lens and sum(B.slot_len(s) >= 0 for s in range(n + 2)) == n
        back = B.export_slots(list(zip(perm, lens, offs)), st2)
        assert [bytes(x) for x in back] == [bytes(x) for x in tickets]
        h1, h2 = st1.cpu().numpy(), st2.cpu().numpy()
        assert np.array_equal(h1, h2)
        _assert_only_the_records_were_written(t, A, h1, lens, offs)
        b = _eager_over(sc, GalleryIndex, B, {k: perm[s] for k, s in a.slot_of.items()})
        over_b = b.vtg_pairs(pairs)
        assert np.array_equal(over_b, over_a) and np.array_equal(over_b, ref), (mode, float(np.max(np.abs(over_b - ref))))
    finally:
        B.close(); a.close(); G._set_mode(t, "none")


# ---- 2. chunk and length edges
def _filled_by_hand(t, sc, lens, max_len, compensated):
    """A cache whose slot s holds a prefix of lens[s] random tokens, filled by cache.fill in one packed call."""
    rng = np.random.RandomState(5)
    cache = t.model.engine.prefix_cache(len(lens), max_len, compensated)
    st = _PackState(sc, "tvg")
    for ln in lens:
        st.add_seq(rng.randint(10, 1000, size=ln), np.arange(ln), np.ones(ln, np.uint8), None)
    batch, src, feats = st.upload()
    with sc._call_options("tvg"):
        cache.fill(batch, t.model.engine.assemble(src, feats), np.arange(len(lens), dtype=np.int32))
    return cache


def test_forty_nine_moves_of_every_length_edge(tiny):
    t = tiny
    sc = G._scorer(t)
    TG._set_tvg(t, sc, "full")
    lens = ([1, 31, 32, 33, 64] * 10)[:49]
    A = _filled_by_hand(t, sc, lens, 64, bool(sc.split_tvg))
    B = t.model.engine.prefix_cache(49, 64, A.compensated)
    try:
        assert [A.slot_len(s) for s in range(49)] == lens
        offs, total = _laid_out(A, lens)
        st1, st2 = _staging(total), _staging(total)
        tickets = A.export_slots(list(zip(range(49), lens, offs)), st1)                      # 48 + 1 moves: two launches
        rev = list(range(48, -1, -1))
        B.import_slots(list(zip(rev, lens, offs)), st1, tickets)
        assert [B.slot_len(s) for s in rev] == lens
        B.export_slots(list(zip(rev, lens, offs)), st2)
        h1, h2 = st1.cpu().numpy(), st2.cpu().numpy()
        assert np.array_equal(h1, h2)
        _assert_only_the_records_were_written(t, A, h1, lens, offs)
        recs = [h1[o:o + _raw_bytes(t, A, ln)].tobytes() for ln, o in zip(lens, offs)]
        assert len(set(recs)) == 49                                        # every slot's own prefix, not one slot 49 times
        for s in (0, 4, 48):                                               # a single move, of the shortest, the longest and the last slot
            one, two = _staging(A.record_bytes(lens[s]) + 512), _staging(A.record_bytes(lens[s]) + 512)
            tk = A.export_slots([(s, lens[s], 256)], one)
            B.import_slots([(7, lens[s], 256)], one, tk)
            B.export_slots([(7, lens[s], 256)], two)
            g1 = one.cpu().numpy()
            assert np.array_equal(g1, two.cpu().numpy()) and g1[256:256 + _raw_bytes(t, A, lens[s])].tobytes() == recs[s]
            _assert_only_the_records_were_written(t, A, g1, [lens[s]], [256])
    finally:
        A.close(); B.close(); TG._set_tvg(t, sc, "full")


# ---- 3. ownership
def test_an_import_writes_its_own_slot_alone(tiny):
    t = tiny
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = G._t2v_pairs(t)
    ref = sc.vtg(pairs)
    a = GalleryIndex(sc).build()
    try:
        k0, k1 = a.keys[0], a.keys[1]
        s0, s1 = a.slot_of[k0], a.slot_of[k1]
        ln = a.cache.slot_len(s0)
        st = _staging(a.cache.record_bytes(ln))
        tk = a.cache.export_slots([(s0, ln, 0)], st)
        a.cache.import_slots([(s1, ln, 0)], st, tk)                        # video 0's prefix now also in the slot of video 1
        others = pairs[pairs[:, 0] != k1[0]]
        assert len(others) and np.array_equal(a.vtg_pairs(others), ref[pairs[:, 0] != k1[0]])
        moved = _eager_over(sc, GalleryIndex, a.cache, {k: s for k, s in a.slot_of.items() if k not in (k0, k1)} | {k0: s1})
        got = moved.vtg_pairs(pairs)                                       # video 0 read from the slot of video 1, video 1 from the batch
        assert np.array_equal(got, ref)
    finally:
        a.close()


@pytest.mark.parametrize("mode", ["attn", "full"])
def test_a_shorter_record_into_a_slot_that_held_a_longer_prefix(tiny, mode):
    t = tiny
    sc, tg = TG._index(t, mode)
    try:
        lens = [len(p) for p in sc.tvg_split]
        long_, short = int(np.argmax(lens)), int(np.argmin(lens))
        k_long, k_short = sc.tvg_split[long_].tobytes(), sc.tvg_split[short].tobytes()
        s_long, s_short = tg.slot_of[k_long], tg.slot_of[k_short]
        assert tg.cache.slot_len(s_long) == lens[long_] > lens[short] == tg.cache.slot_len(s_short)
        st = _staging(tg.cache.record_bytes(lens[short]))
        tk = tg.cache.export_slots([(s_short, lens[short], 0)], st)
        tg.cache.import_slots([(s_long, lens[short], 0)], st, tk)
        assert tg.cache.slot_len(s_long) == lens[short]
        moved = _eager_over(sc, TextGalleryIndex, tg.cache, {k_short: s_long})
        pair = np.array([[1, short]], np.int64)
        want = sc.tvg(pair)
        assert np.all(np.isfinite(want)) and np.array_equal(moved.tvg_pairs(pair), want)      # positions beyond the short prompt hold the long one's K / V
    finally:
        tg.close(); TG._set_tvg(t, sc, "full")


# ---- 4. the index
PASSES = ((0, 1), (2, 3, 0), (4, 5), (1, 2, 5))


def _tiered(sc, capacity, cls=GalleryIndex, records=None):
    gal = cls(sc, fill="lazy", host_budget_bytes=0)
    gal.budget_bytes = capacity * gal.per_slot_bytes()
    probe = sc.engine.prefix_cache(1, gal.slot_positions(), gal.compensated())
    gal.host_budget_bytes = (len(gal.keys) if records is None else records) * probe.record_bytes(gal.slot_positions())
    probe.close()
    gal.build()
    assert gal.n_slots == capacity and gal.host is not None and gal.host.n_records == (len(gal.keys) if records is None else records)
    assert gal.host.arena.is_pinned() and gal.host.arena.numel() <= 8 << 20
    return gal


@pytest.mark.parametrize("mode", ["none", "full"])
def test_the_index_restores_what_it_spilled(tiny, mode):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, mode)
    sc = LZ._scorer(t, max_tokens=96, second_split=(1, 3, 5))
    sc.set_vtg_mode(t.model.vtg_mode())
    gal = _tiered(sc, n // 2)
    plain = LZ._lazy(sc, capacity=n // 2)
    try:
        for videos in PASSES:
            pairs = np.array([[j, i] for j in videos for i in range(n)], np.int64)
            want = sc.vtg(pairs)
            assert np.all(np.isfinite(want))
            for _ in range(2):
                got = gal.vtg_pairs(pairs)
                assert np.array_equal(got, want), (videos, float(np.max(np.abs(got - want))))
                assert np.array_equal(plain.vtg_pairs(pairs), want)
        hs = gal.host.stats
        assert hs.spilled > 0 and hs.restored > 0 and hs.bytes_to_host > 0 and hs.bytes_from_host > 0
        assert set(gal.stats.as_dict()) == {"hits", "misses", "admitted", "evicted", "prefix_tokens_packed"}
        # a pass whose keys all have a slot or a record packs no prefix token: video 0 lost its slots two passes ago
        keys0 = [k for k in gal.keys if k[0] == 0]
        assert len(keys0) == 2 and all(k not in gal.slot_of and gal.host.has(k) for k in keys0) and all(k not in plain.slot_of for k in keys0)
        pairs = np.array([[0, i] for i in range(n)], np.int64)
        want = sc.vtg(pairs)
        restored = hs.restored
        got, d = LZ._delta(gal, lambda: gal.vtg_pairs(pairs))
        assert np.array_equal(got, want)
        assert d["prefix_tokens_packed"] == 0 and d["hits"] == 2 and d["misses"] == 0 and hs.restored == restored + 2
        got, d = LZ._delta(plain, lambda: plain.vtg_pairs(pairs))
        assert np.array_equal(got, want) and d["prefix_tokens_packed"] > 0 and d["hits"] == 0
    finally:
        gal.close(); plain.close(); G._set_mode(t, "none")
    assert gal.host is None


# ---- 5. the text gallery
@pytest.mark.parametrize("mode", ["attn", "full"])
def test_text_gallery_prompts_of_unequal_length_through_the_tier(tiny, mode):
    t = tiny
    sc = G._scorer(t)
    TG._set_tvg(t, sc, mode)
    tg = _tiered(sc, 1, cls=TextGalleryIndex)
    try:
        lens = [len(p) for p in sc.tvg_split]
        long_, short = int(np.argmax(lens)), int(np.argmin(lens))
        assert lens[long_] > lens[short] and tg.cache.compensated == bool(sc.split_tvg)
        #                 hits misses admitted evicted | restored spilled
        script = ((long_, (0, 1, 1, 0), (0, 0)), (short, (0, 1, 1, 1), (0, 1)), (long_, (1, 0, 0, 1), (1, 1)), (short, (1, 0, 0, 1), (1, 0)),
                  (short, (1, 0, 0, 0), (0, 0)), (long_, (1, 0, 0, 1), (1, 0)))
        for i, want_d, want_h in script:
            pairs = np.array([[1, i]], np.int64)
            h0 = (tg.host.stats.restored, tg.host.stats.spilled)
            got, d = LZ._delta(tg, lambda: tg.tvg_pairs(pairs))
            want = sc.tvg(pairs)
            assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == want_d, (i, d)
            assert (tg.host.stats.restored - h0[0], tg.host.stats.spilled - h0[1]) == want_h
            assert np.all(np.isfinite(want)) and np.array_equal(got, want), (i, got, want)
            assert tg.cache.slot_len(0) == lens[i]
    finally:
        tg.close(); TG._set_tvg(t, sc, "full")


# ---- 6. staleness
def test_a_weight_change_drops_the_records_and_an_old_ticket_is_refused_at_scoring_time(tiny):
    t = tiny
    n = t.spec["n"]
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    pairs = G._t2v_pairs(t)
    gal = _tiered(sc, n // 2)
    eager = GalleryIndex(sc).build()
    try:
        first, second = pairs[pairs[:, 0] < n // 2], pairs[pairs[:, 0] >= n // 2]
        for part in (first, second, first):
            assert np.array_equal(gal.vtg_pairs(part), sc.vtg(part))
        assert len(gal.host.rec_of) > 0 and gal.host.stats.restored > 0
        plans = list(eager.iter_plans(pairs))
        used = [int(s) for s in plans[0].slots_used]
        lens = [eager.cache.slot_len(s) for s in used]
        offs, total = _laid_out(eager.cache, lens)
        st = _staging(total)
        old = eager.cache.export_slots(list(zip(used, lens, offs)), st)
        t.model.engine.load_weight("final_norm", t.w["final_norm"] * 1.01)
        records, dropped, restored = len(gal.host.rec_of), gal.host.stats.dropped, gal.host.stats.restored
        got = gal.vtg_pairs(first)                                         # the index: its slots and its records are of the old weights
        assert gal.host.stats.dropped == dropped + records and gal.host.stats.restored == restored and gal.host.rec_of == {}
        assert np.array_equal(got, sc.vtg(first))
        assert np.array_equal(gal.vtg_pairs(second), sc.vtg(second)) and np.array_equal(gal.vtg_pairs(first), sc.vtg(first))
        assert gal.host.stats.restored > restored                          # ... and the tier works on, over records of the new weights
        assert np.array_equal(eager.vtg_pairs(pairs), sc.vtg(pairs))       # directly: slots of the new weights (the eager index refilled them) ...
        plans = list(eager.iter_plans(pairs))
        assert [int(s) for s in plans[0].slots_used] == used and [eager.cache.slot_len(s) for s in used] == lens
        eager.s.run(plans[0], eager.cache)
        eager.cache.import_slots(list(zip(used, lens, offs)), st, old)     # ... take the old records: the tickets import, with the state they recorded,
        assert [eager.cache.slot_len(s) for s in used] == lens
        with pytest.raises(eng.BlimError, match="stale"):                  # and the engine refuses their slots when a call names them
            eager.s.run(plans[0], eager.cache)
    finally:
        t.model.engine.load_weight("final_norm", t.w["final_norm"])
        gal.close(); eager.close()


# ---- 7. refusals
def test_refusals_are_host_side(tiny):
    t = tiny
    G._set_mode(t, "none")
    sc = G._scorer(t)
    sc.set_vtg_mode(t.model.vtg_mode())
    a = GalleryIndex(sc).build()
    A = a.cache
    E = t.model.engine
    other = E.prefix_cache(2, A.max_len, True)                             # another geometry: the lo parts
    try:
        ln = A.slot_len(0)
        rb = A.record_bytes(ln)
        assert A.slot_len(1) == ln and A.record_bytes(0) == -1 and A.record_bytes(A.max_len + 1) == -1
        st = _staging(2 * rb)
        good = [(0, ln, 0), (1, ln, rb)]
        tk = A.export_slots(good, st)
        before = st.cpu().numpy().copy()

        def refused(call, moves, match, staging=st, tickets=None, code=None):
            with pytest.raises(eng.BlimError, match=match) as err:
                call(moves, staging, *(() if tickets is None else (tickets,)))
            assert code is None or f"(code {code})" in str(err.value)
        for call, tks in ((A.export_slots, None), (A.import_slots, tk)):
            refused(call, [], "at least 1", tickets=None if tks is None else [], code=-1)
            refused(call, [(0, ln, 0), (A.n_slots, ln, rb)], "move 1 outside", tickets=tks, code=-1)
            refused(call, [(0, ln, 0), (-1, ln, rb)], "outside", tickets=tks, code=-1)
            refused(call, [(0, ln, 0), (0, ln, rb)], r"twice \(move 1\)", tickets=tks, code=-1)
            refused(call, [(0, ln, 0), (1, ln, rb + 128)], "move 1 is not a multiple of 256", tickets=tks, code=-1)
            refused(call, [(0, ln, 0), (1, ln, rb + 256)], "move 1 .* does not fit the staging", tickets=tks, code=-1)
            refused(call, [(0, ln, 0), (1, ln, rb - 256)], "moves 0 and 1 overlap", tickets=tks, code=-1)
            refused(call, [(0, ln, rb - 256), (1, ln, 0)], "moves 1 and 0 overlap", tickets=tks, code=-1)
        spare = E.prefix_cache(2, A.max_len, False)
        try:
            refused(spare.export_slots, [(0, ln, 0)], "never filled", code=-3)
            refused(spare.import_slots, [(0, ln, 0), (1, ln, rb)], "len", tickets=[tk[0], _with(tk[1], len=ln - 1)], code=-1)
        finally:
            spare.close()
        refused(A.export_slots, [(0, ln, 0), (1, ln - 1, rb)], "move 1 is not slot 1's filled length", code=-1)
        refused(A.import_slots, good, "ticket of move 1 was not written", tickets=[tk[0], _with(tk[1], magic=0)], code=-1)
        refused(A.import_slots, good, "ticket of move 1 has another geometry", tickets=[tk[0], _with(tk[1], kv_w=tk[1].kv_w * 2)], code=-1)
        refused(other.import_slots, good, "ticket of move 0 has another geometry", tickets=tk, code=-1)
        refused(A.import_slots, [(0, ln, 0), (1, ln - 1, rb)], "len", tickets=tk, code=-1)
        refused(A.import_slots, [(0, ln, 0), (1, 0, rb)], "len 0 of move 1", tickets=tk, code=-1)
        big = _staging(4 * rb)
        refused(A.import_slots, [(0, A.max_len + 1, 0)], "does not fit a slot", staging=big, tickets=[_with(tk[0], len=A.max_len + 1)], code=-1)
        with pytest.raises(AssertionError):                                # staging is device memory, like every data pointer of the ABI
            A.export_slots(good, torch.empty(2 * rb, dtype=torch.uint8))
        # nothing was launched by any of them, and no slot lost its state
        assert np.array_equal(st.cpu().numpy(), before) and [A.slot_len(s) for s in range(A.n_slots)] == [ln] * A.n_slots
        pairs = G._t2v_pairs(t)
        assert np.array_equal(a.vtg_pairs(pairs), sc.vtg(pairs))
        # the Python layer: an arena that is not pinned, a tier under an eager index
        with pytest.raises(ValueError, match="pinned"):
            HostTier(A, A.max_len, 4 * rb, arena=torch.empty(4 * rb, dtype=torch.uint8))
        with pytest.raises(ValueError, match="lazy"):
            GalleryIndex(sc, host_budget_bytes=1 << 20)
        with pytest.raises(ValueError, match="lazy"):
            TextGalleryIndex(sc, fill="eager", host_budget_bytes=1 << 20)
    finally:
        other.close(); a.close()


def _with(ticket, **fields):
    import ctypes as C
    out = eng.PcTicket()
    C.memmove(C.byref(out), C.byref(ticket), C.sizeof(eng.PcTicket))
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def test_fp8_engines_have_no_cache_to_export():
    t = P._build("tiny", dtype="f8")
    try:
        with pytest.raises(eng.BlimError, match="fp8"):
            t.model.engine.prefix_cache(2, 32, False)
        with pytest.raises(ValueError, match="fp8"):
            GalleryIndex(G._scorer(t), fill="lazy", host_budget_bytes=1 << 20)
    finally:
        t.model.engine.close()


# ---- 8. the CLI
def test_search_cli_prints_the_same_lines_with_the_tier():
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)
    slot = GL.cache_bytes(dims, 1, 64, False)                              # the dry run's 58-token prefixes: slots of 64 positions
    base = [sys.executable, "-m", "blim_amd.search", "--synthetic", "8", "--query_ids", "0", "2", "0", "2", "--topk", "4", "--vtg_precise", "none",
            "--gallery_fill", "lazy", "--gallery_gb", repr(2.5 * slot / 2**30)]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    for name, more in (("plain", []), ("tier", ["--gallery_host_gb", repr(8.5 * slot / 2**30)])):
        r = subprocess.run(base + more, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = r
        assert "2 slots" in r.stderr
    assert runs["tier"].stdout == runs["plain"].stdout and len(runs["plain"].stdout.splitlines()) == 4
    assert "host tier" not in runs["plain"].stderr
    err = runs["tier"].stderr.splitlines()
    at = [n for n, line in enumerate(err) if line.startswith("gallery stats: ")]
    assert len(at) == 1 and err[at[0] + 1].startswith("gallery host tier: ")
    stats = json.loads(err[at[0]].split("gallery stats: ")[1])
    tier = json.loads(err[at[0] + 1].split("gallery host tier: ")[1])
    plain = json.loads(runs["plain"].stderr.split("gallery stats: ")[1].splitlines()[0])
    assert set(stats) == set(plain) == {"hits", "misses", "admitted", "evicted", "prefix_tokens_packed"}
    assert tier["records"] == 8 and tier["spilled"] >= 1 and tier["restored"] >= 1
    assert stats["hits"] == plain["hits"] + tier["restored"] and stats["prefix_tokens_packed"] < plain["prefix_tokens_packed"]     # the slots go to the same keys either way
    r = subprocess.run(base[:-4] + ["--gallery_host_gb", "0.01"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--gallery_fill lazy" in r.stderr
