"""CPU: the host tier's host side (blim_amd/gallery.py: HostTier, `host_budget_bytes`) -- the policy with exact counts over scripted passes
(restored, spilled, dropped, evicted, hits), its determinism, the tier's own least-recently-used order, inclusive records, exports before imports, the transaction
rule of a failed import, an index without a tier, the CLI's refusals and the three entry points in blim.h and in the built library.  The engine and the cache are
fakes in the style of tests/test_lazy_gallery_host.py; the GPU side is tests/test_host_tier_gpu.py."""
import numpy as np
import pytest
import torch

import test_gallery_host as GH
import test_lazy_gallery_host as LH
from blim_amd import engine as eng
from blim_amd import gallery as GL
from blim_amd import search as SR

TEXTS = LH.TEXTS
PLEN = LH.PLEN
RB = 256                                  # the fake cache's record size


class _Mem:
    """Stands in for the pinned arena and the device staging buffer: slices that record nothing but accept copy_."""

    def __init__(self, n, pinned=True):
        self.n, self.pinned = n, pinned

    def is_pinned(self):
        return self.pinned

    def numel(self):
        return self.n

    def __getitem__(self, sl):
        return _Mem(sl.stop - sl.start, self.pinned)

    def copy_(self, src, non_blocking=False):
        assert non_blocking and src.n == self.n
        return self


class _Cache(LH._Cache):
    """The fake cache of the lazy tests, with the three calls of the tier: the log keeps what was issued, in order."""

    def __init__(self):
        super().__init__()
        self.log = []
        self.fail_import = False

    def record_bytes(self, ln):
        return RB if 1 <= ln <= 64 else -1

    def export_slots(self, moves, staging):
        assert all(self.lens.get(sl, -1) == ln for sl, ln, _ in moves) and len({off for _, _, off in moves}) == len(moves)
        self.log.append(("export", [sl for sl, _, _ in moves]))
        return [("ticket", sl, ln) for sl, ln, _ in moves]

    def import_slots(self, moves, staging, tickets):
        if self.fail_import:
            raise eng.BlimError("import failed")
        assert all(t[0] == "ticket" and t[2] == ln for t, (_, ln, _) in zip(tickets, moves))
        self.log.append(("import", [sl for sl, _, _ in moves]))
        for sl, ln, _ in moves:
            self.lens[sl] = ln


def _tiered(scorer, capacity, records, stage_records=16, cls=GL.GalleryIndex):
    g = LH._lazy(scorer, capacity, cls)
    g.cache = _Cache()
    g.host = GL.HostTier(g.cache, 64, records * RB, stage_records=stage_records, arena=_Mem(records * RB), staging=_Mem(stage_records * RB), sync=lambda: None)
    return g


def _pass(g, videos):
    h0 = g.host.stats.as_dict() if g.host is not None else {}
    _, d = LH._pass(g, LH._pairs(videos))
    if g.host is not None:
        d.update({k: v - h0[k] for k, v in g.host.stats.as_dict().items()})
    return d


def _counts(d):
    return tuple(d[k] for k in ("hits", "misses", "admitted", "evicted", "restored", "spilled", "dropped"))


SCRIPT = ([0, 1], [2, 3], [0, 1], [2, 3], [4, 0], [1], [2, 3, 4, 0], [0, 1])
#          hits misses admitted evicted restored spilled dropped
WANT = ((0, 2, 2, 0, 0, 0, 0),      # two free slots
        (0, 2, 2, 2, 0, 2, 0),      # videos 0 and 1 lose their slots and are exported
        (2, 0, 0, 2, 2, 2, 0),      # 0 and 1 come back by import; 2 and 3 are exported
        (2, 0, 0, 2, 2, 0, 0),      # 2 and 3 come back; 0 and 1 have records already: nothing is exported
        (1, 1, 1, 2, 1, 0, 0),      # 0 is restored over 2, 4 is new and admitted over 3: both losers have records
        (1, 0, 0, 1, 1, 0, 0),      # 1 restored into the slot of 0 (used before 4 in the last pass), which has a record
        (2, 2, 0, 1, 1, 0, 0),      # 4 pinned; 0 restored into the slot of 1 (has a record); 2 and 3 find no slot to take (0 and 4 are needed): misses, packed in the batch
        (2, 0, 0, 1, 1, 1, 1))      # 0 pinned; 1 restored into the slot of 4, which has no record, and none is free: that of 2 -- the oldest the pass does not need -- goes


def _run_script(g):
    return [_counts(_pass(g, v)) for v in SCRIPT]


# ---- the policy, exact counts
def test_policy_counts_over_a_scripted_sequence():
    s = GH._fake_scorer(TEXTS, n_videos=5)
    g = _tiered(s, capacity=2, records=4)
    got = _run_script(g)
    assert got == list(WANT), got
    st, hs = g.stats.as_dict(), g.host.stats.as_dict()
    assert st["hits"] == sum(w[0] for w in WANT) and st["evicted"] == sum(w[3] for w in WANT)
    assert hs["bytes_to_host"] == RB * hs["spilled"] and hs["bytes_from_host"] == RB * hs["restored"]
    assert LH._resident(g) == {0, 1} and {k[0] for k in g.host.rec_of} == {0, 1, 3, 4}
    assert set(st) == {"hits", "misses", "admitted", "evicted", "prefix_tokens_packed"}


def test_a_pass_served_by_restores_packs_no_prefix_token():
    s = GH._fake_scorer(TEXTS, n_videos=4)
    g = _tiered(s, capacity=2, records=4)
    for v in ([0, 1], [2, 3]):
        assert _pass(g, v)["prefix_tokens_packed"] == 2 * PLEN
    d = _pass(g, [0, 1])
    assert d["prefix_tokens_packed"] == 0 and d["restored"] == 2 and d["hits"] == 2
    plain = LH._lazy(GH._fake_scorer(TEXTS, n_videos=4), 2)
    for v in ([0, 1], [2, 3]):
        LH._pass(plain, LH._pairs(v))
    _, d = LH._pass(plain, LH._pairs([0, 1]))
    assert d["prefix_tokens_packed"] == 2 * PLEN and d["hits"] == 0


def test_the_policy_is_deterministic():
    runs = []
    for _ in range(2):
        g = _tiered(GH._fake_scorer(TEXTS, n_videos=5), capacity=2, records=4)
        counts = _run_script(g)
        runs.append((counts, g.cache.log, dict(g.slot_of), dict(g.host.rec_of)))
    assert runs[0] == runs[1]


# ---- the tier's own order
def test_the_least_recently_used_record_whose_key_the_pass_does_not_need_gives_way():
    s = GH._fake_scorer(TEXTS, n_videos=6)
    g = _tiered(s, capacity=1, records=2)
    for v in ([0], [1], [2]):                                            # 0 and 1 are exported: the two records
        _pass(g, v)
    assert {k[0] for k in g.host.rec_of} == {0, 1}
    d = _pass(g, [0])                                                    # 0 restored (its record is used now); 2 needs a record: that of 1 goes
    assert (d["restored"], d["spilled"], d["dropped"]) == (1, 1, 1) and {k[0] for k in g.host.rec_of} == {0, 2}
    d = _pass(g, [3])                                                    # 0 has its record (inclusive): nothing exported, nothing dropped
    assert (d["restored"], d["spilled"], d["dropped"], d["admitted"]) == (0, 0, 0, 1)
    d = _pass(g, [0])                                                    # 3 needs a record; 0's is needed by the pass: that of 2 goes, although 0's is older by spill
    assert (d["restored"], d["spilled"], d["dropped"]) == (1, 1, 1) and {k[0] for k in g.host.rec_of} == {0, 3}


def test_a_victim_without_a_record_to_take_is_lost_as_today():
    s = GH._fake_scorer(TEXTS, n_videos=3)
    g = _tiered(s, capacity=1, records=1)
    _pass(g, [0]); _pass(g, [1])                                         # 0 holds the only record
    d = _pass(g, [0])                                                    # 1 loses its slot; the one record is 0's, which the pass needs
    assert (d["restored"], d["spilled"], d["dropped"], d["evicted"]) == (1, 0, 0, 1)
    assert {k[0] for k in g.host.rec_of} == {0}
    d = _pass(g, [1])
    assert (d["restored"], d["admitted"], d["misses"]) == (0, 1, 1)


def test_inclusive_records_are_not_exported_twice():
    s = GH._fake_scorer(TEXTS, n_videos=2)
    g = _tiered(s, capacity=1, records=2)
    for v in ([0], [1], [0], [1], [0], [1]):
        _pass(g, v)
    assert g.host.stats.spilled == 2 and g.host.stats.restored == 4 and g.host.stats.dropped == 0
    assert [op for op, _ in g.cache.log].count("export") == 2


# ---- execution
def test_exports_are_issued_before_imports_and_large_transfers_are_chunked():
    s = GH._fake_scorer(TEXTS, n_videos=6)
    g = _tiered(s, capacity=3, records=6, stage_records=2)
    _pass(g, [0, 1, 2]); _pass(g, [3, 4, 5])
    del g.cache.log[:]
    _pass(g, [0, 1, 2])                                                  # three exports (3, 4, 5), then three imports, two slots at a time
    ops = [op for op, _ in g.cache.log]
    assert ops == ["export", "export", "import", "import"]
    assert [len(sl) for _, sl in g.cache.log] == [2, 1, 2, 1]
    assert sorted(sum((sl for op, sl in g.cache.log if op == "export"), [])) == sorted(sum((sl for op, sl in g.cache.log if op == "import"), []))


def test_victims_of_admissions_are_exported_at_pass_open_and_leave_when_the_call_commits():
    s = GH._fake_scorer(TEXTS, n_videos=3)
    g = _tiered(s, capacity=1, records=2)
    _pass(g, [0])
    plans = list(g.iter_plans(np.asarray(LH._pairs([1]))))               # planned, not run
    assert g.cache.log == [("export", [0])] and LH._resident(g) == {0} and {k[0] for k in g.host.rec_of} == {0}
    assert g.stats.evicted == 0 and plans[0].admits is not None
    g.run(plans[0])
    assert LH._resident(g) == {1} and g.stats.evicted == 1


def test_a_failing_import_commits_nothing():
    s = GH._fake_scorer(TEXTS, n_videos=2)
    g = _tiered(s, capacity=1, records=2)
    _pass(g, [0]); _pass(g, [1])
    slot_of, stats, host = dict(g.slot_of), g.stats.as_dict(), g.host.stats.as_dict()
    g.cache.fail_import = True
    with pytest.raises(eng.BlimError, match="import failed"):
        list(g.iter_plans(np.asarray(LH._pairs([0]))))
    assert g.slot_of == slot_of and g.stats.as_dict() == stats
    assert g.host.stats.restored == host["restored"] and g.host.stats.bytes_from_host == host["bytes_from_host"]
    g.cache.fail_import = False
    d = _pass(g, [0])
    assert (d["restored"], d["hits"], d["evicted"]) == (1, 1, 1)


def test_a_mode_or_weight_change_forgets_every_record():
    s = GH._fake_scorer(TEXTS, n_videos=3)
    g = _tiered(s, capacity=1, records=3)
    for v in ([0], [1], [2]):
        _pass(g, v)
    assert len(g.host.rec_of) == 2
    g._drop()
    assert g.host.rec_of == {} and g.host.stats.dropped == 2 and g.slot_of == {}
    d = _pass(g, [0])
    assert (d["restored"], d["admitted"]) == (0, 1)


# ---- without a tier
def test_an_index_without_a_tier_issues_no_transfer_and_counts_as_today():
    s = GH._fake_scorer(TEXTS, n_videos=4)
    g = LH._lazy(s, 2)
    g.cache = _Cache()
    assert g.host is None and g.host_budget_bytes is None
    for v in ([0, 1], [2, 3], [0, 1]):
        LH._pass(g, LH._pairs(v))
    assert g.cache.log == []
    assert g.stats.as_dict() == dict(hits=0, misses=6, admitted=6, evicted=4, prefix_tokens_packed=6 * PLEN)


def test_refusals_in_python():
    s = GH._fake_scorer(TEXTS, n_videos=2)
    with pytest.raises(ValueError, match="lazy"):
        GL.GalleryIndex(s, host_budget_bytes=1 << 20)
    with pytest.raises(ValueError, match="lazy"):
        GL.TextGalleryIndex(s, fill="eager", host_budget_bytes=1 << 20)
    assert GL.GalleryIndex(s, fill="lazy", host_budget_bytes=1 << 20).host_budget_bytes == 1 << 20
    with pytest.raises(ValueError, match="pinned"):
        GL.HostTier(_Cache(), 64, 4 * RB, arena=_Mem(4 * RB, pinned=False), staging=_Mem(4 * RB))
    with pytest.raises(ValueError, match="pinned"):                      # a real pageable tensor
        GL.HostTier(_Cache(), 64, 4 * RB, arena=torch.empty(4 * RB, dtype=torch.uint8), staging=_Mem(4 * RB))


# ---- ABI, library, CLI
def test_abi_declares_and_the_library_exports_the_slot_moves():
    names = {"blim_prefix_cache_record_bytes", "blim_prefix_cache_export", "blim_prefix_cache_import"}
    assert names <= set(eng.declared_symbols())
    header = open(eng.HEADER_PATH).read()
    assert "#define BLIM_ABI_VERSION 9" in header and "blim_pc_move" in header and "blim_pc_ticket" in header
    lib = eng.load_library()
    assert all(hasattr(lib, s) for s in names)
    import ctypes as C
    assert C.sizeof(eng.PcMove) == 16 and C.sizeof(eng.PcTicket) == 56 + eng.PC_TICKET_LAYERS


def test_cli_host_tier_flags_need_the_lazy_fill():
    p = SR.get_args_parser()
    a = p.parse_args(["--query_ids", "0"])
    assert a.gallery_host_gb is None and a.text_gallery_host_gb is None
    for flag in ("--gallery_host_gb", "--text_gallery_host_gb"):
        with pytest.raises(SystemExit, match="gallery_fill lazy"):
            SR.check_args(p.parse_args(["--query_ids", "0", flag, "0.5"]))
        with pytest.raises(SystemExit, match="gallery_fill lazy"):
            SR.check_args(p.parse_args(["--query_ids", "0", "--gallery_fill", "eager", flag, "0.5"]))
        SR.check_args(p.parse_args(["--query_ids", "0", "--gallery_fill", "lazy", flag, "0.5"]))
