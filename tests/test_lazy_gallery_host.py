"""CPU: the lazy gallery's host side (blim_amd/gallery.py `fill="lazy"`) -- the replacement policy with exact counts, the admissions a plan
carries (PairScorer._pack_vtg / _plan_tvg: Plan.admits), the transaction rule (planning alone changes nothing; a call that returned commits; a failed call does
not), the plans after a commit against an eager index's, the two new entry points in blim.h and the CLI's --gallery_fill.  The GPU side is
tests/test_lazy_gallery_gpu.py."""
import numpy as np
import pytest
import torch

import test_gallery_host as GH
import test_text_gallery_host as TH
from blim_amd import engine as eng
from blim_amd import gallery as GL
from blim_amd import search as SR

NV = GH.NV
TEXTS = [([1, 2], [3], [7, 8, 9]), ([1, 2], [3], [5]), ([1, 2], [3], [6, 6])]      # one prompt split; responses of 3, 1 and 2 tokens
PLEN = 2 + NV + 1


class _Cache:
    """What a plan reads of a cache: the filled length per slot.  The fake engine call below records what a call admitted."""

    def __init__(self):
        self.lens = {}

    def slot_len(self, slot):
        return self.lens.get(slot, -1)


def _lazy(scorer, capacity, cls=GL.GalleryIndex):
    g = cls(scorer, fill="lazy")
    g.n_slots, g.cache = capacity, _Cache()
    ran = []

    def run(plan, cache):                     # the engine call: an admitted slot holds its prefix once the call has returned
        ran.append(plan)
        for _, slot, _, ln, _ in ([] if plan.admits is None else plan.admits.tolist()):
            cache.lens[slot] = ln
        return torch.zeros(plan.n_pairs)
    scorer.run = run
    g.ran = ran
    return g


def _pass(g, pairs):
    """One pass as PairScorer.score drives it: plan k + 1 is made after call k returned."""
    before = g.stats.as_dict()
    plans = []
    for p in g.iter_plans(np.asarray(pairs)):
        g.run(p)
        plans.append(p)
    return plans, {k: v - before[k] for k, v in g.stats.as_dict().items()}


def _resident(g):
    return {k[0] for k in g.slot_of}


def _pairs(videos, text=0):
    return [[j, text] for j in videos]


# ---- the policy, exact counts
def test_policy_counts_capacity_two():
    s = GH._fake_scorer(TEXTS, n_videos=4)
    g = _lazy(s, 2)
    _, d = _pass(g, _pairs([0, 1]))                                                # A
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (0, 2, 2, 0) and _resident(g) == {0, 1}
    assert d["prefix_tokens_packed"] == 2 * PLEN
    _, d = _pass(g, _pairs([1, 2]))                                                # B: video 0 is the least recently used and not needed
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (1, 1, 1, 1) and _resident(g) == {1, 2}
    assert d["prefix_tokens_packed"] == PLEN
    for order in ([0, 1, 2, 3], [3, 2, 1, 0]):                                     # C, and C in the reverse pair order: both slots pinned
        _, d = _pass(g, _pairs(order))
        assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (2, 2, 0, 0) and _resident(g) == {1, 2}
        assert d["prefix_tokens_packed"] == 2 * PLEN
    assert sorted(g.slot_of.values()) == [0, 1]
    g.stats.reset()
    assert g.stats.as_dict() == dict(hits=0, misses=0, admitted=0, evicted=0, prefix_tokens_packed=0)


def test_lru_follows_the_order_of_use_not_of_admission():
    s = GH._fake_scorer(TEXTS, n_videos=5)
    g = _lazy(s, 3)
    _pass(g, _pairs([0, 1, 2]))
    _pass(g, _pairs([0]))                                                          # video 0 used again: 1 is now the oldest
    _, d = _pass(g, _pairs([3]))
    assert d["evicted"] == 1 and _resident(g) == {0, 2, 3}
    _, d = _pass(g, _pairs([4, 0]))                                                # 2 is older than 3
    assert d["evicted"] == 1 and _resident(g) == {0, 3, 4}


def test_a_dense_scan_keeps_its_resident_set():
    s = GH._fake_scorer(TEXTS, n_videos=6)
    g = _lazy(s, 2)
    _pass(g, _pairs(range(6)))                                                     # the first two misses take the free slots
    assert _resident(g) == {0, 1}
    for _ in range(2):
        _, d = _pass(g, _pairs(range(6)))
        assert (d["hits"], d["misses"], d["admitted"], d["evicted"]) == (2, 4, 0, 0) and _resident(g) == {0, 1}


def test_zero_capacity_admits_nothing():
    s = GH._fake_scorer(TEXTS, n_videos=2)
    g = _lazy(s, 0)
    plans, d = _pass(g, _pairs([0, 1]))
    assert all(p.admits is None for p in plans) and d["admitted"] == 0 and d["misses"] == 2 and g.slot_of == {}


# ---- the plans
def test_a_miss_with_a_free_slot_is_admitted_and_not_read_in_its_own_plan():
    s = GH._fake_scorer(TEXTS, n_videos=2)
    g = _lazy(s, 2)
    pairs = np.array([[0, 0], [0, 1], [1, 0], [0, 2]])
    plans = list(g.iter_plans(pairs))
    assert len(plans) == 1
    p = plans[0]
    rows, seq_start, seq_len = p.rows.numpy(), p.batch.seq_start.numpy(), p.batch.seq_len.numpy()
    assert p.admits.dtype == np.int32 and p.admits.shape == (2, 5)
    for (seq, slot, start, ln, row), want_slot in zip(p.admits.tolist(), (0, 1)):
        assert slot == want_slot and ln == PLEN
        assert start == seq_start[seq] and ln == seq_len[seq] and p.batch.pfx_len.numpy()[seq] == 0
        assert rows[row] == start + ln - 1
    assert np.all(p.pfx_slot.numpy() == -1) and len(p.slots_used) == 0             # the continuations keep the in-batch prefix
    assert p.prefix_tokens == 2 * PLEN
    # ... and the batch itself is the one an index without slots plans
    want = list(GL.GalleryIndex(s).iter_plans(pairs))
    assert GH.plan_difference(p, want[0]) is None and want[0].admits is None


def test_after_the_commit_the_pass_is_an_eager_index_plan():
    s = GH._fake_scorer(TEXTS, n_videos=2)
    g = _lazy(s, 2)
    pairs = np.array([[0, 0], [0, 1], [1, 0], [0, 2]])
    _pass(g, pairs)
    assert g.slot_of == {g.keys[0]: 0, g.keys[1]: 1}
    got = list(g.iter_plans(pairs))
    eager = GH._gallery(s, {0: 0, 1: 1})
    want = list(eager.iter_plans(pairs))
    assert len(got) == len(want) == 1
    a, b = got[0], want[0]
    assert GH.plan_difference(a, b) is None
    assert torch.equal(a.pfx_slot, b.pfx_slot) and np.array_equal(a.slots_used, b.slots_used) and a.admits is None and b.admits is None
    assert a.prefix_tokens == b.prefix_tokens == 0                                 # zero prefix tokens for the videos
    assert a.n_tokens == 2 + 1 + 2                                                 # the bodies alone: 2 + 0 + 1 (video 0), 2 (video 1)


def test_planning_twice_without_running_changes_nothing():
    s = GH._fake_scorer(TEXTS, n_videos=3)
    g = _lazy(s, 2)
    _pass(g, _pairs([0]))
    slot_of, stats, stamp = dict(g.slot_of), g.stats.as_dict(), dict(g._stamp)
    first = list(g.iter_plans(np.array(_pairs([1, 2]))))
    second = list(g.iter_plans(np.array(_pairs([1, 2]))))
    assert g.slot_of == slot_of and g.stats.as_dict() == stats and g._stamp == stamp and len(g.ran) == 1
    assert first[0].admits.tolist() == second[0].admits.tolist()                   # the reservations of the plans never run were dropped
    with pytest.raises(RuntimeError, match="earlier pass"):                        # ... and those plans are not run any more
        g.run(first[0])
    g.run(second[0])                                                               # video 1 takes the free slot, video 2 the slot of video 0 (not needed by the pass)
    assert _resident(g) == {1, 2} and g.stats.admitted == 1 + 2 and g.stats.evicted == 1


def test_a_failed_call_commits_nothing():
    s = GH._fake_scorer(TEXTS, n_videos=3)
    g = _lazy(s, 2)
    _pass(g, _pairs([0]))
    slot_of, stats = dict(g.slot_of), g.stats.as_dict()

    def boom(plan, cache):
        raise eng.BlimError("engine call failed")
    s.run = boom
    p = next(g.iter_plans(np.array(_pairs([1, 2]))))
    with pytest.raises(eng.BlimError):
        g.run(p)
    assert g.slot_of == slot_of and g.stats.as_dict() == stats


def test_a_pass_over_several_calls_reads_what_the_call_before_admitted():
    """max_tokens small: each video's group is a call of its own.  Two prompt splits per video share nothing; the second pass over the same pairs hits."""
    s = GH._fake_scorer(TEXTS, n_videos=3, max_tokens=PLEN + 3)
    g = _lazy(s, 3)
    pairs = np.array([[j, i] for j in range(3) for i in (0, 2)])
    plans, d = _pass(g, pairs)
    assert len(plans) == 3 and [len(p.admits) for p in plans] == [1, 1, 1] and d["admitted"] == 3
    plans, d = _pass(g, pairs)
    assert d["hits"] == 3 and d["prefix_tokens_packed"] == 0 and sum(p.n_tokens for p in plans) == 3 * (2 + 1)


def test_an_eager_index_has_no_hook_and_counts_its_static_slots():
    s = GH._fake_scorer(TEXTS, n_videos=3)
    g = GH._gallery(s, {0: 0})
    assert g.fill == "eager" and g.admit is None
    s.run = lambda plan, cache: torch.zeros(plan.n_pairs)
    plans, d = _pass(g, _pairs([0, 1, 2]))
    assert all(p.admits is None for p in plans)
    assert (d["hits"], d["misses"], d["admitted"], d["evicted"], d["prefix_tokens_packed"]) == (1, 2, 0, 0, 2 * PLEN)
    with pytest.raises(ValueError, match="fill"):
        GL.GalleryIndex(s, fill="sometimes")
    with pytest.raises(ValueError, match="priority"):
        GL.GalleryIndex(s, priority=[0, 1, 2], fill="lazy")


# ---- the text gallery: caption prompts of unequal lengths
def test_text_gallery_admits_the_prompt_and_reuses_a_slot_for_a_shorter_one():
    prompts = [[9, 8, 7, 6, 5, 4, 3], [9, 8, 7], [9, 8, 7, 6, 5]]
    s = TH._fake_scorer(prompts, n_videos=3, C=4)
    g = _lazy(s, 1, GL.TextGalleryIndex)
    plans, d = _pass(g, [[2, 0]])
    (seq, slot, start, ln, row), = plans[0].admits.tolist()
    assert (seq, slot, start, ln) == (0, 0, 0, 7) and plans[0].rows.numpy()[row] == 6          # the prompt's last row: the pair's first
    assert plans[0].pfx_slot.numpy().tolist() == [-1, -1] and d["admitted"] == 1
    plans, d = _pass(g, [[1, 0]])                                                  # a hit: three clip tokens over the slot
    assert plans[0].n_tokens == 3 and plans[0].pfx_slot.numpy().tolist() == [0] and plans[0].rows.numpy()[0] == -1 and d["hits"] == 1
    plans, d = _pass(g, [[1, 1]])                                                  # the shorter prompt takes the slot over
    assert plans[0].admits.tolist() == [[0, 0, 0, 3, 0]] and (d["admitted"], d["evicted"]) == (1, 1)
    assert g.cache.slot_len(0) == 3 and list(g.slot_of) == [np.asarray(prompts[1], np.int64).tobytes()]
    plans, d = _pass(g, [[0, 1], [0, 0]])                                          # text 1 pinned, text 0 has no slot to take
    assert (d["hits"], d["misses"], d["admitted"]) == (1, 1, 0)
    want = list(TH._index(s, [1]).iter_plans(np.array([[0, 1], [0, 0]])))
    assert TH.plan_difference(plans[0], want[0]) is None and torch.equal(plans[0].pfx_slot, want[0].pfx_slot)


# ---- ABI, library, CLI
def test_abi_declares_and_the_library_exports_the_admit_entry_points():
    syms = set(eng.declared_symbols())
    assert {"blim_score_vtg_admit", "blim_score_tvg_admit"} <= syms
    header = open(eng.HEADER_PATH).read()
    assert "#define BLIM_ABI_VERSION 9" in header and "blim_pc_admit" in header
    lib = eng.load_library()
    assert all(hasattr(lib, s) for s in ("blim_score_vtg_admit", "blim_score_tvg_admit"))


def test_cli_gallery_fill_parses_and_the_refusals_stand():
    p = SR.get_args_parser()
    assert p.parse_args(["--query_ids", "0"]).gallery_fill == "eager"
    assert p.parse_args(["--query_ids", "0", "--gallery_fill", "lazy"]).gallery_fill == "lazy"
    with pytest.raises(SystemExit):
        p.parse_args(["--gallery_fill", "never"])
    for argv, msg in ([["--dtype", "f8", "--query_ids", "0"], "f8"], [["--shard", "2", "0", "--query_ids", "0"], "shard"], [[], "query"],
                      [["--query", "a dog runs"], "candidates all"], [["--direction", "v2t"], "video_ids"]):
        with pytest.raises(SystemExit, match=msg):
            SR.check_args(p.parse_args(argv + ["--gallery_fill", "lazy"]))
    SR.check_args(p.parse_args(["--query_ids", "0", "--gallery_fill", "lazy", "--gallery_gb", "0.5"]))
