"""CPU: the gallery index's host side (blim_amd/gallery.py, blim_amd/search.py) -- cached plan construction (pfx_slot, negative row references, the
tokenizer_model_max_length cut, slots under a budget, the (video, pre, post) key), plans without a slot against the scorer's own, the cache's byte size and the
CLI's refusals.  The GPU side is tests/test_gallery_gpu.py."""
import types

import numpy as np
import pytest
import torch

from blim_amd import engine as eng
from blim_amd import gallery as GL
from blim_amd import search as SR
from blim_amd import synth
from blim_amd.pair_scorer import PairScorer
from blim_amd.synth import IGNORE_INDEX, IMAGE_TOKEN_INDEX

H, NV = 16, 5           # hidden size, video tokens per video


def _fake_scorer(texts, n_videos=4, max_row_len=None, max_tokens=4096):
    """A PairScorer with host-only stand-ins for the engine and the projector: texts = [(pre, post, resp)]."""
    s = PairScorer.__new__(PairScorer)
    s.vtg_split = [(np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(r, np.int64)) for a, b, r in texts]
    s.video = [np.zeros((1, NV, 8), np.float32) for _ in range(n_videos)]
    s._upcoming, s._upcoming_pos = {}, {}
    feats = {j: torch.full((NV, H), float(j)) for j in range(n_videos)}
    s.video_feat = lambda j, tvg: feats[int(j)]
    s.max_tokens, s.max_row_len, s.device = max_tokens, max_row_len, "cpu"
    s.split_vtg, s.split_tvg, s.vtg_mode = False, False, None
    s.m = types.SimpleNamespace(dims=types.SimpleNamespace(hidden_size=H), dtype=torch.float32)
    s.engine = types.SimpleNamespace(dtype="f16")
    return s


class _FakeCache:
    def __init__(self, lens):
        self.lens = lens

    def slot_len(self, slot):
        return self.lens[slot]


def _gallery(scorer, slots):
    g = GL.GalleryIndex(scorer)
    g.slot_of = {g.keys[k]: s for k, s in slots.items()}
    g.cache = _FakeCache({s: g.prefix_len(g.keys[k]) for k, s in slots.items()})
    return g


def test_keys_are_video_and_prompt_split():
    s = _fake_scorer([([1, 2], [3], [7, 8, 9]), ([1, 2], [3], [5, 6]), ([1], [4, 4], [5, 6])], n_videos=3)
    g = GL.GalleryIndex(s)
    assert len(g.splits) == 2                                  # two distinct (pre, post) splits over three texts
    assert len(g.keys) == 3 * 2
    assert g.keys[0] == (0, np.array([1, 2], np.int64).tobytes(), np.array([3], np.int64).tobytes())
    assert g.prefix_len(g.keys[0]) == 2 + NV + 1


def test_cached_plan_names_slots_and_cached_rows():
    texts = [([1, 2], [3], [7, 8, 9]), ([1, 2], [3], [5]), ([1, 2], [3], [6, 6])]
    s = _fake_scorer(texts, n_videos=2)
    g = _gallery(s, {0: 0})                                    # video 0 cached in slot 0, video 1 in the batch
    pairs = np.array([[0, 0], [0, 1], [1, 0], [0, 2]])
    plans = list(g.iter_plans(pairs))
    assert len(plans) == 1
    p = plans[0]
    plen = 2 + NV + 1
    slot = p.pfx_slot.numpy().tolist()
    rows = p.rows.numpy()
    assert list(p.slots_used) == [0]
    # video 0 (cached): text 0 -> body of 2 tokens, text 2 -> body of 1 token, text 1 -> one-token response: the cached row alone
    # video 1 (in batch): its prefix sequence, then text 0's body
    assert slot == [0, 0, -1, -1]
    pfx_len = p.batch.pfx_len.numpy().tolist()
    assert pfx_len == [plen, plen, 0, plen]
    rs = p.row_start.numpy()
    per_pair = [rows[rs[k]:rs[k + 1]].tolist() for k in range(p.n_pairs)]
    assert per_pair[0] == [-1, 0, 1]                          # (video 0, text 0): cached last row of slot 0, then the own rows
    assert per_pair[1] == [-1]                                # (video 0, text 1)
    assert per_pair[2] == [-1, 2]                             # (video 0, text 2)
    assert per_pair[3][0] == 3 + plen - 1                     # (video 1, text 0): the in-batch prefix's last row
    assert p.n_tokens == 2 + 1 + plen + 2
    # positions of a cached continuation follow the slot's prefix
    assert p.batch.positions.numpy()[:2].tolist() == [plen, plen + 1]
    assert np.concatenate(p.out_index).tolist() == [0, 1, 3, 2]


def test_all_cached_one_token_responses_keep_the_batch_non_empty():
    s = _fake_scorer([([1, 2], [3], [5])], n_videos=2)
    g = _gallery(s, {0: 0, 1: 1})
    p = next(g.iter_plans(np.array([[0, 0], [1, 0]])))
    assert p.n_tokens == 1 and p.pfx_slot.numpy().tolist() == [-1]
    assert p.rows.numpy().tolist() == [-1, -2]


def test_rows_cut_at_tokenizer_model_max_length():
    plen = 2 + NV + 1
    s = _fake_scorer([([1, 2], [3], [7, 8, 9, 10])], n_videos=1, max_row_len=plen + 2)
    g = _gallery(s, {0: 0})
    p = next(g.iter_plans(np.array([[0, 0]])))
    assert p.labels.numpy().tolist() == [7, 8]
    assert p.rows.numpy().tolist() == [-1, 0]
    s = _fake_scorer([([1, 2], [3], [7])], n_videos=1, max_row_len=plen)
    with pytest.raises(ValueError, match="tokenizer_model_max_length"):
        next(_gallery(s, {0: 0}).iter_plans(np.array([[0, 0]])))


def test_slot_plan_under_a_budget():
    keys = [(j, b"", b"") for j in range(5)]
    assert GL.slot_plan(keys, 100, None) == {k: i for i, k in enumerate(keys)}
    assert GL.slot_plan(keys, 100, 250) == {keys[0]: 0, keys[1]: 1}
    assert GL.slot_plan(keys, 100, 350, priority=[4, 2, 0, 1, 3]) == {keys[4]: 0, keys[2]: 1, keys[0]: 2}
    assert GL.slot_plan(keys, 100, 99) == {}
    with pytest.raises(ValueError):
        GL.slot_plan(keys, 100, None, priority=[0, 0, 1, 2, 3])


def test_cache_byte_size_formula():
    d = synth.ModelDims()                                     # 7B: 28 layers, 4 KV heads of 128, H 3584
    assert GL.cache_bytes(d, 1, 320, False) == (28 * 320 * 1024 + 3584) * 2
    assert GL.cache_bytes(d, 10, 320, True) == 10 * (28 * 320 * 2048 + 2 * 3584) * 2


def test_abi_declares_the_cache_entry_points():
    syms = set(eng.declared_symbols())
    for s in ("blim_prefix_cache_bytes", "blim_prefix_cache_create", "blim_prefix_cache_destroy", "blim_prefix_cache_fill", "blim_prefix_cache_slot_len",
              "blim_score_vtg_cached"):
        assert s in syms
    assert "#define BLIM_ABI_VERSION 9" in open(eng.HEADER_PATH).read()


@pytest.mark.parametrize("argv,msg", [
    (["--dtype", "f8", "--query_ids", "0"], "f8"),
    (["--shard", "2", "0", "--query_ids", "0"], "shard"),
    ([], "query"),
    (["--query", "a dog runs"], "candidates all"),
    (["--query", "a dog", "--candidates", "all", "--synthetic", "8"], "tokenizer"),
    (["--query_ids", "0", "--calibration_store", "/tmp/store"], "calibration_store"),
    (["--query_ids", "0", "--second_pass", "auto"], "second_pass auto"),
    (["--query_ids", "0", "--c", "1", "0", "0", "0"], "c2 = 0"),
])
def test_cli_refusals(argv, msg):
    args = SR.get_args_parser().parse_args(argv)
    with pytest.raises(SystemExit, match=msg):
        SR.check_args(args)


def test_cli_refuses_more_than_one_rank():
    args = SR.get_args_parser().parse_args(["--query_ids", "0"])
    with pytest.raises(SystemExit, match="world size"):
        SR.check_args(args, world=2)
    SR.check_args(args, world=1)


def test_cli_default_blend_reranks_by_the_likelihood():
    args = SR.get_args_parser().parse_args(["--query_ids", "0"])
    SR.check_args(args)
    assert args.c[0] == 1.0 and args.c[2] == 1.0


def test_prior_memo_is_dropped_after_a_weight_or_mode_change():
    s = _fake_scorer([([1, 2], [3], [5, 6])], n_videos=2)
    s.tvg_split = [np.array([9, 8, 7], np.int64)]
    s.m.tvg_prefix_length = 2
    s.engine.weights_version = 0
    s.tvg_mode = "full"
    calls = []

    def tvg(pairs, cpn=False):
        calls.append(len(pairs))
        return np.full(len(pairs), float(s.engine.weights_version), np.float32)
    s.tvg = tvg
    g = GL.GalleryIndex(s)
    cand = np.array([[0, 1]])
    assert g._t2v_prior([0], cand).tolist() == [[0.0, 0.0]]
    assert g._t2v_prior([0], cand).tolist() == [[0.0, 0.0]] and calls == [2]      # memoised
    s.engine.weights_version = 1                                                     # a weight / adapter change
    assert g._t2v_prior([0], cand).tolist() == [[1.0, 1.0]] and calls == [2, 2]
    s.tvg_mode = "attn"                                                              # a TVG mode change
    g._t2v_prior([0], cand)
    assert calls == [2, 2, 2]


def plan_difference(a, b):
    """None when two plans are the same call, array for array; else the name of the first field that differs (pfx_slot / slots_used apart: only a plan made
    over a prefix source carries them)."""
    for k in ("positions", "key_visible", "seq_start", "seq_len", "pfx_start", "pfx_len", "own_start", "blk_seq", "blk_q0"):
        x, y = getattr(a.batch, k), getattr(b.batch, k)
        if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
            return "batch." + k
    for k in ("src_index", "rows", "labels", "row_start", "feats"):
        x, y = getattr(a, k), getattr(b, k)
        if (x is None) != (y is None) or (x is not None and not (x.dtype == y.dtype and torch.equal(x, y))):
            return k
    if [o.tolist() for o in a.out_index] != [o.tolist() for o in b.out_index]:
        return "out_index"
    for k in ("kind", "n_pairs", "n_tokens", "n_rows"):
        if getattr(a, k) != getattr(b, k):
            return k
    return None


def _random_texts(n):
    """Two prompt splits, responses of 1 - 4 tokens."""
    return [([1, i % 2], [2], list(range(3, 4 + i % 4))) for i in range(n)]


@pytest.mark.parametrize("max_tokens", [64, 4096])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_plans_without_a_slot_are_the_scorers_own(C, max_tokens):
    rng = np.random.RandomState(10 * C + max_tokens)
    s = _fake_scorer(_random_texts(5), n_videos=4, max_tokens=max_tokens)
    s.num_clips = C
    pairs = np.stack([rng.randint(0, 4, 40), rng.randint(0, 5, 40)], axis=1)
    got, want = list(GL.GalleryIndex(s).iter_plans(pairs)), list(s.iter_vtg(pairs))
    assert len(got) == len(want) and (len(want) > 1) == (max_tokens == 64)
    assert [plan_difference(a, b) for a, b in zip(got, want)] == [None] * len(want)
    assert all(p.pfx_slot is None and p.slots_used is None for p in want)
    assert all(np.all(p.pfx_slot.numpy() == -1) and len(p.slots_used) == 0 for p in got)


def test_planning_cached_videos_projects_none():
    s = _fake_scorer(_random_texts(5), n_videos=4, max_tokens=64)
    calls = []
    s.video_feat = lambda j, tvg: calls.append(j) or torch.zeros((NV, H))
    g = _gallery(s, {k: k for k in range(4 * 2)})                # every (video, split) prefix has a slot
    rng = np.random.RandomState(2)
    pairs = np.stack([rng.randint(0, 4, 40), rng.randint(0, 5, 40)], axis=1)
    plans = list(g.iter_plans(pairs))
    assert sum(p.n_pairs for p in plans) == 40 and calls == []
    g = _gallery(s, {k: k for k in range(2, 4 * 2)})             # ... all but video 0's: it alone is projected
    list(g.iter_plans(pairs))
    assert calls and set(calls) == {0}
