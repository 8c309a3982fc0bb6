"""CPU: the text gallery's host side (blim_amd/gallery.py: TextGalleryIndex; blim_amd/search.py --direction v2t) -- cached TVG plan construction (no prompt sequence
for a cached text, pfx_slot / pfx_len, the negative first row, merged segments, num_clips == 1, SEG_MAX chunks), token counts, slots under a budget, shared slots of
duplicate prompts, plans without a slot against the scorer's own, the v2t blend against combine_and_rank and the CLI's refusals.  The GPU side is tests/test_text_gallery_gpu.py."""
import types

import numpy as np
import pytest
import torch

from blim_amd import engine as eng
from blim_amd import gallery as GL
from blim_amd import search as SR
from blim_amd import synth
from blim_amd import training_utils as TU
from blim_amd.pair_scorer import PairScorer
from test_gallery_host import plan_difference

H = 16


def _fake_scorer(prompts, n_videos=4, C=4, max_tokens=4096):
    """A PairScorer with host-only stand-ins for the engine and the projector: prompts = the texts' caption prompts (token lists)."""
    s = PairScorer.__new__(PairScorer)
    s.tvg_split = [np.asarray(p, np.int64) for p in prompts]
    s.vtg_split = [(np.array([1], np.int64), np.array([2], np.int64), np.array([3, 4], np.int64)) for _ in prompts]
    s.video = [np.zeros((1, 5, 8), np.float32) for _ in range(n_videos)]
    s._upcoming, s._upcoming_pos = {}, {}
    feats = {j: torch.full((max(C - 1, 1), H), float(j)) for j in range(n_videos)}
    s.video_feat = lambda j, tvg: feats[int(j)]
    s.num_clips = C
    s.tvg_video_labels = np.arange(100, 100 + n_videos).astype(np.int32)
    s.max_tokens, s.max_row_len, s.device = max_tokens, None, "cpu"
    s.split_vtg, s.split_tvg, s.vtg_mode, s.tvg_mode = False, False, None, "full"
    s.m = types.SimpleNamespace(dims=types.SimpleNamespace(hidden_size=H), dtype=torch.float32)
    d7 = synth.ModelDims()
    s.engine = types.SimpleNamespace(dtype="f16", weights_version=0, prefix_cache_bytes=lambda n, L, comp: GL.cache_bytes(d7, n, L, comp))
    return s


class _FakeCache:
    def __init__(self, lens):
        self.lens = lens

    def slot_len(self, slot):
        return self.lens[slot]


def _index(scorer, cached_texts):
    """Slots for the prompts of the given texts, in that order."""
    g = GL.TextGalleryIndex(scorer)
    for i in cached_texts:
        g.slot_of.setdefault(scorer.tvg_split[i].tobytes(), len(g.slot_of))
    g.cache = _FakeCache({sl: len(np.frombuffer(k, np.int64)) for k, sl in g.slot_of.items()})
    return g


def _per_pair(p, C):
    rows = p.rows.numpy()
    return [rows[k * C:(k + 1) * C].tolist() for k in range(p.n_pairs)]


def test_cached_and_uncached_texts_share_a_call():
    s = _fake_scorer([[9, 8, 7, 6, 5], [9, 8, 7]], n_videos=3)
    g = _index(s, [0])                                         # text 0 cached in slot 0, text 1 keeps its in-batch prompt
    pairs = np.array([[2, 0], [1, 1]])
    plans = list(g.iter_plans(pairs))
    assert len(plans) == 1
    p = plans[0]
    assert p.kind == "tvg" and p.row_start is None
    # text 0: one sequence of 3 clip tokens over slot 0; text 1: its prompt (3 tokens), then 3 clip tokens over it
    assert p.pfx_slot.numpy().tolist() == [0, -1, -1]
    assert p.batch.pfx_len.numpy().tolist() == [5, 0, 3]
    assert p.batch.pfx_start.numpy().tolist()[2] == 3
    assert p.batch.seq_len.numpy().tolist() == [3, 3, 3]
    assert list(p.slots_used) == [0]
    pp = _per_pair(p, 4)
    assert pp[0] == [-1, 0, 1, 2]                             # the cached last prompt row of slot 0 predicts clip 0
    assert pp[1] == [3 + 3 - 1, 6, 7, 8]                      # the in-batch prompt's last row
    assert p.batch.positions.numpy().tolist() == [5, 6, 7, 0, 1, 2, 3, 4, 5]
    assert p.labels.numpy().tolist() == [102, 101]
    assert np.concatenate(p.out_index).tolist() == [0, 1]
    assert p.n_tokens == 3 + 3 + 3


def test_two_videos_of_one_text_are_one_segmented_sequence():
    s = _fake_scorer([[9, 8, 7, 6]], n_videos=3)
    g = _index(s, [0])
    p, = g.iter_plans(np.array([[2, 0], [0, 0]]))
    assert p.batch.n_seqs == 1 and p.pfx_slot.numpy().tolist() == [0]
    assert p.batch.own_start.numpy().tolist() == [0, 0, 0, 3, 3, 3]
    assert p.batch.positions.numpy().tolist() == [4, 5, 6, 4, 5, 6]
    assert _per_pair(p, 4) == [[-1, 0, 1, 2], [-1, 3, 4, 5]]
    assert p.labels.numpy().tolist() == [100, 102]            # videos in ascending order within a text
    assert np.concatenate(p.out_index).tolist() == [1, 0]


def test_all_cached_plans_pack_the_clip_tokens_alone():
    rng = np.random.RandomState(0)
    s = _fake_scorer([list(range(5, 5 + n)) for n in (4, 7, 5, 9, 6)], n_videos=4)
    g = _index(s, range(5))
    pairs = np.stack([rng.randint(0, 4, 30), rng.randint(0, 5, 30)], axis=1)
    plans = list(g.iter_plans(pairs))
    assert sum(p.n_pairs for p in plans) == 30
    for p in plans:
        assert p.n_tokens == (4 - 1) * p.n_pairs
        assert np.all(p.pfx_slot.numpy() >= 0)
    assert sorted(np.concatenate([np.concatenate(p.out_index) for p in plans]).tolist()) == list(range(30))


def test_one_clip_leaves_cached_rows_and_a_dummy_token():
    s = _fake_scorer([[9, 8, 7], [9, 8]], n_videos=2, C=1)
    g = _index(s, [0, 1])
    p, = g.iter_plans(np.array([[0, 0], [1, 1], [1, 0]]))
    assert p.n_tokens == 1 and p.pfx_slot.numpy().tolist() == [-1]       # the batch is not empty; the dummy sequence names no slot
    assert p.rows.numpy().tolist() == [-1, -1, -2]
    assert sorted(p.slots_used.tolist()) == [0, 1]
    # uncached at C == 1: the prompt alone, its last row scored
    g = _index(s, [])
    p, = g.iter_plans(np.array([[0, 0]]))
    assert p.n_tokens == 3 and p.rows.numpy().tolist() == [2]


def test_merged_sequences_are_cut_at_seg_max():
    s = _fake_scorer([[9, 8, 7]], n_videos=100)
    g = _index(s, [0])
    pairs = np.stack([np.arange(100), np.zeros(100, np.int64)], axis=1)
    p, = g.iter_plans(pairs)
    per = GL.SEG_MAX // 3
    assert p.batch.seq_len.numpy().tolist() == [3 * per, 3 * (100 - per)]
    assert p.pfx_slot.numpy().tolist() == [0, 0]
    own = p.batch.own_start.numpy()
    assert own[3 * per - 1] == 3 * (per - 1) and own[3 * per] == 0          # own_start counts from the sequence's own first token


def test_calls_are_cut_at_max_tokens():
    s = _fake_scorer([[9, 8, 7], [6, 5, 4, 3]], n_videos=8, max_tokens=12)
    g = _index(s, [0])
    pairs = np.array([[j, 0] for j in range(6)] + [[0, 1], [1, 1]])
    plans = list(g.iter_plans(pairs))
    assert all(p.n_tokens <= 12 for p in plans)
    assert [p.n_pairs for p in plans] == [4, 2, 2]             # 12 tokens of text 0 | 6 of text 0 (a prompt + one video of text 1 would not fit) | 4 + 6 of text 1
    assert plans[2].pfx_slot.numpy().tolist() == [-1, -1]


def test_slot_length_mismatch_is_an_error():
    s = _fake_scorer([[9, 8, 7]], n_videos=1)
    g = _index(s, [0])
    g.cache = _FakeCache({0: 2})
    with pytest.raises(RuntimeError, match="holds 2 positions.*text 0 has 3"):
        next(g.iter_plans(np.array([[0, 0]])))


def test_duplicate_prompts_share_a_slot():
    s = _fake_scorer([[9, 8, 7], [5, 5], [9, 8, 7]], n_videos=2)
    g = GL.TextGalleryIndex(s)
    assert len(g.keys) == 2 and g.keys[0] == np.array([9, 8, 7], np.int64).tobytes()
    g = _index(s, [0])
    p, = g.iter_plans(np.array([[0, 0], [1, 2]]))
    assert p.pfx_slot.numpy().tolist() == [0, 0] and list(p.slots_used) == [0]
    assert p.rows.numpy()[[0, 4]].tolist() == [-1, -1]


def test_slot_budget_with_tvg_slot_bytes():
    s = _fake_scorer([list(range(n)) for n in (37, 77, 50, 64)])
    s.split_tvg = True
    g = GL.TextGalleryIndex(s)
    assert g.slot_positions() == 96                           # the longest prompt rounded up to the key tile
    per = g.per_slot_bytes()
    assert per == (28 * 96 * 1024 * 2 + 2 * 3584) * 2         # 7B, compensated: 11.0 MB of K / V (+ lo) and the hidden row (hi | lo)
    assert GL.slot_plan(g.keys, per, None) == {k: i for i, k in enumerate(g.keys)}
    assert GL.slot_plan(g.keys, per, 3 * per + per // 2) == {g.keys[0]: 0, g.keys[1]: 1, g.keys[2]: 2}
    assert GL.slot_plan(g.keys, per, per - 1) == {}
    s.split_tvg = False
    assert g.per_slot_bytes() == (28 * 96 * 1024 + 3584) * 2


def test_fp8_engines_are_refused():
    s = _fake_scorer([[1, 2]])
    s.engine.dtype = "f8"
    with pytest.raises(ValueError, match="fp8"):
        GL.TextGalleryIndex(s)


def _combine_v2t(monkeypatch, ql, cand_l, prior, iv2, cpn, alpha, c, finetuned):
    """The blended v2t matrix training_utils.combine_and_rank hands to get_recall for "blim"."""
    n = iv2.shape[0]
    seen = []
    monkeypatch.setattr(TU, "get_recall", lambda t2v, v2t, a, b: seen.append(np.array(v2t)) or {})
    v2t = {"internvideo2": iv2, "candidate_likelihood": cand_l, "query_likelihood": ql, "candidate_prior": prior}
    t2v = {k: np.zeros((n, n), np.float32) for k in v2t}
    args = types.SimpleNamespace(resume="finetuned.pth" if finetuned else "", eval=True, cpn=cpn, alpha=list(alpha), c=list(c))
    TU.combine_and_rank(t2v, v2t, args, n)
    monkeypatch.undo()
    return seen[-1]


@pytest.mark.parametrize("finetuned", [False, True])
@pytest.mark.parametrize("cpn", [False, True])
def test_rerank_is_the_v2t_half_of_combine_and_rank(monkeypatch, finetuned, cpn):
    n = 6
    rng = np.random.RandomState(3)
    VT, TV, IV = (rng.randn(n, n).astype(np.float32) for _ in range(3))       # [video, text]
    PR = np.repeat(rng.randn(1, n).astype(np.float32), n, axis=0)               # the prior depends on the text only
    alpha, c = (0.8, 0.3), (0.6, 0.5, 0.7, 0.4)
    full = _combine_v2t(monkeypatch, TV, VT, PR, IV, cpn, alpha, c, finetuned)
    s = _fake_scorer([[1, 2, 3 + i] for i in range(n)], n_videos=n)
    g = GL.TextGalleryIndex(s)
    tvg_calls = []
    g.vtg_pairs = lambda pairs: VT[pairs[:, 0], pairs[:, 1]]
    g.tvg_pairs = lambda pairs: tvg_calls.append(len(pairs)) or TV[pairs[:, 0], pairs[:, 1]]
    g.v2t_prior = lambda videos, cand: PR[np.asarray(videos)[:, None], cand]
    videos = np.array([4, 0, 2])
    cand = np.stack([rng.permutation(n)[:4] for _ in videos])
    order, blended = g.rerank(videos, cand, first_stage=np.take_along_axis(IV[videos], cand, 1), cpn=cpn, alpha=alpha, c=c, finetuned=finetuned)
    for q, v in enumerate(videos):
        want = full[v, cand[q]]
        o = np.argsort(-want, kind="stable")
        assert np.array_equal(order[q], cand[q][o])
        assert np.array_equal(blended[q], want[o])
    assert bool(tvg_calls) == finetuned                        # zero-shot: no TVG call


def test_v2t_prior_memo_by_text_and_token_count():
    s = _fake_scorer([[1, 2], [1, 3], [1, 4]], n_videos=3)
    s.video[2] = np.zeros((1, 7, 8), np.float32)              # another token count: its own prior, its own pass
    calls = []

    def vtg(pairs, cpn=False):
        assert cpn
        calls.append(np.asarray(pairs).tolist())
        return np.array([10.0 * s.engine.weights_version + i + 0.01 * s.video[j].shape[1] for j, i in pairs], np.float32)
    s.vtg = vtg
    g = GL.TextGalleryIndex(s)
    got = g.v2t_prior([0, 1], np.array([[0, 1], [1, 2]]))
    assert calls == [[[0, 0], [0, 1], [1, 2]]]                # (text 1, 5 tokens) scored once, with the first video that asked
    assert got.dtype == np.float32 and np.allclose(got, [[0.05, 1.05], [1.05, 2.05]])
    g.v2t_prior([1], np.array([[0, 2]]))
    assert len(calls) == 1                                     # memoised
    got = g.v2t_prior([2, 0], np.array([[0], [0]]))
    assert calls[1] == [[2, 0]] and np.allclose(got, [[0.07], [0.05]])
    s.engine.weights_version = 1                               # a weight / adapter change drops the memo
    assert np.allclose(g.v2t_prior([0], np.array([[0]])), [[10.05]])
    s.vtg_mode = "full"                                        # ... and so does a VTG mode change
    g.v2t_prior([0], np.array([[0]]))
    assert len(calls) == 4


def test_abi_declares_the_cached_tvg_entry_point():
    assert "blim_score_tvg_cached" in set(eng.declared_symbols())
    assert "#define BLIM_ABI_VERSION 9" in open(eng.HEADER_PATH).read()


@pytest.mark.parametrize("argv,msg", [
    (["--direction", "v2t", "--video_ids", "0", "--query_ids", "1"], "not --query"),
    (["--direction", "v2t", "--video_ids", "0", "--query", "a dog"], "not --query"),
    (["--video_ids", "0", "--query_ids", "1"], "--video_ids are the queries of --direction v2t"),
    (["--direction", "v2t"], "needs --video_ids"),
    (["--direction", "v2t", "--video_ids", "0", "--c", "1", "1", "1", "0"], "c3 = 0"),
    (["--direction", "v2t", "--video_ids", "0", "--c", "1", "1", "1"], "4 values"),
    (["--direction", "v2t", "--video_ids", "0", "--dtype", "f8"], "f8"),
    (["--direction", "v2t", "--video_ids", "0", "--shard", "2", "0"], "shard"),
    (["--direction", "v2t", "--video_ids", "0", "--calibration_store", "/tmp/store"], "calibration_store"),
    (["--direction", "v2t", "--video_ids", "0", "--second_pass", "auto"], "second_pass auto"),
    # today's t2v refusals, unchanged
    (["--dtype", "f8", "--query_ids", "0"], "f8"),
    ([], "query"),
    (["--query", "a dog runs"], "candidates all"),
    (["--query_ids", "0", "--c", "1", "0", "0", "0"], "c2 = 0"),
])
def test_cli_refusals(argv, msg):
    args = SR.get_args_parser().parse_args(argv)
    with pytest.raises(SystemExit, match=msg):
        SR.check_args(args)


def test_cli_default_blend_per_direction():
    args = SR.get_args_parser().parse_args(["--query_ids", "0"])
    assert args.c is None and args.direction == "t2v"
    SR.check_args(args)
    assert args.c == [1.0, 0.0, 1.0, 0.0]
    args = SR.get_args_parser().parse_args(["--direction", "v2t", "--video_ids", "3", "4"])
    SR.check_args(args)
    assert args.c == [1.0, 0.0, 1.0, 1.0] and args.video_ids == [3, 4]          # c1 = 0, c3 = 1: the VTG likelihood alone
    args = SR.get_args_parser().parse_args(["--direction", "v2t", "--video_ids", "3", "--c", "1", "0.5", "0", "0.5"])
    SR.check_args(args)                                                            # c2 = 0 does not act on v2t
    with pytest.raises(SystemExit, match="world size"):
        SR.check_args(args, world=2)


@pytest.mark.parametrize("max_tokens", [64, 4096])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_plans_without_a_slot_are_the_scorers_own(C, max_tokens):
    rng = np.random.RandomState(10 * C + max_tokens)
    s = _fake_scorer([list(range(5, 5 + n)) for n in (4, 7, 5, 9, 6)], n_videos=4, C=C, max_tokens=max_tokens)
    pairs = np.stack([rng.randint(0, 4, 40), rng.randint(0, 5, 40)], axis=1)
    got, want = list(GL.TextGalleryIndex(s).iter_plans(pairs)), list(s.iter_tvg(pairs))
    assert len(got) == len(want) and (len(want) > 1) == (max_tokens == 64 and C > 1)
    assert [plan_difference(a, b) for a, b in zip(got, want)] == [None] * len(want)
    assert all(p.pfx_slot is None and p.slots_used is None for p in want)
    assert all(np.all(p.pfx_slot.numpy() == -1) and len(p.slots_used) == 0 for p in got)
