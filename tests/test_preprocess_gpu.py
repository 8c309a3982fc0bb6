"""GPU: frame preprocessing on the device and raw frames in extraction and search (csrc/preprocess.hip: blim_preprocess_frames;
blim_amd/vision.py: preprocess_device, VisionEncoder.video_feature_u8; blim_amd/extract.py: --preprocess device; blim_amd/search.py: add_video by `frames`,
--query_video x.npy).  The reference of every comparison is the host path -- vision.preprocess, i.e. PIL's resize and numpy's normalisation -- and every
comparison is bit for bit: the kernels are integer arithmetic on the host's taps and a lookup in the host's table.  The raw calls carry sentinels around the
output and the workspace.  The host side is tests/test_preprocess_host.py."""
import json
import os
import types

import numpy as np
import pytest
import torch

import test_preprocess_host as PH
from blim_amd import engine as eng
from blim_amd import retrieval_utils as RU
from blim_amd import search as SR
from blim_amd import synth
from blim_amd import vision as V
from blim_amd.gallery import GalleryIndex, TextGalleryIndex
from blim_amd.modeling import BlimModel, DDPLike

pytestmark = pytest.mark.gpu
GUARD = 4096                 # sentinel elements on each side of a buffer
OUT_MARK, WS_MARK = 0x7A5C, 0xA7
# (S, H, W): every path of the two passes at the smallest sizes -- one pixel; a few; both passes skipped; horizontal only; vertical only; one axis up and one down;
# 251 taps a pixel; and the extractor's 448 with two ordinary video sizes
SMALL = [(32, 1, 1), (32, 7, 5), (32, 32, 32), (32, 32, 50), (32, 50, 32), (32, 33, 31), (32, 3, 2000)]
LARGE = [(448, 240, 320), (448, 360, 640)]


def frames_of(T, H, W, seed=0):
    """uint8 [T, H, W, 3]: random, checkerboard (both clips act), smooth, ... in turn."""
    kinds = ("random", "checkerboard", "smooth")
    return np.stack([PH.frame(kinds[t % 3], H, W, seed + t) for t in range(T)])


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def host_bits(f, S, dtype):
    want = V.preprocess(f, S)
    return bits(want.to(torch.bfloat16) if dtype == "bf16" else want)


def raw_call(f, S, lut, drop=(), over=None):
    """blim_preprocess_frames on buffers with sentinels around them -> (code, out uint16 [T, 3, S, S], the out buffer's interior untouched?).  `drop`: pointer
    arguments passed as NULL; `over`: integer arguments replaced (a dict).  The sentinels around the output and the workspace are asserted here."""
    lib = V._pre_lib()
    T, H, W = f.shape[:3]
    dev = torch.device("cuda")
    x = torch.from_numpy(f).to(dev)
    tabs = {}
    for name, n in (("x", W), ("y", H)):
        if n != S:
            b, k = V.bicubic_tables(n, S)
            tabs[name] = (torch.from_numpy(b.copy()).to(dev), torch.from_numpy(k.copy()).to(dev), k.shape[1])
        else:
            tabs[name] = (None, None, 0)
    n_out, n_ws = T * 3 * S * S, (T * H * S * 3 if W != S else 0)
    assert lib.blim_preprocess_workspace_bytes(T, H, W, S) == n_ws
    out = torch.full((GUARD + n_out + GUARD,), OUT_MARK, dtype=torch.int16, device=dev)
    ws = torch.full((GUARD + n_ws + GUARD,), WS_MARK, dtype=torch.uint8, device=dev)
    table = torch.from_numpy(np.ascontiguousarray(lut).view(np.int16)).to(dev)
    ptr = {"frames": x.data_ptr(), "xb": eng._ptr(tabs["x"][0]), "xk": eng._ptr(tabs["x"][1]), "yb": eng._ptr(tabs["y"][0]), "yk": eng._ptr(tabs["y"][1]),
           "lut": table.data_ptr(), "out": out.data_ptr() + 2 * GUARD, "workspace": (ws.data_ptr() + GUARD) if n_ws else None}
    for name in drop:
        ptr[name] = None
    n = dict(T=T, H=H, W=W, S=S, xks=tabs["x"][2], yks=tabs["y"][2])
    n.update(over or {})
    rc = lib.blim_preprocess_frames(ptr["frames"], n["T"], n["H"], n["W"], n["S"], ptr["xb"], ptr["xk"], n["xks"], ptr["yb"], ptr["yk"], n["yks"], ptr["lut"],
                                    ptr["out"], ptr["workspace"], eng._stream())
    torch.cuda.synchronize()
    o, w = out.cpu().numpy().view(np.uint16), ws.cpu().numpy()
    assert (o[:GUARD] == OUT_MARK).all() and (o[GUARD + n_out:] == OUT_MARK).all(), "the output's sentinels"
    assert (w[:GUARD] == WS_MARK).all() and (w[GUARD + n_ws:] == WS_MARK).all(), "the workspace's sentinels"
    inner = o[GUARD:GUARD + n_out]
    return rc, inner.reshape(T, 3, S, S), bool((inner == OUT_MARK).all()) and bool((w == WS_MARK).all())


# ---- 1. equality with the host path
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("S,H,W", SMALL, ids=lambda v: str(v))
@pytest.mark.parametrize("T", [1, 5])
def test_small_shapes_equal_the_host_path_bit_for_bit(S, H, W, T, dtype):
    f = frames_of(T, H, W)
    want = host_bits(f, S, dtype)
    got = V.preprocess_device(f, S, dtype)
    assert got.dtype == eng.torch_dtype_of(dtype) and tuple(got.shape) == (T, 3, S, S) and got.is_cuda
    assert np.array_equal(bits(got), want), int((bits(got) != want).sum())
    rc, raw, _ = raw_call(f, S, V.normalise_lut(dtype))
    assert rc == 0 and np.array_equal(raw, want)
    again = V.preprocess_device(torch.from_numpy(f), S, dtype)                 # a torch tensor; the tables, the table and the workspace are reused
    assert np.array_equal(bits(again), want)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("S,H,W", LARGE, ids=lambda v: str(v))
def test_video_sizes_equal_the_host_path_bit_for_bit(S, H, W, dtype):
    f = frames_of(2, H, W, seed=7)
    want = host_bits(f, S, dtype)
    got = bits(V.preprocess_device(f, S, dtype))
    assert np.array_equal(got, want), int((got != want).sum())
    rc, raw, _ = raw_call(f, S, V.normalise_lut(dtype))
    assert rc == 0 and np.array_equal(raw, want)


def test_a_call_reuses_what_earlier_calls_left_on_the_device():
    f = frames_of(1, 40, 50)
    V.preprocess_device(f, 32)
    state = V._pre_state[str(torch.device("cuda", torch.cuda.current_device()))]
    held = {k: v for k, v in state.items()}
    V.preprocess_device(frames_of(1, 40, 50, seed=3), 32)
    assert set(state) == set(held) and all(state[k] is held[k] for k in held)
    small = bits(V.preprocess_device(frames_of(1, 9, 11), 32))                # a smaller video after a larger one: the larger workspace serves it
    assert state["workspace"] is held["workspace"] and np.array_equal(small, host_bits(frames_of(1, 9, 11), 32, "f16"))


# ---- 2. the bytes, read back: layout and channel order, independently of the normalisation
@pytest.mark.parametrize("S,H,W", [SMALL[1], SMALL[2], SMALL[3], SMALL[4], SMALL[5], LARGE[0]], ids=lambda v: str(v))
def test_the_output_read_as_integers_is_pils_bytes_with_the_channel_in_the_high_byte(S, H, W):
    f = frames_of(2, H, W, seed=11)
    lut = (np.arange(256, dtype=np.uint16)[None, :] + 256 * np.arange(3, dtype=np.uint16)[:, None]).astype(np.uint16)
    rc, out, _ = raw_call(f, S, lut)
    assert rc == 0
    want = np.stack([PH.pil_resize(x, S) for x in f]).transpose(0, 3, 1, 2)   # [T, 3, S, S] bytes
    assert np.array_equal(out >> 8, np.broadcast_to(np.arange(3, dtype=np.uint16)[None, :, None, None], out.shape))
    assert np.array_equal((out & 0xFF).astype(np.uint8), want)
    got = bits(V.preprocess_device(f, S, "f16", lut=lut))
    assert np.array_equal(got, out)


# ---- 3. bad arguments: refused on the host, nothing launched
def test_bad_arguments_are_refused_and_nothing_is_written():
    lib = V._pre_lib()
    f = frames_of(1, 33, 31)
    lut = V.normalise_lut("f16")
    cases = [(dict(drop=("frames",)), "null"), (dict(drop=("lut",)), "null"), (dict(drop=("out",)), "null"),
             (dict(drop=("xb",)), "horizontal"), (dict(drop=("xk",)), "horizontal"), (dict(drop=("workspace",)), "horizontal"),
             (dict(drop=("yb",)), "vertical"), (dict(drop=("yk",)), "vertical"),
             (dict(over=dict(xks=0)), "xks"), (dict(over=dict(yks=0)), "yks"), (dict(over=dict(xks=-3)), "xks"),
             (dict(over=dict(T=0)), "1 .. 8192"), (dict(over=dict(H=0)), "1 .. 8192"), (dict(over=dict(W=-1)), "1 .. 8192"), (dict(over=dict(S=0)), "1 .. 8192"),
             (dict(over=dict(T=8193)), "1 .. 8192"), (dict(over=dict(H=8193)), "1 .. 8192"), (dict(over=dict(W=8193)), "1 .. 8192"),
             (dict(over=dict(S=8193)), "1 .. 8192")]
    for more, msg in cases:
        rc, _, untouched = raw_call(f, 32, lut, **more)
        assert rc == -1 and untouched, more                                     # BLIM_ERR_ARG; every byte of the buffers still the sentinel
        assert msg in lib.blim_last_error().decode(), (more, lib.blim_last_error().decode())
    for T, H, W, S in ((0, 1, 1, 1), (1, 8193, 1, 1), (1, 1, -5, 1), (1, 1, 1, 8193)):
        assert lib.blim_preprocess_workspace_bytes(T, H, W, S) == -1 and "1 .. 8192" in lib.blim_last_error().decode()
    assert lib.blim_preprocess_workspace_bytes(2, 5, 7, 7) == 0 and lib.blim_preprocess_workspace_bytes(2, 5, 7, 3) == 2 * 5 * 3 * 3
    # a skipped pass needs none of its arguments
    rc, out, _ = raw_call(frames_of(1, 32, 32), 32, lut, drop=("xb", "xk", "yb", "yk", "workspace"), over=dict(xks=0, yks=0))
    assert rc == 0 and np.array_equal(out, host_bits(frames_of(1, 32, 32), 32, "f16"))
    rc, out, _ = raw_call(f, 32, lut)                                           # ... and the good call after the refused ones
    assert rc == 0 and np.array_equal(out, host_bits(f, 32, "f16"))


# ---- 4. the tower on raw frames
SMALL_TOWER = dict(image_size=96, depth=1)


@pytest.fixture(scope="module")
def tower():
    enc = V.VisionEncoder(V.VisionDims(**SMALL_TOWER), dtype="f16")
    enc.init_synthetic_weights(5)
    yield enc
    enc.close()


def test_video_feature_u8_equals_the_tower_on_host_preprocessed_frames(tower):
    f = frames_of(16, 60, 80, seed=2)
    want = tower.video_feature(V.preprocess(f, 96))
    got = tower.video_feature_u8(f)
    assert got.dtype == torch.float16 and tuple(got.shape) == (4, 64, 1024) and not got.is_cuda and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    assert not torch.equal(got, tower.video_feature_u8(frames_of(16, 60, 80, seed=3)))      # (the features depend on the frames)
    enc = V.VisionEncoder(V.VisionDims(**SMALL_TOWER), dtype="bf16")
    try:
        enc.init_synthetic_weights(5)
        assert torch.equal(enc.video_feature_u8(f), enc.video_feature(V.preprocess(f, 96)))
    finally:
        enc.close()


# ---- 5. extraction
def test_extract_with_device_preprocessing_writes_the_same_tensors(tmp_path, monkeypatch):
    from blim_amd import extract as X
    monkeypatch.chdir(tmp_path)
    rs = np.random.RandomState(0)
    os.makedirs("data/MSRVTT/frames")
    vids = ["video1", "video2", "video3"]
    for v in vids:
        np.save(f"data/MSRVTT/frames/{v}.npy", rs.randint(0, 256, size=(16, 120, 160, 3), dtype=np.uint8))
    base = ["--dataset", "MSRVTT", "--num_chunk", "1", "--chunk_idx", "0", "--batch_size", "2", "--synthetic", "21", "--clear"]
    assert X.main(X.get_args_parser().parse_args(base)) == 3
    host = {v: torch.load(f"data/MSRVTT/features/{v}.pth", weights_only=True) for v in vids}
    assert X.main(X.get_args_parser().parse_args(base + ["--preprocess", "device"])) == 3
    for v in vids:
        got = torch.load(f"data/MSRVTT/features/{v}.pth", weights_only=True)
        assert tuple(got.shape) == (4, 64, 1024) and got.dtype == torch.float16 and torch.isfinite(got.float()).all()
        assert torch.equal(got, host[v]), v
    assert not torch.equal(host["video1"], host["video2"])


# ---- 6. search: a video that arrives as frames
@pytest.fixture(scope="module")
def lm():
    """A two-layer scorer whose video features have the small tower's shape: 4 clips x 64 tokens x 1024."""
    dims = synth.ModelDims(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=1024)
    model = BlimModel(dims, max_positions=1024, dtype="f16")
    model.engine.init_synthetic_weights(0)
    prob = synth.make_problem(1, 4, dims, tok_per_clip=64, text_len=(3, 8))
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    model.vtg_precise = None
    yield types.SimpleNamespace(dims=dims, model=model, prob=prob)
    model.engine.close()


def _scorer(t):
    prob = t.prob
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    Tt = lambda rows: [torch.from_numpy(r) for r in rows]
    vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
    tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
    sc = RU.PairScorer(DDPLike(t.model), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video],
                       torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels), t.dims.num_clips, max_tokens=4096)
    sc.set_vtg_mode(t.model.vtg_mode())
    return sc


def _featuriser(argv):
    args = SR.get_args_parser().parse_args(argv + ["--vision_synthetic", "5"])
    SR.check_args(args)
    fz = SR.FrameFeaturiser(args, V.VisionDims(**SMALL_TOWER))
    assert fz.enc is None and fz.num_frames == 16                              # the tower is created at the first use of frames
    return args, fz


def _served(t, lines):
    args, fz = _featuriser(["--serve", "--candidates", "all", "--vtg_precise", "none"])
    sc = _scorer(t)
    gal = GalleryIndex(sc).build()
    try:
        srv = SR.Server(gal, [str(j) for j in range(len(t.prob.video))], len(t.prob.vtg_ids), None, args, content_hash=lambda x: eng.hash_device(x.contiguous().to(t.model.device)),
                        featuriser=fz)
        out = []
        summary = SR.serve(iter(lines), out.append, srv, batch_queries=4, batch_wait_ms=0.0)
        return [json.loads(x) for x in out], summary, fz.enc is not None
    finally:
        gal.close()
        fz.close()


def test_a_video_added_by_frames_is_the_video_added_by_its_features(lm, tower, tmp_path):
    f = frames_of(40, 60, 80, seed=5)                                          # 40 frames: sampled to 16 by the extractor's rule
    stack, feat = str(tmp_path / "clip.npy"), str(tmp_path / "clip.pth")
    np.save(stack, f)
    sampled = f[V.sample_frame_indices(41, 16).clip(0, 39)]
    torch.save(tower.video_feature(V.preprocess(sampled, 96)), feat)           # the file the extractor would have written (the fixture's tower: same seed)
    queries = [{"id": 2, "caption": 0, "candidates": ["0", "clip", "3"]}, {"id": 3, "caption": 2}]
    by_frames = [{"id": 0, "caption": 1}, {"id": 1, "add_video": {"vid": "clip", "frames": stack}}] + queries + [{"id": 4, "add_video": {"vid": "twin", "features": feat}}]
    by_feats = [{"id": 0, "caption": 1}, {"id": 1, "add_video": {"vid": "clip", "features": feat}}] + queries + [{"id": 4, "add_video": {"vid": "twin", "frames": stack}}]
    a, sa, tower_a = _served(lm, [json.dumps(x) for x in by_frames])
    b, sb, tower_b = _served(lm, [json.dumps(x) for x in by_feats])
    assert [x["id"] for x in a] == [0, 1, 2, 3, 4] and a[1] == {"id": 1, "added": "clip", "index": 4, "videos": 5}
    assert a[:4] == b[:4]                                                      # the same answer lines, scores included
    assert "clip" in a[2]["videos"] and len(a[3]["videos"]) == 5 and all(np.isfinite(x["scores"]).all() for x in (a[0], a[2], a[3]))
    assert "those of video 'clip'" in a[4]["error"] and a[4] == b[4]           # the same content, whichever way it came: a duplicate
    assert sa == sb and sa["videos_added"] == 1 and sa["errors"] == 1 and tower_a and tower_b
    # a tower that cannot be loaded: an error line, the process goes on
    args, _ = _featuriser(["--serve", "--candidates", "all", "--vtg_precise", "none"])
    args.vision_synthetic, args.vision_model_path = None, str(tmp_path / "no_checkpoint_here")
    fz = SR.FrameFeaturiser(args, V.VisionDims(**SMALL_TOWER))
    with pytest.raises(ValueError, match="vision tower cannot be loaded"):
        fz(sampled)


def test_a_v2t_query_video_given_as_frames_ranks_as_its_feature_file(lm, tower, tmp_path):
    f = frames_of(16, 60, 80, seed=6)
    stack, feat = str(tmp_path / "x.npy"), str(tmp_path / "x.pth")
    np.save(stack, f)
    torch.save(tower.video_feature(V.preprocess(f, 96)), feat)
    lines = []
    base = ["--direction", "v2t", "--candidates", "all", "--vtg_precise", "none", "--query_video"]
    for path in (stack, feat):
        if path == stack:
            args, fz = _featuriser(base + [path])
        else:                                                                  # (a run over feature files takes no tower flag, and makes no tower)
            args, fz = SR.get_args_parser().parse_args(base + [path]), None
            SR.check_args(args)
        try:
            feats = SR.query_video_features(args.query_video, args, featuriser=fz)
        finally:
            if fz is not None:
                assert fz.enc is not None
                fz.close()
        sc = _scorer(lm)
        v, = sc.add_videos(feats).tolist()
        gal = GalleryIndex(sc).build()
        tg = TextGalleryIndex(sc, video_index=gal)
        try:
            n = len(lm.prob.vtg_ids)
            order, blended = tg.rerank([v], np.arange(n)[None], first_stage=None, cpn=False, alpha=args.alpha, c=args.c, finetuned=False)
            lines.append({"query": "video:x", "texts": [int(i) for i in order[0]], "scores": [float(x) for x in blended[0]]})
        finally:
            tg.close(); gal.close()
    assert v == 4 and len(lines[0]["texts"]) == 4 and np.isfinite(lines[0]["scores"]).all() and lines[0] == lines[1]
