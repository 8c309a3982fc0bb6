"""CPU: frame preprocessing for the GPU and raw frames in the search service (blim_amd/vision.py: bicubic_tables, normalise_lut,
preprocess_device's argument checks; blim_amd/search.py: add_video by `frames`, --query_video x.npy, --vision_model_path / --vision_synthetic; include/blim.h:
blim_preprocess_*).  The resize rule the kernels implement is restated here in numpy, driven by vision.bicubic_tables, and must equal PIL byte for byte; the table
must equal what vision.preprocess computes for every (channel, byte).  The serve tests use tests/test_grow_host.py's fakes and a stub featuriser: no engine, no
tower.  The GPU side is tests/test_preprocess_gpu.py."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import test_grow_host as GR
from blim_amd import engine as eng
from blim_amd import search as SR
from blim_amd import vision as V

NV = GR.NV
SIZES = [(240, 320), (360, 640), (448, 300), (1080, 1920), (7, 5), (448, 448), (449, 447), (1, 1), (3, 2000), (224, 224), (720, 1280), (100, 448)]
TINY = [(7, 5), (1, 1), (3, 2000), (32, 32), (32, 50), (50, 32), (33, 31)]
KINDS = ("random", "smooth", "checkerboard")


def frame(kind, H, W, seed=0):
    """uint8 [H, W, 3].  The 0 / 255 checkerboard drives the bicubic lobes below 0 and above 255: both clips act."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "smooth":
        return (np.add.outer(np.arange(H) * 3, np.arange(W) * 5)[..., None] + np.array([0, 80, 160])).astype(np.uint8)
    return (((np.add.outer(np.arange(H) // 3, np.arange(W) // 3)[..., None] + np.arange(3)) % 2) * 255).astype(np.uint8)      # cells of 3 x 3 pixels


def resize_pass(img, out_size, axis, unclipped=False):
    """One pass of the rule in include/blim.h along `axis` of a uint8 array: acc = 1 << 21, acc += k[i] * pixel[first + i], clip(acc >> 22, 0, 255)."""
    bounds, coeffs = V.bicubic_tables(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    acc = np.full((out_size,) + src.shape[1:], 1 << 21, dtype=np.int64)
    for i in range(coeffs.shape[1]):
        live = i < bounds[:, 1]
        idx = np.where(live, bounds[:, 0] + i, 0)
        k = np.where(live, coeffs[:, i], 0).astype(np.int64)
        acc += k.reshape((-1,) + (1,) * (src.ndim - 1)) * src[idx]
    assert np.all(np.abs(acc) < 2**31)                                     # the kernels accumulate in int32
    if unclipped:
        return acc >> 22
    return np.moveaxis(np.clip(acc >> 22, 0, 255).astype(np.uint8), 0, axis)


def resize(f, S):
    """uint8 [H, W, 3] -> [S, S, 3]: horizontal then vertical, a pass skipped when its size does not change."""
    x = f if f.shape[1] == S else resize_pass(f, S, 1)
    return x if x.shape[0] == S else resize_pass(x, S, 0)


def pil_resize(f, S):
    img = Image.fromarray(f).convert("RGB")
    return np.asarray(img if img.size == (S, S) else img.resize((S, S), resample=Image.BICUBIC))


@pytest.mark.parametrize("S,sizes", [(448, SIZES), (32, TINY)])
def test_the_restated_resize_equals_pil_byte_for_byte(S, sizes):
    clipped_low = clipped_high = False
    for H, W in sizes:
        for kind in KINDS:
            f = frame(kind, H, W)
            want, got = pil_resize(f, S), resize(f, S)
            assert got.shape == want.shape == (S, S, 3)
            assert np.array_equal(got, want), (H, W, kind, int((got != want).sum()))
            if kind == "checkerboard" and W != S and W > 3:                 # the overshoot is there: unclipped sums leave 0 .. 255 on both sides
                raw = resize_pass(f, S, 1, unclipped=True)
                clipped_low, clipped_high = clipped_low or bool((raw < 0).any()), clipped_high or bool((raw > 255).any())
    assert clipped_low and clipped_high


def test_bicubic_tables_shapes_bounds_and_memo():
    for n_in, n_out in ((1280, 448), (300, 448), (1, 32), (2000, 32), (5, 448)):
        b, k = V.bicubic_tables(n_in, n_out)
        support = 2.0 * max(n_in / n_out, 1.0)
        assert b.dtype == k.dtype == np.int32 and b.shape == (n_out, 2) and k.shape == (n_out, 2 * int(np.ceil(support)) + 1)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b.sum(axis=1) <= n_in).all() and (b[:, 1] <= k.shape[1]).all()
        assert all((k[x, b[x, 1]:] == 0).all() for x in range(n_out))
        assert np.abs(k.sum(axis=1).astype(np.int64) - (1 << 22)).max() <= k.shape[1]      # normalised weights, each rounded once
        assert V.bicubic_tables(n_in, n_out)[0] is b and not b.flags.writeable and not k.flags.writeable
    with pytest.raises(ValueError):
        V.bicubic_tables(0, 4)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_the_lut_is_what_preprocess_computes_for_every_channel_and_byte(dtype):
    lut = V.normalise_lut(dtype)
    assert lut.dtype == np.uint16 and lut.shape == (3, 256)
    frames = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 1, 1, 3)))      # frame v: one pixel of value v
    want = V.preprocess(frames, 1)                                         # [256, 3, 1, 1] half; no resize
    if dtype == "bf16":
        want = want.to(torch.bfloat16)                                     # VisionEncoder.encode's cast of a half tensor
    want = want.view(torch.int16).numpy().view(np.uint16)[:, :, 0, 0].T
    assert np.array_equal(lut, want)
    assert len(np.unique(lut[0])) > 200                                    # (a table, not a constant)
    with pytest.raises(ValueError):
        V.normalise_lut("f8")


def test_preprocess_device_refuses_bad_frames_before_it_touches_the_device():
    good = np.zeros((2, 4, 5, 3), np.uint8)
    bad = {"dtype": good.astype(np.float32), "rank": good[0], "channels": np.zeros((2, 4, 5, 4), np.uint8), "contiguous": good[:, :, ::2],
           "torch dtype": torch.zeros((2, 4, 5, 3)), "torch contiguous": torch.zeros((2, 4, 5, 3), dtype=torch.uint8)[:, ::2], "a list": [[1, 2, 3]],
           "too large": np.zeros((1, 1, 8193, 3), np.uint8), "empty": np.zeros((0, 4, 5, 3), np.uint8)}
    for name, f in bad.items():
        with pytest.raises(ValueError, match="preprocess_device"):
            V.preprocess_device(f, 32)
    with pytest.raises(ValueError, match="f16 or bf16"):
        V.preprocess_device(good, 32, "f8")
    with pytest.raises(ValueError, match="image size"):
        V.preprocess_device(good, 0)


# ---- the serve loop: add_video by frames (a stub featuriser)
class _Stub:
    """Frames -> a feature tensor of the fake scorer's shape whose content is the frames' first byte; counts its calls."""
    num_frames = 16

    def __init__(self, fail=None):
        self.seen, self.fail = [], fail

    def __call__(self, frames):
        self.seen.append(tuple(frames.shape))
        assert frames.dtype == np.uint8 and frames.flags["C_CONTIGUOUS"]
        if self.fail:
            raise ValueError(self.fail)
        return torch.full((1, NV, 8), float(frames[0, 0, 0, 0]))


def _server(tmp_path, stub, content_hash=None):
    srv, passes, feats = GR._server(tmp_path, content_hash=content_hash)
    srv.featuriser = stub

    def stack(name, value=0, shape=(16, 6, 5, 3), dtype=np.uint8):
        path = tmp_path / name
        np.save(str(path), np.full(shape, value, dtype=dtype))
        return str(path)
    return srv, passes, feats, stack


def test_server_takes_the_featuriser_as_a_constructor_argument():
    import inspect
    p = inspect.signature(SR.Server.__init__).parameters["featuriser"]
    assert p.default is None


@pytest.mark.parametrize("B", [1, 5])
def test_an_add_by_frames_is_a_barrier_and_replies_stay_in_arrival_order(tmp_path, B):
    stub = _Stub()
    srv, passes, feats, stack = _server(tmp_path, stub)
    lines = [json.dumps({"id": 0, "caption": 1}),
             json.dumps({"id": 1, "caption": 2, "candidates": ["v0", "new"]}),                     # in front of the add: the id is not known yet
             json.dumps({"id": 2, "add_video": {"vid": "new", "frames": stack("a.npy", 1, shape=(40, 6, 5, 3))}}),
             json.dumps({"id": 3, "caption": 2, "candidates": ["v0", "new"]}),
             json.dumps({"id": 4, "caption": 0})]
    out, summary = GR._serve(srv, lines, B)
    assert [x["id"] for x in out] == [0, 1, 2, 3, 4]
    assert "unknown video id" in out[1]["error"]
    assert out[2] == {"id": 2, "added": "new", "index": 4, "videos": 5}
    assert sorted(out[0]["videos"]) == ["v0", "v1", "v2", "v3"] and sorted(out[3]["videos"]) == ["new", "v0"]
    assert sorted(out[4]["videos"]) == ["new", "v0", "v1", "v2", "v3"]
    assert len(passes) == (3 if B == 1 else 2)
    assert summary == {"requests": 5, "batches": 5 if B == 1 else 1, "mean_batch": 1.0 if B == 1 else 5.0, "errors": 1, "texts_added": 0, "videos_added": 1}
    assert stub.seen == [(16, 6, 5, 3)]                                                             # 40 frames sampled to 16, one tower call
    assert len(srv.s.video) == 5 and torch.equal(srv.s.video[4], torch.full((1, NV, 8), 1.0)) and srv.n_vid.tolist() == [NV] * 5


def test_a_bad_frames_request_gets_its_error_line_and_adds_nothing(tmp_path):
    stub = _Stub()
    srv, passes, feats, stack = _server(tmp_path, stub, content_hash=lambda t: t.numpy().tobytes())
    good, feature_file = stack("good.npy", 2), feats("good.pth", 2.0)
    garbage = tmp_path / "garbage.npy"
    garbage.write_bytes(b"not an array file")
    pickled = tmp_path / "pickled.npy"
    np.save(str(pickled), np.array([{"a": 1}], dtype=object), allow_pickle=True)
    existing = "add_video takes vid (the new video's id) and features (the path of its feature file)"
    bad = [
        ({"vid": "x", "frames": good, "features": feature_file}, existing),                        # both forms
        ({"vid": "x"}, existing),                                                                  # neither
        ({"vid": "x", "frames": good, "fps": 30}, existing),
        ({"vid": "x", "frames": stack("float.npy", dtype=np.float32)}, "uint8"),
        ({"vid": "x", "frames": stack("rank.npy", shape=(6, 5, 3))}, "rank 4"),
        ({"vid": "x", "frames": stack("channels.npy", shape=(16, 6, 5, 4))}, "3 channels"),
        ({"vid": "x", "frames": stack("none.npy", shape=(0, 6, 5, 3))}, "no frame"),
        ({"vid": "x", "frames": str(tmp_path / "missing.npy")}, "cannot read"),
        ({"vid": "x", "frames": str(garbage)}, "cannot read"),
        ({"vid": "x", "frames": str(pickled)}, "cannot read"),
        ({"vid": "x", "frames": 7}, "path"),
        ({"vid": "v1", "frames": good}, "already in the gallery"),
    ]
    lines = [json.dumps({"id": n, "add_video": a}) for n, (a, _) in enumerate(bad)]
    lines.append(json.dumps({"id": "q", "add_video": {"vid": "x", "frames": good}, "caption": 0}))
    out, summary = GR._serve(srv, lines, 4)
    for x, (a, msg) in zip(out, bad):
        assert set(x) == {"id", "error"} and msg in x["error"], (a, x)
    assert out[0]["error"] == out[1]["error"] == out[2]["error"] == existing                       # today's line, unchanged
    assert "carries no query" in out[-1]["error"]
    assert stub.seen == [] and passes == [] and len(srv.s.video) == 4 and len(srv.vids) == 4 and "videos_added" not in summary
    assert summary["errors"] == summary["requests"] == len(lines)
    # a tower that cannot be loaded, a server without one: error lines, and the process goes on
    srv.featuriser = _Stub(fail="the vision tower cannot be loaded (KeyError: 'vit.patch.w')")
    out, _ = GR._serve(srv, [json.dumps({"id": 0, "add_video": {"vid": "x", "frames": good}})], 1)
    assert "vision tower cannot be loaded" in out[0]["error"] and len(srv.s.video) == 4
    srv.featuriser = None
    out, _ = GR._serve(srv, [json.dumps({"id": 0, "add_video": {"vid": "x", "frames": good}})], 1)
    assert "no vision tower" in out[0]["error"] and len(srv.s.video) == 4
    # the good stack joins; the same content as a feature file, or as frames again, is a duplicate; a short stack is sampled up to 16
    srv.featuriser = stub
    out, summary = GR._serve(srv, [json.dumps({"id": 0, "add_video": {"vid": "x", "frames": good}}),
                                   json.dumps({"id": 1, "add_video": {"vid": "y", "features": feature_file}}),
                                   json.dumps({"id": 2, "add_video": {"vid": "z", "frames": stack("again.npy", 2)}}),
                                   json.dumps({"id": 3, "add_video": {"vid": 7, "frames": stack("short.npy", 3, shape=(3, 4, 4, 3))}}),
                                   json.dumps({"id": 4, "caption": 0, "candidates": [7, "x"]})], 4)
    assert out[0] == {"id": 0, "added": "x", "index": 4, "videos": 5}
    assert "those of video 'x'" in out[1]["error"] and "those of video 'x'" in out[2]["error"]
    assert out[3] == {"id": 3, "added": "7", "index": 5, "videos": 6} and sorted(out[4]["videos"]) == ["7", "x"]
    assert stub.seen == [(16, 6, 5, 3), (16, 6, 5, 3), (16, 4, 4, 3)] and summary["videos_added"] == 2


def test_frame_stacks_are_sampled_by_the_extractors_rule(tmp_path):
    from blim_amd import extract as X
    a = np.arange(40, dtype=np.uint8)[:, None, None, None] * np.ones((1, 2, 2, 3), np.uint8)
    path = str(tmp_path / "s.npy")
    np.save(path, a)
    got = SR.load_frame_stack(path, 16)
    assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, X.read_frames(path, False, "MSRVTT", 16)) and got.shape == (16, 2, 2, 3)
    assert got[:, 0, 0, 0].tolist() == np.linspace(0, 39, 16, dtype=int).tolist()
    np.save(path, a[:1])
    assert SR.load_frame_stack(path, 16)[:, 0, 0, 0].tolist() == [0] * 16
    np.save(path, a[:16])
    assert np.array_equal(SR.load_frame_stack(path, 16), a[:16])


def test_query_video_files_are_frame_stacks_when_they_end_in_npy(tmp_path):
    stub = _Stub()
    feat = tmp_path / "a.pth"
    torch.save(torch.full((1, NV, 8), 5.0), str(feat))
    stack = tmp_path / "b.npy"
    np.save(str(stack), np.full((20, 3, 3, 3), 9, np.uint8))
    args = SR.get_args_parser().parse_args(["--direction", "v2t", "--candidates", "all", "--query_video", str(feat), str(stack)])
    got = SR.query_video_features(args.query_video, args, featuriser=stub)
    assert torch.equal(got[0], torch.full((1, NV, 8), 5.0)) and torch.equal(got[1], torch.full((1, NV, 8), 9.0)) and stub.seen == [(16, 3, 3, 3)]
    assert SR.is_frame_stack("x.npy") and not SR.is_frame_stack("x.pth") and not SR.is_frame_stack("x.npy.pth") and not SR.is_frame_stack(None)
    np.save(str(stack), np.zeros((20, 3, 3), np.uint8))
    with pytest.raises(ValueError, match="rank 4"):
        SR.query_video_features([str(stack)], args, featuriser=stub)


# ---- the commands' flags
def test_check_args_accepts_the_tower_flags_only_where_frames_can_arrive():
    p = SR.get_args_parser()
    a = p.parse_args(["--serve"])
    assert a.vision_model_path is None and a.vision_synthetic is None
    SR.check_args(a)
    SR.check_args(p.parse_args(["--serve", "--vision_synthetic", "3"]))
    SR.check_args(p.parse_args(["--serve", "--vision_model_path", "./tower"]))
    SR.check_args(p.parse_args(["--direction", "v2t", "--candidates", "all", "--query_video", "a.npy", "--vision_synthetic", "3"]))
    SR.check_args(p.parse_args(["--direction", "v2t", "--candidates", "all", "--query_video", "a.pth", "b.npy", "--vision_model_path", "./tower"]))
    SR.check_args(p.parse_args(["--direction", "v2t", "--candidates", "all", "--query_video", "a.npy"]))         # the tower comes from --model_path
    for argv in (["--query_ids", "0", "--vision_synthetic", "3"],
                 ["--query_ids", "0", "--vision_model_path", "./tower"],
                 ["--direction", "v2t", "--video_ids", "0", "--vision_synthetic", "3"],
                 ["--direction", "v2t", "--candidates", "all", "--query_video", "a.pth", "--vision_synthetic", "3"]):
        with pytest.raises(SystemExit, match="raw frames"):
            SR.check_args(p.parse_args(argv))
    with pytest.raises(SystemExit, match="not both"):
        SR.check_args(p.parse_args(["--serve", "--vision_synthetic", "3", "--vision_model_path", "./tower"]))
    # the refusals there were keep their words, whatever the new flags say
    for argv, msg in ((["--dtype", "f8", "--serve"], "--dtype f8 is not supported"), (["--shard", "2", "0", "--serve"], "--shard is not supported"),
                      (["--serve", "--direction", "v2t", "--query_video", "a.npy", "--candidates", "all"], "v2t is not served"),
                      (["--direction", "v2t", "--query_video", "a.npy"], "no first-stage row"),
                      (["--query_ids", "0", "--query_video", "a.npy"], "--direction v2t")):
        with pytest.raises(SystemExit, match=msg):
            SR.check_args(p.parse_args(argv + ["--vision_synthetic", "3"]))
    with pytest.raises(SystemExit, match="world size 2"):
        SR.check_args(p.parse_args(["--serve", "--vision_synthetic", "3"]), world=2)


def test_extract_takes_preprocess_host_by_default():
    from blim_amd import extract as X
    base = ["--dataset", "MSRVTT", "--num_chunk", "1", "--chunk_idx", "0"]
    assert X.get_args_parser().parse_args(base).preprocess == "host"
    assert X.get_args_parser().parse_args(base + ["--preprocess", "device"]).preprocess == "device"
    with pytest.raises(SystemExit):
        X.get_args_parser().parse_args(base + ["--preprocess", "pil"])


def test_preprocess_abi_is_declared_and_exported():
    names = ("blim_preprocess_workspace_bytes", "blim_preprocess_frames")
    assert set(names) <= set(eng.declared_symbols())
    header = open(eng.HEADER_PATH).read()
    assert "#define BLIM_ABI_VERSION 9" in header and "1 << 21" in header and ">> 22" in header
    lib = eng.load_library()
    assert all(hasattr(lib, s) for s in names) and lib.blim_abi_version() == 9
