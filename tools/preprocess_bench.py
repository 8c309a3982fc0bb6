"""Frame preprocessing on the host and on the device: the extraction rate of `python -m blim_amd.extract --preprocess host | device` over
pre-decoded frame stacks, the kernels' time per video (HIP events around blim_preprocess_frames), and the latency of featurising one clip as `--serve` does for
an add_video request that brings frames.

    python tools/preprocess_bench.py [--videos 64] [--reps 5] [--sizes 360x640 720x1280] [--batch_size 8] [--num_workers 4] [--out FILE.json]

The extraction legs run the command itself, one process per run, host and device alternated; the rate is the one the command prints (decoding and preprocessing
included, the tower's start-up not).  The frame stacks are written to a temporary directory: 8 distinct random stacks, linked to --videos names."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": list(xs)}


def extraction(args, H, W):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        frames = os.path.join(tmp, "frames")
        os.makedirs(frames)
        rng = np.random.default_rng(H)
        for i in range(min(8, args.videos)):
            np.save(os.path.join(tmp, f"src{i}.npy"), rng.integers(0, 256, (16, H, W, 3), dtype=np.uint8))
        for i in range(args.videos):
            os.symlink(os.path.join(tmp, f"src{i % 8}.npy"), os.path.join(frames, f"video{i:03d}.npy"))
        cmd = [sys.executable, "-m", "blim_amd.extract", "--dataset", "MSRVTT", "--num_chunk", "1", "--chunk_idx", "0", "--synthetic", "21", "--clear",
               "--frames_dir", frames, "--batch_size", str(args.batch_size), "--num_workers", str(args.num_workers)]
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        rates = {"host": [], "device": []}
        for rep in range(args.reps):
            for mode in ("host", "device"):
                r = subprocess.run(cmd + ["--preprocess", mode], cwd=tmp, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"extract --preprocess {mode} failed ({r.returncode}): {r.stderr[-2000:]}")
                m = re.search(r"(\d+) videos in ([0-9.]+)s \(([0-9.]+) videos/s", r.stdout)
                assert m and int(m.group(1)) == args.videos, r.stdout[-500:]
                rates[mode].append(float(m.group(3)))
                print(f"# extract {H}x{W} rep {rep} {mode}: {m.group(3)} videos/s", file=sys.stderr, flush=True)
        out = {mode: spread(v) for mode, v in rates.items()}
    return out


def kernels(H, W, S=448, T=16, iters=30):
    import torch

    from blim_amd import engine as eng
    from blim_amd import vision as V
    rng = np.random.default_rng(W)
    f = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    for _ in range(2):
        V.preprocess(f, S)
    host_ms = (time.perf_counter() - t0) / 2 * 1e3
    V.preprocess_device(f, S); torch.cuda.synchronize()
    wall = []
    for _ in range(10):
        t0 = time.perf_counter()
        V.preprocess_device(f, S); torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    lib = V._pre_lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = V._pre_state[str(dev)]
    x = torch.from_numpy(f).to(dev)
    (xb, xk, xks), (yb, yk, yks) = V._device_tables(st, dev, W, S), V._device_tables(st, dev, H, S)
    out = torch.empty((T, 3, S, S), dtype=torch.float16, device=dev)
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng._check(lib.blim_preprocess_frames(eng._ptr(x), T, H, W, S, eng._ptr(xb), eng._ptr(xk), xks, eng._ptr(yb), eng._ptr(yk), yks, eng._ptr(st[("lut", "f16")]),
                                              eng._ptr(out), eng._ptr(st["workspace"]), eng._stream()), "blim_preprocess_frames")
        b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    moved = f.nbytes + 2 * T * H * S * 3 + out.numel() * 2                     # frames read, workspace written and read, output written
    k = statistics.median(ms)
    return {"host_preprocess_ms_one_thread": host_ms, "device_call_ms_upload_included": spread(wall), "kernels_ms": spread(ms), "upload_bytes": int(f.nbytes),
            "half_tensor_bytes": int(out.numel() * 2), "bytes_moved": int(moved), "gb_per_s": moved / k / 1e6}


def serve_latency(H, W, n_frames=40, iters=10):
    import torch

    from blim_amd import search as SR
    args = SR.get_args_parser().parse_args(["--serve", "--vision_synthetic", "21"])
    fz = SR.FrameFeaturiser(args)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clip.npy")
        np.save(path, np.random.default_rng(1).integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8))
        fz(SR.load_frame_stack(path, fz.num_frames)); torch.cuda.synchronize()     # the tower is made here
        load, feat = [], []
        for _ in range(iters):
            t0 = time.perf_counter()
            a = SR.load_frame_stack(path, fz.num_frames)
            t1 = time.perf_counter()
            fz(a)                                                               # ends with the copy of the features to the host
            t2 = time.perf_counter()
            load.append((t1 - t0) * 1e3); feat.append((t2 - t1) * 1e3)
    fz.close()
    return {"frames_in_file": n_frames, "load_and_sample_ms": spread(load), "preprocess_tower_download_ms": spread(feat)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--videos", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--sizes", nargs="+", default=["360x640", "720x1280"])
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--skip_extract", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    sizes = [tuple(int(n) for n in s.split("x")) for s in args.sizes]
    res = {"args": vars(args), "extract_videos_per_s": {}, "kernels": {}, "serve": {}}
    if not args.skip_extract:                                                  # first: this process has not opened the GPU yet
        for H, W in sizes:
            res["extract_videos_per_s"][f"{H}x{W}"] = extraction(args, H, W)
    for H, W in sizes:
        res["kernels"][f"{H}x{W}"] = kernels(H, W)
    res["serve"][f"{sizes[0][0]}x{sizes[0][1]}"] = serve_latency(*sizes[0])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
