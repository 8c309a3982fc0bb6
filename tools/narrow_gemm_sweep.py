"""blim_gemm alone, the residual epilogue in fp16: time per launch of the 256 x 256 kernel (tile = 0) and of the narrow-tile kernel (tile = 2, csrc/gemm.hip:
gemm_narrow_kernel) at M in {32 .. 4096} x (N, K) in {(3584, 3584), (3584, 18944)} -- o_proj and down of the 7B decoder.  HIP events around `--inner` back-to-back
launches, the two tiles alternated `--reps` times in one process, medians and spreads; the results of the two tiles are compared bit for bit at every shape.  The auto
rule's constant (gemm.hpp: GEMM_NARROW_TILES) is read off this table: the largest count of 256 x 256 tiles below which the narrow kernel is never the slower one.

    python tools/narrow_gemm_sweep.py --out profiles/r16_narrow_gemm_sweep.json

--lo6: the compensated form instead -- A = [hi | lo] rows (lda = 2 K), the e2m3 second pass over K6 = K on images built once per shape (f6_build), the 256 x 256
kernel (tile_lo6 = 0) against gemm_narrow_lo6_kernel (tile_lo6 = 2); that table sets GEMM_NARROW_LO6_TILES.

    python tools/narrow_gemm_sweep.py --lo6 --ms 256,512,1024,2048,4096 --out profiles/r18_narrow_lo6_sweep.json

--qkv: the QKV epilogue instead (bias, RoPE, 16-bit outputs) at N = 4608 (28 + 4 + 4 heads, rope_cols = 4096), K = 3584 -- the 7B decoder's QKV projection -- in the
three forms run_layers launches: plain; hi | lo outputs over the w_wrap_k walk (A = [hi | lo], K = 2 x 3584); hi | lo outputs behind the e2m3 second pass.  The
256 x 256 kernel (tile_qkv = 0) against gemm_nqkv_kernel (tile_qkv = 2); the minimum over the three forms sets GEMM_NARROW_QKV_TILES.

    python tools/narrow_gemm_sweep.py --qkv --ms 256,512,768,1024,1536,2048,4096 --out profiles/r19_narrow_qkv_sweep.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blim_amd import engine as eng  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="32,64,128,256,512,1024,2048,4096")
    ap.add_argument("--shapes", default="3584x3584,3584x18944", help="N x K")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lo6", action="store_true", help="the compensated form: the e2m3 second pass, tile_lo6 instead of tile")
    ap.add_argument("--qkv", action="store_true", help="the QKV epilogue at N = 4608, K = 3584 in its plain, wrap and e2m3 forms: tile_qkv")
    a = ap.parse_args()
    if a.qkv:
        return main_qkv(a)
    field = "tile_lo6" if a.lo6 else "tile"
    launches = eng.gemm_narrow_lo6_launches if a.lo6 else eng.gemm_narrow_launches
    lib = eng.load_library()
    tdt = torch.float16 if a.dtype == "f16" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for shape in a.shapes.split(","):
        N, K = (int(x) for x in shape.split("x"))
        w = (torch.randn((N, K), device="cuda", generator=g) * 0.02).to(tdt)
        for M in (int(x) for x in a.ms.split(",")):
            x = torch.randn((M, K), device="cuda", generator=g).to(tdt)
            base = torch.randn((M, N), device="cuda", generator=g)
            kw = {}
            if a.lo6:                                                                 # [hi | lo] rows with true lo parts (2^-11 of the values in fp16); the images are built below
                x32 = torch.randn((M, K), device="cuda", generator=g)
                hi = x32.to(tdt)
                x = torch.cat([hi, (x32 - hi.float()).to(tdt)], dim=1).contiguous()
                kw = dict(lda=2 * K, K6=K, A6=torch.empty(lib.blim_f6_tiles_bytes(M, K), dtype=torch.uint8, device="cuda"),
                          W6=torch.empty(lib.blim_f6_tiles_bytes(N, K), dtype=torch.uint8, device="cuda"))
                eng.gemm("resid", a.dtype, x, w, M, N, K, base.clone(), f6_build=1, **{**kw, "K6": 0})
            out = {}
            for tile in (0, 2):                                                       # the same bits, and a warm-up of both kernels
                c = base.clone()
                n0 = launches()
                eng.gemm("resid", a.dtype, x, w, M, N, K, c, **{field: tile}, **kw)
                torch.cuda.synchronize()
                assert launches() - n0 == (1 if tile == 2 else 0)
                out[tile] = c
            assert torch.equal(out[0].view(torch.int32), out[2].view(torch.int32)), (M, N, K, "the two tiles' results differ")
            c = base.clone()
            ts = {0: [], 2: []}
            for _ in range(a.reps):
                for tile in (0, 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.inner):
                        eng.gemm("resid", a.dtype, x, w, M, N, K, c, **{field: tile}, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    ts[tile].append(e0.elapsed_time(e1) * 1e3 / a.inner)
            med = {t: float(np.median(v)) for t, v in ts.items()}
            r = {"M": M, "N": N, "K": K, "tiles_256": -(-M // 256) * -(-N // 256), "tiles_narrow": -(-M // 64) * -(-N // 64), "wide_us": med[0], "narrow_us": med[2],
                 "wide_spread": float((max(ts[0]) - min(ts[0])) / med[0]), "narrow_spread": float((max(ts[2]) - min(ts[2])) / med[2]), "narrow_over_wide": med[2] / med[0],
                 "wide_tflops": 2.0 * M * N * K / med[0] * 1e-6, "narrow_tflops": 2.0 * M * N * K / med[2] * 1e-6}
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = {"dtype": a.dtype, "reps": a.reps, "inner": a.inner, "threshold_tiles_in_library": eng.gemm_narrow_threshold(), "rows": rows}
    if a.lo6:
        res.update(form="lo6", threshold_tiles_in_library=eng.gemm_narrow_lo6_threshold())
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


def main_qkv(a):
    lib = eng.load_library()
    tdt = torch.float16 if a.dtype == "f16" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(1)
    N, K, rope_cols = 4608, 3584, 4096
    w = (torch.randn((N, K), device="cuda", generator=g) * 0.02).to(tdt)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    rows = []
    for M in (int(x) for x in a.ms.split(",")):
        stride = (M + 255) // 256 * 256
        table = eng.rope_rows(torch.arange(M, dtype=torch.int32, device="cuda"), 1.0e6, 32768, stride)
        x32 = torch.randn((M, K), device="cuda", generator=g)
        hi = x32.to(tdt)
        x2 = torch.cat([hi, (x32 - hi.float()).to(tdt)], dim=1).contiguous()              # [hi | lo] rows with true lo parts
        common = dict(bias=bias, rope_cols=rope_cols, rope_rows=table, rope_stride=stride)
        a6 = torch.empty(lib.blim_f6_tiles_bytes(M, K), dtype=torch.uint8, device="cuda")
        w6 = torch.empty(lib.blim_f6_tiles_bytes(N, K), dtype=torch.uint8, device="cuda")
        forms = {"plain": (K, dict(lda=2 * K), False),
                 "split_wrap": (2 * K, dict(lda=2 * K, w_wrap_k=K, lo_off=N), True),
                 "split_e2m3": (K, dict(lda=2 * K, lo_off=N, A6=a6, W6=w6, K6=K), True)}
        eng.gemm("qkv", a.dtype, x2, w, M, N, K, torch.empty((M, 2 * N), dtype=tdt, device="cuda"), lda=2 * K, lo_off=N, A6=a6, W6=w6, f6_build=1, **common)   # the images, once
        for form, (Kc, kw, split) in forms.items():
            new = lambda: torch.zeros((M, 2 * N if split else N), dtype=tdt, device="cuda")
            out = {}
            for tile in (0, 2):                                                           # the same bits, and a warm-up of both kernels
                c = new()
                n0 = eng.gemm_narrow_qkv_launches()
                eng.gemm("qkv", a.dtype, x2, w, M, N, Kc, c, tile_qkv=tile, **kw, **common)
                torch.cuda.synchronize()
                assert eng.gemm_narrow_qkv_launches() - n0 == (1 if tile == 2 else 0)
                out[tile] = c
            assert torch.equal(out[0].view(torch.int16), out[2].view(torch.int16)), (M, form, "the two kernels' results differ")
            c = new()
            ts = {0: [], 2: []}
            for _ in range(a.reps):
                for tile in (0, 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.inner):
                        eng.gemm("qkv", a.dtype, x2, w, M, N, Kc, c, tile_qkv=tile, **kw, **common)
                    e1.record()
                    torch.cuda.synchronize()
                    ts[tile].append(e0.elapsed_time(e1) * 1e3 / a.inner)
            med = {t: float(np.median(v)) for t, v in ts.items()}
            r = {"form": form, "M": M, "N": N, "K": K, "tiles_256": -(-M // 256) * -(-N // 256), "tiles_narrow": -(-M // 64) * -(-N // 64), "wide_us": med[0], "narrow_us": med[2],
                 "wide_spread": float((max(ts[0]) - min(ts[0])) / med[0]), "narrow_spread": float((max(ts[2]) - min(ts[2])) / med[2]), "narrow_over_wide": med[2] / med[0]}
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = {"form": "qkv", "dtype": a.dtype, "reps": a.reps, "inner": a.inner, "threshold_tiles_in_library": eng.gemm_narrow_qkv_threshold(), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
