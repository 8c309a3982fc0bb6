"""Where a wave's time goes inside one K-step of the compensated GEMM's SECOND pass (gemm.hip phase 2; instrumented library: `make -C blim_amd/csrc waitprof`).

Every wave, per step: [quadrants A + B: 16 MFMAs, 6 refills from the step's own tile, 3 LDS-DMA] [vmcnt: my LDS-DMA pieces of the next tile] [barrier] [quadrant C: 8 MFMAs,
2 refills + scales from the next tile, 2 LDS-DMA] [quadrant D: 8 MFMAs, 4 refills, 2 LDS-DMA].  Numbers are shader-clock cycles (s_memtime) summed over the pass's K loop of each tile,
averaged over tiles.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from blim_amd import engine as eng
lib = eng.load_library(os.path.join(ROOT, "tools", "bin", "libblim_hip_waitprof.so"))
names = ("qa+qb", "vmcnt", "barrier", "qc", "qd")
for (M, N, K) in ((32768, 37888, 3584), (32768, 3584, 18944)):
    a = torch.empty((M, 2 * K), dtype=torch.float16, device="cuda"); w = torch.empty((N, K), dtype=torch.float16, device="cuda")
    a.normal_(); a[:, K:] *= 2.0 ** -11; w.normal_(std=0.02)
    nwg = (M // 256) * (N // 256)
    st = torch.zeros((nwg * 3, 8), dtype=torch.int64, device="cuda")
    eng.gemm_f16_lo6(a, w); torch.cuda.synchronize()
    lib.blim_debug_gemm_stamps(st.data_ptr())
    eng.gemm_f16_lo6(a, w); torch.cuda.synchronize()
    lib.blim_debug_gemm_stamps(None)
    s = st.cpu().numpy().astype(np.float64)
    loop_us = (s[:nwg, 2] - s[:nwg, 1]).mean() * 0.01
    wt = s[nwg:].reshape(nwg, 2, 8)[:, :, :5]
    print(f"{M}x{N}x{K}: both passes {loop_us:.1f} us per tile ({K // 64} 16-bit + {K // 128} e2m3 K-steps)")
    for g in range(2):
        tot = wt[:, g].sum(axis=1).mean()
        parts = wt[:, g].mean(axis=0)
        print(f"   waves {4 * g}-{4 * g + 3}: {tot / (K // 128):.0f} cycles per e2m3 K-step | " + "  ".join(f"{n} {v / (K // 128):.0f}" for n, v in zip(names, parts)), flush=True)
    del a, w
