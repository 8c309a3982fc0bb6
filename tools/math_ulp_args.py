"""Writes the argument files of tools/math_ulp_probe.hip: every argument that the row kernels' sqrtf, 1.0f / x, a / b, expf and logf meet on the inputs of
tests/score_kernel_inputs.py, formed in f32 as the kernels form them (the sums in float64, rounded once: the probe measures the FUNCTIONS, not the sums).
    python tools/math_ulp_args.py DIR          -> DIR/{sqrt,rcp,div,div_b,exp,log}.bin (float32)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import score_kernel_inputs as I  # noqa: E402

f32 = np.float32
args = {k: [] for k in ("sqrt", "rcp", "div", "div_b", "exp", "log")}


def add(name, v):
    v = np.asarray(v, f32).reshape(-1)
    args[name].append(v[np.isfinite(v)])


def div(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1))
    ok = np.isfinite(a) & (b != 0)
    args["div"].append(a[ok])
    args["div_b"].append(b[ok])


def rms_rows(x, H, w):
    x = np.asarray(x, np.float64)[:, :H]
    x = x[np.isfinite(x).all(1)]
    ss = (x * x).sum(1).astype(f32)
    div(ss, f32(H))
    var = (ss / f32(H) + f32(I.RMS_EPS)).astype(f32)
    add("sqrt", var)
    root = np.sqrt(var).astype(f32)
    add("rcp", root)
    return np.abs(np.asarray(w, np.float64) * (x / root.astype(np.float64)[:, None])).max(1).astype(f32)


def softmax_rows(lg):
    lg = np.asarray(lg, f32)
    a = (lg - lg.max(1, keepdims=True)).astype(f32)
    add("exp", a)
    add("log", np.exp(a.astype(np.float64)).sum(1))


for cc in [I.rms(c) for c in I.RMS] + [I.rms6(c) for c in I.RMS6]:
    rms_rows(cc.x, cc.H, cc.w)
for c in I.RMS_F8:
    cc = I.rms_f8(c)
    amax = rms_rows(cc.x, cc.H, cc.w)
    amax = amax[amax > 0]
    div(amax, f32(448.0))
    add("rcp", amax / f32(448.0))
for c in I.LSE:
    cc = I.lse(c)
    with np.errstate(invalid="ignore"):
        a = (cc.m - cc.m.max(1, keepdims=True)).astype(f32)
    add("exp", a)
    live = np.isfinite(a)
    add("log", (np.where(live, cc.s.astype(np.float64) * np.exp(np.where(live, a, 0.0).astype(np.float64)), 0.0)).sum(1))
for c in I.CE:
    cc = I.ce(c)
    softmax_rows(cc.buf[:, :cc.V])
for c in I.TVG:
    cc = I.tvg(c)
    softmax_rows(cc.buf[:, :cc.nv])
    div(np.asarray(cc.ref, np.float64) * cc.clips, f32(cc.clips))
for c in I.SEG:
    cc = I.seg(c)
    for p in range(cc.n_pairs):
        sg = cc.lp[cc.row_start[p]:cc.row_start[p + 1]]
        den = np.count_nonzero(sg) if cc.mode == 0 else len(sg)
        if den:
            div(sg.astype(np.float64).sum(), f32(den))
for c in I.GM:
    div(f32(1.0), f32(c[0]))

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
for k, v in args.items():
    np.concatenate(v).astype(f32).tofile(os.path.join(out, k + ".bin"))
    print(k, sum(len(a) for a in v))
