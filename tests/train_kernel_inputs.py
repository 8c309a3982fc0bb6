"""TEST INFRASTRUCTURE: the inputs of tests/test_train_kernels_gpu.py, made on the host as exact 16-bit / f32 values, with their float64 references
(oracle/train_kernels_ref.py) computed once per case.  tests/test_train_kernels_ref.py runs its emulation and its wrong rules over exactly these cases.

The shapes are the smallest at which each kernel takes another path (the case lists say which); every list covers every value the kernels' code distinguishes,
not the full cross product."""
import functools
import types
import zlib

import numpy as np

from oracle import train_kernels_ref as K
from oracle.attention_ref import round16

DTYPES = ("f16", "bf16")
SEED, SCALE, DROP = 0x5EED1234ABCD, 2.0, 0.1
f32 = np.float32


def rs_of(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def v16(rs, shape, dtype, scale=1.0):
    return round16(rs.standard_normal(shape) * scale, dtype)


def v32(rs, shape, scale=1.0):
    return (rs.standard_normal(shape) * scale).astype(f32)


def up(x, m):
    return -(-x // m) * m


# ---- lora_down: 32 tokens per workgroup, the four waves split K / 16 steps as ceil(steps / 4) each.  K = 16: one step, three idle waves; 48: wave 3 idle;
# 80: 2 / 2 / 1 / 0; 1024: the ordinary case.  (T, K, r, adapters, p)
LORA_DOWN = [(1, 16, 1, 1, 0.0), (31, 48, 4, 2, DROP), (33, 80, 8, 3, DROP), (70, 1024, 16, 3, 0.0), (70, 1024, 4, 1, DROP), (33, 16, 16, 3, DROP), (70, 80, 1, 2, 0.0),
             (31, 1024, 8, 2, DROP), (70, 48, 8, 3, DROP)]


@functools.lru_cache(maxsize=None)
def lora_down(case, dtype):
    T, Kc, r, n, p = case
    rs = rs_of("down", case, dtype)
    c = types.SimpleNamespace(T=T, K=Kc, r=r, n=n, p=p, ldx=Kc + 64, site=40, dtype=dtype)
    c.x = v16(rs, (T, Kc), dtype)
    c.A = [v32(rs, (r, Kc), Kc ** -0.5) for _ in range(n)]
    c.ref, c.tol = K.lora_down(c.x, c.A, r, SCALE, p, SEED, c.site, dtype)
    return c


# ---- lora_wgrad (dB, dA): 128 columns x 1,024-row time splits, 64 rows per stage.  (T, columns, r[, p, family])
LORA_DB = [(1, 8, 4), (63, 136, 16), (65, 264, 4), (1024, 100, 16), (1025, 136, 4), (2049, 264, 16), (2049, 100, 4), (65, 8, 16)]
LORA_DA = [(1, 8, 4, 0.0, "gauss"), (63, 136, 16, DROP, "gauss"), (65, 264, 4, DROP, "gauss"), (1024, 136, 16, 0.0, "gauss"), (1025, 8, 4, DROP, "gauss"),
           (2049, 264, 16, 0.0, "gauss"), (65, 136, 16, 0.0, "span"), (1025, 264, 4, DROP, "span"), (65, 136, 16, 0.0, "tiny"), (65, 136, 16, DROP, "huge")]


@functools.lru_cache(maxsize=None)
def lora_dB(case, dtype):
    T, N, r = case
    rs = rs_of("dB", case, dtype)
    c = types.SimpleNamespace(T=T, N=N, r=r, ldy=104 if N == 100 else N + 8, ldu=r + 16, u_off=8, dtype=dtype)
    c.dy, c.u, c.dB0 = v16(rs, (T, N), dtype), v16(rs, (T, r), dtype), v32(rs, (N, r))
    c.ref, c.tol = K.lora_dB(c.dy, c.u, c.dB0)
    return c


@functools.lru_cache(maxsize=None)
def lora_dA(case, dtype):
    T, Kc, r, p, family = case
    rs = rs_of("dA", case, dtype)
    c = types.SimpleNamespace(T=T, K=Kc, r=r, p=p, ldx=Kc + 8, site=43, family=family, dtype=dtype)
    c.x, c.dA0 = v16(rs, (T, Kc), dtype), v32(rs, (r, Kc))
    # span: rows from 1e-3 to 1e4 inside one tensor, the loss scale's range; tiny / huge: its two ends alone (fp16: at 1e-3 the hi AND the lo part are subnormal)
    mag = {"span": 10.0 ** rs.uniform(-3.0, 4.0, size=(T, 1)), "tiny": 1e-3, "huge": 1e4}.get(family, 1.0)
    c.du = (rs.standard_normal((T, r)) * mag).astype(f32)
    c.ref, c.tol = K.lora_dA(c.du, c.x, c.dA0, p, SEED, c.site, dtype)
    return c


# ---- lora_du: 32 rows per wave, 128 per workgroup; N = 16: one step; 64: exactly one unrolled group of four; 80: 4 + 1 tail; 272: two slices; 1040: five;
# 100: round_up(N, 16) = 112 with zero columns behind N.  (T, N, r)
LORA_DU = [(1, 16, 4), (31, 64, 16), (33, 80, 4), (127, 272, 16), (129, 1040, 4), (129, 80, 16), (33, 1040, 16), (65, 100, 16)]


@functools.lru_cache(maxsize=None)
def lora_du(case, dtype):
    T, N, r = case
    rs = rs_of("du", case, dtype)
    Np = up(N, 16)
    c = types.SimpleNamespace(T=T, N=N, r=r, Np=Np, ldy=Np + 8, dtype=dtype, slices=K.du_splits(T, Np))
    c.dy = np.zeros((T, Np))
    c.dy[:, :N] = v16(rs, (T, N), dtype)
    c.B = v32(rs, (N, r), N ** -0.5)
    c.ref, c.tol = K.lora_du(c.dy, c.B, SCALE, dtype)
    return c


# ---- lora_dx.  (T, K, adapters, r, p, out16)
LORA_DX = [(5, 4, 1, 4, 0.0, False), (37, 132, 3, 16, DROP, False), (37, 132, 1, 8, DROP, True), (9, 1024, 3, 4, DROP, True), (70, 1024, 1, 16, 0.0, False),
           (41, 4, 3, 4, DROP, True)]


@functools.lru_cache(maxsize=None)
def lora_dx(case, dtype):
    T, Kc, n, r, p, out16 = case
    rs = rs_of("dx", case, dtype)
    c = types.SimpleNamespace(T=T, K=Kc, n=n, r=r, p=p, out16=out16, ldd=Kc + 12, ldo=Kc + 4, site=16, dtype=dtype)
    c.dx0 = v32(rs, (T, Kc))
    c.du = [v32(rs, (T, r)) for _ in range(n)]
    c.A = [v32(rs, (r, Kc), 0.3) for _ in range(n)]
    c.ref, c.tol, c.tol16 = K.lora_dx(c.dx0, c.du, c.A, r, p, SEED, c.site, dtype)
    return c


# ---- rmsnorm_bwd.  Families: gauss; parallel: w dy = alpha x (1 + 1e-3 noise), the two terms of rs w dy - x c nearly cancel; norms: a row of norm 1e3 beside one
# of 1e-3.  plain (256 threads x 8 float4): (H, n_rows, flags, family), flags of "rows", "acc", "out16".  fused (4 rows per workgroup, clamped tail rows):
# (n_rows, H, adapters, r, p, flags, family)
RMS_PLAIN = [(4, 1, "", "gauss"), (1020, 5, "rows", "gauss"), (1024, 5, "acc", "parallel"), (1028, 5, "out16", "norms"), (3584, 1, "acc out16", "gauss"),
             (8192, 5, "rows acc", "parallel"), (8192, 1, "out16", "norms"), (1024, 5, "", "norms"), (1028, 1, "rows", "parallel")]
RMS_FUSED = [(1, 128, 1, 4, 0.0, "", "gauss"), (3, 1028, 3, 16, DROP, "acc out16", "parallel"), (4, 4096, 1, 4, DROP, "acc", "norms"), (5, 128, 3, 16, DROP, "out16", "gauss"),
             (7, 1028, 1, 16, 0.0, "acc", "norms"), (7, 4096, 3, 4, DROP, "acc out16", "gauss"), (5, 4096, 3, 16, 0.0, "", "parallel")]
RMS_EPS = 1e-6


def _rms_rows(rs, n, H, family):
    x, w = v32(rs, (n, H)), (1.0 + 0.2 * rs.standard_normal(H)).astype(f32)
    if family == "norms":
        x = (x * np.where(np.arange(n) % 2 == 0, 1e3, 1e-3)[:, None]).astype(f32)
    if family == "parallel":
        dy = (0.7 * x.astype(np.float64) / w * (1.0 + 1e-3 * rs.standard_normal((n, H)))).astype(f32)
    else:
        dy = v32(rs, (n, H))
    return x, w, dy


@functools.lru_cache(maxsize=None)
def rms_plain(case, dtype):
    H, n, flags, family = case
    rs = rs_of("rms", case, dtype)
    c = types.SimpleNamespace(H=H, n=n, flags=flags.split(), family=family, dtype=dtype)
    c.n_buf = 2 * n + 1 if "rows" in c.flags else n
    c.rows = rs.permutation(c.n_buf)[:n].astype(np.int32) if "rows" in c.flags else np.arange(n, dtype=np.int32)
    xr, c.w, c.dy = _rms_rows(rs, n, H, family)
    c.x = v32(rs, (c.n_buf, H))
    c.x[c.rows] = xr
    c.prior = v32(rs, (c.n_buf, H))
    c.ref, c.tol, c.tol16 = K.rmsnorm_bwd(c.dy, xr, c.w, RMS_EPS, c.prior[c.rows] if "acc" in c.flags else None, dtype)
    return c


@functools.lru_cache(maxsize=None)
def rms_fused(case, dtype):
    n, H, na, r, p, flags, family = case
    rs = rs_of("rmsf", case, dtype)
    c = types.SimpleNamespace(H=H, n=n, na=na, r=r, p=p, flags=flags.split(), family=family, site=24, dtype=dtype)
    c.x, c.w, c.dy = _rms_rows(rs, n, H, family)
    c.prior = v32(rs, (n, H))
    c.du = [v32(rs, (n, r), 0.1) for _ in range(na)]
    c.A = [v32(rs, (r, H), 0.3) for _ in range(na)]
    prior = c.prior if "acc" in c.flags else None
    c.ref, c.tol, c.tol16 = K.rmsnorm_bwd(c.dy, c.x, c.w, RMS_EPS, prior, dtype, lora=(c.du, c.A, r, p, SEED, c.site))
    # the unfused pair: lora_dx into dy, then the plain backward
    c.dy2, c.tol_dx, _ = K.lora_dx(c.dy, c.du, c.A, r, p, SEED, c.site)
    return c


# ---- ce_fwd_bwd.  (V, ldd kind, label_div, form)
CE = [(1, "V", 1, "dl32"), (5, "64", 4, "dl16"), (255, "64", 1, "dl16"), (256, "V", 4, "dl32"), (257, "64", 4, "dl32"), (1000, "64", 1, "dl16"), (1000, "V", 4, "dl16"),
      (257, "V", 1, "dl16")]
CE_LOSS0, CE_ROWS = 3.25, 16


@functools.lru_cache(maxsize=None)
def ce(case, dtype):
    V, kind, div, form = case
    rs = rs_of("ce", case, dtype)
    R = CE_ROWS
    c = types.SimpleNamespace(V=V, R=R, div=div, form=form, ldl=V + 3, ldd=V if kind == "V" else up(V, 64), coef=float(f32(1024.0 / R)), dtype=dtype)
    c.logits = rs.uniform(-30.0, 30.0, size=(R, V)).astype(f32)                  # a spread of about 60 within a row
    c.logits[5] = rs.standard_normal(V).astype(f32)
    c.logits[5, V // 2] = 40.0                                                   # one logit dominates; the row's label is that column
    n_lab = R // div
    lab = rs.randint(0, V, size=n_lab).astype(np.int32)
    lab[5 // div] = V // 2
    lab[0 if div > 1 else 1], lab[-1] = -100, V + (0 if div > 1 else 2)          # ignored rows: the ignore index, and one label >= V
    if div == 1:
        lab[2] = V
    c.labels = lab
    c.res = K.ce_fwd_bwd(c.logits, lab, div, c.coef, c.ldd, CE_LOSS0, dtype if form == "dl16" else None)
    return c


# ---- gelu: rows * H = 513 is no multiple of 256; the grid covers +-14 (exp(-x^2 / 2) underflows beyond 13.3), +-0 and random values
GELU_ROWS, GELU_H = 3, 171


@functools.lru_cache(maxsize=None)
def gelu(dtype):
    rs = rs_of("gelu", dtype)
    x = np.concatenate([np.linspace(-14.0, 14.0, 225), [0.0, -0.0, 13.5, -13.5, 12.0, -12.0], rs.standard_normal(GELU_ROWS * GELU_H - 231) * 3.0])
    c = types.SimpleNamespace(x=round16(x, dtype).reshape(GELU_ROWS, GELU_H), dh=v32(rs, (GELU_ROWS, GELU_H)), dtype=dtype)
    c.fwd, c.tol_fwd = K.gelu(c.x, dtype)
    c.bwd, c.tol_bwd = K.gelu(c.x, dtype, c.dh)
    return c


# ---- adamw, grad_stats: 256 * 1024 + 5 exceeds grad_stats's 1,024-workgroup grid, so its strided loop runs
OPT_N = [1, 255, 257, 256 * 1024 + 5]
ADAM = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.05, inv_scale=1.0 / 1024.0)


@functools.lru_cache(maxsize=None)
def opt(n):
    rs = rs_of("opt", n)
    c = types.SimpleNamespace(n=n, p=v32(rs, n), m=v32(rs, n, 0.1), v=(rs.standard_normal(n) ** 2 * 0.01).astype(f32), g=[v32(rs, n, 1024.0) for _ in range(3)])
    c.g[0][0], c.v[0] = 0.0, 0.0                                                 # g = 0 with v = 0: the denominator is eps alone
    return c
