"""Inputs of the GEMM tests (tests/test_gemm_ref.py on the CPU, tests/test_gemm_gpu.py on the GPU): made on the host as exact 16-bit (or e4m3) values, returned as
float64 arrays that hold exactly those values, so that the kernel and the float64 reference (oracle/gemm_ref.py) see the same numbers.

Two families.  "moderate": N(0, 1) activations, N(0, 0.05) weights, biases of the size of the results (sigma = 0.05 sqrt(K)).  "integer": small integers and a small K,
so that every product and every partial sum is an integer below 2^24 -- exact in f32 in any order -- and a result compares bit for bit with its correctly rounded
reference."""
import types
import zlib

import numpy as np

from oracle import blim_oracle as O
from oracle import gemm_ref as R


def rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def moderate(M, N, K, dtype, tag=0, w_cols=None):
    """(a [M, K], w [N, w_cols or K]) of the moderate family."""
    g = rng("moderate", M, N, K, dtype, tag)
    return R.round16(g.randn(M, K), dtype), R.round16(0.05 * g.randn(N, w_cols or K), dtype)


def bias_for(N, K, tag=0, scale=1.0):
    """f32 bias of the size of the results (as float64 values)."""
    return (scale * 0.05 * np.sqrt(K) * rng("bias", N, K, tag).randn(N)).astype(np.float32).astype(np.float64)


def integer(M, N, K, tag=0, w_cols=None):
    """Integers: a in [-4, 4], w in [-3, 3] (exact in fp16, bf16 and e4m3); |acc| <= 12 K."""
    g = rng("integer", M, N, K, tag)
    return g.randint(-4, 5, (M, K)).astype(np.float64), g.randint(-3, 4, (N, w_cols or K)).astype(np.float64)


def wrapped(M, N, K1, dtype, tag=0):
    """The w_wrap_k form: a [M, 2 K1] = [first | second], two independent operands of the moderate family (the second half four times the first's size, so that
    losing it -- or the second walk over W -- is an O(1) error whatever the output format), w [N, K1]."""
    g = rng("wrapped", M, N, K1, dtype, tag)
    a = np.concatenate([g.randn(M, K1), 4.0 * g.randn(M, K1)], axis=1)
    return R.round16(a, dtype), R.round16(0.05 * g.randn(N, K1), dtype)


def hi_lo(x, dtype):
    """[hi | lo] of float64 values x along the last axis."""
    hi, lo = R.split16(x, dtype)
    return np.concatenate([hi, lo], axis=1)


def tile_map_operands(M, N, K=64):
    """Integer family for the persistent loop: acc[m, n] = tn + 64 tm + 2^11 (m % 64) + 2^17 (n % 128) with (tm, tn) = (m // 256, n // 256): below 2^24 (tm < 32,
    tn < 64), so exact in f32; every tile has its own values and so has every element of a 64 x 128 block.  Four live K columns, the rest zero; every operand value
    has at most 7 significant bits (exact in bf16 and fp16)."""
    assert M // 256 < 32 and N // 256 < 64
    a, w = np.zeros((M, K)), np.zeros((N, K))
    m, n = np.arange(M), np.arange(N)
    a[:, 0], w[:, 0] = 1.0, n // 256
    a[:, 1], w[:, 1] = m // 256, 64.0
    a[:, 2], w[:, 2] = m % 64, 2048.0
    a[:, 3], w[:, 3] = 1024.0, 128.0 * (n % 128)
    return a, w


def tile_map_expected(M, N):
    m, n = np.arange(M)[:, None], np.arange(N)[None, :]
    return (n // 256 + 64 * (m // 256) + 2048 * (m % 64) + 2 ** 17 * (n % 128)).astype(np.float64)


# ---- QKV
ROPE_THETA = 100.0   # (not a model's 1e6: with it the upper half of the 64 frequencies turns a position below 300 by less than 0.3 rad -- sin ~ 0, the rotation the
MAX_POS = 300        # identity -- and a wrong pairing or sign would not show on those columns; theta = 100 turns every dimension by more than a radian)


def positions(M, tag=0):
    """Non-monotonic, repeated, and the table's last position."""
    g = rng("pos", M, tag)
    p = g.randint(0, MAX_POS, M).astype(np.int32)
    p[0] = MAX_POS - 1
    if M > 3:
        p[1], p[2], p[3] = 7, 7, 0
    return p


def qkv_problem(M, nh, nkv, K, dtype, tag=0):
    """a [M, K]; w, bias in the STORED row order of the q / k heads (natural rows permuted by R.qkv_row_order); pos [M]."""
    N = (nh + 2 * nkv) * 128
    a, w_nat = moderate(M, N, K, dtype, ("qkv", tag))
    b_nat = bias_for(N, K, ("qkv", tag))
    order = R.qkv_row_order(nh, nkv)
    return a, w_nat[order], b_nat[order], positions(M, tag)


# ---- SwiGLU
def swiglu_problem(M, N, K, dtype, tag=0):
    """a [M, K], w [N, K] in the stored order (16 gate / 16 up rows interleaved).  One in eight gate ROWS of W is scaled so that its pre-activation is 30 N(0, 1):
    |g| of 20 - 40 on most rows, and on a few beyond 88, where exp(-g) overflows f32 and the sigmoid leaves f32's normal range.  The up rows are six times the gate rows' size: for
    small g and u silu(g) u = g u / 2 = silu(u) g to first order, so gate and up of one size would hide a swap from a bf16 comparison on a fifth of the elements."""
    a, w = moderate(M, N, K, dtype, ("swiglu", tag))
    g = rng("swiglu-big", M, N, K, tag)
    r = np.arange(N)
    w[r % 32 >= 16] = R.round16(6.0 * w[r % 32 >= 16], dtype)
    gate_rows = np.flatnonzero(((r % 32 == 3) | (r % 32 == 11)) & ((r // 32) % 2 == 0))          # one in eight gate rows, the first of them row 3
    w[gate_rows] = R.round16(w[gate_rows] * (30.0 / (0.05 * np.sqrt(K))), dtype)
    return a, w


# ---- LSE
def lse_problem(M, N, K, dtype, tag=0):
    """Logits of the moderate family times 20 (so that a tile's exps spread over many orders of magnitude), row 1 (when there is one) all very negative, row 2 with one dominant logit of
    about +80; labels in every tile, on a tile's first and last column, on the last valid column, and at -1 and >= N."""
    g = rng("lse", M, N, K, dtype, tag)
    a, w = R.round16(g.randn(M, K), dtype), R.round16(0.05 * 20.0 / np.sqrt(K / 64.0) * g.randn(N, K), dtype)
    if M > 2:
        a[:, :2] = 0.0                                               # K columns 0 and 1 belong to the two special rows
        a[1, :], a[2, :] = 0.0, 0.0
        a[1, 0] = -64.0
        w[:, 0] = R.round16(8.0 + 0.25 * np.abs(g.randn(N)), dtype)  # row 1: logit = -64 (8 + |.| / 4): all near -520, spread over ~ 30
        a[2, 1] = 1.0
        w[:, 1] = R.round16(0.5 * g.randn(N), dtype)
        w[5 % N, 1] = 80.0                                           # row 2: one logit of +80 among logits of size 0.5
    nt = (N + 255) // 256
    lab = g.randint(0, N, M).astype(np.int32)
    special = [0, N - 1, 255 if N > 255 else N - 1, 256 if N > 256 else 0, 256 * (nt - 1), -1, N, N + 300, -7]
    for i, v in enumerate(special):
        if i < M:
            lab[M - 1 - i] = v
    for t in range(nt):                                              # a label in every tile
        if nt + 9 + t < M:
            lab[t] = min(256 * t + 17, N - 1)
    return a, w, lab


# ---- fp8
def e4m3_values(shape, g, scale):
    """Exact e4m3 values of size `scale`."""
    return R.e4m3_decode(R.e4m3_encode(scale * g.randn(*shape)))


# ---- whole cases: operands + the reference's result, shared by the CPU and the GPU tests
def qkv_case(M, nh, nkv, K, dtype, tag=0, table=None):
    """table: (cos, sin) [MAX_POS, 64] float32 as the kernel will read them (default: the float32 oracle's)."""
    c = types.SimpleNamespace(M=M, nh=nh, nkv=nkv, K=K, N=(nh + 2 * nkv) * 128, dtype=dtype)
    c.a, c.w, c.bias, c.pos = qkv_problem(M, nh, nkv, K, dtype, tag)
    if table is None:
        cos, sin = O.rope_tables(128, ROPE_THETA, MAX_POS)
        table = cos[:, :64], sin[:, :64]
    c.table = table
    c.cos, c.sin = table[0][c.pos].astype(np.float64), table[1][c.pos].astype(np.float64)
    c.acc, c.A = R.product(c.a, c.w)
    c.ref, c.pre = R.epi_qkv(c.acc, c.A, K, c.bias, c.cos, c.sin, nh, nkv)
    return c


def resid_case(M, N, K, dtype, with_in, with_bias, tag=0, resid_scale=1.0, prod_scale=1.0):
    c = types.SimpleNamespace(M=M, N=N, K=K, dtype=dtype)
    c.a, c.w = moderate(M, N, K, dtype, ("resid", tag))
    c.w = R.round16(c.w * prod_scale, dtype)
    g = rng("resid", M, N, K, tag)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    c.c_before = f32(resid_scale * g.randn(M, N))                     # C's content before the call
    c.resid_in = f32(resid_scale * g.randn(M, N)) if with_in else None
    c.resid = c.resid_in if with_in else c.c_before
    c.bias = bias_for(N, K, ("resid", tag), prod_scale) if with_bias else None
    c.acc, c.A = R.product(c.a, c.w)
    c.ref, c.pre = R.epi_resid(c.acc, c.A, K, c.resid, c.bias)
    return c


def f8_swiglu_case(M, N, K, tag=0):
    """fp8 SwiGLU with the fused e4m3 output: a, w exact e4m3 values of size 1 (w's gate rows partly large, as in swiglu_problem), f32 row / column scales."""
    c = types.SimpleNamespace(M=M, N=N, K=K)
    g = rng("f8swiglu", M, N, K, tag)
    c.a, c.w = e4m3_values((M, K), g, 1.0), e4m3_values((N, K), g, 1.0)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    c.row_scale, c.col_scale = f32(0.5 + g.rand(M)), f32(0.05 * (0.5 + g.rand(N)))
    r = np.arange(N)
    big = (r % 32 < 16) & (g.rand(N) < 0.125)
    c.col_scale[big] *= 16.0
    acc, A = R.product(c.a, c.w)
    sc = c.row_scale[:, None] * c.col_scale[None, :]
    c.acc, c.A = acc * sc, A * sc
    ref, pre = R.epi_swiglu(c.acc, c.A, K)
    # the dequantisation acc * (row_scale * col_scale): two more f32 roundings on each accumulator, passed through like the accumulation error
    M_, h = c.acc.shape[0], N // 2
    v = (2.0 * R.U * np.abs(c.acc)).reshape(M_, N // 32, 2, 16)
    gt, up = c.acc.reshape(M_, N // 32, 2, 16)[:, :, 0].reshape(M_, h), c.acc.reshape(M_, N // 32, 2, 16)[:, :, 1].reshape(M_, h)
    c.ref, c.pre = ref, pre + np.abs(R.silu_grad(gt) * up) * v[:, :, 0].reshape(M_, h) + np.abs(R.silu(gt)) * v[:, :, 1].reshape(M_, h)

    def near_boundary():
        """[M, N / 256] bool: blocks whose amax is within the f32 tolerance of 448 2^k, where the kernel's own amax may pick the neighbouring scale."""
        b, t = np.abs(c.ref).reshape(M, -1, 128), R.tolerance(c.ref, c.pre, "f32").reshape(M, -1, 128)
        amax, tb = b.max(axis=2), t.max(axis=2)
        e = R.e8m0_exponent(amax).astype(np.float64)
        return (amax + tb > FP8 * 2.0 ** e) | (amax - tb <= FP8 * 2.0 ** (e - 1))
    c.near_boundary = near_boundary
    return c


FP8 = 448.0
