"""GPU: the GEMM kernels (csrc/gemm.hip), epilogue by epilogue and form by form, through blim_gemm against the float64 reference of oracle/gemm_ref.py.

Inputs: tests/gemm_inputs.py (16-bit / e4m3 values made on the host; the reference sees exactly those).  The assertion is max |got - ref| / tol <= 1 per element with
R.tolerance (from the reference alone: accumulation gamma_K A, the epilogue's f32 operations, the output's rounding, doubled); the integer family compares bit for
bit.  Every output buffer holds a sentinel before the call; ldc exceeds the output width, every 16-bit epilogue also runs with ldc % 8 == 4 (element stores), and
what the call does not own -- padding columns, the gap between the hi and lo halves, rows >= M, label_logit of rows without a valid label -- must still hold the
sentinel afterwards.  tests/test_gemm_ref.py shows on the CPU that these inputs tell the wrong rules from the right one.  Measured figures:
profiles/r13_gemm_direct.md (each test prints its own as GEMM_MEASURE)."""
import numpy as np
import pytest
import torch

import gemm_inputs as GI
from blim_amd import engine as eng
from oracle import blim_oracle as O
from oracle import gemm_ref as R

pytestmark = pytest.mark.gpu

SENT16 = 0x7E7E                     # fp16: a NaN; bf16: 5.3e37 -- never a value these inputs produce
SENT32 = 0x7E7E7E7E                 # f32: 8.4e37
SENT8 = 0x7E
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ("f16", "bf16")
M_EDGES = (1, 255, 257, 326, 386, 513)          # 326 / 386 end inside the first / second 64-row block of a SPLIT pass
XROWS = 3                                        # rows >= M every output buffer carries (they must keep the sentinel)


# ---------------------------------------------------------------------------- device helpers
def dev16(values, dtype):
    return torch.from_numpy(np.ascontiguousarray(R.bits16(values, dtype)).view(np.int16)).cuda().view(TDT[dtype])


def dev16_bits(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).cuda().view(TDT[dtype])


def host16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def dev8(values):
    return torch.from_numpy(R.e4m3_encode(values)).cuda()


def sent16(rows, ld, dtype):
    return dev16_bits(np.full((rows, ld), SENT16, np.uint16), dtype)


def sent32(*shape):
    return torch.from_numpy(np.full(shape, SENT32, np.int32)).cuda().view(torch.float32)


def bits32(t):
    return t.view(torch.int32).cpu().numpy()


def measure(**kw):
    print("GEMM_MEASURE " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def ratio(got, ref, tol):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "non-finite output"
    err = np.abs(got - ref)
    assert (err[tol == 0] == 0).all()
    nz = tol > 0
    return float((err[nz] / tol[nz]).max()) if nz.any() else 0.0


def ld_for(n_out, ld4):
    """A row stride beyond the output width: a multiple of 8, or (ld4) = 4 mod 8: the kernel's element-store path."""
    return (n_out + 7) // 8 * 8 + (12 if ld4 else 8)


class Out16:
    """A 16-bit output buffer [M + XROWS, ldc] full of sentinels, plain or hi | lo."""

    def __init__(self, M, n_out, dtype, ld4=False, split=False):
        self.M, self.n, self.dtype, self.split = M, n_out, dtype, split
        if split:
            self.lo_off = (n_out + 7) // 8 * 8 + (12 if ld4 else 8)        # a multiple of 8 (vector stores), or 4 mod 8 beside an ldc that is 4 mod 8
            self.ldc = 2 * self.lo_off + (4 if ld4 else 8)
        else:
            self.lo_off, self.ldc = 0, ld_for(n_out, ld4)
        assert self.ldc % 8 == (4 if ld4 else 0) and self.ldc % 4 == 0 and self.lo_off % 4 == 0
        self.t = sent16(M + XROWS, self.ldc, dtype)

    def read(self):
        """-> (hi [M, n] float64, lo or None); asserts every sentinel."""
        raw = host16(self.t)
        own = np.zeros(raw.shape, bool)
        own[:self.M, :self.n] = True
        if self.split:
            own[:self.M, self.lo_off:self.lo_off + self.n] = True
        assert (raw[~own] == SENT16).all(), "a 16-bit element outside the output (padding column, hi | lo gap, row >= M) was written"
        self.raw = raw
        hi = R.from_bits16(raw[:self.M, :self.n], self.dtype)
        return hi, (R.from_bits16(raw[:self.M, self.lo_off:self.lo_off + self.n], self.dtype) if self.split else None)


def check16(o, ref, pre, what, **info):
    """The plain or split 16-bit output o against (ref, pre); returns the ratio(s)."""
    dtype = o.dtype
    hi, lo = o.read()
    x = ratio(hi, ref, R.tolerance(ref, pre, dtype))
    r = {"ratio": x}
    if o.split:
        r["ratio_hilo"] = ratio(hi + lo, ref, R.tolerance(ref, pre, dtype, split=True))
        bound = R.EPS[dtype] * np.abs(hi) + (R.F16_FLOOR if dtype == "f16" else 0.0)            # from the output alone: lo is a rounding error of hi
        assert (np.abs(lo) <= bound).all(), "a lo value larger than half an ulp of its hi value"
    measure(test=what, dtype=dtype, split=int(o.split), ldc=o.ldc, **info, **r)
    assert max(r.values()) <= 1.0, (what, info, r)
    return r


def f32_out(M, N, ld_extra=4):
    ldc = N + ld_extra
    return sent32(M + XROWS, ldc), ldc


def read_f32(t, M, N, before=None):
    """-> [M, N] float64; everything else still holds the sentinel (or `before`, the buffer's bits before an in-place call)."""
    raw = bits32(t)
    own = np.zeros(raw.shape, bool)
    own[:M, :N] = True
    want = np.full(raw.shape, SENT32, np.int32) if before is None else before
    assert (raw[~own] == want[~own]).all(), "an f32 element outside the output (padding column, row >= M) was written"
    return t.cpu().numpy()[:M, :N].astype(np.float64)


# ---------------------------------------------------------------------------- 1. the K walk
K_WALK = (64, 128, 192, 256, 320, 384, 448, 704)          # 1 - 7 and 11 K-steps: past the five-slot ring's wrap in both parities
K_WRAP = (64, 192, 320)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", ["f32", "bf16"])
def test_k_walk(epi, dtype):
    M = N = 256
    worst = 0.0
    for wrap in (False, True):
        for K1 in (K_WRAP if wrap else K_WALK):
            K = 2 * K1 if wrap else K1
            for family in ("integer", "moderate"):
                if family == "integer":
                    a, w = GI.integer(M, N, K, ("walk", wrap), w_cols=K1)
                else:
                    a, w = GI.wrapped(M, N, K1, dtype) if wrap else GI.moderate(M, N, K, dtype, "walk")
                acc, A = R.product(a, w, w_wrap_k=K1 if wrap else 0)
                kw = dict(w_wrap_k=K1) if wrap else {}
                if epi == "f32":
                    c, ldc = f32_out(M, N)
                    eng.gemm("f32", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, c, scale=0.37 if family == "moderate" else 1.0, **kw)
                    got = read_f32(c, M, N)
                    ref, pre = R.epi_f32(acc, A, K, 0.37 if family == "moderate" else 1.0)
                    if family == "integer":
                        assert np.array_equal(got, ref), (K, wrap)
                    else:
                        worst = max(worst, ratio(got, ref, R.tolerance(ref, pre, "f32")))
                else:
                    o = Out16(M, N, dtype)
                    eng.gemm("bf16", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, o.t, **kw)
                    hi, _ = o.read()
                    ref, pre = R.epi_bf16(acc, A, K)
                    if family == "integer":                       # the accumulator is exact: its correctly rounded 16-bit value, bit for bit
                        assert np.array_equal(o.raw[:M, :N], R.bits16(R.round16(ref, dtype), dtype)), (K, wrap)
                    else:
                        worst = max(worst, ratio(hi, ref, R.tolerance(ref, pre, dtype)))
    measure(test="k_walk", epi=epi, dtype=dtype, ratio=worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------- 2. edges of M and N
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld4", [False, True])
@pytest.mark.parametrize("form", ["plain", "bias", "gelu"])
def test_edges_bf16(form, ld4, dtype):
    K = 128
    for M in M_EDGES:
        for N in (4, 260, 500):
            a, w = GI.moderate(M, N, K, dtype, "edge")
            bias = None if form == "plain" else GI.bias_for(N, K, "edge")
            acc, A = R.product(a, w)
            ref, pre = R.epi_bf16(acc, A, K, bias, act=1 if form == "gelu" else 0)
            o = Out16(M, N, dtype, ld4)
            kw = {} if bias is None else dict(bias=dev32(bias))
            eng.gemm("bf16", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, o.t, act=1 if form == "gelu" else 0, **kw)
            check16(o, ref, pre, "edges_bf16", form=form, M=M, N=N)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_f32(dtype):
    K = 128
    for M in M_EDGES:
        for N in (4, 260, 500):
            for extra in (4, 3):                                   # ldc % 4 == 0: float4 stores; otherwise element stores
                a, w = GI.moderate(M, N, K, dtype, "edge")
                acc, A = R.product(a, w)
                ref, pre = R.epi_f32(acc, A, K, -1.75)
                c, ldc = f32_out(M, N, extra)
                eng.gemm("f32", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, c, scale=-1.75)
                x = ratio(read_f32(c, M, N), ref, R.tolerance(ref, pre, "f32"))
                measure(test="edges_f32", dtype=dtype, M=M, N=N, ldc=ldc, ratio=x)
                assert x <= 1.0, (M, N, extra, x)


# ---------------------------------------------------------------------------- 3. the residual epilogue
def run_resid(c, dtype, what):
    M, N, K = c.M, c.N, c.K
    ldc = N + 4
    buf = np.full((M + XROWS, ldc), SENT32, np.int32)
    kw = {}
    if c.resid_in is None:
        buf[:M, :N] = c.c_before.astype(np.float32).view(np.int32)
    else:                                                           # C holds the sentinel everywhere: it is not read
        rin = np.full((M, ldc), np.nan, np.float32)
        rin[:, :N] = c.resid_in
        kw["resid_in"] = torch.from_numpy(rin).cuda()
    if c.bias is not None:
        kw["bias"] = dev32(c.bias)
    t = torch.from_numpy(buf).cuda().view(torch.float32)
    eng.gemm("resid", dtype, dev16(c.a, dtype), dev16(c.w, dtype), M, N, K, t, **kw)
    got = read_f32(t, M, N)
    x = ratio(got, c.ref, R.tolerance(c.ref, c.pre, "f32"))
    measure(test=what, dtype=dtype, M=M, N=N, resid_in=int(c.resid_in is not None), bias=int(c.bias is not None), ratio=x)
    assert x <= 1.0, (what, M, N, x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_in", [False, True])
def test_resid(with_in, with_bias, dtype):
    for M in M_EDGES:
        for N in (4, 260, 500):
            run_resid(GI.resid_case(M, N, 128, dtype, with_in, with_bias), dtype, "resid")
    # a residual of 1e3 against a product (and bias) of 1e-2: resid + (acc + bias) within the f32 bound of THAT order
    run_resid(GI.resid_case(257, 260, 128, dtype, with_in, with_bias, "big", resid_scale=1e3, prod_scale=0.02), dtype, "resid_1e3")


# ---------------------------------------------------------------------------- 4. log-sum-exp partials and the label gather
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [256, 260, 1000])
def test_lse(N, dtype):
    K = 128
    for M in M_EDGES:
        a, w, lab = GI.lse_problem(M, N, K, dtype)
        acc, A = R.product(a, w)
        ref = R.epi_lse(acc, A, K, lab)
        nt = (N + 255) // 256
        part, ll = sent32(M + XROWS, nt, 2), sent32(M + XROWS)
        eng.gemm("lse", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, None, labels=torch.from_numpy(lab).cuda(), lse_part=part, label_logit=ll)
        run_lse_checks(part, ll, ref, lab, M, N, dtype, "lse")


def run_lse_checks(part, ll, ref, lab, M, N, dtype, what):
    assert (bits32(part)[M:] == SENT32).all(), "an lse partial of a row >= M was written"
    p = part.cpu().numpy()[:M].astype(np.float64)
    ok = (lab >= 0) & (lab < N)
    llb = bits32(ll)
    assert (llb[M:] == SENT32).all() and (llb[:M][~ok] == SENT32).all(), "label_logit of a row without a valid label was written"
    m, s = p[..., 0], p[..., 1]
    r = dict(ratio_m=ratio(m, ref["m"], ref["tol_m"]), ratio_s=ratio(s, ref["s"], ref["tol_s"]))
    if ok.any():
        r["ratio_label"] = ratio(ll.cpu().numpy()[:M][ok].astype(np.float64), ref["label"][ok], ref["tol_label"][ok])
    r["ratio_lse"] = ratio(R.lse_combine(m, s), ref["lse"], ref["tol_lse"])
    measure(test=what, dtype=dtype, M=M, N=N, **r)
    assert max(r.values()) <= 1.0, (what, M, N, r)


# ---------------------------------------------------------------------------- 5. QKV + bias + RoPE
def rope_table(pos, stride, theta=GI.ROPE_THETA):
    """The table blim_rope_rows builds for pos, on the device, and its rows' (cos, sin) [len(pos), 64] as the kernel will read them."""
    t = eng.rope_rows(torch.from_numpy(pos).cuda(), theta, GI.MAX_POS, stride)
    torch.cuda.synchronize()
    cos, sin = R.rope_rows_unpack(t.cpu().numpy(), len(pos))
    return t, cos, sin


@pytest.mark.parametrize("theta", [GI.ROPE_THETA, 1.0e6])
def test_rope_rows_table(theta):
    """blim_rope_rows against the float32 oracle's table, positions out of range clamped, the rows beyond n_tokens of every chunk untouched."""
    pos = np.concatenate([GI.positions(300), [-5, GI.MAX_POS, GI.MAX_POS + 1000, -2 ** 31, 2 ** 31 - 1]]).astype(np.int32)
    stride = len(pos) + 7
    t, cos, sin = rope_table(pos, stride, theta)
    full = t.cpu().numpy()
    assert np.isnan(full[:, len(pos):]).all(), "a table row >= n_tokens was written"
    oc, osn = O.rope_tables(128, theta, GI.MAX_POS)
    p = np.clip(pos.astype(np.int64), 0, GI.MAX_POS - 1)
    tol = R.rope_table_tolerance(pos, theta, GI.MAX_POS)
    x = max(ratio(cos, oc[p][:, :64].astype(np.float64), tol), ratio(sin, osn[p][:, :64].astype(np.float64), tol))
    measure(test="rope_rows", theta=theta, ratio=x)
    assert x <= 1.0
    assert np.array_equal(cos[-5:], cos[[np.flatnonzero(p == v)[0] for v in (0, GI.MAX_POS - 1, GI.MAX_POS - 1, 0, GI.MAX_POS - 1)]])      # clamped, bit for bit
    assert np.array_equal(cos[1], cos[2]) and np.array_equal(sin[1], sin[2])                                                         # a repeated position


QKV_HEADS = ((1, 1), (2, 1), (3, 1), (4, 2))      # N = 384 (half-empty last tile), 512 (rope / plain boundary between waves of one tile), 640, 1024


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("heads", QKV_HEADS)
def test_qkv(heads, split, dtype):
    nh, nkv = heads
    K = 128
    for M in M_EDGES:
        for ld4 in (False, True):
            if ld4 and M not in (257, 386):
                continue
            pos = GI.positions(M)
            table, cos, sin = rope_table(pos, M + 9)
            c = GI.qkv_case(M, nh, nkv, K, dtype, table=None)
            c.cos, c.sin = cos.astype(np.float64), sin.astype(np.float64)
            ref, pre = R.epi_qkv(c.acc, c.A, K, c.bias, c.cos, c.sin, nh, nkv)
            o = Out16(M, c.N, dtype, ld4, split)
            eng.gemm("qkv", dtype, dev16(c.a, dtype), dev16(c.w, dtype), M, c.N, K, o.t, bias=dev32(c.bias), rope_cols=(nh + nkv) * 128, rope_rows=table,
                     rope_stride=M + 9, lo_off=o.lo_off)
            check16(o, ref, pre, "qkv", nh=nh, nkv=nkv, M=M)


def test_qkv_reads_a_host_written_table():
    """The same epilogue fed a table written on the host in gemm.hpp's chunk-major layout (the float32 oracle's values): the layout statement of R.rope_rows_layout
    and the device's gather agree."""
    M, nh, nkv, K, dtype = 257, 2, 1, 64, "f16"
    c = GI.qkv_case(M, nh, nkv, K, dtype)
    tab = R.rope_rows_layout(c.table[0], c.table[1], c.pos, M + 3, GI.MAX_POS)
    o = Out16(M, c.N, dtype)
    eng.gemm("qkv", dtype, dev16(c.a, dtype), dev16(c.w, dtype), M, c.N, K, o.t, bias=dev32(c.bias), rope_cols=(nh + nkv) * 128, rope_rows=torch.from_numpy(tab).cuda(),
             rope_stride=M + 3)
    check16(o, c.ref, c.pre, "qkv_host_table", M=M)


# ---------------------------------------------------------------------------- 6. SwiGLU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("N", [64, 288, 512, 768])
def test_swiglu(N, split, dtype):
    K = 128
    for M in M_EDGES:
        for ld4 in (False, True):
            if ld4 and M not in (257, 386):
                continue
            a, w = GI.swiglu_problem(M, N, K, dtype)
            acc, A = R.product(a, w)
            ref, pre = R.epi_swiglu(acc, A, K)
            o = Out16(M, N // 2, dtype, ld4, split)
            eng.gemm("swiglu", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, o.t, lo_off=o.lo_off)
            check16(o, ref, pre, "swiglu", M=M, N=N)
            assert M < 255 or np.abs(acc).max() > 40                # the large gates are there


# ---------------------------------------------------------------------------- 7. split outputs of the plain epilogue
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld4", [False, True])
def test_split_bf16(ld4, dtype):
    K = 128
    for M in M_EDGES:
        for N in (260, 512):
            a, w = GI.moderate(M, N, K, dtype, "split")
            bias = GI.bias_for(N, K, "split")
            acc, A = R.product(a, w)
            ref, pre = R.epi_bf16(acc, A, K, bias)
            o = Out16(M, N, dtype, ld4, split=True)
            eng.gemm("bf16", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, o.t, bias=dev32(bias), lo_off=o.lo_off)
            check16(o, ref, pre, "split_bf16", M=M, N=N)


# ---------------------------------------------------------------------------- 8. fp16 saturation
@pytest.mark.parametrize("saturate", [1, 0])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("epi", ["bf16", "qkv", "swiglu"])
def test_f16_saturation(epi, split, saturate):
    """An accumulator beyond 65504 leaves as +-65504 (f16_saturate = 1) or +-inf (0); a NaN operand gives NaN either way.  Checked on the hi half of split outputs."""
    dtype, M, K = "f16", 257, 64
    N = 384 if epi == "qkv" else 512
    a = np.full((M, K), 8.0)
    w = np.full((N, K), 256.0)                                     # acc = 64 * 8 * 256 = 131072
    w[1::2] = -256.0                                               # odd (stored) rows negative
    if epi == "swiglu":
        r = np.arange(N)
        w[r % 32 < 16] = 0.0625                                    # gate = 32: silu(32) = 32; up = +-131072 / 32 ... times 32
        w[r % 32 >= 16] = np.where(r[r % 32 >= 16] % 2 == 1, -8.0, 8.0)[:, None]
    a[5, 3] = np.nan
    o = Out16(M, N // 2 if epi == "swiglu" else N, dtype, split=split)
    kw = dict(lo_off=o.lo_off)
    if epi == "qkv":
        pos = np.zeros(M, np.int32)                                # position 0: the identity rotation
        table, _, _ = rope_table(pos, M)
        kw.update(bias=dev32(np.zeros(N)), rope_cols=256, rope_rows=table, rope_stride=M)
    eng.gemm(epi, dtype, dev16(a, dtype), dev16_bits(R.bits16(w, dtype), dtype), M, N, K, o.t, f16_saturate=saturate, **kw)
    hi, _ = o.read()
    assert np.isnan(hi[5]).all(), "a NaN operand did not give NaN"
    rest = np.delete(hi, 5, axis=0)
    big = 65504.0 if saturate else np.inf
    if epi == "swiglu":
        sign = np.where(np.arange(N // 2) % 2 == 1, -1.0, 1.0)
    elif epi == "qkv":
        assert np.array_equal(R.qkv_row_order(1, 1) % 2, np.arange(N) % 2)                         # the row permutation keeps a row's parity
        sign = np.where(np.arange(N) % 2 == 1, -1.0, 1.0)
    else:
        sign = np.where(np.arange(N) % 2 == 1, -1.0, 1.0)
    assert np.array_equal(rest, np.broadcast_to(big * sign, rest.shape)), (epi, split, saturate)


# ---------------------------------------------------------------------------- 9. the persistent tile loop and its two tile maps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(4352, 4096), (2048, 8448)])
def test_persistent_loop_tile_maps(shape, dtype):
    """(4352, 4096): 272 tiles, the round-robin map (chosen by shape), more virtual block ids than tiles (the `continue` path), a last band of one M-tile.
    (2048, 8448): 264 tiles, the contiguous map, more tiles than CUs.  Every element holds its own f(row, col): bit-exact over the whole output."""
    M, N = shape
    a, w = GI.tile_map_operands(M, N)
    c, ldc = f32_out(M, N)
    eng.gemm("f32", dtype, dev16(a, dtype), dev16(w, dtype), M, N, 64, c)
    torch.cuda.synchronize()
    got = c[:M, :N].cpu().numpy()
    assert (bits32(c[M:]) == SENT32).all() and (bits32(c[:, N:]) == SENT32).all()
    want = GI.tile_map_expected(M, N)
    bad = got != want
    assert not bad.any(), f"{int(bad.sum())} wrong elements, first at {np.argwhere(bad)[0]}: tiles {sorted(set(map(tuple, (np.argwhere(bad) // 256).tolist())))[:8]}"


# ---------------------------------------------------------------------------- 10. the e2m3 second pass (lo6)
def lo6_operands(M, N, K, dtype, w_fn=None, tag=0):
    """a = [hi | lo] [M, 2 K] (lo a true lo part, with ragged block magnitudes), w [N, K]; the reference product hi . w + e2m3(lo) . e2m3(w) and its A."""
    g = GI.rng("lo6", M, N, K, dtype, tag)
    x = g.randn(M, K) * (1 + 3 * (g.rand(M, K) < 0.01))
    hi, lo = R.split16(x, dtype)
    w = w_fn(M, N, K, dtype) if w_fn else R.round16(0.05 * g.randn(N, K), dtype)
    _, _, lo6 = R.e2m3_quant(lo)
    _, _, w6 = R.e2m3_quant(w)
    acc = hi @ w.T + lo6 @ w6.T
    A = np.abs(hi) @ np.abs(w).T + np.abs(lo6) @ np.abs(w6).T
    return np.concatenate([hi, lo], axis=1), w, acc, A


def f6_buffers(M, N, K):
    lib = eng.load_library()
    return (torch.full((lib.blim_f6_tiles_bytes(M, K),), SENT8, dtype=torch.uint8, device="cuda"),
            torch.full((lib.blim_f6_tiles_bytes(N, K),), SENT8, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [128, 256, 640])
def test_lo6_qkv_and_lse(K, dtype):
    M, nh, nkv = 326, 2, 1
    N = (nh + 2 * nkv) * 128
    a, w, acc, A = lo6_operands(M, N, K, dtype)
    bias = GI.bias_for(N, K, "lo6")
    pos = GI.positions(M)
    table, cos, sin = rope_table(pos, M + 9)
    ref, pre = R.epi_qkv(acc, A, 2 * K, bias, cos.astype(np.float64), sin.astype(np.float64), nh, nkv)
    a6, w6 = f6_buffers(M, N, K)
    o = Out16(M, N, dtype, split=True)
    eng.gemm("qkv", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, o.t, bias=dev32(bias), rope_cols=(nh + nkv) * 128, rope_rows=table, rope_stride=M + 9,
             lo_off=o.lo_off, A6=a6, W6=w6, f6_build=1)
    check16(o, ref, pre, "lo6_qkv", M=M, K=K)
    # the images the entry built are the reference quantiser's, byte for byte
    assert np.array_equal(a6.cpu().numpy().reshape(-1, K // 128, R.F6_TILE_BYTES), R.e2m3_tiles(a[:, K:], False))
    assert np.array_equal(w6.cpu().numpy().reshape(-1, K // 128, R.F6_TILE_BYTES), R.e2m3_tiles(w, True))
    # LSE with the second pass: N = 512 and a ragged N = 500
    for n in (512, 500):
        w_fn = lambda M_, N_, K_, dt: R.round16(20.0 * 0.05 / np.sqrt(K_ / 64.0) * GI.rng("lo6-lse", N_, K_, dt).randn(N_, K_), dt)
        a, w, acc, A = lo6_operands(M, n, K, dtype, w_fn, "lse")
        lab = GI.lse_problem(M, n, 64, dtype)[2]
        r = R.epi_lse(acc, A, 2 * K, lab)
        a6, w6 = f6_buffers(M, n, K)
        part, ll = sent32(M + XROWS, 2, 2), sent32(M + XROWS)
        eng.gemm("lse", dtype, dev16(a, dtype), dev16(w, dtype), M, n, K, None, labels=torch.from_numpy(lab).cuda(), lse_part=part, label_logit=ll, A6=a6, W6=w6, f6_build=1)
        run_lse_checks(part, ll, r, lab, M, n, dtype, "lo6_lse")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [128, 256, 640])
def test_lo6_swiglu_and_its_fused_tile_writer(K, dtype):
    M, N = 386, 512
    w_fn = lambda M_, N_, K_, dt: GI.swiglu_problem(M_, N_, K_, dt, "lo6")[1]
    a, w, acc, A = lo6_operands(M, N, K, dtype, w_fn)
    ref, pre = R.epi_swiglu(acc, A, 2 * K)
    ad, wd = dev16(a, dtype), dev16(w, dtype)
    for split in (False, True):
        a6, w6 = f6_buffers(M, N, K)
        o = Out16(M, N // 2, dtype, split=split)
        eng.gemm("swiglu", dtype, ad, wd, M, N, K, o.t, lo_off=o.lo_off, A6=a6, W6=w6, f6_build=1)
        check16(o, ref, pre, "lo6_swiglu", M=M, K=K)
    stored_lo = o.raw[:M, o.lo_off:o.lo_off + N // 2].copy()
    # out6: the lo half leaves as the e2m3 tiles of the consuming GEMM instead of the 16-bit store
    lib = eng.load_library()
    out6 = torch.full((lib.blim_f6_tiles_bytes(M, N // 2),), SENT8, dtype=torch.uint8, device="cuda")
    o2 = Out16(M, N // 2, dtype, split=True)
    eng.gemm("swiglu", dtype, ad, wd, M, N, K, o2.t, lo_off=o2.lo_off, A6=a6, W6=w6, f6_build=1, out6=out6)
    raw = host16(o2.t)
    assert (raw[:, N // 2:] == SENT16).all() and (raw[M:] == SENT16).all(), "with out6 the lo half at C + lo_off must stay unwritten"
    assert np.array_equal(raw[:M, :N // 2], o.raw[:M, :N // 2]), "the hi half differs from the non-fused call's"
    img = out6.cpu().numpy().reshape(-1, N // 256, R.F6_TILE_BYTES)
    want = R.e2m3_tiles(R.from_bits16(stored_lo, dtype), False)     # rows >= M: zero blocks, scale byte 0
    assert np.array_equal(img, want), "out6 is not the tile image of the lo half the non-fused call stores"
    # ... and byte for byte what launch_f6_tiles writes for those stored rows (built by the entry from a [hi | lo] operand that carries them)
    carrier = np.zeros((M, N), np.uint16)
    carrier[:, N // 2:] = stored_lo
    a6b, w6b = f6_buffers(M, 4, N // 2)
    c, _ = f32_out(M, 4)
    c.zero_()
    eng.gemm("resid", dtype, dev16_bits(carrier, dtype), dev16(np.zeros((4, N // 2)), dtype), M, 4, N // 2, c, A6=a6b, W6=w6b, f6_build=1)
    assert np.array_equal(out6.cpu().numpy(), a6b.cpu().numpy())


# ---------------------------------------------------------------------------- 11. fp8 forms
def test_f8_swiglu_fused_e4m3_output():
    M, N, K = 300, 512, 256
    c = GI.f8_swiglu_case(M, N, K)
    I = N // 2
    ldc, stride = I + 16, 512 + 256                                 # bytes per row / per K-step of the consumer: both larger than the minimum
    out8 = torch.full((M + XROWS, ldc), SENT8, dtype=torch.uint8, device="cuda")
    mx = torch.full((I // 128 * stride,), SENT8, dtype=torch.uint8, device="cuda")
    eng.gemm("swiglu", "f8", dev8(c.a), dev8(c.w), M, N, K, None, ldc=ldc, row_scale=dev32(c.row_scale), col_scale=dev32(c.col_scale), out8=out8, out_mx=mx, mx_stride=stride)
    b, mxh = out8.cpu().numpy(), mx.cpu().numpy()
    assert (b[M:] == SENT8).all() and (b[:, I:] == SENT8).all(), "an e4m3 byte outside the output was written"
    for k in range(I // 128):
        assert (mxh[k * stride + 512:(k + 1) * stride] == SENT8).all(), "a scale byte beyond the row tiles was written"
    _, e_ref, _ = R.quant_e4m3_mx(c.ref)
    rows = np.arange(M)
    e_got = np.stack([mxh[R.mx_index(rows, k, stride)].astype(np.int64) - 127 for k in range(I // 128)], axis=1)
    near = c.near_boundary()
    diff = e_got != e_ref
    assert (np.abs(e_got - e_ref)[diff] == 1).all() and not (diff & ~near).any(), "a scale byte differs from the reference's away from a binade boundary"
    assert near.mean() <= 0.02
    sc = np.repeat(2.0 ** e_got.astype(np.float64), 128, axis=1)
    deq = R.e4m3_decode(b[:M, :I]) * sc
    tol = R.tolerance(c.ref, c.pre, "f32")
    bound = 0.5 * R.e4m3_ulp(np.minimum((np.abs(c.ref) + tol) / sc, 448.0)) * sc + tol
    x = ratio(deq, c.ref, bound)
    measure(test="f8_swiglu_out8", M=M, N=N, K=K, ratio=x, scale_bytes_off_by_one=int(diff.sum()), near_boundary=int(near.sum()))
    assert x <= 1.0
    # the plain fp8 SwiGLU (fp16 output) on the same operands
    o = Out16(M, I, "f16")
    eng.gemm("swiglu", "f8", dev8(c.a), dev8(c.w), M, N, K, o.t, row_scale=dev32(c.row_scale), col_scale=dev32(c.col_scale))
    check16(o, c.ref, c.pre, "f8_swiglu_f16", M=M, N=N)


def test_f8_resid_with_mx_scaled_a_is_exact():
    """EPI_RESID with a_mx: integer-valued e4m3 operands, power-of-two E8M0 block scales and column scales, an integer residual: every term is exact in f32."""
    M, N, K = 300, 260, 384
    g = GI.rng("f8resid")
    a, w = GI.integer(M, N, K, "f8")
    e = g.randint(-2, 3, (M, K // 128))
    cs = 2.0 ** g.randint(-3, 1, N)
    stride = 512 + 256
    mx = np.full(K // 128 * stride, SENT8, np.uint8)
    for k in range(K // 128):
        mx[R.mx_index(np.arange(M), k, stride)] = (e[:, k] + 127).astype(np.uint8)
    before = g.randint(-50, 51, (M, N)).astype(np.float64)
    ref = before + sum((a[:, 128 * k:128 * k + 128] * 2.0 ** e[:, k:k + 1]) @ w[:, 128 * k:128 * k + 128].T for k in range(K // 128)) * cs[None, :]
    ldc = N + 4
    buf = np.full((M + XROWS, ldc), SENT32, np.int32)
    buf[:M, :N] = before.astype(np.float32).view(np.int32)
    t = torch.from_numpy(buf).cuda().view(torch.float32)
    eng.gemm("resid", "f8", dev8(a), dev8(w), M, N, K, t, col_scale=dev32(cs), a_mx=torch.from_numpy(mx).cuda(), mx_stride=stride)
    got = read_f32(t, M, N)
    assert np.array_equal(got, ref)
    assert np.abs(ref - before).max() > 100


# ---------------------------------------------------------------------------- 12. the trainer's fused SwiGLU forms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("I", [32, 144, 256])
def test_trainer_swiglu_forward(I, dtype):
    """EPI_BF16 with swiglu_act: C = gate | up as usual, act = silu(gate16) * up16 from the rounded values C holds, in interior tiles (M = 513, I = 256) and edges."""
    N, K = 2 * I, 128
    for M in (255, 513):
        a, w = GI.swiglu_problem(M, N, K, dtype, "train")
        acc, A = R.product(a, w)
        ref, pre = R.epi_bf16(acc, A, K)
        o = Out16(M, N, dtype)
        act = Out16(M, I, dtype)
        eng.gemm("bf16", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, o.t, swiglu_act=act.t, swiglu_act_ld=act.ldc)
        check16(o, ref, pre, "train_fwd_c", M=M, I=I)
        c16 = R.from_bits16(o.raw[:M, :N], dtype)
        aref, apre = R.train_swiglu_act(c16)
        check16(act, aref, apre, "train_fwd_act", M=M, I=I)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("I", [32, 144, 256])
def test_trainer_swiglu_backward(I, dtype):
    """EPI_BF16 with swiglu_gu: the tile d act is not stored; the saved gate | up rows (row stride > 2 I) become [d gate | d up] in place."""
    N, K = I, 128
    for M in (255, 513):
        a, w = GI.moderate(M, N, K, dtype, "train-bwd")
        g = GI.rng("train-bwd", M, I, dtype)
        gu = R.round16(g.randn(M, 2 * I) * np.where(g.rand(M, 2 * I) < 0.05, 12.0, 1.0), dtype)
        acc, A = R.product(a, w)
        ref, pre = R.train_swiglu_gu(acc, A, K, gu, dtype)
        buf = Out16(M, 2 * I, dtype)
        bits = host16(buf.t)
        bits[:M, :2 * I] = R.bits16(gu, dtype)
        buf.t = dev16_bits(bits, dtype)
        c = Out16(M, N, dtype)
        eng.gemm("bf16", dtype, dev16(a, dtype), dev16(w, dtype), M, N, K, c.t, f16_saturate=0, swiglu_gu=buf.t, swiglu_ld=buf.ldc)
        assert (host16(c.t) == SENT16).all(), "the d act tile was stored"
        check16(buf, ref, pre, "train_bwd", M=M, I=I)
