"""GPU: the trainer's LoRA, RMSNorm-backward, cross-entropy, GELU, AdamW and gradient-statistics kernels (csrc/train_kernels.hip), each driven alone through
blim_lora_down / blim_lora_grads / blim_lora_dx / blim_rmsnorm_bwd / blim_ce_fwd_bwd / blim_gelu / blim_adamw_raw / blim_grad_stats_raw against the float64
reference of oracle/train_kernels_ref.py.

Inputs: tests/train_kernel_inputs.py -- exact 16-bit / f32 values made on the host, references computed once per case.  EVERY element a call owns is compared:
max |got - ref| / tol <= 1 with the per-element tolerance the reference derives from its own magnitudes (printed as TRAIN_KERNEL_MEASURE); where tol = 0 the
result must be exact.  What a call does not own -- row padding, rows at T and beyond, rows a gather does not name, dx in the out16 form, the x columns of an
augmented row -- holds a sentinel before the call and must hold it afterwards.  Workspaces are filled with 0xFF bytes; inputs a kernel's contract says it never
reads hold NaN; every reduction kernel is called twice and must give identical bits.  tests/test_train_kernels_ref.py shows on the CPU that these inputs tell the
wrong rules from the right one.  Measured figures: profiles/r17_train_kernels_direct.md."""
import math

import numpy as np
import pytest
import torch

import train_kernel_inputs as TI
from blim_amd import engine as eng
from oracle import train_kernels_ref as K
from oracle.attention_ref import bits16, from_bits16

pytestmark = pytest.mark.gpu

NAN16 = {"f16": 0x7E00, "bf16": 0x7FC0}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
SENT16 = 0x7B7B                     # 61280 as fp16, 1.3e36 as bf16: never a result of these inputs
SENT32 = 0x7E7E7E7E                 # 8.4e37 as f32
ids = lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


def dev16(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).cuda().view(TDT[dtype])


def rows16(x, n_rows, ld, dtype, fill):
    """x [T, cols] 16-bit values as rows of stride ld in an [n_rows, ld] array of bit patterns; everything else holds `fill`."""
    out = np.full((n_rows, ld), fill, np.uint16)
    out[:x.shape[0], :x.shape[1]] = bits16(x, dtype)
    return out


def bits_of(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.element_size() == 2 else t.view(torch.int32).cpu().numpy()


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def sent32(shape):
    return np.full(shape, SENT32, np.int32).view(np.float32)


def nan32(shape):
    return np.full(shape, np.nan, np.float32)


def poisoned(n_bytes):
    assert n_bytes > 0
    return torch.full((n_bytes,), 0xFF, dtype=torch.uint8, device="cuda")          # 0xFFFF / 0xFFFFFFFF: NaN in fp16, bf16 and f32


def ratio(got, ref, tol, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite values (a poisoned workspace element or a never-read input was read)"
    err = np.abs(got - ref)
    assert (err[tol == 0] == 0).all(), f"{what}: an element with zero tolerance is not exact"
    return float(np.max(err[tol > 0] / tol[tol > 0])) if (tol > 0).any() else 0.0


def measure(kernel, dtype, case, **figs):
    print(f"TRAIN_KERNEL_MEASURE kernel={kernel} dtype={dtype} case={ids(case)} " + " ".join(f"{k}={v:.4g}" for k, v in figs.items()))
    assert all(math.isfinite(v) and v <= 1.0 for k, v in figs.items() if not k.startswith("info_")), (kernel, dtype, case, figs)      # a NaN figure fails too


# ---------------------------------------------------------------------------- lora_down
def run_lora_down(c):
    n_rows = c.T + 3
    host = rows16(c.x, n_rows, c.ldx, c.dtype, SENT16)
    x16 = dev16(host, c.dtype)
    ws = poisoned(eng.lora_down_workspace_bytes(c.n, c.K))
    eng.lora_down(x16, c.T, c.K, [dev32(a) for a in c.A], c.r, TI.SCALE, c.p, TI.SEED, c.site, ws)
    torch.cuda.synchronize()
    return host, bits_of(x16)


@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.LORA_DOWN, ids=ids)
def test_lora_down(case, dtype):
    c = TI.lora_down(case, dtype)
    before, after = run_lora_down(c)
    own = np.zeros(before.shape, bool)
    own[:c.T, c.K:c.K + c.n * c.r] = True
    assert (after[~own] == before[~own]).all(), "something outside columns K .. K + n r of rows < T was written (x columns, row padding, rows >= T)"
    measure("lora_down", dtype, case, u=ratio(from_bits16(after[:c.T, c.K:c.K + c.n * c.r], dtype), c.ref, c.tol, "u"))
    assert (run_lora_down(c)[1] == after).all(), "a second call gave other bits"


# ---------------------------------------------------------------------------- lora_wgrad: dB, dA
def run_dB(c):
    dy = rows16(c.dy, c.T, c.ldy, c.dtype, NAN16[c.dtype])                       # columns [N, ldy): never read into the result
    u = np.full((c.T, c.ldu), SENT16, np.uint16)
    u[:, c.u_off:c.u_off + c.r] = bits16(c.u, c.dtype)
    dB = dev32(np.concatenate([c.dB0.reshape(-1), sent32(16)]))
    ws = poisoned(eng.lora_grads_workspace_bytes(eng.LORA_DB, c.T, c.N, 0, c.r))
    eng.lora_grads(eng.LORA_DB, c.T, c.r, ws, c.dtype, N=c.N, dy16=dev16(dy, c.dtype), ldy=c.ldy, u16=dev16(u, c.dtype), ldu=c.ldu, u16_offset=c.u_off, dB=dB)
    torch.cuda.synchronize()
    return dB


@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.LORA_DB, ids=ids)
def test_lora_dB(case, dtype):
    c = TI.lora_dB(case, dtype)
    dB = run_dB(c)
    assert (bits_of(dB)[c.N * c.r:] == SENT32).all(), "dB was written beyond [N, r]"
    measure("lora_dB", dtype, case, dB=ratio(dB.cpu().numpy()[:c.N * c.r].reshape(c.N, c.r), c.ref, c.tol, "dB"))
    assert (bits_of(run_dB(c)) == bits_of(dB)).all(), "a second call gave other bits"


def run_dA(c):
    x = rows16(c.x, c.T, c.ldx, c.dtype, NAN16[c.dtype])
    dA = dev32(np.concatenate([c.dA0.reshape(-1), sent32(16)]))
    ws = poisoned(eng.lora_grads_workspace_bytes(eng.LORA_DA, c.T, 0, c.K, c.r))
    eng.lora_grads(eng.LORA_DA, c.T, c.r, ws, c.dtype, K=c.K, x16=dev16(x, c.dtype), ldx=c.ldx, du=dev32(c.du), drop_p=c.p, seed=TI.SEED, site=c.site, dA=dA)
    torch.cuda.synchronize()
    return dA


@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.LORA_DA, ids=ids)
def test_lora_dA(case, dtype):
    """The span family holds du rows from 1e-3 to 1e4 in one tensor: info_rel is the kernel's own error relative to sum_t |du| |drop(x)| (the hi / lo claim of
    csrc/train_kernels.hip: ~3e-5 in fp16)."""
    c = TI.lora_dA(case, dtype)
    dA = run_dA(c)
    assert (bits_of(dA)[c.r * c.K:] == SENT32).all(), "dA was written beyond [r, K]"
    got = dA.cpu().numpy()[:c.r * c.K].reshape(c.r, c.K).astype(np.float64)
    xs = K.dropped(c.x, K.mask(TI.SEED, c.site, c.T, c.K, c.p), dtype) if c.p > 0 else c.x
    mag = np.abs(c.du.astype(np.float64)).T @ np.abs(xs)
    measure("lora_dA_" + c.family, dtype, case, dA=ratio(got, c.ref, c.tol, "dA"), info_rel=float(np.max(np.abs(got - c.ref) / np.maximum(mag, 1e-300))))
    assert (bits_of(run_dA(c)) == bits_of(dA)).all(), "a second call gave other bits"


# ---------------------------------------------------------------------------- lora_du
def run_du(c):
    dy = rows16(c.dy, c.T, c.ldy, c.dtype, NAN16[c.dtype])                       # columns [N, Np) are zero (the contract), [Np, ldy) never read
    du = dev32(np.concatenate([nan32(c.T * c.r), sent32(2 * c.r)]))              # du is OVERWRITTEN: what it held must not matter
    ws = poisoned(eng.lora_grads_workspace_bytes(eng.LORA_DU, c.T, c.N, 0, c.r))
    eng.lora_grads(eng.LORA_DU, c.T, c.r, ws, c.dtype, N=c.N, dy16=dev16(dy, c.dtype), ldy=c.ldy, B=dev32(c.B), scale=TI.SCALE, du=du)
    torch.cuda.synchronize()
    return du


@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.LORA_DU, ids=ids)
def test_lora_du(case, dtype):
    c = TI.lora_du(case, dtype)
    du = run_du(c)
    assert (bits_of(du)[c.T * c.r:] == SENT32).all(), "du was written at row T or beyond"
    measure("lora_du", dtype, case, du=ratio(du.cpu().numpy()[:c.T * c.r].reshape(c.T, c.r), c.ref, c.tol, "du"))
    assert (bits_of(run_du(c)) == bits_of(du)).all(), "a second call gave other bits"


@pytest.mark.parametrize("dtype", TI.DTYPES)
def test_lora_grads_trio_in_one_call(dtype):
    """dB, du and dA of one adapter in ONE call, the trainer's lora_backward: du feeds dA inside the call, the three share the workspace."""
    T, N, Kc, r = 65, 100, 136, 16
    b, a, d = TI.lora_dB((T, N, r), dtype), TI.lora_dA((T, Kc, r, TI.DROP, "gauss"), dtype), TI.lora_du((T, N, r), dtype)
    dy = rows16(d.dy, T, d.ldy, dtype, NAN16[dtype])
    u = rows16(b.u, T, r, dtype, SENT16)
    dB, du, dA = dev32(b.dB0), dev32(nan32((T, r))), dev32(a.dA0)
    flags = eng.LORA_DB | eng.LORA_DU | eng.LORA_DA
    ws = poisoned(eng.lora_grads_workspace_bytes(flags, T, N, Kc, r))
    eng.lora_grads(flags, T, r, ws, dtype, N=N, K=Kc, dy16=dev16(dy, dtype), ldy=d.ldy, u16=dev16(u, dtype), ldu=r, x16=dev16(rows16(a.x, T, a.ldx, dtype, NAN16[dtype]), dtype),
                   ldx=a.ldx, B=dev32(d.B), scale=TI.SCALE, drop_p=TI.DROP, seed=TI.SEED, site=a.site, dB=dB, du=du, dA=dA)
    torch.cuda.synchronize()
    dB_ref, dB_tol = K.lora_dB(d.dy[:, :N], b.u, b.dB0)
    got_du = du.cpu().numpy()
    dA_ref, dA_tol = K.lora_dA(got_du, a.x, a.dA0, TI.DROP, TI.SEED, a.site, dtype)          # dA of the du the call itself produced
    measure("lora_trio", dtype, (T, N, Kc, r), dB=ratio(dB.cpu().numpy(), dB_ref, dB_tol, "dB"), du=ratio(got_du, d.ref, d.tol, "du"),
            dA=ratio(dA.cpu().numpy(), dA_ref, dA_tol, "dA"))


# ---------------------------------------------------------------------------- lora_dx
@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.LORA_DX, ids=ids)
def test_lora_dx(case, dtype):
    c = TI.lora_dx(case, dtype)
    host = sent32((c.T + 2, c.ldd)).copy()
    host[:c.T, :c.K] = c.dx0
    dx = dev32(host)
    out16 = dev16(np.full((c.T + 2, c.ldo), SENT16, np.uint16), dtype) if c.out16 else None
    eng.lora_dx(dx, c.T, c.K, [dev32(a) for a in c.du], [dev32(a) for a in c.A], c.r, c.p, TI.SEED, c.site, out16=out16, dtype=dtype)
    torch.cuda.synchronize()
    after = bits_of(dx)
    if c.out16:
        assert (after == host.view(np.int32)).all(), "the out16 form wrote dx"
        o = bits_of(out16)
        assert (o[c.T:] == SENT16).all() and (o[:, c.K:] == SENT16).all(), "out16 was written beyond [T, K]"
        measure("lora_dx16", dtype, case, out16=ratio(from_bits16(o[:c.T, :c.K], dtype), c.ref, c.tol16, "out16"))
    else:
        assert (after[c.T:] == SENT32).all() and (after[:, c.K:] == SENT32).all(), "dx was written beyond [T, K]"
        measure("lora_dx", dtype, case, dx=ratio(dx.cpu().numpy()[:c.T, :c.K], c.ref, c.tol, "dx"))


# ---------------------------------------------------------------------------- rmsnorm_bwd
def run_rms(c, rows, n_buf, x, prior, acc, want16, **lora):
    named = np.zeros(n_buf + 1, bool)
    named[rows] = True
    host = sent32((n_buf + 1, c.H)).copy()
    host[named] = prior[named[:-1].nonzero()[0]] if acc else np.nan             # without accumulate the rows are overwritten: what they held must not matter
    dx = dev32(host)
    out16 = dev16(np.full((n_buf + 1, c.H), SENT16, np.uint16), c.dtype) if want16 else None
    xbuf = np.concatenate([x, nan32((1, c.H))])
    eng.rmsnorm_bwd(dx, dev32(c.dy), dev32(xbuf), dev32(c.w), TI.RMS_EPS, len(rows), c.H, rows=torch.from_numpy(rows).cuda() if lora.get("gather") else None,
                    accumulate=int(acc), out16=out16, dtype=c.dtype, **{k: v for k, v in lora.items() if k != "gather"})
    torch.cuda.synchronize()
    b = bits_of(dx)
    assert (b[~named] == SENT32).all(), "a row that the call does not name was written"
    o = None
    if want16:
        o = bits_of(out16)
        assert (o[~named] == SENT16).all(), "out16: a row that the call does not name was written"
        o = from_bits16(o[rows], c.dtype)
    return dx.cpu().numpy()[rows], o, b


@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.RMS_PLAIN, ids=ids)
def test_rmsnorm_bwd_plain(case, dtype):
    c = TI.rms_plain(case, dtype)
    args = (c, c.rows, c.n_buf, c.x, c.prior, "acc" in c.flags, "out16" in c.flags)
    g, g16, b = run_rms(*args, gather="rows" in c.flags)
    figs = dict(dx=ratio(g, c.ref, c.tol, "dx"))
    if g16 is not None:
        figs["out16"] = ratio(g16, c.ref, c.tol16, "out16")
    measure("rmsnorm_bwd_" + c.family, dtype, case, **figs)
    assert (run_rms(*args, gather="rows" in c.flags)[2] == b).all(), "a second call gave other bits"


@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.RMS_FUSED, ids=ids)
def test_rmsnorm_bwd_fused_adapters(case, dtype):
    c = TI.rms_fused(case, dtype)
    rows = np.arange(c.n, dtype=np.int32)
    acc, want16 = "acc" in c.flags, "out16" in c.flags
    lora = dict(du=[dev32(a) for a in c.du], A=[dev32(a) for a in c.A], r=c.r, drop_p=c.p, seed=TI.SEED, site=c.site)
    g, g16, b = run_rms(c, rows, c.n, c.x, c.prior, acc, want16, **lora)
    figs = dict(dx=ratio(g, c.ref, c.tol, "dx"))
    if g16 is not None:
        figs["out16"] = ratio(g16, c.ref, c.tol16, "out16")
    # the unfused pair on the device: blim_lora_dx into a copy of dy, then the plain backward -- the same bound holds each of the two, so they meet within the sum
    dy2 = dev32(c.dy)
    eng.lora_dx(dy2, c.n, c.H, lora["du"], lora["A"], c.r, c.p, TI.SEED, c.site, dtype=dtype)
    dx2 = dev32(c.prior if acc else nan32((c.n, c.H)))
    eng.rmsnorm_bwd(dx2, dy2, dev32(c.x), dev32(c.w), TI.RMS_EPS, c.n, c.H, accumulate=int(acc), dtype=dtype)
    torch.cuda.synchronize()
    figs["pair"] = ratio(dx2.cpu().numpy(), c.ref, c.tol, "unfused pair")
    figs["fused_vs_pair"] = ratio(g, dx2.cpu().numpy().astype(np.float64), 2.0 * c.tol, "fused against the pair")
    measure("rmsnorm_bwd_fused_" + c.family, dtype, case, **figs)
    assert (run_rms(c, rows, c.n, c.x, c.prior, acc, want16, **lora)[2] == b).all(), "a second call gave other bits"


# ---------------------------------------------------------------------------- ce_fwd_bwd
def run_ce(c):
    lg = nan32((c.R, c.ldl))                                                     # columns [V, ldl) are never read
    lg[:, :c.V] = c.logits
    loss = dev32(np.array([TI.CE_LOSS0, 0.0], np.float32))                       # *loss is incremented; the word behind it must stay
    loss.view(torch.int32)[1] = SENT32
    dl16 = dev16(np.full((c.R + 1, c.ldd), SENT16, np.uint16), c.dtype) if c.form == "dl16" else None
    dl32 = dev32(sent32((c.R + 1, c.ldd))) if c.form == "dl32" else None
    eng.ce_fwd_bwd(dev32(lg), c.V, torch.from_numpy(c.labels).cuda(), c.div, c.R, c.coef, loss, poisoned(eng.ce_workspace_bytes(c.R)), dl16=dl16, dl32=dl32, dtype=c.dtype)
    torch.cuda.synchronize()
    return loss, dl16 if dl16 is not None else dl32


@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("case", TI.CE, ids=ids)
def test_ce_fwd_bwd(case, dtype):
    c = TI.ce(case, dtype)
    loss, dl = run_ce(c)
    b = bits_of(dl)
    assert (b[c.R] == (SENT16 if c.form == "dl16" else SENT32)).all(), "a gradient row beyond n_rows was written"
    assert bits_of(loss)[1] == SENT32
    got = from_bits16(b[:c.R], dtype) if c.form == "dl16" else dl.cpu().numpy()[:c.R]
    assert (np.asarray(got)[:, c.V:] == 0).all() and (np.asarray(got)[~c.res.ok] == 0).all()          # padding columns and ignored rows: exact zeros
    measure("ce_" + c.form, dtype, case, d=ratio(got, c.res.d, c.res.tol_d16 if c.form == "dl16" else c.res.tol_d, "d"),
            loss=ratio([float(loss[0])], np.array([c.res.loss]), np.array([c.res.tol_loss]), "loss"))          # finite: every per-row loss slot of the workspace was written
    loss2, dl2 = run_ce(c)
    assert (bits_of(dl2) == b).all() and (bits_of(loss2) == bits_of(loss)).all(), "a second call gave other bits"


# ---------------------------------------------------------------------------- gelu
@pytest.mark.parametrize("dtype", TI.DTYPES)
def test_gelu_forward_and_backward(dtype):
    c = TI.gelu(dtype)
    R, H = TI.GELU_ROWS, TI.GELU_H
    pre = dev16(bits16(c.x, dtype), dtype)
    fwd = dev16(np.full((R + 1, H + 5), SENT16, np.uint16), dtype)
    eng.gelu(pre, fwd, R, H)
    bwd = dev16(np.full((R + 1, H), SENT16, np.uint16), dtype)
    eng.gelu(pre, bwd, R, H, dh=dev32(c.dh))
    torch.cuda.synchronize()
    f, b = bits_of(fwd), bits_of(bwd)
    assert (f[R] == SENT16).all() and (f[:, H:] == SENT16).all() and (b[R] == SENT16).all(), "gelu wrote beyond [rows, H]"
    measure("gelu", dtype, (R, H), fwd=ratio(from_bits16(f[:R, :H], dtype), c.fwd, c.tol_fwd, "fwd"), bwd=ratio(from_bits16(b[:R], dtype), c.bwd, c.tol_bwd, "bwd"))


# ---------------------------------------------------------------------------- adamw, grad_stats
@pytest.mark.parametrize("n", TI.OPT_N)
def test_adamw_three_chained_steps(n):
    c, h = TI.opt(n), TI.ADAM
    tail = sent32(8)
    p, m, v = (dev32(np.concatenate([a, tail])) for a in (c.p, c.m, c.v))
    worst = 0.0
    for step in (1, 2, 3):
        before = [t.cpu().numpy()[:n] for t in (p, m, v)]                      # each step is checked from the state the kernel itself left
        eng.adamw_raw(p[:n], dev32(c.g[step - 1]), m[:n], v[:n], h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["inv_scale"], step)
        torch.cuda.synchronize()
        r = K.adamw(before[0], c.g[step - 1], before[1], before[2], h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["inv_scale"], step)
        worst = max(worst, ratio(p.cpu().numpy()[:n], r.p, r.tol_p, "p"), ratio(m.cpu().numpy()[:n], r.m, r.tol_m, "m"), ratio(v.cpu().numpy()[:n], r.v, r.tol_v, "v"))
    for t in (p, m, v):
        assert (bits_of(t)[n:] == SENT32).all(), "adamw wrote beyond n"
    measure("adamw", "f32", (n,), pmv=worst)


@pytest.mark.parametrize("n", TI.OPT_N)
def test_grad_stats(n):
    c = TI.opt(n)
    inv = TI.ADAM["inv_scale"]

    def run(g):
        stats = dev32(np.array([2.5, 7.0, 0.0], np.float32))
        stats.view(torch.int32)[2] = SENT32
        eng.grad_stats_raw(dev32(g), inv, stats[:2], poisoned(eng.grad_stats_workspace_bytes(n)))
        torch.cuda.synchronize()
        assert bits_of(stats)[2] == SENT32
        return stats
    s = run(c.g[0])
    want, tol = K.grad_stats(c.g[0], inv, [2.5, 7.0])
    assert float(s[1]) == 7.0, "stats[1] was touched without an inf / NaN"
    measure("grad_stats", "f32", (n,), ss=ratio([float(s[0])], want[:1], np.array([tol]), "stats[0]"))
    assert (bits_of(run(c.g[0])) == bits_of(s)).all(), "a second call gave other bits"
    for bad in (np.inf, np.nan):
        g = c.g[0].copy()
        g[-1] = bad
        assert float(run(g)[1]) == 1.0, f"{bad} at the last element was not flagged"


# ---------------------------------------------------------------------------- refusals: calls that launch nothing
def test_refused_arguments_are_named():
    H = 128
    f = lambda *s: torch.zeros(s, device="cuda")
    x16 = torch.zeros((4, H), dtype=torch.float16, device="cuda")
    rows = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(eng.BlimError, match="out16 with rows"):
        eng.rmsnorm_bwd(f(4, H), f(2, H), f(4, H), f(H), 1e-6, 2, H, rows=rows, out16=x16)
    with pytest.raises(eng.BlimError, match="adapters with rows"):
        eng.rmsnorm_bwd(f(4, H), f(2, H), f(4, H), f(H), 1e-6, 2, H, rows=rows, du=[f(2, 4)], A=[f(4, H)], r=4)
    with pytest.raises(eng.BlimError, match="> 4096"):
        eng.rmsnorm_bwd(f(1, 4100), f(1, 4100), f(1, 4100), f(4100), 1e-6, 1, 4100, du=[f(1, 4)], A=[f(4, 4100)], r=4)
    with pytest.raises(eng.BlimError, match="> 8192"):
        eng.rmsnorm_bwd(f(1, 8196), f(1, 8196), f(1, 8196), f(8196), 1e-6, 1, 8196)
    with pytest.raises(eng.BlimError, match="workspace"):
        eng.lora_down(torch.zeros((4, 16 + 64), dtype=torch.float16, device="cuda"), 4, 16, [f(4, 16)], 4, 1.0, 0.0, 0, 0, poisoned(eng.lora_down_workspace_bytes(1, 16) - 16))
    with pytest.raises(eng.BlimError):
        eng.lora_down(torch.zeros((4, 16 + 64), dtype=torch.float16, device="cuda"), 4, 16, [f(17, 16)], 17, 1.0, 0.0, 0, 0, poisoned(4096))          # r > 16
    assert eng.lora_grads_workspace_bytes(0, 4, 16, 16, 4) == -1 and eng.ce_workspace_bytes(0) == -1 and eng.grad_stats_workspace_bytes(0) == -1
