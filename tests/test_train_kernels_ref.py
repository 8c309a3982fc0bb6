"""CPU: oracle/train_kernels_ref.py, the float64 reference of tests/test_train_kernels_gpu.py, checked without a GPU.

1. Every reference is pinned to an independent statement of the operation: torch float64 autograd for y = w x rsqrt(mean x^2 + eps), cross_entropy, exact-erf
   GELU and y = s B A (mask o x) (the four LoRA gradients); the fused-adapter RMSNorm backward = lora_dx followed by the plain backward; torch.optim.AdamW over
   three steps with weight decay and a loss scale.
2. An emulation of each kernel's roundings in numpy (f32 sums, 16-bit operands, the hi / lo split, the native exponential modelled as f32) stays inside the
   tolerance on exactly the inputs the GPU tests use (tests/train_kernel_inputs.py).
3. Each wrong rule of K.RULES leaves the tolerance on AT LEAST ONE case of the input set of every kernel it can change (printed as TRAIN_KERNEL_RULE lines, case by
   case).  Not on every case: lo_dropped hides in fp16 at T >= 1024 and A_unrounded at K = 1024 and on the one-element case, inside the f32 term n U sum |a||b| and an
   output's own half ulp (profiles/r17_train_kernels_direct.md)."""
import numpy as np
import pytest
import torch

import train_kernel_inputs as TI
from oracle import train_kernels_ref as K
from oracle.attention_ref import round16

f32 = np.float32
DT = TI.DTYPES


def ratio(got, ref, tol):
    """max |got - ref| / tol; where tol = 0 the value must be exact; a non-finite value is outside every tolerance."""
    got, ref, tol = (np.asarray(a, np.float64) for a in (got, ref, tol))
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    if (err[tol == 0] != 0).any():
        return float("inf")
    return float(np.max(err[tol > 0] / tol[tol > 0])) if (tol > 0).any() else 0.0


# ---------------------------------------------------------------------------- 1. pins
def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_rmsnorm_bwd_is_autograd_of_the_forward(accumulate):
    rs = np.random.RandomState(1)
    x, w, dy, prior = rs.standard_normal((5, 36)), 1 + 0.2 * rs.standard_normal(36), rs.standard_normal((5, 36)), rs.standard_normal((5, 36))
    eps = float(f32(1e-6))
    tx = _t(x)
    y = torch.from_numpy(w) * tx * torch.rsqrt((tx * tx).mean(1, keepdim=True) + eps)
    (y * torch.from_numpy(dy)).sum().backward()
    got, _, _ = K.rmsnorm_bwd(dy, x, w, 1e-6, prior if accumulate else None)
    np.testing.assert_allclose(got, tx.grad.numpy() + (prior if accumulate else 0.0), rtol=1e-11, atol=1e-13)


def test_fused_rmsnorm_bwd_is_lora_dx_then_the_plain_backward():
    c = TI.rms_fused(TI.RMS_FUSED[1], "f16")
    plain, _, _ = K.rmsnorm_bwd(c.dy2, c.x, c.w, TI.RMS_EPS, c.prior, "f16")
    np.testing.assert_allclose(c.ref, plain, rtol=1e-12, atol=1e-14)


def test_cross_entropy_is_torch_cross_entropy():
    c = TI.ce(TI.CE[4], "f16")                                           # V = 257, label_div 4, labels -100 and V among them
    lab = np.repeat(c.labels, c.div).astype(np.int64)
    lab_t = np.where((lab >= 0) & (lab < c.V), lab, -100)
    lg = _t(c.logits)
    loss = torch.nn.functional.cross_entropy(lg, torch.from_numpy(lab_t), ignore_index=-100, reduction="sum")
    (loss * c.coef).backward()
    np.testing.assert_allclose(c.res.d[:, :c.V], lg.grad.numpy(), rtol=1e-10, atol=1e-12)      # atol: torch's own p - 1 in float64 on the dominated row
    assert (c.res.d[:, c.V:] == 0).all() and (c.res.d[~c.res.ok] == 0).all() and (~c.res.ok).sum() == 8
    np.testing.assert_allclose(c.res.loss, TI.CE_LOSS0 + loss.item(), rtol=1e-12)


def test_gelu_is_torch_exact_erf_gelu():
    c = TI.gelu("f16")
    x = _t(c.x)
    y = torch.nn.functional.gelu(x)
    (y * torch.from_numpy(c.dh.astype(np.float64))).sum().backward()
    np.testing.assert_allclose(c.fwd, y.detach().numpy(), rtol=1e-9, atol=1e-14)       # atol: torch forms 1 + erf, which loses the far negative tail that erfc keeps
    np.testing.assert_allclose(c.bwd, x.grad.numpy(), rtol=1e-9, atol=1e-14)


def test_lora_gradients_are_autograd_of_the_adapter():
    """y = s (mask o x) A^T B^T with 16-bit values of x, A, B and p = 0.5 (the multiplier 2 keeps mask o x exact): dB, dA, du and dx of L = sum dy o y."""
    rs = np.random.RandomState(2)
    T, Kc, N, r, s, p, seed, site = 37, 24, 20, 4, 2.0, 0.5, 99, 7
    x, A, B, dy = (round16(rs.standard_normal(sh), "f16") for sh in ((T, Kc), (r, Kc), (N, r), (T, N)))
    m = K.mask(seed, site, T, Kc, p)
    assert set(np.unique(m)) == {0.0, 2.0}
    tx, tA, tB = _t(x), _t(A), _t(B)
    u = s * (tx * torch.from_numpy(m)) @ tA.T
    u.retain_grad()
    ((u @ tB.T) * torch.from_numpy(dy)).sum().backward()
    un = u.detach().numpy()
    np.testing.assert_allclose(K.lora_down(x, [A.astype(f32)], r, s, p, seed, site, "f16")[0], un, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(K.lora_dB(dy, un, np.zeros((N, r)))[0], tB.grad.numpy(), rtol=1e-12, atol=1e-13)
    du = K.lora_du(dy, B.astype(f32), s, "f16")[0]
    np.testing.assert_allclose(du, u.grad.numpy() * s, rtol=1e-12, atol=1e-13)          # du carries the scale: it is d L / d (xs A^T)
    np.testing.assert_allclose(K.lora_dA(du, x, np.zeros((r, Kc)), p, seed, site, "f16")[0], tA.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(K.lora_dx(np.zeros((T, Kc)), [du], [A], r, p, seed, site)[0], tx.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_adamw_is_torch_adamw_over_three_steps():
    c = TI.opt(257)
    h = TI.ADAM
    p = torch.from_numpy(c.p.astype(np.float64)).requires_grad_(True)
    o = torch.optim.AdamW([p], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    o.state[p] = dict(step=torch.tensor(0.0), exp_avg=torch.from_numpy(c.m.astype(np.float64)), exp_avg_sq=torch.from_numpy(c.v.astype(np.float64)))
    st = (c.p, c.m, c.v)
    for step in (1, 2, 3):
        p.grad = torch.from_numpy(c.g[step - 1].astype(np.float64) * h["inv_scale"])
        o.step()
        r = K.adamw(*st[:1], c.g[step - 1], *st[1:], h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["inv_scale"], step)
        st = (r.p, r.m, r.v)
    np.testing.assert_allclose(st[0], p.detach().numpy(), rtol=1e-6, atol=2e-7)          # the reference takes the hyperparameters and 1 - beta^t as f32:
    np.testing.assert_allclose(st[1], o.state[p]["exp_avg"].numpy(), rtol=1e-6, atol=5e-7)      # 1 - 0.9f and 1 - 0.95f are 2.4e-7 off, relative


def test_grad_stats_rule():
    s, tol = K.grad_stats(np.array([3.0, 4.0], f32), 0.5, np.array([1.0, 7.0]))
    assert s[0] == 1.0 + 6.25 and s[1] == 7.0 and tol > 0
    assert K.grad_stats(np.array([1.0, np.inf], f32), 1.0, np.array([0.0, 7.0]))[0][1] == 1.0
    assert K.grad_stats(np.array([np.nan], f32), 1.0, np.array([0.0, 7.0]))[0][1] == 1.0
    assert K.grad_stats(np.array([3e38], f32), 2.0, np.array([0.0, 0.0]))[0][1] == 1.0          # the SCALED value overflows
    assert K.grad_stats(np.array([3.2e38], f32), 1.0, np.array([0.0, 7.0]))[0][1] == 1.0        # finite, but beyond the kernel's 3.0e38f threshold
    assert K.grad_stats(np.array([2.9e38], f32), 1.0, np.array([0.0, 7.0]))[0][1] == 7.0


def test_du_splits_take_the_paths_the_cases_name():
    assert [TI.lora_du(c, "f16").slices[1] for c in TI.LORA_DU[:5]] == [1, 1, 1, 2, 5]
    assert K.du_splits(129, 1040) == (13, 5) and K.du_splits(127, 272) == (9, 2)


# ---------------------------------------------------------------------------- 2. emulations of the kernels' roundings
def _mm(a, b):
    return np.matmul(a.astype(f32), b.astype(f32))


def emu_lora_down(c):
    out = np.zeros((c.T, c.n * c.r))
    steps = c.K // 16
    per = (steps + 3) // 4
    for seg in range(c.n):
        A16 = round16(c.A[seg], c.dtype)
        xs = K.dropped(c.x, K.mask(TI.SEED, c.site + seg, c.T, c.K, c.p), c.dtype) if c.p > 0 else c.x
        tot = np.zeros((c.T, c.r), f32)
        for w in range(4):
            sl = slice(16 * w * per, 16 * min(steps, (w + 1) * per))
            tot = tot + _mm(xs[:, sl], A16[:, sl].T)
        out[:, seg * c.r:(seg + 1) * c.r] = round16(f32(TI.SCALE) * tot, c.dtype)
    return out


def emu_dB(c):
    out = c.dB0.astype(f32)
    for t0 in range(0, c.T, K.TSPLIT):
        out = out + _mm(c.dy[t0:t0 + K.TSPLIT].T, c.u[t0:t0 + K.TSPLIT])
    return out


def emu_dA(c):
    xs = K.dropped(c.x, K.mask(TI.SEED, c.site, c.T, c.K, c.p), c.dtype) if c.p > 0 else c.x
    hi, lo = K.split_hilo(c.du, c.dtype)
    out = c.dA0.astype(f32)
    for t0 in range(0, c.T, K.TSPLIT):
        sl = slice(t0, t0 + K.TSPLIT)
        out = out + (f32(256.0) * _mm(hi[sl].T, xs[sl]) + _mm(lo[sl].T, xs[sl]))
    return out


def emu_du(c):
    per, ns = c.slices
    B16 = np.zeros((c.Np, c.r))
    B16[:c.N] = round16(c.B, c.dtype)
    out = np.zeros((c.T, c.r), f32)
    for s in range(ns):
        sl = slice(16 * s * per, 16 * min(c.Np // 16, (s + 1) * per))
        out = out + f32(TI.SCALE) * _mm(c.dy[:, sl], B16[sl])
    return out


def _emu_dx_term(du, A, r, p, site, T, Kc):
    l = np.zeros((T, Kc), f32)
    for seg in range(len(A)):
        acc = np.zeros((T, Kc), f32)
        for j in range(r):
            acc = acc + du[seg][:, j:j + 1].astype(f32) * A[seg][j:j + 1].astype(f32)
        if p > 0:
            acc = acc * K.mask(TI.SEED, site + seg, T, Kc, p).astype(f32)
        l = l + acc
    return l


def emu_dx(c):
    o = c.dx0.astype(f32) + _emu_dx_term(c.du, c.A, c.r, c.p, c.site, c.T, c.K)
    return o, round16(o, c.dtype)


def emu_rms(dy, x, w, prior, dtype, l=None):
    x, w, d = x.astype(f32), w.astype(f32), dy.astype(f32)
    H = f32(x.shape[1])
    if l is not None:
        d = d + l
    ss = (x * x).sum(1, keepdims=True, dtype=f32)
    dot = (w * d * x).sum(1, keepdims=True, dtype=f32)
    rs = (f32(1.0) / np.sqrt((ss / H + f32(TI.RMS_EPS)).astype(f32))).astype(f32)
    cc = (rs * rs * rs * dot / H).astype(f32)
    g = (rs * w * d - x * cc).astype(f32)
    if prior is not None:
        g = g + prior.astype(f32)
    return g, round16(g, dtype)


def emu_ce(c):
    lg = c.logits.astype(f32)
    lab = np.repeat(c.labels, c.div)
    ok = (lab >= 0) & (lab < c.V)
    a = lg - lg.max(1, keepdims=True)
    e = np.exp(a).astype(f32)                                            # the native exponential modelled as f32
    s = e.sum(1, keepdims=True, dtype=f32)
    onehot = np.zeros_like(lg)
    onehot[np.arange(c.R)[ok], lab[ok]] = 1
    d = np.zeros((c.R, c.ldd), f32)
    d[:, :c.V] = np.where(ok[:, None], f32(c.coef) * (e * (f32(1.0) / s) - onehot), f32(0))
    row = np.where(ok, -(a[np.arange(c.R), np.where(ok, lab, 0)] - np.log(s[:, 0]).astype(f32)), f32(0)).astype(f32)
    return (round16(d, c.dtype) if c.form == "dl16" else d), f32(TI.CE_LOSS0) + row.sum(dtype=f32)


def emu_gelu(c):
    x = torch.from_numpy(c.x.astype(f32))
    cdf = 0.5 * (1.0 + torch.erf(x * f32(0.70710678118654752)))
    fwd = (x * cdf).numpy()
    bwd = (torch.from_numpy(c.dh) * (cdf + x * f32(0.3989422804014327) * torch.exp(-0.5 * x * x))).numpy()
    return round16(fwd, c.dtype), round16(bwd, c.dtype)


def emu_adamw(p, g, m, v, step):
    h = {k: f32(x) for k, x in TI.ADAM.items()}
    c1, c2 = (f32(x) for x in K.bias_corrections(h["b1"], h["b2"], step))
    one = f32(1.0)
    gr = g * h["inv_scale"]
    pv = p * (one - h["lr"] * h["wd"])
    mv = h["b1"] * m + (one - h["b1"]) * gr
    vv = h["b2"] * v + (one - h["b2"]) * gr * gr
    return pv - (h["lr"] / c1) * mv / (np.sqrt(vv) / np.sqrt(c2) + h["eps"]), mv, vv


@pytest.mark.parametrize("dtype", DT)
def test_emulated_kernels_stay_inside_the_tolerance_on_the_gpu_inputs(dtype):
    worst = {}

    def note(name, x):
        worst[name] = max(worst.get(name, 0.0), x)

    for case in TI.LORA_DOWN:
        c = TI.lora_down(case, dtype)
        note("lora_down", ratio(emu_lora_down(c), c.ref, c.tol))
    for case in TI.LORA_DB:
        c = TI.lora_dB(case, dtype)
        note("dB", ratio(emu_dB(c), c.ref, c.tol))
    for case in TI.LORA_DA:
        c = TI.lora_dA(case, dtype)
        note("dA_" + c.family, ratio(emu_dA(c), c.ref, c.tol))
    for case in TI.LORA_DU:
        c = TI.lora_du(case, dtype)
        note("du", ratio(emu_du(c), c.ref, c.tol))
    for case in TI.LORA_DX:
        c = TI.lora_dx(case, dtype)
        o32, o16 = emu_dx(c)
        note("dx", max(ratio(o32, c.ref, c.tol), ratio(o16, c.ref, c.tol16)))
    for case in TI.RMS_PLAIN:
        c = TI.rms_plain(case, dtype)
        g, g16 = emu_rms(c.dy, c.x[c.rows], c.w, c.prior[c.rows] if "acc" in c.flags else None, dtype)
        note("rms_" + c.family, max(ratio(g, c.ref, c.tol), ratio(g16, c.ref, c.tol16)))
    for case in TI.RMS_FUSED:
        c = TI.rms_fused(case, dtype)
        g, g16 = emu_rms(c.dy, c.x, c.w, c.prior if "acc" in c.flags else None, dtype, _emu_dx_term(c.du, c.A, c.r, c.p, c.site, c.n, c.H))
        note("rmsf_" + c.family, max(ratio(g, c.ref, c.tol), ratio(g16, c.ref, c.tol16)))
    for case in TI.CE:
        c = TI.ce(case, dtype)
        d, loss = emu_ce(c)
        note("ce_d", ratio(d, c.res.d, c.res.tol_d16 if c.form == "dl16" else c.res.tol_d))
        note("ce_loss", abs(float(loss) - c.res.loss) / c.res.tol_loss)
    c = TI.gelu(dtype)
    fwd, bwd = emu_gelu(c)
    note("gelu_fwd", ratio(fwd, c.fwd, c.tol_fwd))
    note("gelu_bwd", ratio(bwd, c.bwd, c.tol_bwd))
    for n in TI.OPT_N:
        c = TI.opt(n)
        st = (c.p, c.m, c.v)
        for step in (1, 2, 3):
            h = TI.ADAM
            r = K.adamw(st[0], c.g[step - 1], st[1], st[2], h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["inv_scale"], step)
            st = emu_adamw(st[0], c.g[step - 1], st[1], st[2], step)                 # the next step starts from the emulated (f32) state, as on the GPU
            note("adamw", max(ratio(st[0], r.p, r.tol_p), ratio(st[1], r.m, r.tol_m), ratio(st[2], r.v, r.tol_v)))
        s, tol = K.grad_stats(c.g[0], TI.ADAM["inv_scale"], [2.5, 7.0])
        got = f32(2.5) + ((c.g[0] * f32(TI.ADAM["inv_scale"])) ** 2).sum(dtype=f32)
        note("grad_stats", abs(float(got) - s[0]) / tol)
    for name, x in sorted(worst.items()):
        print(f"TRAIN_KERNEL_EMU dtype={dtype} kernel={name} worst_ratio={x:.4g}")
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------- 3. the wrong rules leave the tolerance
def _rule_figures(rule, dtype):
    """[(case label, ratio)] of `rule` over every GPU case it can change."""
    out = []
    if rule in ("A_unrounded", "kslice_skipped", "mask_site_plus1", "mask_ldx"):
        for case in TI.LORA_DOWN:
            c = TI.lora_down(case, dtype)
            if (rule == "mask_site_plus1" and (c.n < 2 or c.p == 0)) or (rule == "mask_ldx" and c.p == 0):
                continue
            wrong, _ = K.lora_down(c.x, c.A, c.r, TI.SCALE, c.p, TI.SEED, c.site, dtype, ldx=c.ldx, rule=rule)
            out.append((f"down{case}", ratio(round16(wrong, dtype), c.ref, c.tol)))
    if rule in ("lo_dropped", "dA_not_transposed", "tsplit_skipped", "mask_site_plus1", "mask_ldx"):
        for case in TI.LORA_DA:
            c = TI.lora_dA(case, dtype)
            if (rule in ("mask_site_plus1", "mask_ldx") and c.p == 0) or (rule == "tsplit_skipped" and c.T <= K.TSPLIT):
                continue
            wrong, _ = K.lora_dA(c.du, c.x, c.dA0, c.p, TI.SEED, c.site, dtype, ldx=c.ldx, rule=rule)
            out.append((f"dA{case}", ratio(wrong, c.ref, c.tol)))
    if rule == "tsplit_skipped":
        for case in TI.LORA_DB:
            c = TI.lora_dB(case, dtype)
            if c.T > K.TSPLIT:
                out.append((f"dB{case}", ratio(K.lora_dB(c.dy, c.u, c.dB0, rule=rule)[0], c.ref, c.tol)))
    if rule == "du_accumulated":
        for case in TI.LORA_DU:
            c = TI.lora_du(case, dtype)
            out.append((f"du{case}", ratio(K.lora_du(c.dy, c.B, TI.SCALE, dtype, du0=np.full((c.T, c.r), np.nan), rule=rule)[0], c.ref, c.tol)))
    if rule == "mask_site_plus1":
        for case in TI.LORA_DX:
            c = TI.lora_dx(case, dtype)
            if c.n >= 2 and c.p > 0:
                out.append((f"dx{case}", ratio(K.lora_dx(c.dx0, c.du, c.A, c.r, c.p, TI.SEED, c.site, rule=rule)[0], c.ref, c.tol)))
    if rule in ("c_no_H", "rs2", "accumulate_ignored", "mask_site_plus1"):
        if rule != "mask_site_plus1":
            for case in TI.RMS_PLAIN:
                c = TI.rms_plain(case, dtype)
                if rule == "accumulate_ignored" and "acc" not in c.flags:
                    continue
                wrong = K.rmsnorm_bwd(c.dy, c.x[c.rows], c.w, TI.RMS_EPS, c.prior[c.rows] if "acc" in c.flags else None, rule=rule)[0]
                out.append((f"rms{case}", ratio(wrong, c.ref, c.tol)))
        for case in TI.RMS_FUSED:
            c = TI.rms_fused(case, dtype)
            if (rule == "accumulate_ignored" and "acc" not in c.flags) or (rule == "mask_site_plus1" and (c.na < 2 or c.p == 0)):
                continue
            wrong = K.rmsnorm_bwd(c.dy, c.x, c.w, TI.RMS_EPS, c.prior if "acc" in c.flags else None, lora=(c.du, c.A, c.r, c.p, TI.SEED, c.site), rule=rule)[0]
            out.append((f"rmsf{case}", ratio(wrong, c.ref, c.tol)))
    if rule in ("label_div_ignored", "pad_not_zeroed"):
        for case in TI.CE:
            c = TI.ce(case, dtype)
            if (rule == "label_div_ignored" and c.div == 1) or (rule == "pad_not_zeroed" and c.ldd == c.V):
                continue
            wrong = K.ce_fwd_bwd(c.logits, c.labels, c.div, c.coef, c.ldd, TI.CE_LOSS0, pad=np.nan, rule=rule).d
            out.append((f"ce{case}", ratio(wrong, c.res.d, c.res.tol_d16 if c.form == "dl16" else c.res.tol_d)))
    return out


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rule", K.RULES)
def test_every_wrong_rule_leaves_the_tolerance_on_the_gpu_inputs(rule, dtype):
    figs = _rule_figures(rule, dtype)
    assert figs, rule
    shown = [x for _, x in figs if x > 1.0]
    for label, x in figs:
        print(f"TRAIN_KERNEL_RULE rule={rule} dtype={dtype} case={label} ratio={x:.4g}")
    print(f"TRAIN_KERNEL_RULE rule={rule} dtype={dtype} cases={len(figs)} shown_on={len(shown)} least={min(x for _, x in figs):.4g} worst={max(x for _, x in figs):.4g}")
    # the rule must leave the tolerance on the input set of EVERY kernel it can change (a single case may hide it: one element, or a long sum whose f32 term is wider)
    for kernel in sorted({label.split("(")[0] for label, _ in figs}):
        assert max(x for label, x in figs if label.split("(")[0] == kernel) > 1.0, (rule, dtype, kernel, figs)
