"""CPU: the float64 reference of the trainer's attention backward and of the RoPE backward (oracle/attention_bwd_ref.py) -- what tests/test_attention_bwd_gpu.py
compares the kernels with -- pinned without any GPU result:

  * packed_attention_bwd against central finite differences of oracle/attention_ref.packed_attention and against torch.autograd on a float64 restatement
    (a GQA case and a masked case each);
  * rope_bwd_ref as the adjoint of the RoPE that oracle/gemm_ref.epi_qkv states: <rope(x), y> = <x, rope_bwd(y)>, pass-through beyond rope_cols, clamped positions;
  * the tolerance: a numpy emulation of the kernel's roundings lands inside it on every input the GPU tests use, and leaves it on at least one of them when one
    of the terms P_round, D_o16, P_sub, dS_sub is dropped (P_sub on the `sink` family, where a key's dV is a sum of subnormal P alone).  dS_round cannot show
    that way: in dQ and dK the rounding of P enters through the same sum eps |dS| as the rounding of dS, and the overall factor 2 covers either of the two
    alone.  f32 and lse_f32 are below 1 % of the bound on these inputs and are not shown to be needed;
  * the wrong rules: on the inputs of SENSITIVITY (all GPU inputs) each lands beyond 10 tol on at least 90 % of the elements it can move at all, in fp16 and in bf16."""
import numpy as np
import pytest
import torch

import attention_bwd_inputs as AI
from oracle import attention_bwd_ref as B
from oracle import attention_ref as R


def _small(masked, nh, nkv, seed, D=16):
    rs = np.random.RandomState(seed)
    b = AI._pack([7, 1, 12, 5])
    if masked:
        b.key_visible[b.seq_start[0]:b.seq_start[0] + 3] = 0        # left padding
        b.key_visible[b.seq_start[2] + np.array([4, 11])] = 0       # the middle and position L - 1
        b.key_visible[b.seq_start[3]:b.seq_start[3] + 5] = 0        # nothing visible
    q, k, v, dout = rs.randn(b.T, nh, D), rs.randn(b.T, nkv, D), rs.randn(b.T, nkv, D), rs.randn(b.T, nh, D)
    return b, q, k, v, dout, D ** -0.5


def _loss(b, q, k, v, dout, scale):
    z = np.zeros(len(b.seq_start), np.int32)
    return float((R.packed_attention(q, k, v, b.key_visible, b.seq_start, b.seq_len, z, z, scale)[0] * dout).sum())


@pytest.mark.parametrize("masked,nh,nkv", [(False, 4, 2), (True, 2, 2), (True, 6, 2), (False, 7, 1)])
def test_reference_matches_central_finite_differences(masked, nh, nkv):
    b, q, k, v, dout, scale = _small(masked, nh, nkv, seed=nh + 10 * masked)
    r = B.packed_attention_bwd(q, k, v, dout, b.key_visible, b.seq_start, b.seq_len, scale)
    rs = np.random.RandomState(1)
    h = 1e-5
    for name, x, g in (("q", q, r.dq), ("k", k, r.dk), ("v", v, r.dv)):
        worst = 0.0
        for _ in range(60):
            idx = tuple(rs.randint(n) for n in x.shape)
            keep = x[idx]
            x[idx] = keep + h
            up = _loss(b, q, k, v, dout, scale)
            x[idx] = keep - h
            dn = _loss(b, q, k, v, dout, scale)
            x[idx] = keep
            worst = max(worst, abs((up - dn) / (2 * h) - g[idx]))
        # central differences: h^2 / 6 f''' + the loss's own rounding 2^-52 |loss| / h -- some 1e-9 here
        assert worst <= 1e-7 * max(1.0, float(np.abs(g).max())), (name, worst)
    assert (r.dq[~b.owned] == 0).all() and (r.dk[~b.owned] == 0).all() and (r.dv[~b.owned] == 0).all()
    if masked:
        s0 = b.seq_start[3]
        assert (r.dq[s0:s0 + 5] == 0).all() and (r.dk[s0:s0 + 5] == 0).all() and (r.dv[s0:s0 + 5] == 0).all()       # rows without a visible key


@pytest.mark.parametrize("masked,nh,nkv", [(False, 4, 2), (True, 6, 2), (True, 7, 1)])
def test_reference_matches_autograd_on_a_float64_restatement(masked, nh, nkv):
    b, q, k, v, dout, scale = _small(masked, nh, nkv, seed=3 + nh)
    r = B.packed_attention_bwd(q, k, v, dout, b.key_visible, b.seq_start, b.seq_len, scale)
    tq, tk, tv = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    G = nh // nkv
    loss = torch.zeros((), dtype=torch.float64)
    for s0, n in zip(b.seq_start, b.seq_len):
        s0, n = int(s0), int(n)
        see = torch.tril(torch.ones(n, n, dtype=torch.bool)) & torch.tensor(b.key_visible[s0:s0 + n] != 0)[None, :]
        for h in range(nh):
            sc = scale * tq[s0:s0 + n, h] @ tk[s0:s0 + n, h // G].T
            rows = see.any(dim=1)
            p = torch.softmax(sc.masked_fill(~see, float("-inf"))[rows], dim=-1)
            loss = loss + (p @ tv[s0:s0 + n, h // G] * torch.tensor(dout[s0:s0 + n, h])[rows]).sum()
    loss.backward()
    for name, t, g in (("q", tq, r.dq), ("k", tk, r.dk), ("v", tv, r.dv)):
        got = t.grad.numpy() if t.grad is not None else np.zeros_like(g)
        assert np.abs(got - g).max() <= 1e-12 * max(1.0, float(np.abs(g).max())), name


@pytest.mark.parametrize("nh,nkv", AI.GQA)
def test_rope_bwd_is_the_adjoint_of_the_qkv_epilogue_rope(nh, nkv):
    rs = np.random.RandomState(nh)
    T, n_pos, qn = 37, 50, (nh + 2 * nkv) * 128
    pos = rs.randint(-5, n_pos + 5, T)
    pos[:4] = [0, n_pos - 1, -3, n_pos + 7]
    ang = rs.rand(n_pos, 64) * 6.28
    cos, sin = np.cos(ang), np.sin(ang)
    x, y = rs.randn(T, qn), rs.randn(T, qn)
    pp = B.clamp_positions(pos, n_pos)
    assert pp.min() == 0 and pp.max() == n_pos - 1 and (pp[:4] == [0, n_pos - 1, 0, n_pos - 1]).all()
    fwd = B.rope_fwd(x, cos[pp], sin[pp], nh, nkv)
    bwd, pre = B.rope_bwd_ref(y, (nh + nkv) * 128, pos, cos, sin)
    assert abs((fwd * y).sum() - (x * bwd).sum()) <= 1e-11 * np.abs(fwd * y).sum()
    assert (bwd[:, (nh + nkv) * 128:] == y[:, (nh + nkv) * 128:]).all() and (pre[:, (nh + nkv) * 128:] == 0).all()      # the V columns pass through
    assert not (bwd[:, :(nh + nkv) * 128] == y[:, :(nh + nkv) * 128]).all()
    none, _ = B.rope_bwd_ref(y, 0, pos, cos, sin)
    assert (none == y).all()


def _ratios(b, ref, got):
    out = []
    for g, want, tol in zip(got, (ref.dq, ref.dk, ref.dv), (ref.tol_dq, ref.tol_dk, ref.tol_dv)):
        err, t = np.abs(g - want)[b.owned], tol[b.owned]
        assert (err[t == 0] == 0).all()
        out.append(float((err[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0)
    return out


EMU_CASES = AI.GPU_CASES + [(f"L{L}", "gauss", 4, 2) for L in (1, 33, 129)]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_emulated_kernel_roundings_land_inside_the_tolerance_and_no_term_is_padding(dtype):
    shown = {}
    for case in EMU_CASES:
        b, f, ref = AI.problem(*case, dtype)
        em = AI.emulate(b, f)
        x = _ratios(b, ref, em)
        print("ATTN_BWD_EMU", dtype, case, " ".join(f"{v:.3f}" for v in x))
        assert max(x) <= 1.0, (case, x)
        for term in ("P_round", "D_o16") + (("P_sub", "dS_sub") if dtype == "f16" else ()):
            if not shown.get(term):
                shown[term] = max(_ratios(b, AI.reference(b, f, drop=(term,)), em)) > 1.0
    assert all(shown.values()), shown


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("rule,batch,family,nh,nkv", AI.SENSITIVITY)
def test_gpu_inputs_tell_each_wrong_rule_from_the_right_one(rule, batch, family, nh, nkv, dtype):
    assert (batch, family, nh, nkv) in AI.GPU_CASES
    b, f, ref = AI.problem(batch, family, nh, nkv, dtype)
    wrong = AI.reference(b, f, rule=rule)
    masks = B.touched(rule, ref, wrong, b.key_visible, b.owned, b.seq_start, b.seq_len)
    assert any(m.any() for m in masks), "the rule touches nothing on these inputs"
    for name, m in zip(("dq", "dk", "dv"), masks):
        d, tol = np.abs(getattr(wrong, name) - getattr(ref, name)), getattr(ref, "tol_" + name)
        m3 = np.broadcast_to(m[:, :, None], d.shape)
        # outside the mask the rule changes nothing (float64 noise of a differently ordered sum at the most)
        assert (d[~m3] <= 1e-9 * np.maximum(tol[~m3], 1e-30)).all() or (d[~m3] <= 1e-12).all(), (rule, name)
        if m.any():
            frac = float((d > 10 * tol)[m3].mean())
            print("ATTN_BWD_RULE", dtype, rule, name, f"{frac:.3f}")
            assert frac >= 0.9, (rule, name, frac)


def test_every_rule_has_its_sensitivity_case():
    assert {s[0] for s in AI.SENSITIVITY} == set(B.RULES)
