"""CPU: the float64 attention reference the GPU tests of the attention kernel compare with (oracle/attention_ref.py) -- pinned to the oracle's decoder layer, checked
against a dense additive-mask formulation, and shown to tell every deliberately wrong rule from the right one on the very inputs the GPU tests use."""
import numpy as np
import pytest

import attention_inputs as AI
from blim_amd import synth
from oracle import attention_ref as R
from oracle import blim_oracle as O
from oracle.gen_golden import CASES


@pytest.mark.parametrize("which", ["plain", "cpn"])
def test_reference_reproduces_the_oracle_layer_on_tiny(which):
    """parts["attn"] of O.decoder_layer (pinned to the reference project's goldens by tests/test_oracle_golden.py) from the oracle's own q / k / v, one sequence per
    batch row, under the plain key mask and under the CPN mask."""
    spec = CASES["tiny"]
    dims = synth.ModelDims(**spec["dims"])
    w = synth.synthetic_weights(dims, spec["wseed"])
    prob = synth.make_problem(spec["pseed"], spec["n"], dims, tok_per_clip=spec["tok_per_clip"], text_len=spec["text_len"])
    ocfg = O.OracleConfig(**spec["dims"])
    om = O.OracleModel(ocfg, w); om.set_tvg_prefix_length(prob.tvg_prefix_length)
    ids = O.padding_ids(prob.tvg_ids, prob.tvg_labels, prob.tvg_masks, synth.PAD_ID)
    sel = [0, 1, 2]
    mask, cpn, emb, _ = om.prepare_inputs_labels_for_multimodal(ids[0][sel], ids[2][sel], ids[1][sel], [prob.video[i] for i in sel], tvg=True)
    mm = mask if which == "plain" else cpn
    assert which == "plain" or (cpn != mask).any()
    B, L, _ = emb.shape
    parts = {}
    cos, sin = O.rope_tables(ocfg.head_dim, ocfg.rope_theta, L)
    om.decoder_layer(0, emb, O.additive_mask(mm, L), cos, sin, parts)
    nh, nkv, hd = ocfg.num_heads, ocfg.num_kv_heads, ocfg.head_dim
    q, k, v = (parts[n].reshape(B * L, -1, hd) for n in ("q", "k", "v"))
    out, _, _, _ = R.packed_attention(q, k, v, mm.reshape(-1), np.arange(B) * L, np.full(B, L), np.zeros(B, int), np.zeros(B, int), hd ** -0.5)
    want = parts["attn"].reshape(B * L, nh, hd)
    live = (mm.astype(bool).cumsum(axis=1) > 0).reshape(-1)                      # rows with a visible key (the oracle averages V uniformly over the others)
    assert live.sum() > 0.5 * B * L
    assert np.abs(out[live] - want[live]).max() <= 1e-6 * np.abs(want[live]).max()


def dense_formulation(b, f):
    """The same rule as one [T, T'] additive mask per sequence over the GATHERED keys -- written with explicit loops over queries, independently of the reference."""
    T, nh, nkv = b.T, f.nh, f.nkv
    G = nh // nkv
    out = np.zeros((T, nh, AI.D))
    for s in range(len(b.seq_start)):
        s0, n, p0, pn = b.seq_start[s], b.seq_len[s], b.pfx_start[s], b.pfx_len[s]
        keys = list(range(p0, p0 + pn)) + list(range(s0, s0 + n))
        add = np.full((n, len(keys)), -np.inf)
        for i in range(n):
            lo = 0 if b.own_start is None else b.own_start[s0 + i]
            for c, t in enumerate(keys):
                own_ok = c < pn or (lo <= c - pn <= i)
                if own_ok and b.key_visible[t]:
                    add[i, c] = 0.0
        for h in range(nh):
            sc = AI.SCALE * f.q[s0:s0 + n, h] @ f.k[keys, h // G].T + add
            m = sc.max(axis=1, keepdims=True)
            p = np.exp(sc - np.where(np.isfinite(m), m, 0.0))
            l = p.sum(axis=1, keepdims=True)
            out[s0:s0 + n, h] = (p / np.where(l > 0, l, 1.0)) @ f.v[keys, h // G]
    return out


@pytest.mark.parametrize("batch,family", [("masks", "gauss"), ("seg_ragged", "prev"), ("cache", "self")])
def test_reference_agrees_with_a_dense_additive_mask(batch, family):
    b, f, (ref, A, lse, _) = AI.problem(batch, family, 4, 2, "f16")
    want = dense_formulation(b, f)
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (ref[~b.owned] == 0).all() and (A >= np.abs(ref) - 1e-12).all()
    empty = b.owned & (np.abs(A).max(axis=(1, 2)) == 0)
    assert (lse[empty] == R.EMPTY_LSE).all() and (lse[b.owned & ~empty] < 1e3).all()
    if batch == "masks":
        assert empty.sum() == 5 + 36                                                 # batch_masks: 5 queries of E and 36 of F see no key


def test_round16_matches_the_formats():
    import torch
    x = np.random.RandomState(0).randn(4096) * np.exp(np.random.RandomState(1).randn(4096) * 4)
    for dtype, tdt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        want = torch.from_numpy(x).to(torch.float32).to(tdt).to(torch.float64).numpy()
        got = R.round16(x.astype(np.float32), dtype)
        assert np.array_equal(got, want)
        assert np.array_equal(R.from_bits16(R.bits16(got, dtype), dtype), got)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("rule,batch,family", AI.SENSITIVITY)
def test_wrong_rules_leave_the_tolerance(rule, batch, family, dtype):
    """The sensitivity condition of the GPU tests: on their inputs, the result of a wrong rule differs from the reference by more than 10 tol in at least one element
    on >= 90 % of the rows whose visible set the rule changes -- a kernel that implemented the wrong rule could not pass."""
    b, f, (ref, A, _, sub) = AI.problem(batch, family, 2, 1, dtype)
    wrong, _, _, _, sig_w = AI.reference(b, f, rule=rule, return_sig=True)
    sig = AI.reference(b, f, return_sig=True)[4]
    changed = (sig != sig_w) & b.owned
    assert changed.sum() >= 50
    hit = (np.abs(wrong - ref) > 10 * R.tolerance(ref, A, dtype, sub=sub)).any(axis=(1, 2))
    assert hit[changed].mean() >= 0.9, (rule, hit[changed].mean())


def test_the_two_scales_round_the_empty_row_exponent_either_way():
    """A row without a visible key: fma(-1e30, c, -fp32(-1e30 c)) is the product's rounding error.  Negative at SCALE (exp2 -> 0 with or without the kernel's select
    on the reference maximum), positive at SCALE_UP (exp2 -> inf without it): the mask test's second scale is the one that needs the select."""
    def residual(scale):
        c = np.float32(np.float32(scale) * np.float32(1.4426950408889634))
        return float(np.float32(-1.0e30)) * float(c) - float(np.float32(-1.0e30) * c)          # the float64 product of two fp32 values is exact
    assert residual(AI.SCALE) < -1e20 and residual(AI.SCALE_UP) > 1e20


def test_every_wrong_rule_is_covered():
    assert {r for r, _, _ in AI.SENSITIVITY} == set(R.RULES)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_kernel_emulation_against_the_brackets(dtype):
    """What the tolerance constants rest on, from a numpy emulation of the kernel's arithmetic (tile order, lazy maximum, 16-bit P, fp32 sums) on the moderate family:
    the plain form stays at or below 0.82 of the c = 1 bracket, the compensated form at or below 0.0011 of it (14 times under the 1/64 threshold), and a compensated
    kernel that lost any one of its five first-order terms (K_lo.Q_hi, K_hi.Q_lo, V_lo.P, V.P_lo, the lo output) would be at least four times beyond the threshold."""
    rs = np.random.RandomState(3)
    n, nk = 48, 160
    x = {name: rs.randn(nk if name != "q" else n, AI.D) for name in ("q", "k", "v")}
    hi = {a: R.round16(x[a], dtype) for a in x}
    lo = {a: R.round16(x[a] - hi[a], dtype) for a in x}
    see = np.ones((n, nk), bool)
    see[:, rs.rand(nk) < 0.1] = False

    def exact(q, k, v):
        sc = np.where(see, AI.SCALE * q @ k.T, -np.inf)
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        return p @ v, p @ np.abs(v)

    ref, A = exact(hi["q"], hi["k"], hi["v"])
    plain = R.emulate_kernel(hi["q"], hi["k"], hi["v"], see, AI.SCALE, dtype)
    bracket = R.tolerance(ref, A, dtype) / 2
    r_plain = np.max(np.abs(R.round16(plain, dtype) - ref) / bracket)
    full = {a: hi[a] + lo[a] for a in x}
    ref2, A2 = exact(full["q"], full["k"], full["v"])
    bracket2 = R.tolerance(ref2, A2, dtype) / 2
    comp = R.emulate_kernel(hi["q"], hi["k"], hi["v"], see, AI.SCALE, dtype, q_lo=lo["q"], k_lo=lo["k"], v_lo=lo["v"])
    r_comp = np.max(np.abs(comp - ref2) / bracket2)                                    # (the hi + lo output carries the fp32 value to ~2^-20)
    zq, zk = np.zeros_like(lo["q"]), np.zeros_like(lo["k"])
    lost = {"K_lo.Q_hi": dict(q_lo=lo["q"], k_lo=zk, v_lo=lo["v"]), "K_hi.Q_lo": dict(q_lo=zq, k_lo=lo["k"], v_lo=lo["v"]),
            "V_lo.P": dict(q_lo=lo["q"], k_lo=lo["k"], v_lo=zk), "V.P_lo": dict(q_lo=lo["q"], k_lo=lo["k"], v_lo=lo["v"], keep_p_lo=False)}
    r_lost = {name: np.max(np.abs(R.emulate_kernel(hi["q"], hi["k"], hi["v"], see, AI.SCALE, dtype, **kw) - ref2) / bracket2) for name, kw in lost.items()}
    r_lost["lo output"] = np.max(np.abs(R.round16(comp, dtype) - ref2) / bracket2)
    print(f"ATTN_EMULATION dtype={dtype} plain={r_plain:.4f} compensated={r_comp:.5f} " + " ".join(f"without[{n}]={x:.4f}" for n, x in r_lost.items()))
    assert r_plain <= 0.82
    assert r_comp <= 0.0011
    for name, x in r_lost.items():
        assert x >= 4 / 64, (name, x)
