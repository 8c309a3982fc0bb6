"""CPU: the float64 GEMM reference the GPU tests of csrc/gemm.hip compare with (oracle/gemm_ref.py) -- its weight-row layouts pinned to gemm.hpp's words, its qkv and
swiglu epilogues pinned to the oracle's decoder layer, its quantisers to independent statements, and every deliberately wrong rule shown to leave the tolerance on
the very inputs the GPU tests use (beyond 10 tol on at least 90 % of the elements the rule touches, at the smallest shape of the GPU cases)."""
import os
import re

import numpy as np
import pytest

import gemm_inputs as GI
from blim_amd import synth
from oracle import blim_oracle as O
from oracle import gemm_ref as R
from oracle.gen_golden import CASES

HPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "blim_amd", "csrc", "gemm.hpp")
DTYPES = ("f16", "bf16")


# ---------------------------------------------------------------------------- layouts
def test_qkv_row_permutation_is_gemm_hpp_s():
    src = open(HPP).read()
    m = re.search(r"static inline int qkv_perm_row\(int cprime\) \{ return ([^;]+); \}", src)
    assert m, "gemm.hpp no longer states qkv_perm_row"
    c = np.arange(128)
    assert np.array_equal(eval(m.group(1), {"cprime": c}), R.qkv_perm_row(c))        # the C expression uses only + * >> &: the same in Python
    assert "16*(c'>>5) + (c'&15) + 64*((c'>>4)&1)" in src
    p = R.qkv_perm_row(c)
    assert sorted(p) == list(range(128))
    # by hand: 16 rows d = 0..15, then their partners 64..79, then 16..31, 80..95, ...
    assert list(p[:34]) == list(range(0, 16)) + list(range(64, 80)) + [16, 17]
    assert p[48] == 80 and p[127] == 127 and p[96] == 48 and p[112] == 112
    assert all(p[c0 + 16] == p[c0] + 64 for c0 in range(128) if (c0 >> 4) % 2 == 0)     # partners d, d + 64 sit 16 stored rows apart: fragments (2p, 2p + 1) of a lane
    order = R.qkv_row_order(2, 1)                                                     # q0 q1 k0 v0
    assert sorted(order) == list(range(512)) and np.array_equal(order[384:], np.arange(384, 512))          # the v head in natural order
    assert np.array_equal(order[128:256], 128 + p) and np.array_equal(order[256:384], 256 + p)
    inv = R.inverse(order)
    assert np.array_equal(order[inv], np.arange(512)) and np.array_equal(inv[order], np.arange(512))
    assert inv[64] == 16 and inv[128 + 65] == 128 + 17


def test_swiglu_interleave_is_gemm_hpp_s():
    src = open(HPP).read()
    assert "group g = r>>5, t = r&31" in src and "t < 16 -> gate row 16g+t, else up row 16g+(t-16)" in src
    I = 96
    order = R.swiglu_row_order(I)
    for r in range(2 * I):
        g, t = r >> 5, r & 31
        assert order[r] == (16 * g + t if t < 16 else I + 16 * g + (t - 16))
    assert sorted(order) == list(range(2 * I))
    assert list(order[:18]) == list(range(16)) + [I, I + 1] and order[32] == 16 and order[48] == I + 16
    inv = R.inverse(order)
    assert np.array_equal(order[inv], np.arange(2 * I)) and inv[I] == 16 and inv[16] == 32


# ---------------------------------------------------------------------------- the oracle's decoder layer
def test_qkv_and_swiglu_reproduce_the_oracle_layer_on_tiny():
    """parts q / k / v / act of O.decoder_layer from the oracle's own normalised inputs and weights, the weights in the kernel's stored row order."""
    spec = CASES["tiny"]
    dims = synth.ModelDims(**spec["dims"])
    w = synth.synthetic_weights(dims, spec["wseed"])
    prob = synth.make_problem(spec["pseed"], spec["n"], dims, tok_per_clip=spec["tok_per_clip"], text_len=spec["text_len"])
    ocfg = O.OracleConfig(**spec["dims"])
    om = O.OracleModel(ocfg, w); om.set_tvg_prefix_length(prob.tvg_prefix_length)
    ids = O.padding_ids(prob.vtg_ids, prob.vtg_labels, prob.vtg_masks, synth.PAD_ID)
    mask, _, emb, _ = om.prepare_inputs_labels_for_multimodal(ids[0][[0, 1]], ids[2][[0, 1]], ids[1][[0, 1]], [prob.video[0], prob.video[1]])
    B, L, H = emb.shape
    parts = {}
    cos, sin = O.rope_tables(ocfg.head_dim, ocfg.rope_theta, L)
    om.decoder_layer(0, emb, O.additive_mask(mask, L), cos, sin, parts)
    nh, nkv = ocfg.num_heads, ocfg.num_kv_heads
    P = "layers.0."
    w_nat = np.concatenate([w[P + "q_proj.w"], w[P + "k_proj.w"], w[P + "v_proj.w"]]).astype(np.float64)
    b_nat = np.concatenate([w[P + "q_proj.b"], w[P + "k_proj.b"], w[P + "v_proj.b"]]).astype(np.float64)
    order = R.qkv_row_order(nh, nkv)
    x = parts["xn1"].reshape(B * L, H).astype(np.float64)
    acc, A = R.product(x, w_nat[order])
    pos = np.tile(np.arange(L), B)
    got, _ = R.epi_qkv(acc, A, H, b_nat[order], cos[pos][:, :64], sin[pos][:, :64], nh, nkv)
    want = np.concatenate([parts[n].reshape(B * L, -1) for n in ("q", "k", "v")], axis=1)
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()                      # the oracle computes in float32
    h2 = O.rms_norm(parts["resid_mid"], w[P + "post_norm"], ocfg.rms_eps).reshape(B * L, H).astype(np.float64)
    I = ocfg.intermediate_size
    w_gu = np.concatenate([w[P + "gate_proj.w"], w[P + "up_proj.w"]]).astype(np.float64)[R.swiglu_row_order(I)]
    acc, A = R.product(h2, w_gu)
    got, _ = R.epi_swiglu(acc, A, H)
    want = parts["act"].reshape(B * L, I)
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()


# ---------------------------------------------------------------------------- quantisers
def test_e4m3_rules_against_torch_and_by_hand():
    import torch
    g = GI.rng("e4m3")
    x = np.concatenate([g.randn(4000) * 100, g.randn(4000), g.randn(2000) * 0.01, [0.0, 448.0, 464.0, 1000.0, -500.0, 2.0 ** -9, 2.0 ** -10, 17.0, 19.0, 0.0009765625 * 3]])
    want = torch.from_numpy(np.clip(x, -448, 448)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = R.e4m3_encode(x)
    nz = x != 0
    assert np.array_equal(got[nz], want[nz])
    assert np.array_equal(R.e4m3_decode(np.arange(256, dtype=np.uint8))[:127], torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy())
    assert R.e4m3_decode(R.e4m3_encode(17.0)) == 16.0 and R.e4m3_decode(R.e4m3_encode(19.0)) == 20.0             # ties to the even code
    # the block scale: smallest e with amax 2^-e <= 448
    assert list(R.e8m0_exponent(np.array([448.0, 448.0001, 896.0, 897.0, 224.0, 1.0, 0.0, 447.9]))) == [0, 1, 1, 2, -1, -8, 0, 0]
    x = g.randn(5, 256) * np.array([1e-3, 1.0, 30.0, 1e3, 0.0])[:, None]
    q, e, deq = R.quant_e4m3_mx(x)
    amax = np.abs(x).reshape(5, 2, 128).max(axis=2)
    live = amax > 0
    assert (amax[live] * 2.0 ** -e[live] <= 448).all() and (amax[live] * 2.0 ** -(e[live] - 1.0) > 448).all() and (e[~live] == 0).all()
    assert (np.abs(deq - x) <= 0.5 * R.e4m3_ulp(x / np.repeat(2.0 ** e, 128, axis=1)) * np.repeat(2.0 ** e, 128, axis=1) + 1e-300).all()
    # the table index of gemm.hpp: row in tile = 128 wm + 16 mi + fr -> (wm 16 + fr) 8 + mi
    for row, k in ((0, 0), (17, 0), (128 + 16 * 3 + 5, 2), (256 + 255, 1)):
        r = row & 255
        wm, mi, fr = r >> 7, (r >> 4) & 7, r & 15
        assert R.mx_index(row, k, 512) == k * 512 + (row >> 8) * 256 + (wm * 16 + fr) * 8 + mi
    assert len(set(R.mx_index(np.arange(512), 0, 512))) == 512


def _tiles_decode(tiles, n_rows, K, w_side):
    """The operand-tile image of gemm.hpp read back, written from the header's words independently of R.e2m3_tiles (byte-wise loops over lanes)."""
    nt, nk = tiles.shape[:2]
    codes, e8 = np.zeros((nt * 256, K), np.uint8), np.zeros((nt * 256, K // 32), np.uint8)
    for t in range(nt):
        for k in range(nk):
            blk = tiles[t, k]
            for fb in range(16):
                for lane in range(64):
                    r, g = lane & 15, lane >> 4
                    b24 = np.concatenate([blk[fb * 1536 + lane * 16:fb * 1536 + lane * 16 + 16], blk[fb * 1536 + 1024 + lane * 8:fb * 1536 + 1024 + lane * 8 + 8]])
                    v = int.from_bytes(bytes(b24), "little")
                    codes[t * 256 + fb * 16 + r, k * 128 + 32 * g:k * 128 + 32 * g + 32] = [(v >> (6 * j)) & 63 for j in range(32)]
            for row in range(256):
                for g in range(4):
                    idx = ((row >> 6) * 4 + g) * 64 + (row & 15) * 4 + ((row >> 4) & 3) if w_side else ((row >> 7) * 4 + g) * 128 + (row & 15) * 8 + ((row >> 4) & 7)
                    e8[t * 256 + row, k * 4 + g] = blk[24576 + idx]
    return codes, e8


@pytest.mark.parametrize("w_side", [False, True])
def test_e2m3_tiles_follow_the_header_s_layout(w_side):
    g = GI.rng("e2m3", w_side)
    x = g.randn(300, 256) * np.exp(g.randn(300, 1))
    x[:, 32:64] = 0.0
    x[5, 64:96] = [7.5 * 2.0 ** -3] + [0.0] * 31                     # amax / scale exactly 7.5
    tiles = R.e2m3_tiles(x, w_side)
    assert tiles.shape == (2, 2, R.F6_TILE_BYTES)
    codes, e8 = _tiles_decode(tiles, 300, 256, w_side)
    c, e, val = R.e2m3_quant(x)
    assert np.array_equal(codes[:300], c) and np.array_equal(e8[:300], e) and not codes[300:].any() and not e8[300:].any()
    assert (e[:, 1] == 0).all() and not c[:, 32:64].any() and e[5, 2] == 127 - 3 and c[5, 64] == 31
    blocks = np.abs(x).reshape(300, 8, 32).max(axis=2)
    sc = 2.0 ** (e.astype(np.float64) - 127)
    live = blocks > 0
    assert (blocks[live] / sc[live] <= 7.5).all() and (blocks[live] / sc[live] > 3.75).all()
    assert (np.abs(val - x) <= np.repeat(sc, 32, axis=1) * 0.25 + 1e-300).all()        # the grid's coarsest half step (1/2 above 4) times the scale


def test_split_rule():
    for dtype in DTYPES:
        x = GI.rng("split").randn(4000) * 3.0
        hi, lo = R.split16(x, dtype)
        assert np.array_equal(hi, R.round16(x, dtype)) and (np.abs(lo) <= R.EPS[dtype] * np.abs(hi) * (1 + 2 * R.EPS[dtype])).all()
        assert (np.abs(hi + lo - x) <= R.EPS[dtype] ** 2 * np.abs(x) + R.F16_FLOOR).all()
        assert (np.abs(hi + lo - x) <= 0.5 * R.tolerance(x, 0.0, dtype, split=True)).all()
    assert R.saturate16(np.array([1e6, -1e6, 65520.0, np.nan]), "f16")[:3].tolist() == [65504.0, -65504.0, 65504.0]
    assert np.isinf(R.saturate16(np.array([1e6]), "f16", saturate=False)).all() and np.isnan(R.saturate16(np.array([np.nan]), "f16")).all()


# ---------------------------------------------------------------------------- an f32 evaluation stays inside the tolerance
def test_a_float32_evaluation_in_another_order_is_inside_the_tolerance():
    """Not a proof of the bounds -- a check that they are not too tight: numpy's float32 matmul (its own blocking and order) followed by float32 epilogues."""
    f32 = np.float32
    a, w = GI.moderate(130, 96, 704, "f16")
    acc, A = R.product(a, w)
    acc32 = a.astype(f32) @ w.astype(f32).T
    ref, pre = R.epi_f32(acc, A, 704, 0.37)
    assert (np.abs((acc32 * f32(0.37)).astype(np.float64) - ref) <= R.tolerance(ref, pre, "f32")).all()
    bias, resid = GI.bias_for(96, 704), 1e3 * GI.rng("r").randn(130, 96).astype(f32).astype(np.float64)
    ref, pre = R.epi_resid(acc, A, 704, resid, bias)
    got = resid.astype(f32) + (acc32 + bias.astype(f32)[None, :])
    assert (np.abs(got.astype(np.float64) - ref) <= R.tolerance(ref, pre, "f32")).all()
    a, w = GI.swiglu_problem(130, 64, 128, "f16")
    acc, A = R.product(a, w)
    acc32 = (a.astype(f32) @ w.astype(f32).T).reshape(130, 2, 2, 16)
    gt, up = acc32[:, :, 0].reshape(130, -1), acc32[:, :, 1].reshape(130, -1)
    with np.errstate(over="ignore"):
        got = gt * (f32(1) / (f32(1) + np.exp(-gt))) * up
    ref, pre = R.epi_swiglu(acc, A, 128)
    assert (np.abs(got.astype(np.float64) - ref) <= R.tolerance(ref, pre, "f32")).all()
    assert np.abs(acc.reshape(130, 2, 2, 16)[:, :, 0]).max() > 40                  # the large gates are there


# ---------------------------------------------------------------------------- wrong rules
def beyond(wrong, ref, tol, touched=None, k=10.0):
    """Fraction of the touched elements on which the wrong rule's result is further than k tol from the reference."""
    d = np.abs(np.asarray(wrong, np.float64) - ref)
    t = np.ones(d.shape, bool) if touched is None else np.broadcast_to(touched, d.shape)
    assert t.sum() > 0
    return float((d[t] > k * tol[t]).mean())


def report(rule, dtype, frac):
    print(f"GEMM_RULE rule={rule} dtype={dtype} beyond_10_tol={frac:.4f}")
    assert frac >= 0.9, (rule, dtype, frac)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rule", ["rope_partner32", "rope_sin_sign", "bias_after_rope", "last_k_head_plain", "first_v_head_rotated"])
def test_wrong_qkv_rules_leave_the_tolerance(rule, dtype):
    c = GI.qkv_case(257, 1, 1, 64, dtype)
    wrong, _ = R.epi_qkv(c.acc, c.A, c.K, c.bias, c.cos, c.sin, c.nh, c.nkv, rule=rule)
    tol = R.tolerance(c.ref, c.pre, dtype)
    cols = np.zeros(c.ref.shape[1], bool)
    nh, nkv = c.nh, c.nkv
    if rule == "last_k_head_plain":
        cols[(nh + nkv - 1) * 128:(nh + nkv) * 128] = True
    elif rule == "first_v_head_rotated":
        cols[(nh + nkv) * 128:(nh + nkv + 1) * 128] = True
    else:
        cols[:(nh + nkv) * 128] = True
    touched = cols[None, :] & (c.pos != 0)[:, None]                 # position 0 is the identity rotation
    report(rule, dtype, beyond(wrong, c.ref, tol, touched))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rule", ["gate_up_swapped", "interleave32", "silu_of_up"])
def test_wrong_swiglu_rules_leave_the_tolerance(rule, dtype):
    a, w = GI.swiglu_problem(255, 64, 64, dtype)
    acc, A = R.product(a, w)
    ref, pre = R.epi_swiglu(acc, A, 64)
    wrong, _ = R.epi_swiglu(acc, A, 64, rule=rule)
    report(rule, dtype, beyond(wrong, ref, R.tolerance(ref, pre, dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rule", ["a_lo_dropped", "w_not_wrapped"])
@pytest.mark.parametrize("epi", ["f32", "bf16"])
def test_wrong_wrap_rules_leave_the_tolerance(epi, rule, dtype):
    a, w = GI.wrapped(256, 256, 64, dtype)
    acc, A = R.product(a, w, w_wrap_k=64)
    wacc, wA = R.product(a, w, w_wrap_k=64, rule=rule)
    if epi == "f32":
        (ref, pre), (wrong, _) = R.epi_f32(acc, A, 128), R.epi_f32(wacc, wA, 128)
        tol = R.tolerance(ref, pre, "f32")
    else:
        (ref, pre), (wrong, _) = R.epi_bf16(acc, A, 128), R.epi_bf16(wacc, wA, 128)
        tol = R.tolerance(ref, pre, dtype)
    report(f"{rule}/{epi}", dtype, beyond(wrong, ref, tol))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rule", ["resid_no_bias", "resid_in_ignored", "resid_twice", "scale_ignored"])
def test_wrong_f32_epilogue_rules_leave_the_tolerance(rule, dtype):
    c = GI.resid_case(255, 260, 64, dtype, with_in=True, with_bias=True)
    if rule == "scale_ignored":
        ref, pre = R.epi_f32(c.acc, c.A, c.K, 0.37)
        wrong, _ = R.epi_f32(c.acc, c.A, c.K, 0.37, rule=rule)
    else:
        ref, pre = c.ref, c.pre
        wrong, _ = R.epi_resid(c.acc, c.A, c.K, c.resid, c.bias, rule=rule, c_before=c.c_before)
    report(rule, dtype, beyond(wrong, ref, R.tolerance(ref, pre, "f32")))


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_lse_rules_leave_the_tolerance(dtype):
    M, N, K = 255, 260, 64
    a, w, lab = GI.lse_problem(M, N, K, dtype)
    acc, A = R.product(a, w)
    ref = R.epi_lse(acc, A, K, lab)
    wrong = R.epi_lse(acc, A, K, lab, rule="lse_pad_exp0")
    last = np.zeros(ref["s"].shape, bool)
    last[:, -1] = True                                             # the ragged last tile: 4 valid columns, 252 of padding
    report("lse_pad_exp0", dtype, beyond(wrong["s"], ref["s"], ref["tol_s"], last))
    assert np.array_equal(wrong["s"][:, 0], ref["s"][:, 0])
    wrong = R.epi_lse(acc, A, K, lab, rule="label_next_tile")
    ok = (lab >= 0) & (lab < N)
    assert np.isnan(ref["label"][~ok]).all() and (~ok).sum() >= 4 and ok.sum() > 200
    report("label_next_tile", dtype, beyond(wrong["label"][ok], ref["label"][ok], ref["tol_label"][ok]))
    # the partials give the row's log-sum-exp back, and the special rows are what they claim to be
    assert np.abs(R.lse_combine(ref["m"], ref["s"]) - ref["lse"]).max() < 1e-9
    assert acc[1].max() < -500 and abs(acc[2].max() - 80) < 1e-9 and np.sort(acc[2])[-2] < 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_split_rule_leaves_the_tolerance(dtype):
    a, w = GI.moderate(255, 260, 64, dtype)
    acc, A = R.product(a, w)
    ref, pre = R.epi_bf16(acc, A, 64)
    hi, lo = R.split16(ref, dtype, rule="lo_is_round_x")
    report("lo_is_round_x", dtype, beyond(hi + lo, ref, R.tolerance(ref, pre, dtype, split=True)))
    hi, lo = R.split16(ref, dtype)
    assert (np.abs(hi + lo - ref) <= R.tolerance(ref, pre, dtype, split=True)).all()


def test_wrong_e4m3_scale_is_seen_and_few_rows_sit_on_a_binade_boundary():
    """The fp8 SwiGLU case of the GPU test: a scale one binade too small differs in EVERY scale byte, and the rows whose amax is within the tolerance of a boundary
    (448 2^k: there the kernel's f32 amax may fall on the other side) are at most 2 % of the (row, tile column) blocks."""
    c = GI.f8_swiglu_case(300, 512, 256)
    _, e, _ = R.quant_e4m3_mx(c.ref)
    _, ew, _ = R.quant_e4m3_mx(c.ref, rule="e4m3_scale_small")
    print(f"GEMM_RULE rule=e4m3_scale_small dtype=f8 beyond_10_tol={float((ew != e).mean()):.4f}")
    assert (ew == e - 1).all()
    near = c.near_boundary()
    print(f"GEMM_RULE e8m0 blocks near a binade boundary: {int(near.sum())} of {near.size}")
    assert near.mean() <= 0.02
