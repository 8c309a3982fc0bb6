"""GPU: `--vtg_precise select` -- the engine's per-layer compensation mask (options "precise_layers" / "precise_layer_bits"), the two attention forms it makes
reachable, and the measured mask over a whole 7B evaluation.  The host-side logic is tests/test_vtg_select_host.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import lora_fixture as LF
import test_gpu_parity as P
from blim_amd import checkpoint as CK
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd.modeling import BlimModel, DDPLike

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTG = ("v2t_vtg", "v2t_vtg_cpn", "t2v_vtg")


def _select(model, mask):
    model.vtg_precise = "select"
    model.resolve_vtg("select", np.asarray(mask, dtype=np.uint8))
    model.clear_cache()


def _full(model):
    model.vtg_precise = "full"
    model.clear_cache()


def _vtg_both_paths(t):
    """The VTG passes through the fused PairScorer (the last layer pruned to the scored rows) and the literal forward() (every row)."""
    return {lit: P._six_passes(t, lit, names=VTG) for lit in (False, True)}


@pytest.mark.parametrize("case", ["tiny", "deep"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_all_ones_mask_is_bit_equal_to_full(case, dtype):
    t = P._build(case, device_synth=(case == "deep"), dtype=dtype)
    try:
        _full(t.model)
        ref = _vtg_both_paths(t)
        _select(t.model, np.full(t.dims.num_layers, 15))
        got = _vtg_both_paths(t)
        for lit in ref:
            for k in ref[lit]:
                assert np.array_equal(got[lit][k], ref[lit][k]), (case, dtype, lit, k)
        # the mask is for VTG calls only: the TVG passes under a select request are the fully compensated ones too
        _select(t.model, np.zeros(t.dims.num_layers))
        tv = P._six_passes(t, False, names=P.TVG_PASSES)
        _full(t.model)
        tf = P._six_passes(t, False, names=P.TVG_PASSES)
        for k in tv:
            assert np.array_equal(tv[k], tf[k]), k
    finally:
        t.model.engine.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_all_ones_mask_with_adapters_apart_is_bit_equal_to_full(dtype):
    spec, g, dims, prob = LF.load_case("lora_tiny")
    w, tr = LF.base_weights_host(spec, dims), LF.trainable_of(spec, dims)
    model = BlimModel(dims, max_positions=1024, dtype=dtype)
    try:
        model.engine.load_weights(w)
        for n in CK.expected_adapters(dims):
            model.engine.load_adapter(n, tr[n + ":A"], tr[n + ":B"], LF.R, LF.ALPHA)
        model.set_tvg_prefix_length(prob.tvg_prefix_length)
        t = types.SimpleNamespace(spec=spec, dims=dims, model=model, prob=prob, dtype=dtype, case="lora_tiny")
        _full(model)
        ref = _vtg_both_paths(t)
        _select(model, np.full(dims.num_layers, 15))
        got = _vtg_both_paths(t)
        for lit in ref:
            for k in ref[lit]:
                assert np.array_equal(got[lit][k], ref[lit][k]), (dtype, lit, k)
        # every unit plain, adapters apart: still the reference's scores within the bar
        _select(model, np.zeros(dims.num_layers))
        for lit, res in _vtg_both_paths(t).items():
            for k, v in P._worst_rel(res, g).items():
                assert v < P.SCORE_RTOL, (dtype, lit, k, v)
    finally:
        model.engine.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_all_zero_mask_stays_within_the_bar_of_the_goldens(dtype, capsys):
    t = P._build("tiny", dtype=dtype)
    g = np.load(os.path.join(P.GOLD, "tiny.npz"))
    try:
        _select(t.model, np.zeros(t.dims.num_layers))
        w = {lit: P._worst_rel(r, g) for lit, r in _vtg_both_paths(t).items()}
    finally:
        t.model.engine.close()
    with capsys.disabled():
        print(f"\n[tiny {dtype}, every unit plain] worst relative deviation vs the fp32 reference: {w}")
    for lit, r in w.items():
        for k, v in r.items():
            assert v < P.SCORE_RTOL, (dtype, lit, k, v)


def test_single_unit_flips_on_full7b(capsys):
    """Each class plain in the first and in the last layer alone: the scores move (the unit really runs plain), stay finite and stay inside the bar of the fp32 reference."""
    t = P._build("full7b", device_synth=True, dtype="f16")
    g = np.load(os.path.join(P.GOLD, "full7b.npz"))
    L = t.dims.num_layers
    rows = []
    try:
        _full(t.model)
        ref = P._six_passes(t, False, names=("v2t_vtg",))["v2t_vtg"]
        for li in (0, L - 1):
            for c, name in enumerate("AOGD"):
                mask = np.full(L, 15, np.uint8); mask[li] = 15 & ~(1 << c)
                _select(t.model, mask)
                got = P._six_passes(t, False, names=("v2t_vtg",))
                S = got["v2t_vtg"]
                m = ref != -100.0
                worst = P._worst_rel(got, g)["v2t_vtg"]
                rows.append((f"{name}{li}", float(np.max(np.abs(S[m] - ref[m]) / np.abs(ref[m]))), worst))
                assert np.all(np.isfinite(S[m])), (name, li)
                assert not np.array_equal(S, ref), (name, li)
                assert worst < P.SCORE_RTOL, (name, li, worst)
    finally:
        t.model.engine.close()
    with capsys.disabled():
        print("\n[full7b f16] one unit plain: (unit, max deviation from full, worst vs the fp32 reference) " + ", ".join(f"{u} {a:.1e} {b:.1e}" for u, a, b in rows))


def _attention_of(model, bits):
    """One decoder layer, forward() over one 64-token causal row in precise mode under layer bits `bits`: (qkv [T, 2 qkv_n], attention output [T, 2 H]) workspaces."""
    E = model.engine
    dims = model.dims
    T = 64
    emb = (torch.randn((1, T, dims.hidden_size), generator=torch.Generator().manual_seed(3)) * 0.5).to(model.dtype).cuda()
    m8 = torch.ones((1, T), dtype=torch.uint8, device="cuda")
    E.set_layer_mask(np.array([bits], dtype=np.uint8))
    E.set_precise(True, embeds=False, mlp=True, layers=True)
    try:
        E.forward(emb, m8, want_logits=False, want_hidden=True)
    finally:
        E.set_precise(False)
    qkv_n = (dims.num_heads + 2 * dims.num_kv_heads) * 128
    return E.debug_read("qkv", (T, 2 * qkv_n), model.dtype).float().cpu(), E.debug_read("attn", (T, 2 * dims.hidden_size), model.dtype).float().cpu()


def _exact_attention(q, k, v, nh, nkv):
    """f64 causal GQA attention of the q / k / v rows (q / k columns in the epilogue's head order: the dot products do not depend on it)."""
    T = q.shape[0]
    q = q.double().view(T, nh, 128); k = k.double().view(T, nkv, 128); v = v.double().view(T, nkv, 128)
    out = torch.empty((T, nh, 128), dtype=torch.float64)
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool))
    for h in range(nh):
        kh = h // (nh // nkv)
        s = (q[:, h] @ k[:, kh].T) / np.sqrt(128.0)
        s = s.masked_fill(~causal, -np.inf)
        out[:, h] = torch.softmax(s, dim=-1) @ v[:, kh]
    return out.reshape(T, nh * 128)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_mixed_attention_forms(dtype, capsys):
    """attention.hip's two forms that only the mask reaches.  Plain products + [hi | lo] store (QKV plain, o_proj compensated: bits 14): hi is bit-equal to the plain
    kernel's output (bits 12), lo is the residual of the f32 output (|lo| <= half a 16-bit step of hi) and hi + lo is nearer the exact attention of the same inputs than
    hi alone.  Split products + hi-only store (QKV compensated, o_proj plain: bits 13): bit-equal to the hi half of the whole-call compensated form (bits 15), within one
    16-bit rounding of the exact attention of the hi + lo inputs."""
    t = P._build("tiny", layers=1, dtype=dtype)
    d = t.dims
    H, nh, nkv = d.hidden_size, d.num_heads, d.num_kv_heads
    qn = (nh + 2 * nkv) * 128
    eps = 2.0 ** -11 if dtype == "f16" else 2.0 ** -8
    try:
        _, a12 = _attention_of(t.model, 12)
        qkv14, a14 = _attention_of(t.model, 14)
        qkv15, a15 = _attention_of(t.model, 15)
        _, a13 = _attention_of(t.model, 13)
    finally:
        t.model.engine.close()
    # plain products, [hi | lo] store
    hi, lo = a14[:, :H], a14[:, H:]
    assert torch.equal(hi, a12[:, :H])
    assert torch.count_nonzero(lo) > 0 and bool(torch.all(lo.abs() <= eps * hi.abs() + 6e-8))       # half a 16-bit step of hi (+ the fp16 subnormal step)
    x = qkv14[:, :qn]
    ref = _exact_attention(x[:, :nh * 128], x[:, nh * 128:(nh + nkv) * 128], x[:, (nh + nkv) * 128:], nh, nkv)
    rms = lambda a: float(torch.sqrt(torch.mean(a * a)))
    e_hi, e_hilo = rms(hi.double() - ref), rms(hi.double() + lo.double() - ref)          # (the 16-bit P of the plain products stays in both)
    assert e_hilo < e_hi
    # split products, hi-only store
    assert torch.equal(a13[:, :H], a15[:, :H])
    x = qkv15[:, :qn].double() + qkv15[:, qn:].double()
    ref2 = _exact_attention(x[:, :nh * 128], x[:, nh * 128:(nh + nkv) * 128], x[:, (nh + nkv) * 128:], nh, nkv)
    scale = ref2.abs().max()
    e13 = float(((a13[:, :H].double() - ref2).abs() / (ref2.abs() + scale * eps)).max())
    e15 = float(((a15[:, :H].double() + a15[:, H:].double() - ref2).abs()).max() / scale)
    with capsys.disabled():
        print(f"\n[attention forms, {dtype}] plain + [hi|lo] store: rms |hi - exact| {e_hi:.2e}, |hi + lo - exact| {e_hilo:.2e}; "
              f"split + hi store: rel {e13:.2e} (one rounding {eps:.1e}); whole-call hi + lo vs exact {e15:.2e} of max")
    assert e13 < 1.5 * eps


def test_adapter_load_after_a_resolved_select_forces_a_re_measure():
    t = P._build("tiny", dtype="f16")
    M, E = t.model, t.model.engine
    try:
        prob = t.prob
        tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
        Tt = lambda rows: [torch.from_numpy(r) for r in rows]
        vtg = RU.padding_ids(Tt(prob.vtg_ids), Tt(prob.vtg_labels), Tt(prob.vtg_masks), tok)
        tvg = RU.padding_ids(Tt(prob.tvg_ids), Tt(prob.tvg_labels), Tt(prob.tvg_masks), tok)
        mk = lambda: RU.PairScorer(DDPLike(M), vtg[0], vtg[2], vtg[1], tvg[0], tvg[2], tvg[1], [torch.from_numpy(v) for v in prob.video],
                                   torch.from_numpy(prob.video_vocab), torch.from_numpy(prob.tvg_video_labels), t.dims.num_clips)
        M.vtg_precise = "select"
        cal = RU.calibration_pairs(torch.from_numpy(prob.v2t_sims), t.spec["topk"], n_queries=32, per_query=8)
        with pytest.raises(RuntimeError):
            M(inputs_embeds=torch.zeros((1, 4, t.dims.hidden_size), dtype=M.dtype, device="cuda"))      # unresolved select: forward() refuses
        # a bar no unit can meet forces the mask path (plain fails), so the mask is measured and resolved
        chosen, table = mk().calibrate_vtg_select(cal, bar=1e-9, n_eval=3 * len(cal))
        assert chosen == "select" and M.vtg_mode() == "select" and len(table["units"]) == 4 * ((t.dims.num_layers + 3) // 4)
        assert np.array_equal(M.vtg_select_mask(), np.array(table["mask"], np.uint8))
        E.set_layer_mask(np.zeros(t.dims.num_layers, np.uint8))                    # (as if a cheaper mask had been measured)
        M.resolve_vtg("select", np.zeros(t.dims.num_layers, np.uint8))
        dims = t.dims
        r = 8
        n = CK.expected_adapters(dims)[0]
        n_out, n_in = synth.weight_shapes(dims)[n]
        E.load_adapter(n, np.random.RandomState(0).randn(r, n_in).astype(np.float32) * 0.01, np.zeros((n_out, r), np.float32), r, 16.0)
        assert M.vtg_mode() == "auto" and M.vtg_select_mask() is None                     # stale: evaluation() measures again
        assert np.array_equal(E.layer_mask, np.full(dims.num_layers, 15))                  # and until then the engine runs the full form
        chosen2, table2 = mk().calibrate_vtg_select(cal, bar=1e-9, n_eval=3 * len(cal))
        assert chosen2 == "select" and "units" in table2 and M.vtg_mode() == "select"
    finally:
        E.close()


def test_select_on_heavy7b_holds_the_bar_over_a_whole_evaluation(capsys):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vtg_select_validate.py"), "--n", "400", "--weights", "heavy7b", "--no_step"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout[r.stdout.index("{"):])
    mats = {k: v for k, v in d.items() if isinstance(v, dict) and "entries" in v}
    assert len(mats) == 6
    with capsys.disabled():
        print(f"\n[heavy7b, N = 400, 7B] select -> {d['vtg_chosen']}, mask {d['mask']} (k = {d['k']}), calibration {d['calibration_seconds']} s; "
              f"{d['seconds_full']} s full, {d['seconds_select']} s select; "
              + "; ".join(f"{k} max {v['max']:.1e} over {v['over_1e-3']}" for k, v in mats.items()))
    assert all(v["over_1e-3"] == 0 for v in mats.values()), mats
    assert all(v["bit_equal"] for k, v in mats.items() if "(TVG" in k)


def test_main_eval_with_select_runs_end_to_end():
    r = subprocess.run([sys.executable, "-m", "blim_amd.main", "--eval", "--synthetic", "64", "--vtg_precise", "select", "--topk", "8"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "vtg_precise select" in r.stderr, r.stderr[-2000:]
