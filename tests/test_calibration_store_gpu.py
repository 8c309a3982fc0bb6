"""GPU: `--calibration_store` -- the device content hash (blim_hash_device) against its numpy statement, the engine's weights fingerprint
(blim_weights_fingerprint: load order, sensitivity, adapters, merge vs apart), and cold / warm evaluations with the store.  The host-side logic is
tests/test_calibration_store_host.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from blim_amd import calibration_store as CS
from blim_amd import engine as E
from blim_amd import retrieval_utils as RU
from blim_amd import synth
from blim_amd.modeling import BlimModel, DDPLike

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(vocab_size=151700, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1, mm_hidden_size=64)


def _hash_both_grids(t, monkeypatch):
    """blim_hash_device under its own grid and under a forced 3-workgroup grid."""
    a = E.hash_device(t)
    monkeypatch.setenv("BLIM_HASH_GRID", "3")
    b = E.hash_device(t)
    monkeypatch.delenv("BLIM_HASH_GRID")
    return a, b


@pytest.mark.parametrize("n", [1, 7, 4096 + 3, 300_000_007])
def test_device_hash_matches_numpy(n, monkeypatch):
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    t = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    want = CS.hash_bytes(t.cpu().numpy())
    a, b = _hash_both_grids(t, monkeypatch)
    assert a == want and b == want, (n, a, b, want)
    if n > 1:                                                           # an address that is not 16-B aligned (the byte-wise path)
        assert E.hash_device(t[1:]) == CS.hash_bytes(t[1:].cpu().numpy())
        assert E.hash_device(t, nbytes=n - 1) == CS.hash_bytes(t[: n - 1].cpu().numpy())


def test_device_hash_beyond_4gib(monkeypatch):
    n = 4 * 2**30 + 21
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(11)
    for s in range(0, n, 2**30):                                        # (random bytes in 1 GiB pieces)
        e = min(n, s + 2**30)
        t[s:e] = torch.randint(0, 256, (e - s,), dtype=torch.uint8, device="cuda", generator=g)
    host = t.cpu().numpy()
    want = CS.hash_bytes(host)
    a, b = _hash_both_grids(t, monkeypatch)
    assert a == want and b == want
    t[n - 1] ^= 1                                                       # one bit of the last byte, past 4 GiB
    assert E.hash_device(t) != want


# ----------------------------------------------------------------------------- the weights fingerprint
def _dims():
    return synth.ModelDims(**TINY)


def _engine(w, order=None, dtype="f16"):
    m = BlimModel(_dims(), max_positions=512, dtype=dtype)
    names = list(w) if order is None else order
    for n in names:
        m.engine.load_weight(n, w[n])
    assert m.engine.weights_ready()
    return m


def test_fingerprint_is_load_order_independent_and_content_sensitive():
    dims = _dims()
    w = synth.synthetic_weights(dims, 3)
    names = list(w)
    m1 = _engine(w)
    m2 = _engine(w, order=names[::-1])
    try:
        f1, f2 = m1.engine.fingerprint(), m2.engine.fingerprint()
        assert f1 == f2 and len(f1) == 32 and m1.engine.fingerprint() == f1
        # one element of the last layer's down projection
        last = f"layers.{dims.num_layers - 1}.down_proj.w"
        w2 = dict(w); w2[last] = w[last].copy(); w2[last][5, 7] += 0.01
        m2.engine.load_weight(last, w2[last])
        assert m2.engine.fingerprint() != f1
        m2.engine.load_weight(last, w[last])
        assert m2.engine.fingerprint() == f1                            # back to the same content: the same fingerprint
        # the fp32 visual head below the 16-bit rounding (hi unchanged): its hi + lo rows tell
        vh = w["visual_head"].copy()
        i = np.unravel_index(np.argmax(np.abs(vh)), vh.shape)
        vh[i] = np.float32(vh[i]) * np.float32(1 + 2.0 ** -14)
        m2.engine.load_weight("visual_head", vh)
        assert m2.engine.fingerprint() != f1
        m2.engine.load_weight("visual_head", w["visual_head"])
        # adapters kept apart, and their scaling
        n = "layers.0.q_proj.w"
        n_out, n_in = synth.weight_shapes(dims)[n]
        rng = np.random.RandomState(0)
        A, B = (rng.randn(8, n_in) * 0.01).astype(np.float32), (rng.randn(n_out, 8) * 0.01).astype(np.float32)
        m2.engine.load_adapter(n, A, B, 8, 16.0)
        f_ad = m2.engine.fingerprint()
        assert f_ad != f1
        m2.engine.clear_adapters(); m2.engine.load_adapter(n, A, B, 8, 32.0)
        f_ad32 = m2.engine.fingerprint()
        assert f_ad32 not in (f1, f_ad)
        m2.engine.clear_adapters()
        assert m2.engine.fingerprint() == f1
        # merge (W + (alpha / r) B A folded into the base weight) vs apart
        wm = dict(w); wm[n] = w[n] + (16.0 / 8) * (B @ A)
        m3 = _engine(wm)
        try:
            assert m3.engine.fingerprint() not in (f1, f_ad)
        finally:
            m3.engine.close()
        # the compute dtype is part of it
        m4 = _engine(w, dtype="bf16")
        try:
            assert m4.engine.fingerprint() != f1
        finally:
            m4.engine.close()
    finally:
        m1.engine.close(); m2.engine.close()


# ----------------------------------------------------------------------------- evaluations with the store
def _evaluate(model, prob, store, vtg, tvg, topk=8):
    tok = types.SimpleNamespace(pad_token_id=synth.PAD_ID)
    nz = lambda x: np.where(x == 0, np.float32(1e-6), x)
    args = types.SimpleNamespace(topk=topk, num_clips=model.dims.num_clips, cpn=True, resume="x", eval=True, dataset="MSRVTT", batch_size_eval=16,
                                 iv2_scores={"v2t": torch.from_numpy(nz(prob.v2t_sims)), "t2v": torch.from_numpy(nz(prob.t2v_sims))}, max_tokens=32768, dedup=True,
                                 calibration_store=store)
    model.clear_cache()
    model.tvg_precise = tvg
    model.vtg_precise = vtg
    model.set_tvg_prefix_length(prob.tvg_prefix_length)
    t2v, v2t = RU.evaluation(DDPLike(model), synth.ProblemLoader(prob, 16), torch.device("cuda", 0), tok, args)
    return t2v, v2t, args._eval_stats


def test_auto_warm_run_is_bit_equal_to_a_run_without_the_store(tmp_path):
    dims = _dims()
    model = BlimModel(dims, max_positions=512, dtype="f16")
    try:
        model.engine.init_synthetic_weights(3)
        prob = synth.make_problem(2, 48, dims, tok_per_clip=8, text_len=(3, 8))
        store = str(tmp_path / "store")
        t0, v0, s0 = _evaluate(model, prob, None, "auto", "auto")
        t1, v1, s1 = _evaluate(model, prob, store, "auto", "auto")
        t2, v2, s2 = _evaluate(model, prob, store, "auto", "auto")
    finally:
        model.engine.close()
    assert "calibration_source" not in s0
    assert s1["calibration_source"] == "measured" and s2["calibration_source"] == "store"
    assert s1["weights_fingerprint"] == s2["weights_fingerprint"] and len(os.listdir(store)) == 1
    assert s0["vtg_precise"] == s1["vtg_precise"] == s2["vtg_precise"] and s0["tvg_precise"] == s2["tvg_precise"]
    for d0, d2 in ((t0, t2), (v0, v2)):
        for k in d0:
            assert np.array_equal(d0[k], d2[k]), k


def test_select_cold_then_warm_on_heavy7b(capsys):
    """N = 400, 7B dims, `--vtg_precise select`: a record made on Gaussian weights is a miss for heavy7b; the heavy7b warm run verifies the stored mask and is
    bit-equal to its cold run (tools/calibration_store_bench.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "calibration_store_bench.py"), "--n", "400", "--weights", "gaussian,heavy7b", "--modes", "select",
                        "--no_full"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout[r.stdout.index("{"):])
    g, h = d["gaussian"]["select"], d["heavy7b"]["select"]
    with capsys.disabled():
        print(f"\n[heavy7b, N = 400, 7B, select] cold: {h['cold']['source']} mask {h['cold']['mask']} calibration {h['cold']['calibration_seconds']} s, "
              f"{h['cold']['seconds']} s; warm: {h['warm']['source']} calibration {h['warm']['calibration_seconds']} s, {h['warm']['seconds']} s")
    assert d["gaussian"]["fingerprint"] != d["heavy7b"]["fingerprint"]
    assert g["cold"]["source"] == "measured" and g["warm"]["source"] == "store"
    assert h["cold"]["source"] == "measured"                            # the Gaussian record in the same store is a miss
    assert h["cold"]["vtg"] == "select" and h["warm"]["source"] == "store" and h["same_mask"] and h["warm"]["mask"] == h["cold"]["mask"]
    assert h["warm_bit_equal_cold"] and h["recall_equal"]
    assert h["warm"]["calibration_seconds"] < h["cold"]["calibration_seconds"]
