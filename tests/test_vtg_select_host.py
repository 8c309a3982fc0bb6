"""CPU: `--vtg_precise select` -- the per-layer, per-GEMM compensation mask of the VTG calls (calibration.CalibrationMixin.calibrate_vtg_select) on synthetic
deviation laws, its agreement over two gloo ranks, and the request / resolution plumbing of BlimModel and main.py.  The engine side is covered by
tests/test_vtg_select_gpu.py."""
import os
import socket
import types

import numpy as np
import pytest
import torch

from blim_amd import calibration as CAL
from blim_amd import retrieval_utils as RU
from blim_amd.synth import ModelDims

DIMS = ModelDims()          # the 7B configuration: 28 layers -> 4 classes x 7 groups = 28 units


class _FakeEngine:
    can_precise = True

    def __init__(self):
        self.masks = []

    def set_layer_mask(self, bits):
        self.masks.append(None if bits is None else np.asarray(bits, dtype=np.uint8).copy())


class _Fake(CAL.CalibrationMixin):
    """What calibrate_vtg_select reads of a PairScorer: engine, m.dims, device, set_vtg_mode (the measurement itself is handed in)."""

    def __init__(self):
        self.engine, self.m, self.device, self.mode = _FakeEngine(), types.SimpleNamespace(dims=DIMS), torch.device("cpu"), None
        self.resolved = None
        self.m.resolve_vtg = lambda mode, mask=None: setattr(self, "resolved", (mode, None if mask is None else np.asarray(mask).copy()))

    def set_vtg_mode(self, mode):
        self.mode = mode


def _pair_noise(block, seed=0):
    """A deterministic, rank-independent |N(0, 1)|-like value per (video, text) pair."""
    b = np.asarray(block, dtype=np.int64).reshape(-1, 2)
    h = (b[:, 0] * 1000003 + b[:, 1] * 7919 + seed * 104729) % 2147483647
    return np.abs(np.array([np.random.RandomState(int(x)).randn() for x in h]))


def _unit_weights(seed=1):
    """Per-(class, layer) sensitivity: the normalised-input GEMMs (QKV, gate|up) of a few layers dominate, as on trained weights."""
    rng = np.random.RandomState(seed)
    w = np.abs(rng.randn(4, DIMS.num_layers)) * 2e-6
    w[0, [0, 1, 27]] = 3e-4
    w[2, [1, 2, 26]] = 2e-4
    return w


def _monotone_law(weights, scale=1.0):
    """dev(pair, mask) = noise(pair) x sum of the weights of the plain (class, layer) units: grows with every unit made plain."""
    def measure(mask, block):
        m = np.zeros(DIMS.num_layers, np.int64) if mask is None else np.asarray(mask, np.int64)
        plain = np.array([[(m[l] >> c) & 1 == 0 for l in range(DIMS.num_layers)] for c in range(4)])
        return _pair_noise(block) * float((weights * plain).sum()) * scale
    return measure


def _pairs():
    sims = np.random.RandomState(5).randn(600, 600).astype(np.float32)
    return RU.calibration_pairs(sims, 16, n_queries=32, per_query=8), RU.calibration_pairs(sims, 16, n_queries=256, per_query=8)


def test_units_masks_and_costs():
    units = CAL.vtg_select_units(28, 4)
    assert len(units) == 28 and units[0] == (0, 0, 4) and units[-1] == (3, 24, 28)
    assert len(CAL.vtg_select_units(30, 4)) == 32 and CAL.vtg_select_units(30, 4)[7] == (0, 28, 30)
    m = CAL.vtg_unit_mask(28, [(2, 4, 8), (0, 0, 4)])
    assert m.dtype == np.uint8 and list(m[:4]) == [14] * 4 and list(m[4:8]) == [11] * 4 and set(m[8:]) == {15}
    f = [CAL.vtg_unit_flops(DIMS, (c, 0, 4)) for c in range(4)]
    assert f[2] > f[3] > f[0] > f[1]                         # gate|up 58 %, down 29 %, QKV 7 %, o_proj 5.5 % of a layer's GEMM flops


def test_plain_passing_short_circuits():
    sc = _Fake()
    calls = []
    law = _monotone_law(_unit_weights() * 1e-3)
    first, _ = _pairs()
    chosen, table = sc.calibrate_vtg_select(first, n_eval=48000, measure=lambda mask, b: (calls.append(mask), law(mask, b))[1])
    assert chosen == "none" and sc.mode is None and sc.resolved == ("none", None)
    assert all(m is None for m in calls) and "units" not in table


def _largest_passing_prefix(sc, law, pairs, order_names, n_eval, bar=1e-3, z=4.5, tail_margin=0.8):
    units = CAL.vtg_select_units(DIMS.num_layers, 4)
    by_name = {f"{CAL.VTG_UNIT_CLASSES[u[0]]}{u[1]}-{u[2] - 1}": u for u in units}
    best = 0
    for k in range(len(units) + 1):
        d = law(CAL.vtg_unit_mask(DIMS.num_layers, [by_name[n] for n in order_names[:k]]), pairs)
        st = sc._stats(d, n_eval)
        a, b = sc._passes([d], st, n_eval, len(pairs), bar, z, tail_margin)
        if a and b:
            best = k
    return best


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_largest_passing_prefix_on_monotone_laws(seed):
    first, confirm = _pairs()
    law = _monotone_law(_unit_weights(seed))
    sc = _Fake()
    chosen, table = sc.calibrate_vtg_select(first, n_eval=48000, confirm_pairs=confirm, measure=law)
    assert chosen == "select" and sc.mode == "select"
    assert len(table["units"]) == 28 and len(table["probes"]) <= 5
    assert table["none"]["max"] > 1e-3                                       # plain alone fails
    want = _largest_passing_prefix(sc, law, first, table["order"], 48000)
    assert 0 < want < 28 and table["k"] == want, (table["k"], want, table["probes"])
    mask = np.array(table["mask"], dtype=np.uint8)
    assert sc.resolved[0] == "select" and np.array_equal(sc.resolved[1], mask) and np.array_equal(sc.engine.masks[-1], mask)
    assert np.array_equal(sc.engine.masks[0], np.full(28, 15, np.uint8))     # the full form before anything is measured
    assert table["confirm"] and table["confirm"][-1]["accepted"] and table["seconds"] >= 0.0
    # the sensitive units (QKV of layers 0, 1, 27; gate|up of 1, 2, 26) stay compensated; the order is by deviation per flop saved
    assert all((mask[l] & 1) for l in (0, 1, 27)) and all((mask[l] & 4) for l in (1, 2, 26))
    rows = {r["unit"]: r for r in table["units"]}
    ratio = [rows[n]["rms"] / rows[n]["flops"] for n in table["order"]]
    assert ratio == sorted(ratio)


def test_confirmation_reject_steps_back_then_falls_back_to_full():
    first, confirm = _pairs()
    seen = {(int(a), int(b)) for a, b in first}
    base = _monotone_law(_unit_weights(1))

    def stricter_outside(factor_of_k):
        def law(mask, block):
            d = base(mask, block)
            extra = np.array([(int(a), int(b)) not in seen for a, b in np.asarray(block)], dtype=bool)
            n_plain = 0 if mask is None else int(sum(bin(15 - int(x)).count("1") for x in mask))
            d[extra] *= factor_of_k(n_plain)
            return d
        return law

    # the confirmation sample is 40 x worse once more than a few (class, layer) bits are plain: the first pick is rejected, a halved k accepted
    sc = _Fake()
    ch, table = sc.calibrate_vtg_select(first, n_eval=48000, confirm_pairs=confirm, measure=stricter_outside(lambda n: 40.0 if n > 20 else 1.0))
    ks = [c["k"] for c in table["confirm"]]
    assert ch == "select" and len(ks) >= 2 and ks[1] == ks[0] // 2 and not table["confirm"][0]["accepted"] and table["confirm"][-1]["accepted"]
    assert table["k"] == ks[-1] > 0
    # ... and when the confirmation sample rejects every plain unit: three tries, then all ones
    sc = _Fake()
    ch, table = sc.calibrate_vtg_select(first, n_eval=48000, confirm_pairs=confirm, measure=stricter_outside(lambda n: 1e4 if n else 1.0))
    ks = [c["k"] for c in table["confirm"]]
    assert len(ks) == 3 and ks[1] == ks[0] // 2 and ks[2] == ks[1] // 2 and not any(c["accepted"] for c in table["confirm"])
    assert ch == "select" and table["k"] == 0 and table["mask"] == [15] * 28 and np.array_equal(sc.resolved[1], np.full(28, 15))


def test_lognormal_heavy_tail_is_never_let_through():
    """Every plain unit adds a log-normal deviation (sigma 0.9, the heavy7b law): a 256-pair sample sits inside the bar, but the tail of 48,000 entries does not."""
    first, confirm = _pairs()

    def law(mask, block):
        m = np.zeros(28, np.int64) if mask is None else np.asarray(mask, np.int64)
        n_plain = int(sum(bin(15 - int(x)).count("1") for x in m))
        b = np.asarray(block, np.int64)
        z = np.array([np.random.RandomState(int(x)).randn() for x in (b[:, 0] * 7919 + b[:, 1]) % 2147483647])
        return (4e-5 * np.sqrt(n_plain)) * np.exp(0.9 * z)

    sc = _Fake()
    ch, table = sc.calibrate_vtg_select(first, n_eval=48000, confirm_pairs=confirm, measure=law)
    assert table["mask"] == [15] * 28 and table["k"] == 0
    assert all(not p["passed"] for p in table["probes"])
    # the same law over a whole evaluation's 48,000 entries does exceed the bar with one unit plain
    pop = 4e-5 * np.exp(0.9 * np.random.RandomState(0).randn(48000))
    assert pop.max() > 1e-3


# ----------------------------------------------------------------------------- two gloo ranks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_worker(rank, world, port, out_q):
    torch._C._get_accelerator = lambda: torch.device("cpu")          # (see tests/test_distributed_gloo.py: _cpu_rank)
    import torch.distributed as dist
    from blim_amd import distributed as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    D.init_distributed_mode(backend="gloo")
    first, confirm = _pairs()
    sizes = []
    law = _monotone_law(_unit_weights(2))
    sc = _Fake()
    ch, table = sc.calibrate_vtg_select(first, n_eval=48000, confirm_pairs=confirm, share=(world, rank),
                                        measure=lambda mask, b: (sizes.append(len(b)), law(mask, b))[1])
    out_q.put((rank, ch, table["mask"], table["order"], max(sizes)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_reach_the_same_mask():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, c0, m0, o0, s0), (_, c1, m1, o1, s1) = res
    assert c0 == c1 == "select" and m0 == m1 and o0 == o1
    assert s0 <= 1024 and s1 <= 1024                                        # each rank scored its own half of the (confirmation) sample only
    first, confirm = _pairs()
    _, t1 = _Fake().calibrate_vtg_select(first, n_eval=48000, confirm_pairs=confirm, measure=_monotone_law(_unit_weights(2)))
    assert t1["mask"] == m0                                                 # = the one-process decision


# ----------------------------------------------------------------------------- request / resolution, driver
class _MaskEngine(_FakeEngine):
    def __init__(self):
        super().__init__()
        self.weights_version, self.dtype, self.layer_mask = 0, "f16", None

    def set_layer_mask(self, bits):
        super().set_layer_mask(bits)
        self.layer_mask = None if bits is None else np.asarray(bits, dtype=np.uint8).copy()


def test_select_request_and_its_resolution_follow_the_weights():
    from blim_amd.modeling import BlimModel
    m = BlimModel.__new__(BlimModel)
    m.engine, m.dims = _MaskEngine(), DIMS
    m._vtg_request, m._tvg_request, m._vtg_resolved, m._tvg_resolved = None, "full", None, None
    m.vtg_precise = "select"
    assert m.vtg_precise == "select" and m.vtg_mode() == "auto" and m.vtg_select_mask() is None       # unresolved
    mask = np.full(28, 15, np.uint8); mask[3:9] = 10
    m.resolve_vtg("select", mask)
    assert m.vtg_mode() == "select" and np.array_equal(m.vtg_select_mask(), mask) and np.array_equal(m.engine.layer_mask, mask)
    m.engine.weights_version += 1                                                    # new weights / adapters: stale
    assert m.vtg_mode() == "auto" and m.vtg_select_mask() is None
    m.resolve_vtg("none")
    assert m.vtg_mode() is None and m.vtg_select_mask() is None
    with pytest.raises(ValueError):
        m.resolve_vtg("select")                                                      # a select resolution names its mask
    m.resolve_vtg("select", mask)
    m.vtg_precise = "full"                                                           # a new request: the engine's mask back to the full form
    assert m.vtg_mode() == "full" and np.array_equal(m.engine.layer_mask, np.full(28, 15)) and m.vtg_select_mask() is None
    with pytest.raises(ValueError):
        m.vtg_precise = "selected"


def test_engine_resets_the_mask_on_every_weight_change():
    """Engine._weights_changed (no device needed: the ctypes calls are stubbed)."""
    from blim_amd import engine as E
    e = E.Engine.__new__(E.Engine)
    calls = []
    e.lib = types.SimpleNamespace(blim_set_option=lambda h, k, v: (calls.append((k, v)), 0)[1])
    e.h, e.dims, e.dtype, e.weights_version = None, DIMS, "f16", 0
    e._layer_mask, e._layer_bits_live = None, None
    e._weights_changed()
    assert e.weights_version == 1 and calls == [] and e.layer_mask is None
    mask = np.full(28, 15, np.uint8); mask[0] = 3; mask[27] = 0
    e.set_layer_mask(mask)
    assert sorted(calls) == sorted([(b"precise_layer_bits", (0 << 4) | 3), (b"precise_layer_bits", (27 << 4) | 0)])
    calls.clear()
    e._weights_changed()
    assert e.weights_version == 2 and np.array_equal(e.layer_mask, np.full(28, 15))
    assert sorted(calls) == sorted([(b"precise_layer_bits", (0 << 4) | 15), (b"precise_layer_bits", (27 << 4) | 15)])
    with pytest.raises(ValueError):
        e.set_layer_mask(np.full(27, 15))
    with pytest.raises(ValueError):
        e.set_layer_mask(np.full(28, 16))


def test_main_accepts_select():
    from blim_amd import main as M
    a = M.get_args_parser().parse_args(["--eval", "--vtg_precise", "select"])
    assert a.vtg_precise == "select"
    assert M.get_args_parser().parse_args(["--eval"]).vtg_precise == "auto"          # the default is unchanged
    with pytest.raises(SystemExit):
        M.get_args_parser().parse_args(["--eval", "--vtg_precise", "sel"])


def test_select_flops_accounting():
    from blim_amd.pair_scorer import executed_flops, lo6_pass_flops
    full = executed_flops(DIMS, 4096, 64, "vtg", "full")
    assert executed_flops(DIMS, 4096, 64, "vtg", "select", layer_bits=np.full(28, 15)) == pytest.approx(full)
    plain_layers = executed_flops(DIMS, 4096, 64, "vtg", "select", layer_bits=np.zeros(28))
    assert executed_flops(DIMS, 4096, 64, "vtg", None) < plain_layers < full
    assert lo6_pass_flops(DIMS, 4096, 64, "vtg", "select", layer_bits=np.full(28, 15)) == pytest.approx(lo6_pass_flops(DIMS, 4096, 64, "vtg", "full"))
