"""CPU: `--calibration_store DIR` -- the numpy statement of the device content hash, the store's records and keys, the verify-or-measure flow of a stored
`--vtg_precise select` decision (on synthetic deviation laws, as tests/test_vtg_select_host.py does), and the multi-rank rules over two gloo ranks.  The device
side (blim_hash_device, blim_weights_fingerprint, whole evaluations) is tests/test_calibration_store_gpu.py."""
import json
import os
import socket
import types

import numpy as np
import pytest
import torch

from blim_amd import calibration as CAL
from blim_amd import calibration_store as CS
from blim_amd import retrieval_utils as RU
from blim_amd.synth import ModelDims

DIMS = ModelDims()
M64 = (1 << 64) - 1


# ----------------------------------------------------------------------------- the hash
def _mix1(x):
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _mix2(x):
    x = ((x ^ (x >> 33)) * 0xFF51AFD7ED558CCD) & M64
    x = ((x ^ (x >> 33)) * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def _hash_py(data: bytes):
    """The definition of csrc/kernels.hpp in plain Python integers (an independent statement of calibration_store.hash_bytes)."""
    n = len(data)
    padded = data + b"\0" * (-n % 8)
    s1 = s2 = 0
    for i in range(len(padded) // 8):
        w = int.from_bytes(padded[8 * i: 8 * i + 8], "little")
        s1 = (s1 + _mix1(w ^ (((i + 1) * CS.HASH_C1) & M64))) & M64
        s2 = (s2 + _mix2(w ^ (((i + 1) * CS.HASH_C2) & M64))) & M64
    return _mix1(s1 ^ (((n + 1) * CS.HASH_C1) & M64)), _mix2(s2 ^ (((n + 1) * CS.HASH_C2) & M64))


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 16, 4099])
def test_numpy_hash_matches_its_definition(n):
    data = np.random.RandomState(n).randint(0, 256, size=n, dtype=np.uint8).tobytes()
    assert CS.hash_bytes(data) == _hash_py(data)
    assert CS.hash_bytes(np.frombuffer(data, np.uint8)) == _hash_py(data)
    assert CS.hash_bytes(data, chunk_words=3) == _hash_py(data)               # the chunking of the numpy statement does not show


def test_hash_is_index_and_length_sensitive():
    rng = np.random.RandomState(0)
    a = rng.randint(0, 256, size=4096, dtype=np.uint8)
    h = CS.hash_bytes(a)
    w = a.view("<u8").copy()
    w[[3, 17]] = w[[17, 3]]                                                   # the same words, two of them swapped
    assert CS.hash_bytes(w.view(np.uint8)) != h
    z = np.zeros(64, np.uint8)
    z2 = z.copy(); z2[8] = 1
    z3 = z.copy(); z3[16] = 1                                                 # the same word value at another index
    assert len({CS.hash_bytes(z), CS.hash_bytes(z2), CS.hash_bytes(z3)}) == 3
    assert CS.hash_bytes(b"abc") != CS.hash_bytes(b"abc\0")                   # zero padding: the byte length tells them apart
    assert CS.hash_bytes(b"") != CS.hash_bytes(b"\0" * 8)
    b = a.copy(); b[-1] ^= 1                                                  # one bit of the last byte
    assert CS.hash_bytes(b) != h
    assert all(0 <= x <= M64 for x in h)


# ----------------------------------------------------------------------------- keys and records
class _FakeEngine:
    can_precise = True

    def __init__(self, fp="0123456789abcdef0123456789abcdef"):
        self.masks, self.dtype, self.lo6, self._fp = [], "f16", True, fp

    def set_layer_mask(self, bits):
        self.masks.append(None if bits is None else np.asarray(bits, dtype=np.uint8).copy())

    def fingerprint(self):
        return self._fp


def _mod(fp="0123456789abcdef0123456789abcdef"):
    return types.SimpleNamespace(engine=_FakeEngine(fp), vtg_precise="select", tvg_precise="auto", masked_query_zero=False, _second_request=None)


def _args(**kw):
    return types.SimpleNamespace(lora_mode=kw.get("lora_mode", "apart"), f8_mask=kw.get("f8_mask", None))


def _fields(**over):
    f = CS.key_fields(_mod(), _args(), "0123456789abcdef0123456789abcdef", "libdigest")
    for k, v in over.items():
        f[k] = v
    return f


def test_key_changes_with_every_field():
    base = CS.key_of(_fields())
    assert CS.key_of(_fields()) == base
    changes = {"fingerprint": "f" * 32, "dtype": "bf16", "second_pass": "auto", "precise_lo6": False, "masked_query_zero": True, "lora_mode": "merge",
               "f8_mask": 12, "vtg_precise": "auto", "tvg_precise": "full", "library": "another build", "schema": CS.SCHEMA + 1}
    assert set(changes) | {"criterion"} == set(_fields())                     # every field of the key is exercised
    keys = {k: CS.key_of(_fields(**{k: v})) for k, v in changes.items()}
    for c in ("bar", "z", "tail_margin"):
        crit = dict(_fields()["criterion"]); crit[c] *= 1.5
        keys["criterion." + c] = CS.key_of(_fields(criterion=crit))
    assert base not in keys.values() and len(set(keys.values())) == len(keys), keys
    assert _fields()["criterion"] == {"bar": 1e-3, "z": 4.5, "tail_margin": 0.8}
    # the options are read off the model and the driver's arguments
    m = _mod(); m.masked_query_zero = True; m._second_request = "auto"
    f = CS.key_fields(m, _args(lora_mode="merge", f8_mask=12), "ff", "lib")
    assert f["masked_query_zero"] and f["lora_mode"] == "merge" and f["f8_mask"] == 12 and f["second_pass"] == "auto" and f["precise_lo6"] is None


def _decisions():
    return {"vtg": {"request": "select", "mode": "select", "mask": [15] * 4 + [0] * 24, "n_eval": 48000,
                    "table": {"k": 24, "mask": [15] * 4 + [0] * 24, "none": {"max": 2e-3, "rms": np.float64(3e-4), "pred": float("inf"), "n": np.int64(256)}}},
            "tvg": {"request": "auto", "mode": "full", "mask": None, "n_eval": 32000, "table": {}}}


def test_record_round_trip_and_miss(tmp_path):
    st = CS.CalibrationStore(str(tmp_path / "store"))
    key = CS.key_of(_fields())
    assert st.load(key) is None                                               # a miss, no directory yet
    p = st.save(key, _fields(), _decisions())
    assert os.path.dirname(p) == st.dir and not [f for f in os.listdir(st.dir) if f.endswith(".tmp")]
    rec = st.load(key)
    assert rec["schema"] == CS.SCHEMA and rec["key"] == key and rec["fields"] == json.loads(json.dumps(_fields()))
    d = rec["decisions"]
    assert d["vtg"]["mask"] == [15] * 4 + [0] * 24 and d["vtg"]["n_eval"] == 48000 and d["tvg"]["mode"] == "full"
    assert d["vtg"]["table"]["none"]["pred"] == float("inf") and d["vtg"]["table"]["none"]["n"] == 256
    assert st.load(CS.key_of(_fields(dtype="bf16"))) is None                  # another key: a miss


@pytest.mark.parametrize("content", [b"", b"{\"schema\": 1, \"key\": ", b"\x00\xff garbage", b"[1, 2, 3]", b"{\"schema\": 1}"])
def test_corrupt_or_truncated_records_are_ignored(tmp_path, capsys, content):
    st = CS.CalibrationStore(str(tmp_path))
    key = CS.key_of(_fields())
    with open(st.path(key), "wb") as f:
        f.write(content)
    assert st.load(key) is None
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "ignoring" in err


def test_other_schema_or_key_is_ignored(tmp_path, capsys):
    st = CS.CalibrationStore(str(tmp_path))
    key = CS.key_of(_fields())
    st.save(key, _fields(), _decisions())
    rec = json.load(open(st.path(key)))
    for bad in (dict(rec, schema=CS.SCHEMA + 1), dict(rec, key="0" * 40), dict(rec, decisions={"vtg": {"mode": 3}})):
        json.dump(bad, open(st.path(key), "w"))
        assert st.load(key) is None
    assert capsys.readouterr().err.count("ignoring") == 3
    st.save(key, _fields(), _decisions())                                     # a good record replaces a bad one
    assert st.load(key) is not None


# ----------------------------------------------------------------------------- verify or measure (`--vtg_precise select`)
class _Fake(CAL.CalibrationMixin):
    def __init__(self):
        self.engine, self.m, self.device, self.mode = _FakeEngine(), types.SimpleNamespace(dims=DIMS), torch.device("cpu"), None
        self.resolved = None
        self.m.resolve_vtg = lambda mode, mask=None: setattr(self, "resolved", (mode, None if mask is None else np.asarray(mask).copy()))

    def set_vtg_mode(self, mode):
        self.mode = mode


def _pair_noise(block):
    b = np.asarray(block, dtype=np.int64).reshape(-1, 2)
    h = (b[:, 0] * 1000003 + b[:, 1] * 7919) % 2147483647
    return np.abs(np.array([np.random.RandomState(int(x)).randn() for x in h]))


def _law(scale=1.0):
    """dev(pair, mask) = noise(pair) x the summed sensitivity of the plain (class, layer) units: the QKV and gate|up units of a few layers dominate."""
    w = np.abs(np.random.RandomState(1).randn(4, DIMS.num_layers)) * 2e-6
    w[0, [0, 1, 27]] = 3e-4
    w[2, [1, 2, 26]] = 2e-4

    def measure(mask, block):
        m = np.zeros(DIMS.num_layers, np.int64) if mask is None else np.asarray(mask, np.int64)
        plain = np.array([[(m[l] >> c) & 1 == 0 for l in range(DIMS.num_layers)] for c in range(4)])
        return _pair_noise(block) * float((w * plain).sum()) * scale
    return measure


def _pairs():
    sims = np.random.RandomState(5).randn(600, 600).astype(np.float32)
    return RU.calibration_pairs(sims, 16, n_queries=32, per_query=8), RU.calibration_pairs(sims, 16, n_queries=256, per_query=8)


def _session(tmp_path, rec=None, writer=True):
    fields = _fields()
    return CS.StoreSession(CS.CalibrationStore(str(tmp_path)), CS.key_of(fields), fields, rec, writer=writer)


def test_cold_then_warm_select(tmp_path):
    first, confirm = _pairs()
    calls = []
    law = _law()
    counted = lambda mask, b: (calls.append(None if mask is None else tuple(int(x) for x in mask)), law(mask, b))[1]
    ses = _session(tmp_path)
    cold = _Fake()
    ch, table = CS.vtg_select_with_store(cold, ses, first, confirm, 48000, None, measure=counted)
    assert ch == "select" and ses.finish() == "measured"
    n_cold = len(calls)
    rec = ses.store.load(ses.key)
    assert rec["decisions"]["vtg"]["mask"] == table["mask"] and rec["decisions"]["vtg"]["n_eval"] == 48000
    # warm: one probe of the stored mask on the sample (the reference is cached per block), the same resolution
    calls.clear()
    ses2 = _session(tmp_path, rec)
    warm = _Fake()
    ch2, t2 = CS.vtg_select_with_store(warm, ses2, first, confirm, 48000, None, measure=counted)
    assert ch2 == "select" and t2["source"] == "store" and t2["mask"] == table["mask"] and t2["verify"]["accepted"]
    assert len(calls) == 1 and calls[0] == tuple(table["mask"]) and n_cold > 10
    assert warm.mode == "select" and warm.resolved[0] == "select" and np.array_equal(warm.resolved[1], np.array(table["mask"], np.uint8))
    assert np.array_equal(warm.engine.masks[-1], np.array(table["mask"], np.uint8))
    mtime = os.path.getmtime(ses.store.path(ses.key))
    assert ses2.finish() == "store" and os.path.getmtime(ses.store.path(ses.key)) == mtime       # nothing changed: not rewritten
    # a larger evaluation than the mask was confirmed at: the forced confirmation is added, and the record remembers the larger n_eval
    calls.clear()
    ses3 = _session(tmp_path, ses.store.load(ses.key))
    ch3, t3 = CS.vtg_select_with_store(_Fake(), ses3, first, confirm, 96000, None, measure=counted)
    assert ch3 == "select" and t3["verify"]["forced_confirm"] and "confirm" in t3["verify"] and len(calls) == 2
    assert ses3.finish() == "store" and ses.store.load(ses.key)["decisions"]["vtg"]["n_eval"] == 96000


def test_failed_verification_falls_back_to_the_cold_path(tmp_path):
    first, confirm = _pairs()
    ses = _session(tmp_path)
    CS.vtg_select_with_store(_Fake(), ses, first, confirm, 48000, None, measure=_law())
    ses.finish()
    rec = ses.store.load(ses.key)
    # other weights behind the same key (what the fingerprint normally rules out) or another evaluation's pairs: 10 x the deviations -- the stored mask fails
    ses2 = _session(tmp_path, rec)
    sc = _Fake()
    ch, table = CS.vtg_select_with_store(sc, ses2, first, confirm, 48000, None, measure=_law(10.0))
    assert "units" in table and table["rejected_verify"]["accepted"] is False            # the cold calibration ran
    want_ch, want = _Fake().calibrate_vtg_select(first, n_eval=48000, confirm_pairs=confirm, measure=_law(10.0))
    assert ch == want_ch and table["mask"] == want["mask"] and table["mask"] != rec["decisions"]["vtg"]["mask"]
    assert ses2.finish() == "store_rejected"
    assert ses.store.load(ses.key)["decisions"]["vtg"]["mask"] == want["mask"]           # the cold result replaced the record


def test_plain_resolution_is_only_adopted_through_the_check(tmp_path):
    first, confirm = _pairs()
    small = _law(1e-3)                                                                    # plain passes
    ses = _session(tmp_path)
    ch, _ = CS.vtg_select_with_store(_Fake(), ses, first, confirm, 48000, None, measure=small)
    assert ch == "none" and ses.finish() == "measured"
    rec = ses.store.load(ses.key)
    assert rec["decisions"]["vtg"]["mode"] == "none"
    calls = []
    sc = _Fake()
    ch2, t2 = CS.vtg_select_with_store(sc, _session(tmp_path, rec), first, confirm, 48000, None, measure=lambda m, b: (calls.append(m), small(m, b))[1])
    assert ch2 == "none" and t2["source"] == "store" and calls == [None] and sc.mode is None and sc.resolved == ("none", None)
    # ... and rejected when plain no longer holds
    ses3 = _session(tmp_path, rec)
    ch3, t3 = CS.vtg_select_with_store(_Fake(), ses3, first, confirm, 48000, None, measure=_law())
    assert ch3 == "select" and "units" in t3 and ses3.finish() == "store_rejected"


def test_auto_decisions_compare_with_the_record(tmp_path):
    ses = _session(tmp_path)
    ses.record("tvg", "auto", "full", {"attn": {"max": 1e-2}}, 32000)
    assert ses.finish() == "measured"
    rec = ses.store.load(ses.key)
    s2 = _session(tmp_path, rec)
    s2.record("tvg", "auto", "full", {"attn": {"max": 2e-2}}, 32000)
    assert s2.finish() == "store"
    s3 = _session(tmp_path, rec)
    s3.record("tvg", "auto", "attn", {"attn": {"max": 1e-4}}, 32000)
    assert s3.finish() == "store_rejected" and ses.store.load(ses.key)["decisions"]["tvg"]["mode"] == "attn"
    # a reader that is not the writer (an emulated rank, a rank other than 0) never writes
    s4 = _session(tmp_path, None, writer=False)
    s4.record("tvg", "auto", "full", {}, 32000)
    s4.finish()
    assert ses.store.load(ses.key)["decisions"]["tvg"]["mode"] == "attn"


def test_main_accepts_calibration_store():
    from blim_amd import main as M
    assert M.get_args_parser().parse_args(["--eval"]).calibration_store is None        # off by default
    assert M.get_args_parser().parse_args(["--eval", "--calibration_store", "/x/y"]).calibration_store == "/x/y"


# ----------------------------------------------------------------------------- two gloo ranks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_worker(rank, world, port, dirs, fps, out_q):
    torch._C._get_accelerator = lambda: torch.device("cpu")          # (see tests/test_distributed_gloo.py: _cpu_rank)
    import torch.distributed as dist
    from blim_amd import distributed as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    D.init_distributed_mode(backend="gloo")
    try:
        ses = CS.open_session(dirs[rank], _mod(fps[rank]), _args(), torch.device("cpu"), collective=True, rank=rank, writer=rank == 0)
        out_q.put((rank, "ok", ses.key, ses.stored("vtg")))
    except RuntimeError as ex:
        out_q.put((rank, "raised", str(ex), None))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(dirs, fps):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, dirs, fps, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_two_gloo_ranks_rank0_record_is_broadcast(tmp_path):
    d0, d1 = str(tmp_path / "rank0"), str(tmp_path / "rank1")                # rank 1's directory holds nothing: what it sees came from rank 0
    fp = "00112233445566778899aabbccddeeff"
    fields = CS.key_fields(_mod(fp), _args(), fp, CS.library_digest())
    key = CS.key_of(fields)
    CS.CalibrationStore(d0).save(key, fields, _decisions())
    (r0, s0, k0, v0), (r1, s1, k1, v1) = _two_ranks([d0, d1], [fp, fp])
    assert s0 == s1 == "ok" and k0 == k1 == key
    assert v0 == v1 and v1["mask"] == _decisions()["vtg"]["mask"]
    assert not os.path.exists(d1)


def test_two_gloo_ranks_fingerprint_mismatch_raises(tmp_path):
    d = str(tmp_path)
    (r0, s0, m0, _), (r1, s1, m1, _) = _two_ranks([d, d], ["a" * 32, "b" * 32])
    assert s0 == s1 == "raised" and "a" * 32 in m0 and "b" * 32 in m0 and "same weights" in m1
