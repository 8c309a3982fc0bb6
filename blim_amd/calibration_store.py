"""`--calibration_store DIR`: the numeric modes an evaluation MEASURED (calibration.py: `--vtg_precise auto | select`, `--tvg_precise auto`, `--second_pass auto`) kept
across runs, keyed by a content fingerprint of the weights.

What a calibration decides depends only on the weights, the adapters, the numeric options and the library build; the in-process reuse (BlimModel's resolutions, tied to
Engine.weights_version) ends with the process.  The store keeps one JSON record per key in DIR:
- the key (`key_fields`): Engine.fingerprint() (blim_weights_fingerprint: every placed tensor as the kernels read it, the adapters kept apart, the visual head, the
  config), the dtype, every option that changes numerics (second pass / precise_lo6, masked_query_zero, lora_mode, f8_mask), the request strings, the criterion
  (bar, z, tail_margin) and a digest of the loaded libblim_hip.so -- a kernel change changes numerics;
- the record: per decision ("vtg", "tvg", "second") the request, the resolved mode (and the `select` mask), the n_eval it was made at and the original table.
A stored decision is never adopted unchecked: it is verified on the evaluation's own calibration sample with the cold path's rule (calibration.CalibrationMixin.
verify_vtg_select; the `auto` decisions are the same single check the cold path makes), and a failed verification falls back to the cold calibration, whose result
replaces the record.  Records that cannot be read, are truncated or carry another schema are ignored with one warning.  Writes are atomic (temp file + os.replace)
and come from rank 0 of a real job only; emulated ranks (`--shard`) only read.
"""
from __future__ import annotations

import hashlib
import inspect
import json
import os
import sys
import tempfile
import time
from typing import Optional

import numpy as np

SCHEMA = 1
SOURCES = ("measured", "store", "store_rejected")

_M64 = (1 << 64) - 1
HASH_C1, HASH_C2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03


# ----------------------------------------------------------------------------- the device hash, restated (csrc/kernels.hpp: launch_hash_device)
def _mix1(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _mix2(x):
    x = (x ^ (x >> np.uint64(33))) * np.uint64(0xFF51AFD7ED558CCD)
    x = (x ^ (x >> np.uint64(33))) * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def _mix_int(k: int, x: int) -> int:
    with np.errstate(over="ignore"):
        return int((_mix1 if k == 1 else _mix2)(np.array([x & _M64], dtype=np.uint64))[0])


def hash_bytes(buf, chunk_words: int = 1 << 23):
    """(d1, d2) of the buffer's bytes: little-endian 64-bit words w_i (the last one zero-padded), S_k = sum_i mix_k(w_i ^ (i + 1) C_k) mod 2^64, then
    d_k = mix_k(S_k ^ (bytes + 1) C_k).  NOT cryptographic.  What blim_hash_device computes on the device, bit for bit, for any launch grid."""
    b = np.frombuffer(memoryview(buf).cast("B"), dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    n = int(b.size)
    n_full = n // 8
    s1 = s2 = 0
    with np.errstate(over="ignore"):
        c1, c2 = np.uint64(HASH_C1), np.uint64(HASH_C2)
        for w0 in range(0, n_full, chunk_words):
            w1 = min(n_full, w0 + chunk_words)
            w = b[8 * w0: 8 * w1].view("<u8")
            i = np.arange(w0 + 1, w1 + 1, dtype=np.uint64)
            s1 = (s1 + int(_mix1(w ^ (i * c1)).sum(dtype=np.uint64))) & _M64
            s2 = (s2 + int(_mix2(w ^ (i * c2)).sum(dtype=np.uint64))) & _M64
        if n % 8:
            tail = np.zeros(8, np.uint8)
            tail[: n % 8] = b[8 * n_full:]
            w = tail.view("<u8")
            i = np.array([n_full + 1], dtype=np.uint64)
            s1 = (s1 + int(_mix1(w ^ (i * c1))[0])) & _M64
            s2 = (s2 + int(_mix2(w ^ (i * c2))[0])) & _M64
    return _mix_int(1, s1 ^ (((n + 1) * HASH_C1) & _M64)), _mix_int(2, s2 ^ (((n + 1) * HASH_C2) & _M64))


# ----------------------------------------------------------------------------- the key
def criterion() -> dict:
    """bar, z, tail_margin of the calibrations (the defaults of CalibrationMixin.calibrate_vtg, which evaluation() uses for every decision)."""
    from .calibration import CalibrationMixin
    p = inspect.signature(CalibrationMixin.calibrate_vtg).parameters
    return {k: float(p[k].default) for k in ("bar", "z", "tail_margin")}


_lib_digest = {}


def library_digest(path: Optional[str] = None) -> str:
    """sha256 of the libblim_hip.so file the process loads (a kernel change changes numerics)."""
    from . import engine as E
    path = path or E.LIB_PATH
    st = os.stat(path)
    k = (path, st.st_size, st.st_mtime_ns)
    if k not in _lib_digest:
        h = hashlib.sha256()
        with open(path, "rb") as f:
            for blk in iter(lambda: f.read(1 << 22), b""):
                h.update(blk)
        _lib_digest[k] = h.hexdigest()
    return _lib_digest[k]


def key_fields(mod, args, fingerprint: str, lib_digest: str) -> dict:
    """Everything a stored decision depends on besides the evaluation's own pairs (those are re-measured on every hit)."""
    eng = mod.engine
    second = getattr(mod, "_second_request", None)
    return {
        "schema": SCHEMA,
        "fingerprint": str(fingerprint),
        "dtype": str(eng.dtype),
        "second_pass": second,
        "precise_lo6": None if second == "auto" else bool(getattr(eng, "lo6", False)),
        "masked_query_zero": bool(getattr(mod, "masked_query_zero", False)),
        "lora_mode": str(getattr(args, "lora_mode", "apart") or "apart"),
        "f8_mask": getattr(args, "f8_mask", None),
        "vtg_precise": getattr(mod, "vtg_precise", None),
        "tvg_precise": getattr(mod, "tvg_precise", None),
        "criterion": criterion(),
        "library": str(lib_digest),
    }


def key_of(fields: dict) -> str:
    return hashlib.sha256(json.dumps(fields, sort_keys=True).encode()).hexdigest()[:40]


def _plain(x):
    """JSON-safe copy of a calibration table (numpy scalars / arrays -> Python; inf stays a float: json writes Infinity and reads it back)."""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return _plain(x.tolist())
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    if isinstance(x, (np.bool_,)):
        return bool(x)
    return x


# ----------------------------------------------------------------------------- the directory
class CalibrationStore:
    """One JSON file per key in `directory`."""

    def __init__(self, directory: str):
        self.dir = str(directory)

    def path(self, key: str) -> str:
        return os.path.join(self.dir, f"calibration-{key}.json")

    def load(self, key: str) -> Optional[dict]:
        """The record stored under `key`, or None: missing, unreadable, truncated, another schema or another key -- the last four with one warning line."""
        p = self.path(key)
        if not os.path.exists(p):
            return None
        try:
            with open(p) as f:
                rec = json.load(f)
            ok = isinstance(rec, dict) and rec.get("schema") == SCHEMA and rec.get("key") == key and isinstance(rec.get("decisions"), dict)
            ok = ok and all(isinstance(d, dict) and isinstance(d.get("mode"), (str, type(None))) for d in rec["decisions"].values())
        except Exception as ex:                                          # (truncated JSON, binary garbage, a directory in its place, ...)
            print(f"calibration store: ignoring unreadable record {p} ({type(ex).__name__}: {ex})", file=sys.stderr, flush=True)
            return None
        if not ok:
            print(f"calibration store: ignoring record {p} (another schema or key, or malformed; this version writes schema {SCHEMA})", file=sys.stderr, flush=True)
            return None
        return rec

    def save(self, key: str, fields: dict, decisions: dict) -> str:
        """Atomic write: a temp file in the same directory, then os.replace."""
        os.makedirs(self.dir, exist_ok=True)
        rec = {"schema": SCHEMA, "key": key, "fields": _plain(fields), "written": time.strftime("%Y-%m-%dT%H:%M:%S"), "decisions": _plain(decisions)}
        fd, tmp = tempfile.mkstemp(prefix=".calibration-", suffix=".tmp", dir=self.dir)
        try:
            with os.fdopen(fd, "w") as f:
                json.dump(rec, f, indent=1)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, self.path(key))
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return self.path(key)


# ----------------------------------------------------------------------------- one evaluation's use of the store
class StoreSession:
    """The record of one evaluation: what was stored (`stored(kind)`), what this evaluation decided (`record(...)`), and at the end the source and the write."""

    def __init__(self, store: CalibrationStore, key: str, fields: dict, record: Optional[dict], writer: bool):
        self.store, self.key, self.fields, self.writer = store, key, fields, bool(writer)
        self.loaded = (record or {}).get("decisions", {}) if record else {}
        self.decisions = {k: dict(v) for k, v in self.loaded.items()}
        self.verified, self.rejected = [], []

    @property
    def fingerprint(self) -> str:
        return self.fields["fingerprint"]

    def stored(self, kind: str) -> Optional[dict]:
        return self.loaded.get(kind)

    def record(self, kind: str, request, mode, table, n_eval, mask=None, verified: Optional[bool] = None):
        """This evaluation's decision of `kind`.  verified: True / False when a stored decision was checked (verify_vtg_select); None -- the `auto` kinds, whose
        check IS the cold calibration -- compares the measured decision with the stored one."""
        old = self.loaded.get(kind)
        new = {"request": request, "mode": mode, "mask": None if mask is None else [int(b) for b in mask], "n_eval": None if n_eval is None else int(n_eval),
               "table": _plain(table)}
        if old is not None:
            if verified is None:
                verified = old.get("mode") == mode and old.get("mask") == new["mask"]
            (self.verified if verified else self.rejected).append(kind)
            if verified:
                # a stored decision that held: kept, with the largest n_eval it has been confirmed at
                new = dict(old, n_eval=max(int(old.get("n_eval") or 0), int(n_eval or 0)))
        self.decisions[kind] = new

    def source(self) -> str:
        if self.rejected:
            return "store_rejected"
        return "store" if self.verified else "measured"

    def finish(self) -> str:
        """Writes the record (rank 0 of a real job; not an emulated rank) when it changed; returns the calibration source."""
        if self.writer and self.decisions and self.decisions != self.loaded:
            try:
                self.store.save(self.key, self.fields, self.decisions)
            except OSError as ex:
                print(f"calibration store: could not write {self.store.path(self.key)} ({ex}); the run goes on", file=sys.stderr, flush=True)
        return self.source()


def vtg_select_with_store(cal, ses: Optional[StoreSession], pairs, confirm_pairs, n_eval, share, measure=None):
    """`--vtg_precise select` with a store session (or None): a stored decision is verified on this evaluation's sample (CalibrationMixin.verify_vtg_select); a miss
    or a failed verification runs the cold calibration (calibrate_vtg_select), whose result goes into the record.  Every rank of a job takes the same branch: the
    record is rank 0's and the verification's deviations are gathered like the cold path's.  Returns (chosen, table); table["source"] says where the decision came from."""
    stored = ses.stored("vtg") if ses is not None else None
    tried = None
    if stored is not None and stored.get("request") == "select" and stored.get("mode") in ("none", "select"):
        ok, chosen, vt = cal.verify_vtg_select(stored, pairs, n_eval=n_eval, share=share, confirm_pairs=confirm_pairs, measure=measure)
        if ok:
            table = dict(stored.get("table") or {}, verify=vt["verify"], seconds=vt["seconds"], source="store")
            ses.record("vtg", "select", chosen, table, n_eval, mask=stored.get("mask") if chosen == "select" else None, verified=True)
            return chosen, table
        tried = vt
    chosen, table = cal.calibrate_vtg_select(pairs, n_eval=n_eval, share=share, confirm_pairs=confirm_pairs, measure=measure)
    table["source"] = "measured" if tried is None else "store_rejected"
    if tried is not None:
        table["rejected_verify"] = tried["verify"]
        table["seconds"] = table.get("seconds", 0.0) + tried["seconds"]
    if ses is not None:
        ses.record("vtg", "select", chosen, table, n_eval, mask=table.get("mask") if chosen == "select" else None, verified=None if tried is None else False)
    return chosen, table


def open_session(directory: str, mod, args, device, collective: bool, rank: int, writer: bool) -> StoreSession:
    """Fingerprint, key and record of this evaluation.  In a multi-rank job every rank computes its own fingerprint and key, they are all-gathered and the job stops
    when they differ (ranks that loaded different weights); rank 0 reads the record and broadcasts it.  Without a process group (one process, `--shard`) the process
    reads the record itself."""
    fp = mod.engine.fingerprint()
    fields = key_fields(mod, args, fp, library_digest())
    key = key_of(fields)
    store = CalibrationStore(directory)
    if collective:
        import torch.distributed as dist
        keys = [None] * dist.get_world_size()
        dist.all_gather_object(keys, (key, fp))
        check_same_keys(keys)
        box = [store.load(key) if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        rec = box[0]
    else:
        rec = store.load(key)
    return StoreSession(store, key, fields, rec, writer=writer)


def check_same_keys(keys):
    """keys: every rank's (key, fingerprint).  Raises when they differ."""
    if len({k for k, _ in keys}) > 1:
        fps = ", ".join(f"rank {r}: {fp}" for r, (_, fp) in enumerate(keys))
        raise RuntimeError("calibration store: the ranks of this job do not hold the same weights and options (weights fingerprints " + fps + "); "
                           "every rank must load the same checkpoint, adapters and numeric options")
