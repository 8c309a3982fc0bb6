"""ctypes binding of libblim_hip.so (include/blim.h).

PyTorch is used only for device memory / streams: every tensor handed to the engine is a CUDA(HIP)
tensor whose data_ptr() goes through the C ABI.  There is NO CPU fallback: importing works without a
GPU (so the CPU test-suite can check symbols and host logic), but creating an engine or launching a
kernel without the library or without a device raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Optional, Sequence

import numpy as np

from .synth import ModelDims, weight_shapes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BLIM_LIB_PATH") or os.path.join(_HERE, "libblim_hip.so")     # override: A/B of two builds (tools/)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "blim.h")

DTYPE_F32, DTYPE_BF16 = 0, 1
COMPUTE_DTYPES = {"bf16": 0, "f16": 1, "f8": 2}     # "f8": e4m3 operands for the big GEMMs + lm_head, fp16 everywhere else
DEFAULT_COMPUTE_DTYPE = os.environ.get("BLIM_DTYPE", "f16")   # fp16 = the reference's own autocast dtype


def torch_dtype_of(name: str):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16, "f8": torch.float16}[name]


class BlimError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32),
                ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32),
                ("mm_hidden_size", C.c_int32), ("num_clips", C.c_int32), ("max_positions", C.c_int32),
                ("compute_dtype", C.c_int32), ("rms_eps", C.c_float), ("rope_theta", C.c_float)]


class Batch(C.Structure):
    _fields_ = [("n_tokens", C.c_int64), ("n_seqs", C.c_int32), ("n_blocks", C.c_int32),
                ("positions", C.c_void_p), ("key_visible", C.c_void_p), ("seq_start", C.c_void_p),
                ("seq_len", C.c_void_p), ("pfx_start", C.c_void_p), ("pfx_len", C.c_void_p),
                ("blk_seq", C.c_void_p), ("blk_q0", C.c_void_p), ("own_start", C.c_void_p)]


class AttentionArgs(C.Structure):
    """blim_attention_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("batch", C.POINTER(Batch)), ("qkv", C.c_void_p), ("ldq", C.c_int64),
                ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32), ("dtype16", C.c_int32), ("use_tr_read", C.c_int32),
                ("v_lo_off", C.c_int64), ("out_lo_off", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64), ("scale", C.c_float),
                ("lse_out", C.c_void_p), ("out8", C.c_void_p), ("ldo8", C.c_int64), ("out_mx", C.c_void_p), ("mx_stride", C.c_int64),
                ("pfx_cache", C.c_void_p), ("pfx_slot", C.c_void_p), ("pc_slot_stride", C.c_int64), ("pc_ld", C.c_int64), ("pc_lo_off", C.c_int64),
                ("pc_n_slots", C.c_int32), ("pc_max_len", C.c_int32)]


class AttentionBwdArgs(C.Structure):
    """blim_attention_bwd_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("qkv", C.c_void_p), ("ldq", C.c_int64), ("dout", C.c_void_p), ("ldo", C.c_int64), ("o16", C.c_void_p),
                ("ldo16", C.c_int64), ("lse", C.c_void_p), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32), ("dtype16", C.c_int32),
                ("key_visible", C.c_void_p), ("seq_start", C.c_void_p), ("seq_len", C.c_void_p), ("n_seqs", C.c_int32), ("max_len", C.c_int32),
                ("scale", C.c_float), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("dqkv", C.c_void_p), ("n_tokens", C.c_int64)]


class LoraDownArgs(C.Structure):
    """blim_lora_down_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("x16", C.c_void_p), ("ldx", C.c_int64), ("T", C.c_int64), ("K", C.c_int32), ("n_adapters", C.c_int32),
                ("r", C.c_int32), ("dtype16", C.c_int32), ("A", C.c_void_p * 3), ("scale", C.c_float), ("drop_p", C.c_float), ("seed", C.c_uint64),
                ("site", C.c_uint32), ("reserved", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class LoraGradsArgs(C.Structure):
    """blim_lora_grads_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("flags", C.c_int32), ("dtype16", C.c_int32), ("T", C.c_int64), ("N", C.c_int32), ("K", C.c_int32),
                ("r", C.c_int32), ("reserved", C.c_int32), ("dy16", C.c_void_p), ("ldy", C.c_int64), ("u16", C.c_void_p), ("ldu", C.c_int64),
                ("x16", C.c_void_p), ("ldx", C.c_int64), ("B", C.c_void_p), ("scale", C.c_float), ("drop_p", C.c_float), ("seed", C.c_uint64),
                ("site", C.c_uint32), ("reserved2", C.c_int32), ("dB", C.c_void_p), ("du", C.c_void_p), ("dA", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


class LoraDxArgs(C.Structure):
    """blim_lora_dx_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("dx", C.c_void_p), ("ldd", C.c_int64), ("T", C.c_int64), ("K", C.c_int32), ("n_adapters", C.c_int32),
                ("r", C.c_int32), ("dtype16", C.c_int32), ("du", C.c_void_p * 3), ("A", C.c_void_p * 3), ("drop_p", C.c_float), ("site", C.c_uint32),
                ("seed", C.c_uint64), ("out16", C.c_void_p), ("ldo", C.c_int64)]


class RmsnormBwdArgs(C.Structure):
    """blim_rmsnorm_bwd_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("dx", C.c_void_p), ("dy", C.c_void_p), ("x", C.c_void_p), ("rows", C.c_void_p), ("n_rows", C.c_int64),
                ("H", C.c_int32), ("accumulate", C.c_int32), ("w", C.c_void_p), ("eps", C.c_float), ("dtype16", C.c_int32), ("out16", C.c_void_p),
                ("n_adapters", C.c_int32), ("r", C.c_int32), ("du", C.c_void_p * 3), ("A", C.c_void_p * 3), ("drop_p", C.c_float), ("site", C.c_uint32),
                ("seed", C.c_uint64)]


class RmsnormArgs(C.Structure):
    """blim_rmsnorm_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("x", C.c_void_p), ("ldx", C.c_int64), ("rows", C.c_void_p), ("n_rows", C.c_int64), ("n_src", C.c_int64),
                ("H", C.c_int32), ("dtype16", C.c_int32), ("w", C.c_void_p), ("eps", C.c_float), ("saturate", C.c_int32), ("out16", C.c_void_p),
                ("ldo", C.c_int64), ("out_lo", C.c_void_p), ("out_f32", C.c_void_p), ("out6", C.c_void_p)]


LORA_DB, LORA_DU, LORA_DA = 1, 2, 4


class GemmArgs(C.Structure):
    """blim_gemm_args (include/blim.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("epi", C.c_int32), ("dtype", C.c_int32), ("A", C.c_void_p), ("lda", C.c_int64), ("W", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("act", C.c_int32), ("C", C.c_void_p), ("ldc", C.c_int64), ("bias", C.c_void_p),
                ("resid_in", C.c_void_p), ("scale", C.c_float), ("w_wrap_k", C.c_int32), ("lo_off", C.c_int64), ("f16_saturate", C.c_int32),
                ("rope_cols", C.c_int32), ("rope_rows", C.c_void_p), ("rope_stride", C.c_int64), ("labels", C.c_void_p), ("lse_part", C.c_void_p),
                ("label_logit", C.c_void_p), ("row_scale", C.c_void_p), ("col_scale", C.c_void_p), ("a_mx", C.c_void_p), ("out8", C.c_void_p),
                ("out_mx", C.c_void_p), ("mx_stride", C.c_int64), ("A6", C.c_void_p), ("W6", C.c_void_p), ("K6", C.c_int32), ("f6_build", C.c_int32),
                ("out6", C.c_void_p), ("swiglu_act", C.c_void_p), ("swiglu_act_ld", C.c_int64), ("swiglu_gu", C.c_void_p), ("swiglu_ld", C.c_int64), ("tile", C.c_int32),
                ("tile_lo6", C.c_int32), ("tile_qkv", C.c_int32)]


EPILOGUES = {"bf16": 0, "f32": 1, "resid": 2, "qkv": 3, "swiglu": 4, "lse": 5}
TVG_RANK_MAX_K = 1024            # BLIM_TVG_RANK_MAX_K (include/blim.h): the largest k of blim_tvg_rank / blim_score_tvg_first


def declared_symbols(header: str = HEADER_PATH) -> Sequence[str]:
    """Names of every function include/blim.h declares."""
    text = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(blim_[a-z0-9_]+)\s*\(", text)))


_lib = None


def load_library(path: str = LIB_PATH):
    """Loads the shared library (raises BlimError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- FIRST: torch ships its own HIP runtime; loaded after ours, the process ends up with two and
    #                              the second one sees no device (build() followed by smoke() in one process did exactly that)
    if not os.path.exists(path):
        raise BlimError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"(or `make -C blim_amd/csrc`). The BLiM engine has no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
    sig = {
        "blim_abi_version": ([], C.c_int),
        "blim_last_error": ([], C.c_char_p),
        "blim_create": ([C.POINTER(Config), C.POINTER(vp)], C.c_int),
        "blim_destroy": ([vp], None),
        "blim_load_weight": ([vp, C.c_char_p, vp, i32, i32], C.c_int),
        "blim_init_synthetic_weights": ([vp, u64], C.c_int),
        "blim_weights_ready": ([vp], C.c_int),
        "blim_load_adapter": ([vp, C.c_char_p, vp, vp, i32, f32], C.c_int),
        "blim_clear_adapters": ([vp], C.c_int),
        "blim_num_adapters": ([vp], C.c_int),
        "blim_reserve": ([vp, i64, i64], C.c_int),
        "blim_project_video": ([vp, vp, i64, i32, vp, vp], C.c_int),
        "blim_group_mean": ([vp, vp, i64, i32, vp, vp], C.c_int),
        "blim_assemble": ([vp, vp, i64, vp, vp, vp], C.c_int),
        "blim_decode": ([vp, C.POINTER(Batch), vp, vp, i64, vp, vp, vp], C.c_int),
        "blim_vtg_logprobs": ([vp, vp, vp, i64, vp, vp], C.c_int),
        "blim_segment_mean": ([vp, vp, vp, i32, i32, vp, vp], C.c_int),
        "blim_lm_head": ([vp, vp, i64, vp, vp], C.c_int),
        "blim_ce_rows": ([vp, vp, i64, i32, vp, i64, vp, vp], C.c_int),
        "blim_visual_head": ([vp, vp, i64, vp, vp], C.c_int),
        "blim_visual_head_f32": ([vp, vp, i64, vp, vp], C.c_int),
        "blim_tvg_scores": ([vp, vp, vp, i32, vp, i32, vp, vp], C.c_int),
        "blim_tvg_logits": ([vp, vp, vp, i32, i32, vp, vp], C.c_int),
        "blim_set_video_vocab": ([vp, vp, i32, vp], C.c_int),
        "blim_tvg_logits_f32": ([vp, vp, i32, vp, vp], C.c_int),
        "blim_score_vtg": ([vp, C.POINTER(Batch), vp, vp, vp, i64, vp, i32, vp, vp], C.c_int),
        "blim_score_tvg": ([vp, C.POINTER(Batch), vp, vp, vp, i32, vp, i32, vp, vp], C.c_int),
        "blim_forward": ([vp, vp, vp, i32, i32, vp, vp, vp], C.c_int),
        "blim_fill_bell_bf16": ([vp, i64, u64, C.c_char_p, f32, f32, vp], C.c_int),
        "blim_fill_bell_f32": ([vp, i64, u64, C.c_char_p, f32, f32, i32, vp], C.c_int),
        "blim_gemm_bf16": ([vp, i64, vp, i32, i32, i32, vp, i64, vp], C.c_int),
        "blim_gemm_f16": ([vp, i64, vp, i32, i32, i32, vp, i64, vp], C.c_int),
        "blim_f6_tiles_bytes": ([i64, i32], C.c_int64),
        "blim_gemm_f16_lo6": ([vp, vp, i32, i32, i32, vp, vp, vp, vp], C.c_int),
        "blim_quant_rows": ([vp, i64, i64, i32, i32, vp, vp, vp], C.c_int),
        "blim_gemm_f8": ([vp, i64, vp, vp, vp, i32, i32, i32, vp, i64, vp], C.c_int),
        "blim_attention": ([C.POINTER(AttentionArgs), vp], C.c_int),
        "blim_attention_bwd_workspace_bytes": ([i64, i32, i32, i32], C.c_int64),
        "blim_attention_bwd": ([C.POINTER(AttentionBwdArgs), vp], C.c_int),
        "blim_rope_bwd": ([vp, vp, i64, i32, i32, vp, vp, vp, i32, i32, vp], C.c_int),
        "blim_lora_down_workspace_bytes": ([i32, i32], C.c_int64),
        "blim_lora_down": ([C.POINTER(LoraDownArgs), vp], C.c_int),
        "blim_lora_grads_workspace_bytes": ([i32, i64, i32, i32, i32], C.c_int64),
        "blim_lora_grads": ([C.POINTER(LoraGradsArgs), vp], C.c_int),
        "blim_lora_dx": ([C.POINTER(LoraDxArgs), vp], C.c_int),
        "blim_rmsnorm_bwd": ([C.POINTER(RmsnormBwdArgs), vp], C.c_int),
        "blim_ce_workspace_bytes": ([i64], C.c_int64),
        "blim_ce_fwd_bwd": ([vp, i64, i32, vp, i32, i64, f32, vp, vp, i64, vp, i32, vp, i64, vp], C.c_int),
        "blim_gelu": ([i32, vp, i64, vp, vp, i64, i32, i32, vp], C.c_int),
        "blim_adamw_raw": ([vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, i32, vp], C.c_int),
        "blim_grad_stats_workspace_bytes": ([i64], C.c_int64),
        "blim_grad_stats_raw": ([vp, i64, f32, vp, vp, i64, vp], C.c_int),
        "blim_rmsnorm": ([C.POINTER(RmsnormArgs), vp], C.c_int),
        "blim_rmsnorm_f8": ([vp, i64, i64, i32, vp, f32, vp, vp, vp], C.c_int),
        "blim_lse_combine": ([vp, i32, vp, vp, i64, vp, vp], C.c_int),
        "blim_tvg_criterion": ([vp, i64, i32, vp, i32, i32, vp, vp], C.c_int),
        "blim_tvg_rank": ([vp, i64, i32, i32, vp, i64, i32, vp, f32, i32, vp, vp, vp, i64, vp], C.c_int),
        "blim_tvg_rank_within": ([vp, i64, i32, i32, vp, i64, i32, i32, vp, vp, vp, vp, i32, f32, i32, vp, vp, vp], C.c_int),
        "blim_rank_rows": ([vp, i64, i32, i32, i32, vp, vp, vp], C.c_int),
        "blim_tvg_cols": ([vp, i64, i32, i32, vp, i32, vp, i64, i64, vp], C.c_int),
        "blim_score_tvg_first": ([vp, C.POINTER(Batch), vp, vp, i32, vp, i32, vp, f32, i32, vp, vp, vp, vp], C.c_int),
        "blim_score_tvg_first_within": ([vp, C.POINTER(Batch), vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, i32, f32, i32, vp, vp, vp], C.c_int),
        "blim_tvg_first_cached": ([vp, vp, vp, i32, vp, i32, vp, i64, i32, vp], C.c_int),
        "blim_group_mean_rows": ([vp, vp, i64, i32, i32, i32, i32, vp], C.c_int),
        "blim_assemble_rows": ([vp, vp, i64, i32, vp, vp, i32, vp], C.c_int),
        "blim_gemm": ([C.POINTER(GemmArgs), vp], C.c_int),
        "blim_gemm_narrow_launches": ([], C.c_int64),
        "blim_gemm_narrow_threshold": ([], C.c_int32),
        "blim_gemm_narrow_lo6_launches": ([], C.c_int64),
        "blim_gemm_narrow_lo6_threshold": ([], C.c_int32),
        "blim_gemm_narrow_qkv_launches": ([], C.c_int64),
        "blim_gemm_narrow_qkv_threshold": ([], C.c_int32),
        "blim_rope_rows_bytes": ([i32], C.c_int64),
        "blim_rope_rows": ([vp, i64, f32, i32, vp, vp, i64, vp], C.c_int),
        "blim_timing_enable": ([vp, i32], C.c_int),
        "blim_timing_num_classes": ([], C.c_int),
        "blim_timing_class_name": ([i32], C.c_char_p),
        "blim_timing_report": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)], C.c_int),
        "blim_set_option": ([vp, C.c_char_p, i32], C.c_int),
        "blim_debug_read": ([vp, C.c_char_p, vp, i64, vp], C.c_int),
        "blim_debug_gemm_stamps": ([vp], C.c_int),
        "blim_hash_device": ([vp, i64, vp, vp], C.c_int),
        "blim_weights_fingerprint": ([vp, vp, vp], C.c_int),
        "blim_prefix_cache_bytes": ([vp, i32, i32, i32], C.c_int64),
        "blim_prefix_cache_create": ([vp, i32, i32, i32, C.POINTER(vp)], C.c_int),
        "blim_prefix_cache_destroy": ([vp], None),
        "blim_prefix_cache_fill": ([vp, vp, C.POINTER(Batch), vp, vp, vp], C.c_int),
        "blim_prefix_cache_slot_len": ([vp, i32], C.c_int),
        "blim_score_vtg_cached": ([vp, vp, C.POINTER(Batch), vp, vp, i32, vp, vp, vp, i64, vp, i32, vp, vp], C.c_int),
        "blim_score_tvg_cached": ([vp, vp, C.POINTER(Batch), vp, vp, i32, vp, vp, vp, i32, vp, i32, vp, vp], C.c_int),
        "blim_score_vtg_admit": ([vp, vp, C.POINTER(Batch), vp, vp, i32, vp, i32, vp, vp, vp, i64, vp, i32, vp, vp], C.c_int),
        "blim_score_tvg_admit": ([vp, vp, C.POINTER(Batch), vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, vp, vp], C.c_int),
        "blim_prefix_cache_record_bytes": ([vp, i32], C.c_int64),
        "blim_prefix_cache_export": ([vp, vp, vp, i32, vp, i64, vp, vp], C.c_int),
        "blim_prefix_cache_import": ([vp, vp, vp, i32, vp, i64, vp, vp], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise BlimError(f"{what} failed (code {rc}): {load_library().blim_last_error().decode()}")


def _ptr(t) -> int:
    """data_ptr of a contiguous device tensor (or None)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "engine buffers must be contiguous device tensors"
    return t.data_ptr()


def _stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


def vocab_key_of(video_vocab):
    """Identity of a video vocabulary tensor for "is this the one the engine holds?" (literal TVG path): address, shape, torch's in-place version counter AND a content
    fingerprint -- callers pass temporaries such as `vocab.to(dev)`, and the caching allocator hands the next temporary of the same shape the same address, so
    (address, shape) alone let another data set's vocabulary score against a stale registered copy.  The fingerprint is two sums over 4,096 strided values
    (one tiny device -> host copy per call of the literal, non-hot path)."""
    if not hasattr(video_vocab, "data_ptr"):
        return (id(video_vocab),)
    flat = video_vocab.reshape(-1)
    pick = flat[:: max(1, flat.numel() // 4096)][:4096].double()
    fp = (float(pick.sum()), float((pick * pick).sum()))
    return (video_vocab.data_ptr(), tuple(video_vocab.shape), int(getattr(video_vocab, "_version", 0)), fp)


class PackedBatch:
    """Device-side description of packed sequences (blim_batch).  Built from host numpy arrays."""

    def __init__(self, positions: np.ndarray, key_visible: np.ndarray, seq_start: np.ndarray, seq_len: np.ndarray,
                 pfx_start: Optional[np.ndarray] = None, pfx_len: Optional[np.ndarray] = None, device="cuda", own_start: Optional[np.ndarray] = None):
        """own_start (optional, [n_tokens]): first own-segment index (inside its sequence) each token attends to -- segmented sequences
        (blim.h: blim_batch.own_start); None or all zeros = plain causal sequences."""
        import torch
        n_seqs = len(seq_start)
        if pfx_start is None:
            pfx_start = np.zeros(n_seqs, dtype=np.int32)
            pfx_len = np.zeros(n_seqs, dtype=np.int32)
        seq_len = np.asarray(seq_len, dtype=np.int32)
        nblk = (seq_len + 31) // 32
        blk_seq = np.repeat(np.arange(n_seqs, dtype=np.int32), nblk)
        blk_q0 = (np.concatenate([np.arange(n, dtype=np.int32) for n in nblk]) * 32).astype(np.int32) if n_seqs else np.zeros(0, np.int32)
        self.n_tokens = int(len(positions))
        self.max_position = int(np.max(positions)) if len(positions) else 0     # checked against the engine's RoPE table
        self.n_seqs = int(n_seqs)
        self.n_blocks = int(len(blk_seq))
        # one host->device copy for all index arrays
        parts = [np.asarray(positions, np.int32), np.asarray(seq_start, np.int32), seq_len, np.asarray(pfx_start, np.int32),
                 np.asarray(pfx_len, np.int32), blk_seq, blk_q0]
        offs = np.cumsum([0] + [len(p) for p in parts])
        flat = torch.from_numpy(np.concatenate(parts)).to(device)
        self._flat = flat
        self.positions, self.seq_start, self.seq_len, self.pfx_start, self.pfx_len, self.blk_seq, self.blk_q0 = \
            [flat[offs[i]:offs[i + 1]] for i in range(7)]
        self.key_visible = torch.from_numpy(np.ascontiguousarray(key_visible, dtype=np.uint8)).to(device)
        self.own_start = None
        if own_start is not None and np.any(np.asarray(own_start) != 0):
            own_start = np.asarray(own_start, dtype=np.int32)
            assert len(own_start) == self.n_tokens
            self.own_start = torch.from_numpy(np.ascontiguousarray(own_start)).to(device)

    def struct(self, max_positions: Optional[int] = None) -> Batch:
        if max_positions is not None and self.max_position >= max_positions:
            raise BlimError(f"a sequence reaches position {self.max_position} but the engine's RoPE table holds {max_positions} positions: "
                            f"create the engine / BlimModel with a larger max_positions")
        b = Batch()
        b.n_tokens, b.n_seqs, b.n_blocks = self.n_tokens, self.n_seqs, self.n_blocks
        b.positions = self.positions.data_ptr(); b.key_visible = self.key_visible.data_ptr()
        b.seq_start = self.seq_start.data_ptr(); b.seq_len = self.seq_len.data_ptr()
        b.pfx_start = self.pfx_start.data_ptr(); b.pfx_len = self.pfx_len.data_ptr()
        b.blk_seq = self.blk_seq.data_ptr(); b.blk_q0 = self.blk_q0.data_ptr()
        b.own_start = self.own_start.data_ptr() if self.own_start is not None else None
        return b


class Engine:
    """One scoring engine on the current HIP device."""

    def __init__(self, dims: ModelDims, max_positions: int = 4096, dtype: Optional[str] = None):
        import torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise BlimError("no HIP device visible: the BLiM engine has no CPU fallback")
        self.dims = dims
        self.max_positions = int(max_positions)
        self.dtype = dtype or DEFAULT_COMPUTE_DTYPE          # "f16" | "bf16": 16-bit format of activations / weights / MFMA operands
        self.torch_dtype = torch_dtype_of(self.dtype)
        cfg = Config(dims.vocab_size, dims.hidden_size, dims.intermediate_size, dims.num_layers, dims.num_heads, dims.num_kv_heads,
                     dims.mm_hidden_size, dims.num_clips, max_positions, COMPUTE_DTYPES[self.dtype], dims.rms_eps, dims.rope_theta)
        h = C.c_void_p()
        _check(self.lib.blim_create(C.byref(cfg), C.byref(h)), "blim_create")
        self.h = h
        self.device = torch.device("cuda", torch.cuda.current_device())
        # mirrors the engine's default of option "precise_lo6" (include/blim.h): the compensated modes' second pass over K in e2m3 on fp16 engines
        # (bf16 engines: off by default -- their parity mode runs the second pass in bf16 -- on with set_option("precise_lo6", 1) / BLIM_PRECISE_LO6=1: round 6)
        lo6_ok = dims.hidden_size % 128 == 0 and dims.intermediate_size % 128 == 0 and max(dims.hidden_size, dims.intermediate_size) <= 20480
        self.lo6 = lo6_ok and ((dtype == "f16" and os.environ.get("BLIM_PRECISE_LO6", "1") != "0") or (dtype == "bf16" and os.environ.get("BLIM_PRECISE_LO6", "0") == "1"))
        self._precise_mlp = True          # the engine's default of option "precise_mlp"
        self.weights_version = 0          # bumped by every weight / adapter change: what a measured numeric mode was measured on (modeling.py: resolve_*)
        self._layer_mask = None           # set_layer_mask: per-layer compensation bits of the VTG calls under `--vtg_precise select` (None: no mask)
        self._layer_bits_live = None      # what the engine's "precise_layer_bits" hold (None: its default, all set)

    def close(self):
        if getattr(self, "h", None):
            self.lib.blim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights
    def load_weight(self, name: str, arr: np.ndarray):
        """One tensor: canonical name, float32 numpy array in the checkpoint's natural [out, in] layout."""
        shape = weight_shapes(self.dims)[name]
        assert tuple(arr.shape) == tuple(shape), (name, arr.shape, shape)
        a = np.ascontiguousarray(arr, dtype=np.float32)
        _check(self.lib.blim_load_weight(self.h, name.encode(), a.ctypes.data, DTYPE_F32, 0), f"blim_load_weight({name})")
        self._weights_changed()

    def load_weights(self, weights: Dict[str, np.ndarray]):
        """weights: canonical name -> float32 numpy array; every tensor of the model must be present."""
        for name, arr in weights.items():
            self.load_weight(name, arr)
        _check(self.lib.blim_weights_ready(self.h), "blim_weights_ready")

    def weights_ready(self) -> bool:
        return self.lib.blim_weights_ready(self.h) == 0

    def init_synthetic_weights(self, seed: int):
        _check(self.lib.blim_init_synthetic_weights(self.h, seed), "blim_init_synthetic_weights")
        self._weights_changed()

    # ---- LoRA adapters kept apart (blim.h: blim_load_adapter; the reference's --resume flow, main.py:96-105, 125-128)
    def load_adapter(self, weight_name: str, A: np.ndarray, B: np.ndarray, lora_r: int, lora_alpha: float):
        """A [r, in], B [out, r] float32 (peft's lora_A.weight / lora_B.weight) of the adapter on canonical weight `weight_name`."""
        n_out, n_in = weight_shapes(self.dims)[weight_name]
        assert tuple(A.shape) == (lora_r, n_in) and tuple(B.shape) == (n_out, lora_r), (weight_name, A.shape, B.shape, (n_out, n_in), lora_r)
        a = np.ascontiguousarray(A, dtype=np.float32); b = np.ascontiguousarray(B, dtype=np.float32)
        _check(self.lib.blim_load_adapter(self.h, weight_name.encode(), a.ctypes.data, b.ctypes.data, int(lora_r), float(lora_alpha)), f"blim_load_adapter({weight_name})")
        self._weights_changed()

    def clear_adapters(self):
        _check(self.lib.blim_clear_adapters(self.h), "blim_clear_adapters")
        self._weights_changed()

    def _weights_changed(self):
        """Every weight / adapter change: a mask measured on the old weights says nothing about the new ones -- it goes back to all ones (the `full` form) until a
        calibration measures again (modeling.py: vtg_select_mask)."""
        self.weights_version += 1
        if self._layer_mask is not None:
            self.set_layer_mask(np.full(self.dims.num_layers, 15, dtype=np.uint8))

    def num_adapters(self) -> int:
        return int(self.lib.blim_num_adapters(self.h))

    def fingerprint(self) -> str:
        """Content fingerprint (32 hex digits) of everything the scores depend on -- placed weights as the kernels read them, adapters kept apart, visual head,
        config (blim_weights_fingerprint; NOT cryptographic) -- the key of `--calibration_store` (calibration_store.py).  Computed once per weights_version."""
        fp = getattr(self, "_fingerprint", None)
        if fp is None or fp[0] != self.weights_version:
            out = (C.c_uint64 * 2)()
            _check(self.lib.blim_weights_fingerprint(self.h, out, _stream()), "blim_weights_fingerprint")
            fp = self._fingerprint = (self.weights_version, f"{out[0]:016x}{out[1]:016x}")
        return fp[1]

    def reserve(self, max_tokens: int, max_rows: int, compensated: bool = False):
        """Pre-size the workspaces.  compensated=True (16-bit engines): size them for compensated calls ([hi | lo] rows) and, on a "precise_lo6" engine, build the weights'
        e2m3 images and tile workspaces NOW -- a shortage of device memory is this call's error, not a scoring call's (blim.h: blim_reserve looks at the engine's
        compensated state, which the scoring paths only switch on around each call)."""
        if compensated and self.can_precise:
            self.set_precise(True, embeds=True, mlp=True)
            try:
                _check(self.lib.blim_reserve(self.h, max_tokens, max_rows), "blim_reserve")
            finally:
                self.set_precise(False)
        else:
            _check(self.lib.blim_reserve(self.h, max_tokens, max_rows), "blim_reserve")

    def set_option(self, key: str, value: int):
        _check(self.lib.blim_set_option(self.h, key.encode(), value), "blim_set_option")
        if key == "precise_lo6":
            self.lo6 = self._lo6_live = bool(value)

    @property
    def can_precise(self) -> bool:
        return self.dtype in ("f16", "bf16")

    def set_precise(self, on: bool, embeds: bool = False, mlp: bool = True, tvg: bool = False, layers: bool = False):
        """Compensated mode for the following calls (16-bit engines; a no-op request on others): every 16-bit activation travels as hi + lo and the GEMMs take
        both parts (fp16 engines: the lo part on the e2m3 MFMA, option "precise_lo6").  The host turns it on for the TVG calls, whose scores are ~10x smaller in
        magnitude than the VTG ones, and for the VTG calls of checkpoints that need it (`--vtg_precise`).
        embeds=True: the input embeddings (assemble -> decode / score_*) are [hi | lo] rows of width 2H as well -- the fused path, whose projected video features
        are produced in this mode; the literal forward() keeps [B, L, H] embeddings.  mlp=False: only the attention branch (QKV, attention, o_proj) and the
        scored rows are compensated -- the TVG calls' "attn" mode.  tvg=True: the call is a TVG call -- on a bf16 engine that was asked for the e2m3 second pass
        (`second_pass = "e2m3"`, round 6) it still takes the bf16 second pass: TVG scores are ~10x smaller in magnitude, read 1.7 - 2.6e-4 with the e2m3 pass against
        1 - 2.4e-5 with the bf16 one at 7B depth, and cost a few percent of an evaluation either way.  layers=True (VTG calls under `--vtg_precise select`): the call
        follows the per-layer mask of set_layer_mask (when one is set) instead of `mlp`."""
        on = bool(on) and self.can_precise
        embeds = bool(embeds) and on
        want6 = bool(self.lo6) and not (bool(tvg) and on and self.dtype == "bf16")
        if want6 != getattr(self, "_lo6_live", bool(self.lo6)):
            _check(self.lib.blim_set_option(self.h, b"precise_lo6", int(want6)), "blim_set_option")
            self._lo6_live = want6
        if on != getattr(self, "_precise", False):
            self.set_option("precise", int(on))
            self._precise = on
        if embeds != getattr(self, "_precise_embeds", False):
            self.set_option("precise_embeds", int(embeds))
            self._precise_embeds = embeds
        mlp = bool(mlp)
        if on and mlp != getattr(self, "_precise_mlp", True):
            self.set_option("precise_mlp", int(mlp))
            self._precise_mlp = mlp
        masked = bool(layers) and on and self._layer_mask is not None and not bool(tvg)
        if masked != getattr(self, "_precise_layers", False):
            self.set_option("precise_layers", int(masked))
            self._precise_layers = masked

    def set_layer_mask(self, bits):
        """Per-layer compensation mask of the VTG calls (`--vtg_precise select`; engine options "precise_layers" / "precise_layer_bits", include/blim.h): bits[l] says
        which units of layer l run compensated -- bit 0 QKV + attention, 1 o_proj, 2 gate|up, 3 down; uint8 [num_layers], or None for no mask.  Takes effect on the
        calls that set_precise(..., layers=True) brackets (the VTG calls); the TVG calls never use it."""
        if bits is None:
            self._layer_mask = None
            return
        if not self.can_precise:
            raise BlimError("set_layer_mask: fp8 engines have no compensated modes")
        bits = np.asarray(bits).astype(np.int64).reshape(-1)
        if bits.shape != (self.dims.num_layers,) or np.any(bits < 0) or np.any(bits > 15):
            raise ValueError(f"set_layer_mask: {self.dims.num_layers} values in 0 .. 15 expected, got {bits.tolist()}")
        live = self._layer_bits_live if self._layer_bits_live is not None else np.full(self.dims.num_layers, 15, dtype=np.int64)
        for li in np.nonzero(bits != live)[0]:
            _check(self.lib.blim_set_option(self.h, b"precise_layer_bits", int((int(li) << 4) | int(bits[li]))), "blim_set_option")
        self._layer_bits_live = bits.copy()
        self._layer_mask = bits.astype(np.uint8)

    @property
    def layer_mask(self):
        return None if self._layer_mask is None else self._layer_mask.copy()

    # ---- component ops (torch device tensors in/out)
    def project_video(self, feats, which: int):
        import torch
        n = feats.shape[0]
        out = torch.empty((n, self.dims.hidden_size * (2 if getattr(self, "_precise", False) else 1)), dtype=self.torch_dtype, device=self.device)
        _check(self.lib.blim_project_video(self.h, _ptr(feats), n, which, _ptr(out), _stream()), "blim_project_video")
        return out

    def group_mean(self, x, group: int):
        import torch
        n_out = x.shape[0] // group
        out = torch.empty((n_out, x.shape[1]), dtype=self.torch_dtype, device=self.device)
        _check(self.lib.blim_group_mean(self.h, _ptr(x), n_out, group, _ptr(out), _stream()), "blim_group_mean")
        return out

    def assemble(self, src_index, feats=None):
        import torch
        n = src_index.shape[0]
        out = torch.empty((n, self.dims.hidden_size * (2 if getattr(self, "_precise_embeds", False) else 1)), dtype=self.torch_dtype, device=self.device)
        _check(self.lib.blim_assemble(self.h, _ptr(src_index), n, _ptr(feats), _ptr(out), _stream()), "blim_assemble")
        return out

    def decode(self, batch: PackedBatch, embeds, out_rows=None, want_f32=False, want_bf16=True):
        import torch
        n = batch.n_tokens if out_rows is None else out_rows.shape[0]
        H = self.dims.hidden_size
        ob = torch.empty((n, H), dtype=self.torch_dtype, device=self.device) if want_bf16 else None
        of = torch.empty((n, H), dtype=torch.float32, device=self.device) if want_f32 else None
        bs = batch.struct(self.max_positions)
        _check(self.lib.blim_decode(self.h, C.byref(bs), _ptr(embeds), _ptr(out_rows), n, _ptr(ob), _ptr(of), _stream()), "blim_decode")
        return ob, of

    def vtg_logprobs(self, hidden_bf16, labels):
        import torch
        n = hidden_bf16.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        _check(self.lib.blim_vtg_logprobs(self.h, _ptr(hidden_bf16), _ptr(labels), n, _ptr(out), _stream()), "blim_vtg_logprobs")
        return out

    def tvg_logits(self, vh_bf16, vocab_clip_major, n_pairs: int):
        import torch
        out = torch.empty((n_pairs, self.dims.num_clips, vocab_clip_major.shape[1]), dtype=torch.float32, device=self.device)
        _check(self.lib.blim_tvg_logits(self.h, _ptr(vh_bf16), _ptr(vocab_clip_major), vocab_clip_major.shape[1], n_pairs, _ptr(out), _stream()),
               "blim_tvg_logits")
        return out

    def set_video_vocab(self, video_vocab):
        """video_vocab [N, clips, M] (any float dtype, host or device): registered with the engine as hi + lo 16-bit operands (blim_set_video_vocab);
        score_tvg / tvg_scores / tvg_logits called without a vocabulary then use it."""
        import torch
        v = torch.as_tensor(video_vocab).to(device=self.device, dtype=torch.float32).permute(1, 0, 2).contiguous()      # clip-major [clips, N, M]
        assert v.shape[0] == self.dims.num_clips and v.shape[2] == self.dims.mm_hidden_size, tuple(v.shape)
        _check(self.lib.blim_set_video_vocab(self.h, _ptr(v), int(v.shape[1]), _stream()), "blim_set_video_vocab")
        self.n_vocab = int(v.shape[1])
        self._vocab_key = vocab_key_of(video_vocab)

    def tvg_logits_f32(self, vh_f32, n_pairs: int):
        """vh_f32 [n_pairs * clips, M] float32 -> logits [n_pairs, clips, n_vocab] against the registered vocabulary (three-term compensated product)."""
        import torch
        out = torch.empty((n_pairs, self.dims.num_clips, self.n_vocab), dtype=torch.float32, device=self.device)
        _check(self.lib.blim_tvg_logits_f32(self.h, _ptr(vh_f32), n_pairs, _ptr(out), _stream()), "blim_tvg_logits_f32")
        return out

    def lm_head(self, hidden_bf16):
        import torch
        n = hidden_bf16.shape[0]
        out = torch.empty((n, self.dims.vocab_size), dtype=torch.float32, device=self.device)
        _check(self.lib.blim_lm_head(self.h, _ptr(hidden_bf16), n, _ptr(out), _stream()), "blim_lm_head")
        return out

    def visual_head(self, hidden_bf16):
        import torch
        n = hidden_bf16.shape[0]
        out = torch.empty((n, self.dims.mm_hidden_size), dtype=self.torch_dtype, device=self.device)
        _check(self.lib.blim_visual_head(self.h, _ptr(hidden_bf16), n, _ptr(out), _stream()), "blim_visual_head")
        return out

    def visual_head_f32(self, hidden_f32):
        """float32 [n, H] -> float32 [n, M]: head and hidden rows as hi + lo 16-bit operands (blim_visual_head_f32)."""
        import torch
        n = hidden_f32.shape[0]
        out = torch.empty((n, self.dims.mm_hidden_size), dtype=torch.float32, device=self.device)
        _check(self.lib.blim_visual_head_f32(self.h, _ptr(hidden_f32), n, _ptr(out), _stream()), "blim_visual_head_f32")
        return out

    def tvg_scores(self, vh_bf16, vocab_clip_major, labels):
        """vh [n_pairs*clips, M] bf16; vocab [clips, n_vocab, M] bf16; labels [n_pairs] int32."""
        import torch
        n_pairs = labels.shape[0]
        out = torch.empty(n_pairs, dtype=torch.float32, device=self.device)
        _check(self.lib.blim_tvg_scores(self.h, _ptr(vh_bf16), _ptr(vocab_clip_major), vocab_clip_major.shape[1], _ptr(labels), n_pairs,
                                        _ptr(out), _stream()), "blim_tvg_scores")
        return out

    def _score(self, name: str, batch: PackedBatch, embeds, rows, tail, n_pairs: int, cache=None, pfx_slot=None, slots_used=(), admits=None):
        """blim_score_<vtg | tvg>, or its _cached form when a PrefixCache is given, or its _admit form when that call also captures prefixes (admits: host ints
        [n_admit, 5] = (seq, slot, start, len, row), blim.h: blim_pc_admit): the output buffer and the arguments the forms share.  tail: the entry's own arguments
        between `rows` and `n_pairs`."""
        import torch
        out = torch.empty(n_pairs, dtype=torch.float32, device=self.device)
        bs = batch.struct(self.max_positions)
        head = (self.h, C.byref(bs))
        if cache is not None:
            su = np.ascontiguousarray(slots_used, dtype=np.int32)
            name, head = name + "_cached", (self.h, cache.h, C.byref(bs), _ptr(pfx_slot), su.ctypes.data if len(su) else None, len(su))
            if admits is not None and len(admits):
                ad = np.ascontiguousarray(admits, dtype=np.int32).reshape(-1, 5)
                name, head = name[:-len("_cached")] + "_admit", head + (ad.ctypes.data, len(ad))
        _check(getattr(self.lib, name)(*head, _ptr(embeds), _ptr(rows), *tail, n_pairs, _ptr(out), _stream()), name)
        return out

    def score_vtg(self, batch: PackedBatch, embeds, rows, labels, row_start, **cached):
        return self._score("blim_score_vtg", batch, embeds, rows, (_ptr(labels), rows.shape[0], _ptr(row_start)), row_start.shape[0] - 1, **cached)

    # ---- gallery prefix cache (blim.h: blim_prefix_cache_*; blim_amd/prefix_index.py)
    def prefix_cache_bytes(self, n_slots: int, max_len: int, compensated: bool) -> int:
        return int(self.lib.blim_prefix_cache_bytes(self.h, int(n_slots), int(max_len), int(bool(compensated))))

    def prefix_cache(self, n_slots: int, max_len: int, compensated: bool) -> "PrefixCache":
        return PrefixCache(self, n_slots, max_len, compensated)

    def score_tvg(self, batch: PackedBatch, embeds, rows, vocab_clip_major, labels, **cached):
        """vocab_clip_major None: the vocabulary registered with set_video_vocab()."""
        n_vocab = self.n_vocab if vocab_clip_major is None else vocab_clip_major.shape[1]
        return self._score("blim_score_tvg", batch, embeds, rows, (_ptr(vocab_clip_major), n_vocab, _ptr(labels)), labels.shape[0], **cached)

    def score_tvg_first(self, batch: PackedBatch, embeds, rows, k: int, prior_rows=None, prior_of=None, alpha: float = 0.0, full: bool = False):
        """blim_score_tvg_first: rows int32 [n] (device) name the caption prompts' last tokens, prior_rows int32 [n_prior] the prior sequences' scored tokens,
        prior_of int32 [n] row r's prior row (< 0: none) -> (idx int32 [n, k], val f32 [n, k][, lp f32 [n, n_vocab] with full]): the best k VOCABULARY entries
        of log P(clip 0 | text) (- alpha * the prior's) in the stable descending order, ranked on the device."""
        import torch
        n = int(rows.shape[0])
        n_prior = 0 if prior_rows is None else int(prior_rows.shape[0])
        idx = torch.empty((n, int(k)), dtype=torch.int32, device=self.device)
        val = torch.empty((n, int(k)), dtype=torch.float32, device=self.device)
        lp = torch.empty((n, self.n_vocab), dtype=torch.float32, device=self.device) if full else None
        bs = batch.struct(self.max_positions)
        _check(self.lib.blim_score_tvg_first(self.h, C.byref(bs), _ptr(embeds), _ptr(rows), n, _ptr(prior_rows) if n_prior else None, n_prior, _ptr(prior_of),
                                             float(alpha), int(k), _ptr(idx), _ptr(val), _ptr(lp), _stream()), "blim_score_tvg_first")
        return (idx, val, lp) if full else (idx, val)

    def score_tvg_first_within(self, batch: PackedBatch, embeds, rows, k: int, row_of, within, within_off, prior_rows=None, prior_of=None, alpha: float = 0.0,
                               n_within: Optional[int] = None):
        """blim_score_tvg_first_within: score_tvg_first's rows / prior_rows; per QUERY q (device int32): row_of [n_q] its row of `rows`, prior_of [n_q] its prior row
        (< 0: none), within[within_off[q] .. within_off[q + 1]) its list of vocabulary entries -> (idx int32 [n_q, k], val f32 [n_q, k]): the best min(k, m_q)
        POSITIONS of q's list by the whole-vocabulary term, then -1 / NaN.  n_within: the entries of `within` that count (default: all of them)."""
        import torch
        n = int(rows.shape[0])
        n_q = int(within_off.shape[0]) - 1
        n_prior = 0 if prior_rows is None else int(prior_rows.shape[0])
        idx = torch.empty((max(n_q, 0), int(k)), dtype=torch.int32, device=self.device)
        val = torch.empty((max(n_q, 0), int(k)), dtype=torch.float32, device=self.device)
        bs = batch.struct(self.max_positions)
        _check(self.lib.blim_score_tvg_first_within(self.h, C.byref(bs), _ptr(embeds), _ptr(rows), n, _ptr(prior_rows) if n_prior else None, n_prior, n_q,
                                                    _ptr(row_of), _ptr(prior_of), _ptr(within), _ptr(within_off), int(within.shape[0] if n_within is None else n_within), float(alpha), int(k),
                                                    _ptr(idx), _ptr(val), _stream()), "blim_score_tvg_first_within")
        return idx, val

    def rank_rows(self, values, k: int):
        """blim_rank_rows over a device f32 [n_rows, n] -> (idx int32 [n_rows, k], val f32 [n_rows, k]): the first k of every row in blim_tvg_rank's order."""
        import torch
        n_rows = int(values.shape[0])
        idx = torch.empty((n_rows, int(k)), dtype=torch.int32, device=self.device)
        val = torch.empty((n_rows, int(k)), dtype=torch.float32, device=self.device)
        rank_rows(values, int(values.shape[1]), int(k), idx, val)
        return idx, val

    def forward(self, embeds, mask, want_logits=True, want_hidden=True):
        """Literal forward: embeds [B,L,H] bf16, mask [B,L] uint8 -> (logits f32 [B,L,V] | None, hidden f32 [B,L,H] | None)."""
        import torch
        B, L, H = embeds.shape
        if getattr(self, "_precise_embeds", False):        # [hi | lo] rows of width 2 * hidden (compensated mode with split embeddings)
            H //= 2
        lg = torch.empty((B, L, self.dims.vocab_size), dtype=torch.float32, device=self.device) if want_logits else None
        hd = torch.empty((B, L, H), dtype=torch.float32, device=self.device) if want_hidden else None
        _check(self.lib.blim_forward(self.h, _ptr(embeds), _ptr(mask), B, L, _ptr(lg), _ptr(hd), _stream()), "blim_forward")
        return lg, hd

    def debug_read(self, which: str, shape, dtype):
        """Copy of an internal workspace as the last decode left it (bring-up aid)."""
        import torch
        out = torch.empty(shape, dtype=dtype, device=self.device)
        _check(self.lib.blim_debug_read(self.h, which.encode(), _ptr(out), out.numel() * out.element_size(), _stream()), "blim_debug_read")
        return out

    # ---- timing
    def timing_enable(self, on: bool):
        _check(self.lib.blim_timing_enable(self.h, int(on)), "blim_timing_enable")

    def timing_report(self) -> Dict[str, Dict[str, float]]:
        n = self.lib.blim_timing_num_classes()
        ms = (C.c_double * n)(); calls = (C.c_int64 * n)(); fl = (C.c_double * n)()
        _check(self.lib.blim_timing_report(self.h, ms, calls, fl), "blim_timing_report")
        return {self.lib.blim_timing_class_name(i).decode(): {"ms": ms[i], "calls": int(calls[i]), "flops": fl[i]} for i in range(n)}


PC_TICKET_LAYERS = 256


class PcMove(C.Structure):
    """blim.h: blim_pc_move."""
    _fields_ = [("slot", C.c_int32), ("len", C.c_int32), ("offset", C.c_int64)]


class PcTicket(C.Structure):
    """blim.h: blim_pc_ticket -- what an exported slot needs to come back: its length, the state it was computed under, the record's geometry."""
    _fields_ = [("magic", C.c_uint32), ("len", C.c_int32), ("num_layers", C.c_int32), ("kv_w", C.c_int32), ("hid_w", C.c_int32),
                ("precise", C.c_int32), ("embeds", C.c_int32), ("mlp", C.c_int32), ("layers", C.c_int32), ("lo6", C.c_int32), ("mqz", C.c_int32), ("n_bits", C.c_int32),
                ("epoch", C.c_uint64), ("bits", C.c_uint8 * PC_TICKET_LAYERS)]


def _pc_moves(moves):
    """[(slot, len, offset)] -> a blim_pc_move array."""
    arr = (PcMove * max(len(moves), 1))()
    for k, (slot, ln, off) in enumerate(moves):
        arr[k].slot, arr[k].len, arr[k].offset = int(slot), int(ln), int(off)
    return arr


class PrefixCache:
    """Device-resident K / V + last-row hidden state of prefixes (blim.h: blim_prefix_cache_*), one slot per prefix: VTG video prefixes or TVG caption prompts."""

    def __init__(self, engine: Engine, n_slots: int, max_len: int, compensated: bool):
        self.engine, self.lib = engine, engine.lib
        self.n_slots, self.max_len, self.compensated = int(n_slots), int(max_len), bool(compensated)
        self.bytes = engine.prefix_cache_bytes(n_slots, max_len, compensated)
        h = C.c_void_p()
        _check(self.lib.blim_prefix_cache_create(engine.h, self.n_slots, self.max_len, int(self.compensated), C.byref(h)), "blim_prefix_cache_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.blim_prefix_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fill(self, batch: PackedBatch, embeds, slot_of_seq):
        """batch: prefix sequences only; slot_of_seq: host int [n_seqs]."""
        sl = np.ascontiguousarray(slot_of_seq, dtype=np.int32)
        assert len(sl) == batch.n_seqs
        bs = batch.struct(self.engine.max_positions)
        _check(self.lib.blim_prefix_cache_fill(self.engine.h, self.h, C.byref(bs), _ptr(embeds), sl.ctypes.data, _stream()), "blim_prefix_cache_fill")

    def slot_len(self, slot: int) -> int:
        return int(self.lib.blim_prefix_cache_slot_len(self.h, int(slot)))

    # ---- slot export / import (blim.h: blim_prefix_cache_export / _import; blim_amd/prefix_index.py: HostTier)
    def record_bytes(self, length: int) -> int:
        """Bytes of the packed record of a slot with `length` filled positions (a multiple of 256; -1: length outside 1 .. max_len)."""
        return int(self.lib.blim_prefix_cache_record_bytes(self.h, int(length)))

    def export_slots(self, moves, staging) -> List["PcTicket"]:
        """moves [(slot, len, offset)]: each slot's packed record is written at `offset` bytes into staging (device uint8) -> one ticket per move, for import_slots.
        Stream-ordered; never waits for the device."""
        mv, tk = _pc_moves(moves), (PcTicket * max(len(moves), 1))()
        _check(self.lib.blim_prefix_cache_export(self.engine.h, self.h, mv, len(moves), _ptr(staging), staging.numel() * staging.element_size(), tk, _stream()),
               "blim_prefix_cache_export")
        out = []
        for k in range(len(moves)):
            t = PcTicket()
            C.memmove(C.byref(t), C.byref(tk[k]), C.sizeof(PcTicket))
            out.append(t)
        return out

    def import_slots(self, moves, staging, tickets):
        """The reverse: the records at the moves' offsets in staging become the moves' slots, under the state their tickets recorded."""
        assert len(tickets) == len(moves)
        mv, tk = _pc_moves(moves), (PcTicket * max(len(moves), 1))()
        for k, t in enumerate(tickets):
            C.memmove(C.byref(tk[k]), C.byref(t), C.sizeof(PcTicket))
        _check(self.lib.blim_prefix_cache_import(self.engine.h, self.h, mv, len(moves), _ptr(staging), staging.numel() * staging.element_size(), tk, _stream()),
               "blim_prefix_cache_import")

    def score_vtg(self, batch: PackedBatch, pfx_slot, slots_used, embeds, rows, labels, row_start, admits=None):
        """blim_score_vtg_cached: pfx_slot device int32 [n_seqs] (-1: in-batch prefix); slots_used host ints (every slot read); rows[r] < 0: slot -(rows[r] + 1)'s hidden row.
        admits (host ints [n_admit, 5] = (seq, slot, start, len, row); non-empty: blim_score_vtg_admit): in-batch prefix sequences the call also captures into slots."""
        return self.engine.score_vtg(batch, embeds, rows, labels, row_start, cache=self, pfx_slot=pfx_slot, slots_used=slots_used, admits=admits)

    def score_tvg(self, batch: PackedBatch, pfx_slot, slots_used, embeds, rows, vocab_clip_major, labels, admits=None):
        """blim_score_tvg_cached (non-empty admits: blim_score_tvg_admit): Engine.score_tvg with the slot conventions of score_vtg above (a slot holds a caption prompt;
        its hidden row predicts clip 0)."""
        return self.engine.score_tvg(batch, embeds, rows, vocab_clip_major, labels, cache=self, pfx_slot=pfx_slot, slots_used=slots_used, admits=admits)

    def tvg_first_cols(self, slots, cols, chunk_rows: int = 0):
        """blim_tvg_first_cached: slots host ints [n_slots] (caption prompts), cols device int32 [n_cols] (vocabulary entries) -> device f32 [n_cols, n_slots],
        out[c][q] = log P(clip 0 of entry cols[c] | the prompt in slots[q]), from the slots' stored hidden rows: no decode.  chunk_rows 0: the engine's default."""
        import torch
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        out = torch.empty((int(cols.shape[0]), len(sl)), dtype=torch.float32, device=self.engine.device)
        _check(self.lib.blim_tvg_first_cached(self.engine.h, self.h, sl.ctypes.data, len(sl), _ptr(cols), int(cols.shape[0]), _ptr(out), len(sl), int(chunk_rows),
                                              _stream()), "blim_tvg_first_cached")
        return out


def ce_rows(logits, labels, V: Optional[int] = None):
    """logprob[r] = log_softmax(logits[r, :V])[labels[r]] (0 where labels[r] < 0); logits f32 [n, ld], labels int32 [n]; V = ld unless given."""
    import torch
    lib = load_library()
    n, ld = logits.shape
    out = torch.empty(n, dtype=torch.float32, device=logits.device)
    _check(lib.blim_ce_rows(None, _ptr(logits), ld, ld if V is None else V, _ptr(labels), n, _ptr(out), _stream()), "blim_ce_rows")
    return out


# ---- the scoring path's row kernels alone (tests; include/blim.h): pass-throughs to the launchers of csrc/kernels.hip over caller-owned device tensors.
def rmsnorm(x, w, eps: float, n_rows: int, H: int, dtype: str, ldx: Optional[int] = None, rows=None, n_src: int = 0, out16=None, ldo: int = 0, out_lo=None,
            lo_offset: Optional[int] = None, out_f32=None, saturate: bool = True, out6=None):
    """blim_rmsnorm: x f32 [*, ldx], w f32 [H]; out16 16-bit rows of stride ldo (0 = H), out_lo a tensor of its own or, with lo_offset, that many 16-bit elements
    into out16 (the [hi | lo] rows of the compensated mode); out_f32 f32 [n_rows, H]; out6 uint8 [f6_tiles_bytes(n_rows, H)]."""
    a = RmsnormArgs()
    a.struct_bytes = C.sizeof(RmsnormArgs)
    a.x = _ptr(x); a.ldx = x.shape[1] if ldx is None else ldx; a.rows = _ptr(rows); a.n_rows = n_rows; a.n_src = n_src; a.H = H; a.dtype16 = COMPUTE_DTYPES[dtype]
    a.w = _ptr(w); a.eps = eps; a.saturate = int(saturate); a.out16 = _ptr(out16); a.ldo = ldo
    a.out_lo = _ptr(out16) + 2 * lo_offset if lo_offset is not None else _ptr(out_lo)
    a.out_f32 = _ptr(out_f32); a.out6 = _ptr(out6)
    _check(load_library().blim_rmsnorm(C.byref(a), _stream()), "blim_rmsnorm")


def f6_tiles_bytes(n_rows: int, K: int) -> int:
    return int(load_library().blim_f6_tiles_bytes(n_rows, K))


def rmsnorm_f8(x, w, eps: float, n_rows: int, H: int, out8, scale, ldx: Optional[int] = None):
    """blim_rmsnorm_f8: out8 uint8 [n_rows, H] e4m3 bytes, scale f32 [n_rows]."""
    _check(load_library().blim_rmsnorm_f8(_ptr(x), x.shape[1] if ldx is None else ldx, n_rows, H, _ptr(w), eps, _ptr(out8), _ptr(scale), _stream()), "blim_rmsnorm_f8")


def lse_combine(part, label_logit, labels, logprob):
    """blim_lse_combine: part f32 [n_rows, n_tiles, 2] = (max, sum exp) partials; logprob f32 [>= n_rows] is written."""
    n_rows, n_tiles = part.shape[0], part.shape[1]
    _check(load_library().blim_lse_combine(_ptr(part), n_tiles, _ptr(label_logit), _ptr(labels), n_rows, _ptr(logprob), _stream()), "blim_lse_combine")


def tvg_criterion(logits, n_vocab: int, labels, n_pairs: int, clips: int, score):
    """blim_tvg_criterion: logits f32 [n_pairs * clips, ld], labels int32 [n_pairs]; score f32 [>= n_pairs] is written."""
    _check(load_library().blim_tvg_criterion(_ptr(logits), logits.shape[1], n_vocab, _ptr(labels), n_pairs, clips, _ptr(score), _stream()), "blim_tvg_criterion")


def tvg_rank(logits, n_vocab: int, k: int, idx_out, val_out, prior_logits=None, prior_of=None, alpha: float = 0.0, logprob_out=None, n_rows: Optional[int] = None,
             n_prior: Optional[int] = None):
    """blim_tvg_rank: logits f32 [n_rows, ld] (prior_logits f32 [n_prior, ld_prior], prior_of int32 [n_rows]); idx_out int32 / val_out f32 [>= n_rows * k] and the
    optional logprob_out f32 [n_rows, ld_out] are written."""
    _check(load_library().blim_tvg_rank(_ptr(logits), 0 if logits is None else logits.shape[1], n_vocab, logits.shape[0] if n_rows is None else n_rows, _ptr(prior_logits),
                                        0 if prior_logits is None else prior_logits.shape[1], (0 if prior_logits is None else prior_logits.shape[0]) if n_prior is None else n_prior,
                                        _ptr(prior_of), float(alpha), k, _ptr(idx_out), _ptr(val_out), _ptr(logprob_out), 0 if logprob_out is None else logprob_out.shape[1],
                                        _stream()), "blim_tvg_rank")


def tvg_rank_within(logits, n_vocab: int, k: int, within, within_off, idx_out, val_out, row_of=None, prior_logits=None, prior_of=None, alpha: float = 0.0,
                    n_rows: Optional[int] = None, n_prior: Optional[int] = None, n_q: Optional[int] = None, n_within: Optional[int] = None):
    """blim_tvg_rank_within: logits f32 [n_rows, ld]; per query q (device int32) row_of [n_q] (None: q), prior_of [n_q], within[within_off[q] .. within_off[q + 1]);
    idx_out int32 / val_out f32 [>= n_q * k] are written: positions into q's list and the terms' bits, -1 / NaN from the list's length on."""
    _check(load_library().blim_tvg_rank_within(_ptr(logits), 0 if logits is None else logits.shape[1], n_vocab, logits.shape[0] if n_rows is None else n_rows,
                                               _ptr(prior_logits), 0 if prior_logits is None else prior_logits.shape[1],
                                               (0 if prior_logits is None else prior_logits.shape[0]) if n_prior is None else n_prior,
                                               (within_off.shape[0] - 1) if n_q is None else n_q, _ptr(row_of), _ptr(prior_of), _ptr(within), _ptr(within_off),
                                               (0 if within is None else within.shape[0]) if n_within is None else n_within, float(alpha), k, _ptr(idx_out),
                                               _ptr(val_out), _stream()), "blim_tvg_rank_within")


def tvg_cols(logits, n_vocab: int, cols, out, out0: int = 0, n_rows: Optional[int] = None, n_cols: Optional[int] = None):
    """blim_tvg_cols: logits f32 [n_rows, ld], cols int32 [n_cols] (device); out f32 [n_cols, ld_out]: out[c, out0 + r] = log_softmax(logits[r, :n_vocab])[cols[c]]."""
    _check(load_library().blim_tvg_cols(_ptr(logits), 0 if logits is None else logits.shape[1], n_vocab, logits.shape[0] if n_rows is None else n_rows, _ptr(cols),
                                        cols.shape[0] if n_cols is None else n_cols, _ptr(out), 0 if out is None else out.shape[1], out0, _stream()), "blim_tvg_cols")


def rank_rows(values, n: int, k: int, idx_out, val_out, n_rows: Optional[int] = None):
    """blim_rank_rows: values f32 [n_rows, ld]; idx_out int32 / val_out f32 [>= n_rows * k] are written: the first k of blim_tvg_rank's order on the given values."""
    _check(load_library().blim_rank_rows(_ptr(values), 0 if values is None else values.shape[1], n, values.shape[0] if n_rows is None else n_rows, k, _ptr(idx_out),
                                         _ptr(val_out), _stream()), "blim_rank_rows")


def group_mean_rows(out, inp, n_out: int, group: int, H: int, dtype: str, split: bool = False):
    """blim_group_mean_rows: inp 16-bit [n_out * group, H] (split: 2 H) -> out [n_out, H] (split: 2 H)."""
    _check(load_library().blim_group_mean_rows(_ptr(out), _ptr(inp), n_out, group, H, COMPUTE_DTYPES[dtype], int(split), _stream()), "blim_group_mean_rows")


def assemble_rows(out, src_index, n_tokens: int, H: int, table, feats, split: bool = False):
    """blim_assemble_rows: out[t] = table[src[t]] (src[t] >= 0) or feats[-(src[t] + 1)]; split: out / feats rows are [hi | lo] of width 2 H."""
    _check(load_library().blim_assemble_rows(_ptr(out), _ptr(src_index), n_tokens, H, _ptr(table), _ptr(feats), int(split), _stream()), "blim_assemble_rows")


def segment_mean(logprob, row_start, mode: int = 0):
    """mode 0: sum / count_nonzero (VTG), mode 1: plain mean (TVG)."""
    import torch
    lib = load_library()
    n = row_start.shape[0] - 1
    out = torch.empty(n, dtype=torch.float32, device=logprob.device)
    _check(lib.blim_segment_mean(None, _ptr(logprob), _ptr(row_start), n, mode, _ptr(out), _stream()), "blim_segment_mean")
    return out


def hash_device(t, nbytes: Optional[int] = None):
    """(d1, d2): content hash of a contiguous device tensor's bytes (or its first `nbytes`), blim_hash_device -- calibration_store.hash_bytes states it in numpy."""
    lib = load_library()
    n = t.numel() * t.element_size() if nbytes is None else int(nbytes)
    assert t.is_cuda and t.is_contiguous() and 0 <= n <= t.numel() * t.element_size()
    out = (C.c_uint64 * 2)()
    _check(lib.blim_hash_device(_ptr(t), n, out, _stream()), "blim_hash_device")
    return int(out[0]), int(out[1])


def fill_bell_bf16(out, seed: int, name: str, std: float, mean: float = 0.0):
    lib = load_library()
    _check(lib.blim_fill_bell_bf16(_ptr(out), out.numel(), seed, name.encode(), std, mean, _stream()), "blim_fill_bell_bf16")
    return out


def quant_rows(x):
    """x [M,K] bf16/f16 -> (e4m3 bytes as uint8 [M,K], f32 scale [M] = absmax / 448)."""
    import torch
    lib = load_library()
    M, K = x.shape
    q = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    _check(lib.blim_quant_rows(_ptr(x), x.stride(0), M, K, 0 if x.dtype == torch.bfloat16 else 1, _ptr(q), _ptr(sc), _stream()), "blim_quant_rows")
    return q, sc


def gemm_f8(a8, a_scale, w8, w_scale):
    """(a8 [M,K] . w8 [N,K]^T) * a_scale[m] * w_scale[n] -> f16 [M,N]; a8 / w8 hold e4m3 bytes (uint8)."""
    import torch
    lib = load_library()
    M, K = a8.shape
    N = w8.shape[0]
    out = torch.empty((M, N), dtype=torch.float16, device=a8.device)
    _check(lib.blim_gemm_f8(_ptr(a8), K, _ptr(a_scale), _ptr(w8), _ptr(w_scale), M, N, K, _ptr(out), N, _stream()), "blim_gemm_f8")
    return out


def gemm_f16_lo6(a_hilo, w):
    """The compensated GEMM of fp16 engines (option "precise_lo6"): a_hilo [M, 2K] f16 rows [hi | lo], w [N, K] f16 -> (C f32 [M, N] = hi . w^T + e2m3(lo) . e2m3(w)^T,
    the e2m3 operand tiles of lo and of w as uint8 [row tiles, K / 128, 25600] -- layout: csrc/gemm.hpp)."""
    import torch
    lib = load_library()
    M, K2 = a_hilo.shape
    N, K = w.shape
    assert K2 == 2 * K and a_hilo.dtype == torch.float16 and w.dtype == torch.float16 and a_hilo.is_contiguous() and w.is_contiguous()
    a6 = torch.empty(lib.blim_f6_tiles_bytes(M, K), dtype=torch.uint8, device=w.device)
    w6 = torch.empty(lib.blim_f6_tiles_bytes(N, K), dtype=torch.uint8, device=w.device)
    out = torch.empty((M, N), dtype=torch.float32, device=w.device)
    _check(lib.blim_gemm_f16_lo6(_ptr(a_hilo), _ptr(w), M, N, K, _ptr(a6), _ptr(w6), _ptr(out), _stream()), "blim_gemm_f16_lo6")
    return out, a6.view(-1, K // 128, 25600), w6.view(-1, K // 128, 25600)


def attention(qkv, batch: PackedBatch, num_heads: int, num_kv_heads: int, out, scale: float = 128 ** -0.5, use_tr_read: int = 1, v_lo_off: int = 0,
              out_lo_off: int = 0, lse_out=None, out8=None, out_mx=None, mx_stride: int = 0, pfx_cache=None, pfx_slot=None, pc_slot_stride: int = 0,
              pc_ld: int = 0, pc_lo_off: int = 0, pc_n_slots: int = 0, pc_max_len: int = 0):
    """The decoder's attention kernel alone (blim_attention): qkv 16-bit [T, ldq] rows [q | k | v (| lo parts at +v_lo_off)], out 16-bit [T, ldo] written in place
    (hi | lo at +out_lo_off); the row strides are the tensors' widths.  Optional: lse_out f32 [T, num_heads]; out8 uint8 [T, ldo8] + out_mx uint8 (fused e4m3 output);
    pfx_cache 16-bit + pfx_slot int32 [n_seqs] (the prefix-cache forms).  The fields are blim.h's blim_attention_args."""
    import torch
    lib = load_library()
    assert qkv.dim() == 2 and out.dim() == 2 and qkv.dtype == out.dtype and qkv.dtype in (torch.bfloat16, torch.float16)
    bs = batch.struct()
    a = AttentionArgs()
    a.struct_bytes = C.sizeof(AttentionArgs)
    a.batch = C.pointer(bs); a.qkv = _ptr(qkv); a.ldq = qkv.shape[1]; a.num_heads = num_heads; a.num_kv_heads = num_kv_heads
    a.dtype16 = COMPUTE_DTYPES["bf16" if qkv.dtype == torch.bfloat16 else "f16"]; a.use_tr_read = int(use_tr_read)
    a.v_lo_off = v_lo_off; a.out_lo_off = out_lo_off; a.out = _ptr(out); a.ldo = out.shape[1]; a.scale = scale
    a.lse_out = _ptr(lse_out); a.out8 = _ptr(out8); a.ldo8 = out8.shape[1] if out8 is not None else 0; a.out_mx = _ptr(out_mx); a.mx_stride = mx_stride
    a.pfx_cache = _ptr(pfx_cache); a.pfx_slot = _ptr(pfx_slot); a.pc_slot_stride = pc_slot_stride; a.pc_ld = pc_ld; a.pc_lo_off = pc_lo_off
    a.pc_n_slots = pc_n_slots; a.pc_max_len = pc_max_len
    _check(lib.blim_attention(C.byref(a), _stream()), "blim_attention")
    return out


def attention_bwd_workspace_bytes(n_tokens: int, n_seqs: int, num_heads: int, max_len: int) -> int:
    return int(load_library().blim_attention_bwd_workspace_bytes(n_tokens, n_seqs, num_heads, max_len))


def attention_bwd(qkv, dout, o16, lse, batch: PackedBatch, num_heads: int, num_kv_heads: int, max_len: int, dqkv, workspace, scale: float = 128 ** -0.5):
    """The trainer's attention backward alone (blim_attention_bwd): qkv / dout / o16 16-bit [T, ld*] (the row strides are the tensors' widths), lse f32
    [T, num_heads]; batch gives key_visible, seq_start, seq_len (no prefixes); dqkv f32 [T, ldq] is written in place on the sequences' rows; workspace: a uint8
    tensor of attention_bwd_workspace_bytes(T, n_seqs, num_heads, max_len) bytes or more.  The fields are blim.h's blim_attention_bwd_args."""
    import torch
    lib = load_library()
    assert qkv.dim() == 2 and dout.dim() == 2 and o16.dim() == 2 and dqkv.shape == qkv.shape and dqkv.dtype == torch.float32 and lse.dtype == torch.float32
    assert qkv.dtype == dout.dtype == o16.dtype and qkv.dtype in (torch.bfloat16, torch.float16) and workspace.dtype == torch.uint8
    a = AttentionBwdArgs()
    a.struct_bytes = C.sizeof(AttentionBwdArgs)
    a.qkv = _ptr(qkv); a.ldq = qkv.shape[1]; a.dout = _ptr(dout); a.ldo = dout.shape[1]; a.o16 = _ptr(o16); a.ldo16 = o16.shape[1]; a.lse = _ptr(lse)
    a.num_heads = num_heads; a.num_kv_heads = num_kv_heads; a.dtype16 = COMPUTE_DTYPES["bf16" if qkv.dtype == torch.bfloat16 else "f16"]
    a.key_visible = _ptr(batch.key_visible); a.seq_start = _ptr(batch.seq_start); a.seq_len = _ptr(batch.seq_len); a.n_seqs = batch.n_seqs; a.max_len = max_len
    a.scale = scale; a.workspace = _ptr(workspace); a.workspace_bytes = workspace.numel(); a.dqkv = _ptr(dqkv); a.n_tokens = qkv.shape[0]
    _check(lib.blim_attention_bwd(C.byref(a), _stream()), "blim_attention_bwd")
    return dqkv


def rope_bwd(dqkv, rope_cols: int, positions, cos, sin, out16):
    """blim_rope_bwd: dqkv f32 [T, qkv_n] -> out16 16-bit [T, qkv_n] (written in place), the inverse rotation on the columns < rope_cols; positions int32 [T],
    cos / sin f32 [n_pos, 64], all on the device."""
    import torch
    lib = load_library()
    assert dqkv.dim() == 2 and dqkv.dtype == torch.float32 and out16.dtype in (torch.bfloat16, torch.float16) and out16.numel() >= dqkv.numel()
    assert cos.shape == sin.shape and cos.shape[1] == 64 and cos.dtype == sin.dtype == torch.float32 and positions.dtype == torch.int32
    _check(lib.blim_rope_bwd(_ptr(out16), _ptr(dqkv), dqkv.shape[0], dqkv.shape[1], rope_cols, _ptr(positions), _ptr(cos), _ptr(sin), cos.shape[0],
                             COMPUTE_DTYPES["bf16" if out16.dtype == torch.bfloat16 else "f16"], _stream()), "blim_rope_bwd")
    return out16


# ---- the trainer's remaining kernels alone (include/blim.h: blim_lora_down .. blim_grad_stats_raw).  Tensors are device tensors written in place; `workspace` is a
# uint8 tensor of the entry's *_workspace_bytes(...) or more; `dtype` is "f16" / "bf16".  Row strides are explicit: the tests pad their rows.
def _dt16(t) -> int:
    import torch
    assert t.dtype in (torch.bfloat16, torch.float16)
    return COMPUTE_DTYPES["bf16" if t.dtype == torch.bfloat16 else "f16"]


def _ptr3(ts):
    arr = (C.c_void_p * 3)()
    for i, t in enumerate(ts):
        arr[i] = _ptr(t)
    return arr


def lora_down_workspace_bytes(n_adapters: int, K: int) -> int:
    return int(load_library().blim_lora_down_workspace_bytes(n_adapters, K))


def lora_down(x16, T: int, K: int, A: Sequence, r: int, scale: float, drop_p: float, seed: int, site: int, workspace, ldx: Optional[int] = None):
    """blim_lora_down: x16 16-bit [rows >= T, ldx], A a list of 1..3 f32 [r, K] tensors; columns K .. K + len(A) * r of rows < T are written."""
    a = LoraDownArgs()
    a.struct_bytes = C.sizeof(LoraDownArgs)
    a.x16 = _ptr(x16); a.ldx = x16.shape[1] if ldx is None else ldx; a.T = T; a.K = K; a.n_adapters = len(A); a.r = r; a.dtype16 = _dt16(x16)
    a.A = _ptr3(A); a.scale = scale; a.drop_p = drop_p; a.seed = seed; a.site = site
    a.workspace = _ptr(workspace); a.workspace_bytes = workspace.numel()
    _check(load_library().blim_lora_down(C.byref(a), _stream()), "blim_lora_down")
    return x16


def lora_grads_workspace_bytes(flags: int, T: int, N: int, K: int, r: int) -> int:
    return int(load_library().blim_lora_grads_workspace_bytes(flags, T, N, K, r))


def lora_grads(flags: int, T: int, r: int, workspace, dtype: str, N: int = 0, K: int = 0, dy16=None, ldy: int = 0, u16=None, ldu: int = 0, x16=None, ldx: int = 0,
               B=None, scale: float = 1.0, drop_p: float = 0.0, seed: int = 0, site: int = 0, dB=None, du=None, dA=None, u16_offset: int = 0):
    """blim_lora_grads: flags = LORA_DB | LORA_DU | LORA_DA.  u16_offset: u16 starts that many 16-bit elements into the tensor (the u~ columns of an augmented row)."""
    a = LoraGradsArgs()
    a.struct_bytes = C.sizeof(LoraGradsArgs)
    a.flags = flags; a.dtype16 = COMPUTE_DTYPES[dtype]; a.T = T; a.N = N; a.K = K; a.r = r
    a.dy16 = _ptr(dy16); a.ldy = ldy; a.u16 = None if u16 is None else _ptr(u16) + 2 * u16_offset; a.ldu = ldu; a.x16 = _ptr(x16); a.ldx = ldx; a.B = _ptr(B)
    a.scale = scale; a.drop_p = drop_p; a.seed = seed; a.site = site; a.dB = _ptr(dB); a.du = _ptr(du); a.dA = _ptr(dA)
    a.workspace = _ptr(workspace); a.workspace_bytes = workspace.numel()
    _check(load_library().blim_lora_grads(C.byref(a), _stream()), "blim_lora_grads")


def lora_dx(dx, T: int, K: int, du: Sequence, A: Sequence, r: int, drop_p: float, seed: int, site: int, out16=None, dtype: str = "f16"):
    """blim_lora_dx: dx f32 [rows >= T, ldd] (+)= the adapters' input gradient; with out16 ([rows, ldo] 16-bit) dx is only read."""
    a = LoraDxArgs()
    a.struct_bytes = C.sizeof(LoraDxArgs)
    a.dx = _ptr(dx); a.ldd = dx.shape[1]; a.T = T; a.K = K; a.n_adapters = len(A); a.r = r
    a.dtype16 = COMPUTE_DTYPES[dtype] if out16 is None else _dt16(out16)
    a.du = _ptr3(du); a.A = _ptr3(A); a.drop_p = drop_p; a.site = site; a.seed = seed; a.out16 = _ptr(out16); a.ldo = out16.shape[1] if out16 is not None else 0
    _check(load_library().blim_lora_dx(C.byref(a), _stream()), "blim_lora_dx")


def rmsnorm_bwd(dx, dy, x, w, eps: float, n_rows: int, H: int, rows=None, accumulate: int = 0, out16=None, dtype: str = "f16", du: Sequence = (), A: Sequence = (),
                r: int = 0, drop_p: float = 0.0, seed: int = 0, site: int = 0):
    """blim_rmsnorm_bwd: dx, x f32 [*, H], dy f32 [n_rows, H]; rows int32 [n_rows] (gather); out16 16-bit [*, H]; du / A: the fused adapters."""
    a = RmsnormBwdArgs()
    a.struct_bytes = C.sizeof(RmsnormBwdArgs)
    a.dx = _ptr(dx); a.dy = _ptr(dy); a.x = _ptr(x); a.rows = _ptr(rows); a.n_rows = n_rows; a.H = H; a.accumulate = accumulate; a.w = _ptr(w); a.eps = eps
    a.dtype16 = COMPUTE_DTYPES[dtype] if out16 is None else _dt16(out16)
    a.out16 = _ptr(out16); a.n_adapters = len(A); a.r = r; a.du = _ptr3(du); a.A = _ptr3(A); a.drop_p = drop_p; a.site = site; a.seed = seed
    _check(load_library().blim_rmsnorm_bwd(C.byref(a), _stream()), "blim_rmsnorm_bwd")


def ce_workspace_bytes(n_rows: int) -> int:
    return int(load_library().blim_ce_workspace_bytes(n_rows))


def ce_fwd_bwd(logits, V: int, labels, label_div: int, n_rows: int, coef: float, loss, workspace, dl16=None, dl32=None, dtype: str = "f16"):
    """blim_ce_fwd_bwd: logits f32 [n_rows, ldl], labels int32, loss f32 [1] (incremented), dl16 16-bit or dl32 f32 [n_rows, ldd]."""
    out = dl16 if dl16 is not None else dl32
    _check(load_library().blim_ce_fwd_bwd(_ptr(logits), logits.shape[1], V, _ptr(labels), label_div, n_rows, coef, _ptr(dl16), _ptr(dl32),
                                          out.shape[1] if out is not None else 0, _ptr(loss), COMPUTE_DTYPES[dtype] if dl16 is None else _dt16(dl16),
                                          _ptr(workspace), workspace.numel(), _stream()), "blim_ce_fwd_bwd")


def gelu(pre16, out16, rows: int, H: int, dh=None):
    """blim_gelu: forward (dh None) out16 [rows, ldo] = gelu(pre16 [rows, H]); backward out16 [rows, H] = 16-bit(dh * gelu'(pre16))."""
    _check(load_library().blim_gelu(0 if dh is None else 1, _ptr(out16), out16.shape[1], _ptr(pre16), _ptr(dh), rows, H, _dt16(pre16), _stream()), "blim_gelu")


def adamw_raw(p, g, exp_avg, exp_avg_sq, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, inv_scale: float, step: int):
    _check(load_library().blim_adamw_raw(_ptr(p), _ptr(g), _ptr(exp_avg), _ptr(exp_avg_sq), p.numel(), lr, beta1, beta2, eps, weight_decay, inv_scale, step, _stream()),
           "blim_adamw_raw")


def grad_stats_workspace_bytes(n: int) -> int:
    return int(load_library().blim_grad_stats_workspace_bytes(n))


def grad_stats_raw(g, inv_scale: float, stats, workspace):
    _check(load_library().blim_grad_stats_raw(_ptr(g), g.numel(), inv_scale, _ptr(stats), _ptr(workspace), workspace.numel(), _stream()), "blim_grad_stats_raw")


_GEMM_POINTERS = ("bias", "resid_in", "rope_rows", "labels", "lse_part", "label_logit", "row_scale", "col_scale", "a_mx", "out8", "out_mx", "A6", "W6", "out6",
                  "swiglu_act", "swiglu_gu")
_GEMM_INTS = ("act", "w_wrap_k", "lo_off", "rope_cols", "rope_stride", "mx_stride", "K6", "f6_build", "swiglu_act_ld", "swiglu_ld", "tile", "tile_lo6", "tile_qkv")


def gemm(epi: str, dtype: str, a, w, M: int, N: int, K: int, c=None, lda: Optional[int] = None, ldc: Optional[int] = None, scale: float = 1.0,
         f16_saturate: int = 1, **fields):
    """The GEMM kernel alone (blim_gemm): epi one of EPILOGUES, dtype "bf16" / "f16" / "f8"; a [M, lda] and w [N, K] device tensors of that format (f8: uint8
    e4m3 bytes), c the output buffer ([rows, ldc]: its width is the row stride unless ldc is given; None where the epilogue has no C).  Every other field of
    blim.h's blim_gemm_args by keyword: tensors for the pointers (bias, resid_in, rope_rows, labels, lse_part, label_logit, row_scale, col_scale, a_mx, out8,
    out_mx, A6, W6, out6, swiglu_act, swiglu_gu), ints for act, w_wrap_k, lo_off, rope_cols, rope_stride, mx_stride, K6, f6_build, swiglu_act_ld, swiglu_ld,
    tile (0 = 256 x 256 tiles, 1 = auto, 2 = the narrow residual kernel: the same bits; gemm_narrow_launches() tells which kernel ran), tile_lo6 (the same three
    values for the residual epilogue with A6 / W6: 2 = the narrow kernel with the e2m3 second pass; gemm_narrow_lo6_launches()), tile_qkv (the same three values
    for the QKV epilogue on fp16 / bf16 operands: 2 = the narrow QKV kernel; gemm_narrow_qkv_launches())."""
    lib = load_library()
    g = GemmArgs()
    g.struct_bytes = C.sizeof(GemmArgs)
    g.epi = EPILOGUES[epi]; g.dtype = COMPUTE_DTYPES[dtype]
    g.A = _ptr(a); g.lda = a.shape[1] if lda is None else lda; g.W = _ptr(w); g.M = M; g.N = N; g.K = K
    g.C = _ptr(c); g.ldc = (c.shape[1] if c is not None else 0) if ldc is None else ldc
    g.scale = scale; g.f16_saturate = int(f16_saturate)
    for k, v in fields.items():
        if k in _GEMM_POINTERS:
            setattr(g, k, _ptr(v))
        elif k in _GEMM_INTS:
            setattr(g, k, int(v))
        else:
            raise TypeError(f"gemm(): unknown field {k!r}")
    _check(lib.blim_gemm(C.byref(g), _stream()), "blim_gemm")
    return c


def gemm_narrow_launches() -> int:
    """Launches of the narrow residual GEMM kernel by this process so far (blim_gemm_narrow_launches)."""
    return int(load_library().blim_gemm_narrow_launches())


def gemm_narrow_threshold() -> int:
    """The auto rule's constant: tile = 1 / option "narrow_gemm" = 1 take the narrow kernel below this many 256 x 256 tiles (blim_gemm_narrow_threshold)."""
    return int(load_library().blim_gemm_narrow_threshold())


def gemm_narrow_lo6_launches() -> int:
    """Launches of the narrow residual GEMM kernel with the e2m3 second pass by this process so far (blim_gemm_narrow_lo6_launches): a counter of its own,
    gemm_narrow_launches() does not move on them."""
    return int(load_library().blim_gemm_narrow_lo6_launches())


def gemm_narrow_lo6_threshold() -> int:
    """The auto rule's constant: tile_lo6 = 1 / option "narrow_lo6" = 1 take that kernel below this many 256 x 256 tiles (blim_gemm_narrow_lo6_threshold)."""
    return int(load_library().blim_gemm_narrow_lo6_threshold())


def gemm_narrow_qkv_launches() -> int:
    """Launches of the narrow QKV GEMM kernel by this process so far (blim_gemm_narrow_qkv_launches): a counter of its own, the other two do not move on them."""
    return int(load_library().blim_gemm_narrow_qkv_launches())


def gemm_narrow_qkv_threshold() -> int:
    """The auto rule's constant: tile_qkv = 1 / option "narrow_qkv" = 1 take that kernel below this many 256 x 256 tiles (blim_gemm_narrow_qkv_threshold)."""
    return int(load_library().blim_gemm_narrow_qkv_threshold())


def rope_rows(positions, rope_theta: float, max_positions: int, stride: Optional[int] = None):
    """blim_rope_rows: positions int32 [T] (device) -> f32 [8, stride, 16], the cos / sin table of the QKV epilogue (csrc/gemm.hpp: rope_rows); rows >= T of
    every chunk are left as allocated (NaN here)."""
    import torch
    lib = load_library()
    T = positions.numel()
    stride = T if stride is None else stride
    ws = torch.empty(lib.blim_rope_rows_bytes(max_positions), dtype=torch.uint8, device=positions.device)
    out = torch.full((8, stride, 16), float("nan"), dtype=torch.float32, device=positions.device)
    _check(lib.blim_rope_rows(_ptr(positions), T, rope_theta, max_positions, _ptr(ws), _ptr(out), stride, _stream()), "blim_rope_rows")
    return out


def gemm_bf16(a, w):
    """a [M,K], w [N,K] (both bf16 or both f16) -> [M,N] of the same dtype (plain epilogue)."""
    import torch
    lib = load_library()
    M, K = a.shape
    N = w.shape[0]
    assert a.dtype == w.dtype and a.dtype in (torch.bfloat16, torch.float16)
    out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    fn = lib.blim_gemm_bf16 if a.dtype == torch.bfloat16 else lib.blim_gemm_f16
    _check(fn(_ptr(a), K, _ptr(w), M, N, K, _ptr(out), N, _stream()), "blim_gemm")
    return out
