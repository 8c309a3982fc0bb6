"""Offline feature extraction on the MI355X engine: host side of blim_vision_* (include/blim.h).

Mirrors what the reference's extract.py does per video (extract.py:96-110):

    frames uint8 [16, H, W, 3] --UMTImageProcessor--> fp16 [16, 3, 448, 448]            (vision_tower_builder.py:441-475)
      --model.encode_video_image(video, ..., return_video_feature=True)-->  [4, 64, 1024] (modeling_videochat_flash.py:126-181:
        4 clips x 4 frames through UMTVisionTower, vision_tower_builder.py:525-571, then ToMe 3136 -> 64 tokens per clip,
        mm_projector_builder.py:100-154)
      --torch.save(feature.half(), ./data/<DS>/features/<vid>.pth)-->                    the files blim_amd.dataloader reads

All tensor work runs in HIP (csrc/vision.hip + the engine's GEMM); this module holds the configuration, the position table
(host numpy, computed once), the weight naming and the ctypes binding.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import engine as eng

IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # UMTImageProcessor defaults, vision_tower_builder.py:442


@dataclass
class VisionDims:
    """build_vit's constants (vision_tower_builder.py:506-523) and the 'umt-hd' image size (:613-614)."""
    image_size: int = 448
    patch_size: int = 16
    num_frames: int = 4              # mm_local_num_frames
    hidden_size: int = 1024
    num_heads: int = 16
    mlp_hidden: int = 4096
    depth: int = 23                  # encoder_depth 24 + mm_vision_select_layer (-2) + 1
    tome_tokens: int = 64            # 16 * num_frames (mm_projector_builder.py:147)

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def tokens_per_clip(self) -> int:
        return self.num_frames * self.grid * self.grid


def vision_weight_shapes(d: VisionDims) -> Dict[str, Tuple[int, ...]]:
    D, Hm, P = d.hidden_size, d.mlp_hidden, d.patch_size
    s: Dict[str, Tuple[int, ...]] = {"vit.patch.w": (D, 3 * P * P), "vit.patch.b": (D,), "vit.norm.w": (D,), "vit.norm.b": (D,)}
    for i in range(d.depth):
        B = f"vit.blocks.{i}."
        s[B + "norm1.w"] = (D,); s[B + "norm1.b"] = (D,); s[B + "q_bias"] = (D,); s[B + "v_bias"] = (D,)
        s[B + "qkv.w"] = (3 * D, D); s[B + "proj.w"] = (D, D); s[B + "proj.b"] = (D,)
        s[B + "norm2.w"] = (D,); s[B + "norm2.b"] = (D,)
        s[B + "fc1.w"] = (Hm, D); s[B + "fc1.b"] = (Hm,); s[B + "fc2.w"] = (D, Hm); s[B + "fc2.b"] = (D,)
    return s


def vision_weight_dist(name: str) -> Tuple[float, float]:
    """(std, mean) of a synthetic tensor: LayerNorm gains bell(1, 0.1), everything else bell(0, 0.02) -- the rule
    blim_vision_init_synthetic_weights applies on device."""
    return (0.1, 1.0) if (name.endswith("norm1.w") or name.endswith("norm2.w") or name == "vit.norm.w") else (0.02, 0.0)


def checkpoint_key(name: str) -> str:
    """Canonical tensor name -> key in the VideoChat-Flash checkpoint (model.vision_tower = UMTVisionTower, whose .vision_tower is
    the PretrainVisionTransformer with its .encoder: vision_tower_builder.py:272-433, 525-556)."""
    root = "model.vision_tower.vision_tower.encoder."
    if name == "vit.patch.w": return root + "patch_embed.proj.weight"          # [D, 3, 1, P, P]: flattened to [D, 3*P*P] on load
    if name == "vit.patch.b": return root + "patch_embed.proj.bias"
    if name == "vit.norm.w": return root + "vision_layernorm.weight"
    if name == "vit.norm.b": return root + "vision_layernorm.bias"
    _, _, i, rest = name.split(".", 3)
    m = {"norm1.w": "norm1.weight", "norm1.b": "norm1.bias", "q_bias": "attn.q_bias", "v_bias": "attn.v_bias", "qkv.w": "attn.qkv.weight",
         "proj.w": "attn.proj.weight", "proj.b": "attn.proj.bias", "norm2.w": "norm2.weight", "norm2.b": "norm2.bias",
         "fc1.w": "mlp.fc1.weight", "fc1.b": "mlp.fc1.bias", "fc2.w": "mlp.fc2.weight", "fc2.b": "mlp.fc2.bias"}[rest]
    return f"{root}blocks.{i}.{m}"


# ----------------------------------------------------------------------------- position table (host, once)

def _sinusoid_table(n_position: int, d_hid: int) -> np.ndarray:
    """vision_tower_builder.py:188-232: float64 angles pos / 10000^(2*(j//2)/d), sin on even and cos on odd columns, cast to f32."""
    j = np.arange(d_hid)
    ang = np.arange(n_position, dtype=np.float64)[:, None] / np.power(10000.0, 2 * (j // 2) / d_hid)[None, :]
    out = ang.copy()
    out[:, 0::2] = np.sin(ang[:, 0::2]); out[:, 1::2] = np.cos(ang[:, 1::2])
    return out.astype(np.float32)


def _bicubic_axis(in_n: int, out_n: int):
    """Source taps and cubic-convolution weights (A = -0.75) of one axis of F.interpolate(mode='bicubic', align_corners=False)."""
    A = np.float32(-0.75)
    scale = np.float32(in_n) / np.float32(out_n)
    src = (scale * (np.arange(out_n, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)).astype(np.float32)
    fl = np.floor(src)
    t = (src - fl).astype(np.float32)
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    w = np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=-1).astype(np.float32)
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, in_n - 1)
    return idx, w


def _bicubic_resize(x: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """x [N, C, H, W] f32 -> [N, C, out_h, out_w]."""
    iy, wy = _bicubic_axis(x.shape[2], out_h)
    ix, wx = _bicubic_axis(x.shape[3], out_w)
    tmp = np.zeros(x.shape[:3] + (out_w,), dtype=np.float32)
    for k in range(4):
        tmp += x[:, :, :, ix[:, k]] * wx[None, None, None, :, k]
    out = np.zeros(x.shape[:2] + (out_h, out_w), dtype=np.float32)
    for k in range(4):
        out += tmp[:, :, iy[:, k], :] * wy[None, None, :, k, None]
    return out


def pos_embed(d: VisionDims) -> np.ndarray:
    """[tokens_per_clip, hidden] f32 table added to the patch embeddings (vision_tower_builder.py:304-313, 353): the 4 x 14 x 14
    checkpoint table, bicubically resized to the grid when image_size != 224 (get_sinusoid_encoding_table2, :222-269)."""
    if d.num_frames != 4:
        raise NotImplementedError("position table: clips of 4 frames (the checkpoint's frame count; no temporal interpolation on the extraction path)")
    D, T, G = d.hidden_size, d.num_frames, d.grid
    if d.image_size == 224:
        return _sinusoid_table(T * G * G, D)
    tab = _sinusoid_table(T * 14 * 14, D)
    if G != 14:
        t4 = np.ascontiguousarray(tab.reshape(T, 14, 14, D).transpose(0, 3, 1, 2))
        tab = _bicubic_resize(t4, G, G).transpose(0, 2, 3, 1).reshape(T * G * G, D)
    return np.ascontiguousarray(tab, dtype=np.float32)


# ----------------------------------------------------------------------------- binding

class VisionConfigC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("image_size", "patch_size", "num_frames", "hidden_size", "num_heads", "mlp_hidden", "depth", "tome_tokens",
                                          "compute_dtype")]


_bound = False


def _lib():
    global _bound
    lib = eng.load_library()
    if not _bound:
        vp, i32, u64 = C.c_void_p, C.c_int32, C.c_uint64
        lib.blim_vision_create.argtypes = [C.POINTER(VisionConfigC), C.POINTER(vp)]; lib.blim_vision_create.restype = C.c_int
        lib.blim_vision_destroy.argtypes = [vp]; lib.blim_vision_destroy.restype = None
        lib.blim_vision_load_weight.argtypes = [vp, C.c_char_p, vp, i32, i32]; lib.blim_vision_load_weight.restype = C.c_int
        lib.blim_vision_init_synthetic_weights.argtypes = [vp, u64]; lib.blim_vision_init_synthetic_weights.restype = C.c_int
        lib.blim_vision_set_pos_embed.argtypes = [vp, vp]; lib.blim_vision_set_pos_embed.restype = C.c_int
        lib.blim_vision_ready.argtypes = [vp]; lib.blim_vision_ready.restype = C.c_int
        lib.blim_vision_encode.argtypes = [vp, vp, i32, vp, vp, vp]; lib.blim_vision_encode.restype = C.c_int
        lib.blim_tome_merge.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]; lib.blim_tome_merge.restype = C.c_int
        _bound = True
    return lib


class VisionEncoder:
    """One vision encoder on the current HIP device."""

    def __init__(self, dims: Optional[VisionDims] = None, dtype: Optional[str] = None):
        import torch
        self.lib = _lib()
        if not torch.cuda.is_available():
            raise eng.BlimError("no HIP device visible: the vision encoder has no CPU fallback")
        self.dims = dims or VisionDims()
        self.dtype = dtype or "f16"                              # extract.py runs the tower under autocast(float16)
        if self.dtype not in ("f16", "bf16"):
            raise ValueError("vision encoder dtype: f16 or bf16")
        self.torch_dtype = eng.torch_dtype_of(self.dtype)
        d = self.dims
        cfg = VisionConfigC(d.image_size, d.patch_size, d.num_frames, d.hidden_size, d.num_heads, d.mlp_hidden, d.depth, d.tome_tokens,
                            eng.COMPUTE_DTYPES[self.dtype])
        h = C.c_void_p()
        eng._check(self.lib.blim_vision_create(C.byref(cfg), C.byref(h)), "blim_vision_create")
        self.h = h
        self.device = torch.device("cuda", torch.cuda.current_device())
        tab = pos_embed(d)
        eng._check(self.lib.blim_vision_set_pos_embed(self.h, tab.ctypes.data), "blim_vision_set_pos_embed")

    def close(self):
        if getattr(self, "h", None):
            self.lib.blim_vision_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights
    def load_weight(self, name: str, arr: np.ndarray):
        shape = vision_weight_shapes(self.dims)[name]
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(shape)      # the Conv3d kernel [D, 3, 1, P, P] flattens to [D, 3*P*P]
        eng._check(self.lib.blim_vision_load_weight(self.h, name.encode(), a.ctypes.data, eng.DTYPE_F32, 0), f"blim_vision_load_weight({name})")

    def load_weights(self, weights: Dict[str, np.ndarray]):
        for name, arr in weights.items():
            self.load_weight(name, arr)
        eng._check(self.lib.blim_vision_ready(self.h), "blim_vision_ready")

    def load_checkpoint(self, model_path: str):
        """The vision-tower tensors of the VideoChat-Flash checkpoint (sharded safetensors; main.py:96 loads the same files)."""
        from .checkpoint import open_base_checkpoint
        keys, get = open_base_checkpoint(model_path)
        have = set(keys)
        for name in vision_weight_shapes(self.dims):
            k = checkpoint_key(name)
            if k not in have:
                raise KeyError(f"vision tensor '{name}' ({k}) not found in {model_path}")
            self.load_weight(name, get(k))
        eng._check(self.lib.blim_vision_ready(self.h), "blim_vision_ready")

    def init_synthetic_weights(self, seed: int):
        eng._check(self.lib.blim_vision_init_synthetic_weights(self.h, seed), "blim_vision_init_synthetic_weights")

    # ---- compute
    def encode(self, frames, want_feat: bool = False):
        """frames: device tensor [n_clips * T, 3, S, S] (or [n_clips, T, 3, S, S]) of normalised pixels.
        Returns (tome f32 [n_clips, tome_tokens, D], feat f32 [n_clips, L, D] | None)."""
        import torch
        d = self.dims
        x = frames.to(device=self.device, dtype=self.torch_dtype).reshape(-1, d.num_frames, 3, d.image_size, d.image_size).contiguous()
        n = x.shape[0]
        tome = torch.empty((n, d.tome_tokens, d.hidden_size), dtype=torch.float32, device=self.device)
        feat = torch.empty((n, d.tokens_per_clip, d.hidden_size), dtype=torch.float32, device=self.device) if want_feat else None
        eng._check(self.lib.blim_vision_encode(self.h, eng._ptr(x), n, eng._ptr(feat), eng._ptr(tome), eng._stream()), "blim_vision_encode")
        return tome, feat

    def tome_merge(self, x, target: int):
        """ToMe alone on f32 tokens [b, p, c] -> [b, target, c] (bipartite soft matching, size-weighted averages)."""
        import torch
        b, p, c = x.shape
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty((b, target, c), dtype=torch.float32, device=self.device)
        eng._check(self.lib.blim_tome_merge(self.h, eng._ptr(x), b, p, c, c // 64, target, eng._ptr(out), eng._stream()), "blim_tome_merge")
        return out

    def video_feature(self, frames):
        """One video's frames [n_clips * T, 3, S, S] -> the tensor extract.py:107-110 saves: fp16 [n_clips, tome_tokens, D] on host."""
        import torch
        tome, _ = self.encode(frames)
        return tome.to(torch.float16).cpu()

    def video_feature_u8(self, frames_u8):
        """One video's raw frames, uint8 [n_clips * T, H, W, 3] -> video_feature(preprocess(frames_u8)), bit for bit, with the resize and the normalisation
        on the device (preprocess_device)."""
        return self.video_feature(preprocess_device(frames_u8, self.dims.image_size, self.dtype, self.device))


def vit_attention(qkv, n_clips: int, heads: int):
    """The encoder's attention alone (blim_vit_attention): qkv 16-bit device tensor [n_clips * L, 3 * heads * 64] -> [n_clips * L, heads * 64]."""
    import torch
    lib = eng.load_library()
    vp, i32 = C.c_void_p, C.c_int32
    lib.blim_vit_attention.argtypes = [vp, i32, i32, i32, i32, vp, vp]; lib.blim_vit_attention.restype = C.c_int
    assert qkv.dtype in (torch.float16, torch.bfloat16) and qkv.shape[1] == 3 * heads * 64 and qkv.shape[0] % n_clips == 0
    out = torch.empty((qkv.shape[0], heads * 64), dtype=qkv.dtype, device=qkv.device)
    eng._check(lib.blim_vit_attention(eng._ptr(qkv), n_clips, qkv.shape[0] // n_clips, heads, eng.COMPUTE_DTYPES["f16" if qkv.dtype == torch.float16 else "bf16"],
                                      eng._ptr(out), eng._stream()), "blim_vit_attention")
    return out


# ----------------------------------------------------------------------------- preprocessing (host)

def preprocess(frames_u8: np.ndarray, image_size: int = 448):
    """UMTImageProcessor.preprocess (vision_tower_builder.py:454-475): RGB uint8 [T, H, W, 3] -> bicubic resize to (S, S) (PIL, as
    transformers' `resize` does for uint8 images), x 1/255, normalise with the ImageNet mean / std, channels first; returns a
    torch half tensor [T, 3, S, S] (extract.py:58 .half())."""
    import torch
    from PIL import Image
    out = np.empty((len(frames_u8), 3, image_size, image_size), dtype=np.float32)
    mean = np.asarray(IMAGE_MEAN, np.float32)[:, None, None]; std = np.asarray(IMAGE_STD, np.float32)[:, None, None]
    for i, f in enumerate(frames_u8):
        img = Image.fromarray(np.asarray(f, dtype=np.uint8)).convert("RGB")
        if img.size != (image_size, image_size):
            img = img.resize((image_size, image_size), resample=Image.BICUBIC)
        a = np.asarray(img, dtype=np.float32).transpose(2, 0, 1) * np.float32(1.0 / 255.0)
        out[i] = (a - mean) / std
    return torch.from_numpy(out).half()


# ----------------------------------------------------------------------------- preprocessing (device)

_RESIZE_BITS = 22                    # PIL's fixed-point precision for 8-bit images
_PRE_MAX_DIM = 8192                  # blim_preprocess_frames' limit on T, H, W, S
_tables: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray]] = {}


def _bicubic_kernel(x: np.ndarray) -> np.ndarray:
    """Keys' cubic with a = -0.5 on float64 distances (PIL's BICUBIC)."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def bicubic_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """The taps of one axis of PIL's 8-bit bicubic resize from in_size to out_size: (bounds int32 [out, 2] = (first tap, tap count), coeffs int32
    [out, ksize], zero past the count).  Pillow's coefficient rule in float64: the kernel is stretched by max(scale, 1), a tap window is
    [int(center - support + 0.5), int(center + support + 0.5)) clipped to the axis, the weights are divided by their sum taken in tap order, and a weight w
    becomes int(+-0.5 + w * 2**22).  Memoised per size pair; the arrays are read-only."""
    key = (int(in_size), int(out_size))
    if key in _tables:
        return _tables[key]
    n_in, n_out = key
    if n_in < 1 or n_out < 1:
        raise ValueError("bicubic_tables: sizes must be at least 1")
    scale = n_in / n_out
    stretch = max(scale, 1.0)
    support = 2.0 * stretch
    ksize = 2 * int(np.ceil(support)) + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    first = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    count = np.minimum(np.trunc(center + support + 0.5), n_in).astype(np.int64) - first
    tap = np.arange(ksize, dtype=np.int64)[None, :]
    live = tap < count[:, None]
    w = np.where(live, _bicubic_kernel((tap + first[:, None] - center[:, None] + 0.5) * (1.0 / stretch)), 0.0)
    total = np.zeros(n_out, dtype=np.float64)
    for i in range(ksize):                                                 # in tap order: a pairwise sum rounds differently
        total += w[:, i]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    coeffs = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << _RESIZE_BITS)).astype(np.int32)
    coeffs[~live] = 0
    bounds = np.stack([first, count], axis=1).astype(np.int32)
    assert np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 1] >= 1) and np.all(bounds.sum(axis=1) <= n_in) and np.all(bounds[:, 1] <= ksize)
    bounds.setflags(write=False); coeffs.setflags(write=False)
    _tables[key] = (bounds, coeffs)
    return _tables[key]


def normalise_lut(dtype: str = "f16") -> np.ndarray:
    """uint16 [3, 256]: the 16-bit pattern `preprocess` (followed by VisionEncoder.encode's cast for a bf16 tower) gives channel c of a pixel of value v,
    computed with preprocess' own expressions, so that a lookup equals the host path by construction."""
    import torch
    if dtype not in ("f16", "bf16"):
        raise ValueError("normalise_lut dtype: f16 or bf16")
    mean = np.asarray(IMAGE_MEAN, np.float32)[:, None]; std = np.asarray(IMAGE_STD, np.float32)[:, None]
    a = np.arange(256, dtype=np.float32)[None, :] * np.float32(1.0 / 255.0)
    t = torch.from_numpy(np.ascontiguousarray((a - mean) / std, dtype=np.float32)).half()
    if dtype == "bf16":
        t = t.to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


_pre_bound = False
_pre_state: Dict = {}                # per device: uploaded tables and LUTs, the workspace


def _pre_lib():
    global _pre_bound
    lib = eng.load_library()
    if not _pre_bound:
        vp, i32 = C.c_void_p, C.c_int32
        lib.blim_preprocess_workspace_bytes.argtypes = [i32, i32, i32, i32]; lib.blim_preprocess_workspace_bytes.restype = C.c_int64
        lib.blim_preprocess_frames.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]; lib.blim_preprocess_frames.restype = C.c_int
        _pre_bound = True
    return lib


def _device_tables(state: Dict, device, in_size: int, out_size: int):
    """(bounds, coeffs, ksize) on the device, uploaded once per size pair; (None, None, 0) for a pass that is skipped."""
    import torch
    if in_size == out_size:
        return None, None, 0
    key = ("taps", in_size, out_size)
    if key not in state:
        bounds, coeffs = bicubic_tables(in_size, out_size)
        assert int((bounds[:, 0] + bounds[:, 1]).max()) <= in_size and int(bounds[:, 1].max()) <= coeffs.shape[1]       # what the kernel trusts
        state[key] = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coeffs.copy()).to(device), int(coeffs.shape[1]))
    return state[key]


def preprocess_device(frames_u8, image_size: int = 448, dtype: str = "f16", device=None, lut: Optional[np.ndarray] = None):
    """`preprocess` on the GPU (blim_preprocess_frames): uint8 RGB frames [T, H, W, 3], a numpy array or a torch tensor (host or device) -> a device tensor
    [T, 3, S, S] of `dtype` ("f16" | "bf16") that equals preprocess(frames, S) (cast with .to(bfloat16) for bf16) bit for bit.  One upload of the raw frames;
    the taps, the table and the workspace live on the device and are reused by later calls (stream-ordered: call from one thread per device).  `lut`
    replaces normalise_lut(dtype) (uint16 [3, 256]; tests read the resized bytes back through it)."""
    import torch
    if dtype not in ("f16", "bf16"):
        raise ValueError("preprocess_device dtype: f16 or bf16")
    if isinstance(frames_u8, np.ndarray):
        if frames_u8.dtype != np.uint8:
            raise ValueError(f"preprocess_device: frames must be uint8 (got {frames_u8.dtype})")
        if frames_u8.ndim == 4 and not frames_u8.flags["C_CONTIGUOUS"]:
            raise ValueError("preprocess_device: frames must be contiguous")
    elif isinstance(frames_u8, torch.Tensor):
        if frames_u8.dtype != torch.uint8:
            raise ValueError(f"preprocess_device: frames must be uint8 (got {frames_u8.dtype})")
        if frames_u8.dim() == 4 and not frames_u8.is_contiguous():
            raise ValueError("preprocess_device: frames must be contiguous")
    else:
        raise ValueError("preprocess_device: frames must be a numpy array or a torch tensor")
    if len(frames_u8.shape) != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"preprocess_device: frames must be [T, H, W, 3] (got {tuple(frames_u8.shape)})")
    T, H, W = (int(n) for n in frames_u8.shape[:3])
    S = int(image_size)
    if min(T, H, W, S) < 1 or max(T, H, W, S) > _PRE_MAX_DIM:
        raise ValueError(f"preprocess_device: T, H, W and the image size must lie in 1 .. {_PRE_MAX_DIM} (got {T}, {H}, {W}, {S})")
    if not torch.cuda.is_available():
        raise eng.BlimError("no HIP device visible: preprocess_device has no CPU fallback (preprocess is the host path)")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _pre_lib()
    state = _pre_state.setdefault(str(device), {})
    x = (torch.from_numpy(frames_u8) if isinstance(frames_u8, np.ndarray) else frames_u8).to(device)
    xb, xk, xks = _device_tables(state, device, W, S)
    yb, yk, yks = _device_tables(state, device, H, S)
    if lut is None:
        if ("lut", dtype) not in state:
            state[("lut", dtype)] = torch.from_numpy(normalise_lut(dtype).view(np.int16)).to(device)
        table = state[("lut", dtype)]
    else:
        lut = np.ascontiguousarray(lut)
        if lut.dtype != np.uint16 or lut.shape != (3, 256):
            raise ValueError("preprocess_device: lut must be uint16 [3, 256]")
        table = torch.from_numpy(lut.view(np.int16)).to(device)
    need = int(lib.blim_preprocess_workspace_bytes(T, H, W, S))
    if need < 0:
        raise eng.BlimError(f"blim_preprocess_workspace_bytes failed (code {need}): {lib.blim_last_error().decode()}")
    ws = state.get("workspace")
    if need and (ws is None or ws.numel() < need):
        ws = state["workspace"] = torch.empty(need, dtype=torch.uint8, device=device)
    out = torch.empty((T, 3, S, S), dtype=eng.torch_dtype_of(dtype), device=device)
    with torch.cuda.device(device):
        eng._check(lib.blim_preprocess_frames(eng._ptr(x), T, H, W, S, eng._ptr(xb), eng._ptr(xk), xks, eng._ptr(yb), eng._ptr(yk), yks, eng._ptr(table), eng._ptr(out),
                                              eng._ptr(ws) if need else None, eng._stream()), "blim_preprocess_frames")
    return out


def sample_frame_indices(vlen, num_frames: int = 16) -> np.ndarray:
    """extract.py:54: np.linspace(0, vlen - 2, num_frames, dtype=int); vlen may be fractional (30 * fps of a cut DiDeMo video): only linspace truncates."""
    return np.linspace(0, vlen - 2, num_frames, dtype=int)
