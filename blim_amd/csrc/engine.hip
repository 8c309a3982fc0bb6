// C-ABI of the scoring engine (include/blim.h): weight store, workspaces and the launch sequence of
// the decoder / scoring heads.  One engine per process per GPU; all kernels are launched on the
// caller's stream.
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "engine.hpp"

// ---------------------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";
void blim_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* blim_last_error(void) { return g_err; }
extern "C" int blim_abi_version(void) { return BLIM_ABI_VERSION; }

static const char* kTimeClassNames[TC_COUNT] = {"gemm_qkv_rope", "attention", "gemm_o_resid", "gemm_gateup_swiglu", "gemm_down_resid",
                                                "rmsnorm", "lm_head_lse", "gemm_other", "misc", "quantize_fp8"};

int dev_alloc(blim_engine* e, void** p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes));
    e->owned.push_back(*p);
    return BLIM_OK;
}
int ensure(DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes) return BLIM_OK;
    if (b.p) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    const size_t want = bytes + bytes / 8 + 4096;
    HIP_TRY(hipMalloc(&b.p, want));
    b.bytes = want;
    return BLIM_OK;
}
// ---------------------------------------------------------------------------- weight layout kernels
// dst row r <- src row map(r); modes: 0 identity, 1 q/k RoPE pair interleave inside each 128-row head,
// 2 gate rows of the fused gate|up matrix, 3 up rows.  SRC_F32: convert to bf16 (RNE).
__device__ __forceinline__ int64_t src_row_of(int64_t r, int mode) {
    if (mode == 1) { const int64_t h = r >> 7; const int c = (int)(r & 127); return (h << 7) + 16 * (c >> 5) + (c & 15) + 64 * ((c >> 4) & 1); }
    return r;
}
template <bool SRC_F32, int DT>
__global__ void place_rows_kernel(bf16_t* dst, const void* src, int64_t n_rows, int K, int mode) {
    // grid-stride over (row, 4-element chunk)
    const int chunks = K / 4;
    const int64_t total = n_rows * chunks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / chunks;
        const int c = (int)(i - r * chunks);
        int64_t drow, srow;
        if (mode == 2) { srow = r; drow = (r >> 4) * 32 + (r & 15); }
        else if (mode == 3) { srow = r; drow = (r >> 4) * 32 + 16 + (r & 15); }
        else { drow = r; srow = src_row_of(r, mode); }
        uint2 pk;
        if (SRC_F32) {
            const float4 v = *(const float4*)((const float*)src + srow * K + 4 * c);
            pk = make_uint2(pack2<DT>(v.x, v.y), pack2<DT>(v.z, v.w));
        } else {   // bf16 source
            pk = *(const uint2*)((const bf16_t*)src + srow * K + 4 * c);
            if (DT == DT_F16)
                pk = make_uint2(pack2<DT>(__uint_as_float(pk.x << 16), __uint_as_float(pk.x & 0xFFFF0000u)),
                                pack2<DT>(__uint_as_float(pk.y << 16), __uint_as_float(pk.y & 0xFFFF0000u)));
        }
        *(uint2*)(dst + drow * K + 4 * c) = pk;
    }
}
// f32 vector placement (biases, norm weights): dst[map(i)] = f32(src[i])
template <bool SRC_F32>
__global__ void place_vec_kernel(float* dst, const void* src, int64_t n, int mode) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t s = src_row_of(i, mode);
    dst[i] = SRC_F32 ? ((const float*)src)[s] : bf16_to_f32(((const bf16_t*)src)[s]);
}
__global__ void rope_table_kernel(float* cosb, float* sinb, int n_pos, int half, float theta, int head_dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pos * half) return;
    const int p = i / half, k = i - p * half;
    // modeling_qwen2_flash.py:112: inv_freq = 1 / theta^(2k/d) in f32; :120-125 angle = pos * inv_freq in f32
    const float inv = 1.0f / powf(theta, (float)(2 * k) / (float)head_dim);
    const float ang = (float)p * inv;
    cosb[i] = cosf(ang);
    sinb[i] = sinf(ang);
}
// table[chunk q][t][16] with q = {cos, sin} x 4 groups of 16 dims: cos / sin of every token's position, gathered once per batch so that the 28 QKV
// epilogues read their RoPE factors by row; chunk-major so that the 16 consecutive rows of an MFMA fragment are contiguous (gemm.hpp)
__global__ void rope_rows_kernel(float* rows, const int32_t* pos, const float* cosb, const float* sinb, int64_t n_tokens, int64_t stride, int n_pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one float4 per thread: 32 per token
    if (i >= n_tokens * 32) return;
    const int64_t t = i >> 5;
    const int c = (int)(i & 31);                                            // float4 index inside cos[64] | sin[64]
    const int p = min(max(pos[t], 0), n_pos - 1);
    const float* src = (c < 16 ? cosb : sinb) + (int64_t)p * 64 + 4 * (c & 15);
    const int q = (c >> 4) * 4 + ((c & 15) >> 2);                           // chunk: {cos, sin} x (d / 16)
    *(float4*)(rows + ((int64_t)q * stride + t) * 16 + 4 * (c & 3)) = *(const float4*)src;
}
__global__ void dense_batch_kernel(int32_t* pos, int32_t* seq_start, int32_t* seq_len, int32_t* pfx, int32_t* blk_seq, int32_t* blk_q0,
                                   int B, int L, int nblk_per_seq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * L) pos[i] = i % L;
    if (i < B) { seq_start[i] = i * L; seq_len[i] = L; pfx[i] = 0; }
    if (i < B * nblk_per_seq) { blk_seq[i] = i / nblk_per_seq; blk_q0[i] = 32 * (i % nblk_per_seq); }
}

// ---------------------------------------------------------------------------- create / destroy
// sizes the e2m3 second pass (lo6) takes: hidden and intermediate sizes multiples of 128, at most 20480
static bool lo6_sizes_ok(const blim_config& c) {
    return c.hidden_size % 128 == 0 && c.intermediate_size % 128 == 0 && c.hidden_size <= 20480 && c.intermediate_size <= 20480;
}
extern "C" int blim_create(const blim_config* cfg, blim_engine** out) {
    ARG_CHECK(cfg && out);
    ARG_CHECK(cfg->hidden_size > 0 && cfg->num_heads > 0 && cfg->num_kv_heads > 0 && cfg->num_layers > 0);
    ARG_CHECK(cfg->hidden_size % cfg->num_heads == 0);
    if (cfg->hidden_size / cfg->num_heads != 128) {
        blim_set_error("head_dim %d unsupported: the attention / RoPE kernels are built for head_dim 128", cfg->hidden_size / cfg->num_heads);
        return BLIM_ERR_ARG;
    }
    ARG_CHECK(cfg->num_heads % cfg->num_kv_heads == 0 && cfg->num_heads / cfg->num_kv_heads <= 8);
    ARG_CHECK(cfg->hidden_size % 64 == 0 && cfg->intermediate_size % 64 == 0 && cfg->mm_hidden_size % 64 == 0);
    ARG_CHECK(cfg->vocab_size > 0 && cfg->max_positions > 0 && cfg->num_clips > 0);
    ARG_CHECK(cfg->compute_dtype == BLIM_COMPUTE_BF16 || cfg->compute_dtype == BLIM_COMPUTE_F16 || cfg->compute_dtype == BLIM_COMPUTE_F8);
    ARG_CHECK(cfg->compute_dtype != BLIM_COMPUTE_F8 || (cfg->hidden_size % 128 == 0 && cfg->intermediate_size % 128 == 0));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        blim_set_error("no HIP device visible: the BLiM engine has no CPU fallback");
        return BLIM_ERR_HIP;
    }
    blim_engine* e = new blim_engine();
    e->c = *cfg;
    if (cfg->compute_dtype == BLIM_COMPUTE_F8) { e->f8 = true; e->c.compute_dtype = BLIM_COMPUTE_F16; }
    // fp16 engines: the compensated modes' second pass over K runs in e2m3 (gemm.hip, phase 2) unless BLIM_PRECISE_LO6=0 / option "precise_lo6" = 0.  bf16 engines keep the
    // 16-bit second pass by default (their parity mode: 1 - 3e-6 at 7B depth) and take the e2m3 pass with option "precise_lo6" = 1 / BLIM_PRECISE_LO6=1 (round 6)
    e->lo6 = !e->f8 && cfg->compute_dtype == DT_F16 && lo6_sizes_ok(*cfg);
    if (getenv("BLIM_PRECISE_LO6") && atoi(getenv("BLIM_PRECISE_LO6")) == 0) e->lo6 = false;
    if (getenv("BLIM_PRECISE_LO6") && atoi(getenv("BLIM_PRECISE_LO6")) == 1 && !e->f8 && cfg->compute_dtype == DT_BF16 && lo6_sizes_ok(*cfg)) e->lo6 = true;
    if (getenv("BLIM_LO6_FUSED_TILES") && atoi(getenv("BLIM_LO6_FUSED_TILES")) == 0) e->lo6_fuse = false;
    if (getenv("BLIM_LO6_FUSED_MASK")) e->lo6_fuse_mask = atoi(getenv("BLIM_LO6_FUSED_MASK"));
    const int H = cfg->hidden_size, I = cfg->intermediate_size, V = cfg->vocab_size, M = cfg->mm_hidden_size;
    e->qkv_n = (cfg->num_heads + 2 * cfg->num_kv_heads) * 128;
    e->L.resize(cfg->num_layers);
    e->layer_bits.assign(cfg->num_layers, 15);
    int rc = BLIM_OK;
#define A(ptr, count, type) do { if (rc == BLIM_OK) rc = dev_alloc(e, (void**)&(ptr), (size_t)(count) * sizeof(type)); } while (0)
    A(e->embed, (int64_t)V * H, bf16_t);
    A(e->lm_head, (int64_t)V * H, bf16_t);
    A(e->visual_head, (int64_t)M * H, bf16_t);
    A(e->final_norm, H, float);
    for (int w = 0; w < 2; ++w) {
        A(e->mlp_w0[w], (int64_t)H * M, bf16_t); A(e->mlp_b0[w], H, float);
        A(e->mlp_w2[w], (int64_t)H * H, bf16_t); A(e->mlp_b2[w], H, float);
    }
    for (auto& l : e->L) {
        A(l.norm1, H, float); A(l.norm2, H, float);
        A(l.wqkv, (int64_t)e->qkv_n * H, bf16_t); A(l.bqkv, e->qkv_n, float);
        A(l.wo, (int64_t)H * H, bf16_t);
        A(l.wgu, (int64_t)2 * I * H, bf16_t);
        A(l.wd, (int64_t)H * I, bf16_t);
        if (e->f8) {
            A(l.wqkv8, (int64_t)e->qkv_n * H, uint8_t); A(l.sqkv, e->qkv_n, float);
            A(l.wo8, (int64_t)H * H, uint8_t); A(l.so, H, float);
            A(l.wgu8, (int64_t)2 * I * H, uint8_t); A(l.sgu, 2 * I, float);
            A(l.wd8, (int64_t)H * I, uint8_t); A(l.sd, H, float);
        }
    }
    if (e->f8) { A(e->lm_head8, (int64_t)V * H, uint8_t); A(e->s_lm, V, float); }
    A(e->rope_cos, (int64_t)cfg->max_positions * 64, float);
    A(e->rope_sin, (int64_t)cfg->max_positions * 64, float);
#undef A
    if (rc != BLIM_OK) { blim_destroy(e); return rc; }
    const int n = cfg->max_positions * 64;
    hipLaunchKernelGGL(rope_table_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, e->rope_cos, e->rope_sin, cfg->max_positions, 64, cfg->rope_theta, 128);
    if (hipDeviceSynchronize() != hipSuccess) { blim_set_error("rope table init failed"); blim_destroy(e); return BLIM_ERR_HIP; }
    *out = e;
    return BLIM_OK;
}

extern "C" void blim_destroy(blim_engine* e) {
    if (!e) return;
    hipDeviceSynchronize();
    for (void* p : e->owned) hipFree(p);
    for (void* p : e->aug_owned) hipFree(p);
    for (void* p : e->ad_owned) hipFree(p);
    if (e->lm6) hipFree(e->lm6);
    DevBuf* bufs[] = {&e->visual_head3, &e->hs3, &e->vocab3, &e->vocab1, &e->vh3, &e->feats_aug, &e->hid_aug, &e->resid_live, &e->resid, &e->xn, &e->qkv, &e->attn, &e->act, &e->hsel, &e->lse_part, &e->lab_logit, &e->logprob, &e->stage,
                      &e->proj_tmp, &e->vh, &e->tvg_logits, &e->dense_idx, &e->rope_rows, &e->act_mx, &e->attn_mx, &e->x8, &e->a8, &e->act8, &e->hsel8, &e->rscale, &e->a6, &e->a6b, &e->h6};
    for (DevBuf* b : bufs) if (b->p) hipFree(b->p);
    for (auto& s : e->spans) { hipEventDestroy(s.a); hipEventDestroy(s.b); }
    delete e;
}

// ---------------------------------------------------------------------------- weights
struct WeightSlot { int kind; /*0 matrix->bf16, 1 vector->f32*/ void* dst; int64_t rows; int64_t cols; int mode; int64_t dst_row_off; };

static bool find_slot(blim_engine* e, const std::string& name, WeightSlot& s) {
    const blim_config& c = e->c;
    const int H = c.hidden_size, I = c.intermediate_size, V = c.vocab_size, M = c.mm_hidden_size;
    const int64_t qn = (int64_t)c.num_heads * 128, kn = (int64_t)c.num_kv_heads * 128;
    auto mat = [&](void* d, int64_t r, int64_t k, int mode, int64_t off) { s = {0, d, r, k, mode, off}; return true; };
    auto vec = [&](void* d, int64_t n, int mode, int64_t off) { s = {1, d, n, 1, mode, off}; return true; };
    if (name == "embed_tokens") return mat(e->embed, V, H, 0, 0);
    if (name == "lm_head") return mat(e->lm_head, V, H, 0, 0);
    if (name == "visual_head") return mat(e->visual_head, M, H, 0, 0);
    if (name == "final_norm") return vec(e->final_norm, H, 0, 0);
    for (int w = 0; w < 2; ++w) {
        const std::string p = w ? "tvg_mlp." : "mlp.";
        if (name == p + "0.w") return mat(e->mlp_w0[w], H, M, 0, 0);
        if (name == p + "0.b") return vec(e->mlp_b0[w], H, 0, 0);
        if (name == p + "2.w") return mat(e->mlp_w2[w], H, H, 0, 0);
        if (name == p + "2.b") return vec(e->mlp_b2[w], H, 0, 0);
    }
    int li = -1; char rest[64] = "";
    if (sscanf(name.c_str(), "layers.%d.%63s", &li, rest) == 2 && li >= 0 && li < c.num_layers) {
        LayerW& l = e->L[li];
        const std::string r(rest);
        if (r == "input_norm") return vec(l.norm1, H, 0, 0);
        if (r == "post_norm") return vec(l.norm2, H, 0, 0);
        if (r == "q_proj.w") return mat(l.wqkv, qn, H, 1, 0);
        if (r == "k_proj.w") return mat(l.wqkv, kn, H, 1, qn);
        if (r == "v_proj.w") return mat(l.wqkv, kn, H, 0, qn + kn);
        if (r == "q_proj.b") return vec(l.bqkv, qn, 1, 0);
        if (r == "k_proj.b") return vec(l.bqkv, kn, 1, qn);
        if (r == "v_proj.b") return vec(l.bqkv, kn, 0, qn + kn);
        if (r == "o_proj.w") return mat(l.wo, H, H, 0, 0);
        if (r == "gate_proj.w") return mat(l.wgu, I, H, 2, 0);
        if (r == "up_proj.w") return mat(l.wgu, I, H, 3, 0);
        if (r == "down_proj.w") return mat(l.wd, H, I, 0, 0);
    }
    return false;
}

// visual_head is trained in fp32 (main.py:104-107) and arrives as a full tensor of the resume file: besides its 16-bit copy the engine keeps it as
// [hi | lo | hi] rows (3 H wide) -- the W side of the three-term product the compensated TVG calls form with the final hidden states (adapters.hpp).
// A 16-bit rounding of the head alone left 2e-4 on the bf16 engine's TVG scores of a fine-tuned checkpoint (tests/golden/lora7b.npz).
int engine_set_visual_head3(blim_engine* e, const void* dev_src, int dtype, hipStream_t s) {
    const int H = e->c.hidden_size, M = e->c.mm_hidden_size;
    TRY(ensure(e->visual_head3, (size_t)M * 3 * H * 2));
    if (dtype == BLIM_DTYPE_F32) return launch_split3_f32((uint16_t*)e->visual_head3.p, nullptr, (const float*)dev_src, M, H, 1, e->c.compute_dtype, s);
    // bf16 source: the placed 16-bit copy is exact, lo = 0
    HIP_TRY(hipMemsetAsync(e->visual_head3.p, 0, (size_t)M * 3 * H * 2, s));
    TRY(launch_copy_rows16((uint16_t*)e->visual_head3.p, 3 * (int64_t)H, (const uint16_t*)e->visual_head, H, M, H, s));
    return launch_copy_rows16((uint16_t*)e->visual_head3.p + 2 * H, 3 * (int64_t)H, (const uint16_t*)e->visual_head, H, M, H, s);
}

static int place_weight(blim_engine* e, const std::string& name, const void* dev_src, int dtype) {
    WeightSlot s;
    if (!find_slot(e, name, s)) { blim_set_error("unknown weight name '%s'", name.c_str()); return BLIM_ERR_ARG; }
    if (s.kind == 0) {
        ARG_CHECK(s.cols % 4 == 0);
        bf16_t* dst = (bf16_t*)s.dst + s.dst_row_off * s.cols;
        const int64_t total = s.rows * (s.cols / 4);
        const int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
        const bool f16 = e->c.compute_dtype == BLIM_COMPUTE_F16;
        if (dtype == BLIM_DTYPE_F32) {
            if (f16) hipLaunchKernelGGL((place_rows_kernel<true, DT_F16>), dim3(grid), dim3(256), 0, 0, dst, dev_src, s.rows, (int)s.cols, s.mode);
            else hipLaunchKernelGGL((place_rows_kernel<true, DT_BF16>), dim3(grid), dim3(256), 0, 0, dst, dev_src, s.rows, (int)s.cols, s.mode);
        } else {
            if (f16) hipLaunchKernelGGL((place_rows_kernel<false, DT_F16>), dim3(grid), dim3(256), 0, 0, dst, dev_src, s.rows, (int)s.cols, s.mode);
            else hipLaunchKernelGGL((place_rows_kernel<false, DT_BF16>), dim3(grid), dim3(256), 0, 0, dst, dev_src, s.rows, (int)s.cols, s.mode);
        }
    } else {
        float* dst = (float*)s.dst + s.dst_row_off;
        const int grid = (int)((s.rows + 255) / 256);
        if (dtype == BLIM_DTYPE_F32) hipLaunchKernelGGL(place_vec_kernel<true>, dim3(grid), dim3(256), 0, 0, dst, dev_src, s.rows, s.mode);
        else hipLaunchKernelGGL(place_vec_kernel<false>, dim3(grid), dim3(256), 0, 0, dst, dev_src, s.rows, s.mode);
    }
    HIP_TRY(hipGetLastError());
    if (name == "visual_head") TRY(engine_set_visual_head3(e, dev_src, dtype, 0));
    e->loaded[name] = true;
    e->f8_ready = false;
    e->lo6_ready = false;
    if (s.kind == 0) e->c6_dirty.insert(s.dst);              // (finalize_lo6 re-derives the e2m3 image of THIS matrix only)
    e->aug_ready = false;          // the augmented copies of adapted weights are rebuilt from the placed base weights on the next call
    // A merged update (blim_train_merge) stays marked until EVERY adapted matrix has been re-placed: reloading one tensor -- a norm, a bias, one projection -- must
    // not lift the "update would apply twice" guard of blim_load_adapter while the other projections still hold W + s B A.
    e->merged_pending.erase(name);
    if (e->merged_pending.empty()) e->lora_merged = false;
    return BLIM_OK;
}

static std::vector<std::string> all_weight_names(const blim_engine* e) {
    std::vector<std::string> n = {"embed_tokens", "final_norm", "lm_head", "visual_head"};
    for (const char* p : {"mlp", "tvg_mlp"}) for (const char* t : {"0.w", "0.b", "2.w", "2.b"}) n.push_back(std::string(p) + "." + t);
    for (int i = 0; i < e->c.num_layers; ++i)
        for (const char* t : {"input_norm", "post_norm", "q_proj.w", "q_proj.b", "k_proj.w", "k_proj.b", "v_proj.w", "v_proj.b", "o_proj.w",
                              "gate_proj.w", "up_proj.w", "down_proj.w"})
            n.push_back("layers." + std::to_string(i) + "." + t);
    return n;
}

extern "C" int blim_load_weight(blim_engine* e, const char* name, const void* data, int32_t dtype, int32_t on_device) {
    ARG_CHECK(e && name && data && (dtype == BLIM_DTYPE_F32 || dtype == BLIM_DTYPE_BF16));
    WeightSlot s;
    if (!find_slot(e, name, s)) { blim_set_error("unknown weight name '%s'", name); return BLIM_ERR_ARG; }
    const void* src = data;
    if (!on_device) {
        const size_t bytes = (size_t)s.rows * s.cols * (dtype == BLIM_DTYPE_F32 ? 4 : 2);
        TRY(ensure(e->stage, bytes));
        HIP_TRY(hipMemcpy(e->stage.p, data, bytes, hipMemcpyHostToDevice));
        src = e->stage.p;
    }
    e->weights_epoch++;
    TRY(place_weight(e, name, src, dtype));
    HIP_TRY(hipDeviceSynchronize());
    return BLIM_OK;
}

static uint64_t fnv1a64(const char* s) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (; *s; ++s) { h ^= (uint8_t)*s; h *= 0x100000001B3ull; }
    return h;
}
static const double kSigma4 = 37837.22723328507;  // sqrt(4 * (65536^2 - 1) / 12)

extern "C" int blim_init_synthetic_weights(blim_engine* e, uint64_t seed) {
    ARG_CHECK(e);
    e->weights_epoch++;
    for (const std::string& name : all_weight_names(e)) {
        WeightSlot s;
        if (!find_slot(e, name, s)) { blim_set_error("internal: no slot for %s", name.c_str()); return BLIM_ERR_STATE; }
        const int64_t n = s.rows * s.cols;
        const bool is_norm = name.size() >= 4 && name.compare(name.size() - 4, 4, "norm") == 0;
        const float std_ = is_norm ? 0.1f : 0.02f, mean = is_norm ? 1.0f : 0.0f;
        const float scale = (float)((double)std_ / kSigma4);
        if (s.kind == 0) {
            TRY(ensure(e->stage, (size_t)n * 2));
            TRY(launch_fill_bell_bf16((bf16_t*)e->stage.p, n, seed, fnv1a64(name.c_str()), scale, mean, 0));
            TRY(place_weight(e, name, e->stage.p, BLIM_DTYPE_BF16));
        } else {
            TRY(ensure(e->stage, (size_t)n * 4));
            TRY(launch_fill_bell_f32((float*)e->stage.p, n, seed, fnv1a64(name.c_str()), scale, mean, 1, 0));
            TRY(place_weight(e, name, e->stage.p, BLIM_DTYPE_F32));
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    return BLIM_OK;
}

extern "C" int blim_weights_ready(const blim_engine* e) {
    ARG_CHECK(e);
    for (const std::string& n : all_weight_names(e)) {
        auto it = e->loaded.find(n);
        if (it == e->loaded.end()) { blim_set_error("weight '%s' not loaded", n.c_str()); return BLIM_ERR_STATE; }
    }
    return BLIM_OK;
}

// ---------------------------------------------------------------------------- content fingerprints (kernels.hpp: launch_hash_device, the definition)
static AdapterW* find_adapter(blim_engine* e, const std::string& name, int* n_out, int* n_in);
struct HashItem { std::string name; std::vector<int64_t> shape; const void* p; int64_t bytes; };

// digests of device buffers: every buffer's two sums in one device array, one copy back, hash_finalize on the host -> dig[2 i], dig[2 i + 1]
static int hash_items(const std::vector<HashItem>& items, hipStream_t s, std::vector<uint64_t>& dig) {
    const size_t n = items.size();
    dig.assign(2 * n, 0);
    if (!n) return BLIM_OK;
    unsigned long long* acc = nullptr;
    HIP_TRY(hipMalloc((void**)&acc, 16 * n));
    std::vector<uint64_t> sums(2 * n, 0);
    int rc = BLIM_OK;
    if (hipMemsetAsync(acc, 0, 16 * n, s) != hipSuccess) { blim_set_error("hash: hipMemsetAsync failed"); rc = BLIM_ERR_HIP; }
    for (size_t i = 0; i < n && rc == BLIM_OK; ++i) rc = launch_hash_device(items[i].p, items[i].bytes, acc + 2 * i, 0, s);
    if (rc == BLIM_OK && (hipMemcpyAsync(sums.data(), acc, 16 * n, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) {
        blim_set_error("hash: copying the sums back failed");
        rc = BLIM_ERR_HIP;
    }
    hipFree(acc);
    if (rc != BLIM_OK) return rc;
    for (size_t i = 0; i < n; ++i) hash_finalize(&sums[2 * i], items[i].bytes, &dig[2 * i]);
    return BLIM_OK;
}
// the same definition over a host buffer (the fingerprint's manifest)
static void hash_host(const std::vector<uint8_t>& b, uint64_t out[2]) {
    uint64_t sums[2] = {0, 0};
    const int64_t n = (int64_t)b.size();
    for (int64_t i = 0; i < (n + 7) / 8; ++i) {
        uint64_t w = 0;
        for (int k = 0; k < 8 && 8 * i + k < n; ++k) w |= (uint64_t)b[8 * i + k] << (8 * k);
        sums[0] += hash_mix1(w ^ ((uint64_t)(i + 1) * HASH_C1));
        sums[1] += hash_mix2(w ^ ((uint64_t)(i + 1) * HASH_C2));
    }
    hash_finalize(sums, n, out);
}

extern "C" int blim_hash_device(const void* p, int64_t bytes, uint64_t out[2], void* stream) {
    ARG_CHECK(out && bytes >= 0 && (p || bytes == 0));
    std::vector<uint64_t> d;
    TRY(hash_items({HashItem{"", {bytes}, p, bytes}}, (hipStream_t)stream, d));
    out[0] = d[0]; out[1] = d[1];
    return BLIM_OK;
}

// Everything the scores depend on, as the kernels read it: the placed base tensors (fused q|k|v, interleaved gate|up, 16-bit copies; norms and biases in f32), the
// visual head's [hi | lo | hi] rows, the f32 A / B of every adapter kept apart, and the config.  Not the derived images (e4m3 / e2m3 copies, augmented weights: rebuilt
// from these) nor the video vocabulary (per evaluation).  Per-tensor digests in name order, each with its name and shape, then the hash of that manifest.
extern "C" int blim_weights_fingerprint(blim_engine* e, uint64_t out[2], void* stream) {
    ARG_CHECK(e && out);
    TRY(blim_weights_ready(e));
    const blim_config& c = e->c;
    const int64_t H = c.hidden_size, I = c.intermediate_size, V = c.vocab_size, M = c.mm_hidden_size;
    std::vector<HashItem> items;
    auto add = [&](const std::string& name, const void* p, std::vector<int64_t> shape, int64_t elem) {
        int64_t bytes = elem;
        for (int64_t d : shape) bytes *= d;
        items.push_back(HashItem{name, shape, p, bytes});
    };
    add("embed_tokens", e->embed, {V, H}, 2);
    add("lm_head", e->lm_head, {V, H}, 2);
    add("visual_head", e->visual_head, {M, H}, 2);
    if (e->visual_head3.p) add("visual_head:hilo", e->visual_head3.p, {M, 3 * H}, 2);
    add("final_norm", e->final_norm, {H}, 4);
    for (int w = 0; w < 2; ++w) {
        const std::string p = w ? "tvg_mlp." : "mlp.";
        add(p + "0.w", e->mlp_w0[w], {H, M}, 2); add(p + "0.b", e->mlp_b0[w], {H}, 4);
        add(p + "2.w", e->mlp_w2[w], {H, H}, 2); add(p + "2.b", e->mlp_b2[w], {H}, 4);
    }
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = "layers." + std::to_string(i) + ".";
        const LayerW& l = e->L[i];
        add(p + "input_norm", l.norm1, {H}, 4); add(p + "post_norm", l.norm2, {H}, 4);
        add(p + "qkv.w", l.wqkv, {e->qkv_n, H}, 2); add(p + "qkv.b", l.bqkv, {e->qkv_n}, 4);
        add(p + "o_proj.w", l.wo, {H, H}, 2); add(p + "gate_up.w", l.wgu, {2 * I, H}, 2); add(p + "down_proj.w", l.wd, {H, I}, 2);
    }
    std::vector<std::string> adapted = {"lm_head", "mlp.0.w", "mlp.2.w", "tvg_mlp.0.w", "tvg_mlp.2.w"};
    if (!e->AD.empty())
        for (int i = 0; i < c.num_layers; ++i)
            for (const char* t : {"q_proj.w", "k_proj.w", "v_proj.w", "o_proj.w"}) adapted.push_back("layers." + std::to_string(i) + "." + t);
    for (const std::string& n : adapted) {
        int n_out = 0, n_in = 0;
        const AdapterW* a = find_adapter(e, n, &n_out, &n_in);
        if (!a || !a->A) continue;
        add(n + ":lora_A", a->A, {e->lora_r, a->n_in}, 4);
        add(n + ":lora_B", a->B, {a->n_out, e->lora_r}, 4);
    }
    std::sort(items.begin(), items.end(), [](const HashItem& a, const HashItem& b) { return a.name < b.name; });
    std::vector<uint64_t> dig;
    TRY(hash_items(items, (hipStream_t)stream, dig));
    std::vector<uint8_t> m;
    auto put = [&](const void* p, size_t n) { m.insert(m.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    const char tag[] = "blim weights fingerprint v1";
    put(tag, sizeof(tag));
    const int32_t cfg[] = {c.vocab_size, c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads, c.num_kv_heads, c.mm_hidden_size, c.num_clips,
                           e->f8 ? BLIM_COMPUTE_F8 : c.compute_dtype, e->lora_r};
    const float cfg_f[] = {c.rms_eps, c.rope_theta, e->lora_scale};
    put(cfg, sizeof(cfg));
    put(cfg_f, sizeof(cfg_f));
    for (size_t i = 0; i < items.size(); ++i) {
        put(items[i].name.c_str(), items[i].name.size() + 1);
        const int64_t nd = (int64_t)items[i].shape.size();
        put(&nd, 8);
        put(items[i].shape.data(), 8 * items[i].shape.size());
        put(&dig[2 * i], 16);
    }
    hash_host(m, out);
    return BLIM_OK;
}

// fp8 mode: (re)build the e4m3 copies of the big matrices from the placed 16-bit ones (per stored row: scale = absmax / 448)
static int finalize_f8(blim_engine* e) {
    if (!e->f8 || e->f8_ready) return BLIM_OK;
    TRY(blim_weights_ready(e));
    const blim_config& c = e->c;
    const int H = c.hidden_size, I = c.intermediate_size;
    for (auto& l : e->L) {
        TRY(launch_quant_rows(l.wqkv, H, e->qkv_n, H, c.compute_dtype, l.wqkv8, l.sqkv, 0));
        TRY(launch_quant_rows(l.wo, H, H, H, c.compute_dtype, l.wo8, l.so, 0));
        TRY(launch_quant_rows(l.wgu, H, 2 * (int64_t)I, H, c.compute_dtype, l.wgu8, l.sgu, 0));
        TRY(launch_quant_rows(l.wd, I, H, I, c.compute_dtype, l.wd8, l.sd, 0));
    }
    TRY(launch_quant_rows(e->lm_head, H, c.vocab_size, H, c.compute_dtype, e->lm_head8, e->s_lm, 0));
    HIP_TRY(hipDeviceSynchronize());
    e->f8_ready = true;
    return BLIM_OK;
}

static int build_aug(blim_engine* e);
// option "precise_lo6": the e2m3 tile images of the weights the compensated GEMMs' second pass reads (kernels.hpp: launch_f6_tiles).  Derived state, kept per matrix:
// an image is rebuilt when its source matrix was (re)placed since (c6_dirty), the augmented matrices' images when the augmented matrices were rebuilt -- loading new
// adapters every epoch (training.py: adapters_into_engine) does not touch the MLP's images.  Allocation failures say what was being built.
static int c6_alloc(blim_engine* e, uint8_t** q, size_t bytes, bool aug, const char* what) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        blim_set_error("option 'precise_lo6': out of device memory for the e2m3 image of %s (%zu MB; the images take 0.78 byte per decoder / head weight: "
                       "set option 'precise_lo6' = 0 to run the second pass on the 16-bit weights instead)", what, bytes >> 20);
        return BLIM_ERR_NOMEM;
    }
    (aug ? e->aug_owned : e->owned).push_back(p);
    *q = (uint8_t*)p;
    return BLIM_OK;
}
static int finalize_lo6(blim_engine* e) {
    if (!e->lo6 || e->lo6_ready) return BLIM_OK;
    TRY(blim_weights_ready(e));
    const blim_config& c = e->c;
    const int H = c.hidden_size, I = c.intermediate_size, dt = c.compute_dtype;
    auto base = [&](uint8_t** img, const bf16_t* w, int64_t n, int K, const char* what) -> int {
        if (*img && !e->c6_dirty.count((const void*)w)) return BLIM_OK;
        if (!*img) TRY(c6_alloc(e, img, f6_tiles_bytes(n, K), false, what));
        return launch_f6_tiles(w, K, n, K, dt, true, *img, 0);
    };
    for (auto& l : e->L) {
        // adapters apart: QKV and o_proj read the augmented matrices' images only -- the base images are not built (0.6 GB at 7B and two quantisation passes per layer saved);
        // their matrices stay in c6_dirty (below), so the images are built once the adapters are cleared
        if (!e->aug) { TRY(base(&l.wqkv6, l.wqkv, e->qkv_n, H, "q/k/v_proj")); TRY(base(&l.wo6, l.wo, H, H, "o_proj")); }
        TRY(base(&l.wgu6, l.wgu, 2 * (int64_t)I, H, "gate/up_proj")); TRY(base(&l.wd6, l.wd, H, I, "down_proj"));
    }
    if (e->aug) {                         // adapters apart: the adapted projections' augmented weights [W | B_hi | B_lo | 0] (K = H + aug, a multiple of 128)
        TRY(build_aug(e));
        const int Hq = H + e->aug;
        for (auto& d : e->AD) {
            if (d.wqkv_aug6) continue;                                    // built since the augmented matrices were (free_aug clears the pointers)
            TRY(c6_alloc(e, &d.wqkv_aug6, f6_tiles_bytes(e->qkv_n, Hq), true, "q/k/v_proj + adapters")); TRY(c6_alloc(e, &d.wo_aug6, f6_tiles_bytes(H, Hq), true, "o_proj + adapters"));
            TRY(launch_f6_tiles(d.wqkv_aug, Hq, e->qkv_n, Hq, dt, true, d.wqkv_aug6, 0));
            TRY(launch_f6_tiles(d.wo_aug, Hq, H, Hq, dt, true, d.wo_aug6, 0));
        }
    }
    {   // lm_head: the augmented copy when adapters are apart (rebuilt with them), the base matrix otherwise
        const int Hl = H + e->aug;
        const bf16_t* src = e->aug ? (const bf16_t*)e->lm_aug : e->lm_head;
        if (e->lm6_k != Hl) {
            if (e->lm6) { hipFree(e->lm6); e->lm6 = nullptr; }
            if (hipMalloc((void**)&e->lm6, f6_tiles_bytes(c.vocab_size, Hl)) != hipSuccess) {
                (void)hipGetLastError(); e->lm6 = nullptr; e->lm6_k = 0;
                blim_set_error("option 'precise_lo6': out of device memory for the e2m3 image of lm_head (%zu MB)", f6_tiles_bytes(c.vocab_size, Hl) >> 20);
                return BLIM_ERR_NOMEM;
            }
            e->lm6_k = Hl; e->lm6_src = nullptr;
        }
        if (e->lm6_src != (const void*)src || e->aug || e->c6_dirty.count((const void*)e->lm_head)) TRY(launch_f6_tiles(src, Hl, c.vocab_size, Hl, dt, true, e->lm6, 0));
        e->lm6_src = (const void*)src;
    }
    HIP_TRY(hipDeviceSynchronize());
    if (e->aug) {                         // (skipped above: still to be derived when the adapters go)
        std::set<const void*> keep;
        for (auto& l : e->L) { if (!l.wqkv6 || e->c6_dirty.count((const void*)l.wqkv)) keep.insert((const void*)l.wqkv); if (!l.wo6 || e->c6_dirty.count((const void*)l.wo)) keep.insert((const void*)l.wo); }
        e->c6_dirty.swap(keep);
    } else e->c6_dirty.clear();
    e->lo6_ready = true;
    return BLIM_OK;
}

// ---------------------------------------------------------------------------- LoRA adapters kept apart (adapters.hpp)
// main.py:96-105: peft LoRA on the projector MLPs' Linear "0" / "2", on every q/k/v/o_proj and on lm_head; main.py:125-128 loads the fine-tuned
// A / B.  The reference evaluates with the adapters APART (y = W x + b + (alpha / r) B (A x)); so does this engine once adapters are loaded.
static AdapterW* find_adapter(blim_engine* e, const std::string& name, int* n_out, int* n_in) {
    const blim_config& c = e->c;
    const int H = c.hidden_size, M = c.mm_hidden_size, V = c.vocab_size, qn = c.num_heads * 128, kn = c.num_kv_heads * 128;
    auto hit = [&](AdapterW* a, int o, int i) { *n_out = o; *n_in = i; return a; };
    if (name == "lm_head") return hit(&e->ad_lm, V, H);
    for (int w = 0; w < 2; ++w) {
        const std::string p = w ? "tvg_mlp." : "mlp.";
        if (name == p + "0.w") return hit(&e->ad_mlp[w][0], H, M);
        if (name == p + "2.w") return hit(&e->ad_mlp[w][1], H, H);
    }
    int li = -1; char rest[64] = "";
    if (sscanf(name.c_str(), "layers.%d.%63s", &li, rest) == 2 && li >= 0 && li < c.num_layers) {
        const std::string r(rest);
        if (r == "q_proj.w") return hit(&e->AD[li].ad[0], qn, H);
        if (r == "k_proj.w") return hit(&e->AD[li].ad[1], kn, H);
        if (r == "v_proj.w") return hit(&e->AD[li].ad[2], kn, H);
        if (r == "o_proj.w") return hit(&e->AD[li].ad[3], H, H);
    }
    return nullptr;
}

static void free_aug(blim_engine* e) {
    for (void* p : e->aug_owned) hipFree(p);
    e->aug_owned.clear();
    for (auto& l : e->AD) { l.wqkv_aug = l.wo_aug = nullptr; l.wqkv_aug6 = l.wo_aug6 = nullptr; for (auto& a : l.ad) a.A16 = nullptr; }
    e->lm_aug = nullptr; e->ad_lm.A16 = nullptr;
    for (int w = 0; w < 2; ++w) { e->w0_aug[w] = e->w2_aug[w] = nullptr; e->ad_mlp[w][0].A16 = e->ad_mlp[w][1].A16 = nullptr; }
    e->aug_ready = false;
    e->lo6_ready = false;                 // (the e2m3 images of the augmented weights went with them; the base matrices' images stay)
}

extern "C" int blim_clear_adapters(blim_engine* e) {
    ARG_CHECK(e);
    e->weights_epoch++;
    HIP_TRY(hipDeviceSynchronize());
    free_aug(e);
    for (void* p : e->ad_owned) hipFree(p);
    e->ad_owned.clear();
    e->AD.clear();
    e->ad_lm = AdapterW();
    for (int w = 0; w < 2; ++w) e->ad_mlp[w][0] = e->ad_mlp[w][1] = AdapterW();
    e->lora_r = 0; e->lora_scale = 0.f; e->aug = 0;
    return BLIM_OK;
}

static std::vector<AdapterW*> all_adapters(blim_engine* e) {
    std::vector<AdapterW*> v = {&e->ad_lm, &e->ad_mlp[0][0], &e->ad_mlp[0][1], &e->ad_mlp[1][0], &e->ad_mlp[1][1]};
    for (auto& l : e->AD) for (auto& a : l.ad) v.push_back(&a);
    return v;
}
extern "C" int blim_num_adapters(blim_engine* e) {
    if (!e) return -1;
    int n = 0;
    for (AdapterW* a : all_adapters(e)) n += a->A != nullptr;
    return n;
}

extern "C" int blim_load_adapter(blim_engine* e, const char* weight_name, const float* A, const float* B, int32_t lora_r, float lora_alpha) {
    ARG_CHECK(e && weight_name && A && B && lora_r > 0 && lora_r <= 16 && lora_alpha > 0.f);
    e->weights_epoch++;
    const float scale = lora_alpha / (float)lora_r;
    if (e->lora_r && (e->lora_r != lora_r || e->lora_scale != scale)) {
        blim_set_error("adapter '%s': r = %d, alpha / r = %g, but the engine's adapters have r = %d, alpha / r = %g (one LoraConfig per model, main.py:96-101)", weight_name, lora_r,
                       scale, e->lora_r, e->lora_scale);
        return BLIM_ERR_ARG;
    }
    if (e->lora_merged) {
        blim_set_error("adapter '%s': the engine's base weights hold a merged LoRA update (blim_train_merge); adapters apart on top of it would apply the update twice -- "
                       "load the base weights again first", weight_name);
        return BLIM_ERR_STATE;
    }
    if (e->AD.empty()) e->AD.resize(e->c.num_layers);
    int n_out = 0, n_in = 0;
    AdapterW* a = find_adapter(e, weight_name, &n_out, &n_in);
    if (!a) { blim_set_error("'%s' is not a LoRA-adapted weight (q/k/v/o_proj, lm_head, mlp / tvg_mlp Linear 0 / 2: main.py:96-101)", weight_name); return BLIM_ERR_ARG; }
    if (!a->A) {
        HIP_TRY(hipMalloc((void**)&a->A, (size_t)lora_r * n_in * 4)); e->ad_owned.push_back(a->A);
        HIP_TRY(hipMalloc((void**)&a->B, (size_t)n_out * lora_r * 4)); e->ad_owned.push_back(a->B);
        a->n_in = n_in; a->n_out = n_out;
    }
    HIP_TRY(hipMemcpy(a->A, A, (size_t)lora_r * n_in * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(a->B, B, (size_t)n_out * lora_r * 4, hipMemcpyHostToDevice));
    e->lora_r = lora_r; e->lora_scale = scale;
    // three adapters (q, k, v) x r columns x (B_hi, B_lo) need 6 r columns: 64 suffice up to r = 10.  fp16 engines take 128 whenever the e4m3 second pass of the
    // compensated modes is possible (option "precise_lo6": its K-steps are 128 deep, so the augmented K must stay a multiple of 128)
    const bool lo6_capable = !e->f8 && e->c.hidden_size % 128 == 0 && e->c.intermediate_size % 128 == 0;      // (16-bit engines: fp16 by default, bf16 by option)
    e->aug = (6 * lora_r <= 64 && !lo6_capable) ? 64 : 128;
    e->aug_ready = false;
    return BLIM_OK;
}

// (re)builds the augmented weight copies [W | B_hi | B_lo | 0] and the adapters' 16-bit A operands from the placed base weights
static int build_aug(blim_engine* e) {
    if (!e->aug || e->aug_ready) return BLIM_OK;
    TRY(blim_weights_ready(e));
    HIP_TRY(hipDeviceSynchronize());
    free_aug(e);
    const blim_config& c = e->c;
    const int H = c.hidden_size, M = c.mm_hidden_size, V = c.vocab_size, dt = c.compute_dtype, r = e->lora_r, G = e->aug;
    const int64_t qn = (int64_t)c.num_heads * 128, kn = (int64_t)c.num_kv_heads * 128;
    auto aalloc = [&](uint16_t** p, size_t elems) -> int {
        HIP_TRY(hipMalloc((void**)p, elems * 2));
        e->aug_owned.push_back(*p);
        return BLIM_OK;
    };
    auto copy = [&](uint16_t** dst, const bf16_t* src, int64_t N, int K) -> int {
        TRY(aalloc(dst, (size_t)N * (K + G)));
        return launch_make_aug(*dst, src, N, K, G, 0);
    };
    // B columns of adapter `seg` of `nseg` sharing one augmented matrix: hi at K + seg r, lo at K + nseg r + seg r; its A operand
    // an adapter that was not loaded (partial resume files): its u columns must read as zeros -- a shared all-zero A operand
    uint16_t* zero_a16 = nullptr;
    TRY(aalloc(&zero_a16, (size_t)32 * std::max(H, M)));
    HIP_TRY(hipMemset(zero_a16, 0, (size_t)32 * std::max(H, M) * 2));
    auto place = [&](AdapterW& a, uint16_t* w_aug, int K, int64_t row0, int seg, int nseg, int row_mode) -> int {
        if (!a.A) { a.A16 = zero_a16; return BLIM_OK; }
        TRY(launch_adapter_b_aug(w_aug, K + G, row0, K + seg * r, K + nseg * r + seg * r, a.B, a.n_out, r, row_mode, dt, 0));
        TRY(aalloc(&a.A16, (size_t)32 * K));
        return launch_adapter_a16(a.A16, a.A, K, r, dt, 0);
    };
    for (int li = 0; li < c.num_layers; ++li) {
        const LayerW& l = e->L[li]; LayerAd& d = e->AD[li];
        TRY(copy(&d.wqkv_aug, l.wqkv, e->qkv_n, H));
        TRY(copy(&d.wo_aug, l.wo, H, H));
        TRY(place(d.ad[0], d.wqkv_aug, H, 0, 0, 3, 1));
        TRY(place(d.ad[1], d.wqkv_aug, H, qn, 1, 3, 1));
        TRY(place(d.ad[2], d.wqkv_aug, H, qn + kn, 2, 3, 0));
        TRY(place(d.ad[3], d.wo_aug, H, 0, 0, 1, 0));
    }
    TRY(copy(&e->lm_aug, e->lm_head, V, H));
    TRY(place(e->ad_lm, e->lm_aug, H, 0, 0, 1, 0));
    for (int w = 0; w < 2; ++w) {
        TRY(copy(&e->w0_aug[w], e->mlp_w0[w], H, M));
        TRY(copy(&e->w2_aug[w], e->mlp_w2[w], H, H));
        TRY(place(e->ad_mlp[w][0], e->w0_aug[w], M, 0, 0, 1, 0));
        TRY(place(e->ad_mlp[w][1], e->w2_aug[w], H, 0, 0, 1, 0));
    }
    HIP_TRY(hipDeviceSynchronize());
    e->aug_ready = true;
    return BLIM_OK;
}
// u columns of the augmented rows x16 [n, ldx] (K real columns; hi + lo halves when lo_off > 0) for one adapter / the q, k, v triple
static int adapter_u(blim_engine* e, void* x16, int64_t ldx, int64_t lo_off, int64_t n, int K, const AdapterW* a0, const AdapterW* a1, const AdapterW* a2, hipStream_t s) {
    AdapterDownArgs d;
    d.n = a1 ? 3 : 1;
    d.A16[0] = a0->A16; d.A16[1] = a1 ? a1->A16 : nullptr; d.A16[2] = a2 ? a2->A16 : nullptr;
    return launch_adapter_down((uint16_t*)x16, ldx, lo_off, n, K, d, e->lora_r, e->lora_scale, e->aug, e->c.compute_dtype, s);
}

// ---------------------------------------------------------------------------- workspaces
static int reserve_tokens(blim_engine* e, int64_t T) {
    const blim_config& c = e->c;
    const int64_t Tp = round_up(T, 256) * (e->precise ? 2 : 1);      // precise mode: [hi | lo] rows of twice the width
    if (e->f8) {
        TRY(ensure(e->x8, (size_t)Tp * c.hidden_size));
        TRY(ensure(e->a8, (size_t)Tp * c.hidden_size));
        TRY(ensure(e->act8, (size_t)Tp * c.intermediate_size));
        TRY(ensure(e->rscale, (size_t)Tp * 4 * 4));      // [x | attn | act | label rows] scales
        TRY(ensure(e->act_mx, (size_t)Tp * (c.intermediate_size / 128)));
        TRY(ensure(e->attn_mx, (size_t)Tp * c.num_heads));
    }
    const int64_t Hq = c.hidden_size + e->aug;        // adapters apart: the QKV / o_proj inputs carry `aug` extra columns (adapters.hpp)
    TRY(ensure(e->resid, (size_t)round_up(T, 256) * c.hidden_size * 4));
    TRY(ensure(e->xn, (size_t)Tp * Hq * 2));
    TRY(ensure(e->qkv, (size_t)Tp * e->qkv_n * 2));
    TRY(ensure(e->attn, (size_t)Tp * Hq * 2));
    TRY(ensure(e->act, (size_t)Tp * std::max<int64_t>(c.intermediate_size, Hq) * 2));     // (also holds the last layer's gathered attention rows)
    return BLIM_OK;
}
static int reserve_rows(blim_engine* e, int64_t R) {
    const blim_config& c = e->c;
    const int64_t Rp = round_up(R, 256);
    const int ntn = (c.vocab_size + 255) / 256;
    TRY(ensure(e->hsel, (size_t)Rp * (c.hidden_size + e->aug) * 2 * (e->precise ? 2 : 1)));
    if (e->f8) TRY(ensure(e->hsel8, (size_t)Rp * c.hidden_size + (size_t)Rp * 4));   // e4m3 rows, then their scales
    TRY(ensure(e->lse_part, (size_t)Rp * ntn * sizeof(float2)));
    TRY(ensure(e->lab_logit, (size_t)Rp * 4));
    TRY(ensure(e->logprob, (size_t)Rp * 4));
    return BLIM_OK;
}
extern "C" int blim_reserve(blim_engine* e, int64_t max_tokens, int64_t max_rows) {
    ARG_CHECK(e && max_tokens >= 0 && max_rows >= 0);
    if (max_tokens) TRY(reserve_tokens(e, max_tokens));
    if (max_rows) TRY(reserve_rows(e, max_rows));
    // compensated calls of a "precise_lo6" engine need the weights' e2m3 images (+0.78 B per decoder / head weight) and two tile workspaces: with the weights in place
    // and the compensated mode on they are built HERE -- a shortage of device memory is this call's BLIM_ERR_NOMEM (the matrix named), not a scoring call's
    if (e->lo6 && e->precise && blim_weights_ready(e) == BLIM_OK) {
        TRY(finalize_lo6(e));
        if (max_tokens) {
            const int64_t Hq = e->c.hidden_size + e->aug;
            TRY(ensure(e->a6, f6_tiles_bytes(max_tokens, (int)std::max<int64_t>(e->c.intermediate_size, Hq))));
            if (e->lo6_fuse) TRY(ensure(e->a6b, f6_tiles_bytes(max_tokens, e->c.intermediate_size)));
        }
    }
    return BLIM_OK;
}

// ---------------------------------------------------------------------------- component ops
GemmParams gp(int dt, const void* A, int64_t lda, const void* W, int64_t M, int N, int K, void* C, int64_t ldc) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.dtype = dt;
    p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.M = (int)M; p.N = N; p.K = K; p.C = C; p.ldc = ldc; p.scale = 1.0f;
    p.f16_saturate = 1;
    return p;
}

// A 16-bit GEMM over rows of `lay` halves of width K1 ([hi | lo] for lay = 2) against W [N, K1].  The form decides every field:
//   plain (comp = false):          the hi halves alone (lda = lay * K1, K = K1) -- a plain unit over [hi | lo] rows reads their hi halves only;
//   compensated, A6 == nullptr:    A = [hi | lo], K counts both halves and W is walked twice (w_wrap_k = K1);
//   compensated, A6 != nullptr:    option "precise_lo6" -- the plain product of the hi halves plus, in the same kernel and into the same accumulators (gemm.hip, phase 2),
//                                  the e2m3 pass over the lo halves' operand tiles A6 (kernels.hpp: launch_f6_tiles, or written by the producer) against W's e2m3 image W6.
// C / ldc / lo_off are the output as it really is: 16-bit outputs leave as hi at C and lo at C + lo_off (0 = no lo output).
static GemmParams gp_hilo(int dt, const void* rows, int64_t K1, int lay, const void* W, const uint8_t* W6, int64_t n, int N, void* C, int64_t ldc, int64_t lo_off, bool comp,
                          const uint8_t* A6) {
    const bool wrap = comp && !A6;
    GemmParams p = gp(dt, rows, (comp ? 2 : lay) * K1, W, n, N, (int)(wrap ? 2 * K1 : K1), C, ldc);
    p.lo_off = lo_off;
    if (wrap) p.w_wrap_k = (int)K1;
    if (comp && A6) { p.A6 = A6; p.W6 = W6; p.K6 = (int)K1; }
    return p;
}

extern "C" int blim_project_video(blim_engine* e, const void* feats, int64_t n_rows, int32_t which, void* out, void* stream) {
    ARG_CHECK(e && feats && out && n_rows > 0 && (which == 0 || which == 1));
    TRY(blim_weights_ready(e));
    TRY(build_aug(e));
    hipStream_t s = (hipStream_t)stream;
    const int H = e->c.hidden_size, M = e->c.mm_hidden_size, G = e->aug;
    const int Ha = H + G, Ma = M + G;
    const int pf = e->precise ? 2 : 1;            // compensated mode: the hidden layer and the output travel as [hi | lo] rows of width 2H
    TRY(ensure(e->proj_tmp, (size_t)round_up(n_rows, 256) * Ha * 2 * pf));
    SpanGuard g(e, s, TC_GEMM_OTHER, 2.0 * n_rows * ((double)Ma * H + (double)Ha * H));
    const void* a1 = feats;
    if (G) {    // adapters apart: [feats | u | 0] rows against [W0 | B | 0]
        TRY(ensure(e->feats_aug, (size_t)round_up(n_rows, 256) * Ma * 2));
        TRY(launch_copy_rows16((uint16_t*)e->feats_aug.p, Ma, (const uint16_t*)feats, M, n_rows, M, s));
        TRY(adapter_u(e, e->feats_aug.p, Ma, 0, n_rows, M, &e->ad_mlp[which][0], nullptr, nullptr, s));
        a1 = e->feats_aug.p;
    }
    GemmParams p1 = gp(e->c.compute_dtype, a1, Ma, G ? (const void*)e->w0_aug[which] : (const void*)e->mlp_w0[which], n_rows, H, Ma, e->proj_tmp.p, (int64_t)pf * Ha);
    p1.bias = e->mlp_b0[which]; p1.act = 1;
    if (e->precise) p1.lo_off = Ha;
    TRY(launch_gemm(EPI_BF16, p1, s));
    if (G) TRY(adapter_u(e, e->proj_tmp.p, (int64_t)pf * Ha, e->precise ? Ha : 0, n_rows, H, &e->ad_mlp[which][1], nullptr, nullptr, s));
    GemmParams p2 = gp_hilo(e->c.compute_dtype, e->proj_tmp.p, Ha, pf, G ? (const void*)e->w2_aug[which] : (const void*)e->mlp_w2[which], nullptr, n_rows, H, out, (int64_t)pf * H,
                            e->precise ? H : 0, e->precise, nullptr);
    p2.bias = e->mlp_b2[which];
    TRY(launch_gemm(EPI_BF16, p2, s));
    return BLIM_OK;
}

extern "C" int blim_group_mean(blim_engine* e, const void* in, int64_t n_out, int32_t group, void* out, void* stream) {
    ARG_CHECK(e && in && out);
    return launch_group_mean((bf16_t*)out, (const bf16_t*)in, n_out, group, e->c.hidden_size, e->c.compute_dtype, (hipStream_t)stream, e->precise);
}

extern "C" int blim_assemble(blim_engine* e, const int32_t* src_index, int64_t n_tokens, const void* feats, void* out_embeds, void* stream) {
    ARG_CHECK(e && src_index && out_embeds && n_tokens > 0);
    TRY(blim_weights_ready(e));
    SpanGuard g(e, (hipStream_t)stream, TC_MISC, 0);
    return launch_assemble((bf16_t*)out_embeds, src_index, n_tokens, e->c.hidden_size, e->embed, (const bf16_t*)feats, (hipStream_t)stream, e->precise && e->precise_embeds);
}

static GemmParams gp8(const void* A8, int64_t lda, const float* a_scale, const void* W8, const float* w_scale, int64_t M, int N, int K, void* C, int64_t ldc) {
    GemmParams p = gp(DT_F8, A8, lda, W8, M, N, K, C, ldc);
    p.row_scale = a_scale; p.col_scale = w_scale;
    return p;
}

// cos / sin of every token's position in the QKV epilogue's chunk-major layout (gemm.hpp: rope_rows); also used by train.hip
int engine_rope_rows(blim_engine* e, const blim_batch* b, hipStream_t s, float** out, int64_t* stride) {
    const int64_t T = b->n_tokens;
    TRY(ensure(e->rope_rows, (size_t)round_up(T, 256) * 128 * 4));
    hipLaunchKernelGGL(rope_rows_kernel, dim3((unsigned)((T * 32 + 255) / 256)), dim3(256), 0, s, (float*)e->rope_rows.p, b->positions, e->rope_cos, e->rope_sin, T, round_up(T, 256),
                       e->c.max_positions);
    HIP_TRY(hipGetLastError());
    *out = (float*)e->rope_rows.p; *stride = round_up(T, 256);
    return BLIM_OK;
}

// option "precise_lo6": the lo halves of [hi | lo] rows of half-width K1 as e2m3 operand tiles in the a6 workspace -- the A6 of the GEMM that follows (gp_hilo).  A launch of
// its own, timed as TC_QUANT inside the GEMM's span
static int lo6_tiles(blim_engine* e, hipStream_t s, const bf16_t* rows, int64_t K1, int64_t n, const uint8_t** A6) {
    SpanGuard gq(e, s, TC_QUANT, 0);
    TRY(launch_f6_tiles(rows + K1, 2 * K1, n, (int)K1, e->c.compute_dtype, false, (uint8_t*)e->a6.p, s));
    *A6 = (const uint8_t*)e->a6.p;
    return BLIM_OK;
}
// the decoder layers' o_proj and down launches: options "narrow_gemm" (the plain and w_wrap_k forms) and "narrow_lo6" (the e2m3 second pass); fp8 keeps the 256 x 256 kernel
static GemmParams narrowed(GemmParams p, const blim_engine* e) { p.narrow = e->narrow_gemm; p.narrow_lo6 = e->narrow_lo6; return p; }

// live_rows / n_live (optional): the rows of the final hidden state the caller will read.  In the LAST layer every other row is dead after the
// attention (its K / V were needed, its own output is not): the live rows' attention outputs and residuals are gathered and o_proj, the norm
// and the MLP run on those n_live rows only -- the same values, 1 / num_layers of the post-attention work saved on every row nobody reads
// (the shared video + prompt prefix of a VTG query: 60 % of the tokens at the reference's shapes; the caption prompt of a TVG text).
// *final_resid / *final_is_live tell the caller where the last layer's output sits.
static int run_layers(blim_engine* e, const blim_batch* b, const void* embeds, hipStream_t s, const int32_t* live_rows, int64_t n_live, float** final_resid,
                      bool* final_is_live) {
    const blim_config& c = e->c;
    const int H = c.hidden_size, I = c.intermediate_size;
    const int64_t T = b->n_tokens;
    TRY(build_aug(e));
    TRY(reserve_tokens(e, T));
    TRY(finalize_f8(e));
    if (e->precise) TRY(finalize_lo6(e));      // (plain calls never read the e2m3 images: a plain-only run -- zero-shot, --vtg_precise none -- neither builds nor allocates them)
    float* resid = (float*)e->resid.p;
    const bool prune = e->prune_last && live_rows && n_live > 0 && n_live <= T - T / 16 && !e->f8;
    if (prune) TRY(ensure(e->resid_live, (size_t)round_up(n_live, 256) * H * 4));
    *final_resid = resid; *final_is_live = false;
    bf16_t* xn = (bf16_t*)e->xn.p; bf16_t* qkv = (bf16_t*)e->qkv.p; bf16_t* attn = (bf16_t*)e->attn.p; bf16_t* act = (bf16_t*)e->act.p;
    // fp8 mode: quantised inputs of the four GEMMs and their per-token scales
    const int64_t Tp = round_up(T, 256);
    uint8_t* x8 = (uint8_t*)e->x8.p; uint8_t* a8 = (uint8_t*)e->a8.p; uint8_t* act8 = (uint8_t*)e->act8.p;
    float* sx = (float*)e->rscale.p; float* sa = sx ? sx + Tp : nullptr; float* sact = sx ? sx + 2 * Tp : nullptr;
    {
        SpanGuard g(e, s, TC_MISC, 0);
        if (e->precise && e->precise_embeds) TRY(launch_hilo_to_f32(resid, (const bf16_t*)embeds, T, H, c.compute_dtype, s));     // embeds are [hi | lo] rows
        else TRY(launch_h16_to_f32(resid, (const bf16_t*)embeds, T * H, c.compute_dtype, s));
    }
    const double tok = (double)T;
    // adapters apart (adapters.hpp): the QKV and o_proj GEMMs take [x | u | u | 0] rows of width Hq against [W | B_hi | B_lo | 0]; they then run in the
    // 16-bit format even on an fp8 engine (the rank-r update would not survive an e4m3 K-step; the MLP, 87 % of a layer's flops and not adapted, stays fp8)
    const int G = e->aug;
    const int64_t Hq = H + G;
    const bool q8 = e->f8 && (e->f8_mask & 1) && !G, o8 = e->f8 && (e->f8_mask & 2) && !G, g8 = e->f8 && (e->f8_mask & 4), d8 = e->f8 && (e->f8_mask & 8);
    float* rope_rows = nullptr;
    {
        SpanGuard g(e, s, TC_MISC, 0);
        int64_t stride = 0;
        TRY(engine_rope_rows(e, b, s, &rope_rows, &stride));
    }
    const int pf = e->precise ? 2 : 1;                              // attention branch: row layout
    const bool masked = e->precise && e->layer_mask_on;             // options "precise_layers" / "precise_layer_bits": compensation per (layer, GEMM class)
    const bool pm = e->precise && e->precise_mlp;                   // MLP branch (option "precise_mlp")
    const int pfm = (pm || masked) ? 2 : 1;                         // MLP branch: row layout
    // the compensated units of layer li: bit 0 QKV + attention products, 1 o_proj, 2 gate|up, 3 down.  A unit's producer writes the lo part it reads (RMSNorm 1 -> QKV,
    // QKV epilogue -> attention, attention -> o_proj, RMSNorm 2 -> gate|up, SwiGLU epilogue -> down); a plain unit reads the hi halves of the same layout
    auto unit_bits = [&](int li) -> int { return masked ? (int)e->layer_bits[li] : e->precise ? (pm ? 15 : 3) : 0; };
    if (e->precise && e->f8) { blim_set_error("option 'precise' needs a 16-bit engine (fp16 or bf16)"); return BLIM_ERR_STATE; }
    // option "precise_lo6": a compensated GEMM = its plain fp16 pass over the hi part + an e2m3 pass over the lo part, in one kernel and into the same accumulators
    // (gp_hilo's third form).  The lo halves reach it as e2m3 operand tiles: written into the a6 workspace by lo6_tiles right before the GEMM, or by the rows' producer
    // (below).  With adapters apart the adapted projections use the augmented weights' images.
    const bool lo6 = e->lo6 && e->precise;
    if (lo6) TRY(ensure(e->a6, f6_tiles_bytes(T, (int)std::max<int64_t>(I, Hq))));
    const bool fuse6_ok = lo6 && e->lo6_fuse && (e->lo6_fuse_mask & 1) && (2 * I) % 256 == 0;    // the gate | up epilogue writes the down GEMM's A6 tiles (gemm.hpp: out6) into a second buffer
    bool any_fuse6 = false;                                                                        // (layers whose gate | up and down both run compensated)
    for (int li = 0; li < c.num_layers; ++li) any_fuse6 |= (unit_bits(li) & 12) == 12;
    if (fuse6_ok && any_fuse6) TRY(ensure(e->a6b, f6_tiles_bytes(T, (int)I)));
    // ... and the RMSNorm kernels write the tiles of their own output's lo part (kernels.hpp: launch_rmsnorm out6) -- the rows' lo halves are then stored only for
    // the adapters' rank-r inputs: norm1 -> QKV input when no adapter is apart (with adapters the GEMM input carries their u columns, written after the norm);
    // norm2 -> gate | up input (no adapters on the MLP)
    const bool n1_tiles_ok = lo6 && e->lo6_fuse && (e->lo6_fuse_mask & 2) && !G && rmsnorm_can_write_tiles((int)H, H, pf * Hq);
    const bool n2_tiles_ok = lo6 && e->lo6_fuse && (e->lo6_fuse_mask & 2) && rmsnorm_can_write_tiles((int)H, H, pfm * H);
    const int dt = c.compute_dtype;
    const uint8_t* a6 = (const uint8_t*)e->a6.p; const uint8_t* a6b = (const uint8_t*)e->a6b.p;
    for (int li = 0; li < c.num_layers; ++li) {
        const LayerW& l = e->L[li];
        const int ub = unit_bits(li);
        const bool cA = ub & 1, cO = ub & 2, cG = ub & 4, cD = ub & 8;
        const bool fuse6 = fuse6_ok && cG && cD, n1_tiles = n1_tiles_ok && cA, n2_tiles = n2_tiles_ok && cG;
        {
            SpanGuard g(e, s, TC_NORM, 0);
            if (q8) TRY(launch_rmsnorm_f8(resid, H, T, H, l.norm1, c.rms_eps, x8, sx, s));
            else TRY(launch_rmsnorm(resid, H, nullptr, T, H, l.norm1, c.rms_eps, xn, dt, nullptr, s, 0, pf * Hq, (cA && !n1_tiles) ? xn + Hq : nullptr, true, n1_tiles ? (uint8_t*)a6 : nullptr));
            if (G) TRY(adapter_u(e, xn, pf * Hq, cA ? Hq : 0, T, H, &e->AD[li].ad[0], &e->AD[li].ad[1], &e->AD[li].ad[2], s));
        }
        {
            SpanGuard g(e, s, TC_GEMM_QKV, 2.0 * tok * Hq * e->qkv_n * (cA ? 2 : 1));
            const uint8_t* t6 = n1_tiles ? a6 : nullptr;
            if (lo6 && cA && !n1_tiles) TRY(lo6_tiles(e, s, xn, Hq, T, &t6));
            GemmParams p = q8 ? gp8(x8, H, sx, l.wqkv8, l.sqkv, T, e->qkv_n, H, qkv, e->qkv_n)
                              : gp_hilo(dt, xn, Hq, pf, G ? (const void*)e->AD[li].wqkv_aug : (const void*)l.wqkv, G ? e->AD[li].wqkv_aug6 : l.wqkv6, T, e->qkv_n, qkv, (int64_t)pf * e->qkv_n,
                                        cA ? e->qkv_n : 0, cA, t6);
            p.bias = l.bqkv; p.rope_cols = (c.num_heads + c.num_kv_heads) * 128; p.rope_rows = rope_rows; p.rope_stride = round_up(T, 256);
            p.narrow_qkv = e->narrow_qkv;                                 // option "narrow_qkv": every 16-bit form of this launch is eligible; fp8 keeps the 256 x 256 kernel
            TRY(launch_gemm(EPI_QKV, p, s));
        }
        if (e->pc_fill) {      // gallery fill: this layer's K / V heads of the prefix rows (+ their lo parts where the attention reads them) into the cache slots
            SpanGuard g(e, s, TC_MISC, 0);
            const blim_prefix_cache* pc = e->pc_fill;
            const int kvh = 2 * c.num_kv_heads * 128;
            TRY(launch_kv_capture(qkv, (int64_t)pf * e->qkv_n, (int64_t)c.num_heads * 128, (cA && pc->comp) ? e->qkv_n : 0, kvh, e->pc_cap_row, T,
                                  pc->kv + (int64_t)li * pc->max_len * pc->kv_w, pc->slot_stride, pc->kv_w, kvh, pc->max_len, pc->n_slots, s));
        }
        {
            SpanGuard g(e, s, TC_ATTN, 0);
            AttnParams a;
            a.dtype = dt;
            a.qkv = qkv; a.ldq = (int64_t)pf * e->qkv_n; a.num_heads = c.num_heads; a.num_kv_heads = c.num_kv_heads;
            a.key_visible = b->key_visible; a.seq_start = b->seq_start; a.seq_len = b->seq_len; a.pfx_start = b->pfx_start; a.pfx_len = b->pfx_len;
            a.blk_seq = b->blk_seq; a.blk_q0 = b->blk_q0; a.own_start = b->own_start; a.n_blocks = b->n_blocks; a.out = attn; a.ldo = (int64_t)pf * Hq; a.scale = 0.08838834764831845f;
            a.v_lo_off = cA ? e->qkv_n : 0; a.out_lo_off = cO ? Hq : 0;            // (four forms: attention.hpp)
            a.out8 = nullptr; a.ldo8 = 0; a.out_mx = nullptr; a.mx_stride = 0; a.lse_out = nullptr;
            if (o8 && e->f8_fuse) { a.out8 = a8; a.ldo8 = H; a.out_mx = (uint8_t*)e->attn_mx.p; a.mx_stride = Tp; }   // fp8: e4m3 + E8M0 per (token, head)
            if (e->pc_read) {      // gallery scoring: sequences that name a slot read their prefix tiles from it (attention.hpp: the cached forms)
                const blim_prefix_cache* pc = e->pc_read;
                AttnPcParams pa;
                static_cast<AttnParams&>(pa) = a;
                pa.pfx_cache = pc->kv + (int64_t)li * pc->max_len * pc->kv_w; pa.pfx_slot = e->pc_slot; pa.pc_slot_stride = pc->slot_stride; pa.pc_ld = pc->kv_w;
                pa.pc_lo_off = pc->comp ? 2 * c.num_kv_heads * 128 : 0; pa.pc_n_slots = pc->n_slots; pa.pc_max_len = pc->max_len;
                TRY(launch_attention_cached(pa, s));
            } else {
                TRY(launch_attention(a, e->attn_tr, s));
            }
            if (e->masked_query_zero) TRY(launch_zero_rows(attn, (int64_t)pf * Hq, b->key_visible, T, (int)(pf * Hq), s));
        }
        const bool fuse_o = o8 && e->f8_fuse;
        if (o8 && !fuse_o) { SpanGuard g(e, s, TC_QUANT, 0); TRY(launch_quant_rows(attn, H, T, H, dt, a8, sa, s)); }
        // ---- the post-attention half of the layer: o_proj -> norm 2 -> gate|up -> down over `n` rows: attention outputs `ao`, residual stream `res`.  Every row of the
        // batch -- or, in the last layer of a call that names its rows, those rows alone (`pruned`).  prune requires !e->f8, so every fp8 flag below is false on pruned rows
        const bool pruned = prune && li == c.num_layers - 1;
        bf16_t* ao = attn; int64_t n = T; float* res = resid;
        if (pruned) {       // gather: attention output -> the free `act` workspace [n_live, pf * Hq] (not in use until the gate|up GEMM), residual -> resid_live
            SpanGuard g(e, s, TC_MISC, 0);
            ao = act; n = n_live; res = (float*)e->resid_live.p;
            TRY(launch_gather_rows(ao, attn, live_rows, n, (int64_t)pf * Hq * 2, T, 0u, s));
            if (G) TRY(adapter_u(e, ao, (int64_t)pf * Hq, cO ? Hq : 0, n, H, &e->AD[li].ad[3], nullptr, nullptr, s));
            TRY(launch_gather_rows(res, resid, live_rows, n, (int64_t)H * 4, T, 0x7fc00000u, s));      // a row outside the batch: NaN (poisoned score)
        } else if (G) {
            SpanGuard g(e, s, TC_MISC, 0);
            TRY(adapter_u(e, ao, (int64_t)pf * Hq, cO ? Hq : 0, n, H, &e->AD[li].ad[3], nullptr, nullptr, s));
        }
        const double rows = (double)n;
        {
            SpanGuard g(e, s, TC_GEMM_O, 2.0 * rows * Hq * H * (cO ? 2 : 1));
            const uint8_t* t6 = nullptr;
            if (lo6 && cO) TRY(lo6_tiles(e, s, ao, Hq, n, &t6));
            GemmParams p = o8 ? gp8(a8, H, fuse_o ? nullptr : sa, l.wo8, l.so, n, H, H, res, H)
                              : gp_hilo(dt, ao, Hq, pf, G ? (const void*)e->AD[li].wo_aug : (const void*)l.wo, G ? e->AD[li].wo_aug6 : l.wo6, n, H, res, H, 0, cO, t6);
            if (fuse_o) { p.a_mx = (const uint8_t*)e->attn_mx.p; p.mx_stride = Tp; }
            TRY(launch_gemm(EPI_RESID, narrowed(p, e), s));
        }
        {
            SpanGuard g(e, s, TC_NORM, 0);
            if (g8) TRY(launch_rmsnorm_f8(res, H, n, H, l.norm2, c.rms_eps, x8, sx, s));
            else TRY(launch_rmsnorm(res, H, nullptr, n, H, l.norm2, c.rms_eps, xn, dt, nullptr, s, 0, pfm * H, (cG && !n2_tiles) ? xn + H : nullptr, true, n2_tiles ? (uint8_t*)a6 : nullptr));
        }
        const bool fuse = g8 && d8 && e->f8_fuse;      // fp8: the gate|up epilogue emits e4m3 + one E8M0 scale per (token, 128 outputs) itself
        {   // SwiGLU output [n, pfm * I] into `act`: on pruned rows it held `ao` only until o_proj above has run (stream order), so it is free again here
            SpanGuard g(e, s, TC_GEMM_GATEUP, 4.0 * rows * H * I * (cG ? 2 : 1));
            const uint8_t* t6 = n2_tiles ? a6 : nullptr;
            if (lo6 && cG && !n2_tiles) TRY(lo6_tiles(e, s, xn, H, n, &t6));
            GemmParams p = g8 ? gp8(x8, H, sx, l.wgu8, l.sgu, n, 2 * I, H, fuse ? (void*)act8 : (void*)act, I)
                              : gp_hilo(dt, xn, H, pfm, l.wgu, l.wgu6, n, 2 * I, act, (int64_t)pfm * I, cD ? I : 0, cG, t6);
            if (fuse) { p.out_mx = (uint8_t*)e->act_mx.p; p.mx_stride = Tp; }
            if (fuse6) p.out6 = (uint8_t*)a6b;          // the epilogue writes the down GEMM's A6 tiles (gemm.hpp: out6)
            TRY(launch_gemm(EPI_SWIGLU, p, s));
        }
        if (d8 && !fuse) { SpanGuard g(e, s, TC_QUANT, 0); TRY(launch_quant_rows(act, I, n, I, dt, act8, sact, s)); }
        {
            SpanGuard g(e, s, TC_GEMM_DOWN, 2.0 * rows * H * I * (cD ? 2 : 1));
            const uint8_t* t6 = fuse6 ? a6b : nullptr;
            if (lo6 && cD && !fuse6) TRY(lo6_tiles(e, s, act, I, n, &t6));
            GemmParams p = d8 ? gp8(act8, I, fuse ? nullptr : sact, l.wd8, l.sd, n, H, I, res, H) : gp_hilo(dt, act, I, pfm, l.wd, l.wd6, n, H, res, H, 0, cD, t6);
            if (fuse) { p.a_mx = (const uint8_t*)e->act_mx.p; p.mx_stride = Tp; }
            TRY(launch_gemm(EPI_RESID, narrowed(p, e), s));
        }
        if (pruned) { *final_resid = res; *final_is_live = true; }
    }
    return BLIM_OK;
}

int check_batch(const blim_batch* b) {
    ARG_CHECK(b && b->n_tokens > 0 && b->n_seqs > 0 && b->n_blocks > 0);
    ARG_CHECK(b->positions && b->key_visible && b->seq_start && b->seq_len && b->pfx_start && b->pfx_len && b->blk_seq && b->blk_q0);
    return BLIM_OK;
}

// final-norm hidden states of the selected rows; `split` (precise mode): out16 rows are [hi | lo] of width 2 W; W = width of one half
// (H, or H + aug when the rows go on to the adapted lm_head: adapters.hpp)
static int decode_impl(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* out_rows, int64_t n_out,
                       void* out_hidden_bf16, bool split, float* out_hidden_f32, void* stream, int64_t W = 0) {
    ARG_CHECK(e && embeds && (out_hidden_bf16 || out_hidden_f32));
    TRY(check_batch(b));
    TRY(blim_weights_ready(e));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = out_rows ? n_out : b->n_tokens;
    ARG_CHECK(n > 0);
    float* fr = nullptr; bool is_live = false;
    TRY(run_layers(e, b, embeds, s, out_rows, out_rows ? n_out : 0, &fr, &is_live));
    SpanGuard g(e, s, TC_NORM, 0);
    const int H = e->c.hidden_size;
    if (W == 0) W = H;
    // (is_live: run_layers carried exactly the requested rows, in order, through the last layer: the final norm reads them straight)
    return launch_rmsnorm(fr, H, is_live ? nullptr : out_rows, n, H, e->final_norm, e->c.rms_eps, (bf16_t*)out_hidden_bf16, e->c.compute_dtype,
                          out_hidden_f32, s, is_live ? n : b->n_tokens, split ? 2 * W : W, split && out_hidden_bf16 ? (bf16_t*)out_hidden_bf16 + W : nullptr);
}
extern "C" int blim_decode(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* out_rows, int64_t n_out,
                           void* out_hidden_bf16, float* out_hidden_f32, void* stream) {
    return decode_impl(e, b, embeds, out_rows, n_out, out_hidden_bf16, false, out_hidden_f32, stream);
}

// lm_head's A operand.  Adapters apart: rows [x | u | u | 0] of width H + aug per half -- `hidden` either has that layout already (`wide`: the engine's
// own hsel) or is a caller's [n, (split ? 2 : 1) * H] buffer, staged into hid_aug first; then the u columns are formed.  -> *A, *ld_half
static int lm_head_input(blim_engine* e, const void* hidden, bool split, bool wide, int64_t n_rows, hipStream_t s, const void** A, int64_t* ld_half) {
    const int H = e->c.hidden_size, G = e->aug, pf = split ? 2 : 1;
    *A = hidden; *ld_half = H;
    if (!G) return BLIM_OK;
    TRY(build_aug(e));
    const int64_t Ha = H + G;
    void* x = (void*)hidden;
    if (!wide) {
        TRY(ensure(e->hid_aug, (size_t)round_up(n_rows, 256) * Ha * 2 * pf));
        x = e->hid_aug.p;
        TRY(launch_copy_rows16((uint16_t*)x, pf * Ha, (const uint16_t*)hidden, (int64_t)pf * H, n_rows, H, s));
        if (split) TRY(launch_copy_rows16((uint16_t*)x + Ha, pf * Ha, (const uint16_t*)hidden + H, (int64_t)pf * H, n_rows, H, s));
    }
    TRY(adapter_u(e, x, pf * Ha, split ? Ha : 0, n_rows, H, &e->ad_lm, nullptr, nullptr, s));
    *A = x; *ld_half = Ha;
    return BLIM_OK;
}
static int vtg_logprobs_impl(blim_engine* e, const void* hidden_bf16, bool split, const int32_t* labels, int64_t n_rows, float* logprob, void* stream, bool wide = false);
extern "C" int blim_vtg_logprobs(blim_engine* e, const void* hidden_bf16, const int32_t* labels, int64_t n_rows, float* logprob, void* stream) {
    return vtg_logprobs_impl(e, hidden_bf16, false, labels, n_rows, logprob, stream);
}
static int vtg_logprobs_impl(blim_engine* e, const void* hidden_bf16, bool split, const int32_t* labels, int64_t n_rows, float* logprob, void* stream, bool wide) {
    ARG_CHECK(e && hidden_bf16 && labels && logprob && n_rows > 0);
    TRY(blim_weights_ready(e));
    hipStream_t s = (hipStream_t)stream;
    const int H = e->c.hidden_size, V = e->c.vocab_size;
    if (!wide) TRY(reserve_rows(e, n_rows));
    const int ntn = (V + 255) / 256;
    HIP_TRY(hipMemsetAsync(e->lab_logit.p, 0, (size_t)n_rows * 4, s));
    uint8_t* h8 = nullptr; float* hs = nullptr;
    const bool l8 = e->f8 && (e->f8_mask & 16) && !e->aug;      // adapters apart: lm_head is adapted and runs in the 16-bit format
    const void* A = hidden_bf16; int64_t Hl = H;
    if (!l8) TRY(lm_head_input(e, hidden_bf16, split, wide, n_rows, s, &A, &Hl));
    if (l8) {
        TRY(finalize_f8(e));
        h8 = (uint8_t*)e->hsel8.p; hs = (float*)(h8 + (size_t)round_up(n_rows, 256) * H);
        SpanGuard g(e, s, TC_QUANT, 0);
        TRY(launch_quant_rows((const bf16_t*)hidden_bf16, H, n_rows, H, e->c.compute_dtype, h8, hs, s));
    }
    {
        SpanGuard g(e, s, TC_LMHEAD_LSE, 2.0 * n_rows * (double)Hl * V * (split ? 2 : 1));
        if (split) ARG_CHECK(!l8);
        const uint8_t* h6 = nullptr;
        if (split && e->lo6 && Hl % 128 == 0) {                          // lo6: the rows' lo parts against the head in e2m3 (gemm.hip phase 2), as in the decoder GEMMs
            TRY(finalize_lo6(e));
            TRY(ensure(e->h6, f6_tiles_bytes(n_rows, (int)Hl)));
            TRY(launch_f6_tiles((const bf16_t*)A + Hl, 2 * Hl, n_rows, (int)Hl, e->c.compute_dtype, false, (uint8_t*)e->h6.p, s));
            h6 = (const uint8_t*)e->h6.p;
        }
        GemmParams p = l8 ? gp8(h8, H, hs, e->lm_head8, e->s_lm, n_rows, V, H, nullptr, 0)
                          : gp_hilo(e->c.compute_dtype, A, Hl, split ? 2 : 1, e->aug ? (const void*)e->lm_aug : (const void*)e->lm_head, e->lm6, n_rows, V, nullptr, 0, 0, split, h6);
        p.labels = labels; p.lse_part = (float2*)e->lse_part.p; p.label_logit = (float*)e->lab_logit.p;
        TRY(launch_gemm(EPI_LSE, p, s));
    }
    SpanGuard g(e, s, TC_MISC, 0);
    return launch_lse_combine((const float2*)e->lse_part.p, ntn, (const float*)e->lab_logit.p, labels, n_rows, logprob, s);
}

extern "C" int blim_segment_mean(blim_engine* e, const float* logprob, const int32_t* row_start, int32_t n_pairs, int32_t mode, float* score, void* stream) {
    (void)e;
    return launch_segment_mean(logprob, row_start, n_pairs, mode, score, (hipStream_t)stream);
}

static int lm_head_impl(blim_engine* e, const void* hidden_bf16, bool split, int64_t n_rows, float* logits, void* stream, bool wide = false) {
    ARG_CHECK(e && hidden_bf16 && logits && n_rows > 0);
    TRY(blim_weights_ready(e));
    const int H = e->c.hidden_size, V = e->c.vocab_size;
    const void* A = hidden_bf16; int64_t Hl = H;
    TRY(lm_head_input(e, hidden_bf16, split, wide, n_rows, (hipStream_t)stream, &A, &Hl));
    SpanGuard g(e, (hipStream_t)stream, TC_GEMM_OTHER, 2.0 * n_rows * (double)Hl * V);
    GemmParams p = gp_hilo(e->c.compute_dtype, A, Hl, split ? 2 : 1, e->aug ? (const void*)e->lm_aug : (const void*)e->lm_head, nullptr, n_rows, V, logits, V, 0, split, nullptr);
    return launch_gemm(EPI_F32, p, (hipStream_t)stream);
}
extern "C" int blim_lm_head(blim_engine* e, const void* hidden_bf16, int64_t n_rows, float* logits, void* stream) {
    return lm_head_impl(e, hidden_bf16, false, n_rows, logits, stream);
}

extern "C" int blim_ce_rows(blim_engine* e, const float* logits, int64_t ld, int32_t n_cols, const int32_t* labels, int64_t n_rows, float* logprob, void* stream) {
    (void)e;
    return launch_ce_rows(logits, ld, n_cols, labels, n_rows, logprob, (hipStream_t)stream);
}

// split (precise mode): hidden rows are [hi | lo] of width 2H and the output rows [hi | lo] of width 2M
static int visual_head_impl(blim_engine* e, const void* hidden_bf16, bool split, int64_t n_rows, void* out_bf16, void* stream) {
    ARG_CHECK(e && hidden_bf16 && out_bf16 && n_rows > 0);
    TRY(blim_weights_ready(e));
    const int H = e->c.hidden_size, M = e->c.mm_hidden_size;
    hipStream_t s = (hipStream_t)stream;
    SpanGuard g(e, s, TC_GEMM_OTHER, 2.0 * n_rows * (double)H * M * (split ? 3 : 1));
    if (split) {    // [hi | hi | lo] hidden rows against the head's [hi | lo | hi] rows: one GEMM of depth 3 H, outputs [hi | lo] of width 2 M
        TRY(ensure(e->hs3, (size_t)round_up(n_rows, 256) * 3 * H * 2));
        TRY(launch_split3_hilo((uint16_t*)e->hs3.p, (const uint16_t*)hidden_bf16, 2 * (int64_t)H, n_rows, H, s));
        GemmParams p = gp(e->c.compute_dtype, e->hs3.p, 3 * (int64_t)H, e->visual_head3.p, n_rows, M, 3 * H, out_bf16, 2 * (int64_t)M);
        p.lo_off = M;
        return launch_gemm(EPI_BF16, p, s);
    }
    GemmParams p = gp(e->c.compute_dtype, hidden_bf16, H, e->visual_head, n_rows, M, H, out_bf16, M);
    return launch_gemm(EPI_BF16, p, s);
}
// modeling_videochat_flash.py:598-599 on FLOAT32 hidden states (the literal path hands the final norm's output over as float32): float32 out, three-term product
extern "C" int blim_visual_head_f32(blim_engine* e, const float* hidden_f32, int64_t n_rows, float* out_f32, void* stream) {
    ARG_CHECK(e && hidden_f32 && out_f32 && n_rows > 0);
    TRY(blim_weights_ready(e));
    const int H = e->c.hidden_size, M = e->c.mm_hidden_size;
    hipStream_t s = (hipStream_t)stream;
    TRY(ensure(e->hs3, (size_t)round_up(n_rows, 256) * 3 * H * 2));
    TRY(launch_split3_f32((uint16_t*)e->hs3.p, nullptr, hidden_f32, n_rows, H, 0, e->c.compute_dtype, s));
    SpanGuard g(e, s, TC_GEMM_OTHER, 6.0 * n_rows * (double)H * M);
    GemmParams p = gp(e->c.compute_dtype, e->hs3.p, 3 * (int64_t)H, e->visual_head3.p, n_rows, M, 3 * H, out_f32, M);
    return launch_gemm(EPI_F32, p, s);
}
extern "C" int blim_visual_head(blim_engine* e, const void* hidden_bf16, int64_t n_rows, void* out_bf16, void* stream) {
    return visual_head_impl(e, hidden_bf16, false, n_rows, out_bf16, stream);
}

// The TVG logits' W operand when the caller passes no vocabulary: the one registered with blim_set_video_vocab.
extern "C" int blim_set_video_vocab(blim_engine* e, const float* vocab_f32, int32_t n_vocab, void* stream) {
    ARG_CHECK(e && vocab_f32 && n_vocab > 0);
    const int M = e->c.mm_hidden_size, C = e->c.num_clips;
    const int64_t rows = (int64_t)C * n_vocab;
    TRY(ensure(e->vocab3, (size_t)rows * 3 * M * 2));
    TRY(ensure(e->vocab1, (size_t)rows * M * 2));
    TRY(launch_split3_f32((uint16_t*)e->vocab3.p, (uint16_t*)e->vocab1.p, vocab_f32, rows, M, 1, e->c.compute_dtype, (hipStream_t)stream));
    e->n_vocab = n_vocab;
    return BLIM_OK;
}

// vh rows: plain [n_pairs * C, M]; split: [hi | lo] of width 2 M.  vocab_bf16 == NULL: the registered vocabulary (then the split form runs the three-term
// product (vh_hi + vh_lo) . (v_hi + v_lo) as one GEMM of depth 3 M: adapters.hpp); vh3_ready: e->vh3 already holds the [hi | hi | lo] rows.
static int tvg_logits_impl(blim_engine* e, const void* vh_bf16, bool split, const void* vocab_bf16, int32_t n_vocab, int32_t n_pairs, float* logits, void* stream, bool vh3_ready = false) {
    ARG_CHECK(e && (vh_bf16 || vh3_ready) && logits && n_vocab > 0 && n_pairs > 0);
    hipStream_t s = (hipStream_t)stream;
    const int M = e->c.mm_hidden_size, C = e->c.num_clips;
    const int pf = split ? 2 : 1;
    SpanGuard g(e, s, TC_GEMM_OTHER, 2.0 * n_pairs * C * (double)M * n_vocab);
    if (!vocab_bf16) {
        if (!e->vocab3.p || e->n_vocab != n_vocab) { blim_set_error("no video vocabulary of %d entries registered (blim_set_video_vocab)", n_vocab); return BLIM_ERR_STATE; }
        if (split || vh3_ready) {
            if (!vh3_ready) {
                TRY(ensure(e->vh3, (size_t)round_up((int64_t)n_pairs * C, 256) * 3 * M * 2));
                TRY(launch_split3_hilo((uint16_t*)e->vh3.p, (const uint16_t*)vh_bf16, 2 * (int64_t)M, (int64_t)n_pairs * C, M, s));
            }
            for (int c = 0; c < C; ++c) {
                GemmParams p = gp(e->c.compute_dtype, (const bf16_t*)e->vh3.p + (int64_t)c * 3 * M, (int64_t)C * 3 * M, (const bf16_t*)e->vocab3.p + (int64_t)c * n_vocab * 3 * M, n_pairs, n_vocab,
                                  3 * M, logits + (int64_t)c * n_vocab, (int64_t)C * n_vocab);
                p.scale = 1.0f / sqrtf((float)M);
                TRY(launch_gemm(EPI_F32, p, s));
            }
            return BLIM_OK;
        }
        vocab_bf16 = e->vocab1.p;
    }
    for (int c = 0; c < C; ++c) {
        GemmParams p = gp(e->c.compute_dtype, (const bf16_t*)vh_bf16 + (int64_t)c * pf * M, (int64_t)C * pf * M, (const bf16_t*)vocab_bf16 + (int64_t)c * n_vocab * M, n_pairs, n_vocab,
                          pf * M, logits + (int64_t)c * n_vocab, (int64_t)C * n_vocab);
        if (split) p.w_wrap_k = M;
        p.scale = 1.0f / sqrtf((float)M);
        TRY(launch_gemm(EPI_F32, p, s));
    }
    return BLIM_OK;
}
// Literal path (retrieval_utils.py:104-106 on float32 visual-head outputs): logits of vh_f32 [n_pairs * C, M] against the registered vocabulary, three-term product
extern "C" int blim_tvg_logits_f32(blim_engine* e, const float* vh_f32, int32_t n_pairs, float* logits, void* stream) {
    ARG_CHECK(e && vh_f32 && logits && n_pairs > 0);
    if (!e->vocab3.p) { blim_set_error("no video vocabulary registered (blim_set_video_vocab)"); return BLIM_ERR_STATE; }
    const int M = e->c.mm_hidden_size, C = e->c.num_clips;
    TRY(ensure(e->vh3, (size_t)round_up((int64_t)n_pairs * C, 256) * 3 * M * 2));
    TRY(launch_split3_f32((uint16_t*)e->vh3.p, nullptr, vh_f32, (int64_t)n_pairs * C, M, 0, e->c.compute_dtype, (hipStream_t)stream));
    return tvg_logits_impl(e, nullptr, true, nullptr, e->n_vocab, n_pairs, logits, stream, true);
}
extern "C" int blim_tvg_logits(blim_engine* e, const void* vh_bf16, const void* vocab_bf16, int32_t n_vocab, int32_t n_pairs, float* logits, void* stream) {
    return tvg_logits_impl(e, vh_bf16, false, vocab_bf16, n_vocab, n_pairs, logits, stream);
}

static int tvg_scores_impl(blim_engine* e, const void* vh_bf16, bool split, const void* vocab_bf16, int32_t n_vocab, const int32_t* labels,
                           int32_t n_pairs, float* score, void* stream) {
    ARG_CHECK(e && labels && score && n_vocab > 0 && n_pairs > 0);
    hipStream_t s = (hipStream_t)stream;
    const int C = e->c.num_clips;
    TRY(ensure(e->tvg_logits, (size_t)n_pairs * C * n_vocab * 4));
    float* lg = (float*)e->tvg_logits.p;
    TRY(tvg_logits_impl(e, vh_bf16, split, vocab_bf16, n_vocab, n_pairs, lg, stream));
    SpanGuard g(e, s, TC_MISC, 0);
    return launch_tvg_score(lg, n_vocab, n_vocab, labels, n_pairs, C, score, s);
}
extern "C" int blim_tvg_scores(blim_engine* e, const void* vh_bf16, const void* vocab_bf16, int32_t n_vocab, const int32_t* labels,
                               int32_t n_pairs, float* score, void* stream) {
    return tvg_scores_impl(e, vh_bf16, false, vocab_bf16, n_vocab, labels, n_pairs, score, stream);
}

// ---------------------------------------------------------------------------- gallery prefix cache (blim.h: blim_prefix_cache_*)
static PcSnap pc_snap(const blim_engine* e) {
    PcSnap s;
    s.epoch = e->weights_epoch;
    s.mqz = e->masked_query_zero;
    s.precise = e->precise;
    if (e->precise) {
        s.embeds = e->precise_embeds; s.lo6 = e->lo6; s.layers = e->layer_mask_on;
        if (e->layer_mask_on) s.bits = e->layer_bits; else s.mlp = e->precise_mlp;
    }
    return s;
}
static const char* pc_diff(const PcSnap& a, const PcSnap& b) {
    if (a.epoch != b.epoch) return "the weights (a weight, adapter or merge changed them since the fill)";
    if (a.precise != b.precise) return "option 'precise'";
    if (a.embeds != b.embeds) return "option 'precise_embeds'";
    if (a.mlp != b.mlp) return "option 'precise_mlp'";
    if (a.layers != b.layers) return "option 'precise_layers'";
    if (a.bits != b.bits) return "option 'precise_layer_bits'";
    if (a.lo6 != b.lo6) return "option 'precise_lo6'";
    if (a.mqz != b.mqz) return "option 'masked_query_zero'";
    return nullptr;
}
static int pc_dims(const blim_engine* e, int32_t n_slots, int32_t max_len, int32_t compensated, int* kv_w, int* hid_w, int64_t* bytes) {
    ARG_CHECK(e && n_slots > 0 && max_len > 0);
    const blim_config& c = e->c;
    *kv_w = 2 * c.num_kv_heads * 128 * (compensated ? 2 : 1);
    *hid_w = c.hidden_size * (compensated ? 2 : 1);
    *bytes = (int64_t)n_slots * ((int64_t)c.num_layers * max_len * *kv_w + *hid_w) * 2;
    return BLIM_OK;
}
extern "C" int64_t blim_prefix_cache_bytes(const blim_engine* e, int32_t n_slots, int32_t max_len, int32_t compensated) {
    int kv_w = 0, hid_w = 0; int64_t bytes = 0;
    return pc_dims(e, n_slots, max_len, compensated, &kv_w, &hid_w, &bytes) == BLIM_OK ? bytes : -1;
}
extern "C" int blim_prefix_cache_create(blim_engine* e, int32_t n_slots, int32_t max_len, int32_t compensated, blim_prefix_cache** out) {
    ARG_CHECK(out);
    *out = nullptr;
    int kv_w = 0, hid_w = 0; int64_t bytes = 0;
    TRY(pc_dims(e, n_slots, max_len, compensated, &kv_w, &hid_w, &bytes));
    if (e->f8) { blim_set_error("prefix cache: fp8 engines are not supported"); return BLIM_ERR_STATE; }
    if (e->c.hidden_size % 8) { blim_set_error("prefix cache: hidden_size %% 8 != 0"); return BLIM_ERR_ARG; }
    blim_prefix_cache* pc = new blim_prefix_cache();
    pc->e = e; pc->n_slots = n_slots; pc->max_len = max_len; pc->comp = compensated != 0; pc->kv_w = kv_w; pc->hid_w = hid_w;
    pc->slot_stride = (int64_t)e->c.num_layers * max_len * kv_w;
    const size_t kv_bytes = (size_t)n_slots * pc->slot_stride * 2;
    if (hipMalloc((void**)&pc->kv, kv_bytes) != hipSuccess || hipMalloc((void**)&pc->hid, (size_t)n_slots * hid_w * 2) != hipSuccess) {
        (void)hipGetLastError();
        if (pc->kv) hipFree(pc->kv);
        delete pc;
        blim_set_error("prefix cache: out of device memory for %d slots of %d positions (%lld MB)", n_slots, max_len, (long long)(bytes >> 20));
        return BLIM_ERR_NOMEM;
    }
    pc->len.assign(n_slots, -1);
    pc->snap.assign(n_slots, PcSnap());
    *out = pc;
    return BLIM_OK;
}
extern "C" void blim_prefix_cache_destroy(blim_prefix_cache* pc) {
    if (!pc) return;
    (void)hipDeviceSynchronize();
    if (pc->kv) hipFree(pc->kv);
    if (pc->hid) hipFree(pc->hid);
    if (pc->map.p) hipFree(pc->map.p);
    delete pc;
}
extern "C" int blim_prefix_cache_slot_len(const blim_prefix_cache* pc, int32_t slot) {
    ARG_CHECK(pc && slot >= 0 && slot < pc->n_slots);
    return pc->len[slot];
}
// lends the cache to run_layers for one call and takes it back on every exit path
struct PcLease {
    blim_engine* e;
    ~PcLease() { e->pc_fill = nullptr; e->pc_cap_row = nullptr; e->pc_read = nullptr; e->pc_slot = nullptr; }
};
extern "C" int blim_prefix_cache_fill(blim_engine* e, blim_prefix_cache* pc, const blim_batch* b, const void* embeds, const int32_t* slot_of_seq, void* stream) {
    ARG_CHECK(e && pc && pc->e == e && embeds && slot_of_seq);
    TRY(check_batch(b));
    if (b->own_start) { blim_set_error("prefix cache fill: segmented sequences (own_start) are not prefixes"); return BLIM_ERR_ARG; }
    if (e->precise && !pc->comp) { blim_set_error("prefix cache fill: a compensated call needs a cache created with compensated = 1"); return BLIM_ERR_STATE; }
    if (!e->attn_tr) { blim_set_error("prefix cache: option 'attn_tr' must be 1"); return BLIM_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    const int n = b->n_seqs;
    const int64_t T = b->n_tokens;
    std::vector<int32_t> h(3 * (size_t)n);
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(h.data(), b->seq_start, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h.data() + n, b->seq_len, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h.data() + 2 * n, b->pfx_len, (size_t)n * 4, hipMemcpyDeviceToHost));
    // device map: [T] destination row per token | [n] last token per sequence | [n] slot per sequence
    std::vector<int32_t> m((size_t)T + 2 * (size_t)n, -1);
    std::vector<bool> seen(pc->n_slots, false);
    for (int q = 0; q < n; ++q) {
        const int st = h[q], ln = h[n + q], slot = slot_of_seq[q];
        if (h[2 * n + q] != 0) { blim_set_error("prefix cache fill: sequence %d names a prefix of its own", q); return BLIM_ERR_ARG; }
        if (slot < 0 || slot >= pc->n_slots) { blim_set_error("prefix cache fill: slot %d of sequence %d outside 0 .. %d", slot, q, pc->n_slots - 1); return BLIM_ERR_ARG; }
        if (seen[slot]) { blim_set_error("prefix cache fill: slot %d named twice", slot); return BLIM_ERR_ARG; }
        seen[slot] = true;
        if (ln < 1 || ln > pc->max_len || st < 0 || (int64_t)st + ln > T) {
            blim_set_error("prefix cache fill: sequence %d of %d tokens (at %d) does not fit a slot of %d positions in a batch of %lld tokens", q, ln, st, pc->max_len, (long long)T);
            return BLIM_ERR_ARG;
        }
        for (int k = 0; k < ln; ++k) m[(size_t)st + k] = slot * pc->max_len + k;
        m[(size_t)T + q] = st + ln - 1;
        m[(size_t)T + n + q] = slot;
    }
    TRY(ensure(pc->map, m.size() * 4));
    HIP_TRY(hipMemcpy(pc->map.p, m.data(), m.size() * 4, hipMemcpyHostToDevice));
    const int32_t* cap = (const int32_t*)pc->map.p;
    const int32_t* last = cap + T;
    const int32_t* slots = last + n;
    for (int q = 0; q < n; ++q) pc->len[slot_of_seq[q]] = -1;        // a failed fill leaves its slots empty
    TRY(reserve_rows(e, n));
    {
        PcLease lease{e};
        e->pc_fill = pc; e->pc_cap_row = cap;
        TRY(decode_impl(e, b, embeds, last, n, e->hsel.p, e->precise, nullptr, stream));     // rows [hi | lo] of width 2 H (precise) or H
    }
    // the last prefix row's final-norm hidden state (it predicts the first response token): hi (| lo) into the slot's hidden row
    TRY(launch_rows_by_index((uint16_t*)pc->hid, pc->hid_w, (const uint16_t*)e->hsel.p, (int64_t)(e->precise ? 2 : 1) * e->c.hidden_size, slots, n,
                             (e->precise ? 2 : 1) * e->c.hidden_size, pc->n_slots, 0, 0, s));
    const PcSnap now = pc_snap(e);
    for (int q = 0; q < n; ++q) { pc->len[slot_of_seq[q]] = h[n + q]; pc->snap[slot_of_seq[q]] = now; }
    return BLIM_OK;
}
// What the two cached scoring entry points share: the checks of the slots a call reads, and the gather of the slots' stored last-row hidden states.
static int pc_check_read(const blim_engine* e, const blim_prefix_cache* pc, const int32_t* slots_used, int32_t n_used) {
    if (!e->attn_tr) { blim_set_error("prefix cache: option 'attn_tr' must be 1"); return BLIM_ERR_STATE; }
    const PcSnap now = pc_snap(e);
    for (int k = 0; k < n_used; ++k) {
        const int slot = slots_used[k];
        if (slot < 0 || slot >= pc->n_slots) { blim_set_error("prefix cache: slot %d outside 0 .. %d", slot, pc->n_slots - 1); return BLIM_ERR_ARG; }
        if (pc->len[slot] < 0) { blim_set_error("prefix cache: slot %d was never filled", slot); return BLIM_ERR_STATE; }
        if (const char* what = pc_diff(pc->snap[slot], now)) { blim_set_error("prefix cache: slot %d is stale: %s differs from its fill", slot, what); return BLIM_ERR_STATE; }
    }
    if (e->precise && !pc->comp) { blim_set_error("prefix cache: a compensated call needs a cache created with compensated = 1"); return BLIM_ERR_STATE; }
    return BLIM_OK;
}
// a cached row -- rows[r] < 0 -- left a poisoned row in hsel (rows of pf halves of width W): the slot's stored hidden state replaces it, hi, then lo (H values each)
static int pc_gather_rows(blim_engine* e, const blim_prefix_cache* pc, const int32_t* rows, int64_t n_rows, int64_t W, hipStream_t s) {
    const int H = e->c.hidden_size;
    const int64_t pf = e->precise ? 2 : 1;
    const uint16_t nan16 = e->c.compute_dtype == DT_F16 ? 0x7E00 : 0x7FC0;
    TRY(launch_rows_by_index((uint16_t*)e->hsel.p, pf * W, (const uint16_t*)pc->hid, pc->hid_w, rows, n_rows, H, pc->n_slots, 1, nan16, s));
    if (e->precise) TRY(launch_rows_by_index((uint16_t*)e->hsel.p + W, pf * W, (const uint16_t*)pc->hid + H, pc->hid_w, rows, n_rows, H, pc->n_slots, 1, 0, s));
    return BLIM_OK;
}

// An admit call (blim.h: blim_pc_admit): a cached scoring call that also captures the in-batch prefixes it names into slots.  pc_admit_begin checks the admissions --
// host values only, before anything is launched --, marks their slots empty and has the device build the two maps the capture reads from them (kernels.hpp:
// launch_admit_map; the admissions travel as kernel arguments): -> *cap [n_tokens] for launch_kv_capture, *row_slot [n_rows] for the hidden-row copy.  Nothing
// here waits for the device or copies from host memory (the workspace's growth aside, as everywhere): the query path packs its next plan while this one runs.
static int pc_admit_begin(blim_engine* e, blim_prefix_cache* pc, const blim_batch* b, const blim_pc_admit* admits, int32_t n_admit, const int32_t* slots_used,
                          int32_t n_used, int64_t n_rows, hipStream_t s, const int32_t** cap, const int32_t** row_slot) {
    TRY(check_batch(b));
    if (e->f8) { blim_set_error("prefix cache admit: fp8 engines are not supported"); return BLIM_ERR_STATE; }
    const int64_t T = b->n_tokens;
    std::vector<char> mark(pc->n_slots, 0);
    for (int k = 0; k < n_used; ++k) if (slots_used[k] >= 0 && slots_used[k] < pc->n_slots) mark[slots_used[k]] = 1;
    for (int a = 0; a < n_admit; ++a) {
        const blim_pc_admit& q = admits[a];
        if (q.slot < 0 || q.slot >= pc->n_slots) { blim_set_error("prefix cache admit: slot %d of admission %d outside 0 .. %d", q.slot, a, pc->n_slots - 1); return BLIM_ERR_ARG; }
        if (mark[q.slot] == 1) { blim_set_error("prefix cache admit: slot %d is read by this call (slots_used) and admitted in it", q.slot); return BLIM_ERR_ARG; }
        if (mark[q.slot] == 2) { blim_set_error("prefix cache admit: slot %d admitted twice", q.slot); return BLIM_ERR_ARG; }
        mark[q.slot] = 2;
        if (q.seq < 0 || q.seq >= b->n_seqs) { blim_set_error("prefix cache admit: sequence %d of admission %d outside the batch's %d", q.seq, a, b->n_seqs); return BLIM_ERR_ARG; }
        if (q.len < 1 || q.len > pc->max_len || q.start < 0 || (int64_t)q.start + q.len > T) {
            blim_set_error("prefix cache admit: len %d (at %d) of admission %d does not fit a slot of %d positions in a batch of %lld tokens", q.len, q.start, a, pc->max_len, (long long)T);
            return BLIM_ERR_ARG;
        }
        if (q.row < 0 || q.row >= n_rows) { blim_set_error("prefix cache admit: row %d of admission %d outside the call's %lld rows", q.row, a, (long long)n_rows); return BLIM_ERR_ARG; }
    }
    for (int a = 0; a < n_admit; ++a) pc->len[admits[a].slot] = -1;          // a failed call leaves its slots empty
    const size_t n_map = (size_t)T + (size_t)n_rows;
    TRY(ensure(pc->map, n_map * 4));
    int32_t* map = (int32_t*)pc->map.p;
    std::vector<int32_t> adm(5 * (size_t)n_admit);
    for (int a = 0; a < n_admit; ++a) {
        const blim_pc_admit& q = admits[a];
        int32_t* d = adm.data() + 5 * (size_t)a;
        d[0] = q.seq; d[1] = q.slot; d[2] = q.start; d[3] = q.len; d[4] = q.row;
    }
    TRY(launch_admit_map(adm.data(), n_admit, map, T, n_rows, pc->max_len, s));      // (the values are kernel arguments: `adm` need not outlive this line)
    *cap = map; *row_slot = map + T;
    return BLIM_OK;
}
// ... and after the decode: the admitted rows' final-norm hidden states (hsel rows of pf halves of width W) become the slots' hidden rows, hi, then lo (H values
// each), and the slots record their lengths and the state they were computed under, as a fill's do
static int pc_admit_finish(blim_engine* e, blim_prefix_cache* pc, const blim_pc_admit* admits, int32_t n_admit, const int32_t* row_slot, int64_t n_rows, int64_t W,
                           hipStream_t s) {
    const int H = e->c.hidden_size;
    const int64_t pf = e->precise ? 2 : 1;
    TRY(launch_rows_by_index((uint16_t*)pc->hid, pc->hid_w, (const uint16_t*)e->hsel.p, pf * W, row_slot, n_rows, H, pc->n_slots, 0, 0, s));
    if (e->precise) TRY(launch_rows_by_index((uint16_t*)pc->hid + H, pc->hid_w, (const uint16_t*)e->hsel.p + W, pf * W, row_slot, n_rows, H, pc->n_slots, 0, 0, s));
    const PcSnap now = pc_snap(e);
    for (int a = 0; a < n_admit; ++a) { pc->len[admits[a].slot] = admits[a].len; pc->snap[admits[a].slot] = now; }
    return BLIM_OK;
}

// Slot export / import (blim.h: blim_prefix_cache_export / _import).  pc_moves_check is what the two share: every check that needs host values only, before anything
// is launched -> the moves as launch_slot_pack takes them.  `tickets` given: an import (the ticket's magic, geometry and length are checked too).
static int64_t pc_record_bytes(const blim_prefix_cache* pc, int64_t len) {
    return round_up(((int64_t)pc->e->c.num_layers * len * pc->kv_w + pc->hid_w) * 2, 256);
}
extern "C" int64_t blim_prefix_cache_record_bytes(const blim_prefix_cache* pc, int32_t len) {
    if (!pc || len < 1 || len > pc->max_len) return -1;
    return pc_record_bytes(pc, len);
}
static int pc_moves_check(const char* what, blim_engine* e, blim_prefix_cache* pc, const blim_pc_move* moves, int32_t n, const void* staging, int64_t staging_bytes,
                          const blim_pc_ticket* tickets, std::vector<int64_t>* mv) {
    if (n < 1) { blim_set_error("prefix cache %s: n = %d moves (at least 1)", what, n); return BLIM_ERR_ARG; }
    if (e->f8) { blim_set_error("prefix cache %s: fp8 engines are not supported", what); return BLIM_ERR_STATE; }
    if (((uintptr_t)staging & 15) != 0 || staging_bytes < 0) { blim_set_error("prefix cache %s: staging must be 16-byte aligned", what); return BLIM_ERR_ARG; }
    std::vector<char> seen(pc->n_slots, 0);
    std::vector<std::pair<int64_t, int>> span((size_t)n);          // (offset, move), sorted below: neighbours must not overlap
    for (int i = 0; i < n; ++i) {
        const blim_pc_move& m = moves[i];
        if (m.slot < 0 || m.slot >= pc->n_slots) { blim_set_error("prefix cache %s: slot %d of move %d outside 0 .. %d", what, m.slot, i, pc->n_slots - 1); return BLIM_ERR_ARG; }
        if (seen[m.slot]) { blim_set_error("prefix cache %s: slot %d named twice (move %d)", what, m.slot, i); return BLIM_ERR_ARG; }
        seen[m.slot] = 1;
        if (m.offset < 0 || m.offset % 256) { blim_set_error("prefix cache %s: offset %lld of move %d is not a multiple of 256", what, (long long)m.offset, i); return BLIM_ERR_ARG; }
        if (tickets) {
            const blim_pc_ticket& t = tickets[i];
            if (t.magic != BLIM_PC_TICKET_MAGIC) { blim_set_error("prefix cache %s: the ticket of move %d was not written by an export", what, i); return BLIM_ERR_ARG; }
            if (t.num_layers != e->c.num_layers || t.kv_w != pc->kv_w || t.hid_w != pc->hid_w || t.n_bits < 0 || t.n_bits > BLIM_PC_TICKET_LAYERS) {
                blim_set_error("prefix cache %s: the ticket of move %d has another geometry (%d layers, widths %d | %d; this cache: %d, %d | %d)", what, i, t.num_layers, t.kv_w,
                               t.hid_w, e->c.num_layers, pc->kv_w, pc->hid_w);
                return BLIM_ERR_ARG;
            }
            if (m.len < 1 || m.len > pc->max_len || m.len != t.len) {
                blim_set_error("prefix cache %s: len %d of move %d (its ticket: %d) does not fit a slot of %d positions", what, m.len, i, t.len, pc->max_len);
                return BLIM_ERR_ARG;
            }
        } else {
            if (pc->len[m.slot] < 0) { blim_set_error("prefix cache %s: slot %d of move %d was never filled", what, m.slot, i); return BLIM_ERR_STATE; }
            if (m.len != pc->len[m.slot]) { blim_set_error("prefix cache %s: len %d of move %d is not slot %d's filled length %d", what, m.len, i, m.slot, pc->len[m.slot]); return BLIM_ERR_ARG; }
            if (pc->snap[m.slot].bits.size() > BLIM_PC_TICKET_LAYERS) { blim_set_error("prefix cache %s: a ticket holds the bits of %d layers at most", what, BLIM_PC_TICKET_LAYERS); return BLIM_ERR_STATE; }
        }
        if (m.offset > staging_bytes || pc_record_bytes(pc, m.len) > staging_bytes - m.offset) {
            blim_set_error("prefix cache %s: the record of move %d (%lld bytes at %lld) does not fit the staging buffer's %lld bytes", what, i, (long long)pc_record_bytes(pc, m.len),
                           (long long)m.offset, (long long)staging_bytes);
            return BLIM_ERR_ARG;
        }
        span[i] = {m.offset, i};
    }
    std::sort(span.begin(), span.end());
    for (int k = 1; k < n; ++k) {
        const int a = span[k - 1].second, b = span[k].second;
        if (span[k - 1].first + pc_record_bytes(pc, moves[a].len) > span[k].first) { blim_set_error("prefix cache %s: the records of moves %d and %d overlap", what, a, b); return BLIM_ERR_ARG; }
    }
    mv->resize(3 * (size_t)n);
    for (int i = 0; i < n; ++i) { (*mv)[3 * (size_t)i] = moves[i].slot; (*mv)[3 * (size_t)i + 1] = moves[i].len; (*mv)[3 * (size_t)i + 2] = moves[i].offset; }
    return BLIM_OK;
}
extern "C" int blim_prefix_cache_export(blim_engine* e, blim_prefix_cache* pc, const blim_pc_move* moves, int32_t n, void* staging, int64_t staging_bytes,
                                        blim_pc_ticket* tickets_out, void* stream) {
    ARG_CHECK(e && pc && pc->e == e && moves && staging && tickets_out);
    std::vector<int64_t> mv;
    TRY(pc_moves_check("export", e, pc, moves, n, staging, staging_bytes, nullptr, &mv));
    TRY(launch_slot_pack(mv.data(), n, 1, (uint16_t*)pc->kv, (uint16_t*)pc->hid, (uint8_t*)staging, e->c.num_layers, pc->max_len, pc->kv_w, pc->hid_w, (hipStream_t)stream));
    for (int i = 0; i < n; ++i) {                  // the tickets: host values the cache already holds
        const PcSnap& sn = pc->snap[moves[i].slot];
        blim_pc_ticket& t = tickets_out[i];
        memset(&t, 0, sizeof t);
        t.magic = BLIM_PC_TICKET_MAGIC; t.len = moves[i].len; t.num_layers = e->c.num_layers; t.kv_w = pc->kv_w; t.hid_w = pc->hid_w;
        t.precise = sn.precise; t.embeds = sn.embeds; t.mlp = sn.mlp; t.layers = sn.layers; t.lo6 = sn.lo6; t.mqz = sn.mqz; t.epoch = sn.epoch;
        t.n_bits = (int32_t)sn.bits.size();
        if (t.n_bits) memcpy(t.bits, sn.bits.data(), sn.bits.size());
    }
    return BLIM_OK;
}
extern "C" int blim_prefix_cache_import(blim_engine* e, blim_prefix_cache* pc, const blim_pc_move* moves, int32_t n, const void* staging, int64_t staging_bytes,
                                        const blim_pc_ticket* tickets, void* stream) {
    ARG_CHECK(e && pc && pc->e == e && moves && staging && tickets);
    std::vector<int64_t> mv;
    TRY(pc_moves_check("import", e, pc, moves, n, staging, staging_bytes, tickets, &mv));
    for (int i = 0; i < n; ++i) pc->len[moves[i].slot] = -1;          // a failed import leaves its slots empty
    TRY(launch_slot_pack(mv.data(), n, 0, (uint16_t*)pc->kv, (uint16_t*)pc->hid, (uint8_t*)staging, e->c.num_layers, pc->max_len, pc->kv_w, pc->hid_w, (hipStream_t)stream));
    for (int i = 0; i < n; ++i) {                  // the ticket's state, not the engine's: pc_check_read stays the one place that refuses a stale slot
        const blim_pc_ticket& t = tickets[i];
        PcSnap sn;
        sn.epoch = t.epoch; sn.precise = t.precise; sn.embeds = t.embeds; sn.mlp = t.mlp; sn.layers = t.layers; sn.lo6 = t.lo6; sn.mqz = t.mqz;
        sn.bits.assign(t.bits, t.bits + t.n_bits);
        pc->len[moves[i].slot] = t.len; pc->snap[moves[i].slot] = sn;
    }
    return BLIM_OK;
}

// ---------------------------------------------------------------------------- fused scoring
// blim_score_vtg (pc == nullptr), or the same over cached video prefixes: the lease and the gather of the slots' rows around the same three calls
static int score_vtg_impl(blim_engine* e, blim_prefix_cache* pc, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used, const blim_batch* b,
                          const void* embeds, const int32_t* rows, const int32_t* labels, int64_t n_rows, const int32_t* row_start, int32_t n_pairs,
                          float* score, void* stream, const blim_pc_admit* admits = nullptr, int32_t n_admit = 0) {
    if (pc) TRY(pc_check_read(e, pc, slots_used, n_used));
    const int32_t* cap = nullptr; const int32_t* row_slot = nullptr;
    if (n_admit) TRY(pc_admit_begin(e, pc, b, admits, n_admit, slots_used, n_used, n_rows, (hipStream_t)stream, &cap, &row_slot));
    TRY(reserve_rows(e, n_rows));
    const int64_t W = e->c.hidden_size + e->aug;
    {
        PcLease lease{e};
        if (pc) { e->pc_read = pc; e->pc_slot = pfx_slot; }
        if (n_admit) { e->pc_fill = pc; e->pc_cap_row = cap; }
        TRY(decode_impl(e, b, embeds, rows, n_rows, e->hsel.p, e->precise, nullptr, stream, W));   // rows laid out for the adapted lm_head: lm_head_input forms the u columns
    }
    if (n_admit) TRY(pc_admit_finish(e, pc, admits, n_admit, row_slot, n_rows, W, (hipStream_t)stream));
    if (pc) TRY(pc_gather_rows(e, pc, rows, n_rows, W, (hipStream_t)stream));
    TRY(vtg_logprobs_impl(e, e->hsel.p, e->precise, labels, n_rows, (float*)e->logprob.p, stream, true));
    return blim_segment_mean(e, (const float*)e->logprob.p, row_start, n_pairs, 0, score, stream);
}
extern "C" int blim_score_vtg(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, const int32_t* labels,
                              int64_t n_rows, const int32_t* row_start, int32_t n_pairs, float* score, void* stream) {
    ARG_CHECK(e && rows && labels && row_start && score && n_rows > 0 && n_pairs > 0);
    return score_vtg_impl(e, nullptr, nullptr, nullptr, 0, b, embeds, rows, labels, n_rows, row_start, n_pairs, score, stream);
}
extern "C" int blim_score_vtg_cached(blim_engine* e, blim_prefix_cache* pc, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                                     const void* embeds, const int32_t* rows, const int32_t* labels, int64_t n_rows, const int32_t* row_start, int32_t n_pairs,
                                     float* score, void* stream) {
    ARG_CHECK(e && pc && pc->e == e && pfx_slot && (slots_used || n_used == 0) && n_used >= 0 && rows && labels && row_start && score && n_rows > 0 && n_pairs > 0);
    return score_vtg_impl(e, pc, pfx_slot, slots_used, n_used, b, embeds, rows, labels, n_rows, row_start, n_pairs, score, stream);
}
extern "C" int blim_score_vtg_admit(blim_engine* e, blim_prefix_cache* pc, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                                    const blim_pc_admit* admits, int32_t n_admit, const void* embeds, const int32_t* rows, const int32_t* labels, int64_t n_rows,
                                    const int32_t* row_start, int32_t n_pairs, float* score, void* stream) {
    ARG_CHECK(e && pc && pc->e == e && pfx_slot && (slots_used || n_used == 0) && n_used >= 0 && (admits || n_admit == 0) && n_admit >= 0 && rows && labels && row_start &&
              score && n_rows > 0 && n_pairs > 0);
    return score_vtg_impl(e, pc, pfx_slot, slots_used, n_used, b, embeds, rows, labels, n_rows, row_start, n_pairs, score, stream, admits, n_admit);
}

// blim_score_tvg (pc == nullptr), or the same over cached caption prompts: a pair's first row (it predicts clip 0) is the prompt's last row -- of the batch, or of a slot
static int score_tvg_impl(blim_engine* e, blim_prefix_cache* pc, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used, const blim_batch* b,
                          const void* embeds, const int32_t* rows, const void* vocab_bf16, int32_t n_vocab, const int32_t* labels, int32_t n_pairs,
                          float* score, void* stream, const blim_pc_admit* admits = nullptr, int32_t n_admit = 0) {
    if (pc) TRY(pc_check_read(e, pc, slots_used, n_used));
    const int64_t n_rows = (int64_t)n_pairs * e->c.num_clips;
    const int32_t* cap = nullptr; const int32_t* row_slot = nullptr;
    if (n_admit) TRY(pc_admit_begin(e, pc, b, admits, n_admit, slots_used, n_used, n_rows, (hipStream_t)stream, &cap, &row_slot));
    TRY(reserve_rows(e, n_rows));
    TRY(ensure(e->vh, (size_t)round_up(n_rows, 256) * e->c.mm_hidden_size * 2 * (e->precise ? 2 : 1)));
    {
        PcLease lease{e};
        if (pc) { e->pc_read = pc; e->pc_slot = pfx_slot; }
        if (n_admit) { e->pc_fill = pc; e->pc_cap_row = cap; }
        TRY(decode_impl(e, b, embeds, rows, n_rows, e->hsel.p, e->precise, nullptr, stream));
    }
    if (n_admit) TRY(pc_admit_finish(e, pc, admits, n_admit, row_slot, n_rows, e->c.hidden_size, (hipStream_t)stream));
    if (pc) TRY(pc_gather_rows(e, pc, rows, n_rows, e->c.hidden_size, (hipStream_t)stream));
    TRY(visual_head_impl(e, e->hsel.p, e->precise, n_rows, e->vh.p, stream));
    return tvg_scores_impl(e, e->vh.p, e->precise, vocab_bf16, n_vocab, labels, n_pairs, score, stream);
}
extern "C" int blim_score_tvg(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, const void* vocab_bf16,
                              int32_t n_vocab, const int32_t* labels, int32_t n_pairs, float* score, void* stream) {
    ARG_CHECK(e && rows && labels && score && n_pairs > 0);       // vocab_bf16 == NULL: the vocabulary registered with blim_set_video_vocab
    return score_tvg_impl(e, nullptr, nullptr, nullptr, 0, b, embeds, rows, vocab_bf16, n_vocab, labels, n_pairs, score, stream);
}
// blim_score_tvg up to the visual head over the n_rows + n_prior named rows, the clip-0 logits alone against the registered vocabulary -- the c = 0 launch of
// tvg_logits_impl with the rows contiguous: a GEMM row does not depend on the rows beside it -- and the rank kernel over the two row blocks
static int tvg_rank_check_k(int32_t k, int32_t n_vocab);
// the clip-0 logits of the R visual-head rows in e->vh against the registered vocabulary -> e->tvg_logits [R, n_vocab] (the one statement of them: both callers below)
static int tvg_first_logits(blim_engine* e, int64_t R, hipStream_t s) {
    const int N = e->n_vocab, M = e->c.mm_hidden_size;
    TRY(ensure(e->tvg_logits, (size_t)R * N * 4));
    float* lg = (float*)e->tvg_logits.p;
    SpanGuard g(e, s, TC_GEMM_OTHER, 2.0 * R * (double)M * N * (e->precise ? 3 : 1));
    GemmParams p;
    if (e->precise) {
        TRY(ensure(e->vh3, (size_t)round_up(R, 256) * 3 * M * 2));
        TRY(launch_split3_hilo((uint16_t*)e->vh3.p, (const uint16_t*)e->vh.p, 2 * (int64_t)M, R, M, s));
        p = gp(e->c.compute_dtype, e->vh3.p, 3 * (int64_t)M, e->vocab3.p, R, N, 3 * M, lg, N);
    } else {
        p = gp(e->c.compute_dtype, e->vh.p, M, e->vocab1.p, R, N, M, lg, N);
    }
    p.scale = 1.0f / sqrtf((float)M);
    return launch_gemm(EPI_F32, p, s);
}
// blim_score_tvg_first up to and including tvg_first_logits (both entries below, after their own refusals): the decode and the visual head over [rows | prior_rows]
static int tvg_first_decode(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, int32_t n_rows, const int32_t* prior_rows, int32_t n_prior,
                            void* stream) {
    const int M = e->c.mm_hidden_size;
    hipStream_t s = (hipStream_t)stream;
    const int64_t R = (int64_t)n_rows + n_prior;
    TRY(reserve_rows(e, R));
    TRY(ensure(e->vh, (size_t)round_up(R, 256) * M * 2 * (e->precise ? 2 : 1)));
    const int32_t* all = rows;
    if (n_prior) {                                                // [rows | prior_rows] side by side (lab_logit: R ints reserved above, idle in a TVG call)
        int32_t* cat = (int32_t*)e->lab_logit.p;
        HIP_TRY(hipMemcpyAsync(cat, rows, (size_t)n_rows * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(cat + n_rows, prior_rows, (size_t)n_prior * 4, hipMemcpyDeviceToDevice, s));
        all = cat;
    }
    TRY(decode_impl(e, b, embeds, all, R, e->hsel.p, e->precise, nullptr, stream));
    TRY(visual_head_impl(e, e->hsel.p, e->precise, R, e->vh.p, stream));
    return tvg_first_logits(e, R, s);
}
extern "C" int blim_score_tvg_first(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, int32_t n_rows, const int32_t* prior_rows, int32_t n_prior,
                                    const int32_t* prior_of, float alpha, int32_t k, int32_t* idx_out, float* val_out, float* logprob_out, void* stream) {
    ARG_CHECK(e && rows && idx_out && val_out && n_rows > 0 && n_prior >= 0 && (prior_rows || n_prior == 0));
    if (e->f8) { blim_set_error("blim_score_tvg_first: fp8 engines are not supported"); return BLIM_ERR_STATE; }
    if (!e->vocab3.p) { blim_set_error("no video vocabulary registered (blim_set_video_vocab)"); return BLIM_ERR_STATE; }
    const int N = e->n_vocab;
    TRY(tvg_rank_check_k(k, N));
    hipStream_t s = (hipStream_t)stream;
    TRY(tvg_first_decode(e, b, embeds, rows, n_rows, prior_rows, n_prior, stream));
    const float* lg = (const float*)e->tvg_logits.p;
    SpanGuard g(e, s, TC_MISC, 0);
    return launch_tvg_rank(lg, N, N, n_rows, lg + (int64_t)n_rows * N, N, n_prior, prior_of, alpha, k, idx_out, val_out, logprob_out, N, s);
}
static int tvg_rank_within_check(const int32_t* within, const int32_t* within_off, int32_t n_q, int32_t n_within, int32_t k);
extern "C" int blim_score_tvg_first_within(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, int32_t n_rows, const int32_t* prior_rows,
                                           int32_t n_prior, int32_t n_q, const int32_t* row_of, const int32_t* prior_of, const int32_t* within,
                                           const int32_t* within_off, int32_t n_within, float alpha, int32_t k, int32_t* idx_out, float* val_out, void* stream) {
    ARG_CHECK(e && rows && idx_out && val_out && n_rows > 0 && n_prior >= 0 && (prior_rows || n_prior == 0));
    if (e->f8) { blim_set_error("blim_score_tvg_first_within: fp8 engines are not supported"); return BLIM_ERR_STATE; }
    if (!e->vocab3.p) { blim_set_error("no video vocabulary registered (blim_set_video_vocab)"); return BLIM_ERR_STATE; }
    TRY(tvg_rank_within_check(within, within_off, n_q, n_within, k));
    const int N = e->n_vocab;
    hipStream_t s = (hipStream_t)stream;
    TRY(tvg_first_decode(e, b, embeds, rows, n_rows, prior_rows, n_prior, stream));
    const float* lg = (const float*)e->tvg_logits.p;
    SpanGuard g(e, s, TC_MISC, 0);
    return launch_tvg_rank_within(lg, N, N, n_rows, lg + (int64_t)n_rows * N, N, n_prior, n_q, row_of, prior_of, within, within_off, n_within, alpha, k, idx_out,
                                  val_out, s);
}
// The cached counterpart for the other direction: the caption prompts' last rows are the slots' stored hidden rows, so the clip-0 log-probabilities of the named
// vocabulary entries given every slot's prompt need no decode -- per chunk of slots the gather, the visual head, tvg_first_logits and the column kernel
static int tvg_first_chunk_rows(int32_t n_vocab) {
    const int64_t rows = ((int64_t)256 << 20) / (4 * (int64_t)n_vocab);         // the logits workspace stays within 256 MiB
    return (int)(std::max<int64_t>(256, std::min<int64_t>(rows, 1 << 30)) / 256 * 256);
}
extern "C" int blim_tvg_first_cached(blim_engine* e, blim_prefix_cache* pc, const int32_t* slots, int32_t n_slots, const int32_t* cols, int32_t n_cols, float* out,
                                     int64_t ld_out, int32_t chunk_rows, void* stream) {
    if (!e || !pc || !slots || !cols || !out) {
        blim_set_error("blim_tvg_first_cached: %s is null", !e ? "e" : !pc ? "pc" : !slots ? "slots" : !cols ? "cols" : "out");
        return BLIM_ERR_ARG;
    }
    if (e->f8) { blim_set_error("blim_tvg_first_cached: fp8 engines are not supported"); return BLIM_ERR_STATE; }
    if (pc->e != e) { blim_set_error("blim_tvg_first_cached: pc belongs to another engine"); return BLIM_ERR_ARG; }
    if (n_slots < 1) { blim_set_error("blim_tvg_first_cached: n_slots = %d < 1", n_slots); return BLIM_ERR_ARG; }
    if (n_cols < 1) { blim_set_error("blim_tvg_first_cached: n_cols = %d < 1", n_cols); return BLIM_ERR_ARG; }
    if (ld_out < n_slots) { blim_set_error("blim_tvg_first_cached: ld_out = %lld below n_slots = %d", (long long)ld_out, n_slots); return BLIM_ERR_ARG; }
    if (chunk_rows < 0 || chunk_rows % 256) { blim_set_error("blim_tvg_first_cached: chunk_rows = %d is not 0 or a multiple of 256", chunk_rows); return BLIM_ERR_ARG; }
    if (!e->vocab3.p) { blim_set_error("no video vocabulary registered (blim_set_video_vocab)"); return BLIM_ERR_STATE; }
    const int N = e->n_vocab, H = e->c.hidden_size, M = e->c.mm_hidden_size;
    const int chunk = chunk_rows ? chunk_rows : tvg_first_chunk_rows(N);
    hipStream_t s = (hipStream_t)stream;
    TRY(pc_check_read(e, pc, slots, n_slots));                     // every slot of every chunk, before anything is launched
    std::vector<int32_t> neg((size_t)n_slots);
    for (int q = 0; q < n_slots; ++q) neg[q] = -(slots[q] + 1);    // the gather's name of a cached row
    for (int q0 = 0; q0 < n_slots; q0 += chunk) {
        const int R = std::min(chunk, n_slots - q0);
        TRY(reserve_rows(e, R));
        TRY(ensure(e->vh, (size_t)round_up(R, 256) * M * 2 * (e->precise ? 2 : 1)));
        int32_t* rows = (int32_t*)e->lab_logit.p;                  // R ints reserved above, idle in a TVG call
        HIP_TRY(hipMemcpyAsync(rows, neg.data() + q0, (size_t)R * 4, hipMemcpyHostToDevice, s));
        TRY(pc_gather_rows(e, pc, rows, R, H, s));
        TRY(visual_head_impl(e, e->hsel.p, e->precise, R, e->vh.p, stream));
        TRY(tvg_first_logits(e, R, s));
        SpanGuard g(e, s, TC_MISC, 0);
        TRY(launch_tvg_cols((const float*)e->tvg_logits.p, N, N, R, cols, n_cols, out, ld_out, q0, s));
    }
    return BLIM_OK;
}
extern "C" int blim_score_tvg_cached(blim_engine* e, blim_prefix_cache* pc, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                                     const void* embeds, const int32_t* rows, const void* vocab_bf16, int32_t n_vocab, const int32_t* labels, int32_t n_pairs,
                                     float* score, void* stream) {
    ARG_CHECK(e && pc && pc->e == e && pfx_slot && (slots_used || n_used == 0) && n_used >= 0 && rows && labels && score && n_pairs > 0);
    return score_tvg_impl(e, pc, pfx_slot, slots_used, n_used, b, embeds, rows, vocab_bf16, n_vocab, labels, n_pairs, score, stream);
}
extern "C" int blim_score_tvg_admit(blim_engine* e, blim_prefix_cache* pc, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                                    const blim_pc_admit* admits, int32_t n_admit, const void* embeds, const int32_t* rows, const void* vocab_bf16, int32_t n_vocab,
                                    const int32_t* labels, int32_t n_pairs, float* score, void* stream) {
    ARG_CHECK(e && pc && pc->e == e && pfx_slot && (slots_used || n_used == 0) && n_used >= 0 && (admits || n_admit == 0) && n_admit >= 0 && rows && labels && score &&
              n_pairs > 0);
    return score_tvg_impl(e, pc, pfx_slot, slots_used, n_used, b, embeds, rows, vocab_bf16, n_vocab, labels, n_pairs, score, stream, admits, n_admit);
}

// ---------------------------------------------------------------------------- literal forward
extern "C" int blim_forward(blim_engine* e, const void* embeds, const uint8_t* mask, int32_t B, int32_t L, float* logits, float* hidden, void* stream) {
    ARG_CHECK(e && embeds && mask && B > 0 && L > 0 && (logits || hidden));
    ARG_CHECK(L <= e->c.max_positions);
    hipStream_t s = (hipStream_t)stream;
    const int64_t T = (int64_t)B * L;
    const int nbs = (L + 31) / 32;
    const size_t need = (size_t)(T + 3 * (size_t)B + 2 * (size_t)B * nbs) * 4;
    TRY(ensure(e->dense_idx, need));
    int32_t* pos = (int32_t*)e->dense_idx.p;
    int32_t* seq_start = pos + T; int32_t* seq_len = seq_start + B; int32_t* pfx = seq_len + B;
    int32_t* blk_seq = pfx + B; int32_t* blk_q0 = blk_seq + (int64_t)B * nbs;
    const int64_t nthr = std::max<int64_t>(T, (int64_t)B * nbs);
    hipLaunchKernelGGL(dense_batch_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pos, seq_start, seq_len, pfx, blk_seq, blk_q0, B, L, nbs);
    HIP_TRY(hipGetLastError());
    blim_batch b;
    b.n_tokens = T; b.n_seqs = B; b.n_blocks = B * nbs; b.positions = pos; b.key_visible = mask; b.seq_start = seq_start; b.seq_len = seq_len;
    b.pfx_start = pfx; b.pfx_len = pfx; b.blk_seq = blk_seq; b.blk_q0 = blk_q0; b.own_start = nullptr;
    TRY(reserve_rows(e, T));
    TRY(decode_impl(e, &b, embeds, nullptr, 0, e->hsel.p, e->precise, hidden, stream, e->c.hidden_size + e->aug));
    if (logits) TRY(lm_head_impl(e, e->hsel.p, e->precise, T, logits, stream, true));
    return BLIM_OK;
}

// ---------------------------------------------------------------------------- synthetic data, plain GEMM
extern "C" int blim_fill_bell_bf16(void* out, int64_t n, uint64_t seed, const char* name, float std_, float mean, void* stream) {
    ARG_CHECK(out && name && n > 0);
    return launch_fill_bell_bf16((bf16_t*)out, n, seed, fnv1a64(name), (float)((double)std_ / kSigma4), mean, (hipStream_t)stream);
}
extern "C" int blim_fill_bell_f32(float* out, int64_t n, uint64_t seed, const char* name, float std_, float mean, int32_t round_bf16, void* stream) {
    ARG_CHECK(out && name && n > 0);
    return launch_fill_bell_f32(out, n, seed, fnv1a64(name), (float)((double)std_ / kSigma4), mean, round_bf16, (hipStream_t)stream);
}
extern "C" int blim_gemm_bf16(const void* A, int64_t lda, const void* W, int32_t M, int32_t N, int32_t K, void* C, int64_t ldc, void* stream) {
    GemmParams p = gp(DT_BF16, A, lda, W, M, N, K, C, ldc);
    return launch_gemm(EPI_BF16, p, (hipStream_t)stream);
}
extern "C" int blim_gemm_f16(const void* A, int64_t lda, const void* W, int32_t M, int32_t N, int32_t K, void* C, int64_t ldc, void* stream) {
    GemmParams p = gp(DT_F16, A, lda, W, M, N, K, C, ldc);
    return launch_gemm(EPI_BF16, p, (hipStream_t)stream);
}
// The compensated GEMM as a building block (tests): A_hilo [M, 2 K] fp16 rows [hi | lo], W [N, K] fp16 -> C f32 [M, N] = hi . W^T + e2m3(lo) . e2m3(W)^T.  a6 / w6
// receive the e2m3 tile images of the lo part and of W (gemm.hpp; blim_f6_tiles_bytes(M | N, K) bytes each).
extern "C" int64_t blim_f6_tiles_bytes(int64_t n_rows, int32_t K) { return (n_rows > 0 && K > 0 && K % 128 == 0) ? (int64_t)f6_tiles_bytes(n_rows, K) : -1; }
extern "C" int blim_gemm_f16_lo6(const void* A_hilo, const void* W, int32_t M, int32_t N, int32_t K, void* a6, void* w6, float* C, void* stream) {
    ARG_CHECK(A_hilo && W && a6 && w6 && C && K % 128 == 0);
    hipStream_t s = (hipStream_t)stream;
    TRY(launch_f6_tiles((const bf16_t*)W, K, N, K, DT_F16, true, (uint8_t*)w6, s));
    TRY(launch_f6_tiles((const bf16_t*)A_hilo + K, 2 * (int64_t)K, M, K, DT_F16, false, (uint8_t*)a6, s));
    HIP_TRY(hipMemsetAsync(C, 0, (size_t)M * N * 4, s));
    GemmParams p = gp(DT_F16, A_hilo, 2 * (int64_t)K, W, M, N, K, C, N);
    p.A6 = (const uint8_t*)a6; p.W6 = (const uint8_t*)w6; p.K6 = K;
    return launch_gemm(EPI_RESID, p, s);
}
extern "C" int blim_quant_rows(const void* in16, int64_t ld, int64_t n_rows, int32_t K, int32_t dtype16, void* out8, float* scale, void* stream) {
    ARG_CHECK(dtype16 == BLIM_COMPUTE_BF16 || dtype16 == BLIM_COMPUTE_F16);
    return launch_quant_rows((const bf16_t*)in16, ld, n_rows, K, dtype16, (uint8_t*)out8, scale, (hipStream_t)stream);
}
extern "C" int blim_gemm_f8(const void* A8, int64_t lda, const float* a_scale, const void* W8, const float* w_scale, int32_t M, int32_t N, int32_t K,
                            void* C, int64_t ldc, void* stream) {
    GemmParams p = gp8(A8, lda, a_scale, W8, w_scale, M, N, K, C, ldc);
    return launch_gemm(EPI_BF16, p, (hipStream_t)stream);
}
// The scoring path's row kernels alone (tests; blim.h): plain pass-throughs to the launchers of kernels.hpp -- no engine, no state.  The launchers check the
// arguments the engine itself could get wrong; the entries add the ones only a caller of raw pointers can (the dtype, a row stride shorter than the row).
extern "C" int blim_rmsnorm(const blim_rmsnorm_args* args, void* stream) {
    ARG_CHECK(args && args->struct_bytes >= (int64_t)sizeof(blim_rmsnorm_args));
    const blim_rmsnorm_args& a = *args;
    ARG_CHECK(a.dtype16 == BLIM_COMPUTE_BF16 || a.dtype16 == BLIM_COMPUTE_F16);
    ARG_CHECK(a.H > 0 && a.ldx >= a.H && (a.ldo == 0 || a.ldo >= a.H) && a.n_rows <= 0x7fffffffll && (!a.rows || a.n_src > 0));
    return launch_rmsnorm(a.x, a.ldx, a.rows, a.n_rows, a.H, a.w, a.eps, (bf16_t*)a.out16, a.dtype16 == BLIM_COMPUTE_F16 ? DT_F16 : DT_BF16, a.out_f32, (hipStream_t)stream,
                          a.n_src, a.ldo, (bf16_t*)a.out_lo, a.saturate != 0, (uint8_t*)a.out6);
}
extern "C" int blim_rmsnorm_f8(const float* x, int64_t ldx, int64_t n_rows, int32_t H, const float* w, float eps, void* out8, float* scale, void* stream) {
    ARG_CHECK(H > 0 && ldx >= H);
    return launch_rmsnorm_f8(x, ldx, n_rows, H, w, eps, (uint8_t*)out8, scale, (hipStream_t)stream);
}
extern "C" int blim_lse_combine(const float* part, int32_t n_tiles, const float* label_logit, const int32_t* labels, int64_t n_rows, float* logprob, void* stream) {
    return launch_lse_combine((const float2*)part, n_tiles, label_logit, labels, n_rows, logprob, (hipStream_t)stream);
}
extern "C" int blim_tvg_criterion(const float* logits, int64_t ld, int32_t n_vocab, const int32_t* labels, int32_t n_pairs, int32_t clips, float* score, void* stream) {
    ARG_CHECK(ld >= n_vocab);
    return launch_tvg_score(logits, ld, n_vocab, labels, n_pairs, clips, score, (hipStream_t)stream);
}
// blim_tvg_rank's refusals, each naming its argument (shared with blim_score_tvg_first, which checks k before it launches anything)
static_assert(TVG_RANK_MAX_K == BLIM_TVG_RANK_MAX_K, "kernels.hpp and blim.h disagree on the largest k");
static int tvg_rank_check_k(int32_t k, int32_t n_vocab) {
    if (k < 1 || k > n_vocab) { blim_set_error("tvg_rank: k = %d outside 1 .. n_vocab = %d", k, n_vocab); return BLIM_ERR_ARG; }
    if (k > BLIM_TVG_RANK_MAX_K) { blim_set_error("tvg_rank: k = %d above BLIM_TVG_RANK_MAX_K = %d", k, BLIM_TVG_RANK_MAX_K); return BLIM_ERR_ARG; }
    return BLIM_OK;
}
extern "C" int blim_tvg_rank(const float* logits, int64_t ld, int32_t n_vocab, int32_t n_rows, const float* prior_logits, int64_t ld_prior, int32_t n_prior,
                             const int32_t* prior_of, float alpha, int32_t k, int32_t* idx_out, float* val_out, float* logprob_out, int64_t ld_out, void* stream) {
    if (!logits || !idx_out || !val_out) { blim_set_error("tvg_rank: %s is null", !logits ? "logits" : !idx_out ? "idx_out" : "val_out"); return BLIM_ERR_ARG; }
    if (n_vocab < 1) { blim_set_error("tvg_rank: n_vocab = %d < 1", n_vocab); return BLIM_ERR_ARG; }
    if (n_rows < 1) { blim_set_error("tvg_rank: n_rows = %d < 1", n_rows); return BLIM_ERR_ARG; }
    TRY(tvg_rank_check_k(k, n_vocab));
    if (ld < n_vocab) { blim_set_error("tvg_rank: ld = %lld below n_vocab = %d", (long long)ld, n_vocab); return BLIM_ERR_ARG; }
    if (n_prior < 0) { blim_set_error("tvg_rank: n_prior = %d < 0", n_prior); return BLIM_ERR_ARG; }
    if (prior_of && !prior_logits) { blim_set_error("tvg_rank: prior_of without prior_logits"); return BLIM_ERR_ARG; }
    if (prior_logits && ld_prior < n_vocab) { blim_set_error("tvg_rank: ld_prior = %lld below n_vocab = %d", (long long)ld_prior, n_vocab); return BLIM_ERR_ARG; }
    if (logprob_out && ld_out < n_vocab) { blim_set_error("tvg_rank: ld_out = %lld below n_vocab = %d", (long long)ld_out, n_vocab); return BLIM_ERR_ARG; }
    return launch_tvg_rank(logits, ld, n_vocab, n_rows, prior_logits, ld_prior, n_prior, prior_of, alpha, k, idx_out, val_out, logprob_out, ld_out, (hipStream_t)stream);
}
// blim_tvg_rank_within's refusals of its own arguments (shared with blim_score_tvg_first_within, which checks them before it launches anything)
static int tvg_rank_within_check(const int32_t* within, const int32_t* within_off, int32_t n_q, int32_t n_within, int32_t k) {
    if (!within || !within_off) { blim_set_error("tvg_rank_within: %s is null", !within ? "within" : "within_off"); return BLIM_ERR_ARG; }
    if (n_q < 1) { blim_set_error("tvg_rank_within: n_q = %d < 1", n_q); return BLIM_ERR_ARG; }
    if (n_within < 0) { blim_set_error("tvg_rank_within: n_within = %d < 0", n_within); return BLIM_ERR_ARG; }
    if (k < 1) { blim_set_error("tvg_rank_within: k = %d < 1", k); return BLIM_ERR_ARG; }
    if (k > BLIM_TVG_RANK_MAX_K) { blim_set_error("tvg_rank_within: k = %d above BLIM_TVG_RANK_MAX_K = %d", k, BLIM_TVG_RANK_MAX_K); return BLIM_ERR_ARG; }
    return BLIM_OK;
}
extern "C" int blim_tvg_rank_within(const float* logits, int64_t ld, int32_t n_vocab, int32_t n_rows, const float* prior_logits, int64_t ld_prior, int32_t n_prior,
                                    int32_t n_q, const int32_t* row_of, const int32_t* prior_of, const int32_t* within, const int32_t* within_off, int32_t n_within,
                                    float alpha, int32_t k, int32_t* idx_out, float* val_out, void* stream) {
    if (!logits || !idx_out || !val_out) { blim_set_error("tvg_rank_within: %s is null", !logits ? "logits" : !idx_out ? "idx_out" : "val_out"); return BLIM_ERR_ARG; }
    if (n_vocab < 1) { blim_set_error("tvg_rank_within: n_vocab = %d < 1", n_vocab); return BLIM_ERR_ARG; }
    if (n_rows < 1) { blim_set_error("tvg_rank_within: n_rows = %d < 1", n_rows); return BLIM_ERR_ARG; }
    TRY(tvg_rank_within_check(within, within_off, n_q, n_within, k));
    if (ld < n_vocab) { blim_set_error("tvg_rank_within: ld = %lld below n_vocab = %d", (long long)ld, n_vocab); return BLIM_ERR_ARG; }
    if (n_prior < 0) { blim_set_error("tvg_rank_within: n_prior = %d < 0", n_prior); return BLIM_ERR_ARG; }
    if (prior_of && !prior_logits) { blim_set_error("tvg_rank_within: prior_of without prior_logits"); return BLIM_ERR_ARG; }
    if (prior_logits && ld_prior < n_vocab) { blim_set_error("tvg_rank_within: ld_prior = %lld below n_vocab = %d", (long long)ld_prior, n_vocab); return BLIM_ERR_ARG; }
    return launch_tvg_rank_within(logits, ld, n_vocab, n_rows, prior_logits, ld_prior, n_prior, n_q, row_of, prior_of, within, within_off, n_within, alpha, k, idx_out,
                                  val_out, (hipStream_t)stream);
}
extern "C" int blim_rank_rows(const float* values, int64_t ld, int32_t n, int32_t n_rows, int32_t k, int32_t* idx_out, float* val_out, void* stream) {
    if (!values || !idx_out || !val_out) { blim_set_error("rank_rows: %s is null", !values ? "values" : !idx_out ? "idx_out" : "val_out"); return BLIM_ERR_ARG; }
    if (n < 1) { blim_set_error("rank_rows: n = %d < 1", n); return BLIM_ERR_ARG; }
    if (n_rows < 1) { blim_set_error("rank_rows: n_rows = %d < 1", n_rows); return BLIM_ERR_ARG; }
    TRY(tvg_rank_check_k(k, n));
    if (ld < n) { blim_set_error("rank_rows: ld = %lld below n = %d", (long long)ld, n); return BLIM_ERR_ARG; }
    return launch_rank_rows(values, ld, n, n_rows, k, idx_out, val_out, (hipStream_t)stream);
}
extern "C" int blim_tvg_cols(const float* logits, int64_t ld, int32_t n_vocab, int32_t n_rows, const int32_t* cols, int32_t n_cols, float* out, int64_t ld_out,
                             int64_t out0, void* stream) {
    if (!logits || !cols || !out) { blim_set_error("tvg_cols: %s is null", !logits ? "logits" : !cols ? "cols" : "out"); return BLIM_ERR_ARG; }
    if (n_vocab < 1) { blim_set_error("tvg_cols: n_vocab = %d < 1", n_vocab); return BLIM_ERR_ARG; }
    if (n_rows < 1) { blim_set_error("tvg_cols: n_rows = %d < 1", n_rows); return BLIM_ERR_ARG; }
    if (n_cols < 1) { blim_set_error("tvg_cols: n_cols = %d < 1", n_cols); return BLIM_ERR_ARG; }
    if (ld < n_vocab) { blim_set_error("tvg_cols: ld = %lld below n_vocab = %d", (long long)ld, n_vocab); return BLIM_ERR_ARG; }
    if (out0 < 0) { blim_set_error("tvg_cols: out0 = %lld < 0", (long long)out0); return BLIM_ERR_ARG; }
    if (ld_out - out0 < n_rows) { blim_set_error("tvg_cols: ld_out = %lld below out0 + n_rows = %lld + %d", (long long)ld_out, (long long)out0, n_rows); return BLIM_ERR_ARG; }
    return launch_tvg_cols(logits, ld, n_vocab, n_rows, cols, n_cols, out, ld_out, out0, (hipStream_t)stream);
}
extern "C" int blim_group_mean_rows(void* out, const void* in, int64_t n_out, int32_t group, int32_t H, int32_t dtype16, int32_t split, void* stream) {
    ARG_CHECK(dtype16 == BLIM_COMPUTE_BF16 || dtype16 == BLIM_COMPUTE_F16);
    return launch_group_mean((bf16_t*)out, (const bf16_t*)in, n_out, group, H, dtype16 == BLIM_COMPUTE_F16 ? DT_F16 : DT_BF16, (hipStream_t)stream, split != 0);
}
extern "C" int blim_assemble_rows(void* out, const int32_t* src_index, int64_t n_tokens, int32_t H, const void* table, const void* feats, int32_t split, void* stream) {
    ARG_CHECK(H > 0);
    return launch_assemble((bf16_t*)out, src_index, n_tokens, H, (const bf16_t*)table, (const bf16_t*)feats, (hipStream_t)stream, split != 0);
}
// The decoder's attention as a building block (tests): fills AttnParams / AttnPcParams as decode_impl does and launches.  The argument errors are reported here
// (the launchers repeat theirs), so that the host-only build of this file sees them too.
extern "C" int blim_attention(const blim_attention_args* args, void* stream) {
    ARG_CHECK(args && args->struct_bytes >= (int64_t)offsetof(blim_attention_args, lse_out));
    blim_attention_args a;
    memset(&a, 0, sizeof a);
    memcpy(&a, args, (size_t)std::min<int64_t>(args->struct_bytes, (int64_t)sizeof a));
    const blim_batch* b = a.batch;
    ARG_CHECK(b && a.qkv && a.out);
    ARG_CHECK(b->n_tokens > 0 && b->n_seqs > 0 && b->n_blocks > 0);
    ARG_CHECK(b->key_visible && b->seq_start && b->seq_len && b->pfx_start && b->pfx_len && b->blk_seq && b->blk_q0);
    ARG_CHECK(a.dtype16 == BLIM_COMPUTE_BF16 || a.dtype16 == BLIM_COMPUTE_F16);
    ARG_CHECK(a.num_heads > 0 && a.num_kv_heads > 0 && a.num_heads % a.num_kv_heads == 0);
    if (a.num_heads / a.num_kv_heads > 8) { blim_set_error("attention: %d query heads per kv head > 8 unsupported", a.num_heads / a.num_kv_heads); return BLIM_ERR_ARG; }
    ARG_CHECK(a.ldq % 8 == 0 && a.ldo % 4 == 0 && a.v_lo_off >= 0 && a.out_lo_off >= 0 && a.v_lo_off % 8 == 0 && a.out_lo_off % 4 == 0);
    const int64_t qn = (int64_t)(a.num_heads + 2 * a.num_kv_heads) * 128, hn = (int64_t)a.num_heads * 128, cn = (int64_t)2 * a.num_kv_heads * 128;
    ARG_CHECK(a.ldq >= qn && a.ldo >= hn);
    if (a.v_lo_off && (a.v_lo_off < qn || a.v_lo_off + qn > a.ldq)) { blim_set_error("attention: the lo parts at v_lo_off overlap [q | k | v] or leave the row (ldq)"); return BLIM_ERR_ARG; }
    if (a.out_lo_off && (a.out_lo_off < hn || a.out_lo_off + hn > a.ldo)) { blim_set_error("attention: the lo output at out_lo_off overlaps the output or leaves the row (ldo)"); return BLIM_ERR_ARG; }
    if ((a.v_lo_off || a.out_lo_off) && !a.use_tr_read) { blim_set_error("attention: the compensated forms read V transposed (use_tr_read = 1)"); return BLIM_ERR_ARG; }
    if (a.out8) {
        ARG_CHECK(a.out_mx && a.dtype16 == BLIM_COMPUTE_F16 && a.ldo8 >= (int64_t)a.num_heads * 128 && a.ldo8 % 4 == 0 && a.mx_stride >= ((b->n_tokens + 255) / 256) * 256);
        if (a.v_lo_off || a.out_lo_off || a.lse_out) { blim_set_error("attention: the fused e4m3 output belongs to the plain form, without lse_out"); return BLIM_ERR_ARG; }
    }
    AttnPcParams p;
    memset(&p, 0, sizeof p);
    p.dtype = a.dtype16 == BLIM_COMPUTE_F16 ? DT_F16 : DT_BF16;
    p.qkv = (const bf16_t*)a.qkv; p.ldq = a.ldq; p.num_heads = a.num_heads; p.num_kv_heads = a.num_kv_heads;
    p.key_visible = b->key_visible; p.seq_start = b->seq_start; p.seq_len = b->seq_len; p.pfx_start = b->pfx_start; p.pfx_len = b->pfx_len;
    p.blk_seq = b->blk_seq; p.blk_q0 = b->blk_q0; p.own_start = b->own_start; p.n_blocks = b->n_blocks; p.out = (bf16_t*)a.out; p.ldo = a.ldo; p.scale = a.scale;
    p.v_lo_off = a.v_lo_off; p.out_lo_off = a.out_lo_off;
    p.out8 = (uint8_t*)a.out8; p.ldo8 = a.ldo8; p.out_mx = (uint8_t*)a.out_mx; p.mx_stride = a.mx_stride; p.lse_out = a.lse_out;
    if (!a.pfx_cache) return launch_attention(p, a.use_tr_read, (hipStream_t)stream);
    if (a.out8 || a.lse_out) { blim_set_error("attention: the prefix-cache forms write a 16-bit output and no lse"); return BLIM_ERR_ARG; }
    if (!a.use_tr_read) { blim_set_error("attention: the prefix-cache forms read V transposed (use_tr_read = 1)"); return BLIM_ERR_ARG; }
    if (a.v_lo_off != 0 && a.pc_lo_off == 0) { blim_set_error("attention: a compensated call needs a prefix cache that holds lo parts"); return BLIM_ERR_ARG; }
    ARG_CHECK(a.pfx_slot && a.pc_n_slots > 0 && a.pc_max_len > 0 && a.pc_ld % 8 == 0 && a.pc_lo_off % 8 == 0 && a.pc_slot_stride % 8 == 0 && a.pc_lo_off >= 0);
    ARG_CHECK(a.pc_ld >= cn && a.pc_slot_stride >= a.pc_max_len * a.pc_ld);
    if (a.pc_lo_off && (a.pc_lo_off < cn || a.pc_lo_off + cn > a.pc_ld)) { blim_set_error("attention: the cache's lo parts at pc_lo_off overlap [k | v] or leave the row (pc_ld)"); return BLIM_ERR_ARG; }
    p.pfx_cache = (const bf16_t*)a.pfx_cache; p.pfx_slot = a.pfx_slot; p.pc_slot_stride = a.pc_slot_stride; p.pc_ld = a.pc_ld; p.pc_lo_off = a.pc_lo_off;
    p.pc_n_slots = a.pc_n_slots; p.pc_max_len = a.pc_max_len;
    return launch_attention_cached(p, (hipStream_t)stream);
}

// The GEMM as a building block (tests): fills GemmParams from the fields the engine and the trainer set and launches.  As for blim_attention the argument errors
// are reported here (launch_gemm repeats its own), so that the host-only build of this file sees them too.
extern "C" int blim_gemm(const blim_gemm_args* args, void* stream) {
    ARG_CHECK(args && args->struct_bytes >= (int64_t)offsetof(blim_gemm_args, bias));
    blim_gemm_args a;
    memset(&a, 0, sizeof a);
    memcpy(&a, args, (size_t)std::min<int64_t>(args->struct_bytes, (int64_t)sizeof a));
    hipStream_t s = (hipStream_t)stream;
    ARG_CHECK(a.epi >= BLIM_EPI_BF16 && a.epi <= BLIM_EPI_LSE);
    ARG_CHECK(a.dtype == BLIM_COMPUTE_BF16 || a.dtype == BLIM_COMPUTE_F16 || a.dtype == BLIM_COMPUTE_F8);
    ARG_CHECK(a.A && a.W && a.M > 0 && a.N > 0 && a.K > 0 && a.lda > 0);
    const bool f8 = a.dtype == BLIM_COMPUTE_F8;
    const int64_t es = f8 ? 1 : 2;
    // tile: 0 = the 256 x 256 kernel, 1 = auto (an ineligible form silently keeps the 256 x 256 kernel), 2 = the narrow kernel -- refused, with the field named, for
    // every form the narrow kernel is not instantiated for
    if (a.tile < 0 || a.tile > 2) { blim_set_error("gemm: tile = %d (0 = 256 x 256, 1 = auto, 2 = narrow)", (int)a.tile); return BLIM_ERR_ARG; }
    if (a.tile == 2) {
        if (a.epi != BLIM_EPI_RESID) { blim_set_error("gemm: tile = 2 (the narrow kernel) has the residual epilogue only (epi = %d)", (int)a.epi); return BLIM_ERR_ARG; }
        if (f8) { blim_set_error("gemm: tile = 2 (the narrow kernel) takes fp16 / bf16 operands (dtype = f8)"); return BLIM_ERR_ARG; }
        if (a.A6 || a.W6) { blim_set_error("gemm: tile = 2 (the narrow kernel) has no e2m3 second pass (A6 / W6)"); return BLIM_ERR_ARG; }
        if (a.a_mx) { blim_set_error("gemm: tile = 2 (the narrow kernel) takes no block-scaled A operand (a_mx)"); return BLIM_ERR_ARG; }
    }
    // tile_lo6: the same three values for the form `tile` refuses, the residual epilogue with the e2m3 second pass (A6 / W6); 2 is refused, with the field named, for every other form
    if (a.tile_lo6 < 0 || a.tile_lo6 > 2) { blim_set_error("gemm: tile_lo6 = %d (0 = 256 x 256, 1 = auto, 2 = narrow)", (int)a.tile_lo6); return BLIM_ERR_ARG; }
    if (a.tile_lo6 == 2) {
        if (a.epi != BLIM_EPI_RESID) { blim_set_error("gemm: tile_lo6 = 2 (the narrow e2m3 kernel) has the residual epilogue only (epi = %d)", (int)a.epi); return BLIM_ERR_ARG; }
        if (f8) { blim_set_error("gemm: tile_lo6 = 2 (the narrow e2m3 kernel) takes fp16 / bf16 operands (dtype = f8)"); return BLIM_ERR_ARG; }
        if (!a.A6 || !a.W6) { blim_set_error("gemm: tile_lo6 = 2 (the narrow e2m3 kernel) needs the e2m3 second pass (A6 / W6)"); return BLIM_ERR_ARG; }
        if (a.w_wrap_k) { blim_set_error("gemm: tile_lo6 = 2 (the narrow e2m3 kernel) takes no wrapped W (w_wrap_k = %d): that form is `tile`'s", (int)a.w_wrap_k); return BLIM_ERR_ARG; }
    }
    // tile_qkv: the same three values for BLIM_EPI_QKV on fp16 / bf16 operands (plain or hi | lo outputs, the w_wrap_k walk, the e2m3 second pass behind hi | lo outputs);
    // 2 is refused, with the field named, for every other form
    if (a.tile_qkv < 0 || a.tile_qkv > 2) { blim_set_error("gemm: tile_qkv = %d (0 = 256 x 256, 1 = auto, 2 = narrow)", (int)a.tile_qkv); return BLIM_ERR_ARG; }
    if (a.tile_qkv == 2) {
        if (a.epi != BLIM_EPI_QKV) { blim_set_error("gemm: tile_qkv = 2 (the narrow QKV kernel) has the QKV epilogue only (epi = %d)", (int)a.epi); return BLIM_ERR_ARG; }
        if (f8) { blim_set_error("gemm: tile_qkv = 2 (the narrow QKV kernel) takes fp16 / bf16 operands (dtype = f8)"); return BLIM_ERR_ARG; }
        if (a.A6 && a.lo_off == 0) { blim_set_error("gemm: tile_qkv = 2 (the narrow QKV kernel) has the e2m3 second pass (A6) behind hi | lo outputs only (lo_off = 0)"); return BLIM_ERR_ARG; }
    }
    ARG_CHECK(a.K * es % 128 == 0 && a.lda * es % 16 == 0);
    ARG_CHECK(a.w_wrap_k == 0 || (a.K == 2 * a.w_wrap_k && a.w_wrap_k * es % 128 == 0));
    ARG_CHECK(a.lda >= a.K);
    const bool out16 = a.epi == BLIM_EPI_BF16 || a.epi == BLIM_EPI_QKV || a.epi == BLIM_EPI_SWIGLU;
    const int64_t n_out = a.epi == BLIM_EPI_SWIGLU ? a.N / 2 : a.N;
    const bool fused8 = a.out8 != nullptr;
    if (fused8) {
        if (!(a.epi == BLIM_EPI_SWIGLU && f8)) { blim_set_error("gemm: the fused e4m3 output (out8) belongs to the fp8 SwiGLU GEMM"); return BLIM_ERR_ARG; }
        ARG_CHECK(a.out_mx && a.N % 256 == 0 && a.ldc % 16 == 0 && a.ldc >= n_out && a.lo_off == 0);
    } else {
        ARG_CHECK(!a.out_mx);
        if (a.epi == BLIM_EPI_LSE) ARG_CHECK(a.labels && a.lse_part && a.label_logit);
        else ARG_CHECK(a.C && a.ldc >= n_out);
    }
    if (a.epi != BLIM_EPI_F32 && a.epi != BLIM_EPI_LSE && !fused8) ARG_CHECK(a.ldc % 4 == 0);
    ARG_CHECK(!f8 || ((a.row_scale || a.a_mx) && a.col_scale));
    ARG_CHECK((!a.a_mx && !a.out_mx) || (f8 && a.mx_stride >= (int64_t)((a.M + 255) / 256) * 256));
    ARG_CHECK(!a.a_mx || a.epi == BLIM_EPI_RESID);
    ARG_CHECK(a.act == 0 || (a.act == 1 && a.epi == BLIM_EPI_BF16));
    ARG_CHECK(!a.bias || a.epi == BLIM_EPI_BF16 || a.epi == BLIM_EPI_RESID || a.epi == BLIM_EPI_QKV);
    ARG_CHECK(!a.resid_in || a.epi == BLIM_EPI_RESID);
    if (a.lo_off) {
        if (!out16 || f8) { blim_set_error("gemm: split (hi | lo) outputs belong to the 16-bit epilogues of a 16-bit dtype"); return BLIM_ERR_ARG; }
        if (a.lo_off < n_out || a.lo_off + n_out > a.ldc) { blim_set_error("gemm: the lo half at lo_off overlaps the output or leaves the row (ldc)"); return BLIM_ERR_ARG; }
        ARG_CHECK(a.lo_off % 4 == 0 && !a.swiglu_act && !a.swiglu_gu);
    }
    if (a.epi == BLIM_EPI_QKV) {
        ARG_CHECK(a.bias && a.rope_rows && a.rope_stride >= a.M && a.N % 128 == 0 && a.rope_cols >= 0 && a.rope_cols % 128 == 0);
        if (a.rope_cols > a.N) { blim_set_error("gemm: rope_cols %d > N %d", a.rope_cols, a.N); return BLIM_ERR_ARG; }
    } else ARG_CHECK(a.rope_cols == 0 && !a.rope_rows);
    if (a.epi == BLIM_EPI_SWIGLU) ARG_CHECK(a.N % 32 == 0);
    if (a.swiglu_act || a.swiglu_gu) {
        if (a.epi != BLIM_EPI_BF16 || f8) { blim_set_error("gemm: the trainer's fused SwiGLU forms belong to the plain 16-bit epilogue"); return BLIM_ERR_ARG; }
        ARG_CHECK(!(a.swiglu_act && a.swiglu_gu));
        ARG_CHECK(!a.swiglu_gu || (a.N % 16 == 0 && a.swiglu_ld % 8 == 0 && a.swiglu_ld >= 2 * (int64_t)a.N));
        ARG_CHECK(!a.swiglu_act || (a.N % 32 == 0 && a.swiglu_act_ld % 8 == 0 && a.swiglu_act_ld >= a.N / 2));
    }
    if (a.A6 || a.W6 || a.f6_build || a.out6) {
        if (f8 || !a.A6 || !a.W6) { blim_set_error("gemm: the e2m3 second pass needs a 16-bit dtype and both A6 and W6"); return BLIM_ERR_ARG; }
        ARG_CHECK(a.w_wrap_k == 0 && (a.epi == BLIM_EPI_RESID || a.epi == BLIM_EPI_QKV || a.epi == BLIM_EPI_SWIGLU || a.epi == BLIM_EPI_LSE));
        if (a.epi == BLIM_EPI_QKV && a.lo_off == 0) { blim_set_error("gemm: lo6 QKV GEMM: hi | lo outputs only"); return BLIM_ERR_ARG; }
        if (a.f6_build) {
            ARG_CHECK(a.K % 128 == 0 && (a.K6 == 0 || a.K6 == a.K) && a.lda >= 2 * (int64_t)a.K);
            a.K6 = a.K;
            TRY(launch_f6_tiles((const bf16_t*)a.W, a.K, a.N, a.K, a.dtype, true, (uint8_t*)a.W6, s));
            TRY(launch_f6_tiles((const bf16_t*)a.A + a.K, a.lda, a.M, a.K, a.dtype, false, (uint8_t*)a.A6, s));
        }
        ARG_CHECK(a.K6 > 0 && a.K6 % 128 == 0);
        ARG_CHECK(!a.out6 || (a.epi == BLIM_EPI_SWIGLU && a.lo_off > 0 && a.N % 256 == 0));
    }
    GemmParams p = gp(a.dtype, a.A, a.lda, a.W, a.M, a.N, a.K, fused8 ? a.out8 : a.C, a.ldc);
    p.narrow = a.tile; p.narrow_lo6 = a.tile_lo6; p.narrow_qkv = a.tile_qkv;
    p.row_scale = a.row_scale; p.col_scale = a.col_scale; p.bias = a.bias; p.resid_in = a.resid_in; p.act = a.act; p.scale = a.scale;
    p.swiglu_gu = (uint16_t*)a.swiglu_gu; p.swiglu_ld = a.swiglu_ld; p.swiglu_act = (uint16_t*)a.swiglu_act; p.swiglu_act_ld = a.swiglu_act_ld;
    p.rope_cols = a.rope_cols; p.rope_rows = a.rope_rows; p.rope_stride = a.rope_stride;
    p.labels = a.labels; p.lse_part = (float2*)a.lse_part; p.label_logit = a.label_logit;
    p.w_wrap_k = a.w_wrap_k; p.lo_off = a.lo_off; p.f16_saturate = a.f16_saturate;
    p.out_mx = (uint8_t*)a.out_mx; p.a_mx = (const uint8_t*)a.a_mx; p.mx_stride = a.mx_stride;
    p.A6 = (const uint8_t*)a.A6; p.W6 = (const uint8_t*)a.W6; p.K6 = a.K6; p.out6 = (uint8_t*)a.out6;
    return launch_gemm((GemmEpi)a.epi, p, s);
}
// blim_rope_rows: the engine's two RoPE kernels into caller-owned memory -- rope_table_kernel fills the workspace (cos | sin of every position, as at creation),
// rope_rows_kernel gathers the rows of `positions` (clamped to [0, max_positions)) into the chunk-major table of gemm.hpp
extern "C" int64_t blim_rope_rows_bytes(int32_t max_positions) { return max_positions > 0 ? (int64_t)max_positions * 64 * 2 * 4 : -1; }
extern "C" int blim_rope_rows(const int32_t* positions, int64_t n_tokens, float rope_theta, int32_t max_positions, void* workspace, float* out, int64_t stride, void* stream) {
    ARG_CHECK(positions && workspace && out && n_tokens > 0 && max_positions > 0 && rope_theta > 0.f);
    if (stride < n_tokens) { blim_set_error("rope_rows: stride %lld < n_tokens %lld (the chunks would overlap)", (long long)stride, (long long)n_tokens); return BLIM_ERR_ARG; }
    ARG_CHECK(n_tokens * 32 < (1ll << 31) * 256 && (int64_t)max_positions * 64 < (1ll << 31));
    hipStream_t s = (hipStream_t)stream;
    float* cosb = (float*)workspace;
    float* sinb = cosb + (int64_t)max_positions * 64;
    const int n = max_positions * 64;
    hipLaunchKernelGGL(rope_table_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cosb, sinb, max_positions, 64, rope_theta, 128);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rope_rows_kernel, dim3((unsigned)((n_tokens * 32 + 255) / 256)), dim3(256), 0, s, out, positions, cosb, sinb, n_tokens, stride, max_positions);
    HIP_TRY(hipGetLastError());
    return BLIM_OK;
}

// ---------------------------------------------------------------------------- timing / options
extern "C" int blim_timing_enable(blim_engine* e, int32_t on) {
    ARG_CHECK(e);
    e->timing = on != 0;
    return BLIM_OK;
}
extern "C" int blim_timing_num_classes(void) { return TC_COUNT; }
extern "C" const char* blim_timing_class_name(int32_t cls) { return (cls >= 0 && cls < TC_COUNT) ? kTimeClassNames[cls] : ""; }
extern "C" int blim_timing_report(blim_engine* e, double* ms, int64_t* calls, double* flops) {
    ARG_CHECK(e && ms && calls && flops);
    for (int i = 0; i < TC_COUNT; ++i) { ms[i] = 0; calls[i] = 0; flops[i] = 0; }
    for (auto& s : e->spans) {
        HIP_TRY(hipEventSynchronize(s.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, s.a, s.b));
        ms[s.cls] += t; calls[s.cls] += 1; flops[s.cls] += s.flops;
        hipEventDestroy(s.a); hipEventDestroy(s.b);
    }
    e->spans.clear();
    return BLIM_OK;
}
extern "C" int blim_debug_read(blim_engine* e, const char* which, void* dst, int64_t bytes, void* stream) {
    ARG_CHECK(e && which && dst && bytes > 0);
    const DevBuf* b = nullptr;
    if (!strcmp(which, "resid")) b = &e->resid;
    else if (!strcmp(which, "xn")) b = &e->xn;
    else if (!strcmp(which, "qkv")) b = &e->qkv;
    else if (!strcmp(which, "attn")) b = &e->attn;
    else if (!strcmp(which, "act")) b = &e->act;
    else if (!strcmp(which, "act8")) b = &e->act8;
    else if (!strcmp(which, "act_mx")) b = &e->act_mx;
    if (!b || !b->p || (size_t)bytes > b->bytes) { blim_set_error("debug_read: no buffer '%s' of %lld bytes", which, (long long)bytes); return BLIM_ERR_ARG; }
    HIP_TRY(hipMemcpyAsync(dst, b->p, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BLIM_OK;
}
extern "C" int blim_debug_gemm_stamps(void* device_buf) {
    gemm_set_debug_stamps((unsigned long long*)device_buf);
    return BLIM_OK;
}
extern "C" int blim_set_option(blim_engine* e, const char* key, int32_t value) {
    ARG_CHECK(e && key);
    if (!strcmp(key, "attn_tr_read")) { e->attn_tr = value; return BLIM_OK; }
    if (!strcmp(key, "f8_mask")) { e->f8_mask = value & 31; return BLIM_OK; }
    if (!strcmp(key, "f8_fuse")) { e->f8_fuse = value != 0; return BLIM_OK; }
    if (!strcmp(key, "precise_embeds")) { e->precise_embeds = value != 0; return BLIM_OK; }
    if (!strcmp(key, "prune_last")) { e->prune_last = value != 0; return BLIM_OK; }
    if (!strcmp(key, "masked_query_zero")) {
        if (value && e->f8) { blim_set_error("option 'masked_query_zero' needs a 16-bit engine (the fp8 mode's attention output leaves the kernel quantised)"); return BLIM_ERR_ARG; }
        e->masked_query_zero = value != 0; return BLIM_OK;
    }
    if (!strcmp(key, "precise_lo6")) {
        if (value && e->f8) { blim_set_error("option 'precise_lo6' needs a 16-bit engine (fp16: the default; bf16: opt-in)"); return BLIM_ERR_ARG; }
        if (value && !lo6_sizes_ok(e->c)) {
            blim_set_error("option 'precise_lo6': hidden and intermediate sizes must be multiples of 128, at most 20480"); return BLIM_ERR_ARG; }
        if (value && e->aug && e->aug % 128) { blim_set_error("option 'precise_lo6': adapters were loaded with a %d-column K extension; set the option before loading adapters", e->aug); return BLIM_ERR_STATE; }
        e->lo6 = value != 0; return BLIM_OK;
    }
    if (!strcmp(key, "narrow_lo6")) {
        if (value < 0 || value > 2) { blim_set_error("option 'narrow_lo6': 0 (off), 1 (auto) or 2 (wherever eligible), got %d", (int)value); return BLIM_ERR_ARG; }
        e->narrow_lo6 = value; return BLIM_OK;
    }
    if (!strcmp(key, "narrow_qkv")) {
        if (value < 0 || value > 2) { blim_set_error("option 'narrow_qkv': 0 (off), 1 (auto) or 2 (wherever eligible), got %d", (int)value); return BLIM_ERR_ARG; }
        e->narrow_qkv = value; return BLIM_OK;
    }
    if (!strcmp(key, "narrow_gemm")) {
        if (value < 0 || value > 2) { blim_set_error("option 'narrow_gemm': 0 (off), 1 (auto) or 2 (wherever eligible), got %d", (int)value); return BLIM_ERR_ARG; }
        e->narrow_gemm = value; return BLIM_OK;
    }
    if (!strcmp(key, "precise_mlp")) { e->precise_mlp = value != 0; return BLIM_OK; }
    if (!strcmp(key, "precise_layers")) {
        if (value && e->f8) { blim_set_error("option 'precise_layers' needs a 16-bit engine (fp16 or bf16)"); return BLIM_ERR_ARG; }
        e->layer_mask_on = value != 0; return BLIM_OK;
    }
    if (!strcmp(key, "precise_layer_bits")) {
        if (e->f8) { blim_set_error("option 'precise_layer_bits' needs a 16-bit engine (fp16 or bf16)"); return BLIM_ERR_ARG; }
        const int32_t layer = value >> 4;
        if (value < 0 || layer >= e->c.num_layers) {
            blim_set_error("option 'precise_layer_bits': value = (layer << 4) | bits with 0 <= layer < %d (got %d)", e->c.num_layers, (int)value); return BLIM_ERR_ARG; }
        e->layer_bits[layer] = (uint8_t)(value & 15); return BLIM_OK;
    }
    if (!strcmp(key, "precise")) {
        if (value && e->f8) { blim_set_error("option 'precise' needs a 16-bit engine (fp16 or bf16)"); return BLIM_ERR_ARG; }
        e->precise = value != 0;
        return BLIM_OK;
    }
    blim_set_error("unknown option '%s'", key);
    return BLIM_ERR_ARG;
}
