// TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): drives the HOST side of the C ABI -- csrc/engine.hip, adapters.hip, train.hip compiled as plain C++ against the
// mock HIP runtime of this directory -- under AddressSanitizer + UBSan.  Kernels do nothing here; what runs is the bookkeeping: create / destroy, weight and adapter
// tables (every name, partial sets, reloads), the lazily built derived copies (augmented weights, the combined 16-bit | e2m3 copies, fp8 copies), workspace growth,
// every option key, the scoring / decode / forward entry points' host logic in every numeric mode, the trainer's life cycle, and the error paths (bad arguments,
// wrong state, out of device memory).  Exit code 0 = every expectation met; the sanitizers abort on their own findings.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/blim.h"

extern "C" size_t mock_hip_mem_limit, mock_hip_mem_in_use;
extern "C" int mock_hip_device_count;
extern "C" size_t mock_hip_live_allocations();

static int failures = 0;
#define EXPECT(cond)                                                                              \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "EXPECT failed: %s (%s:%d) last error: %s\n", #cond, __FILE__, __LINE__, blim_last_error()); ++failures; } \
    } while (0)

static blim_config cfg_of(int dtype, int H = 256, int I = 512, int layers = 2) {
    blim_config c;
    memset(&c, 0, sizeof c);
    c.vocab_size = 1024; c.hidden_size = H; c.intermediate_size = I; c.num_layers = layers; c.num_heads = 2; c.num_kv_heads = 1;
    c.mm_hidden_size = 64; c.num_clips = 4; c.max_positions = 128; c.compute_dtype = dtype; c.rms_eps = 1e-6f; c.rope_theta = 1e6f;
    return c;
}
static std::vector<std::string> weight_names(int layers) {
    std::vector<std::string> n = {"embed_tokens", "final_norm", "lm_head", "visual_head"};
    for (const char* p : {"mlp", "tvg_mlp"}) for (const char* t : {"0.w", "0.b", "2.w", "2.b"}) n.push_back(std::string(p) + "." + t);
    for (int i = 0; i < layers; ++i)
        for (const char* t : {"input_norm", "post_norm", "q_proj.w", "k_proj.w", "v_proj.w", "q_proj.b", "k_proj.b", "v_proj.b", "o_proj.w", "gate_proj.w", "up_proj.w", "down_proj.w"})
            n.push_back("layers." + std::to_string(i) + "." + t);
    return n;
}

struct Batch {
    std::vector<int32_t> pos, seq_start, seq_len, pfx_start, pfx_len, blk_seq, blk_q0, own;
    std::vector<uint8_t> vis;
    blim_batch b;
    Batch(int n_seq, int len, bool with_own) {
        for (int s = 0; s < n_seq; ++s) {
            seq_start.push_back(s * len); seq_len.push_back(len); pfx_start.push_back(0); pfx_len.push_back(s ? len : 0);
            for (int q = 0; q < len; q += 32) { blk_seq.push_back(s); blk_q0.push_back(q); }
            for (int i = 0; i < len; ++i) { pos.push_back(i); vis.push_back(1); own.push_back(0); }
        }
        b.n_tokens = n_seq * len; b.n_seqs = n_seq; b.n_blocks = (int32_t)blk_seq.size();
        b.positions = pos.data(); b.key_visible = vis.data(); b.seq_start = seq_start.data(); b.seq_len = seq_len.data(); b.pfx_start = pfx_start.data(); b.pfx_len = pfx_len.data();
        b.blk_seq = blk_seq.data(); b.blk_q0 = blk_q0.data(); b.own_start = with_own ? own.data() : nullptr;
    }
};

static void load_all(blim_engine* e, const blim_config& c, int dtype_code) {
    std::vector<float> big((size_t)c.vocab_size * c.hidden_size, 0.01f);
    for (const std::string& n : weight_names(c.num_layers)) EXPECT(blim_load_weight(e, n.c_str(), big.data(), dtype_code, 0) == 0);
}

// every scoring-side entry point once, on host buffers standing in for device buffers
static void score_calls(blim_engine* e, const blim_config& c, int n_seq, int len, bool with_own) {
    Batch B(n_seq, len, with_own);
    const int64_t T = B.b.n_tokens;
    const int H = c.hidden_size, wide = 2;
    std::vector<uint16_t> embeds((size_t)T * H * wide, 0), hid((size_t)T * H * wide, 0), feats((size_t)64 * 64 * wide, 0), proj((size_t)64 * H * wide, 0);
    std::vector<float> f32((size_t)T * std::max(H, c.vocab_size), 0.f), scores(64, 0.f), logits((size_t)T * c.vocab_size, 0.f);
    std::vector<int32_t> rows, labels, row_start = {0}, src((size_t)T, 1), vlab(16, 0);
    for (int s = 0; s < n_seq; ++s) { for (int i = 0; i < 4; ++i) { rows.push_back(s * len + len - 5 + i); labels.push_back(7); } row_start.push_back((int32_t)rows.size()); }
    EXPECT(blim_project_video(e, feats.data(), 64, 0, proj.data(), nullptr) == 0);
    EXPECT(blim_project_video(e, feats.data(), 64, 1, proj.data(), nullptr) == 0);
    EXPECT(blim_project_video(e, feats.data(), 64, 2, proj.data(), nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_group_mean(e, proj.data(), 4, 16, hid.data(), nullptr) == 0);
    EXPECT(blim_assemble(e, src.data(), T, proj.data(), embeds.data(), nullptr) == 0);
    EXPECT(blim_decode(e, &B.b, embeds.data(), nullptr, 0, hid.data(), f32.data(), nullptr) == 0);
    EXPECT(blim_decode(e, &B.b, embeds.data(), rows.data(), (int64_t)rows.size(), hid.data(), nullptr, nullptr) == 0);
    EXPECT(blim_score_vtg(e, &B.b, embeds.data(), rows.data(), labels.data(), (int64_t)rows.size(), row_start.data(), n_seq, scores.data(), nullptr) == 0);
    std::vector<float> vocab_f32((size_t)16 * c.num_clips * c.mm_hidden_size, 0.f);
    std::vector<uint16_t> vocab16((size_t)16 * c.num_clips * c.mm_hidden_size, 0);
    EXPECT(blim_set_video_vocab(e, vocab_f32.data(), 16, nullptr) == 0 || c.compute_dtype == BLIM_COMPUTE_F8);
    std::vector<int32_t> trows;
    for (int s = 0; s < n_seq; ++s) for (int i = 0; i < c.num_clips; ++i) trows.push_back(s * len + len - 6 + i);
    EXPECT(blim_score_tvg(e, &B.b, embeds.data(), trows.data(), vocab16.data(), 16, vlab.data(), n_seq, scores.data(), nullptr) == 0);
    std::vector<uint8_t> mask((size_t)2 * 40, 1);
    std::vector<float> hidden_f32((size_t)2 * 40 * H, 0.f), lg((size_t)2 * 40 * c.vocab_size, 0.f);
    EXPECT(blim_forward(e, embeds.data(), mask.data(), 2, 40, lg.data(), hidden_f32.data(), nullptr) == 0);
    EXPECT(blim_vtg_logprobs(e, hid.data(), labels.data(), (int64_t)labels.size(), f32.data(), nullptr) == 0);
    EXPECT(blim_lm_head(e, hid.data(), 8, logits.data(), nullptr) == 0);
    EXPECT(blim_visual_head(e, hid.data(), 8, proj.data(), nullptr) == 0);
    EXPECT(blim_segment_mean(e, f32.data(), row_start.data(), n_seq, 0, scores.data(), nullptr) == 0);
}

// the engine-less attention entry: one good call of every form, then the argument errors it reports itself
static void attention_calls() {
    Batch B(3, 40, true);
    const int64_t T = B.b.n_tokens;
    const int nh = 4, nkv = 2, qn = (nh + 2 * nkv) * 128, hn = nh * 128;
    std::vector<uint16_t> qkv((size_t)T * 2 * qn, 0), out((size_t)T * 2 * hn, 0), cache((size_t)2 * 64 * 4 * nkv * 128, 0);
    std::vector<uint8_t> out8((size_t)T * hn, 0), mx((size_t)nh * 256, 0);
    std::vector<float> lse((size_t)T * nh, 0.f);
    std::vector<int32_t> slot = {-1, 0, 5};
    blim_attention_args a;
    memset(&a, 0, sizeof a);
    a.struct_bytes = sizeof a; a.batch = &B.b; a.qkv = qkv.data(); a.ldq = qn; a.num_heads = nh; a.num_kv_heads = nkv; a.dtype16 = BLIM_COMPUTE_F16; a.use_tr_read = 1;
    a.out = out.data(); a.ldo = hn; a.scale = 0.0883883f;
    const blim_attention_args plain = a;
    EXPECT(blim_attention(&a, nullptr) == 0);
    a.use_tr_read = 0; a.dtype16 = BLIM_COMPUTE_BF16; a.lse_out = lse.data();
    EXPECT(blim_attention(&a, nullptr) == 0);
    a = plain; a.out8 = out8.data(); a.ldo8 = hn; a.out_mx = mx.data(); a.mx_stride = 256;
    EXPECT(blim_attention(&a, nullptr) == 0);
    a = plain; a.ldq = 2 * qn; a.v_lo_off = qn; a.ldo = 2 * hn; a.out_lo_off = hn;
    EXPECT(blim_attention(&a, nullptr) == 0);
    const blim_attention_args comp = a;
    a.pfx_cache = cache.data(); a.pfx_slot = slot.data(); a.pc_slot_stride = 64 * 4 * nkv * 128; a.pc_ld = 4 * nkv * 128; a.pc_lo_off = 2 * nkv * 128; a.pc_n_slots = 2; a.pc_max_len = 64;
    EXPECT(blim_attention(&a, nullptr) == 0);
    const blim_attention_args cached = a;
    a.struct_bytes = (int64_t)((const char*)&a.pfx_cache - (const char*)&a);                      // a caller compiled before the cache fields: the uncached launch
    EXPECT(blim_attention(&a, nullptr) == 0);
    // ---- refusals
    EXPECT(blim_attention(nullptr, nullptr) == BLIM_ERR_ARG);
    a = plain; a.struct_bytes = 8;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.batch = nullptr;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.qkv = nullptr;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.out = nullptr;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    { blim_batch bad = B.b; bad.seq_len = nullptr; a = plain; a.batch = &bad; EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG); }
    a = plain; a.num_heads = 9; a.num_kv_heads = 1; a.ldq = 11 * 128; a.ldo = 9 * 128;                // G > 8
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "> 8"));
    a = plain; a.num_heads = 3;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.dtype16 = BLIM_COMPUTE_F8;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.ldq = qn - 8;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = comp; a.use_tr_read = 0;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.out8 = out8.data(); a.ldo8 = hn; a.mx_stride = 256;                                  // out8 without its scale table
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = cached; a.v_lo_off = 0; a.out_lo_off = 0; a.out8 = out8.data(); a.ldo8 = hn; a.out_mx = mx.data(); a.mx_stride = 256;      // out8 together with a cache
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "prefix-cache"));
    a = cached; a.lse_out = lse.data();
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = cached; a.pc_lo_off = 0;                                                                      // a compensated call, a cache without lo parts
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "lo parts"));
    a = comp; a.v_lo_off = qn - 8;                                                                    // lo parts that overlap [q | k | v] ...
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "v_lo_off"));
    a = comp; a.v_lo_off = qn + 8;                                                                    // ... or leave the row
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "v_lo_off"));
    a = comp; a.out_lo_off = hn - 4;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "out_lo_off"));
    a = comp; a.out_lo_off = hn + 4;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "out_lo_off"));
    a = cached; a.pc_lo_off = 2 * nkv * 128 - 8;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "pc_lo_off"));
    a = cached; a.pc_lo_off = 2 * nkv * 128 + 8;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "pc_lo_off"));
    a = cached; a.pc_ld = 2 * nkv * 128 - 8; a.v_lo_off = 0; a.pc_lo_off = 0;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = cached; a.pc_slot_stride = 63 * a.pc_ld;                                                      // slots that overlap
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = cached; a.pfx_slot = nullptr;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
    a = cached; a.pc_n_slots = 0;
    EXPECT(blim_attention(&a, nullptr) == BLIM_ERR_ARG);
}

// the engine-less attention backward and RoPE backward: the good call, then every refusal of both entries
static void attention_bwd_calls() {
    const int T = 150, nh = 4, nkv = 2, qn = (nh + 2 * nkv) * 128, hn = nh * 128, n_seqs = 2, max_len = 70;
    std::vector<uint16_t> qkv((size_t)T * (qn + 8), 0), dout((size_t)T * (hn + 8), 0), o16((size_t)T * (hn + 2), 0), out16((size_t)T * qn, 0);
    std::vector<float> lse((size_t)T * nh, 0.f), dqkv((size_t)T * (qn + 8), 0.f), cs((size_t)32 * 64, 1.f), sn((size_t)32 * 64, 0.f);
    std::vector<uint8_t> vis(T, 1);
    std::vector<int32_t> start = {3, 80}, len = {70, 33}, pos(T, 5);
    const int64_t need = blim_attention_bwd_workspace_bytes(T, n_seqs, nh, max_len);
    EXPECT(need == (int64_t)T * nh * 4 + 2 * ((int64_t)n_seqs * nh * 128 * 128 * 2) && blim_attention_bwd_workspace_bytes(271, 3, 7, 193) % 16 == 0);
    EXPECT(blim_attention_bwd_workspace_bytes(271, 3, 7, 193) == 7600 + 2 * ((int64_t)3 * 7 * 256 * 256 * 2));              // D of 7588 bytes rounded up to 16
    EXPECT(blim_attention_bwd_workspace_bytes(T, 16384, nh, max_len) == -1 && blim_attention_bwd_workspace_bytes(T, 1 << 30, 1 << 30, 1 << 20) == -1);
    EXPECT(blim_attention_bwd_workspace_bytes(0, n_seqs, nh, max_len) == -1 && blim_attention_bwd_workspace_bytes(T, 0, nh, max_len) == -1);
    EXPECT(blim_attention_bwd_workspace_bytes(T, n_seqs, 0, max_len) == -1 && blim_attention_bwd_workspace_bytes(T, n_seqs, nh, 0) == -1);
    std::vector<uint8_t> ws_mem((size_t)need + 16, 0xFF);
    uint8_t* const ws = ws_mem.data() + (16 - ((uintptr_t)ws_mem.data() & 15)) % 16;
    blim_attention_bwd_args a;
    memset(&a, 0, sizeof a);
    a.struct_bytes = sizeof a; a.qkv = qkv.data(); a.ldq = qn + 8; a.dout = dout.data(); a.ldo = hn + 8; a.o16 = o16.data(); a.ldo16 = hn + 2; a.lse = lse.data();
    a.num_heads = nh; a.num_kv_heads = nkv; a.dtype16 = BLIM_COMPUTE_F16; a.key_visible = vis.data(); a.seq_start = start.data(); a.seq_len = len.data();
    a.n_seqs = n_seqs; a.max_len = max_len; a.scale = 0.0883883f; a.workspace = ws; a.workspace_bytes = need; a.dqkv = dqkv.data(); a.n_tokens = T;
    const blim_attention_bwd_args good = a;
    EXPECT(blim_attention_bwd(&a, nullptr) == 0);
    a.dtype16 = BLIM_COMPUTE_BF16;
    EXPECT(blim_attention_bwd(&a, nullptr) == 0);
    // ---- refusals
    EXPECT(blim_attention_bwd(nullptr, nullptr) == BLIM_ERR_ARG);
    a = good; a.struct_bytes = 8;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.qkv = nullptr;          EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.dout = nullptr;         EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.o16 = nullptr;          EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.lse = nullptr;          EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.key_visible = nullptr;  EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.seq_start = nullptr;    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.seq_len = nullptr;      EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.workspace = nullptr;    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.dqkv = nullptr;         EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.dtype16 = BLIM_COMPUTE_F8;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.num_heads = 3;                                                                        // num_heads % num_kv_heads
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.num_kv_heads = 0;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.ldq = qn + 4;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.ldo = hn + 4;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.ldo16 = hn + 1;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.ldq = qn - 8;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    a = good; a.ldo = hn - 8;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    a = good; a.ldo16 = hn - 2;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    a = good; a.max_len = 0;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.n_seqs = 0;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.n_tokens = 0;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.n_seqs = 16384;                                                                       // 16384 x 4 heads > 65535: the grid's z range
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "z range"));
    a = good; a.workspace = ws + 4; a.workspace_bytes = need - 4;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "aligned"));
    a = good; a.workspace_bytes = need - 2;
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    a = good; a.max_len = 129;                                                                        // Lm 128 -> 192: the same workspace is too small now
    EXPECT(blim_attention_bwd(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    // ---- blim_rope_bwd
    const int rc = (nh + nkv) * 128;
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, rc, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == 0);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, 0, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_BF16, nullptr) == 0);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, qn, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_BF16, nullptr) == 0);
    EXPECT(blim_rope_bwd(nullptr, dqkv.data(), T, qn, rc, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), nullptr, T, qn, rc, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, rc, nullptr, cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, rc, pos.data(), nullptr, sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, rc, pos.data(), cs.data(), nullptr, 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), 0, qn, rc, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, rc, pos.data(), cs.data(), sn.data(), 0, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, rc, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F8, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn + 64, rc, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, rc + 64, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_bwd(out16.data(), dqkv.data(), T, qn, qn + 128, pos.data(), cs.data(), sn.data(), 32, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "rope_cols"));
}

// the engine-less GEMM entry and blim_rope_rows: one good call of every form, then the argument errors they report themselves
static void gemm_calls() {
    const int M = 300, N = 512, K = 128;
    std::vector<uint16_t> A((size_t)M * 2 * K, 0), W((size_t)N * K, 0), C16((size_t)M * 2 * (N + 8), 0), gu((size_t)M * (2 * N + 8), 0), act((size_t)M * N, 0);
    std::vector<float> C32((size_t)M * (N + 4), 0.f), bias(N, 0.f), rope((size_t)128 * 512, 0.f), part((size_t)M * 2 * 2, 0.f), ll(M, 0.f), rs(M, 1.f), cs(N, 1.f);
    std::vector<int32_t> labels(M, 3), pos(M, 5);
    std::vector<uint8_t> a6((size_t)blim_f6_tiles_bytes(M, K), 0), w6((size_t)blim_f6_tiles_bytes(N, K), 0), o6((size_t)blim_f6_tiles_bytes(M, N / 2), 0);
    std::vector<uint8_t> c8((size_t)M * N, 0), mx((size_t)8 * 512, 0), ws((size_t)blim_rope_rows_bytes(64), 0);
    EXPECT(blim_rope_rows_bytes(0) == -1 && blim_rope_rows_bytes(64) == 64 * 64 * 2 * 4);
    EXPECT(blim_rope_rows(pos.data(), M, 1e6f, 64, ws.data(), rope.data(), 512, nullptr) == 0);
    EXPECT(blim_rope_rows(pos.data(), M, 1e6f, 64, ws.data(), rope.data(), M - 1, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "stride"));
    EXPECT(blim_rope_rows(nullptr, M, 1e6f, 64, ws.data(), rope.data(), 512, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rope_rows(pos.data(), M, 1e6f, 0, ws.data(), rope.data(), 512, nullptr) == BLIM_ERR_ARG);
    blim_gemm_args a;
    memset(&a, 0, sizeof a);
    a.struct_bytes = sizeof a; a.epi = BLIM_EPI_BF16; a.dtype = BLIM_COMPUTE_F16; a.A = A.data(); a.lda = K; a.W = W.data(); a.M = M; a.N = N; a.K = K;
    a.C = C16.data(); a.ldc = N + 8; a.scale = 1.f; a.f16_saturate = 1;
    const blim_gemm_args plain = a;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    a.bias = bias.data(); a.act = 1; a.dtype = BLIM_COMPUTE_BF16;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    a = plain; a.ldc = 2 * (N + 8); a.lo_off = N + 8; a.lda = 2 * K; a.K = 2 * K; a.w_wrap_k = K;                  // compensated: [hi | lo] in, hi | lo out
    EXPECT(blim_gemm(&a, nullptr) == 0);
    const blim_gemm_args split = a;
    a = plain; a.swiglu_act = act.data(); a.swiglu_act_ld = N / 2;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    a = plain; a.swiglu_gu = gu.data(); a.swiglu_ld = 2 * N + 8;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    a = plain; a.epi = BLIM_EPI_F32; a.C = C32.data(); a.ldc = N + 3; a.scale = 0.5f;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    a = plain; a.epi = BLIM_EPI_RESID; a.C = C32.data(); a.ldc = N + 4; a.bias = bias.data(); a.resid_in = C32.data();
    EXPECT(blim_gemm(&a, nullptr) == 0);
    const blim_gemm_args resid = a;
    a = plain; a.epi = BLIM_EPI_QKV; a.bias = bias.data(); a.rope_cols = 384; a.rope_rows = rope.data(); a.rope_stride = 512;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    const blim_gemm_args qkv = a;
    a = plain; a.epi = BLIM_EPI_SWIGLU;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    a = plain; a.epi = BLIM_EPI_LSE; a.C = nullptr; a.labels = labels.data(); a.lse_part = part.data(); a.label_logit = ll.data();
    EXPECT(blim_gemm(&a, nullptr) == 0);
    const blim_gemm_args lse = a;
    a = plain; a.epi = BLIM_EPI_SWIGLU; a.lda = 2 * K; a.ldc = 2 * (N / 2 + 8); a.lo_off = N / 2 + 8; a.A6 = a6.data(); a.W6 = w6.data(); a.f6_build = 1; a.out6 = o6.data();
    EXPECT(blim_gemm(&a, nullptr) == 0);
    const blim_gemm_args lo6 = a;
    a = plain; a.dtype = BLIM_COMPUTE_F8; a.epi = BLIM_EPI_SWIGLU; a.row_scale = rs.data(); a.col_scale = cs.data(); a.C = nullptr; a.out8 = c8.data(); a.ldc = N / 2;
    a.out_mx = mx.data(); a.mx_stride = 512;
    EXPECT(blim_gemm(&a, nullptr) == 0);
    const blim_gemm_args f8 = a;
    a = plain; a.dtype = BLIM_COMPUTE_F8; a.epi = BLIM_EPI_RESID; a.C = C32.data(); a.ldc = N + 4; a.a_mx = mx.data(); a.mx_stride = 512; a.col_scale = cs.data();
    EXPECT(blim_gemm(&a, nullptr) == 0);
    a = plain; a.struct_bytes = (int64_t)((const char*)&a.bias - (const char*)&a);                                  // the shortest caller: the plain product
    EXPECT(blim_gemm(&a, nullptr) == 0);
    // ---- refusals
    EXPECT(blim_gemm(nullptr, nullptr) == BLIM_ERR_ARG);
    a = plain; a.struct_bytes = 8;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.epi = 6;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.dtype = 3;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.A = nullptr;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.C = nullptr;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.K = 96;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.ldc = N - 4;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.ldc = N + 2;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.act = 2;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = split; a.lo_off = N - 4;                                                                                     // a lo half that overlaps the output ...
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "lo_off"));
    a = split; a.lo_off = N + 20;                                                                                    // ... or leaves the row
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "lo_off"));
    a = resid; a.lo_off = N;                                                                                         // split outputs of an f32 epilogue
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "split"));
    a = split; a.w_wrap_k = K / 2;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = qkv; a.rope_cols = N + 128;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "rope_cols"));
    a = qkv; a.bias = nullptr;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = qkv; a.rope_stride = M - 1;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = qkv; a.rope_cols = 320;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.rope_cols = 128;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = lse; a.labels = nullptr;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.epi = BLIM_EPI_F32; a.C = C32.data(); a.bias = bias.data();
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.resid_in = C32.data();
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = lo6; a.W6 = nullptr;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "e2m3"));
    a = lo6; a.lda = K;                                                                                              // f6_build without a lo part behind A
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = lo6; a.f6_build = 0; a.K6 = 0;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = lo6; a.lo_off = 0; a.ldc = N / 2 + 8;                                                                        // out6 without split outputs
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = qkv; a.lda = 2 * K; a.A6 = a6.data(); a.W6 = w6.data(); a.f6_build = 1;                                      // lo6 QKV with plain outputs
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "hi | lo"));
    a = f8; a.out_mx = nullptr;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = f8; a.dtype = BLIM_COMPUTE_F16;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "out8"));
    a = f8; a.mx_stride = 256;                                                                                       // M = 300: two row tiles
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = f8; a.col_scale = nullptr;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.swiglu_act = act.data(); a.swiglu_act_ld = N / 2; a.swiglu_gu = gu.data(); a.swiglu_ld = 2 * N + 8;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.swiglu_gu = gu.data(); a.swiglu_ld = 2 * N - 8;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG);
    a = plain; a.epi = BLIM_EPI_SWIGLU; a.swiglu_act = act.data(); a.swiglu_act_ld = N / 2;
    EXPECT(blim_gemm(&a, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "trainer"));
}

// the engine-less entries of the trainer's small kernels: one good call each, then every refusal and the workspace-size arithmetic
static uint8_t* aligned16(std::vector<uint8_t>& mem) { return mem.data() + (16 - ((uintptr_t)mem.data() & 15)) % 16; }
static void train_kernel_calls() {
    const int T = 70, K = 48, N = 100, r = 8, H = 128;
    std::vector<uint16_t> x16((size_t)T * (K + 64), 0), dy16((size_t)T * 120, 0), o16((size_t)T * 2 * H, 0);
    std::vector<float> A((size_t)16 * H, 0.f), B((size_t)N * 16, 0.f), dB((size_t)N * 16, 0.f), du((size_t)T * 16, 0.f), dA((size_t)16 * K, 0.f), f32a((size_t)T * H, 0.f),
        f32b((size_t)T * H, 0.f), f32c((size_t)T * H, 0.f), w(H, 1.f), stats(2, 0.f), loss(1, 0.f);
    std::vector<int32_t> rows = {3, 1, 0}, labels(T, 2);
    std::vector<uint8_t> ws_mem(1 << 20, 0xFF);
    uint8_t* const ws = aligned16(ws_mem);
    // ---- blim_lora_down
    EXPECT(blim_lora_down_workspace_bytes(3, K) == 3 * 16 * K * 2 && blim_lora_down_workspace_bytes(1, 1024) == 32768);
    EXPECT(blim_lora_down_workspace_bytes(0, K) == -1 && blim_lora_down_workspace_bytes(4, K) == -1 && blim_lora_down_workspace_bytes(1, K + 8) == -1 && blim_lora_down_workspace_bytes(1, 0) == -1);
    blim_lora_down_args d;
    memset(&d, 0, sizeof d);
    d.struct_bytes = sizeof d; d.x16 = x16.data(); d.ldx = K + 64; d.T = T; d.K = K; d.n_adapters = 3; d.r = r; d.dtype16 = BLIM_COMPUTE_F16;
    d.A[0] = d.A[1] = d.A[2] = A.data(); d.scale = 2.f; d.drop_p = 0.1f; d.seed = 5; d.site = 8; d.workspace = ws; d.workspace_bytes = blim_lora_down_workspace_bytes(3, K);
    const blim_lora_down_args dgood = d;
    EXPECT(blim_lora_down(&d, nullptr) == 0);
    d.dtype16 = BLIM_COMPUTE_BF16; d.n_adapters = 1; d.r = 16; d.drop_p = 0.f;
    EXPECT(blim_lora_down(&d, nullptr) == 0);
    EXPECT(blim_lora_down(nullptr, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.struct_bytes = 8;      EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.x16 = nullptr;         EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.A[2] = nullptr;        EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.dtype16 = BLIM_COMPUTE_F8; EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.r = 0;                 EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.r = 17;                EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.n_adapters = 4;        EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.T = 0;                 EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.K = 40;                EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.ldx = K + 60;          EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.ldx = K + 16;          EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    d = dgood; d.drop_p = 1.f;          EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.x16 = x16.data() + 1;  EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG);
    d = dgood; d.workspace = nullptr;   EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    d = dgood; d.workspace = ws + 4;    EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "aligned"));
    d = dgood; d.workspace_bytes -= 2;  EXPECT(blim_lora_down(&d, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    // ---- blim_lora_grads
    const int all = BLIM_LORA_DB | BLIM_LORA_DU | BLIM_LORA_DA;
    EXPECT(blim_lora_grads_workspace_bytes(BLIM_LORA_DB, 2049, 264, 0, 16) == 3 * 264 * 16 * 4);                  // three time splits of 1,024 rows
    EXPECT(blim_lora_grads_workspace_bytes(BLIM_LORA_DA, 1024, 0, 136, 4) == 136 * 4 * 4 && blim_lora_grads_workspace_bytes(BLIM_LORA_DA, 1025, 0, 136, 4) == 2 * 136 * 4 * 4);
    EXPECT(blim_lora_grads_workspace_bytes(BLIM_LORA_DU, 33, 16, 0, 4) == 33 * 4 * 4 + 16 * 16 * 2);               // one slice [T, r], rounded up to 16 bytes, then Bt16 [16, 16]
    EXPECT(blim_lora_grads_workspace_bytes(BLIM_LORA_DU, 33, 9, 0, 4) == blim_lora_grads_workspace_bytes(BLIM_LORA_DU, 33, 16, 0, 4));      // N rounds up to 16
    EXPECT(blim_lora_grads_workspace_bytes(all, T, N, K, r) % 16 == 0 && blim_lora_grads_workspace_bytes(all, T, N, K, r) >= blim_lora_grads_workspace_bytes(BLIM_LORA_DU, T, N, K, r));
    EXPECT(blim_lora_grads_workspace_bytes(0, T, N, K, r) == -1 && blim_lora_grads_workspace_bytes(8, T, N, K, r) == -1 && blim_lora_grads_workspace_bytes(all, 0, N, K, r) == -1);
    EXPECT(blim_lora_grads_workspace_bytes(all, T, 0, K, r) == -1 && blim_lora_grads_workspace_bytes(all, T, N, 4, r) == -1 && blim_lora_grads_workspace_bytes(all, T, N, K, 17) == -1);
    EXPECT(blim_lora_grads_workspace_bytes(BLIM_LORA_DA, T, 0, K, r) > 0 && blim_lora_grads_workspace_bytes(BLIM_LORA_DB, T, N, 0, r) > 0);      // the unused width is not looked at
    blim_lora_grads_args g;
    memset(&g, 0, sizeof g);
    g.struct_bytes = sizeof g; g.flags = all; g.dtype16 = BLIM_COMPUTE_F16; g.T = T; g.N = N; g.K = K; g.r = r; g.dy16 = dy16.data(); g.ldy = 120; g.u16 = x16.data() + K; g.ldu = K + 64;
    g.x16 = x16.data(); g.ldx = K + 64; g.B = B.data(); g.scale = 2.f; g.drop_p = 0.1f; g.seed = 5; g.site = 8; g.dB = dB.data(); g.du = du.data(); g.dA = dA.data();
    g.workspace = ws; g.workspace_bytes = blim_lora_grads_workspace_bytes(all, T, N, K, r);
    const blim_lora_grads_args ggood = g;
    EXPECT(blim_lora_grads(&g, nullptr) == 0);
    for (int flags = 1; flags <= 7; ++flags) { g = ggood; g.flags = flags; g.dtype16 = flags & 1 ? BLIM_COMPUTE_BF16 : BLIM_COMPUTE_F16; EXPECT(blim_lora_grads(&g, nullptr) == 0); }
    g = ggood; g.flags = BLIM_LORA_DB; g.ldy = 104; g.B = nullptr; g.x16 = nullptr; g.du = nullptr; g.dA = nullptr; g.K = 0;      // dB alone: N rounded up to 8 is enough, the rest unused
    EXPECT(blim_lora_grads(&g, nullptr) == 0);
    EXPECT(blim_lora_grads(nullptr, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.struct_bytes = 8;      EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.flags = 0;             EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.flags = 8;             EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.dtype16 = BLIM_COMPUTE_F8; EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.r = 17;                EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.T = 0;                 EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.N = 0;                 EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.dy16 = nullptr;        EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.ldy = 116;             EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.ldy = 104;             EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "rounded up to 16"));      // du contracts over round_up(N, 16)
    g = ggood; g.flags = BLIM_LORA_DB; g.ldy = 96; EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "rounded up to 8"));
    g = ggood; g.u16 = nullptr;         EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.ldu = r - 1;           EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.dB = nullptr;          EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.B = nullptr;           EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.du = nullptr;          EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.dA = nullptr;          EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.x16 = nullptr;         EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.K = 44;                EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.ldx = K + 4;           EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.ldx = K - 8;           EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    g = ggood; g.drop_p = -0.1f;        EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG);
    g = ggood; g.workspace = nullptr;   EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    g = ggood; g.workspace = ws + 8;    EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "aligned"));
    g = ggood; g.workspace_bytes -= 2;  EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    g = ggood; g.T = 2049;              EXPECT(blim_lora_grads(&g, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));      // three time splits: the same workspace is too small now
    // ---- blim_lora_dx
    blim_lora_dx_args x;
    memset(&x, 0, sizeof x);
    x.struct_bytes = sizeof x; x.dx = f32a.data(); x.ldd = H; x.T = T; x.K = H - 4; x.n_adapters = 3; x.r = r; x.dtype16 = BLIM_COMPUTE_F16;
    x.du[0] = x.du[1] = x.du[2] = du.data(); x.A[0] = x.A[1] = x.A[2] = A.data(); x.drop_p = 0.1f; x.site = 8; x.seed = 5;
    const blim_lora_dx_args xgood = x;
    EXPECT(blim_lora_dx(&x, nullptr) == 0);
    x.out16 = o16.data(); x.ldo = H; x.dtype16 = BLIM_COMPUTE_BF16; x.n_adapters = 1;
    EXPECT(blim_lora_dx(&x, nullptr) == 0);
    const blim_lora_dx_args x16good = x;
    EXPECT(blim_lora_dx(nullptr, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.struct_bytes = 8;      EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.dx = nullptr;          EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.dx = f32a.data() + 1;  EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.du[1] = nullptr;       EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.A[2] = nullptr;        EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.n_adapters = 0;        EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.r = 17;                EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.T = 0;                 EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.K = H - 2;             EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.ldd = H + 2;           EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.ldd = H - 8;           EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    x = xgood; x.dtype16 = BLIM_COMPUTE_F8; EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = xgood; x.drop_p = 1.5f;         EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = x16good; x.ldo = H - 2;         EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG);
    x = x16good; x.ldo = H - 8;         EXPECT(blim_lora_dx(&x, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    // ---- blim_rmsnorm_bwd
    blim_rmsnorm_bwd_args n;
    memset(&n, 0, sizeof n);
    n.struct_bytes = sizeof n; n.dx = f32a.data(); n.dy = f32b.data(); n.x = f32c.data(); n.n_rows = 5; n.H = H; n.w = w.data(); n.eps = 1e-6f; n.dtype16 = BLIM_COMPUTE_F16;
    const blim_rmsnorm_bwd_args ngood = n;
    EXPECT(blim_rmsnorm_bwd(&n, nullptr) == 0);
    n.rows = rows.data(); n.n_rows = 3; n.accumulate = 1;
    EXPECT(blim_rmsnorm_bwd(&n, nullptr) == 0);
    n = ngood; n.out16 = o16.data(); n.dtype16 = BLIM_COMPUTE_BF16;
    EXPECT(blim_rmsnorm_bwd(&n, nullptr) == 0);
    n.n_adapters = 3; n.r = r; n.du[0] = n.du[1] = n.du[2] = du.data(); n.A[0] = n.A[1] = n.A[2] = A.data(); n.drop_p = 0.1f; n.accumulate = 1;
    EXPECT(blim_rmsnorm_bwd(&n, nullptr) == 0);
    const blim_rmsnorm_bwd_args nfused = n;
    EXPECT(blim_rmsnorm_bwd(nullptr, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.struct_bytes = 8;      EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.dx = nullptr;          EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.dy = nullptr;          EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.x = nullptr;           EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.w = nullptr;           EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.dy = f32b.data() + 1;  EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.n_rows = 0;            EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.H = H + 2;             EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.dtype16 = BLIM_COMPUTE_F8; EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.n_adapters = 4;        EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = ngood; n.H = 8196;              EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "> 8192"));
    n = ngood; n.rows = rows.data(); n.n_rows = 3; n.out16 = o16.data(); EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "out16 with rows"));
    n = nfused; n.out16 = nullptr; n.rows = rows.data(); n.n_rows = 3;   EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "adapters with rows"));
    n = nfused; n.H = 4100;             EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "> 4096"));
    n = nfused; n.r = 0;                EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = nfused; n.r = 17;               EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = nfused; n.du[2] = nullptr;      EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = nfused; n.A[0] = nullptr;       EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    n = nfused; n.drop_p = 1.f;         EXPECT(blim_rmsnorm_bwd(&n, nullptr) == BLIM_ERR_ARG);
    // ---- blim_ce_fwd_bwd
    const int V = 61;
    EXPECT(blim_ce_workspace_bytes(16) == 64 && blim_ce_workspace_bytes(5) == 32 && blim_ce_workspace_bytes(0) == -1 && blim_ce_workspace_bytes(1ll << 31) == -1);
    const int64_t cneed = blim_ce_workspace_bytes(T);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == 0);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 4, T, 0.5f, nullptr, f32b.data(), V, loss.data(), BLIM_COMPUTE_BF16, ws, cneed, nullptr) == 0);
    EXPECT(blim_ce_fwd_bwd(nullptr, 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, nullptr, 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, nullptr, BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 0, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, 0, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, 0, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F8, ws, cneed, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, nullptr, nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "exactly one"));
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), f32b.data(), 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "exactly one"));
    EXPECT(blim_ce_fwd_bwd(f32a.data(), V - 1, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, V - 1, loss.data(), BLIM_COMPUTE_F16, ws, cneed, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "row stride"));
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, nullptr, cneed, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws + 4, cneed, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "aligned"));
    EXPECT(blim_ce_fwd_bwd(f32a.data(), 64, V, labels.data(), 1, T, 0.5f, o16.data(), nullptr, 64, loss.data(), BLIM_COMPUTE_F16, ws, cneed - 16, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    // ---- blim_gelu
    EXPECT(blim_gelu(0, o16.data(), H + 8, x16.data(), nullptr, 20, H, BLIM_COMPUTE_F16, nullptr) == 0);
    EXPECT(blim_gelu(1, o16.data(), H, x16.data(), f32a.data(), 20, H, BLIM_COMPUTE_BF16, nullptr) == 0);
    EXPECT(blim_gelu(0, nullptr, H, x16.data(), nullptr, 20, H, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_gelu(0, o16.data(), H, nullptr, nullptr, 20, H, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_gelu(0, o16.data(), H, x16.data(), nullptr, 0, H, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_gelu(0, o16.data(), H, x16.data(), nullptr, 20, 0, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_gelu(0, o16.data(), H, x16.data(), nullptr, 20, H, BLIM_COMPUTE_F8, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_gelu(0, o16.data(), H - 1, x16.data(), nullptr, 20, H, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "shorter"));
    EXPECT(blim_gelu(1, o16.data(), H, x16.data(), nullptr, 20, H, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_gelu(1, o16.data(), H + 8, x16.data(), f32a.data(), 20, H, BLIM_COMPUTE_F16, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "contiguous"));
    // ---- blim_adamw_raw, blim_grad_stats_raw
    EXPECT(blim_adamw_raw(f32a.data(), f32b.data(), f32c.data(), du.data(), 257, 1e-3f, 0.9f, 0.95f, 1e-8f, 0.05f, 1.f, 1, nullptr) == 0);
    EXPECT(blim_adamw_raw(nullptr, f32b.data(), f32c.data(), du.data(), 257, 1e-3f, 0.9f, 0.95f, 1e-8f, 0.05f, 1.f, 1, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_adamw_raw(f32a.data(), nullptr, f32c.data(), du.data(), 257, 1e-3f, 0.9f, 0.95f, 1e-8f, 0.05f, 1.f, 1, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_adamw_raw(f32a.data(), f32b.data(), nullptr, du.data(), 257, 1e-3f, 0.9f, 0.95f, 1e-8f, 0.05f, 1.f, 1, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_adamw_raw(f32a.data(), f32b.data(), f32c.data(), nullptr, 257, 1e-3f, 0.9f, 0.95f, 1e-8f, 0.05f, 1.f, 1, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_adamw_raw(f32a.data(), f32b.data(), f32c.data(), du.data(), 0, 1e-3f, 0.9f, 0.95f, 1e-8f, 0.05f, 1.f, 1, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_adamw_raw(f32a.data(), f32b.data(), f32c.data(), du.data(), 257, 1e-3f, 0.9f, 0.95f, 1e-8f, 0.05f, 1.f, 0, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_grad_stats_workspace_bytes(1) == 4096 && blim_grad_stats_workspace_bytes(256 * 1024 + 5) == 4096 && blim_grad_stats_workspace_bytes(0) == -1);
    EXPECT(blim_grad_stats_raw(f32a.data(), 257, 1.f, stats.data(), ws, 4096, nullptr) == 0);
    EXPECT(blim_grad_stats_raw(nullptr, 257, 1.f, stats.data(), ws, 4096, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_grad_stats_raw(f32a.data(), 257, 1.f, nullptr, ws, 4096, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_grad_stats_raw(f32a.data(), 0, 1.f, stats.data(), ws, 4096, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_grad_stats_raw(f32a.data(), 257, 1.f, stats.data(), nullptr, 4096, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
    EXPECT(blim_grad_stats_raw(f32a.data(), 257, 1.f, stats.data(), ws + 4, 4096, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "aligned"));
    EXPECT(blim_grad_stats_raw(f32a.data(), 257, 1.f, stats.data(), ws, 4092, nullptr) == BLIM_ERR_ARG && strstr(blim_last_error(), "workspace"));
}

// the scoring path's row kernels alone (blim.h): pass-throughs -- the launchers are mocked here, so what is seen is the entries' own argument checks
static void score_kernel_calls() {
    const int H = 384, n = 5;
    std::vector<float> x((size_t)n * (H + 12), 0.f), w(H, 1.f), of((size_t)n * H, 0.f), part((size_t)n * 3 * 2, 0.f), ll(n, 0.f), lp(n, 0.f), sc(n, 0.f);
    std::vector<uint16_t> o16((size_t)n * 2 * H, 0), in16((size_t)n * 3 * 2 * H, 0), table((size_t)4 * H, 0);
    std::vector<uint8_t> o6((size_t)blim_f6_tiles_bytes(n, H), 0), o8((size_t)n * H, 0);
    std::vector<int32_t> rows = {3, 1, 0, -1, 4}, labels(n, 2), src = {0, -1, 3, -2, 1};
    blim_rmsnorm_args a;
    memset(&a, 0, sizeof a);
    a.struct_bytes = sizeof a; a.x = x.data(); a.ldx = H + 12; a.n_rows = n; a.H = H; a.dtype16 = BLIM_COMPUTE_F16; a.w = w.data(); a.eps = 1e-6f; a.saturate = 1;
    a.out16 = o16.data(); a.ldo = 2 * H; a.out_lo = o16.data() + H; a.out_f32 = of.data(); a.out6 = o6.data();
    const blim_rmsnorm_args good = a;
    EXPECT(blim_rmsnorm(&a, nullptr) == 0);
    a.rows = rows.data(); a.n_src = 4; a.dtype16 = BLIM_COMPUTE_BF16; a.out_lo = nullptr; a.ldo = 0;
    EXPECT(blim_rmsnorm(&a, nullptr) == 0);
    EXPECT(blim_rmsnorm(nullptr, nullptr) == BLIM_ERR_ARG);
    a = good; a.struct_bytes = 8;               EXPECT(blim_rmsnorm(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.dtype16 = BLIM_COMPUTE_F8;      EXPECT(blim_rmsnorm(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.H = 0;                          EXPECT(blim_rmsnorm(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.ldx = H - 4;                    EXPECT(blim_rmsnorm(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.ldo = H - 4;                    EXPECT(blim_rmsnorm(&a, nullptr) == BLIM_ERR_ARG);
    a = good; a.rows = rows.data(); a.n_src = 0; EXPECT(blim_rmsnorm(&a, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_rmsnorm_f8(x.data(), H + 12, n, H, w.data(), 1e-6f, o8.data(), sc.data(), nullptr) == 0);
    EXPECT(blim_rmsnorm_f8(x.data(), H - 4, n, H, w.data(), 1e-6f, o8.data(), sc.data(), nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_lse_combine(part.data(), 3, ll.data(), labels.data(), n, lp.data(), nullptr) == 0);
    EXPECT(blim_tvg_criterion(x.data(), H + 12, H, labels.data(), 1, n, sc.data(), nullptr) == 0);
    EXPECT(blim_tvg_criterion(x.data(), H - 1, H, labels.data(), 1, n, sc.data(), nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_group_mean_rows(o16.data(), in16.data(), n, 3, H, BLIM_COMPUTE_F16, 1, nullptr) == 0);
    EXPECT(blim_group_mean_rows(o16.data(), in16.data(), n, 3, H, BLIM_COMPUTE_BF16, 0, nullptr) == 0);
    EXPECT(blim_group_mean_rows(o16.data(), in16.data(), n, 3, H, BLIM_COMPUTE_F8, 0, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_assemble_rows(o16.data(), src.data(), n, H, table.data(), in16.data(), 1, nullptr) == 0);
    EXPECT(blim_assemble_rows(o16.data(), src.data(), n, 0, table.data(), in16.data(), 0, nullptr) == BLIM_ERR_ARG);
}

int main() {
    EXPECT(blim_abi_version() == BLIM_ABI_VERSION);
    attention_calls();
    attention_bwd_calls();
    gemm_calls();
    train_kernel_calls();
    score_kernel_calls();
    blim_engine* e = nullptr;
    // ---- creation: bad configurations, no device
    {
        blim_config c = cfg_of(BLIM_COMPUTE_F16);
        EXPECT(blim_create(nullptr, &e) == BLIM_ERR_ARG && blim_create(&c, nullptr) == BLIM_ERR_ARG);
        blim_config bad = c; bad.hidden_size = 192;                                    // head_dim != 128
        EXPECT(blim_create(&bad, &e) == BLIM_ERR_ARG && strstr(blim_last_error(), "head_dim"));
        bad = c; bad.compute_dtype = 7;
        EXPECT(blim_create(&bad, &e) == BLIM_ERR_ARG);
        bad = c; bad.num_layers = 0;
        EXPECT(blim_create(&bad, &e) != 0);
        mock_hip_device_count = 0;
        EXPECT(blim_create(&c, &e) != 0);                                              // the product path fails loudly without a device
        mock_hip_device_count = 1;
        mock_hip_mem_limit = 1 << 20;                                                  // out of device memory half way through the weight allocations
        EXPECT(blim_create(&c, &e) != 0);
        mock_hip_mem_limit = 0;
    }
    EXPECT(mock_hip_live_allocations() == 0);                                          // failed creations release what they had taken
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16, BLIM_COMPUTE_F8}) {
        const blim_config c = cfg_of(dtype);
        EXPECT(blim_create(&c, &e) == 0 && e);
        if (!e) continue;
        // ---- weights: state before loading, unknown names, f32 and bf16 sources, host and "device" pointers, synthetic fill, reloads
        EXPECT(blim_weights_ready(e) == BLIM_ERR_STATE);
        {
            Batch B(1, 8, false);
            std::vector<uint16_t> emb((size_t)8 * c.hidden_size, 0), out((size_t)8 * c.hidden_size, 0);
            EXPECT(blim_decode(e, &B.b, emb.data(), nullptr, 0, out.data(), nullptr, nullptr) == BLIM_ERR_STATE && strstr(blim_last_error(), "not loaded"));
        }
        std::vector<float> z(16, 0.f);
        EXPECT(blim_load_weight(e, "layers.0.nonsense", z.data(), BLIM_DTYPE_F32, 0) == BLIM_ERR_ARG && strstr(blim_last_error(), "unknown weight"));
        EXPECT(blim_load_weight(e, "layers.9.q_proj.w", z.data(), BLIM_DTYPE_F32, 0) == BLIM_ERR_ARG);
        EXPECT(blim_load_weight(e, "lm_head", z.data(), 5, 0) == BLIM_ERR_ARG && blim_load_weight(e, nullptr, z.data(), 0, 0) == BLIM_ERR_ARG);
        load_all(e, c, BLIM_DTYPE_F32);
        EXPECT(blim_weights_ready(e) == 0);
        load_all(e, c, BLIM_DTYPE_BF16);
        EXPECT(blim_init_synthetic_weights(e, 3) == 0);
        // ---- options: every key, both values, refusals
        for (const char* k : {"precise", "precise_embeds", "precise_mlp", "precise_lo6", "prune_last", "f8_fuse", "f8_mask", "attn_tr"}) {
            for (int v : {0, 1}) {
                const int rc = blim_set_option(e, k, v);
                EXPECT(rc == 0 || rc == BLIM_ERR_ARG || rc == BLIM_ERR_STATE);
            }
        }
        EXPECT(blim_set_option(e, "no_such_option", 1) == BLIM_ERR_ARG && blim_set_option(e, nullptr, 1) == BLIM_ERR_ARG);
        if (dtype == BLIM_COMPUTE_F8) EXPECT(blim_set_option(e, "precise", 1) != 0 && blim_set_option(e, "precise_lo6", 1) != 0);
        const bool lo6_dims = c.hidden_size % 128 == 0 && c.intermediate_size % 128 == 0;
        // bf16 engines take the e2m3 second pass as an opt-in since round 6 (same size rule as fp16 engines); left off again for the calls below
        if (dtype == BLIM_COMPUTE_BF16) { EXPECT(blim_set_option(e, "precise_lo6", 1) == (lo6_dims ? 0 : BLIM_ERR_ARG)); EXPECT(blim_set_option(e, "precise_lo6", 0) == 0); }
        EXPECT(blim_set_option(e, "prune_last", 1) == 0 && blim_set_option(e, "f8_fuse", 1) == 0 && blim_set_option(e, "f8_mask", 31) == 0);
        // ---- workspaces: growth in steps, then the calls in every numeric mode
        for (int64_t t : {64, 300, 5000, 200}) EXPECT(blim_reserve(e, t, t / 2 + 1) == 0);
        EXPECT(blim_reserve(e, -1, 0) == BLIM_ERR_ARG);
        EXPECT(blim_timing_enable(e, 1) == 0);
        const bool can_precise = dtype != BLIM_COMPUTE_F8;
        for (int precise = 0; precise <= (can_precise ? 1 : 0); ++precise) {
            EXPECT(blim_set_option(e, "precise", precise) == 0);
            for (int mlp = 0; mlp <= precise; ++mlp) {
                EXPECT(blim_set_option(e, "precise_mlp", mlp) == 0);
                if (precise) EXPECT(blim_set_option(e, "precise_embeds", mlp) == 0);
                const bool lo6_engine = dtype == BLIM_COMPUTE_F16 || (dtype == BLIM_COMPUTE_BF16 && lo6_dims);
                for (int lo6 = 0; lo6 <= ((precise && lo6_engine) ? 1 : 0); ++lo6) {
                    if (lo6_engine) EXPECT(blim_set_option(e, "precise_lo6", lo6) == 0);
                    score_calls(e, c, 3, 40, false);
                    score_calls(e, c, 2, 70, true);
                }
            }
        }
        {
            std::vector<double> ms(blim_timing_num_classes()), fl(blim_timing_num_classes());
            std::vector<int64_t> calls(blim_timing_num_classes());
            EXPECT(blim_timing_report(e, ms.data(), calls.data(), fl.data()) == 0);
            for (int i = 0; i < blim_timing_num_classes(); ++i) EXPECT(blim_timing_class_name(i) != nullptr);
            EXPECT(blim_timing_enable(e, 0) == 0);
        }
        // ---- a position beyond the RoPE table
        {
            Batch B(1, 8, false);
            B.pos[3] = 4000;
            std::vector<uint16_t> emb((size_t)8 * c.hidden_size * 2, 0), out((size_t)8 * c.hidden_size * 2, 0);
            const int rc = blim_decode(e, &B.b, emb.data(), nullptr, 0, out.data(), nullptr, nullptr);
            EXPECT(rc == 0 || rc == BLIM_ERR_ARG);          // device data: the library may not see it (blim.h); it must not fault on the host
            blim_batch bad = B.b; bad.n_tokens = 0;
            EXPECT(blim_decode(e, &bad, emb.data(), nullptr, 0, out.data(), nullptr, nullptr) == BLIM_ERR_ARG);
            bad = B.b; bad.seq_len = nullptr;
            EXPECT(blim_decode(e, &bad, emb.data(), nullptr, 0, out.data(), nullptr, nullptr) == BLIM_ERR_ARG);
        }
        // ---- adapters apart: ranks 4 / 8 / 16, partial sets, a rank change refused, reload over a live set, clear; derived copies rebuilt lazily in between
        const int H = c.hidden_size, M = c.mm_hidden_size, V = c.vocab_size, qn = c.num_heads * 128, kn = c.num_kv_heads * 128;
        std::vector<float> A((size_t)16 * std::max(H, M), 0.01f), Bm((size_t)std::max(V, H) * 16, 0.02f), Wbig((size_t)c.vocab_size * H, 0.03f);
        for (int r : {4, 8, 16}) {
            EXPECT(blim_clear_adapters(e) == 0 && blim_num_adapters(e) == 0);
            EXPECT(blim_load_adapter(e, "layers.0.q_proj.w", A.data(), Bm.data(), r, 32.f) == 0);
            EXPECT(blim_load_adapter(e, "layers.0.q_proj.w", A.data(), Bm.data(), r == 4 ? 8 : 4, 32.f) != 0);                     // one rank / scale per engine
            EXPECT(blim_load_adapter(e, "layers.0.nonsense", A.data(), Bm.data(), r, 32.f) == BLIM_ERR_ARG);
            EXPECT(blim_load_adapter(e, "layers.0.q_proj.w", nullptr, Bm.data(), r, 32.f) == BLIM_ERR_ARG && blim_load_adapter(e, "lm_head", A.data(), Bm.data(), 17, 32.f) == BLIM_ERR_ARG);
            if (can_precise) { EXPECT(blim_set_option(e, "precise", 1) == 0); }
            score_calls(e, c, 2, 40, false);                                                     // a partial set: one adapter
            for (int l = 0; l < c.num_layers; ++l)
                for (const char* t : {"q_proj.w", "k_proj.w", "v_proj.w", "o_proj.w"}) EXPECT(blim_load_adapter(e, ("layers." + std::to_string(l) + "." + t).c_str(), A.data(), Bm.data(), r, 32.f) == 0);
            for (const char* n : {"lm_head", "mlp.0.w", "mlp.2.w", "tvg_mlp.0.w", "tvg_mlp.2.w"}) EXPECT(blim_load_adapter(e, n, A.data(), Bm.data(), r, 32.f) == 0);
            EXPECT(blim_num_adapters(e) == 4 * c.num_layers + 5);
            score_calls(e, c, 2, 40, true);
            EXPECT(blim_load_weight(e, "layers.1.down_proj.w", Wbig.data(), BLIM_DTYPE_F32, 0) == 0);     // a base weight replaced under live adapters
            EXPECT(blim_load_adapter(e, "lm_head", A.data(), Bm.data(), r, 32.f) == 0);                   // ... and an adapter reloaded
            if (can_precise) { EXPECT(blim_set_option(e, "precise", 0) == 0); }
            score_calls(e, c, 2, 40, false);
        }
        EXPECT(blim_clear_adapters(e) == 0 && blim_num_adapters(e) == 0);
        (void)qn; (void)kn;
        // ---- out of device memory while a call grows its workspace / builds its derived copies: an error code, and the engine stays usable
        if (dtype == BLIM_COMPUTE_F16) {
            EXPECT(blim_set_option(e, "precise", 1) == 0 && blim_set_option(e, "precise_lo6", 1) == 0);
            EXPECT(blim_load_weight(e, "layers.0.o_proj.w", Wbig.data(), BLIM_DTYPE_F32, 0) == 0);
            mock_hip_mem_limit = mock_hip_mem_in_use + 4096;
            Batch B(60, 120, false);                                                      // 7,200 tokens: more than any call before, the workspaces must grow
            std::vector<uint16_t> emb((size_t)7200 * c.hidden_size * 2, 0), out((size_t)7200 * c.hidden_size * 2, 0);
            EXPECT(blim_decode(e, &B.b, emb.data(), nullptr, 0, out.data(), nullptr, nullptr) != 0);
            mock_hip_mem_limit = 0;
            EXPECT(blim_decode(e, &B.b, emb.data(), nullptr, 0, out.data(), nullptr, nullptr) == 0);
            EXPECT(blim_set_option(e, "precise", 0) == 0);
        }
        // ---- the trainer's life cycle on this engine
        {
            blim_train_config tc; tc.lora_r = 8; tc.lora_alpha = 32.f; tc.lora_dropout = 0.05f;
            const int64_t n = blim_train_flat_size(e, tc.lora_r);
            EXPECT(n > 0 && blim_train_flat_size(e, 17) < 0);
            int64_t off = -1, rows = 0, cols = 0;
            EXPECT(blim_train_param_offset(e, 8, "lm_head:B", &off, &rows, &cols) == 0 && rows == V && cols == 8 && off >= 0 && off + rows * cols <= n);
            EXPECT(blim_train_param_offset(e, 8, "layers.1.k_proj.w:A", &off, &rows, &cols) == 0 && rows == 8 && cols == H);
            EXPECT(blim_train_param_offset(e, 8, "visual_head", &off, &rows, &cols) == 0 && rows == M && cols == H);
            EXPECT(blim_train_param_offset(e, 8, "layers.7.k_proj.w:A", &off, &rows, &cols) != 0 && blim_train_param_offset(e, 8, "lm_head:C", &off, &rows, &cols) != 0);
            std::vector<float> params((size_t)std::max<int64_t>(n, 1), 0.f), grads(params.size(), 0.f), m1(params.size(), 0.f), m2(params.size(), 0.f);
            blim_trainer* t = nullptr;
            EXPECT(blim_train_create(e, nullptr, params.data(), grads.data(), &t) == BLIM_ERR_ARG);
            EXPECT(blim_train_create(e, &tc, params.data(), grads.data(), &t) == 0 && t);
            if (t) {
                EXPECT(blim_train_sync_params(t, nullptr) == 0);
                Batch B(3, 48, false);
                const int64_t T = B.b.n_tokens;
                std::vector<int32_t> src((size_t)T, 5), rows_v = {10, 11, 12, 60, 61}, labels = {1, 2, 3, 4, 5}, trows = {100, 101, 102, 103}, tlab = {2};
                std::vector<uint16_t> feats((size_t)256 * M, 0), vocab((size_t)c.num_clips * 8 * M, 0);
                src[3] = -1; src[4] = -2; src[100] = -(256 + 1);
                blim_train_batch tb; memset(&tb, 0, sizeof tb);
                tb.batch = &B.b; tb.src_index = src.data(); tb.feats = feats.data(); tb.n_feat_rows = 256; tb.tok_per_clip = 64; tb.max_seq_len = 48;
                tb.rows = rows_v.data(); tb.labels = labels.data(); tb.n_rows = 5; tb.tvg_rows = trows.data(); tb.tvg_labels = tlab.data(); tb.n_tvg_rows = 4;
                tb.vocab = vocab.data(); tb.n_vocab = 8; tb.grad_scale = 1024.f; tb.dropout_seed = 9;
                float loss[2] = {0.f, 0.f}, stats[2] = {0.f, 0.f};
                const int rc = blim_train_step(t, &tb, loss, nullptr);
                EXPECT(dtype == BLIM_COMPUTE_F8 ? rc != 0 : rc == 0);
                tb.n_tvg_rows = 0; tb.tvg_rows = nullptr;                                          // VTG rows alone
                if (dtype != BLIM_COMPUTE_F8) EXPECT(blim_train_step(t, &tb, loss, nullptr) == 0);
                EXPECT(blim_train_grad_stats(t, 1.f / 1024.f, stats, nullptr) == 0);
                EXPECT(blim_train_adamw(t, m1.data(), m2.data(), 1e-4f, 0.9f, 0.95f, 1e-8f, 0.02f, 1.f / 1024.f, 1, nullptr) == 0);
                EXPECT(blim_train_merge(t, nullptr) == 0);
                // a merged engine refuses adapters apart until EVERY adapted weight has been re-placed (one reloaded norm used to lift the guard)
                EXPECT(blim_load_adapter(e, "lm_head", A.data(), Bm.data(), 8, 32.f) == BLIM_ERR_STATE);
                EXPECT(blim_load_weight(e, "final_norm", Wbig.data(), BLIM_DTYPE_F32, 0) == 0);
                EXPECT(blim_load_adapter(e, "lm_head", A.data(), Bm.data(), 8, 32.f) == BLIM_ERR_STATE);
                EXPECT(blim_load_weight(e, "lm_head", Wbig.data(), BLIM_DTYPE_F32, 0) == 0);
                EXPECT(blim_load_adapter(e, "lm_head", A.data(), Bm.data(), 8, 32.f) == BLIM_ERR_STATE);      // q/k/v/o and the projector still merged
                load_all(e, c, BLIM_DTYPE_F32);
                EXPECT(blim_load_adapter(e, "lm_head", A.data(), Bm.data(), 8, 32.f) == 0);
                EXPECT(blim_train_merge(t, nullptr) == BLIM_ERR_STATE);                                       // adapters apart: one or the other
                EXPECT(blim_clear_adapters(e) == 0);
                score_calls(e, c, 2, 40, false);
                blim_train_destroy(t);
            }
            blim_train_destroy(nullptr);
        }
        blim_destroy(e);
        e = nullptr;
        EXPECT(mock_hip_live_allocations() == 0);                                      // destroy frees every device allocation of the engine and its trainer
    }
    blim_destroy(nullptr);
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("host sanitizer drive: ok\n");
    return 0;
}
