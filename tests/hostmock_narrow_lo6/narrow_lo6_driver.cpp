// TEST INFRASTRUCTURE (tests/test_narrow_lo6_sanitizers.py): walks the HOST side of the switches of the narrow-tile residual GEMM with the e2m3 second pass -- option
// "narrow_lo6" of blim_set_option and the `tile_lo6` field of blim_gemm_args (blim.h) -- with csrc/engine.hip compiled as plain C++ against the mock HIP runtime of
// ../hostmock, under AddressSanitizer + UBSan.  Kernels and launchers do nothing here; what runs is the option's range check, a compensated decode under every value
// of it on an engine with "precise_lo6" on (run_layers attaches the e2m3 images and hands the value to its o_proj and down launches, whole batch and pruned rows),
// and every refusal of blim_gemm's tile_lo6, each naming its field.  Exit code 0 = every expectation met.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/blim.h"

extern "C" size_t mock_hip_live_allocations();

static int failures = 0;
#define EXPECT(cond)                                                                              \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "EXPECT failed: %s (%s:%d) last error: %s\n", #cond, __FILE__, __LINE__, blim_last_error()); ++failures; } \
    } while (0)
#define REFUSED(call, code, word) EXPECT((call) == (code) && strstr(blim_last_error(), word))

static blim_config cfg_of(int dtype) {
    blim_config c;
    memset(&c, 0, sizeof c);
    c.vocab_size = 1024; c.hidden_size = 256; c.intermediate_size = 512; c.num_layers = 2; c.num_heads = 2; c.num_kv_heads = 1;
    c.mm_hidden_size = 64; c.num_clips = 4; c.max_positions = 128; c.compute_dtype = dtype; c.rms_eps = 1e-6f; c.rope_theta = 1e6f;
    return c;
}

static void walk_option(int dtype) {
    const blim_config c = cfg_of(dtype);
    blim_engine* e = nullptr;
    EXPECT(blim_create(&c, &e) == 0 && e);
    if (!e) return;
    EXPECT(blim_init_synthetic_weights(e, 3) == 0);
    EXPECT(blim_set_option(e, "precise_lo6", 1) == 0);                                               // fp16: the default; bf16: the opt-in
    const int L = 40;
    std::vector<int32_t> pos(L), blk_seq = {0, 0}, blk_q0 = {0, 32};
    std::vector<uint8_t> vis(L, 1);
    for (int i = 0; i < L; ++i) pos[i] = i;
    const int32_t seq_start = 0, seq_len = L, zero = 0;
    blim_batch b;
    memset(&b, 0, sizeof b);
    b.n_tokens = L; b.n_seqs = 1; b.n_blocks = 2; b.positions = pos.data(); b.key_visible = vis.data(); b.seq_start = &seq_start; b.seq_len = &seq_len;
    b.pfx_start = &zero; b.pfx_len = &zero; b.blk_seq = blk_seq.data(); b.blk_q0 = blk_q0.data(); b.own_start = nullptr;
    std::vector<uint16_t> emb((size_t)L * c.hidden_size * 2, 0), hid((size_t)L * c.hidden_size * 2, 0);
    const int32_t rows[2] = {L - 2, L - 1};
    for (int v : {0, 1, 2, 0}) {
        EXPECT(blim_set_option(e, "narrow_lo6", v) == 0);
        EXPECT(blim_set_option(e, "precise", 1) == 0);
        EXPECT(blim_decode(e, &b, emb.data(), nullptr, 0, hid.data(), nullptr, nullptr) == 0);       // compensated, whole batch
        EXPECT(blim_decode(e, &b, emb.data(), rows, 2, hid.data(), nullptr, nullptr) == 0);          // ... and the last layer's pruned rows
        EXPECT(blim_set_option(e, "precise_mlp", 0) == 0);                                           // o_proj alone carries the second pass
        EXPECT(blim_decode(e, &b, emb.data(), rows, 2, hid.data(), nullptr, nullptr) == 0);
        EXPECT(blim_set_option(e, "precise_mlp", 1) == 0);
        EXPECT(blim_set_option(e, "precise", 0) == 0);
        EXPECT(blim_decode(e, &b, emb.data(), rows, 2, hid.data(), nullptr, nullptr) == 0);          // plain: the option has nothing to choose
    }
    for (int v : {3, -1, 1 << 20}) REFUSED(blim_set_option(e, "narrow_lo6", v), BLIM_ERR_ARG, "narrow_lo6");
    EXPECT(blim_set_option(e, "narrow_lo6", 1) == 0);                                                // a refused value left the option as it was: still settable
    EXPECT(blim_set_option(e, "narrow_gemm", 2) == 0);                                               // both options together
    EXPECT(blim_set_option(e, "precise", 1) == 0);
    EXPECT(blim_decode(e, &b, emb.data(), rows, 2, hid.data(), nullptr, nullptr) == 0);
    REFUSED(blim_set_option(nullptr, "narrow_lo6", 1), BLIM_ERR_ARG, "bad argument");
    blim_destroy(e);
    EXPECT(mock_hip_live_allocations() == 0);
}

static void walk_gemm() {
    const int M = 8, N = 128, K = 128;
    std::vector<uint16_t> a((size_t)M * 2 * K, 0), w((size_t)N * K, 0), c16((size_t)M * 2 * N, 0);
    std::vector<float> c32((size_t)M * N, 0.f), scale(128, 1.f), part((size_t)M * 2, 0.f), ll(M, 0.f), rope((size_t)128 * M, 0.f), bias(N, 0.f);
    std::vector<int32_t> labels(M, 0);
    std::vector<uint8_t> img(1 << 16, 0);
    auto base = [&](int epi, int dtype, bool lo6) {
        blim_gemm_args g;
        memset(&g, 0, sizeof g);
        g.struct_bytes = sizeof g; g.epi = epi; g.dtype = dtype; g.A = a.data(); g.lda = 2 * K; g.W = w.data(); g.M = M; g.N = N; g.K = K;
        g.C = (epi == BLIM_EPI_F32 || epi == BLIM_EPI_RESID) ? (void*)c32.data() : (void*)c16.data(); g.ldc = epi == BLIM_EPI_QKV ? 2 * N : N; g.scale = 1.f; g.f16_saturate = 1;
        if (epi == BLIM_EPI_LSE) { g.C = nullptr; g.ldc = 0; g.labels = labels.data(); g.lse_part = part.data(); g.label_logit = ll.data(); }
        if (epi == BLIM_EPI_QKV) { g.bias = bias.data(); g.rope_rows = rope.data(); g.rope_stride = M; g.rope_cols = 128; g.lo_off = N; }
        if (lo6) { g.A6 = img.data(); g.W6 = img.data(); g.K6 = K; }
        return g;
    };
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16}) {
        for (int epi : {BLIM_EPI_RESID, BLIM_EPI_QKV, BLIM_EPI_SWIGLU, BLIM_EPI_LSE}) {              // the epilogues that have a second pass
            blim_gemm_args g = base(epi, dtype, true);
            for (int v : {0, 1}) { g.tile_lo6 = v; EXPECT(blim_gemm(&g, nullptr) == 0); }            // auto on an ineligible form: no error
            g.tile_lo6 = 2;
            if (epi == BLIM_EPI_RESID) EXPECT(blim_gemm(&g, nullptr) == 0);
            else REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "epi");
            for (int v : {3, -1, 1 << 30}) { g.tile_lo6 = v; REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "tile_lo6"); }
        }
        for (int epi : {BLIM_EPI_BF16, BLIM_EPI_F32}) {                                              // ... and those that have none
            blim_gemm_args g = base(epi, dtype, false);
            for (int v : {0, 1}) { g.tile_lo6 = v; EXPECT(blim_gemm(&g, nullptr) == 0); }
            g.tile_lo6 = 2;
            REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "epi");
        }
        {   // the residual epilogue's own forms under tile_lo6 = 2: resid_in and bias; the images built by the call
            blim_gemm_args g = base(BLIM_EPI_RESID, dtype, true);
            g.tile_lo6 = 2; g.resid_in = c32.data(); g.bias = bias.data();
            EXPECT(blim_gemm(&g, nullptr) == 0);
            g.f6_build = 1; g.K6 = 0;
            EXPECT(blim_gemm(&g, nullptr) == 0);
        }
        {   // no second pass: refused under 2 (A6 / W6 named), taken by the 256 x 256 kernel under 0 and 1; one image alone is no second pass either
            blim_gemm_args g = base(BLIM_EPI_RESID, dtype, false);
            for (int v : {0, 1}) { g.tile_lo6 = v; EXPECT(blim_gemm(&g, nullptr) == 0); }
            g.tile_lo6 = 2;
            REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "A6");
            g.A6 = img.data();
            REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "W6");
        }
        {   // the w_wrap_k form is `tile`'s: refused under 2 with the field named, untouched under 1
            blim_gemm_args g = base(BLIM_EPI_RESID, dtype, false);
            g.K = 2 * K; g.w_wrap_k = K;
            g.tile_lo6 = 1;
            EXPECT(blim_gemm(&g, nullptr) == 0);
            g.tile_lo6 = 2; g.A6 = img.data(); g.W6 = img.data(); g.K6 = K;
            REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "w_wrap_k");
        }
        {   // `tile` keeps its refusal of the second pass whatever tile_lo6 says
            blim_gemm_args g = base(BLIM_EPI_RESID, dtype, true);
            g.tile = 2;
            for (int v : {0, 1, 2}) { g.tile_lo6 = v; REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "tile = 2"); }
        }
    }
    {   // fp8: dtype named
        blim_gemm_args g = base(BLIM_EPI_RESID, BLIM_COMPUTE_F8, false);
        g.lda = K; g.row_scale = scale.data(); g.col_scale = scale.data();
        for (int v : {0, 1}) { g.tile_lo6 = v; EXPECT(blim_gemm(&g, nullptr) == 0); }
        g.tile_lo6 = 2;
        REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "dtype");
    }
    {   // a caller compiled before `tile_lo6` existed: the shorter struct reads as tile_lo6 = 0
        blim_gemm_args g = base(BLIM_EPI_RESID, BLIM_COMPUTE_F16, true);
        g.tile_lo6 = 7;
        g.struct_bytes = (int64_t)offsetof(blim_gemm_args, tile_lo6);
        EXPECT(blim_gemm(&g, nullptr) == 0);
    }
}

int main() {
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16}) walk_option(dtype);
    {   // fp8 engines take the option (it has nothing to choose there) and refuse the same values
        const blim_config c = cfg_of(BLIM_COMPUTE_F8);
        blim_engine* e = nullptr;
        EXPECT(blim_create(&c, &e) == 0 && e);
        if (e) {
            for (int v : {0, 1, 2, 0}) EXPECT(blim_set_option(e, "narrow_lo6", v) == 0);
            REFUSED(blim_set_option(e, "narrow_lo6", 3), BLIM_ERR_ARG, "narrow_lo6");
            blim_destroy(e);
        }
        EXPECT(mock_hip_live_allocations() == 0);
    }
    walk_gemm();
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("narrow lo6 sanitizer drive: ok\n");
    return 0;
}
