// TEST INFRASTRUCTURE (tests/test_narrow_gemm_sanitizers.py): walks the HOST side of the narrow-tile residual GEMM's switches -- option "narrow_gemm" of
// blim_set_option and the `tile` field of blim_gemm_args (blim.h) -- with csrc/engine.hip compiled as plain C++ against the mock HIP runtime of ../hostmock, under
// AddressSanitizer + UBSan.  Kernels and launchers do nothing here; what runs is the option's range check, a decode under every value of it (run_layers hands the
// value to its o_proj and down launches), and every refusal of blim_gemm's tile = 2, each naming its field.  Exit code 0 = every expectation met.
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
        EXPECT(blim_set_option(e, "narrow_gemm", v) == 0);
        EXPECT(blim_decode(e, &b, emb.data(), nullptr, 0, hid.data(), nullptr, nullptr) == 0);
        EXPECT(blim_decode(e, &b, emb.data(), rows, 2, hid.data(), nullptr, nullptr) == 0);          // the last layer's pruned rows
        if (dtype != BLIM_COMPUTE_F8) {                                                              // compensated: the w_wrap_k / e2m3 forms of the same launches
            EXPECT(blim_set_option(e, "precise", 1) == 0);
            EXPECT(blim_decode(e, &b, emb.data(), rows, 2, hid.data(), nullptr, nullptr) == 0);
            EXPECT(blim_set_option(e, "precise", 0) == 0);
        }
    }
    for (int v : {3, -1, 1 << 20}) REFUSED(blim_set_option(e, "narrow_gemm", v), BLIM_ERR_ARG, "narrow_gemm");
    EXPECT(blim_set_option(e, "narrow_gemm", 1) == 0);                                               // a refused value left the option as it was: still settable
    REFUSED(blim_set_option(nullptr, "narrow_gemm", 1), BLIM_ERR_ARG, "bad argument");
    blim_destroy(e);
    EXPECT(mock_hip_live_allocations() == 0);
}

static void walk_gemm() {
    const int M = 8, N = 128, K = 128;
    std::vector<uint16_t> a((size_t)M * 2 * K, 0), w((size_t)N * K, 0), c16((size_t)M * 2 * N, 0);
    std::vector<float> c32((size_t)M * N, 0.f), scale(128, 1.f), part((size_t)M * 2, 0.f), ll(M, 0.f), rope((size_t)128 * M, 0.f), bias(N, 0.f);
    std::vector<int32_t> labels(M, 0);
    std::vector<uint8_t> img(1 << 16, 0);
    auto base = [&](int epi, int dtype) {
        blim_gemm_args g;
        memset(&g, 0, sizeof g);
        g.struct_bytes = sizeof g; g.epi = epi; g.dtype = dtype; g.A = a.data(); g.lda = K; g.W = w.data(); g.M = M; g.N = N; g.K = K;
        g.C = (epi == BLIM_EPI_F32 || epi == BLIM_EPI_RESID) ? (void*)c32.data() : (void*)c16.data(); g.ldc = N; g.scale = 1.f; g.f16_saturate = 1;
        if (epi == BLIM_EPI_LSE) { g.C = nullptr; g.ldc = 0; g.labels = labels.data(); g.lse_part = part.data(); g.label_logit = ll.data(); }
        if (epi == BLIM_EPI_QKV) { g.bias = bias.data(); g.rope_rows = rope.data(); g.rope_stride = M; g.rope_cols = 128; }
        return g;
    };
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16}) {
        for (int epi : {BLIM_EPI_BF16, BLIM_EPI_F32, BLIM_EPI_RESID, BLIM_EPI_QKV, BLIM_EPI_SWIGLU, BLIM_EPI_LSE}) {
            blim_gemm_args g = base(epi, dtype);
            for (int tile : {0, 1}) { g.tile = tile; EXPECT(blim_gemm(&g, nullptr) == 0); }          // auto on an ineligible form: no error
            g.tile = 2;
            if (epi == BLIM_EPI_RESID) EXPECT(blim_gemm(&g, nullptr) == 0);
            else REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "epi");
            for (int tile : {3, -1, 1 << 30}) { g.tile = tile; REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "tile"); }
        }
        {   // the residual epilogue's own forms under tile = 2: resid_in, bias, w_wrap_k, lda = 2 K
            blim_gemm_args g = base(BLIM_EPI_RESID, dtype);
            g.tile = 2; g.resid_in = c32.data(); g.bias = bias.data();
            EXPECT(blim_gemm(&g, nullptr) == 0);
            g.lda = 2 * K;
            EXPECT(blim_gemm(&g, nullptr) == 0);
            g.K = 2 * K; g.w_wrap_k = K;
            EXPECT(blim_gemm(&g, nullptr) == 0);
        }
        {   // ... and the e2m3 second pass: refused under 2 (A6 named), taken by the 256 x 256 kernel under 0 and 1
            blim_gemm_args g = base(BLIM_EPI_RESID, dtype);
            g.A6 = img.data(); g.W6 = img.data(); g.K6 = K;
            for (int tile : {0, 1}) { g.tile = tile; EXPECT(blim_gemm(&g, nullptr) == 0); }
            g.tile = 2;
            REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "A6");
            g.A6 = nullptr;
            REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "W6");
        }
    }
    {   // fp8: dtype named; with an MX-scaled A operand as well
        blim_gemm_args g = base(BLIM_EPI_RESID, BLIM_COMPUTE_F8);
        g.row_scale = scale.data(); g.col_scale = scale.data();
        for (int tile : {0, 1}) { g.tile = tile; EXPECT(blim_gemm(&g, nullptr) == 0); }
        g.tile = 2;
        REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "dtype");
        g.row_scale = nullptr; g.a_mx = img.data(); g.mx_stride = 256;
        REFUSED(blim_gemm(&g, nullptr), BLIM_ERR_ARG, "dtype");
    }
    {   // a caller compiled before `tile` existed: the shorter struct reads as tile = 0
        blim_gemm_args g = base(BLIM_EPI_RESID, BLIM_COMPUTE_F16);
        g.tile = 7;
        g.struct_bytes = (int64_t)offsetof(blim_gemm_args, tile);
        EXPECT(blim_gemm(&g, nullptr) == 0);
    }
}

int main() {
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16, BLIM_COMPUTE_F8}) walk_option(dtype);
    walk_gemm();
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("narrow gemm sanitizer drive: ok\n");
    return 0;
}
