// TEST INFRASTRUCTURE (tests/test_prefilter_sanitizers.py): walks the HOST side of blim_score_tvg_first and blim_tvg_rank (blim.h) -- csrc/engine.hip compiled as plain
// C++ against the mock HIP runtime of ../hostmock -- under AddressSanitizer + UBSan.  Kernels do nothing here; what runs is the argument checks, the workspace
// sizing (the [rows | prior_rows] copy into the engine's buffer is a real memcpy under the mock, so a buffer too short for it is an ASan report), and every refusal.
// Exit code 0 = every expectation met.
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

// n sequences of the lengths given, packed one after the other
struct Seqs {
    std::vector<int32_t> pos, seq_start, seq_len, pfx_start, pfx_len, blk_seq, blk_q0;
    std::vector<uint8_t> vis;
    blim_batch b;
    explicit Seqs(const std::vector<int>& lens) {
        int at = 0;
        for (size_t s = 0; s < lens.size(); ++s) {
            seq_start.push_back(at); seq_len.push_back(lens[s]); pfx_start.push_back(0); pfx_len.push_back(0);
            for (int q = 0; q < lens[s]; q += 32) { blk_seq.push_back((int32_t)s); blk_q0.push_back(q); }
            for (int i = 0; i < lens[s]; ++i) { pos.push_back(i); vis.push_back(1); }
            at += lens[s];
        }
        memset(&b, 0, sizeof b);
        b.n_tokens = at; b.n_seqs = (int32_t)lens.size(); b.n_blocks = (int32_t)blk_seq.size();
        b.positions = pos.data(); b.key_visible = vis.data(); b.seq_start = seq_start.data(); b.seq_len = seq_len.data(); b.pfx_start = pfx_start.data(); b.pfx_len = pfx_len.data();
        b.blk_seq = blk_seq.data(); b.blk_q0 = blk_q0.data(); b.own_start = nullptr;
    }
};

static void walk_first(int dtype, int compensated) {
    const blim_config c = cfg_of(dtype);
    blim_engine* e = nullptr;
    EXPECT(blim_create(&c, &e) == 0 && e);
    if (!e) return;
    EXPECT(blim_init_synthetic_weights(e, 3) == 0);
    EXPECT(blim_set_option(e, "precise", compensated) == 0);
    Seqs S({33, 7, 40, 1});                                                            // three prompts and a one-token prior sequence
    std::vector<uint16_t> embeds((size_t)S.b.n_tokens * c.hidden_size * 2, 0);
    const int32_t rows[3] = {32, 39, 79}, prior_rows[2] = {80, 39}, prior_of[3] = {0, -1, 5};
    const int K = 16;
    std::vector<int32_t> idx(3 * K, -7);
    std::vector<float> val(3 * K, 0.f);
    REFUSED(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr), BLIM_ERR_STATE, "no video vocabulary");
    const int N = 1100;
    std::vector<float> vocab((size_t)c.num_clips * N * c.mm_hidden_size, 0.25f);
    EXPECT(blim_set_video_vocab(e, vocab.data(), N, nullptr) == 0);
    std::vector<float> lp((size_t)3 * N, 0.f);
    // ---- the call, from the smallest to one that makes every workspace grow
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 1, nullptr, 0, nullptr, 0.f, 1, idx.data(), val.data(), nullptr, nullptr) == 0);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, K, idx.data(), val.data(), lp.data(), nullptr) == 0);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, prior_rows, 2, prior_of, 0.7f, K, idx.data(), val.data(), lp.data(), nullptr) == 0);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, prior_rows, 2, nullptr, 0.7f, 1024, nullptr, nullptr, nullptr, nullptr) == BLIM_ERR_ARG);
    {
        std::vector<int32_t> many(300), pmany(290);                                   // more rows than one 256-row round of the workspaces
        for (size_t i = 0; i < many.size(); ++i) many[i] = (int32_t)(i % 81);
        for (size_t i = 0; i < pmany.size(); ++i) pmany[i] = (int32_t)((i * 7) % 81);
        std::vector<int32_t> po(300, 289), bi((size_t)300 * 1024);
        std::vector<float> bv((size_t)300 * 1024);
        EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), many.data(), 300, pmany.data(), 290, po.data(), 1.f, 1024, bi.data(), bv.data(), nullptr, nullptr) == 0);
    }
    // ---- refusals: nothing is launched
    EXPECT(blim_score_tvg_first(nullptr, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), nullptr, 3, nullptr, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, K, nullptr, val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, K, idx.data(), nullptr, nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 0, nullptr, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, prior_rows, -1, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 2, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, nullptr, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    EXPECT(blim_score_tvg_first(e, &S.b, nullptr, rows, 3, nullptr, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, nullptr) == BLIM_ERR_ARG);
    REFUSED(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, 0, idx.data(), val.data(), nullptr, nullptr), BLIM_ERR_ARG, "k = 0");
    REFUSED(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, N + 1, idx.data(), val.data(), nullptr, nullptr), BLIM_ERR_ARG, "n_vocab");
    REFUSED(blim_score_tvg_first(e, &S.b, embeds.data(), rows, 3, nullptr, 0, nullptr, 0.f, 1025, idx.data(), val.data(), nullptr, nullptr), BLIM_ERR_ARG, "BLIM_TVG_RANK_MAX_K");
    blim_destroy(e);
    EXPECT(mock_hip_live_allocations() == 0);
}

static void walk_rank() {
    const int N = 70, rows = 2, K = 4;
    std::vector<float> lg((size_t)rows * (N + 3), 0.f), pr((size_t)(N + 3), 0.f), lp((size_t)rows * (N + 3), 0.f), val(rows * K, 0.f);
    std::vector<int32_t> idx(rows * K, 0), po(rows, 0);
    EXPECT(blim_tvg_rank(lg.data(), N + 3, N, rows, nullptr, 0, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr) == 0);
    EXPECT(blim_tvg_rank(lg.data(), N + 3, N, rows, pr.data(), N + 3, 1, po.data(), 0.7f, K, idx.data(), val.data(), lp.data(), N + 3, nullptr) == 0);
    EXPECT(blim_tvg_rank(lg.data(), N + 3, N, rows, pr.data(), N + 3, 0, po.data(), 0.7f, N, idx.data(), val.data(), lp.data(), N, nullptr) == 0);
    REFUSED(blim_tvg_rank(nullptr, N + 3, N, rows, nullptr, 0, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "logits");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, nullptr, 0, 0, nullptr, 0.f, K, nullptr, val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "idx_out");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, nullptr, 0, 0, nullptr, 0.f, K, idx.data(), nullptr, nullptr, 0, nullptr), BLIM_ERR_ARG, "val_out");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, 0, rows, nullptr, 0, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "n_vocab");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, 0, nullptr, 0, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "n_rows");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, nullptr, 0, 0, nullptr, 0.f, 0, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "k = 0");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, nullptr, 0, 0, nullptr, 0.f, N + 1, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "n_vocab");
    REFUSED(blim_tvg_rank(lg.data(), 2000, 2000, rows, nullptr, 0, 0, nullptr, 0.f, 1025, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "BLIM_TVG_RANK_MAX_K");
    REFUSED(blim_tvg_rank(lg.data(), N - 1, N, rows, nullptr, 0, 0, nullptr, 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "ld =");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, pr.data(), N - 1, 1, po.data(), 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "ld_prior");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, nullptr, 0, 0, nullptr, 0.f, K, idx.data(), val.data(), lp.data(), N - 1, nullptr), BLIM_ERR_ARG, "ld_out");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, nullptr, 0, 0, po.data(), 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "prior_of without prior_logits");
    REFUSED(blim_tvg_rank(lg.data(), N + 3, N, rows, pr.data(), N + 3, -1, po.data(), 0.f, K, idx.data(), val.data(), nullptr, 0, nullptr), BLIM_ERR_ARG, "n_prior");
}

int main() {
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16})
        for (int compensated : {0, 1}) walk_first(dtype, compensated);
    walk_rank();
    {   // an fp8 engine is refused whatever else holds
        const blim_config c = cfg_of(BLIM_COMPUTE_F8);
        blim_engine* e = nullptr;
        EXPECT(blim_create(&c, &e) == 0 && e);
        if (e) {
            Seqs S({8});
            std::vector<uint16_t> embeds((size_t)8 * c.hidden_size, 0);
            const int32_t row = 7;
            int32_t idx = 0; float val = 0.f;
            REFUSED(blim_score_tvg_first(e, &S.b, embeds.data(), &row, 1, nullptr, 0, nullptr, 0.f, 1, &idx, &val, nullptr, nullptr), BLIM_ERR_STATE, "fp8");
            blim_destroy(e);
        }
    }
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("prefilter sanitizer drive: ok\n");
    return 0;
}
