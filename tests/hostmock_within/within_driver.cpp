// TEST INFRASTRUCTURE (tests/test_within_sanitizers.py): walks the HOST side of blim_score_tvg_first_within and blim_tvg_rank_within (blim.h) -- csrc/engine.hip
// compiled as plain C++ against the mock HIP runtime of ../hostmock -- under AddressSanitizer + UBSan.  Kernels do nothing here; what runs is the argument checks,
// the workspace sizing (the [rows | prior_rows] copy into the engine's buffer is a real memcpy under the mock, so a buffer too short for it is an ASan report),
// and every refusal.  Exit code 0 = every expectation met.
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

static void walk_first_within(int dtype, int compensated) {
    const blim_config c = cfg_of(dtype);
    blim_engine* e = nullptr;
    EXPECT(blim_create(&c, &e) == 0 && e);
    if (!e) return;
    EXPECT(blim_init_synthetic_weights(e, 3) == 0);
    EXPECT(blim_set_option(e, "precise", compensated) == 0);
    Seqs S({33, 7, 40, 1});                                                            // three prompts and a one-token prior sequence
    std::vector<uint16_t> embeds((size_t)S.b.n_tokens * c.hidden_size * 2, 0);
    const int32_t rows[3] = {32, 39, 79}, prior_rows[2] = {80, 39};
    const int32_t row_of[5] = {0, 0, 2, 1, 7}, prior_of[5] = {0, -1, 5, 1, 0};         // five queries on three rows; a row and a prior outside theirs
    const int32_t within[9] = {3, 1, 1099, -1, 1100, 5, 5, 0, 2147483647}, off[6] = {0, 4, 4, 9, 2, 40};
    const int K = 16;
    std::vector<int32_t> idx(5 * K, -7);
    std::vector<float> val(5 * K, 0.f);
#define FW(e_, b_, emb_, rows_, n_rows_, pr_, n_pr_, n_q_, ro_, po_, wi_, wo_, n_w_, k_, idx_, val_) \
    blim_score_tvg_first_within(e_, b_, emb_, rows_, n_rows_, pr_, n_pr_, n_q_, ro_, po_, wi_, wo_, n_w_, 0.7f, k_, idx_, val_, nullptr)
    REFUSED(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()), BLIM_ERR_STATE, "no video vocabulary");
    const int N = 1100;
    std::vector<float> vocab((size_t)c.num_clips * N * c.mm_hidden_size, 0.25f);
    EXPECT(blim_set_video_vocab(e, vocab.data(), N, nullptr) == 0);
    // ---- the call, from one query to more rows than one 256-row round of the workspaces
    EXPECT(FW(e, &S.b, embeds.data(), rows, 1, nullptr, 0, 1, nullptr, nullptr, within, off, 9, 1, idx.data(), val.data()) == 0);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == 0);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 3, prior_rows, 2, 5, row_of, prior_of, within, off, 9, K, idx.data(), val.data()) == 0);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 3, prior_rows, 2, 5, row_of, prior_of, within, off, 0, 1024, idx.data(), val.data()) == 0);   // k above every list, n_within 0: no error
    {
        std::vector<int32_t> many(300), pmany(290), ro(700), po(700, 289), wo(701), wi(5000);
        for (size_t i = 0; i < many.size(); ++i) many[i] = (int32_t)(i % 81);
        for (size_t i = 0; i < pmany.size(); ++i) pmany[i] = (int32_t)((i * 7) % 81);
        for (size_t i = 0; i < ro.size(); ++i) ro[i] = (int32_t)(i % 300);
        for (size_t i = 0; i < wo.size(); ++i) wo[i] = (int32_t)((i * 7) % 5001);
        for (size_t i = 0; i < wi.size(); ++i) wi[i] = (int32_t)(i % N);
        std::vector<int32_t> bi((size_t)700 * 1024);
        std::vector<float> bv((size_t)700 * 1024);
        EXPECT(FW(e, &S.b, embeds.data(), many.data(), 300, pmany.data(), 290, 700, ro.data(), po.data(), wi.data(), wo.data(), 5000, 1024, bi.data(), bv.data()) == 0);
        EXPECT(FW(e, &S.b, embeds.data(), many.data(), 300, nullptr, 0, 700, ro.data(), nullptr, wi.data(), wo.data(), 5000, 1, bi.data(), bv.data()) == 0);
    }
    // ---- refusals: nothing is launched
    EXPECT(FW(nullptr, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == BLIM_ERR_ARG);
    EXPECT(FW(e, &S.b, embeds.data(), nullptr, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == BLIM_ERR_ARG);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, nullptr, val.data()) == BLIM_ERR_ARG);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), nullptr) == BLIM_ERR_ARG);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 0, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == BLIM_ERR_ARG);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 3, prior_rows, -1, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == BLIM_ERR_ARG);
    EXPECT(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 2, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == BLIM_ERR_ARG);
    EXPECT(FW(e, nullptr, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == BLIM_ERR_ARG);
    EXPECT(FW(e, &S.b, nullptr, rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, K, idx.data(), val.data()) == BLIM_ERR_ARG);
    REFUSED(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, nullptr, off, 9, K, idx.data(), val.data()), BLIM_ERR_ARG, "within is null");
    REFUSED(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, nullptr, 9, K, idx.data(), val.data()), BLIM_ERR_ARG, "within_off is null");
    REFUSED(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 0, row_of, nullptr, within, off, 9, K, idx.data(), val.data()), BLIM_ERR_ARG, "n_q = 0");
    REFUSED(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, -1, K, idx.data(), val.data()), BLIM_ERR_ARG, "n_within = -1");
    REFUSED(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, 0, idx.data(), val.data()), BLIM_ERR_ARG, "k = 0");
    REFUSED(FW(e, &S.b, embeds.data(), rows, 3, nullptr, 0, 5, row_of, nullptr, within, off, 9, 1025, idx.data(), val.data()), BLIM_ERR_ARG, "BLIM_TVG_RANK_MAX_K");
#undef FW
    blim_destroy(e);
    EXPECT(mock_hip_live_allocations() == 0);
}

static void walk_rank_within() {
    const int N = 70, rows = 2, K = 4, n_q = 3, n_w = 9;
    std::vector<float> lg((size_t)rows * (N + 3), 0.f), pr((size_t)(N + 3), 0.f), val(n_q * 1024, 0.f);
    std::vector<int32_t> idx(n_q * 1024, 0), po(n_q, 0), ro(n_q, 1), wi(n_w, 5), wo = {0, 3, 3, 9};
#define RW(lg_, ld_, nv_, nr_, pr_, ldp_, np_, nq_, ro_, po_, wi_, wo_, nw_, k_, idx_, val_) \
    blim_tvg_rank_within(lg_, ld_, nv_, nr_, pr_, ldp_, np_, nq_, ro_, po_, wi_, wo_, nw_, 0.7f, k_, idx_, val_, nullptr)
    EXPECT(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, 1, nullptr, nullptr, wi.data(), wo.data(), n_w, 1, idx.data(), val.data()) == 0);
    EXPECT(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, idx.data(), val.data()) == 0);
    EXPECT(RW(lg.data(), N + 3, N, rows, pr.data(), N + 3, 1, n_q, ro.data(), po.data(), wi.data(), wo.data(), n_w, K, idx.data(), val.data()) == 0);
    EXPECT(RW(lg.data(), N + 3, N, rows, pr.data(), N + 3, 0, n_q, nullptr, po.data(), wi.data(), wo.data(), 0, 1024, idx.data(), val.data()) == 0);      // k above every list, n_within 0
    REFUSED(RW(nullptr, N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "logits");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, nullptr, wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "within is null");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), nullptr, n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "within_off is null");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, nullptr, val.data()), BLIM_ERR_ARG, "idx_out");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, idx.data(), nullptr), BLIM_ERR_ARG, "val_out");
    REFUSED(RW(lg.data(), N + 3, 0, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "n_vocab");
    REFUSED(RW(lg.data(), N + 3, N, 0, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "n_rows");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, 0, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "n_q = 0");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), -1, K, idx.data(), val.data()), BLIM_ERR_ARG, "n_within = -1");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, 0, idx.data(), val.data()), BLIM_ERR_ARG, "k = 0");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, 1025, idx.data(), val.data()), BLIM_ERR_ARG, "BLIM_TVG_RANK_MAX_K");
    REFUSED(RW(lg.data(), N - 1, N, rows, nullptr, 0, 0, n_q, ro.data(), nullptr, wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "ld =");
    REFUSED(RW(lg.data(), N + 3, N, rows, pr.data(), N - 1, 1, n_q, ro.data(), po.data(), wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "ld_prior");
    REFUSED(RW(lg.data(), N + 3, N, rows, nullptr, 0, 0, n_q, ro.data(), po.data(), wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "prior_of without prior_logits");
    REFUSED(RW(lg.data(), N + 3, N, rows, pr.data(), N + 3, -1, n_q, ro.data(), po.data(), wi.data(), wo.data(), n_w, K, idx.data(), val.data()), BLIM_ERR_ARG, "n_prior");
#undef RW
}

int main() {
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16})
        for (int compensated : {0, 1}) walk_first_within(dtype, compensated);
    walk_rank_within();
    {   // an fp8 engine is refused whatever else holds
        const blim_config c = cfg_of(BLIM_COMPUTE_F8);
        blim_engine* e = nullptr;
        EXPECT(blim_create(&c, &e) == 0 && e);
        if (e) {
            Seqs S({8});
            std::vector<uint16_t> embeds((size_t)8 * c.hidden_size, 0);
            const int32_t row = 7, wi = 0, wo[2] = {0, 1};
            int32_t idx = 0; float val = 0.f;
            REFUSED(blim_score_tvg_first_within(e, &S.b, embeds.data(), &row, 1, nullptr, 0, 1, nullptr, nullptr, &wi, wo, 1, 0.f, 1, &idx, &val, nullptr), BLIM_ERR_STATE, "fp8");
            blim_destroy(e);
        }
    }
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("within sanitizer drive: ok\n");
    return 0;
}
