// TEST INFRASTRUCTURE (tests/test_caption_prefilter_sanitizers.py): walks the HOST side of blim_tvg_first_cached, blim_tvg_cols and blim_rank_rows (blim.h) --
// csrc/engine.hip compiled as plain C++ against the mock HIP runtime of ../hostmock -- under AddressSanitizer + UBSan.  Kernels do nothing here; what runs is the
// argument checks, the slots' checks, the chunk loop with its workspace sizing (the slot list's copy into the engine's buffer is a real memcpy under the mock, so a
// buffer too short for a chunk is an ASan report), and every refusal.  Exit code 0 = every expectation met.
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

// n prefix sequences of the lengths given, packed one after the other
struct Prefixes {
    std::vector<int32_t> pos, seq_start, seq_len, pfx_start, pfx_len, blk_seq, blk_q0;
    std::vector<uint8_t> vis;
    blim_batch b;
    explicit Prefixes(const std::vector<int>& lens) {
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

static void walk_cached(int dtype, int compensated) {
    const blim_config c = cfg_of(dtype);
    blim_engine* e = nullptr;
    EXPECT(blim_create(&c, &e) == 0 && e);
    if (!e) return;
    EXPECT(blim_init_synthetic_weights(e, 3) == 0);
    EXPECT(blim_set_option(e, "precise", compensated) == 0);
    const int S = 600;                                                               // slots 0 .. 598 are filled, 599 never is
    blim_prefix_cache* pc = nullptr;
    EXPECT(blim_prefix_cache_create(e, S, 32, compensated, &pc) == 0 && pc);
    if (!pc) { blim_destroy(e); return; }
    {
        std::vector<int> lens(S - 1);
        std::vector<int32_t> into(S - 1);
        for (int i = 0; i < S - 1; ++i) { lens[i] = 1 + i % 5; into[i] = i; }
        Prefixes P(lens);
        std::vector<uint16_t> embeds((size_t)P.b.n_tokens * c.hidden_size * 2, 0);
        EXPECT(blim_prefix_cache_fill(e, pc, &P.b, embeds.data(), into.data(), nullptr) == 0);
    }
    const int n_cols = 5;
    const int32_t cols[n_cols] = {3, 0, 3, -1, 1100};                                 // (device data: the host code never reads it)
    std::vector<int32_t> slots(S - 1);
    for (int i = 0; i < S - 1; ++i) slots[i] = (i * 7) % (S - 1);
    std::vector<float> out((size_t)n_cols * S, 0.f);
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_STATE, "no video vocabulary");
    const int N = 1100;
    std::vector<float> vocab((size_t)c.num_clips * N * c.mm_hidden_size, 0.25f);
    EXPECT(blim_set_video_vocab(e, vocab.data(), N, nullptr) == 0);
    // ---- the call, from one slot to several chunks
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), 1, cols, 1, out.data(), 1, 0, nullptr) == 0);
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr) == 0);
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), 256, cols, n_cols, out.data(), S, 256, nullptr) == 0);          // exactly one chunk
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), 257, cols, n_cols, out.data(), S, 256, nullptr) == 0);          // one row into the second
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), S - 1, cols, n_cols, out.data(), S - 1, 256, nullptr) == 0);    // three chunks, the last partly filled
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), S - 1, cols, n_cols, out.data(), S, 0, nullptr) == 0);          // the default: one chunk
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), S - 1, cols, n_cols, out.data(), S, 512, nullptr) == 0);
    // ---- refusals: nothing is launched
    REFUSED(blim_tvg_first_cached(nullptr, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "e is null");
    REFUSED(blim_tvg_first_cached(e, nullptr, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "pc is null");
    REFUSED(blim_tvg_first_cached(e, pc, nullptr, 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "slots is null");
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, nullptr, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "cols is null");
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, nullptr, S, 0, nullptr), BLIM_ERR_ARG, "out is null");
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 0, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "n_slots");
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, 0, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "n_cols");
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), 2, 0, nullptr), BLIM_ERR_ARG, "ld_out");
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), S, 100, nullptr), BLIM_ERR_ARG, "chunk_rows");
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), S, -256, nullptr), BLIM_ERR_ARG, "chunk_rows");
    {
        const int32_t outside[2] = {4, S}, below[2] = {-1, 4}, empty[3] = {4, 8, S - 1};
        REFUSED(blim_tvg_first_cached(e, pc, outside, 2, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "outside 0");
        REFUSED(blim_tvg_first_cached(e, pc, below, 2, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "outside 0");
        REFUSED(blim_tvg_first_cached(e, pc, empty, 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_STATE, "never filled");
        std::vector<int32_t> late(slots);                                            // a bad slot in the LAST chunk is refused before the first is launched
        late[S - 2] = S - 1;
        REFUSED(blim_tvg_first_cached(e, pc, late.data(), S - 1, cols, n_cols, out.data(), S, 256, nullptr), BLIM_ERR_STATE, "never filled");
    }
    {   // a cache of another engine
        blim_engine* e2 = nullptr;
        EXPECT(blim_create(&c, &e2) == 0 && e2);
        if (e2) {
            REFUSED(blim_tvg_first_cached(e2, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_ARG, "another engine");
            blim_destroy(e2);
        }
    }
    {   // an fp8 engine is refused whatever else holds (it cannot own a cache)
        const blim_config c8 = cfg_of(BLIM_COMPUTE_F8);
        blim_engine* e8 = nullptr;
        EXPECT(blim_create(&c8, &e8) == 0 && e8);
        if (e8) {
            REFUSED(blim_tvg_first_cached(e8, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_STATE, "fp8");
            blim_destroy(e8);
        }
    }
    // ---- stale slots: an option the fills recorded changed
    EXPECT(blim_set_option(e, "masked_query_zero", 1) == 0);
    REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_STATE, "stale");
    EXPECT(blim_set_option(e, "masked_query_zero", 0) == 0);
    EXPECT(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr) == 0);
    if (!compensated) {                                                              // a compensated call on a cache created plain: its slots were filled plain
        EXPECT(blim_set_option(e, "precise", 1) == 0);
        REFUSED(blim_tvg_first_cached(e, pc, slots.data(), 3, cols, n_cols, out.data(), S, 0, nullptr), BLIM_ERR_STATE, "option 'precise'");
        EXPECT(blim_set_option(e, "precise", 0) == 0);
    }
    blim_prefix_cache_destroy(pc);
    blim_destroy(e);
    EXPECT(mock_hip_live_allocations() == 0);
}

static void walk_cols() {
    const int N = 70, rows = 2, n_cols = 3;
    std::vector<float> lg((size_t)rows * (N + 3), 0.f), out((size_t)n_cols * 16, 0.f);
    const int32_t cols[n_cols] = {0, 69, -1};
    EXPECT(blim_tvg_cols(lg.data(), N + 3, N, rows, cols, n_cols, out.data(), 16, 0, nullptr) == 0);
    EXPECT(blim_tvg_cols(lg.data(), N, N, rows, cols, n_cols, out.data(), 16, 14, nullptr) == 0);
    EXPECT(blim_tvg_cols(lg.data(), N, 1, 1, cols, 1, out.data(), 1, 0, nullptr) == 0);
    REFUSED(blim_tvg_cols(nullptr, N + 3, N, rows, cols, n_cols, out.data(), 16, 0, nullptr), BLIM_ERR_ARG, "logits is null");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, rows, nullptr, n_cols, out.data(), 16, 0, nullptr), BLIM_ERR_ARG, "cols is null");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, rows, cols, n_cols, nullptr, 16, 0, nullptr), BLIM_ERR_ARG, "out is null");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, 0, rows, cols, n_cols, out.data(), 16, 0, nullptr), BLIM_ERR_ARG, "n_vocab = 0");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, 0, cols, n_cols, out.data(), 16, 0, nullptr), BLIM_ERR_ARG, "n_rows = 0");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, rows, cols, 0, out.data(), 16, 0, nullptr), BLIM_ERR_ARG, "n_cols = 0");
    REFUSED(blim_tvg_cols(lg.data(), N - 1, N, rows, cols, n_cols, out.data(), 16, 0, nullptr), BLIM_ERR_ARG, "ld =");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, rows, cols, n_cols, out.data(), 16, -1, nullptr), BLIM_ERR_ARG, "out0 = -1");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, rows, cols, n_cols, out.data(), 1, 0, nullptr), BLIM_ERR_ARG, "ld_out");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, rows, cols, n_cols, out.data(), 16, 15, nullptr), BLIM_ERR_ARG, "ld_out");
    REFUSED(blim_tvg_cols(lg.data(), N + 3, N, rows, cols, n_cols, out.data(), 16, INT64_MAX, nullptr), BLIM_ERR_ARG, "ld_out");      // (no overflow in the check)
}

static void walk_rank_rows() {
    const int n = 70, rows = 2, K = 4;
    std::vector<float> v((size_t)rows * (n + 3), 0.f), val((size_t)rows * n, 0.f);
    std::vector<int32_t> idx((size_t)rows * n, 0);
    EXPECT(blim_rank_rows(v.data(), n + 3, n, rows, K, idx.data(), val.data(), nullptr) == 0);
    EXPECT(blim_rank_rows(v.data(), n, n, rows, n, idx.data(), val.data(), nullptr) == 0);
    EXPECT(blim_rank_rows(v.data(), 1, 1, 1, 1, idx.data(), val.data(), nullptr) == 0);
    REFUSED(blim_rank_rows(nullptr, n + 3, n, rows, K, idx.data(), val.data(), nullptr), BLIM_ERR_ARG, "values is null");
    REFUSED(blim_rank_rows(v.data(), n + 3, n, rows, K, nullptr, val.data(), nullptr), BLIM_ERR_ARG, "idx_out is null");
    REFUSED(blim_rank_rows(v.data(), n + 3, n, rows, K, idx.data(), nullptr, nullptr), BLIM_ERR_ARG, "val_out is null");
    REFUSED(blim_rank_rows(v.data(), n + 3, 0, rows, K, idx.data(), val.data(), nullptr), BLIM_ERR_ARG, "n = 0");
    REFUSED(blim_rank_rows(v.data(), n + 3, n, 0, K, idx.data(), val.data(), nullptr), BLIM_ERR_ARG, "n_rows = 0");
    REFUSED(blim_rank_rows(v.data(), n + 3, n, rows, 0, idx.data(), val.data(), nullptr), BLIM_ERR_ARG, "tvg_rank: k = 0");
    REFUSED(blim_rank_rows(v.data(), n + 3, n, rows, n + 1, idx.data(), val.data(), nullptr), BLIM_ERR_ARG, "outside 1 .. n_vocab = 70");
    REFUSED(blim_rank_rows(v.data(), 2000, 2000, rows, 1025, idx.data(), val.data(), nullptr), BLIM_ERR_ARG, "BLIM_TVG_RANK_MAX_K");
    REFUSED(blim_rank_rows(v.data(), n - 1, n, rows, K, idx.data(), val.data(), nullptr), BLIM_ERR_ARG, "ld =");
}

int main() {
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16})
        for (int compensated : {0, 1}) walk_cached(dtype, compensated);
    walk_cols();
    walk_rank_rows();
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("caption prefilter sanitizer drive: ok\n");
    return 0;
}
