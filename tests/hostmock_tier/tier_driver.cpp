// TEST INFRASTRUCTURE (tests/test_host_tier_sanitizers.py): walks the HOST side of slot export / import (blim.h: blim_prefix_cache_record_bytes / _export / _import) --
// csrc/engine.hip compiled as plain C++ against the mock HIP runtime of ../hostmock -- under AddressSanitizer + UBSan.  Kernels do nothing here; what runs is the
// checks of the moves and tickets, the tickets' round trip through a second cache of another layout, the slots' bookkeeping (empty before the work, the ticket's state
// after it: a stale ticket imports and the next cached call refuses its slot), and every refusal.  Exit code 0 = every expectation met.
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

static void walk(int dtype, int compensated) {
    const blim_config c = cfg_of(dtype);
    blim_engine* e = nullptr;
    EXPECT(blim_create(&c, &e) == 0 && e);
    if (!e) return;
    EXPECT(blim_init_synthetic_weights(e, 3) == 0);
    EXPECT(blim_set_option(e, "precise", compensated) == 0);
    blim_prefix_cache *A = nullptr, *B = nullptr;
    EXPECT(blim_prefix_cache_create(e, 4, 64, compensated, &A) == 0 && A);
    EXPECT(blim_prefix_cache_create(e, 6, 96, compensated, &B) == 0 && B);
    if (!A || !B) { blim_destroy(e); return; }
    // ---- record sizes
    const int kv_w = 256 * (1 + compensated), hid_w = c.hidden_size * (1 + compensated);
    for (int len : {1, 31, 64}) {
        const int64_t want = (((int64_t)c.num_layers * len * kv_w + hid_w) * 2 + 255) / 256 * 256;
        EXPECT(blim_prefix_cache_record_bytes(A, len) == want && blim_prefix_cache_record_bytes(B, len) == want);        // the layout does not depend on max_len
    }
    EXPECT(blim_prefix_cache_record_bytes(A, 0) == -1 && blim_prefix_cache_record_bytes(A, 65) == -1 && blim_prefix_cache_record_bytes(nullptr, 8) == -1);
    EXPECT(blim_prefix_cache_record_bytes(B, 65) > 0);
    // ---- fill slots 0, 2, 3 of A (lengths 33, 1, 64); slot 1 stays empty
    const std::vector<int> lens = {33, 1, 64};
    const int32_t slots[3] = {0, 2, 3};
    Prefixes P(lens);
    std::vector<uint16_t> embeds((size_t)P.b.n_tokens * c.hidden_size * 2, 0);
    EXPECT(blim_prefix_cache_fill(e, A, &P.b, embeds.data(), slots, nullptr) == 0);
    EXPECT(blim_prefix_cache_slot_len(A, 0) == 33 && blim_prefix_cache_slot_len(A, 1) == -1 && blim_prefix_cache_slot_len(A, 2) == 1 && blim_prefix_cache_slot_len(A, 3) == 64);
    const int64_t rb = blim_prefix_cache_record_bytes(A, 64);
    const int64_t staging_bytes = 4 * rb;
    void* staging = aligned_alloc(256, (size_t)staging_bytes);
    memset(staging, 0x5A, (size_t)staging_bytes);
    // ---- export, import into B with permuted slots, export again: the tickets agree
    blim_pc_move mv[3] = {{0, 33, 0}, {2, 1, 2 * rb}, {3, 64, rb}};
    blim_pc_ticket tk[3], tk2[3];
    memset(tk, 0, sizeof tk); memset(tk2, 0, sizeof tk2);
    EXPECT(blim_prefix_cache_export(e, A, mv, 3, staging, staging_bytes, tk, nullptr) == 0);
    for (int i = 0; i < 3; ++i) EXPECT(tk[i].magic == BLIM_PC_TICKET_MAGIC && tk[i].len == mv[i].len && tk[i].num_layers == c.num_layers && tk[i].kv_w == kv_w && tk[i].hid_w == hid_w && tk[i].precise == compensated);
    EXPECT(blim_prefix_cache_slot_len(A, 0) == 33);                                   // an export leaves the slot as it is
    blim_pc_move in[3] = {{5, 33, 0}, {0, 1, 2 * rb}, {1, 64, rb}};
    EXPECT(blim_prefix_cache_import(e, B, in, 3, staging, staging_bytes, tk, nullptr) == 0);
    EXPECT(blim_prefix_cache_slot_len(B, 5) == 33 && blim_prefix_cache_slot_len(B, 0) == 1 && blim_prefix_cache_slot_len(B, 1) == 64 && blim_prefix_cache_slot_len(B, 2) == -1);
    EXPECT(blim_prefix_cache_export(e, B, in, 3, staging, staging_bytes, tk2, nullptr) == 0);
    EXPECT(memcmp(tk, tk2, sizeof tk) == 0);
    // ---- more moves than one launch carries
    {
        blim_prefix_cache* W = nullptr;
        EXPECT(blim_prefix_cache_create(e, 49, 32, compensated, &W) == 0 && W);
        if (W) {
            const int64_t r1 = blim_prefix_cache_record_bytes(W, 1);
            std::vector<blim_pc_move> many(49);
            std::vector<blim_pc_ticket> t1(49);
            for (int i = 0; i < 49; ++i) { many[i].slot = i; many[i].len = 1; many[i].offset = i * r1; t1[i] = tk[1]; }
            std::vector<char> wide((size_t)(49 * r1 + 256));
            void* w = (void*)(((uintptr_t)wide.data() + 255) / 256 * 256);
            EXPECT(blim_prefix_cache_import(e, W, many.data(), 49, w, 49 * r1, t1.data(), nullptr) == 0);
            EXPECT(blim_prefix_cache_export(e, W, many.data(), 49, w, 49 * r1, t1.data(), nullptr) == 0);
            REFUSED(blim_prefix_cache_export(e, W, many.data(), 49, w, 49 * r1 - 1, t1.data(), nullptr), BLIM_ERR_ARG, "move 48");
            blim_prefix_cache_destroy(W);
        }
    }
    // ---- refusals shared by the two directions: each names the move
    {
        blim_pc_move m[2] = {{0, 33, 0}, {3, 64, rb}};
        REFUSED(blim_prefix_cache_export(e, A, m, 0, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "at least 1");
        REFUSED(blim_prefix_cache_import(e, A, m, 0, staging, staging_bytes, tk, nullptr), BLIM_ERR_ARG, "at least 1");
        EXPECT(blim_prefix_cache_export(e, A, nullptr, 1, staging, staging_bytes, tk2, nullptr) == BLIM_ERR_ARG);
        EXPECT(blim_prefix_cache_export(e, A, m, 1, nullptr, staging_bytes, tk2, nullptr) == BLIM_ERR_ARG);
        EXPECT(blim_prefix_cache_export(e, A, m, 1, staging, staging_bytes, nullptr, nullptr) == BLIM_ERR_ARG);
        EXPECT(blim_prefix_cache_import(e, A, m, 1, staging, staging_bytes, nullptr, nullptr) == BLIM_ERR_ARG);
        EXPECT(blim_prefix_cache_export(nullptr, A, m, 1, staging, staging_bytes, tk2, nullptr) == BLIM_ERR_ARG);
        blim_pc_move bad[2] = {m[0], m[1]};
        bad[1].slot = 4;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "move 1 outside");
        bad[1].slot = -1;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "outside");
        bad[1] = m[0]; bad[1].offset = rb;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "twice (move 1)");
        bad[1] = m[1]; bad[1].offset = rb + 128;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "multiple of 256");
        bad[1].offset = -256;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "multiple of 256");
        bad[1].offset = 3 * rb + 256;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "does not fit");
        bad[1].offset = 1ll << 40;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "does not fit");
        bad[1].offset = 256;                                                          // inside the record of move 0 (33 positions)
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "overlap");
        bad[0].offset = rb - 256; bad[1].offset = 0;                                  // ... whatever the order of the moves: slot 3's full record at 0 ends at rb
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "moves 1 and 0 overlap");
        bad[0].offset = rb;                                                           // ... and end to end they do not
        EXPECT(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr) == 0);
        REFUSED(blim_prefix_cache_export(e, A, m, 2, (char*)staging + 8, staging_bytes - 8, tk2, nullptr), BLIM_ERR_ARG, "aligned");
        REFUSED(blim_prefix_cache_export(e, A, m, 2, staging, -1, tk2, nullptr), BLIM_ERR_ARG, "staging");
        // ---- export alone
        bad[0] = m[0]; bad[1] = {1, 8, rb};
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_STATE, "never filled");
        bad[1] = m[1]; bad[1].len = 63;
        REFUSED(blim_prefix_cache_export(e, A, bad, 2, staging, staging_bytes, tk2, nullptr), BLIM_ERR_ARG, "filled length");
        EXPECT(blim_prefix_cache_slot_len(A, 0) == 33 && blim_prefix_cache_slot_len(A, 3) == 64);
        // ---- import alone: a refused import leaves its slots as they were
        blim_pc_ticket t[2] = {tk[0], tk[2]};
        t[1].magic = 0;
        REFUSED(blim_prefix_cache_import(e, A, m, 2, staging, staging_bytes, t, nullptr), BLIM_ERR_ARG, "ticket of move 1");
        t[1] = tk[2]; t[1].kv_w += 8;
        REFUSED(blim_prefix_cache_import(e, A, m, 2, staging, staging_bytes, t, nullptr), BLIM_ERR_ARG, "geometry");
        t[1] = tk[2]; t[1].num_layers += 1;
        REFUSED(blim_prefix_cache_import(e, A, m, 2, staging, staging_bytes, t, nullptr), BLIM_ERR_ARG, "geometry");
        t[1] = tk[2]; t[1].hid_w *= 2;
        REFUSED(blim_prefix_cache_import(e, A, m, 2, staging, staging_bytes, t, nullptr), BLIM_ERR_ARG, "geometry");
        t[1] = tk[2]; t[1].n_bits = BLIM_PC_TICKET_LAYERS + 1;
        REFUSED(blim_prefix_cache_import(e, A, m, 2, staging, staging_bytes, t, nullptr), BLIM_ERR_ARG, "geometry");
        t[1] = tk[2]; t[1].len = 63;
        REFUSED(blim_prefix_cache_import(e, A, m, 2, staging, staging_bytes, t, nullptr), BLIM_ERR_ARG, "len 64 of move 1");
        t[1] = tk[2];
        bad[0] = m[0]; bad[1] = m[1]; bad[1].len = 0;
        REFUSED(blim_prefix_cache_import(e, A, bad, 2, staging, staging_bytes, t, nullptr), BLIM_ERR_ARG, "len 0 of move 1");
        blim_pc_move far = {0, 96, 0};                                                // a record of B's longest prefix does not fit a slot of A
        blim_pc_ticket tf = tk[2]; tf.len = 96;
        REFUSED(blim_prefix_cache_import(e, A, &far, 1, staging, 16 * rb, &tf, nullptr), BLIM_ERR_ARG, "does not fit a slot of 64");
        EXPECT(blim_prefix_cache_slot_len(A, 0) == 33 && blim_prefix_cache_slot_len(A, 3) == 64);
        blim_prefix_cache* other = nullptr;                                           // a cache of the other width: another geometry
        EXPECT(blim_prefix_cache_create(e, 2, 64, 1 - compensated, &other) == 0 && other);
        if (other) {
            REFUSED(blim_prefix_cache_import(e, other, m, 1, staging, staging_bytes, tk, nullptr), BLIM_ERR_ARG, "geometry");
            blim_prefix_cache_destroy(other);
        }
    }
    // ---- staleness: a ticket written before a weight change imports with ITS state, and the next cached call naming the slot is refused; a fresh fill is not
    {
        std::vector<float> w((size_t)c.hidden_size, 1.f);
        EXPECT(blim_load_weight(e, "final_norm", w.data(), BLIM_DTYPE_F32, 0) == 0);
        blim_pc_move m = {2, 33, 0};
        EXPECT(blim_prefix_cache_import(e, B, &m, 1, staging, staging_bytes, tk, nullptr) == 0 && blim_prefix_cache_slot_len(B, 2) == 33);
        Prefixes Q({8});
        Q.pfx_len[0] = 33;
        const int32_t used = 2, pfx_slot = 2, rows[2] = {6, 7}, labels[2] = {1, 2}, row_start[2] = {0, 2};
        float score = 0.f;
        std::vector<uint16_t> emb((size_t)8 * c.hidden_size * 2, 0);
        REFUSED(blim_score_vtg_cached(e, B, &Q.b, &pfx_slot, &used, 1, emb.data(), rows, labels, 2, row_start, 1, &score, nullptr), BLIM_ERR_STATE, "stale");
        blim_pc_ticket now;
        EXPECT(blim_prefix_cache_export(e, B, &m, 1, staging, staging_bytes, &now, nullptr) == 0 && now.epoch == tk[0].epoch);      // the ticket's state travelled, not the engine's
        Prefixes R({33});
        const int32_t s2 = 2;
        std::vector<uint16_t> emb2((size_t)33 * c.hidden_size * 2, 0);
        EXPECT(blim_prefix_cache_fill(e, B, &R.b, emb2.data(), &s2, nullptr) == 0);
        EXPECT(blim_score_vtg_cached(e, B, &Q.b, &pfx_slot, &used, 1, emb.data(), rows, labels, 2, row_start, 1, &score, nullptr) == 0);
        EXPECT(blim_prefix_cache_export(e, B, &m, 1, staging, staging_bytes, &now, nullptr) == 0 && now.epoch != tk[0].epoch);
    }
    free(staging);
    blim_prefix_cache_destroy(A);
    blim_prefix_cache_destroy(B);
    blim_destroy(e);
    EXPECT(mock_hip_live_allocations() == 0);
}

int main() {
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16})
        for (int compensated : {0, 1}) walk(dtype, compensated);
    {   // fp8 engines have no prefix cache at all: the entry points are never reached with one
        const blim_config c = cfg_of(BLIM_COMPUTE_F8);
        blim_engine* e = nullptr;
        blim_prefix_cache* pc = nullptr;
        EXPECT(blim_create(&c, &e) == 0 && e);
        if (e) {
            EXPECT(blim_prefix_cache_create(e, 2, 32, 0, &pc) == BLIM_ERR_STATE && !pc);
            blim_destroy(e);
        }
    }
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("host tier sanitizer drive: ok\n");
    return 0;
}
