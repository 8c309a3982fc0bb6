// TEST INFRASTRUCTURE (tests/test_launch_trace_host.py): records WHICH launches the engine's host code makes, with WHICH arguments, in every numeric mode -- the
// proof that a change to csrc/engine.hip's host code (run_layers, the heads, the projector) left every launch as it was.  csrc/engine.hip, adapters.hip and train.hip
// are compiled as plain C++ against the mock HIP runtime of ../hostmock; the launchers the decoder and the heads call are defined HERE (not by the generated
// do-nothing file) and write one line per call: the launcher's name and every argument, GemmParams / AttnParams field by field.  Pointers are written free of
// addresses: alloc<k>+<byte offset> with k the creation rank of the mock allocation counted from the engine's first one, or the name of a buffer of this driver.
// After each entry-point call the timing record's calls and flops per class follow (the mock's events make the times meaningless).
// Output format (stdout): "engine ..." lines as they are; "state <label> : state <k>" opens a state, "state <label> == state <k>" stands for a state whose calls and
// their lines are those of state k; per entry-point call "call <name> : block <k>" followed by the call's lines, or
// "call <name> == block <k>" when the very same lines were written before as block k.  Inside a block a line seen for the first time is "<n>| <text>" with n counting
// the distinct lines, repeated lines are written by number, a run of them on one line as "= <n> <a>-<b> ..." (a-b: the lines a to b in order).  Pointers at offset 0
// drop the "+0"; a dtype equal to the engine's 16-bit compute dtype (the "c=" of its engine line) is written as "c", so fp16 and bf16 engines share their lines.
// The recorded output of this program is tests/golden/launch_trace.txt.  Exit code 0 = every call succeeded and every pointer could be named.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/blim.h"
#include "engine.hpp"

extern "C" size_t mock_hip_live_allocations();
extern "C" long mock_hip_alloc_rank(const void* p, size_t* offset);
extern "C" long mock_hip_allocations_created();

static int failures = 0;

#define EXPECT(cond)                                                                              \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "EXPECT failed: %s (%s:%d) last error: %s\n", #cond, __FILE__, __LINE__, blim_last_error()); ++failures; } \
    } while (0)

// ---------------------------------------------------------------------------- output: every distinct line once
static std::map<std::string, int> seen_lines;
static std::vector<int> pending;      // repeated lines not yet written
static void flush_refs() {
    if (pending.empty()) return;
    printf("=");
    for (size_t i = 0; i < pending.size();) {
        size_t j = i;
        while (j + 1 < pending.size() && pending[j + 1] == pending[j] + 1) ++j;
        if (j > i) printf(" %d-%d", pending[i], pending[j]); else printf(" %d", pending[i]);
        i = j + 1;
    }
    printf("\n");
    pending.clear();
}
static void out_line(const std::string& s) {
    auto it = seen_lines.find(s);
    if (it != seen_lines.end()) { pending.push_back(it->second); return; }
    flush_refs();
    const int n = (int)seen_lines.size() + 1;
    seen_lines[s] = n;
    printf("%d| %s\n", n, s.c_str());
}
// the lines of one entry-point call are collected and written as a block; a call whose block was written before only names it.  Likewise a state whose calls are,
// block for block, those of a state written before only names that state
static bool in_call = false;
static std::vector<std::string> block;
static std::map<std::string, int> seen_blocks, seen_states;
static std::string state_label;
static std::vector<std::pair<std::string, std::vector<std::string>>> state_calls;
static void end_state() {
    if (state_label.empty()) return;
    std::string key;
    for (const auto& c : state_calls) { key += "call " + c.first + "\n"; for (const std::string& l : c.second) { key += l; key += '\n'; } }
    auto st = seen_states.find(key);
    if (st != seen_states.end()) { printf("%s == state %d\n", state_label.c_str(), st->second); state_label.clear(); state_calls.clear(); return; }
    const int sn = (int)seen_states.size() + 1;
    seen_states[key] = sn;
    printf("%s : state %d\n", state_label.c_str(), sn);
    for (const auto& c : state_calls) {
        std::string bkey;
        for (const std::string& l : c.second) { bkey += l; bkey += '\n'; }
        auto it = seen_blocks.find(bkey);
        if (it != seen_blocks.end()) { printf("call %s == block %d\n", c.first.c_str(), it->second); continue; }
        const int n = (int)seen_blocks.size() + 1;
        seen_blocks[bkey] = n;
        printf("call %s : block %d\n", c.first.c_str(), n);
        for (const std::string& l : c.second) out_line(l);
        flush_refs();
    }
    state_label.clear(); state_calls.clear();
}
static void emit(const std::string& s) {
    if (in_call) { block.push_back(s); return; }
    end_state();
    if (!s.compare(0, 6, "state ")) { state_label = s; return; }
    if (s.compare(0, 7, "engine ")) { fprintf(stderr, "a launch outside a traced call: %s\n", s.c_str()); ++failures; }
    printf("%s\n", s.c_str());
}
static void begin_call() { in_call = true; block.clear(); }
static void end_call(const char* name) {
    in_call = false;
    if (state_label.empty()) { fprintf(stderr, "call %s outside a state\n", name); ++failures; }
    state_calls.emplace_back(name, block);
}
struct Line {
    std::string s;
    explicit Line(const char* name) : s(name) {}
    ~Line() { emit(s); }
    Line& f(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char buf[256];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        s += ' '; s += buf;
        return *this;
    }
};

// ---------------------------------------------------------------------------- pointers without addresses
struct HostBuf { const char* p; size_t bytes; const char* name; };
static std::vector<HostBuf> host_bufs;
static long rank_base = 0;      // the creation rank of the present engine's first allocation
template <typename T> static void name_buf(const std::vector<T>& v, const char* name) { host_bufs.push_back({(const char*)v.data(), v.size() * sizeof(T), name}); }
static std::string ptr(const void* p) {
    if (!p) return "0";
    char buf[96];
    size_t off = 0;
    const long r = mock_hip_alloc_rank(p, &off);
    if (r >= 0) { if (off) snprintf(buf, sizeof buf, "alloc%ld+%zu", r - rank_base, off); else snprintf(buf, sizeof buf, "alloc%ld", r - rank_base); return buf; }
    for (const HostBuf& h : host_bufs)
        if ((const char*)p >= h.p && (const char*)p < h.p + h.bytes) {
            if ((const char*)p == h.p) return h.name;
            snprintf(buf, sizeof buf, "%s+%zu", h.name, (size_t)((const char*)p - h.p));
            return buf;
        }
    fprintf(stderr, "a pointer that is neither a mock allocation nor a named buffer of the driver\n");
    ++failures;
    return "?";
}
#define PS(x) ptr(x).c_str()
static int engine_dt = -1;      // the present engine's 16-bit compute dtype
static std::string dts(int d) { return d == engine_dt ? "c" : std::to_string(d); }
#define DT(x) dts(x).c_str()

// ---------------------------------------------------------------------------- the traced launchers
static const char* epi_name(GemmEpi e) { static const char* n[] = {"bf16", "f32", "resid", "qkv", "swiglu", "lse"}; return n[(int)e]; }
static const char* kGemmDefaults =
    "# launch_gemm lines: epilogue dtype (c = the engine's compute dtype) A lda W M N K C ldc always; every other GemmParams field only where it differs from gp()'s defaults: row_scale=0 col_scale=0 "
    "bias=0 resid_in=0 swiglu_gu=0 swiglu_ld=0 swiglu_act=0 swiglu_act_ld=0 act=0 scale=1 rope_cols=0 rope_rows=0 rope_stride=0 labels=0 lse_part=0 label_logit=0 "
    "w_wrap_k=0 lo_off=0 out_mx=0 a_mx=0 mx_stride=0 A6=0 W6=0 K6=0 out6=0 f16_saturate=1 group_m=0 tile_map=0 debug_skip_epilogue=0 debug_stamps=0 narrow=0 "
    "narrow_lo6=0 narrow_qkv=0.  launch_rmsnorm: rows=0 out_f32=0 n_src=0 ldo=0 out_lo=0 saturate=1 out6=0 are left out; launch_attention[_cached]: own_start=0 v_lo_off=0 "
    "out_lo_off=0 out8=0 ldo8=0 out_mx=0 mx_stride=0 lse_out=0 are left out";
int launch_gemm(GemmEpi epi, const GemmParams& p, hipStream_t) {
    Line l("launch_gemm");
    l.f("%s dtype=%s A=%s lda=%lld W=%s M=%d N=%d K=%d C=%s ldc=%lld", epi_name(epi), DT(p.dtype), PS(p.A), (long long)p.lda, PS(p.W), p.M, p.N, p.K, PS(p.C), (long long)p.ldc);
#define FP(field) if (p.field) l.f(#field "=%s", PS(p.field))
#define FI(field) if (p.field) l.f(#field "=%lld", (long long)p.field)
    FP(row_scale); FP(col_scale); FP(bias); FP(resid_in); FP(swiglu_gu); FI(swiglu_ld); FP(swiglu_act); FI(swiglu_act_ld); FI(act);
    if (p.scale != 1.0f) l.f("scale=%.9g", p.scale);
    FI(rope_cols); FP(rope_rows); FI(rope_stride); FP(labels); FP(lse_part); FP(label_logit); FI(w_wrap_k); FI(lo_off); FP(out_mx); FP(a_mx); FI(mx_stride);
    FP(A6); FP(W6); FI(K6); FP(out6);
    if (p.f16_saturate != 1) l.f("f16_saturate=%d", p.f16_saturate);
    FI(group_m); FI(tile_map); FI(debug_skip_epilogue); FP(debug_stamps); FI(narrow); FI(narrow_lo6); FI(narrow_qkv);
#undef FP
#undef FI
    return BLIM_OK;
}
int launch_rmsnorm(const float* x, int64_t ldx, const int32_t* rows, int64_t n_rows, int H, const float* w, float eps, bf16_t* out_h16, int dtype, float* out_f32, hipStream_t,
                   int64_t n_src, int64_t ldo, bf16_t* out_lo, bool saturate, uint8_t* out6) {
    Line l("launch_rmsnorm");
    l.f("x=%s ldx=%lld n_rows=%lld H=%d w=%s eps=%g out_h16=%s dtype=%s", PS(x), (long long)ldx, (long long)n_rows, H, PS(w), eps, PS(out_h16), DT(dtype));
    if (rows) l.f("rows=%s", PS(rows));
    if (out_f32) l.f("out_f32=%s", PS(out_f32));
    if (n_src) l.f("n_src=%lld", (long long)n_src);
    if (ldo) l.f("ldo=%lld", (long long)ldo);
    if (out_lo) l.f("out_lo=%s", PS(out_lo));
    if (!saturate) l.f("saturate=0");
    if (out6) l.f("out6=%s", PS(out6));
    return BLIM_OK;
}
int launch_rmsnorm_f8(const float* x, int64_t ldx, int64_t n_rows, int H, const float* w, float eps, uint8_t* out8, float* scale, hipStream_t) {
    Line("launch_rmsnorm_f8").f("x=%s ldx=%lld n_rows=%lld H=%d w=%s eps=%g out8=%s scale=%s", PS(x), (long long)ldx, (long long)n_rows, H, PS(w), eps, PS(out8), PS(scale));
    return BLIM_OK;
}
static void attn_fields(Line& l, const AttnParams& p) {
    l.f("dtype=%s qkv=%s ldq=%lld num_heads=%d num_kv_heads=%d key_visible=%s seq_start=%s seq_len=%s pfx_start=%s pfx_len=%s blk_seq=%s blk_q0=%s n_blocks=%d", DT(p.dtype),
        PS(p.qkv), (long long)p.ldq, p.num_heads, p.num_kv_heads, PS(p.key_visible), PS(p.seq_start), PS(p.seq_len), PS(p.pfx_start), PS(p.pfx_len), PS(p.blk_seq), PS(p.blk_q0),
        p.n_blocks);
    if (p.own_start) l.f("own_start=%s", PS(p.own_start));
    l.f("out=%s ldo=%lld scale=%.9g", PS(p.out), (long long)p.ldo, p.scale);
    if (p.v_lo_off) l.f("v_lo_off=%lld", (long long)p.v_lo_off);
    if (p.out_lo_off) l.f("out_lo_off=%lld", (long long)p.out_lo_off);
    if (p.out8) l.f("out8=%s", PS(p.out8));
    if (p.ldo8) l.f("ldo8=%lld", (long long)p.ldo8);
    if (p.out_mx) l.f("out_mx=%s", PS(p.out_mx));
    if (p.mx_stride) l.f("mx_stride=%lld", (long long)p.mx_stride);
    if (p.lse_out) l.f("lse_out=%s", PS(p.lse_out));
}
int launch_attention(const AttnParams& p, int use_tr_read, hipStream_t) {
    Line l("launch_attention");
    attn_fields(l, p);
    l.f("use_tr_read=%d", use_tr_read);
    return BLIM_OK;
}
int launch_attention_cached(const AttnPcParams& p, hipStream_t) {
    Line l("launch_attention_cached");
    attn_fields(l, p);
    l.f("pfx_cache=%s pfx_slot=%s pc_slot_stride=%lld pc_ld=%lld pc_lo_off=%lld pc_n_slots=%d pc_max_len=%d", PS(p.pfx_cache), PS(p.pfx_slot), (long long)p.pc_slot_stride, (long long)p.pc_ld,
        (long long)p.pc_lo_off, p.pc_n_slots, p.pc_max_len);
    return BLIM_OK;
}
int launch_f6_tiles(const bf16_t* in, int64_t ld, int64_t n_rows, int K, int dtype, bool w_side, uint8_t* out, hipStream_t) {
    Line("launch_f6_tiles").f("in=%s ld=%lld n_rows=%lld K=%d dtype=%s w_side=%d out=%s", PS(in), (long long)ld, (long long)n_rows, K, DT(dtype), (int)w_side, PS(out));
    return BLIM_OK;
}
int launch_quant_rows(const bf16_t* in, int64_t ld, int64_t n_rows, int K, int dtype, uint8_t* out8, float* scale, hipStream_t) {
    Line("launch_quant_rows").f("in=%s ld=%lld n_rows=%lld K=%d dtype=%s out8=%s scale=%s", PS(in), (long long)ld, (long long)n_rows, K, DT(dtype), PS(out8), PS(scale));
    return BLIM_OK;
}
int launch_gather_rows(void* dst, const void* src, const int32_t* rows, int64_t n_rows, int64_t row_bytes, int64_t n_src, uint32_t fill, hipStream_t) {
    Line("launch_gather_rows").f("dst=%s src=%s rows=%s n_rows=%lld row_bytes=%lld n_src=%lld fill=%#x", PS(dst), PS(src), PS(rows), (long long)n_rows, (long long)row_bytes, (long long)n_src, fill);
    return BLIM_OK;
}
int launch_kv_capture(const bf16_t* qkv, int64_t ldq, int64_t col, int64_t src_lo_off, int width, const int32_t* dst_row, int64_t n_tokens, bf16_t* cache, int64_t slot_stride, int64_t ld,
                      int64_t dst_lo_off, int max_len, int n_slots, hipStream_t) {
    Line("launch_kv_capture").f("qkv=%s ldq=%lld col=%lld src_lo_off=%lld width=%d dst_row=%s n_tokens=%lld cache=%s slot_stride=%lld ld=%lld dst_lo_off=%lld max_len=%d n_slots=%d", PS(qkv),
                                (long long)ldq, (long long)col, (long long)src_lo_off, width, PS(dst_row), (long long)n_tokens, PS(cache), (long long)slot_stride, (long long)ld,
                                (long long)dst_lo_off, max_len, n_slots);
    return BLIM_OK;
}
int launch_zero_rows(bf16_t* x, int64_t ld, const uint8_t* keep, int64_t n_rows, int width, hipStream_t) {
    Line("launch_zero_rows").f("x=%s ld=%lld keep=%s n_rows=%lld width=%d", PS(x), (long long)ld, PS(keep), (long long)n_rows, width);
    return BLIM_OK;
}
int launch_rows_by_index(uint16_t* dst, int64_t ld_dst, const uint16_t* src, int64_t ld_src, const int32_t* idx, int64_t n_rows, int width, int64_t n_bound, int gather, uint16_t fill,
                         hipStream_t) {
    Line("launch_rows_by_index").f("dst=%s ld_dst=%lld src=%s ld_src=%lld idx=%s n_rows=%lld width=%d n_bound=%lld gather=%d fill=%#x", PS(dst), (long long)ld_dst, PS(src), (long long)ld_src,
                                   PS(idx), (long long)n_rows, width, (long long)n_bound, gather, (unsigned)fill);
    return BLIM_OK;
}
int launch_lse_combine(const float2* part, int n_tiles, const float* label_logit, const int32_t* labels, int64_t n_rows, float* logprob, hipStream_t) {
    Line("launch_lse_combine").f("part=%s n_tiles=%d label_logit=%s labels=%s n_rows=%lld logprob=%s", PS(part), n_tiles, PS(label_logit), PS(labels), (long long)n_rows, PS(logprob));
    return BLIM_OK;
}
int launch_h16_to_f32(float* out, const bf16_t* in, int64_t n, int dtype, hipStream_t) {
    Line("launch_h16_to_f32").f("out=%s in=%s n=%lld dtype=%s", PS(out), PS(in), (long long)n, DT(dtype));
    return BLIM_OK;
}
int launch_hilo_to_f32(float* out, const bf16_t* in, int64_t n_rows, int H, int dtype, hipStream_t) {
    Line("launch_hilo_to_f32").f("out=%s in=%s n_rows=%lld H=%d dtype=%s", PS(out), PS(in), (long long)n_rows, H, DT(dtype));
    return BLIM_OK;
}

// ---------------------------------------------------------------------------- the walk
static const int L = 40, H = 384, I = 512, LAYERS = 3;      // hidden 384: the RMSNorm kernels write e2m3 tiles for 256 < H only (kernels.hpp: rmsnorm_can_write_tiles)
static blim_config cfg_of(int dtype) {
    blim_config c;
    memset(&c, 0, sizeof c);
    c.vocab_size = 1024; c.hidden_size = H; c.intermediate_size = I; c.num_layers = LAYERS; c.num_heads = 3; c.num_kv_heads = 1;
    c.mm_hidden_size = 64; c.num_clips = 4; c.max_positions = 128; c.compute_dtype = dtype; c.rms_eps = 1e-6f; c.rope_theta = 1e6f;
    return c;
}

// sequences of the lengths given, packed one after the other; sequence s > 0 may take sequence 0 as its in-batch prefix
struct Batch {
    std::vector<int32_t> pos, seq_start, seq_len, pfx_start, pfx_len, blk_seq, blk_q0;
    std::vector<uint8_t> vis;
    blim_batch b;
    explicit Batch(const std::vector<int>& lens) {
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
    void name(const char* const n[8]) {
        name_buf(pos, n[0]); name_buf(seq_start, n[1]); name_buf(seq_len, n[2]); name_buf(pfx_start, n[3]); name_buf(pfx_len, n[4]); name_buf(blk_seq, n[5]); name_buf(blk_q0, n[6]); name_buf(vis, n[7]);
    }
};

// the driver's own buffers, each named once
struct Buffers {
    Batch B{{L}}, P{{33}}, Q{{8}}, R{{33, 8}};      // the batch of every state; a gallery prefix; its continuation over the cached prefix; prefix + continuation in one batch
    std::vector<uint16_t> embeds, hid, feats, proj, vocab16;
    std::vector<float> f32, scores, logits, vocab_f32;
    std::vector<uint8_t> mask;
    std::vector<int32_t> rows38, rows39, vrows, vlabels, vrow_start, trows, tlabels, slot0, pfx_slot, used, crows, clabels, crow_start, arows, alabels, arow_start, apfx_slot;
    Buffers() : embeds((size_t)64 * H * 2, 0), hid((size_t)64 * (H + 128) * 2, 0), feats((size_t)64 * 64, 0), proj((size_t)64 * H * 2, 0), vocab16((size_t)16 * 4 * 64, 0),
                f32((size_t)64 * H, 0.f), scores(16, 0.f), logits((size_t)L * 1024, 0.f), vocab_f32((size_t)16 * 4 * 64, 0.f), mask(L, 1) {
        for (int i = 0; i < 39; ++i) { rows39.push_back(i); if (i < 38) rows38.push_back(i + 2); }
        vrows = {30, 31, 38, 39}; vlabels = {7, 8, 9, 10}; vrow_start = {0, 2, 4};
        trows = {28, 29, 30, 31, 36, 37, 38, 39}; tlabels = {1, 2};
        slot0 = {0}; pfx_slot = {0}; used = {0};
        Q.pfx_len[0] = 33; crows = {6, 7}; clabels = {1, 2}; crow_start = {0, 2};
        R.pfx_len[1] = 33; arows = {32, 39, 40}; alabels = {1, 2, 3}; arow_start = {0, 3}; apfx_slot = {-1, -1};
        static const char* const nb[8] = {"B.pos", "B.seq_start", "B.seq_len", "B.pfx_start", "B.pfx_len", "B.blk_seq", "B.blk_q0", "B.vis"};
        static const char* const np[8] = {"P.pos", "P.seq_start", "P.seq_len", "P.pfx_start", "P.pfx_len", "P.blk_seq", "P.blk_q0", "P.vis"};
        static const char* const nq[8] = {"Q.pos", "Q.seq_start", "Q.seq_len", "Q.pfx_start", "Q.pfx_len", "Q.blk_seq", "Q.blk_q0", "Q.vis"};
        static const char* const nr[8] = {"R.pos", "R.seq_start", "R.seq_len", "R.pfx_start", "R.pfx_len", "R.blk_seq", "R.blk_q0", "R.vis"};
        B.name(nb); P.name(np); Q.name(nq); R.name(nr);
        name_buf(embeds, "embeds"); name_buf(hid, "hid"); name_buf(feats, "feats"); name_buf(proj, "proj"); name_buf(vocab16, "vocab16"); name_buf(f32, "f32"); name_buf(scores, "scores");
        name_buf(logits, "logits"); name_buf(vocab_f32, "vocab_f32"); name_buf(mask, "mask"); name_buf(rows38, "rows38"); name_buf(rows39, "rows39"); name_buf(vrows, "vrows");
        name_buf(vlabels, "vlabels"); name_buf(vrow_start, "vrow_start"); name_buf(trows, "trows"); name_buf(tlabels, "tlabels"); name_buf(slot0, "slot0"); name_buf(pfx_slot, "pfx_slot");
        name_buf(used, "used"); name_buf(crows, "crows"); name_buf(clabels, "clabels"); name_buf(crow_start, "crow_start"); name_buf(arows, "arows"); name_buf(alabels, "alabels");
        name_buf(arow_start, "arow_start"); name_buf(apfx_slot, "apfx_slot");
    }
};
static Buffers* X;

// after an entry-point call: the timing record's launches and flops per class
static void report(blim_engine* e, const char* call, int rc) {
    const int n = blim_timing_num_classes();
    std::vector<double> ms(n), fl(n);
    std::vector<int64_t> calls(n);
    EXPECT(rc == 0);
    EXPECT(blim_timing_report(e, ms.data(), calls.data(), fl.data()) == 0);
    {
        Line l("timing");      // per class with launches: calls / flops
        l.f("rc=%d", rc);
        for (int i = 0; i < n; ++i) if (calls[i]) l.f("%s=%lld/%.0f", blim_timing_class_name(i), (long long)calls[i], fl[i]);
    }
    end_call(call);
}
#define CALL(name, expr) do { begin_call(); report(e, name, (expr)); } while (0)

static void calls_of_state(blim_engine* e, const std::string& state, bool with_cache, int compensated) {
    emit("state " + state);
    Buffers& x = *X;
    CALL("blim_project_video 0", blim_project_video(e, x.feats.data(), 64, 0, x.proj.data(), nullptr));
    CALL("blim_project_video 1", blim_project_video(e, x.feats.data(), 64, 1, x.proj.data(), nullptr));
    CALL("blim_decode all rows", blim_decode(e, &x.B.b, x.embeds.data(), nullptr, 0, x.hid.data(), x.f32.data(), nullptr));
    CALL("blim_decode 38 rows", blim_decode(e, &x.B.b, x.embeds.data(), x.rows38.data(), 38, x.hid.data(), nullptr, nullptr));
    CALL("blim_decode 39 rows", blim_decode(e, &x.B.b, x.embeds.data(), x.rows39.data(), 39, x.hid.data(), nullptr, nullptr));
    CALL("blim_set_video_vocab", blim_set_video_vocab(e, x.vocab_f32.data(), 16, nullptr));
    CALL("blim_score_vtg", blim_score_vtg(e, &x.B.b, x.embeds.data(), x.vrows.data(), x.vlabels.data(), 4, x.vrow_start.data(), 2, x.scores.data(), nullptr));
    CALL("blim_score_tvg", blim_score_tvg(e, &x.B.b, x.embeds.data(), x.trows.data(), nullptr, 16, x.tlabels.data(), 2, x.scores.data(), nullptr));
    CALL("blim_forward", blim_forward(e, x.embeds.data(), x.mask.data(), 1, L, x.logits.data(), x.f32.data(), nullptr));
    if (!with_cache) return;
    blim_prefix_cache* pc = nullptr;
    EXPECT(blim_prefix_cache_create(e, 2, 64, compensated, &pc) == 0 && pc);
    if (!pc) return;
    CALL("blim_prefix_cache_fill", blim_prefix_cache_fill(e, pc, &x.P.b, x.embeds.data(), x.slot0.data(), nullptr));
    CALL("blim_score_vtg_cached", blim_score_vtg_cached(e, pc, &x.Q.b, x.pfx_slot.data(), x.used.data(), 1, x.embeds.data(), x.crows.data(), x.clabels.data(), 2, x.crow_start.data(), 1,
                                                        x.scores.data(), nullptr));
    const blim_pc_admit adm = {0, 1, 0, 33, 0};
    CALL("blim_score_vtg_admit", blim_score_vtg_admit(e, pc, &x.R.b, x.apfx_slot.data(), x.used.data(), 0, &adm, 1, x.embeds.data(), x.arows.data(), x.alabels.data(), 3, x.arow_start.data(), 1,
                                                      x.scores.data(), nullptr));
    blim_prefix_cache_destroy(pc);
}

// every workspace at its largest size before the first traced call (and again once adapters widen the rows): the allocation ranks the trace prints then stay the same
// from state to state, and a line that recurs is written once
static void reserve_all(blim_engine* e, bool can_precise) {
    if (can_precise) EXPECT(blim_set_option(e, "precise", 1) == 0);
    emit("state reserve");
    begin_call();      // (with "precise_lo6" on, the e2m3 images of the weights are built here)
    EXPECT(blim_reserve(e, 64, 64) == 0);
    end_call("blim_reserve");
    if (can_precise) EXPECT(blim_set_option(e, "precise", 0) == 0);
}
static void load_adapters(blim_engine* e, int r) {
    std::vector<float> A((size_t)16 * H, 0.01f), Bm((size_t)1024 * 16, 0.02f);
    for (int l = 0; l < LAYERS; ++l)
        for (const char* t : {"q_proj.w", "k_proj.w", "v_proj.w", "o_proj.w"}) EXPECT(blim_load_adapter(e, ("layers." + std::to_string(l) + "." + t).c_str(), A.data(), Bm.data(), r, 32.f) == 0);
    for (const char* n : {"lm_head", "mlp.0.w", "mlp.2.w", "tvg_mlp.0.w", "tvg_mlp.2.w"}) EXPECT(blim_load_adapter(e, n, A.data(), Bm.data(), r, 32.f) == 0);
}

static blim_engine* new_engine(int dtype, int lo6, const char* label) {
    const blim_config c = cfg_of(dtype);
    blim_engine* e = nullptr;
    rank_base = mock_hip_allocations_created();
    EXPECT(blim_create(&c, &e) == 0 && e);
    if (!e) return nullptr;
    engine_dt = dtype == BLIM_COMPUTE_F8 ? BLIM_COMPUTE_F16 : dtype;
    emit(std::string("engine ") + label + " c=" + std::to_string(engine_dt));
    EXPECT(blim_init_synthetic_weights(e, 3) == 0);
    if (dtype != BLIM_COMPUTE_F8) EXPECT(blim_set_option(e, "precise_lo6", lo6) == 0);
    EXPECT(blim_timing_enable(e, 1) == 0);
    reserve_all(e, dtype != BLIM_COMPUTE_F8);
    return e;
}
static void set_bits(blim_engine* e, const int bits[LAYERS]) {
    for (int l = 0; l < LAYERS; ++l) EXPECT(blim_set_option(e, "precise_layer_bits", (l << 4) | bits[l]) == 0);
}
// per-layer masks of the three layers: together every bit, and the combinations 12 (gate|up + down), 3, 5, 10
static const int kBits[2][LAYERS] = {{12, 3, 5}, {10, 6, 9}};

// the compensated states of one 16-bit engine: A = "precise" with precise_mlp 0 / 1, B = "precise_layers" under two mask patterns; embeds: the values of "precise_embeds"
static void compensated_states(blim_engine* e, const std::string& tag, const std::vector<int>& embeds, bool cache_on_first) {
    bool first = true;
    for (int pe : embeds) {
        EXPECT(blim_set_option(e, "precise", 1) == 0 && blim_set_option(e, "precise_embeds", pe) == 0);
        for (int mlp : {0, 1}) {
            EXPECT(blim_set_option(e, "precise_mlp", mlp) == 0);
            calls_of_state(e, tag + " precise precise_mlp=" + std::to_string(mlp) + " precise_embeds=" + std::to_string(pe), cache_on_first && first && mlp == 1, 1);
            if (mlp == 1) first = false;
        }
        EXPECT(blim_set_option(e, "precise_layers", 1) == 0);
        for (int k = 0; k < 2; ++k) {
            set_bits(e, kBits[k]);
            calls_of_state(e, tag + " precise_layers pattern=" + std::to_string(k) + " precise_embeds=" + std::to_string(pe), false, 1);
        }
        EXPECT(blim_set_option(e, "precise_layers", 0) == 0);
    }
    EXPECT(blim_set_option(e, "precise", 0) == 0 && blim_set_option(e, "precise_embeds", 0) == 0);
}

static void walk_16bit(int dtype) {
    const std::string dt = dtype == BLIM_COMPUTE_F16 ? "fp16" : "bf16";
    static int rank_turn = 0;
    const int ranks[3] = {4, 8, 16};
    {   // the 16-bit second pass (w_wrap_k): plain, compensated, then the same with adapters apart
        unsetenv("BLIM_LO6_FUSED_MASK");
        blim_engine* e = new_engine(dtype, 0, (dt + " lo6=0").c_str());
        if (!e) return;
        calls_of_state(e, dt + " plain", true, 0);
        compensated_states(e, dt, {0}, true);
        EXPECT(blim_set_option(e, "masked_query_zero", 1) == 0);
        if (dtype == BLIM_COMPUTE_F16) calls_of_state(e, dt + " plain masked_query_zero", false, 0);
        EXPECT(blim_set_option(e, "masked_query_zero", 0) == 0);
        for (const char* k : {"narrow_gemm", "narrow_lo6", "narrow_qkv"}) EXPECT(blim_set_option(e, k, 2) == 0);
        if (dtype == BLIM_COMPUTE_F16) calls_of_state(e, dt + " plain narrow=2", false, 0);
        for (const char* k : {"narrow_gemm", "narrow_lo6", "narrow_qkv"}) EXPECT(blim_set_option(e, k, 0) == 0);
        const int r = ranks[rank_turn++ % 3];
        load_adapters(e, r);
        reserve_all(e, true);
        calls_of_state(e, dt + " adapters r=" + std::to_string(r) + " plain", false, 0);
        compensated_states(e, dt + " adapters r=" + std::to_string(r), {0, 1}, false);
        blim_destroy(e);
        EXPECT(mock_hip_live_allocations() == 0);
    }
    for (int mask = 0; mask < 4; ++mask) {      // the e2m3 second pass, under every value of the fused-tiles mask (read by blim_create)
        const std::string m = std::to_string(mask);
        setenv("BLIM_LO6_FUSED_MASK", m.c_str(), 1);
        blim_engine* e = new_engine(dtype, 1, (dt + " lo6=1 fused_mask=" + m).c_str());
        if (!e) return;
        compensated_states(e, dt + " lo6 mask=" + m, {0}, false);
        if (mask == 3) {
            for (const char* k : {"narrow_gemm", "narrow_lo6", "narrow_qkv"}) EXPECT(blim_set_option(e, k, 2) == 0);
            EXPECT(blim_set_option(e, "precise", 1) == 0);
            calls_of_state(e, dt + " lo6 mask=3 precise narrow=2", false, 1);
            EXPECT(blim_set_option(e, "precise", 0) == 0);
            for (const char* k : {"narrow_gemm", "narrow_lo6", "narrow_qkv"}) EXPECT(blim_set_option(e, k, 0) == 0);
        }
        const int r = ranks[rank_turn++ % 3];
        load_adapters(e, r);
        reserve_all(e, true);
        compensated_states(e, dt + " lo6 mask=" + m + " adapters r=" + std::to_string(r), {0, 1}, false);
        blim_destroy(e);
        EXPECT(mock_hip_live_allocations() == 0);
    }
    unsetenv("BLIM_LO6_FUSED_MASK");
}

static void walk_fp8() {
    blim_engine* e = new_engine(BLIM_COMPUTE_F8, 0, "fp8");
    if (!e) return;
    for (int adapters = 0; adapters < 2; ++adapters) {
        if (adapters) { load_adapters(e, 8); reserve_all(e, false); }
        for (int mask : {31, 5, 10, 0})
            for (int fuse : {0, 1}) {
                EXPECT(blim_set_option(e, "f8_mask", mask) == 0 && blim_set_option(e, "f8_fuse", fuse) == 0);
                calls_of_state(e, std::string("fp8") + (adapters ? " adapters r=8" : "") + " f8_mask=" + std::to_string(mask) + " f8_fuse=" + std::to_string(fuse), false, 0);
            }
    }
    blim_destroy(e);
    EXPECT(mock_hip_live_allocations() == 0);
}

int main() {
    Buffers buffers;
    X = &buffers;
    printf("%s\n", kGemmDefaults);
    for (int dtype : {BLIM_COMPUTE_F16, BLIM_COMPUTE_BF16}) walk_16bit(dtype);
    walk_fp8();
    end_state();
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    fprintf(stderr, "launch trace drive: ok\n");
    return 0;
}
