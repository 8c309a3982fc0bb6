/* blim.h -- C ABI of the MI355X-native BLiM likelihood-scoring engine (libblim_hip.so).
 *
 * The reference (mlvlab/BLiM) is pure Python/PyTorch and has no FFI layer; its boundary for the hot path
 * is the duck-typed Python surface that retrieval_utils.py calls.  This header is
 * the C-ABI the host-side mirror of that surface (blim_amd/modeling.py, blim_amd/retrieval_utils.py)
 * binds with ctypes; every entry point names the reference code it replaces.  INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success or a negative BLIM_ERR_* code and never throws;
 * blim_last_error() returns a message for the calling thread.  All data pointers are DEVICE pointers
 * (HIP) unless the parameter is documented as host; the caller owns every buffer passed in.  Calls are
 * asynchronous on the given hipStream_t (passed as void*; NULL = default stream); the caller synchronises.
 * An engine handle is not thread-safe; distinct handles are independent.  Buffers documented as "bf16" below hold raw
 * 16-bit values of the engine's compute_dtype (bf16 or f16).
 */
#ifndef BLIM_H_
#define BLIM_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BLIM_ABI_VERSION 9
#define BLIM_ERR_ARG (-1)
#define BLIM_ERR_HIP (-2)
#define BLIM_ERR_STATE (-3)
#define BLIM_ERR_NOMEM (-4)

#define BLIM_DTYPE_F32 0
#define BLIM_DTYPE_BF16 1

/* 16-bit compute format of an engine: activations handed across the ABI ("h16" below), the engine's weight copy and the
 * MFMA operand type.  F16 is what the reference itself runs on GPU (main.py:97 .half(), training_utils.py:142 autocast
 * float16) and the default of the Python host; BF16 has the same MFMA rate and an 8-bit mantissa (it holds the 1e-3 bar in the compensated
 * mode, option "precise").  Range: an fp16 engine's 16-bit activation STORES saturate at +-65504 instead of overflowing to inf (the f32
 * residual stream keeps f32's range; NaN / inf operands still propagate) -- where the reference's `.half()` forward turns a SwiGLU product
 * beyond 65504 into NaN scores, the engine returns finite ones; a bf16 engine has f32's range and reproduces the fp32 result
 * (tests/test_gpu_parity.py::test_activations_beyond_fp16_range, tests/golden/saturation.npz recorded from the reference). */
#define BLIM_COMPUTE_BF16 0
#define BLIM_COMPUTE_F16 1
/* fp8 mode (BASELINE.json config 5, "fp8 weights on CDNA4 fp8 MFMA"): q/k/v, o, gate|up, down and
 * lm_head weights are quantised at load to OCP e4m3 with one f32 scale per output row, their input activations per token
 * (scale = absmax / 448; the attention and SwiGLU outputs: one power-of-two E8M0 scale per token and 128 values, written by their
 * producers and fed to the MFMA as its A-side block scale), and multiplied on the block-scaled fp8 MFMA (the f32 scales applied to
 * the f32 accumulator).  Everything else -- attention, RoPE, residual stream, norms, projector, visual head, criteria -- and
 * every 16-bit buffer crossing the ABI is fp16 as with BLIM_COMPUTE_F16.  Scores differ from the fp32 reference at the 1e-2
 * level (reported, not asserted to 1e-3). */
#define BLIM_COMPUTE_F8 2

typedef struct blim_engine blim_engine;

/* Model dimensions: Qwen2Config + mm_* fields of the checkpoint the reference loads (main.py:96-97). */
typedef struct blim_config {
    int32_t vocab_size, hidden_size, intermediate_size, num_layers, num_heads, num_kv_heads;
    int32_t mm_hidden_size; /* projector input width (1024) */
    int32_t num_clips;      /* --num_clips, main.py:59 (4) */
    int32_t max_positions;  /* RoPE table length */
    int32_t compute_dtype;  /* BLIM_COMPUTE_BF16 / BLIM_COMPUTE_F16 / BLIM_COMPUTE_F8 */
    float rms_eps, rope_theta;
} blim_config;

/* A batch of packed token sequences.  Sequence s owns tokens [seq_start[s], seq_start[s]+seq_len[s]) of the
 * packed arrays and may name a shared prefix [pfx_start[s], +pfx_len[s]) (another sequence's tokens, e.g. the
 * video+prompt prefix shared by all text candidates of one query).  Token i of s attends to every prefix token
 * and to own tokens 0..i, restricted to key_visible != 0 (causal AND key-padding AND CPN mask of
 * modeling_qwen2_flash.py:1025-1040 / modeling_videochat_flash.py:409-433).  blk_* list the 32-query blocks:
 * for every sequence, q0 = 0, 32, 64, ... < seq_len. */
typedef struct blim_batch {
    int64_t n_tokens;
    int32_t n_seqs;
    int32_t n_blocks;
    const int32_t* positions;   /* [n_tokens] RoPE position (modeling_qwen2_flash.py:998-1003); every value < blim_config.max_positions
                                 * (device data: not checked by the library, the Python host checks it when it packs the batch) */
    const uint8_t* key_visible; /* [n_tokens] */
    const int32_t* seq_start;   /* [n_seqs] */
    const int32_t* seq_len;     /* [n_seqs] */
    const int32_t* pfx_start;   /* [n_seqs] */
    const int32_t* pfx_len;     /* [n_seqs] (0 = no prefix) */
    const int32_t* blk_seq;     /* [n_blocks] */
    const int32_t* blk_q0;      /* [n_blocks] */
    const int32_t* own_start;   /* [n_tokens] or NULL (ABI v7).  Token i of a sequence attends to its own tokens own_start[i] .. i instead of 0 .. i
                                 * (index inside the sequence): several short continuations of ONE prefix -- the three clip tokens of every candidate
                                 * video of a text, retrieval_utils.py:99-107 -- are packed into one sequence whose segments do not see each other, so the
                                 * 32-query attention blocks are dense instead of holding 3 queries each.  NULL = 0 everywhere (plain causal). */
} blim_batch;

int blim_abi_version(void);
const char* blim_last_error(void);

/* ---- lifetime.  Replaces VideoChatFlashQwenForCausalLM.from_pretrained(...).half().to(device), main.py:96-97. */
int blim_create(const blim_config* cfg, blim_engine** out);
void blim_destroy(blim_engine* e);

/* ---- weights.  `name` is a canonical tensor name (blim_amd/synth.py:weight_shapes); `data` holds the tensor in
 * the checkpoint's natural [out, in] layout as f32 or bf16, on host (on_device = 0) or device.  The engine keeps
 * its own bf16 copy in kernel layout (fused q|k|v with RoPE pair interleave, interleaved gate|up).
 * Replaces load_state_dict / util/misc.py:303-311. */
int blim_load_weight(blim_engine* e, const char* name, const void* data, int32_t dtype, int32_t on_device);
/* Seeded synthetic weights generated on device by the rule of blim_amd/synth.py (no checkpoint available offline). */
int blim_init_synthetic_weights(blim_engine* e, uint64_t seed);
/* 0 when every tensor has been loaded, BLIM_ERR_STATE (message lists a missing tensor) otherwise. */
int blim_weights_ready(const blim_engine* e);

/* ---- content fingerprints (additive in ABI v9; `--calibration_store`, blim_amd/calibration_store.py).  NOT cryptographic: they tell another checkpoint or an
 * edited tensor apart, they do not resist an adversary.  The hash of `bytes` bytes: little-endian 64-bit words w_i (the last one zero-padded), two sums mod 2^64
 * S_k = sum_i mix_k(w_i ^ (i + 1) C_k) with two independent 64-bit finalisers, the byte length mixed in at the end (csrc/kernels.hpp states it; the sums are exact
 * and commutative, so the digest does not depend on the launch grid).  Reads at HBM rate, 64-bit indexing (buffers beyond 4 GiB).
 * blim_hash_device: `p` a DEVICE pointer (any alignment), `out` a HOST array; the call synchronises `stream`.
 * blim_weights_fingerprint: every tensor the scores depend on as the kernels read it -- each tensor placed by blim_load_weight / blim_init_synthetic_weights in its
 * kernel layout (and as blim_train_merge left it), the fp32 visual head's hi + lo rows, the A / B / scaling of every adapter loaded apart -- and the config (dims,
 * compute dtype); not the derived images (e4m3 / e2m3 copies, augmented weights) nor the video vocabulary.  The per-tensor digests are combined in name order with
 * each name and shape: the result does not depend on the order of loading.  BLIM_ERR_STATE until every weight is loaded.  Synchronises `stream`. */
int blim_hash_device(const void* p, int64_t bytes, uint64_t out[2], void* stream);
int blim_weights_fingerprint(blim_engine* e, uint64_t out[2], void* stream);

/* ---- LoRA adapters of a fine-tuned checkpoint, KEPT APART as the reference keeps them.  Replaces main.py:96-105 (peft get_peft_model on the
 * projector `mlp` / `tvg_mlp` Linear "0" / "2", on every q/k/v/o_proj and on lm_head) + main.py:125-128 (load_state_dict of the resume file): the
 * reference evaluates y = W x + b + (alpha / r) B (A x) with A, B as separate matrices; so does the engine for every `weight_name` an adapter was
 * loaded for -- the rank-r term rides in the base product's accumulation (K-augmented operands [x | u] . [W | B]^T, u = (alpha / r) A x, 64 extra K
 * columns), W stays exactly the checkpoint's value and A, B, u travel as hi + lo 16-bit pairs.  `A` [lora_r, in] and `B` [out, lora_r] are HOST
 * float32 arrays in peft's layout (lora_A.weight / lora_B.weight); weight_name is the canonical name of the adapted weight
 * ("layers.<i>.q_proj.w", "lm_head", "mlp.0.w", "tvg_mlp.2.w", ...).  All adapters of an engine share lora_r (<= 16) and lora_alpha (one LoraConfig,
 * main.py:96-101).  Base weights and adapters may be loaded in any order; the augmented weight copies are rebuilt on the next call after either
 * changes.  On an fp8 engine the adapted projections (q/k/v/o, lm_head) run in fp16 once adapters are loaded (the MLP, not adapted, stays e4m3).
 * The alternative -- folding W + (alpha / r) B A into the engine's 16-bit weight on the host before blim_load_weight (blim_amd/checkpoint.py,
 * lora_mode = "merge") -- needs no entry point; it rounds the sum to the engine's format.  An engine whose base weights
 * received a merged update from blim_train_merge refuses adapters (BLIM_ERR_STATE: the update would apply twice) until base weights are loaded again. */
int blim_load_adapter(blim_engine* e, const char* weight_name, const float* A, const float* B, int32_t lora_r, float lora_alpha);
/* Drops every loaded adapter (the engine scores with the base weights again). */
int blim_clear_adapters(blim_engine* e);
/* Number of adapters currently loaded (negative on a NULL engine). */
int blim_num_adapters(blim_engine* e);

/* Pre-size workspaces (optional; they grow on demand, which synchronises the device).  On an engine in the compensated mode (option "precise" = 1 at the time of the
 * call: blim_amd/engine.py's reserve(compensated=True) brackets the call with it) with option "precise_lo6" and its weights in place, this call also builds the
 * weights' e2m3 images and the tile workspaces: running out of device memory is reported here (BLIM_ERR_NOMEM, the matrix named) instead of inside the first
 * compensated scoring call.  Plain calls never build or read the images. */
int blim_reserve(blim_engine* e, int64_t max_tokens, int64_t max_rows);

/* ---- K1: projector.  feats bf16 [n_rows, mm_hidden] -> out bf16 [n_rows, hidden]; which = 0 `mlp`, 1 `tvg_mlp`.
 * Replaces ToMe16_mlp_hd64.forward(video_feature=True), mm_projector_builder.py:156-159. */
int blim_project_video(blim_engine* e, const void* feats, int64_t n_rows, int32_t which, void* out, void* stream);
/* mean over groups of `group` consecutive rows (TVG clip tokens, modeling_videochat_flash.py:243). */
int blim_group_mean(blim_engine* e, const void* in, int64_t n_out, int32_t group, void* out, void* stream);

/* ---- K2: sequence assembly.  out[t] = src_index[t] >= 0 ? embed_tokens[src_index[t]] : feats[-(src_index[t]+1)].
 * Replaces embed_tokens + the splice of modeling_videochat_flash.py:388-440. */
int blim_assemble(blim_engine* e, const int32_t* src_index, int64_t n_tokens, const void* feats, void* out_embeds, void* stream);

/* ---- K3-K9: Qwen2 decoder over a packed batch; writes the final-norm hidden state of rows out_rows[0..n_out)
 * (out_rows = NULL: all tokens) as bf16 and/or f32 (either may be NULL).
 * Replaces Qwen2Model_Flash.forward, modeling_qwen2_flash.py:952-1156. */
int blim_decode(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* out_rows, int64_t n_out,
                void* out_hidden_bf16, float* out_hidden_f32, void* stream);

/* ---- K10+K11: log P(label | hidden) without materialising logits: logprob[r] = log_softmax(lm_head(hidden[r]))[labels[r]],
 * 0 where labels[r] < 0.  Replaces lm_head + .float() (modeling_qwen2_flash.py:1452-1453) + CrossEntropyLoss of
 * VTGCriterion (retrieval_utils.py:23-31). */
int blim_vtg_logprobs(blim_engine* e, const void* hidden_bf16, const int32_t* labels, int64_t n_rows, float* logprob, void* stream);
/* score[p] = sum(logprob[row_start[p] .. row_start[p+1])) / d, d = count_nonzero(...) for mode 0 (VTGCriterion,
 * retrieval_utils.py:32-33) or the row count for mode 1 (TVGCriterion's mean, :42).  e may be NULL. */
int blim_segment_mean(blim_engine* e, const float* logprob, const int32_t* row_start, int32_t n_pairs, int32_t mode, float* score, void* stream);

/* Literal path: logits f32 [n_rows, vocab] = lm_head(hidden) and the criterion on materialised logits. */
int blim_lm_head(blim_engine* e, const void* hidden_bf16, int64_t n_rows, float* logits, void* stream);
/* (e may be NULL for blim_ce_rows) */
int blim_ce_rows(blim_engine* e, const float* logits, int64_t ld, int32_t n_cols, const int32_t* labels, int64_t n_rows, float* logprob, void* stream);

/* ---- K13: visual_head, bf16 [n_rows, hidden] -> bf16 [n_rows, mm_hidden] (modeling_videochat_flash.py:598-599). */
int blim_visual_head(blim_engine* e, const void* hidden_bf16, int64_t n_rows, void* out_bf16, void* stream);
/* The same on FLOAT32 hidden states with a float32 result (device pointers): the head -- an fp32 tensor of the resume file, main.py:104-107 -- and the
 * hidden rows both enter as hi + lo 16-bit operands (three-term product).  What the literal path's forward_visual calls on 16-bit engines. */
int blim_visual_head_f32(blim_engine* e, const float* hidden_f32, int64_t n_rows, float* out_f32, void* stream);
/* ---- K14+K15: vh bf16 [n_pairs, clips, mm_hidden]; vocab bf16 [clips, n_vocab, mm_hidden] (clip-major copy of
 * video_vocab); score[p] = mean_c log_softmax_n(vh[p,c].vocab[c,n] / sqrt(mm_hidden))[labels[p]].
 * Replaces the bmm + TVGCriterion of retrieval_utils.py:106-107, 40-43. */
int blim_tvg_scores(blim_engine* e, const void* vh_bf16, const void* vocab_bf16, int32_t n_vocab, const int32_t* labels,
                    int32_t n_pairs, float* score, void* stream);
/* the logits alone: f32 [n_pairs, clips, n_vocab] (literal path, retrieval_utils.py:106) */
int blim_tvg_logits(blim_engine* e, const void* vh_bf16, const void* vocab_bf16, int32_t n_vocab, int32_t n_pairs, float* logits, void* stream);
/* Registers the video vocabulary (model.module.set_video_vocab, modeling_videochat_flash.py:589-590; retrieval_utils.py:209): `vocab_f32` = DEVICE float32
 * [num_clips][n_vocab][mm_hidden] (clip-major), the clip-mean features of every test video (base_dataset.py:33-37).  The engine keeps it as hi + lo 16-bit
 * operands; blim_tvg_logits / blim_tvg_scores / blim_score_tvg called with vocab_bf16 == NULL then score against it, and in the compensated mode (option
 * "precise": every TVG call of a 16-bit engine) the logits are the three-term product (vh_hi + vh_lo) . (v_hi + v_lo) -- a 16-bit vocabulary alone bounded the
 * bf16 engine's TVG scores at 2 - 7e-4 of the fp32 reference. */
int blim_set_video_vocab(blim_engine* e, const float* vocab_f32, int32_t n_vocab, void* stream);
/* retrieval_utils.py:104-106 for the literal path: logits [n_pairs, num_clips, n_vocab] of FLOAT32 visual-head outputs vh_f32 [n_pairs * num_clips, mm_hidden]
 * (device) against the registered vocabulary, three-term compensated product, / sqrt(mm_hidden). */
int blim_tvg_logits_f32(blim_engine* e, const float* vh_f32, int32_t n_pairs, float* logits, void* stream);

/* ---- Fused scoring: decode + head + criterion in one call.
 * VTG: rows[r] = packed token whose hidden state predicts labels[r]; pair p owns rows [row_start[p], row_start[p+1]). */
int blim_score_vtg(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, const int32_t* labels,
                   int64_t n_rows, const int32_t* row_start, int32_t n_pairs, float* score, void* stream);
/* TVG: rows[p*clips + c] = packed token whose hidden state predicts clip c of pair p. */
int blim_score_tvg(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, const void* vocab_bf16,
                   int32_t n_vocab, const int32_t* labels, int32_t n_pairs, float* score, void* stream);
/* TVG, clip 0 against the WHOLE registered vocabulary (additive in ABI v9; blim_amd/pair_scorer.py: tvg_first): every pair of a text scores clip 0 from the caption
 * prompt's last row, so log P(clip 0 of video j | text) for all j is the log-softmax of ONE logits row.  rows (DEVICE, n_rows) and prior_rows (DEVICE, n_prior; may
 * be NULL with n_prior 0) name packed tokens; the call is blim_score_tvg up to the visual head over those n_rows + n_prior rows, then the clip-0 logits against the
 * registered vocabulary (the three-term product on a compensated call) -- each row bit for bit the one blim_score_tvg forms for a pair of that text -- and
 * blim_tvg_rank over the two row blocks: prior_of (DEVICE [n_rows], may be NULL) names row r's prior row, alpha, k, idx_out / val_out [n_rows, k] and the optional
 * logprob_out [n_rows, n_vocab] are blim_tvg_rank's.  It runs under the options of the TVG calls.  Refused: no registered vocabulary and an fp8 engine
 * (BLIM_ERR_STATE), blim_tvg_rank's refusals of k before anything is launched. */
int blim_score_tvg_first(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, int32_t n_rows, const int32_t* prior_rows, int32_t n_prior,
                         const int32_t* prior_of, float alpha, int32_t k, int32_t* idx_out, float* val_out, float* logprob_out, void* stream);
/* blim_score_tvg_first inside each query's own list of vocabulary entries (additive in ABI v9; pair_scorer.py: tvg_first(within=)): the same launches up to and
 * including the clip-0 logits of the n_rows + n_prior named rows, the same refusals of state, then blim_tvg_rank_within over the two row blocks: n_q queries,
 * row_of / prior_of / within / within_off / n_within, alpha, k and idx_out / val_out [n_q, k] are blim_tvg_rank_within's (row_of indexes rows, prior_of indexes
 * prior_rows).  There is no logprob_out.  blim_tvg_rank_within's refusals of n_q, n_within and k come before anything is launched. */
int blim_score_tvg_first_within(blim_engine* e, const blim_batch* b, const void* embeds, const int32_t* rows, int32_t n_rows, const int32_t* prior_rows,
                                int32_t n_prior, int32_t n_q, const int32_t* row_of, const int32_t* prior_of, const int32_t* within, const int32_t* within_off,
                                int32_t n_within, float alpha, int32_t k, int32_t* idx_out, float* val_out, void* stream);

/* ---- Gallery prefix cache (additive in ABI v9; blim_amd/gallery.py): the K / V of every layer and the last row's final-norm hidden state of prefixes,
 * computed once and kept in device memory, so that a new query is scored on its own continuation tokens alone.  A cache holds prefixes of either kind: a VTG slot
 * is [header][video][instruction] of one gallery video and prompt split (a new text query then packs its response tokens only), a TVG slot is the caption prompt
 * of one gallery text (a new video query then packs its num_clips - 1 clip tokens only).  The fill is kind-neutral: it runs under the options of the calls that
 * will read the slot, and records them.  Layout: slot-major K / V, [n_slots][num_layers][max_len][K heads | V heads (| K_lo | V_lo)] 16-bit values (the lo parts: caches created
 * with compensated = 1, written for the layers whose QKV unit runs compensated), then one hidden row per slot [hi (| lo)], hidden_size values each.
 * blim_prefix_cache_bytes: the device bytes of such a cache (-1 on bad arguments) = n_slots * (num_layers * max_len * 256 * num_kv_heads * (1 + compensated)
 *   + hidden_size * (1 + compensated)) * 2.
 * blim_prefix_cache_create: BLIM_ERR_STATE on an fp8 engine, BLIM_ERR_NOMEM when the device memory is not there.  A cache belongs to one engine.
 * blim_prefix_cache_fill: `b` holds prefix sequences only -- no prefix of their own (pfx_len 0), own_start NULL, every key visible -- and slot_of_seq (HOST, [n_seqs])
 *   names the slot of each (distinct, seq_len <= max_len).  Runs the decoder over the batch as blim_score_vtg would, copies each layer's K / V of the rows into the
 *   slots after its QKV GEMM, and stores the last row's final-norm hidden state.  Each slot records the engine's weights epoch (bumped by blim_load_weight,
 *   blim_init_synthetic_weights, blim_load_adapter, blim_clear_adapters, blim_train_merge) and every option that changes a K / V or hidden value (precise,
 *   precise_embeds, precise_mlp, precise_layers and the layer bits, precise_lo6, masked_query_zero).  Synchronises `stream`.
 * blim_prefix_cache_slot_len: filled length of a slot, -1 when empty (or after a failed fill).
 * blim_score_vtg_cached: blim_score_vtg where sequence s with pfx_slot[s] >= 0 (DEVICE, [n_seqs]) reads its prefix from that slot instead of from packed rows
 *   (b->pfx_len[s] must equal the slot's filled length; pfx_start[s] is then ignored) and -1 keeps the in-batch prefix: one call mixes cached and uncached candidates.
 *   rows[r] < 0 names the cached last-row hidden state of slot -(rows[r] + 1).  slots_used (HOST, n_used entries) lists every slot the call reads through pfx_slot
 *   or rows: a slot that is empty or whose record differs from the engine's present state is refused (BLIM_ERR_STATE, the message names what differs).  The
 *   scores are bit for bit those of blim_score_vtg on the same pairs with the prefixes packed in the batch.  Option "attn_tr" must be 1.
 *   What the library checks is slots_used (host): the device arrays pfx_slot, pfx_len and rows are not read back.  A caller that names a slot in pfx_slot or rows
 *   without listing it in slots_used, or passes a pfx_len other than the slot's filled length, gets WRONG SCORES, not an error -- never a read outside the cache:
 *   pfx_len is clamped to max_len (positions beyond the filled length hold whatever an earlier fill left, or uninitialised values), a pfx_slot >= n_slots reads
 *   the in-batch prefix at pfx_start, a cached row of a slot >= n_slots is a NaN score.  blim_amd/gallery.py derives slots_used from the same plan as the
 *   device arrays.
 * blim_score_tvg_cached: blim_score_tvg with the same conventions (pfx_slot, slots_used, the checks and their messages).  rows[p * num_clips + c] < 0 names the
 *   cached last-row hidden state of slot -(rows + 1): the prompt's last row, which predicts clip 0; it is gathered into the visual head's input after the decode.
 *   Sequences may be segmented (own_start) over a cached prompt: several videos' clip tokens for one text, all naming the text's slot.
 * blim_score_vtg_admit / blim_score_tvg_admit: blim_score_*_cached -- the same scores from the same arguments -- that also CAPTURE in-batch prefixes into slots on the
 *   way through, so that a prefix a call had to compute anyway (a miss) is a cached one for the calls after it.  admits (HOST, n_admit entries; n_admit 0: the cached
 *   call) names them: each a pure prefix sequence of `b` -- pfx_len 0, no own_start segments, every key visible -- with its destination slot, its place in the batch
 *   (start = seq_start[seq], len = seq_len[seq], 1 <= len <= max_len) and row, the index r into rows[] with rows[r] == start + len - 1 (the prefix's last token, whose
 *   final-norm hidden state predicts the first continuation token: the planners always score that row).  The fill's rule: every layer's K / V of the sequence's rows
 *   are copied into the slot after the layer's QKV GEMM (the lo parts too, in compensated caches, for the layers whose QKV unit runs compensated), and the final-norm
 *   hidden state of row rows[row] becomes the slot's hidden row (hi, and lo on a compensated call).  On success every admitted slot records `len` and the engine's
 *   state, as blim_prefix_cache_fill's do; the admitted slots are marked empty before the work starts, so a failed call leaves them empty.  A later call on the same
 *   stream may read the slot: stream order is the only synchronisation, and the call itself never waits for the device (the per-token capture map is built by a
 *   kernel from the admissions, which travel as its arguments: nothing is copied from host memory).  Within the call an admitted prefix is NOT readable: its continuations keep pfx_slot -1.
 *   Refused before anything is launched (BLIM_ERR_ARG, the message names the problem): a slot outside the cache, a slot admitted twice, a slot that is also in
 *   slots_used (reading and overwriting one slot in one call is a race), len outside 1 .. max_len or start + len beyond the batch, row outside rows, seq outside the
 *   batch; and the cached calls' refusals (a compensated call on a plain cache, "attn_tr" 0, an fp8 engine).
 *   What the library checks is the host array: the device arrays (seq_start, seq_len, pfx_len, own_start, key_visible, rows) are not read back.  An admission whose
 *   start / len / row are not its sequence's fills the slot with OTHER rows' values -- wrong scores from that slot later, never a write outside the cache. */
typedef struct blim_pc_admit { int32_t seq, slot, start, len, row; } blim_pc_admit;   /* HOST */
typedef struct blim_prefix_cache blim_prefix_cache;
int64_t blim_prefix_cache_bytes(const blim_engine* e, int32_t n_slots, int32_t max_len, int32_t compensated);
int blim_prefix_cache_create(blim_engine* e, int32_t n_slots, int32_t max_len, int32_t compensated, blim_prefix_cache** out);
void blim_prefix_cache_destroy(blim_prefix_cache* c);
int blim_prefix_cache_fill(blim_engine* e, blim_prefix_cache* c, const blim_batch* b, const void* embeds, const int32_t* slot_of_seq, void* stream);
int blim_prefix_cache_slot_len(const blim_prefix_cache* c, int32_t slot);
int blim_score_vtg_cached(blim_engine* e, blim_prefix_cache* c, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                          const void* embeds, const int32_t* rows, const int32_t* labels, int64_t n_rows, const int32_t* row_start, int32_t n_pairs,
                          float* score, void* stream);
int blim_score_tvg_cached(blim_engine* e, blim_prefix_cache* c, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                          const void* embeds, const int32_t* rows, const void* vocab_bf16, int32_t n_vocab, const int32_t* labels, int32_t n_pairs,
                          float* score, void* stream);
int blim_score_vtg_admit(blim_engine* e, blim_prefix_cache* c, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                         const blim_pc_admit* admits, int32_t n_admit, const void* embeds, const int32_t* rows, const int32_t* labels, int64_t n_rows,
                         const int32_t* row_start, int32_t n_pairs, float* score, void* stream);
int blim_score_tvg_admit(blim_engine* e, blim_prefix_cache* c, const blim_batch* b, const int32_t* pfx_slot, const int32_t* slots_used, int32_t n_used,
                         const blim_pc_admit* admits, int32_t n_admit, const void* embeds, const int32_t* rows, const void* vocab_bf16, int32_t n_vocab,
                         const int32_t* labels, int32_t n_pairs, float* score, void* stream);
/* TVG, clip 0 of named videos given EVERY cached caption prompt, with no decode (additive in ABI v9; blim_amd/gallery.py: TextGalleryIndex.prefilter): a TVG pair's
 * first scored row is the caption prompt's last row, and a slot stores that row's final-norm hidden state.  out[c * ld_out + q] = log P(clip 0 of vocabulary entry
 * cols[c] | the prompt in slots[q]): per chunk of slots the gather of the stored rows, the visual head, the clip-0 logits against the registered vocabulary exactly
 * as blim_score_tvg_first forms them (one statement of them in the engine; the three-term product on a compensated call) and blim_tvg_cols with out0 = the chunk's
 * first index -- each value bit for bit blim_score_tvg_first's logprob_out[row of that prompt][cols[c]].  slots HOST [n_slots], cols DEVICE [n_cols] (blim_tvg_cols'
 * rule for entries outside the vocabulary), out DEVICE f32 [n_cols, ld_out], ld_out >= n_slots.  chunk_rows = 0: max(256, 256 MiB / (4 n_vocab)) rounded down to a
 * multiple of 256, which bounds the logits workspace at 256 MiB; a value does not depend on the chunking.  It runs under the options of the TVG calls.  Nothing
 * waits for the device; the only copy from host memory is the slot list.
 * Refused: null pointers, a cache of another engine, n_slots < 1, n_cols < 1, ld_out < n_slots, chunk_rows < 0 or no multiple of 256 (BLIM_ERR_ARG, the message
 * names the argument); an fp8 engine, no registered vocabulary (BLIM_ERR_STATE); and the cached calls' refusals of the slots with their messages -- outside the
 * cache (BLIM_ERR_ARG), never filled, stale, a compensated call on a cache created plain (BLIM_ERR_STATE) -- before anything is launched. */
int blim_tvg_first_cached(blim_engine* e, blim_prefix_cache* c, const int32_t* slots, int32_t n_slots, const int32_t* cols, int32_t n_cols, float* out, int64_t ld_out,
                          int32_t chunk_rows, void* stream);

/* ---- Slot export / import (additive in ABI v9; blim_amd/gallery.py: HostTier): a slot leaves the prefix cache as a PACKED RECORD and comes back from one, so that
 * a slot can be produced without running the model.  The record of a slot with `len` filled positions: [num_layers][pos < len][kv_w] 16-bit values, then the slot's
 * hidden row of [hid_w] values -- kv_w = 256 * num_kv_heads * (1 + compensated), hid_w = hidden_size * (1 + compensated), the cache's own widths, so a compensated
 * cache's lo parts travel too (those of layers that ran plain as they are: the kernels copy bytes and interpret nothing).  The layout does not depend on the cache's
 * max_len: a record moves between caches of one engine that differ in max_len and slot count.
 * blim_prefix_cache_record_bytes: (num_layers * len * kv_w + hid_w) * 2 rounded up to 256; -1 on bad arguments (len outside 1 .. max_len).
 * blim_prefix_cache_export: packs the slots moves[i].slot into `staging` (DEVICE, 16-byte aligned, staging_bytes long) at moves[i].offset, and writes one ticket per
 *   move (HOST, caller-owned) from host values: the slot's length, the state it was computed under, and the record's geometry.  Only the records' own bytes are
 *   written: their padding and the staging bytes between them are not.
 * blim_prefix_cache_import: the reverse; tickets[i] belongs to moves[i].  The slots are marked empty before the work starts; on success each records `len` and the
 *   TICKET's state (not the engine's present one): a record exported before a weight or option change imports, and the next scoring call that names its slot is
 *   refused as stale, as for any slot.  Only positions < len and the hidden rows of the named slots are written.
 * Both: the moves travel as kernel arguments (48 per launch), no host buffer outlives the call, the call never waits for the device, and stream order is the only
 *   synchronisation -- a later call on the same stream may read an imported slot, or overwrite an exported one.  The transfer between `staging` and host memory is
 *   the caller's.  Refused before anything is launched, the message naming the move: n < 1, a slot outside the cache or named twice, an offset that is not a
 *   multiple of 256, a record outside staging_bytes or overlapping another (BLIM_ERR_ARG); export of an empty slot (BLIM_ERR_STATE) or with len other than the slot's
 *   filled length (BLIM_ERR_ARG); import of a ticket without the magic or with another geometry, len outside 1 .. max_len or other than the ticket's
 *   (BLIM_ERR_ARG); an fp8 engine (BLIM_ERR_STATE).  A ticket is meaningful to the engine that wrote it, while it lives (the weights epoch is the engine's counter). */
#define BLIM_PC_TICKET_MAGIC 0x544B4350u      /* "PCKT" */
#define BLIM_PC_TICKET_LAYERS 256
typedef struct blim_pc_move { int32_t slot; int32_t len; int64_t offset; } blim_pc_move;   /* HOST; offset: bytes into the staging buffer, multiple of 256 */
typedef struct blim_pc_ticket {               /* HOST, plain data */
    uint32_t magic;
    int32_t len;
    int32_t num_layers, kv_w, hid_w;          /* the record's geometry */
    int32_t precise, embeds, mlp, layers, lo6, mqz, n_bits;     /* the slot's recorded state ... */
    uint64_t epoch;
    uint8_t bits[BLIM_PC_TICKET_LAYERS];      /* ... and its n_bits per-layer bits (option "precise_layer_bits") */
} blim_pc_ticket;
int64_t blim_prefix_cache_record_bytes(const blim_prefix_cache* c, int32_t len);
int blim_prefix_cache_export(blim_engine* e, blim_prefix_cache* c, const blim_pc_move* moves, int32_t n, void* staging, int64_t staging_bytes,
                             blim_pc_ticket* tickets_out, void* stream);
int blim_prefix_cache_import(blim_engine* e, blim_prefix_cache* c, const blim_pc_move* moves, int32_t n, const void* staging, int64_t staging_bytes,
                             const blim_pc_ticket* tickets, void* stream);

/* ---- Literal model.forward(inputs_embeds=[B,L,H] bf16, attention_mask=[B,L] u8) -> logits f32 [B,L,V] (may be NULL),
 * hidden f32 [B,L,H] (may be NULL).  Replaces VideoChatFlashQwenForCausalLM.forward, modeling_videochat_flash.py:601-629. */
int blim_forward(blim_engine* e, const void* embeds, const uint8_t* mask, int32_t B, int32_t L, float* logits, float* hidden, void* stream);

/* ---- synthetic data + plain GEMM (bench / tests) */
int blim_fill_bell_bf16(void* out, int64_t n, uint64_t seed, const char* name, float std, float mean, void* stream);
int blim_fill_bell_f32(float* out, int64_t n, uint64_t seed, const char* name, float std, float mean, int32_t round_bf16, void* stream);
/* C [M, ldc] = A [M, lda] . W [N, K]^T, all bf16 (resp. f16) */
int blim_gemm_f16(const void* A, int64_t lda, const void* W, int32_t M, int32_t N, int32_t K, void* C, int64_t ldc, void* stream);
int blim_gemm_bf16(const void* A, int64_t lda, const void* W, int32_t M, int32_t N, int32_t K, void* C, int64_t ldc, void* stream);
/* The compensated GEMM of fp16 engines as a building block (tests; option "precise_lo6"): A_hilo [M, 2 K] fp16 rows [hi | lo], W [N, K] fp16 ->
 * C f32 [M, N] = hi . W^T (fp16 MFMA) + e2m3(lo) . e2m3(W)^T (block-scaled MFMA: e2m3 values with one power-of-two scale per 32), one kernel, one set of
 * accumulators.  a6 / w6 (blim_f6_tiles_bytes(M, K) / (N, K) bytes) receive the e2m3 operand tiles of the lo part and of W in the layout the kernel stages:
 * per (256-row tile, 128-value K-step) 24 KiB of packed 6-bit values in MFMA-lane order + 1 KiB of E8M0 scale bytes (csrc/gemm.hpp).  K % 128 == 0. */
int64_t blim_f6_tiles_bytes(int64_t n_rows, int32_t K);
int blim_gemm_f16_lo6(const void* A_hilo, const void* W, int32_t M, int32_t N, int32_t K, void* a6, void* w6, float* C, void* stream);
/* fp8 building blocks (tests / bench): per-row e4m3 quantisation of a 16-bit matrix (dtype16 = BLIM_COMPUTE_BF16 / _F16;
 * out8 [n_rows, K] bytes, scale [n_rows] = absmax / 448, 1 for an all-zero row), and
 * C f16 [M, ldc] = (A8 [M, lda] . W8 [N, K]^T) * a_scale[m] * w_scale[n] on the block-scaled fp8 MFMA.  K % 128 == 0. */
int blim_quant_rows(const void* in16, int64_t ld, int64_t n_rows, int32_t K, int32_t dtype16, void* out8, float* scale, void* stream);
int blim_gemm_f8(const void* A8, int64_t lda, const float* a_scale, const void* W8, const float* w_scale, int32_t M, int32_t N, int32_t K,
                 void* C, int64_t ldc, void* stream);
/* The decoder's attention kernel alone (tests; additive in ABI v9): every form the engine launches, chosen by the same fields the engine sets (csrc/attention.hpp
 * states them).  qkv 16-bit [n_tokens, ldq] rows [q heads | k heads | v heads (| their lo parts v_lo_off columns further)], head_dim 128, RoPE already applied;
 * `batch` as for blim_decode (positions is not read); out 16-bit [n_tokens, ldo] = softmax(scale q.k over the visible keys) v per query head, hi (| lo at
 * +out_lo_off).  v_lo_off != 0: three-term products over hi + lo operands; out_lo_off != 0: the output leaves as hi + lo; both need use_tr_read = 1.
 * lse_out (may be NULL): f32 [n_tokens, num_heads], natural log-sum-exp of the scaled visible scores, 1e30 for a row without a visible key.
 * out8 (may be NULL; fp16 only): the output as e4m3 bytes [n_tokens, ldo8] with one E8M0 byte per (token, head) in out_mx (layout: csrc/gemm.hpp `a_mx`,
 * mx_stride = bytes per head = 256 * row tiles) INSTEAD of the 16-bit store; `out` must still be a valid pointer.
 * pfx_cache (may be NULL = the uncached launch): sequence s with 0 <= pfx_slot[s] < pc_n_slots reads its prefix keys from rows of slot pfx_slot[s] -- a slot's
 * rows start pc_slot_stride values apart, positions pc_ld apart, each [K heads | V heads (| K_lo | V_lo at +pc_lo_off)] -- every cached key visible, pfx_len
 * clamped to pc_max_len; the cached forms write a 16-bit output only (no out8, no lse_out) and a compensated call needs pc_lo_off != 0.
 * Rows of no sequence and columns beyond num_heads * 128 (resp. out_lo_off + num_heads * 128) are not written.  struct_bytes = sizeof(blim_attention_args)
 * as the caller compiled it: fields added later are read as zero from a shorter struct. */
typedef struct blim_attention_args {
    int64_t struct_bytes;
    const blim_batch* batch;
    const void* qkv;
    int64_t ldq;
    int32_t num_heads, num_kv_heads;
    int32_t dtype16;       /* BLIM_COMPUTE_BF16 / BLIM_COMPUTE_F16 */
    int32_t use_tr_read;   /* engine option "attn_tr_read" */
    int64_t v_lo_off, out_lo_off;
    void* out;
    int64_t ldo;
    float scale;           /* 1 / sqrt(128) in the engine */
    float* lse_out;
    void* out8;
    int64_t ldo8;
    void* out_mx;
    int64_t mx_stride;
    const void* pfx_cache;
    const int32_t* pfx_slot;
    int64_t pc_slot_stride, pc_ld, pc_lo_off;
    int32_t pc_n_slots, pc_max_len;
} blim_attention_args;
int blim_attention(const blim_attention_args* args, void* stream);

/* The trainer's attention backward alone (tests; additive in ABI v9): the kernels of csrc/train_kernels.hip over materialised scores, chosen by the fields the
 * trainer sets (csrc/train.hpp: AttnBwdParams).  Sequences have no shared prefix: token i of sequence s is row seq_start[s] + i, query i sees the keys j <= i with
 * key_visible != 0.  qkv 16-bit [n_tokens, ldq] rows [q heads | k heads | v heads], head_dim 128, RoPE applied; dout 16-bit [n_tokens, ldo] = d(attention
 * output), q-head major; o16 16-bit [n_tokens, ldo16] = the forward's output; lse f32 [n_tokens, num_heads] = the forward's lse_out.  key_visible, seq_start,
 * seq_len: device arrays as in blim_batch; max_len >= the longest seq_len (device data: the library cannot check it).  dqkv f32 [n_tokens, ldq] receives the
 * gradient w.r.t. the post-RoPE q | k | v on the rows of the sequences, columns < (num_heads + 2 num_kv_heads) * 128; nothing else is written.
 * workspace: blim_attention_bwd_workspace_bytes(...) bytes, caller-owned, 16-byte aligned, contents on entry irrelevant -- D f32 [n_tokens, num_heads] rounded up to
 * 16 bytes, then P16 and dS16, 16-bit [n_seqs][num_heads][Lm][Lm] each, Lm = round_up(max_len, 64); -1 for arguments out of range (n_seqs * num_heads > 65535
 * among them).  struct_bytes = sizeof(blim_attention_bwd_args). */
typedef struct blim_attention_bwd_args {
    int64_t struct_bytes;
    const void* qkv;
    int64_t ldq;
    const void* dout;
    int64_t ldo;
    const void* o16;
    int64_t ldo16;
    const float* lse;
    int32_t num_heads, num_kv_heads;
    int32_t dtype16;       /* BLIM_COMPUTE_BF16 / BLIM_COMPUTE_F16 */
    const uint8_t* key_visible;
    const int32_t* seq_start;
    const int32_t* seq_len;
    int32_t n_seqs, max_len;
    float scale;           /* 1 / sqrt(128) in the trainer */
    void* workspace;
    int64_t workspace_bytes;
    float* dqkv;
    int64_t n_tokens;
} blim_attention_bwd_args;
int64_t blim_attention_bwd_workspace_bytes(int64_t n_tokens, int32_t n_seqs, int32_t num_heads, int32_t max_len);
int blim_attention_bwd(const blim_attention_bwd_args* args, void* stream);
/* The RoPE backward that follows it (tests): out16 16-bit [n_tokens, qkv_n] = the inverse rotation of dqkv f32 [n_tokens, qkv_n] on the columns < rope_cols
 * (pairs d, d + 64 of every 128-wide head), the plain 16-bit rounding beyond.  cos / sin: device arrays f32 [n_pos, 64]; the row of token t is
 * min(max(positions[t], 0), n_pos - 1).  qkv_n and rope_cols are multiples of 128, rope_cols <= qkv_n. */
int blim_rope_bwd(void* out16, const float* dqkv, int64_t n_tokens, int32_t qkv_n, int32_t rope_cols, const int32_t* positions, const float* cos, const float* sin,
                  int32_t n_pos, int32_t dtype16, void* stream);

/* ---- The trainer's remaining kernels alone (tests; additive in ABI v9): the LoRA products, the RMSNorm backward, cross-entropy, GELU, AdamW and the gradient
 * statistics of csrc/train_kernels.hip, each behind the launcher the trainer calls (csrc/train.hpp states the operations), over raw device pointers: no engine, no
 * trainer.  Every entry checks its host-visible arguments before any launch (BLIM_ERR_ARG + blim_last_error()); scratch is ONE caller-owned workspace per entry,
 * 16-byte aligned, contents on entry irrelevant, sized by the entry's ..._workspace_bytes(...) (-1 for arguments out of range).  dtype16 = BLIM_COMPUTE_BF16 / _F16,
 * r = the adapter rank, 1..16.  The bases that the kernels read or write as vectors must be 16-byte aligned and are checked: x16, dy16, dx, dy, x, w and
 * every A of the dx / RMSNorm entries (out16: 8 bytes); the others (u16, du, B, dB, dA, the GELU and optimizer arrays) are accessed element by element.  struct_bytes = sizeof(the struct). */

/* u~ = scale * drop(x) A^T of 1..3 adapters reading the same rows: x16 16-bit [T, ldx], columns [0, K) are read, columns K + seg * r + j (seg < n_adapters, j < r)
 * receive 16-bit(scale * sum_k drop_seg(x)[t, k] * 16-bit(A_seg[j, k])); nothing else is written.  A[seg]: f32 [r, K].  Adapter seg uses dropout site `site + seg`;
 * the mask of element (t, k) is drop_mult4's at index t * K + k.  K % 16 == 0, ldx % 8 == 0, ldx >= K + n_adapters * r.
 * workspace: n_adapters 16-bit [16, K] copies of A (rows r.. zeroed by the entry). */
typedef struct blim_lora_down_args {
    int64_t struct_bytes;
    void* x16;
    int64_t ldx, T;
    int32_t K, n_adapters, r, dtype16;
    const float* A[3];
    float scale, drop_p;
    uint64_t seed;
    uint32_t site;
    int32_t reserved;
    void* workspace;
    int64_t workspace_bytes;
} blim_lora_down_args;
int64_t blim_lora_down_workspace_bytes(int32_t n_adapters, int32_t K);
int blim_lora_down(const blim_lora_down_args* args, void* stream);

/* The three gradients of one adapter y += scale * B A drop(x), any subset (flags), in the trainer's order dB, du, dA:
 *   BLIM_LORA_DB  dB f32 [N, r] += sum_t dy16[t, n] * u16[t, j]            dy16 16-bit [T, ldy] (ldy % 8 == 0, ldy >= round_up(N, 8); columns [N, ldy) are not
 *                                                                          read into the result), u16 16-bit rows of stride ldu (the u~ columns of an augmented row)
 *   BLIM_LORA_DU  du f32 [T, r]  = scale * sum_n dy16[t, n] * 16-bit(B[n, j])   B f32 [N, r]; OVERWRITTEN.  The contraction runs over round_up(N, 16) columns:
 *                                                                          ldy >= round_up(N, 16) and dy16 columns [N, round_up(N, 16)) MUST BE ZERO
 *   BLIM_LORA_DA  dA f32 [r, K] += sum_t du[t, j] * drop(x16)[t, k]        x16 16-bit [T, ldx] (K % 8 == 0, ldx % 8 == 0, ldx >= K), du f32 [T, r] (this call's
 *                                                                          when BLIM_LORA_DU is set, else the caller's), entering as hi + lo 16-bit parts
 * workspace: the split reductions' partial sums (the largest of the selected products'), then Bt16 16-bit [16, round_up(N, 16)] for du. */
#define BLIM_LORA_DB 1
#define BLIM_LORA_DU 2
#define BLIM_LORA_DA 4
typedef struct blim_lora_grads_args {
    int64_t struct_bytes;
    int32_t flags, dtype16;
    int64_t T;
    int32_t N, K, r, reserved;
    const void* dy16;
    int64_t ldy;
    const void* u16;
    int64_t ldu;
    const void* x16;
    int64_t ldx;
    const float* B;
    float scale, drop_p;
    uint64_t seed;
    uint32_t site;
    int32_t reserved2;
    float* dB;
    float* du;
    float* dA;
    void* workspace;
    int64_t workspace_bytes;
} blim_lora_grads_args;
int64_t blim_lora_grads_workspace_bytes(int32_t flags, int64_t T, int32_t N, int32_t K, int32_t r);
int blim_lora_grads(const blim_lora_grads_args* args, void* stream);

/* The adapters' input gradient: dx f32 [T, ldd] columns [0, K) += sum_seg keep_seg(t, k) / (1 - p) * sum_j du[seg][t, j] * A[seg][j, k] (du f32 [T, r], A f32 [r, K]).
 * out16 != NULL: dx is only READ and the sum leaves as 16-bit rows [T, ldo] instead.  K % 4 == 0, ldd % 4 == 0, ldo % 4 == 0, both >= K.  No workspace. */
typedef struct blim_lora_dx_args {
    int64_t struct_bytes;
    float* dx;
    int64_t ldd, T;
    int32_t K, n_adapters, r, dtype16;
    const float* du[3];
    const float* A[3];
    float drop_p;
    uint32_t site;
    uint64_t seed;
    void* out16;
    int64_t ldo;
} blim_lora_dx_args;
int blim_lora_dx(const blim_lora_dx_args* args, void* stream);

/* d/dx of y = w * x * rsqrt(mean(x^2) + eps) applied to dy f32 [n_rows, H]: row i of dy belongs to row (rows ? rows[i] : i) of x and dx (f32, row stride H);
 * accumulate != 0 adds to dx.  out16 (rows == NULL): the 16-bit copy of the updated dx rows.  n_adapters > 0 (rows == NULL, H <= 4096): dy is taken as
 * dy + blim_lora_dx's term (du, A, r, drop_p, seed, site as there, K = H), formed on the fly.  H % 4 == 0, H <= 8192.  Refused by name: out16 with rows,
 * adapters with rows, adapters with H > 4096, H > 8192.  No workspace. */
typedef struct blim_rmsnorm_bwd_args {
    int64_t struct_bytes;
    float* dx;
    const float* dy;
    const float* x;
    const int32_t* rows;
    int64_t n_rows;
    int32_t H, accumulate;
    const float* w;
    float eps;
    int32_t dtype16;
    void* out16;
    int32_t n_adapters, r;
    const float* du[3];
    const float* A[3];
    float drop_p;
    uint32_t site;
    uint64_t seed;
} blim_rmsnorm_bwd_args;
int blim_rmsnorm_bwd(const blim_rmsnorm_bwd_args* args, void* stream);

/* Cross-entropy over rows of f32 logits [n_rows, ldl] (columns [V, ldl) are not read): the label of row i is labels[i / label_div]; *loss += sum_i -log_softmax(
 * logits[i])[label]; d = coef * (softmax - onehot) leaves as 16-bit (dl16) or f32 (dl32) rows [n_rows, ldd] -- exactly one of the two -- with columns [V, ldd)
 * written as 0.  A label < 0 or >= V: loss 0 and an all-zero gradient row.  workspace: n_rows floats (the per-row losses, summed in a fixed order). */
int64_t blim_ce_workspace_bytes(int64_t n_rows);
int blim_ce_fwd_bwd(const float* logits, int64_t ldl, int32_t V, const int32_t* labels, int32_t label_div, int64_t n_rows, float coef, void* dl16, float* dl32,
                    int64_t ldd, float* loss, int32_t dtype16, void* workspace, int64_t workspace_bytes, void* stream);

/* Exact-erf GELU on 16-bit pre-activations pre16 [rows, H] (contiguous).  backward == 0: out16 [rows, ldo] = gelu(pre16), ldo >= H, dh not read.
 * backward != 0: out16 [rows, H] = 16-bit(dh * gelu'(pre16)), dh f32 [rows, H], ldo == H. */
int blim_gelu(int32_t backward, void* out16, int64_t ldo, const void* pre16, const float* dh, int64_t rows, int32_t H, int32_t dtype16, void* stream);

/* blim_train_adamw's kernel on caller arrays of n floats (step >= 1 gives the bias corrections), and blim_train_grad_stats's: stats[0] += sum (g * inv_scale)^2,
 * stats[1] = 1 if any g * inv_scale is inf / NaN (otherwise untouched).  workspace of the latter: 1024 floats. */
int blim_adamw_raw(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   float inv_scale, int32_t step, void* stream);
int64_t blim_grad_stats_workspace_bytes(int64_t n);
int blim_grad_stats_raw(const float* g, int64_t n, float inv_scale, float* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The scoring path's row kernels alone (tests; additive in ABI v9): the forward RMSNorm in every kernel and output form, the log-sum-exp combine behind
 * blim_vtg_logprobs, the TVG criterion, the clip mean and the sequence assembly of csrc/kernels.hip, each a plain pass-through to the launcher the engine calls
 * (csrc/kernels.hpp states the operations), over raw device pointers: no engine, no state.  blim_ce_rows and blim_segment_mean above already are such
 * pass-throughs.  Labels, table and feature indices are NOT guarded by these kernels: they must be in range.  Only blim_rmsnorm's gather index is guarded.
 *
 * blim_rmsnorm: row i of the outputs = w * x[rows ? rows[i] : i, :] * rsqrt(mean(x^2) + eps), x f32 rows of stride ldx; rows (int32 [n_rows]) gathers among
 * n_src source rows -- an index outside [0, n_src) gives a poisoned row: NaN in out16 and out_f32, zeros in out_lo and in the row's blocks of out6.
 * out16 16-bit rows of stride ldo (0 = H), out_lo = 16-bit(o - f32(out16)) with the same stride (needs out16), out_f32 f32 [n_rows, H]; at least one of
 * out16 / out_f32.  saturate: fp16 stores clamp to +-65504 instead of overflowing to inf.  out6: the lo parts as the e2m3 operand tiles of the consuming GEMM,
 * blim_f6_tiles_bytes(n_rows, H) bytes, the rows up to the next multiple of 256 zero -- needs out16, H % 128 == 0, 256 < H <= 4096, ldo % 8 == 0.
 * H % 4 == 0, H <= 4096, ldx % 4 == 0, ldo % 4 == 0; x, w, out_f32 16-byte aligned, out16 / out_lo 8-byte (16 where ldo % 8 == 0 and H % 8 == 0). */
typedef struct blim_rmsnorm_args {
    int64_t struct_bytes;
    const float* x;
    int64_t ldx;
    const int32_t* rows;
    int64_t n_rows, n_src;
    int32_t H, dtype16;
    const float* w;
    float eps;
    int32_t saturate;
    void* out16;
    int64_t ldo;
    void* out_lo;
    float* out_f32;
    void* out6;
} blim_rmsnorm_args;
int blim_rmsnorm(const blim_rmsnorm_args* args, void* stream);
/* The fp8 engines' RMSNorm: out8 e4m3 [n_rows, H] = the row / scale, scale [n_rows] = max|row| / 448 (1 for an all-zero row). */
int blim_rmsnorm_f8(const float* x, int64_t ldx, int64_t n_rows, int32_t H, const float* w, float eps, void* out8, float* scale, void* stream);
/* logprob[r] = labels[r] < 0 ? 0 : label_logit[r] - logsumexp of row r's n_tiles (max, sum exp(x - max)) partials; part f32 [n_rows, n_tiles, 2], a tile
 * without columns is (-inf, 0). */
int blim_lse_combine(const float* part, int32_t n_tiles, const float* label_logit, const int32_t* labels, int64_t n_rows, float* logprob, void* stream);
/* score[p] = mean over c < clips of log_softmax(logits[p * clips + c, :n_vocab])[labels[p]]; logits f32 rows of stride ld >= n_vocab. */
int blim_tvg_criterion(const float* logits, int64_t ld, int32_t n_vocab, const int32_t* labels, int32_t n_pairs, int32_t clips, float* score, void* stream);
/* Row log-softmax over the vocabulary plus the exact top k, one launch.  lp[r][j] = log_softmax(logits[r, :n_vocab])[j] with blim_tvg_criterion's own normaliser:
 * as a float, blim_tvg_criterion of row r with label j at clips = 1.  term = lp, or, for 0 <= prior_of[r] < n_prior, lp - alpha * pl with pl the same expression over
 * row prior_of[r] of prior_logits (f32 rows of stride ld_prior), in f32 with two roundings and no fused multiply-add; prior_of (DEVICE [n_rows]) may be NULL, an entry
 * < 0 means no prior (term = lp, the same bits), an entry >= n_prior gives a NaN row, never a read outside the buffer (the device array is not read back).
 * idx_out / val_out [n_rows, k] = the first k of the stable descending order of term: ties to the lower index, -inf after every finite value, NaN last and by
 * index among themselves; exact and deterministic.  logprob_out (optional, rows of stride ld_out) receives the lp rows; columns >= n_vocab are left alone.
 * BLIM_ERR_ARG (the message names the argument): a null logits / idx_out / val_out, n_vocab < 1, n_rows < 1, k < 1, k > n_vocab, k > BLIM_TVG_RANK_MAX_K, ld /
 * ld_prior / ld_out below n_vocab, prior_of without prior_logits, n_prior < 0. */
#define BLIM_TVG_RANK_MAX_K 1024
int blim_tvg_rank(const float* logits, int64_t ld, int32_t n_vocab, int32_t n_rows, const float* prior_logits, int64_t ld_prior, int32_t n_prior,
                  const int32_t* prior_of, float alpha, int32_t k, int32_t* idx_out, float* val_out, float* logprob_out, int64_t ld_out, void* stream);
/* blim_tvg_rank inside a caller's list of columns (additive in ABI v9), one workgroup per QUERY q < n_q, since two queries on one logits row may carry different
 * lists.  All of row_of, prior_of, within and within_off are DEVICE int32 and are never read back.  row_of [n_q] names query q's logits row (NULL: q itself); an
 * entry outside 0 .. n_rows - 1 makes every term of q a NaN and reads nothing.  prior_of [n_q] is blim_tvg_rank's, per query.  Query q's list is
 * within[within_off[q] .. within_off[q + 1]) of within [n_within], within_off [n_q + 1]; offsets are clamped to 0 .. n_within and a decreasing pair is an empty
 * list.  The term of list position p is, bit for bit, blim_tvg_rank's term of column within[p] -- both normalisers stay over the whole row of n_vocab columns --; an
 * entry outside 0 .. n_vocab - 1 has a quiet-NaN term and reads nothing; a list may repeat an entry, each position is ranked on its own.
 * idx_out / val_out [n_q, k]: the first min(k, m_q) POSITIONS into q's own list (m_q its length) in blim_tvg_rank's order -- ties to the lower position, NaN last --
 * and the terms' bits; places from m_q on hold -1 and a quiet NaN.  k > m_q is no error and m_q has no limit.
 * BLIM_ERR_ARG (the message names the argument): a null logits / within / within_off / idx_out / val_out, n_vocab < 1, n_rows < 1, n_q < 1, n_within < 0, k < 1,
 * k > BLIM_TVG_RANK_MAX_K, ld / ld_prior below n_vocab, prior_of without prior_logits, n_prior < 0. */
int blim_tvg_rank_within(const float* logits, int64_t ld, int32_t n_vocab, int32_t n_rows, const float* prior_logits, int64_t ld_prior, int32_t n_prior, int32_t n_q,
                         const int32_t* row_of, const int32_t* prior_of, const int32_t* within, const int32_t* within_off, int32_t n_within, float alpha, int32_t k,
                         int32_t* idx_out, float* val_out, void* stream);
/* blim_tvg_rank's select and sort over GIVEN values (f32 rows of stride ld >= n, n per row): idx_out / val_out [n_rows, k] = the first k of blim_tvg_rank's order
 * applied to the values as they stand -- descending, ties to the lower index, -0 = +0, -inf after every finite value, NaN last and by index among themselves;
 * exact and deterministic.  val_out holds the chosen values' own bits.
 * BLIM_ERR_ARG (the message names the argument): a null values / idx_out / val_out, n < 1, n_rows < 1, ld below n, and blim_tvg_rank's refusals of k in its own
 * words: k < 1, k > n, k > BLIM_TVG_RANK_MAX_K. */
int blim_rank_rows(const float* values, int64_t ld, int32_t n, int32_t n_rows, int32_t k, int32_t* idx_out, float* val_out, void* stream);
/* Named columns of the row log-softmax, transposed: out[c * ld_out + out0 + r] = logits[r * ld + cols[c]] - (mx + logf(sm)) of row r, the normaliser formed by
 * one wave exactly as blim_tvg_criterion and blim_tvg_rank form it -- as a float, blim_tvg_criterion of row r with label cols[c] at clips = 1, and blim_tvg_rank's
 * logprob_out[r][cols[c]].  cols (DEVICE [n_cols]) may repeat; an entry outside 0 .. n_vocab - 1 stores a quiet NaN, never a read outside the row (the device array
 * is not read back).  Nothing else in out is written: columns before out0 and from out0 + n_rows on, and rows >= n_cols, are left alone.
 * BLIM_ERR_ARG (the message names the argument): a null logits / cols / out, n_vocab < 1, n_rows < 1, n_cols < 1, ld < n_vocab, out0 < 0, ld_out < out0 + n_rows. */
int blim_tvg_cols(const float* logits, int64_t ld, int32_t n_vocab, int32_t n_rows, const int32_t* cols, int32_t n_cols, float* out, int64_t ld_out, int64_t out0,
                  void* stream);
/* blim_group_mean / blim_assemble with the engine's fields as arguments: H, the 16-bit type, the embedding table (16-bit [*, H]) and split -- rows [hi | lo] of
 * width 2 H (feature rows and outputs; a table row's lo half is zero).  H % 8 == 0 for the assembly, H % 4 == 0 for the mean. */
int blim_group_mean_rows(void* out, const void* in, int64_t n_out, int32_t group, int32_t H, int32_t dtype16, int32_t split, void* stream);
int blim_assemble_rows(void* out, const int32_t* src_index, int64_t n_tokens, int32_t H, const void* table, const void* feats, int32_t split, void* stream);

/* The GEMM kernel alone (tests; additive in ABI v9): C [M, N] = A [M, K] . W [N, K]^T with every epilogue and operand form the engine and the trainer launch,
 * chosen by the same fields they set (csrc/gemm.hpp states them; a zero / NULL field is "off").  A: row stride lda, W: row stride K (w_wrap_k when set).
 * dtype BLIM_COMPUTE_BF16 / _F16: A, W and 16-bit outputs in that format; BLIM_COMPUTE_F8: A, W e4m3 bytes with row_scale [M] (or the E8M0 table a_mx) and
 * col_scale [N], 16-bit outputs fp16.
 *   BLIM_EPI_BF16    C 16-bit [M, ldc] = act(acc + bias), act 1 = exact-erf GELU.  Trainer forms: swiglu_act != NULL -- the tile is gate | up (16 / 16 columns
 *                    interleaved), stored to C, and silu(gate) * up [M, N / 2] goes to swiglu_act (row stride swiglu_act_ld); swiglu_gu != NULL -- the tile is
 *                    d act and is not stored (C must be valid, it is not written): the saved gate | up rows at swiglu_gu [M, swiglu_ld] become [d gate | d up] in place
 *   BLIM_EPI_F32     C f32 = acc * scale
 *   BLIM_EPI_RESID   C f32 = (resid_in ? resid_in : C) + (acc + bias); resid_in has C's row stride
 *   BLIM_EPI_QKV     C 16-bit = rope(acc + bias) on columns < rope_cols, acc + bias beyond; W rows of q / k heads in the pair-interleaved order of gemm.hpp
 *                    (qkv_perm_row), the output in natural order; rope_rows: the table blim_rope_rows writes, rope_stride >= M rows per chunk
 *   BLIM_EPI_SWIGLU  C 16-bit [M, N / 2] = silu(gate) * up, W rows 16 gate / 16 up interleaved.  BLIM_COMPUTE_F8 with out8 != NULL: the output leaves as e4m3
 *                    bytes at out8 (row stride ldc BYTES, C is not used) with one E8M0 byte per (row, 128 columns) in out_mx (layout: gemm.hpp, mx_stride)
 *   BLIM_EPI_LSE     lse_part f32 [M, ceil(N / 256), 2] = (max, sum exp(x - max)) per 256-column tile, label_logit [M] = the logit of column labels[m]
 *                    (not written for a label < 0 or >= N); C is not used
 * w_wrap_k: A is [hi | lo] along K (K counts both halves), W [N, w_wrap_k] is walked twice.  lo_off != 0 (BF16 / QKV / SWIGLU, 16-bit dtypes): the output leaves
 * as hi at C and lo = round16(x - hi) at C + lo_off elements; the lo half must lie behind the output and inside the row.  f16_saturate: fp16 stores clamp to
 * +-65504 instead of overflowing to inf.  A6 / W6 / K6 (16-bit dtypes; RESID / QKV with lo_off / SWIGLU / LSE): a second pass acc += e2m3(lo of A) . e2m3(W)^T
 * over operand tile images of blim_f6_tiles_bytes(M, K6) / (N, K6) bytes; with f6_build != 0 the entry writes both images first, W6 from W [N, K] and A6 from
 * the lo part that sits K columns behind A (row stride lda), K6 = K, as blim_gemm_f16_lo6 does.  out6 (SWIGLU with lo_off and A6): the lo half leaves as the
 * e2m3 tile image of the consuming GEMM (blim_f6_tiles_bytes(M, N / 2) bytes) INSTEAD of the 16-bit store at C + lo_off.
 * struct_bytes = sizeof(blim_gemm_args) as the caller compiled it: fields added later are read as zero from a shorter struct. */
#define BLIM_EPI_BF16 0
#define BLIM_EPI_F32 1
#define BLIM_EPI_RESID 2
#define BLIM_EPI_QKV 3
#define BLIM_EPI_SWIGLU 4
#define BLIM_EPI_LSE 5
typedef struct blim_gemm_args {
    int64_t struct_bytes;
    int32_t epi;           /* BLIM_EPI_* */
    int32_t dtype;         /* BLIM_COMPUTE_BF16 / _F16 / _F8 */
    const void* A;
    int64_t lda;
    const void* W;
    int32_t M, N, K;
    int32_t act;
    void* C;
    int64_t ldc;
    const float* bias;
    const float* resid_in;
    float scale;           /* BLIM_EPI_F32 */
    int32_t w_wrap_k;
    int64_t lo_off;
    int32_t f16_saturate;
    int32_t rope_cols;
    const float* rope_rows;
    int64_t rope_stride;
    const int32_t* labels;
    float* lse_part;
    float* label_logit;
    const float* row_scale;
    const float* col_scale;
    const void* a_mx;
    void* out8;
    void* out_mx;
    int64_t mx_stride;
    void* A6;
    void* W6;
    int32_t K6;
    int32_t f6_build;
    void* out6;
    void* swiglu_act;
    int64_t swiglu_act_ld;
    void* swiglu_gu;
    int64_t swiglu_ld;
    int32_t tile;          /* 0 = 256 x 256 tiles, 1 = auto, 2 = the narrow kernel (see below) */
    int32_t tile_lo6;      /* the same for BLIM_EPI_RESID with A6 / W6: 0 = 256 x 256 tiles, 1 = auto, 2 = the narrow e2m3 kernel (see below) */
    int32_t tile_qkv;      /* the same for BLIM_EPI_QKV on fp16 / bf16 operands: 0 = 256 x 256 tiles, 1 = auto, 2 = the narrow QKV kernel (see below) */
} blim_gemm_args;
int blim_gemm(const blim_gemm_args* args, void* stream);
/* tile (added at the end of the struct; the ABI version is unchanged -- a shorter struct reads as 0): BLIM_EPI_RESID on fp16 / bf16 operands without A6 / W6 also exists
 * in 64 x 64 tiles, one per 4-wave workgroup, with the same walk over K -- every C element sees the same chain of MFMAs in the same order, so the result is the 256 x 256
 * kernel's bit for bit -- for calls whose 256 x 256 grid leaves most of the chip idle (a few hundred rows against N = 3584: 28 workgroups).  2 = that kernel; any other
 * epilogue, BLIM_COMPUTE_F8, A6 / W6 and a_mx are refused with the field named.  1 = auto: that kernel when the form is eligible and
 * ceil(M / 256) * ceil(N / 256) < blim_gemm_narrow_threshold(), the 256 x 256 kernel otherwise (an ineligible form is not an error).  Other values: BLIM_ERR_ARG.
 * blim_gemm_narrow_launches(): launches of the narrow kernel by this process so far (host-side counter; tests read it to see which kernel ran). */
int64_t blim_gemm_narrow_launches(void);
int32_t blim_gemm_narrow_threshold(void);
/* tile_lo6 (added behind `tile`, same rule: a shorter struct reads as 0): the form `tile` refuses -- BLIM_EPI_RESID on fp16 / bf16 operands WITH the e2m3 second
 * pass (A6 / W6, w_wrap_k = 0) -- exists in 64 x 64 tiles as well.  The kernel walks the hi operand as the narrow kernel does and continues, in the same
 * accumulators, with one block-scaled e2m3 MFMA per 128-value K-step over the same A6 / W6 tile images: every C element sees the 256 x 256 kernel's chain, so the
 * bits are equal.  2 = that kernel; a call without A6 / W6, any other epilogue, BLIM_COMPUTE_F8 and w_wrap_k are refused with the field named.  1 = auto: that
 * kernel when the form is eligible and ceil(M / 256) * ceil(N / 256) < blim_gemm_narrow_lo6_threshold(), the 256 x 256 kernel otherwise (an ineligible form is not
 * an error).  Other values: BLIM_ERR_ARG.  `tile` keeps every behaviour it has (tile = 2 with A6 is still refused): the two fields choose for disjoint forms.
 * blim_gemm_narrow_lo6_launches(): launches of THAT kernel by this process so far -- a counter of its own; blim_gemm_narrow_launches() does not move on them. */
int64_t blim_gemm_narrow_lo6_launches(void);
int32_t blim_gemm_narrow_lo6_threshold(void);
/* tile_qkv (added behind `tile_lo6`, same rule: a shorter struct reads as 0): BLIM_EPI_QKV on fp16 / bf16 operands exists in 64 x 64 tiles as well, in every 16-bit
 * form the 256 x 256 kernel has: plain or hi | lo outputs (lo_off) over the plain or the w_wrap_k walk (lda > K included), and hi | lo outputs behind the e2m3 second
 * pass (A6 / W6).  The K walk is the narrow kernels', the epilogue (bias, RoPE from rope_rows, 16-bit rounding inside the fp16 saturation window, hi | lo) is the
 * 256 x 256 kernel's per element: every stored element is equal bit for bit.  2 = that kernel; any other epilogue, BLIM_COMPUTE_F8 and A6 without lo_off are refused
 * with the field named.  1 = auto: that kernel when the form is eligible and ceil(M / 256) * ceil(N / 256) < blim_gemm_narrow_qkv_threshold(), the 256 x 256 kernel
 * otherwise (an ineligible form is not an error).  Other values: BLIM_ERR_ARG.  `tile` and `tile_lo6` keep every behaviour they have (both still refuse
 * BLIM_EPI_QKV under 2).  blim_gemm_narrow_qkv_launches(): launches of THAT kernel by this process so far -- a counter of its own; the other two do not move. */
int64_t blim_gemm_narrow_qkv_launches(void);
int32_t blim_gemm_narrow_qkv_threshold(void);
/* cos / sin of every token's position as BLIM_EPI_QKV reads them (csrc/gemm.hpp: rope_rows): out f32 [8 = {cos, sin} x 4 groups of 16 dims][stride rows][16],
 * row t of every chunk = position min(max(positions[t], 0), max_positions - 1); stride >= n_tokens.  workspace: blim_rope_rows_bytes(max_positions) bytes (the
 * cos | sin tables of all positions, built by the call as the engine builds its own at creation); out: 128 * stride floats. */
int64_t blim_rope_rows_bytes(int32_t max_positions);
int blim_rope_rows(const int32_t* positions, int64_t n_tokens, float rope_theta, int32_t max_positions, void* workspace, float* out, int64_t stride, void* stream);

/* ---- per-kernel-class timing (hipEvents on the launch stream).  Classes: see blim_timing_class_name. */
int blim_timing_enable(blim_engine* e, int32_t on);
int blim_timing_num_classes(void);
const char* blim_timing_class_name(int32_t cls);
/* Synchronises the recorded events; ms[c] = total ms, calls[c] = launches, flops[c] = FLOPs issued (host arrays of
 * blim_timing_num_classes() entries); then clears the record. */
int blim_timing_report(blim_engine* e, double* ms, int64_t* calls, double* flops);

/* Bring-up aid: copies the first `bytes` bytes of an internal workspace ("resid" f32 [T,H], "xn" bf16 [T,H],
 * "qkv" bf16 [T,(nh+2nkv)*128], "attn" bf16 [T,H], "act" bf16 [T,I]) as the last blim_decode left it. */
int blim_debug_read(blim_engine* e, const char* which, void* dst, int64_t bytes, void* stream);

/* Bring-up aid: when non-NULL, every GEMM workgroup writes s_memrealtime stamps {entry, main loop start, main loop end, exit,
 * C staged in LDS, stores issued} to device_buf[workgroup*8 ..] (u64, 100 MHz); NULL turns it off. */
int blim_debug_gemm_stamps(void* device_buf);

/* "precise" (0/1, fp16 and bf16 engines; fp8 engines refuse it): compensated arithmetic for the following calls (activations as hi + lo,
 *   GEMMs walk K twice): ~21 significant bits per activation on fp16 engines, 16 on bf16 engines (against exact bf16 weights: VTG 2e-6 / TVG
 *   <= 7e-4 from the fp32 reference at 28 layers of the 7B configuration).  The host turns it on for the TVG calls of both dtypes and for the
 *   VTG calls of bf16 engines -- the mode in which BASELINE.json's named dtype holds the 1e-3 bar (blim_amd/modeling.py: vtg_precise);
 * "precise_embeds" (0/1): in precise mode the input embeddings / projector outputs are [hi | lo] rows of width 2 * hidden as well;
 * "precise_mlp" (0/1, default 1): 0 leaves the MLP branch plain in precise mode -- the TVG calls' "attn" mode (1.6x faster than fully compensated; TVG deviation at
 *   7B depth 8e-4 instead of 4e-5 on Gaussian weights, 3e-3 on weights with massive activations: `--tvg_precise auto` measures which one a checkpoint needs);
 * "precise_layers" (0/1, default 0; 16-bit engines) and "precise_layer_bits" (value = (layer << 4) | bits, 0 <= layer < num_layers; every layer starts at 15):
 *   a per-layer compensation mask for precise mode (`--vtg_precise select`).  With "precise_layers" = 1, layer `layer`'s units run compensated where its bits are
 *   set -- bit 0 the QKV GEMM and the attention's three-term products, bit 1 o_proj, bit 2 gate|up, bit 3 down -- and plain elsewhere: the call keeps precise
 *   mode's [hi | lo] buffer layout, a plain unit's GEMM reads only the hi halves and the unit's producer (RMSNorm, QKV epilogue, attention, SwiGLU epilogue)
 *   writes no lo part for it.  The embeddings, the final norm and lm_head stay compensated; "precise_mlp" is ignored while the mask is on.  All bits set
 *   computes what precise mode computes, bit for bit.  fp8 engines refuse both;
 * "precise_lo6" (0/1; 16-bit engines with hidden / intermediate sizes that are multiples of 128.  fp16 engines: default 1, env BLIM_PRECISE_LO6=0 turns it off.  bf16 engines
 *   (round 6): default 0 -- their parity mode walks K a second time in bf16, 1 - 3e-6 at 7B depth -- and 1 is an opt-in (env BLIM_PRECISE_LO6=1, `--second_pass e2m3 | auto`):
 *   a bf16 value's lo part is 2^-9 of it, hi + e2m3(lo) carry about what one fp16 rounding keeps: VTG scores 3 - 7e-5 from the fp32 reference at 7B depth on N(0, 0.02^2)
 *   weights at 1.41x the rate of the bf16 second pass.  Set it before loading adapters (their K extension is 128 columns when the option may be used).  fp8 engines refuse 1):
 *   in precise mode the decoder GEMMs' (and lm_head's) second walk over K -- the product of W with the activations' LO parts, 2^-11 of the values -- runs on the
 *   block-scaled MFMA with e2m3 operands (6 bits, one power-of-two scale per 32 values: four times the 16-bit MFMA rate on gfx950), inside the same kernel and into
 *   the same accumulators.  Weights: e2m3 tile images built on the first compensated call (+0.78 byte per decoder / head weight: 5.9 GB at 7B; a failed allocation
 *   is BLIM_ERR_NOMEM with the matrix named); activations: the lo parts a producer wrote are re-written as operand tiles (one HBM-bound pass per GEMM input).  A
 *   fully compensated call costs 1.49x a plain one instead of 2x and stays within 4e-5 of the fp32 reference where the fp16 second pass reads 4e-6 (28 layers of
 *   the 7B configuration); on weights with a trained checkpoint's massive activations the two differ by <= 1.6e-4 over 16,000 scores (rms 9e-6);
 * "narrow_gemm" (0 / 1 / 2, default 0; other values BLIM_ERR_ARG): blim_gemm's `tile` for the decoder layers' o_proj and down launches -- the plain and the w_wrap_k
 *   forms, adapters apart and the last layer's pruned rows included; 1 = auto, 2 = wherever the form is eligible.  Launches of an ineligible form (fp8 engines, the e2m3
 *   second pass of "precise_lo6") keep the 256 x 256 kernel.  The option changes NO value (the narrow kernel's results are the 256 x 256 kernel's bit for bit), only which
 *   kernel computes it: it is no part of a prefix cache's snapshot of the numeric options, of the calibration store's key or of the weights fingerprint;
 * "narrow_lo6" (0 / 1 / 2, default 0; other values BLIM_ERR_ARG): blim_gemm's `tile_lo6` for the same launches where they carry the e2m3 second pass of "precise_lo6"
 *   (the compensated o_proj and down of fp16 engines, of bf16 engines under "precise_lo6" = 1); 1 = auto, 2 = wherever the form is eligible.  Every other launch is
 *   untouched: the plain and w_wrap_k forms stay "narrow_gemm"'s, fp8 engines keep the 256 x 256 kernel.  Like "narrow_gemm" it changes NO value and is no part of a
 *   prefix cache's snapshot, of the calibration store's key or of the weights fingerprint;
 * "narrow_qkv" (0 / 1 / 2, default 0; other values BLIM_ERR_ARG): blim_gemm's `tile_qkv` for the decoder layers' QKV projection in blim_score, blim_score_cached, blim_hidden
 *   and blim_decode (the trainer's launch is untouched): plain, w_wrap_k and e2m3 second-pass forms alike, adapters apart included; 1 = auto, 2 = wherever the form is
 *   eligible; fp8 engines keep the 256 x 256 kernel.  Like "narrow_gemm" it changes NO value -- q, k and v, and with them the K / V a prefix cache captures, are the
 *   same bits -- and is no part of a prefix cache's snapshot, of the calibration store's key or of the weights fingerprint;
 * "masked_query_zero" (0/1, default 0; 16-bit engines; PARITY-UNPINNED): query positions the key mask hides (blim_batch.key_visible == 0) write a ZERO attention output
 *   instead of attending to their visible keys.  The default is the semantics parity is pinned to -- the reference's eager / SDPA attention classes
 *   (modeling_qwen2_flash.py:288-310, 701-709), where a masked query row is computed like any other.  Its flash-attention-2 class drops such positions before the
 *   kernel and pads zeros back (modeling_qwen2_flash.py:526-563); main.py:96 passes no attn_implementation, so which class a real run used depends on the
 *   checkpoint's config and on whether flash-attn was installed (setup.sh:7).  The only scores that differ are the TVG-CPN prior's (its first gathered row is a
 *   masked position: modeling_videochat_flash.py:414-417).  flash-attn cannot be imported in the build environment: this option restates those lines, it is not
 *   checked against a recorded run (tests/test_gpu_parity.py::test_masked_query_zero_option_matches_its_restatement);
 * "prune_last" (0/1, default 1): calls that name the rows they read (blim_decode with out_rows, blim_score_*) run the LAST layer's o_proj / norm / MLP
 *   on those rows only (same values bit for bit; the other rows' K / V are still produced); after such a call the "resid" / "attn" / "act" workspaces of
 *   blim_debug_read hold the last layer's state of the live rows only -- bring-up code reads them after calls without out_rows, or sets 0;
 * "f8_fuse" (0/1, fp8 engines): quantise the attention / SwiGLU outputs inside their producers (default 1);
 * tuning switches: "attn_tr_read" (0/1); "f8_mask" (BLIM_COMPUTE_F8 engines: which GEMMs take fp8 operands, bit 0 qkv, 1 o_proj,
 * 2 gate|up, 3 down, 4 lm_head; default 31 = all; the others run in fp16 from the retained 16-bit weights) */
int blim_set_option(blim_engine* e, const char* key, int32_t value);

/* ------------------------------------------------------------------------------------------------------------------
 * Offline feature extraction: the UMT-L vision encoder + ToMe token merging that produce the
 * ./data/<DS>/features/<vid>.pth files the scoring path reads.  Replaces model.encode_video_image(video, ...,
 * return_video_feature=True) as extract.py:104 calls it (modeling_videochat_flash.py:126-181 -> UMTVisionTower.forward,
 * vision_tower_builder.py:558-571 -> ToMe16_mlp_hd64.forward(compress=True, local_num_frames=4, return_video_feature=True),
 * mm_projector_builder.py:134-154).  A separate handle: extraction needs no language-model weights. */
typedef struct blim_vision blim_vision;
typedef struct blim_vision_config {
    int32_t image_size;    /* 448 ("umt-hd", vision_tower_builder.py:613-614) */
    int32_t patch_size;    /* 16 */
    int32_t num_frames;    /* frames per clip = mm_local_num_frames (4) */
    int32_t hidden_size;   /* 1024 */
    int32_t num_heads;     /* 16 (head_dim must be 64) */
    int32_t mlp_hidden;    /* 4096 */
    int32_t depth;         /* blocks actually run: encoder_depth 24 + mm_vision_select_layer (-2) + 1 = 23 (vision_tower_builder.py:293) */
    int32_t tome_tokens;   /* tokens per clip after merging: 16 * num_frames = 64 (mm_projector_builder.py:147) */
    int32_t compute_dtype; /* BLIM_COMPUTE_F16 / BLIM_COMPUTE_BF16: format of the GEMM / attention operands (residual stream, LayerNorm and ToMe are f32) */
} blim_vision_config;
int blim_vision_create(const blim_vision_config* cfg, blim_vision** out);
void blim_vision_destroy(blim_vision* v);
/* names: vit.patch.{w,b}, vit.blocks.N.{norm1,norm2}.{w,b}, .q_bias, .v_bias, .qkv.w, .proj.{w,b}, .fc1.{w,b}, .fc2.{w,b}, vit.norm.{w,b}
 * (blim_amd/vision.py:vision_weight_shapes); natural [out, in] layout, f32 or bf16, host or device. */
int blim_vision_load_weight(blim_vision* v, const char* name, const void* data, int32_t dtype, int32_t on_device);
int blim_vision_init_synthetic_weights(blim_vision* v, uint64_t seed);
/* HOST f32 [num_frames * (image_size/patch_size)^2, hidden]: the sinusoidal position table (vision_tower_builder.py:222-269),
 * computed by the host (blim_amd/vision.py:pos_embed). */
int blim_vision_set_pos_embed(blim_vision* v, const float* table_host);
int blim_vision_ready(const blim_vision* v);
/* frames: device 16-bit (compute dtype) [n_clips, num_frames, 3, S, S], normalised pixels.  out_feat (may be NULL): f32
 * [n_clips, L, hidden] encoder output, L = num_frames * (S/patch)^2; out_tome (may be NULL): f32 [n_clips, tome_tokens, hidden]. */
int blim_vision_encode(blim_vision* v, const void* frames, int32_t n_clips, float* out_feat, float* out_tome, void* stream);
/* The encoder's attention alone (tests / bench): qkv 16-bit [n_clips * L, 3 * heads * 64] = [q | k | v] per token, heads of 64; out 16-bit
 * [n_clips * L, heads * 64] = softmax(q k^T / 8) v within each clip, non-causal (vision_tower_builder.py:100-128). */
int blim_vit_attention(const void* qkv, int32_t n_clips, int32_t L, int32_t heads, int32_t dtype16, void* out, void* stream);
/* ToMe alone: x f32 [b, p, c] (c = heads * 64) -> out f32 [b, target, c]; bipartite soft matching + size-weighted merge,
 * mm_projector_builder.py:6-130. */
int blim_tome_merge(blim_vision* v, const float* x, int32_t b, int32_t p, int32_t c, int32_t heads, int32_t target, float* out, void* stream);

/* Frame preprocessing in front of blim_vision_encode (csrc/preprocess.hip): UMTImageProcessor.preprocess for uint8 RGB frames -- PIL's
 * bicubic resize to S x S, x 1/255, mean / std -- with the host path's values bit for bit.  PIL's 8-bit resampler is integer arithmetic on 22-bit fixed-point
 * coefficients, and the normalisation sees 3 x 256 distinct inputs, so the host supplies the taps and a table (blim_amd/vision.py: bicubic_tables,
 * normalise_lut) and the device does no float arithmetic at all.  The rule:
 *   horizontal pass, per output pixel x and channel: acc = 1 << 21; acc += xk[x][i] * pixel[first + i] for i < count, in int32, (first, count) = xb[x];
 *     byte = clip(acc >> 22, 0, 255) with an arithmetic shift, stored into the workspace [T, H, S, 3];
 *   vertical pass: the same rule down the workspace's rows with yb / yk, then out[t, c, y, x] = lut[c][byte];
 *   a pass whose input size equals S is skipped (W == S: no workspace, the frames feed the vertical pass; H == S: the bytes go to the table unchanged), as PIL
 *   skips it.
 * Two launches on `stream`; no engine handle.  blim_preprocess_workspace_bytes: T * H * S * 3, or 0 when W == S; BLIM_ERR_ARG for sizes outside the limit.
 * Refused before anything is launched (BLIM_ERR_ARG, the message names the problem): T, H, W or S outside 1 .. 8192; a null frames, lut or out; a pass that
 * runs without its bounds, its coefficients or (horizontal) the workspace, or with xks / yks < 1.  The tables are trusted to keep first + count <= the input
 * size and count <= xks / yks (the host asserts it before the upload); a table that broke this is clamped to the row, so it reads nothing outside the frames. */
int64_t blim_preprocess_workspace_bytes(int32_t T, int32_t H, int32_t W, int32_t S);
int blim_preprocess_frames(const uint8_t* frames,              /* [T, H, W, 3] RGB */
                           int32_t T, int32_t H, int32_t W, int32_t S,
                           const int32_t* xb, const int32_t* xk, int32_t xks,   /* horizontal: bounds [S, 2] = (first tap, tap count), coefficients [S, xks]; ignored when W == S */
                           const int32_t* yb, const int32_t* yk, int32_t yks,   /* vertical, likewise; ignored when H == S */
                           const uint16_t* lut,                /* [3, 256] 16-bit patterns: channel c, byte v -> output value */
                           void* out,                          /* [T, 3, S, S] 16-bit, the layout blim_vision_encode reads */
                           void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fine-tuning step: what training_utils.py:57-95 does per batch -- the reference's two decoder forwards (VTG rows, TVG rows;
 * here one forward over a packed batch holding both), loss = vtg_loss + tvg_loss, backward into the LoRA adapters of main.py:96-101 (projector mlp / tvg_mlp Linear 0 and 2, every
 * q/k/v/o_proj, lm_head; y = W x + b + alpha/r * B A dropout(x)) and the fp32 visual_head (main.py:104-107), AdamW (main.py:147).
 * Base weights stay frozen in the engine.  The trainable tensors live in ONE flat f32 device buffer owned by the caller (so that the
 * host can all-reduce the matching gradient buffer over RCCL in one call, as DistributedDataParallel does for the reference,
 * main.py:141-143); tensor order: blim_amd/lora.py:trainable_names, every tensor starting on a 64-element boundary. */
typedef struct blim_trainer blim_trainer;
typedef struct blim_train_config {
    int32_t lora_r;       /* main.py --lora_r (8); <= 16 */
    float lora_alpha;     /* --lora_alpha (32) */
    float lora_dropout;   /* --lora_drop (0.05): dropout on the adapters' input, counter-based mask per (step seed, adapter, token, column) */
} blim_train_config;
/* number of f32 elements of the flat parameter / gradient / moment buffers */
int64_t blim_train_flat_size(const blim_engine* e, int32_t lora_r);
/* name = "<weight>:A" | "<weight>:B" | "visual_head" (weights: mlp.{0,2}.w, tvg_mlp.{0,2}.w, lm_head, layers.N.{q,k,v,o}_proj.w) */
int blim_train_param_offset(const blim_engine* e, int32_t lora_r, const char* name, int64_t* offset, int64_t* rows, int64_t* cols);
/* params / grads: device f32 [blim_train_flat_size].  Builds the training copies of the frozen weights (K-augmented copies that
 * carry the adapters' B matrices as 64 extra K columns, and transposed copies for the input-gradient GEMMs). */
/* (An fp8 engine accepts a trainer for loading and MERGING adapters only -- evaluating a fine-tuned checkpoint in fp8 mode; blim_train_step refuses it.) */
int blim_train_create(blim_engine* e, const blim_train_config* cfg, float* params, float* grads, blim_trainer** out);
void blim_train_destroy(blim_trainer* t);
/* after `params` changed (load, optimizer step): refresh the 16-bit copies the forward reads */
int blim_train_sync_params(blim_trainer* t, void* stream);
/* write W + alpha/r * B A (and visual_head) into the ENGINE's scoring weights: evaluation between epochs (main.py:166) sees the
 * fine-tuned model; always merged from the pristine base, so it can be called repeatedly.  BLIM_ERR_STATE while the engine holds adapters apart
 * (blim_load_adapter): one or the other. */
int blim_train_merge(blim_trainer* t, void* stream);
typedef struct blim_train_batch {
    const blim_batch* batch;      /* ONE packed batch holding the VTG rows and the TVG rows (either part may be absent), no shared prefixes */
    const int32_t* src_index;     /* [T] token id >= 0, or -(f + 1): f < n_feat_rows = row f of the `mlp` projection (a VTG row's video token),
                                   * f >= n_feat_rows = clip mean f - n_feat_rows of the `tvg_mlp` projection (a TVG row's clip token) */
    const void* feats;            /* 16-bit [n_feat_rows, mm_hidden]: raw features of the batch's videos, video-major */
    int64_t n_feat_rows;
    int32_t tok_per_clip;         /* rows averaged per clip for the TVG tokens (modeling_videochat_flash.py:243) */
    int32_t max_seq_len;          /* longest row of the batch */
    const int32_t* rows;          /* VTG: [n_rows] token rows whose next-token label is scored */
    const int32_t* labels;        /* VTG: [n_rows] target token ids */
    int64_t n_rows;
    const int32_t* tvg_rows;      /* TVG: [n_samples * num_clips] rows predicting clip c (training_utils.py:73) */
    const int32_t* tvg_labels;    /* TVG: [n_samples] index of the sample's video in the vocabulary */
    int64_t n_tvg_rows;
    const void* vocab;            /* TVG: 16-bit clip-major [num_clips][n_vocab][mm_hidden] */
    int32_t n_vocab;
    float grad_scale;             /* upstream gradient of both losses (AMP loss scale / accum_iter) */
    uint64_t dropout_seed;
} blim_train_batch;
/* training_utils.py:57-85 for one batch: forward of both kinds of rows through the decoder in one pass, loss = vtg_loss + tvg_loss, backward;
 * gradients ACCUMULATE into `grads` (scaled by grad_scale); loss_sums[0] += the summed negative log-likelihood over the n_rows VTG label rows,
 * loss_sums[1] += the same over the n_tvg_rows TVG rows (device f32 [2]; the mean losses of training_utils.py:68 / :79 divide by the row counts) */
/* Reproducible bit for bit from run to run, like the reference's autograd on these shapes: every split reduction (adapter gradients over time
 * splits, du over column slices, the loss sums, the gradient norm) is summed from per-split partials in a fixed order -- no float atomics. */
int blim_train_step(blim_trainer* t, const blim_train_batch* b, float* loss_sums, void* stream);
/* stats[0] += sum((g * inv_scale)^2) over the flat gradient buffer, stats[1] = 1 if any element is inf / nan (device f32 [2]) */
int blim_train_grad_stats(blim_trainer* t, float inv_scale, float* stats, void* stream);
/* torch.optim.AdamW over the flat buffers (g = grad * inv_scale; decoupled weight decay on every tensor: all are 2-D, timm's
 * param_groups_weight_decay exempts only 1-D tensors); step counts from 1; calls blim_train_sync_params */
int blim_train_adamw(blim_trainer* t, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay, float inv_scale,
                     int32_t step, void* stream);
/* bring-up aid: copies a saved activation of the last forward ("res<l>" f32 [T,H], "qkv<l>", "attn<l>", "gu<l>", "dres" f32 [T,H]) */
int blim_train_debug_read(blim_trainer* t, const char* which, void* dst, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BLIM_H_ */
