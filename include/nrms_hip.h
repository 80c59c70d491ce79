/*
 * nrms_hip.h -- C ABI of libnrms_hip.so: the MI355X (gfx950) NRMS train/eval hot path.
 *
 * This is the drop-in boundary beneath the reference's Python plugin API
 * (model/__init__.py:22-23 `import_module('model.'+name).Model(config)`, called as
 * `outputs = model(datas)` at train_eval.py:111,242,323).  The reference has no native
 * layer; every entry point below names the reference lines whose ATen op sequence it
 * replaces (paths relative to /root/reference/MIND_2020/).
 *
 * Conventions
 *   - plain C: POD structs, raw DEVICE pointers, sizes; no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = the default stream).
 *   - the library allocates nothing and owns nothing: activations, gradients and workspace
 *     are caller buffers; workspace sizes come from the *_workspace_bytes queries.
 *   - every call is asynchronous on `stream`, re-entrant across streams, and returns
 *     0 on success or a negative NRMS_E* code; nrms_last_error() gives the (thread-local) text.
 *     Helper streams: nrms_encoder_bwd forks its weight-gradient GEMMs (and the fp16 calls their id-only / weight-only
 *     bookkeeping) onto two helper streams that belong to the pair (device, caller `stream`): created the first time that
 *     stream makes such a call, never shared between caller streams, forked from and joined back into `stream` with events
 *     inside the call -- before it returns, on the error paths too, or in nrms_encoder_bwd_wqkv under NRMS_FLAG_DEFER_WQKV.
 *     Several backwards may therefore be in flight in one process as long as they are on DIFFERENT streams (two engines on
 *     two streams train concurrently); calls on the SAME stream must be issued by one host thread at a time, as stream order
 *     demands anyway.  A pending deferred join (NRMS_FLAG_DEFER_WQKV, fp16) is flushed by the next nrms_encoder_fwd /
 *     nrms_encoder_bwd on that stream in ANY precision, so a caller that never calls nrms_encoder_bwd_wqkv still gets
 *     correct ordering (NRMS_FLAG_DEFER_USER_JOIN: see the flag for where its join happens).  The environment variable
 *     NRMS_NO_SIDE_STREAMS keeps everything on `stream`.
 *   - all matrices are row-major and dense; fp32 unless stated.  M = n_seq * seq_len.
 *   - gradients are ACCUMULATED (+=) into the caller's buffers (zero them per step, as
 *     `model.zero_grad()` does at train_eval.py:115).
 */
#ifndef NRMS_HIP_H
#define NRMS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRMS_OK            0
#define NRMS_EINVAL       -1   /* bad dims / null pointer / unsupported shape */
#define NRMS_ELAUNCH      -2   /* HIP launch or runtime error */
#define NRMS_EWORKSPACE   -3   /* workspace too small */

#define NRMS_PRECISION_FP32   0 /* f32-input MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2_f32): exact fp32 */
#define NRMS_PRECISION_BF16X3 1 /* dense projections as split-bf16: x = hi + lo, hi*hi + hi*lo + lo*hi on
                                   v_mfma_f32_16x16x32_bf16, fp32 accumulate (~2^-16 relative per product);
                                   attention, softmaxes, pooling, loss, optimizer and all HBM tensors stay fp32 */
#define NRMS_PRECISION_BF16   2 /* same kernels, hi*hi only: plain bf16 inputs, fp32 accumulate */
#define NRMS_FP16_KP 320        /* fp16 mode: pitch of x (input features, zero padded) */
#define NRMS_FP16_DP 320        /* pitch of ctx (32 per head, zero padded) */
#define NRMS_FP16_QP 224        /* pitch of t */
#define NRMS_PRECISION_FP16   3 /* fused path: one wavefront per sequence, every contraction on v_mfma_f32_32x32x16_f16
                                   (fp16 operands: 11 significant bits, fp32 accumulate), Q/K/V, attention probabilities
                                   and tanh(.) register-resident, activations kept for the backward in fp16.
                                   Restrictions: seq_len <= 64, d_model <= 316, d_k <= 32, n_heads <= 10, q_dim <= 224,
                                   no output projection, no masks (NRMS_EINVAL otherwise).  With use_output_proj (the
                                   news encoder of nrms_v1, model/nrms_v1.py:109-162: heads wider than 32 + W_O,
                                   dropout after W_O): vocab > 0 with NRMS_FLAG_PAD_ROW_ZERO and no embedding dropout,
                                   seq_len <= 32, 32 < d_k <= 50, 3 n_heads + 1 <= 19, n_heads (d_k - 48) <= 16,
                                   d_model <= 316 a multiple of 10 (d_model / 10 <= 32), q_dim <= 224; the context
                                   dropout then acts on the ten [d_model / 10]-wide blocks of the projection's output
                                   (same padded [M, 320] counter layout).  Activation buffers change
                                   meaning (see nrms_encoder_acts); context-dropout counters run over the padded
                                   [M, NRMS_FP16_DP] layout, 32 columns per head, in the 16-bit-field scheme
                                   (nrms_dropout_keep_mask with d = 320 and site 1 | NRMS_DROPOUT_FIELDS16). */

/* nrms_encoder_desc.flags */
/* The caller guarantees that row 0 of `table` (the padding row, nn.Embedding padding_idx=0,
 * nrms_v0.py:134-136) is all zeros.  A padding token's embedding is then exactly zero (also under
 * dropout), so its Q|K|V row is exactly the bias and it adds nothing to d(w_qkv): the projection and its
 * weight-gradient GEMM run on the non-padding tokens only.  Results are identical to the dense path.
 * The row keeps its value under training (its gradient is identically zero), so the flag is a property
 * of the loaded weights.  Ignored when vocab == 0. */
#define NRMS_FLAG_PAD_ROW_ZERO 1
/* nrms_encoder_bwd leaves d(w_qkv) / d(b_qkv) out (its step 5); the caller runs nrms_encoder_bwd_wqkv with the
 * same descriptor, activations and workspace afterwards.  Everything else, in particular the embedding-table
 * gradient, is complete when nrms_encoder_bwd returns: a data-parallel caller starts the all-reduce of the
 * table gradient (95 % of the gradient bytes) there and lets it run underneath the deferred GEMM.
 * NRMS_PRECISION_FP16: the weight-gradient GEMMs (d(w_qkv), d(b_qkv), d(w_add), d(b_add)) are already running on the
 * library's helper streams when nrms_encoder_bwd returns; with this flag the call does not wait for them (dx and the table
 * gradient are complete in stream order, those four are NOT) and nrms_encoder_bwd_wqkv orders them into the stream. */
#define NRMS_FLAG_DEFER_WQKV 2
/* nrms_encoder_bwd, NRMS_PRECISION_FP16 news encoder: `acts.scratch` is still exactly what the nrms_encoder_fwd call of this
 * step left in it (the caller has not passed that buffer to another forward in between).  The backward then reads the token
 * and title lists the forward built there (live rows, row positions, the three title classes) instead of rebuilding them
 * from the ids (five small launches).  Without the flag nothing in acts.scratch is read by the backward.  The promise is
 * checked on the host: the library remembers which forward (scratch, ids, n_seq, seq_len, ...) last built lists in a scratch
 * buffer and forgets it when ANY nrms_encoder_fwd is handed that buffer again; a backward whose arguments do not match the
 * record rebuilds the lists as if the flag were absent (correct results, five more launches). */
#define NRMS_FLAG_FWD_SCRATCH_KEPT 4
/* User encoder (vocab == 0), NRMS_PRECISION_BF16X3, 33 <= seq_len <= 64, d_model <= 300, even d_k <= 32, n_heads <= 10,
 * q_dim <= 224, no output projection, no mask, no dropout: the whole pass runs as ONE kernel per direction (csrc/user64.hip: a
 * wave per 32-row half of a history, Q / K / V / probabilities / tanh in registers, every product in split-bf16) instead of the
 * projection GEMM -> attention -> additive-attention chain; the weight-gradient and dX GEMMs of the backward are unchanged.
 * Under the flag acts.qkv is NOT [M, 3d] floats but nrms_encoder_fused_qkv_bytes(desc) bytes of operand fragments (internal
 * layout, written by the forward, read by the backward); acts.ctx, acts.t, acts.w keep their meaning (and may all be NULL in
 * inference).  Set on both nrms_encoder_fwd and nrms_encoder_bwd of a pass, or on neither; NRMS_EINVAL for any other shape. */
#define NRMS_FLAG_FUSED_SEQ64 8
/* nrms_encoder_bwd, user encoder (vocab == 0) in fp32 / bf16x3 / bf16, with or without NRMS_FLAG_FUSED_SEQ64; ignored for every
 * other pass.  The call returns WITHOUT ordering `stream` behind the helper stream that runs its weight-gradient GEMMs: dx and
 * d(q_vec) are complete in stream order, d(w_qkv), d(b_qkv), d(w_add), d(b_add) (d(w_o), d(b_o)) are NOT -- nothing before the
 * optimizer reads them, and the next backward on the stream (the news encoder's) can start under them.  The contract:
 *   - until the join, the caller leaves alone everything those GEMMs read: `workspace` (dQKV, ds, the partial slabs), `x`, the
 *     saved activations and w.q_vec.  In particular the next nrms_encoder_bwd on the stream needs ANOTHER workspace buffer.
 *   - the join is the end of the next NRMS_PRECISION_FP16 nrms_encoder_bwd without use_output_proj on the stream (or, where that
 *     call carries NRMS_FLAG_DEFER_WQKV, its nrms_encoder_bwd_wqkv); any other nrms_encoder_fwd / nrms_encoder_bwd /
 *     nrms_encoder_bwd_wqkv on the stream joins when it STARTS; nrms_encoder_join does it for a caller that has neither.
 *   - an error return has joined already.  With NRMS_NO_SIDE_STREAMS there is nothing to join. */
#define NRMS_FLAG_DEFER_USER_JOIN 16

/* nrms_encoder_bwd_adam, news encoder (vocab > 0) whose table gradient is the grouped scatter (NRMS_PRECISION_FP16: with
 * NRMS_FLAG_PAD_ROW_ZERO; fp32 / bf16x3 / bf16: always, unless the environment asks for the atomic scatter): the kernel that sums
 * a table row's gradient applies Adam to that row at once, from the operands in nrms_table_adam.  Every row of the table is
 * updated -- rows without a token in the batch and row 0 with the gradient +0 -- with the bits of
 *     zeroed grads.table -> nrms_encoder_bwd -> nrms_adam_step[_guarded](vocab * d_model, table, grads.table, ...),
 * grads.table is WRITTEN (not accumulated: it needs no zero fill and holds the gradient the optimizer consumed), and the table
 * is modified when the call returns: the caller runs the optimizer over the remaining parameters only (nrms_adam_step_rest).
 * For a caller whose table receives exactly this one scatter per step and whose gradient needs no reduction before the optimizer.
 * No kernel of the library reads the table while the update runs: within a backward only the forward's gather does, and the
 * weight-gradient GEMMs still on the helper streams read the saved activations and the workspace.
 * NRMS_EINVAL: vocab == 0, flags that make the table gradient another kernel, together with NRMS_FLAG_DEFER_WQKV, or through
 * nrms_encoder_bwd (which has no operands for it). */
#define NRMS_FLAG_TABLE_ADAM 32

/* One self-attention + additive-pooling encoder pass over n_seq sequences of seq_len rows.
 * vocab > 0  : news encoder -- input is `ids` [n_seq, seq_len] int64, rows gathered from
 *              `table` (NewsEncoder.forward, model/nrms_v0.py:154-176).
 * vocab == 0 : user encoder -- input is `x` [n_seq, seq_len, d_model]
 *              (UserEncoder.forward, model/nrms_v0.py:188-199). */
typedef struct nrms_encoder_desc {
    int32_t  n_seq;        /* titles (B*(H+C)) or users (B); n_seq * seq_len < 2^31 rows.  Every row index of the fp32 / bf16x3 /
                              bf16 chain is exact over that whole range (csrc/rowdiv.h), and every width up to d_model = 1024 at
                              every seq_len is addressed exactly (the 32 x 32 attention tiles pack their offsets only where they
                              fit): tests/test_hip_extents.py runs 9 M rows and d_model 672 ... 1024 against float64 */
    int32_t  seq_len;      /* L or H, 1..64 */
    int32_t  d_model;      /* config.word_embed_size (nrms_naml user encoder: news_feature_size); multiple of 4, <= 1024 */
    int32_t  n_heads;      /* config.num_attention_heads (v1 / naml news encoder: title_heads_num; naml user encoder:
                              user_heads_num); d_k = d_model / n_heads <= 128.  Even d_k <= 64 runs on the MFMA attention
                              kernels, anything else on the shape-general fp32 kernel (csrc/wide.hip) */
    int32_t  q_dim;        /* config.query_vector_dim (naml user encoder: query_vector_dim_large), multiple of 4, <= 512;
                              above 256 (or d_model > 512) acts.t is required in inference too */
    int32_t  vocab;        /* rows of `table`, or 0 */
    float    p_drop_embed; /* dropout on the gathered embeddings (nrms_v0.py:137); 0 in eval / nrms_v1 */
    float    p_drop_ctx;   /* dropout on the attention output (nrms_v0.py:171-173; nrms_v1.py:161 after W_O) */
    int32_t  precision;    /* NRMS_PRECISION_* */
    int32_t  use_output_proj; /* 1: nrms_v1 topology, MHSA ends in output_linear W_O (nrms_v1.py:55,80) */
    int32_t  mask_mode;    /* bit 0: pairwise attention mask mask_i*mask_j -> -1e9 (nrms_v1.py:27-33);
                              bit 1: additive-attention mask -> -1e9 (nrms_v1.py:100-101); 0 = nrms_v0 */
    int32_t  flags;        /* NRMS_FLAG_*; 0 = none */
    uint64_t seed;         /* counter-based RNG key for the dropout masks (per step) */
    float    loss_scale;   /* NRMS_PRECISION_FP16 backward only: the fp16 gradient tensors are carried multiplied by a
                              power of two and the results divided by it.  <= 0 (recommended): chosen on the device per
                              call as the power of two that puts max |dout| into [64, 128), so no loss reduction, batch
                              size or world size can overflow or flush the fp16 tensors -- 2^9 of head room for the tensors
                              derived from dout (dZ, d(ctx), dQKV, dX).  Weights of unusual norm can use that up: the
                              gradients then come out inf / nan, nrms_adam_step_guarded / nrms_grad_guard count them, and
                              the caller backs off with loss_scale = -n (a negative integer, n <= 24): n more powers of
                              two of head room, max |dout| into [64, 128) / 2^n.  > 0: used as given */
    float    p_drop_attn;  /* dropout on the attention PROBABILITIES (nrms_naml.py:36-39, dropout site 2; 0 in nrms_v0 /
                              nrms_v1); not combinable with NRMS_PRECISION_FP16.  With NRMS_FLAG_PAD_ROW_ZERO an
                              all-padding sequence keeps a closed form: context of query i = b_v x (kept keys of i) /
                              (seq_len (1 - p)) */
    const int32_t* seq_index; /* optional (device) [n_seq]: the call holds a COMPACTED batch and sequence r is sequence
                              seq_index[r] of the full one -- the attention-probability dropout then draws the full batch's
                              decisions (counters by seq_index[r], not r).  fp32 / bf16x3 / bf16 chain only, no embedding or
                              context dropout; null = 0 .. n_seq - 1.  See nrms_sequence_partition / nrms_encoder_empty_fwd */
} nrms_encoder_desc;

/* Parameters, in the reference's own tensor layout ([out,in] Linear weights).
 * w_qkv is W_Q.weight, W_K.weight, W_V.weight stacked on dim 0 (nrms_v0.py:35-37). */
typedef struct nrms_encoder_weights {
    const float* table;    /* [vocab, d]   news_encoder.word_embedding.0.weight, or NULL */
    const float* w_qkv;    /* [3d, d] */
    const float* b_qkv;    /* [3d] */
    const float* w_o;      /* [d, d]       output_linear.weight (nrms_v1.py:55) or NULL */
    const float* b_o;      /* [d] */
    const float* w_add;    /* [q, d]       additive_attention.linear.weight (nrms_v0.py:91) */
    const float* b_add;    /* [q] */
    const float* q_vec;    /* [q]          additive_attention.attention_query_vector (:92-93) */
} nrms_encoder_weights;

typedef struct nrms_encoder_grads {   /* same shapes as the weights; accumulated */
    float* table;          /* dense [vocab, d]; row 0 never written (padding_idx=0, nrms_v0.py:136) */
    float* w_qkv;
    float* b_qkv;
    float* w_o;            /* NULL unless use_output_proj */
    float* b_o;
    float* w_add;
    float* b_add;
    float* q_vec;
} nrms_encoder_grads;

/* Activations the forward saves for the backward (caller-owned).  In eval only `qkv`,
 * `ctx` (and `x` for the news encoder) are required scratch; `t` and `w` may then be NULL. */
typedef struct nrms_encoder_acts {
    float* x;              /* [M, d]   news encoder only: gathered word embeddings AFTER dropout
                                       (the user encoder's input is the caller's `x`); may be NULL if vocab==0.
                                       With NRMS_FLAG_PAD_ROW_ZERO only the non-padding tokens are stored, compact,
                                       in ascending token order (the buffer is still sized [M, d]) */
    float* qkv;            /* [M, 3d]  Q|K|V projections incl. bias, columns HEAD-MAJOR: head h occupies columns
                                       [3 d_k h, 3 d_k (h+1)) as Q | K | V (internal layout, read by the backward
                                       only).  With NRMS_FLAG_PAD_ROW_ZERO the rows of sequences that consist of
                                       padding only are left unwritten (the attention takes their closed form) */
    float* attn;           /* [M, d]   use_output_proj only: head-concatenated attention output (input of W_O) */
    float* ctx;            /* [M, d]   head-concatenated attention output AFTER dropout */
    float* t;              /* [M, q]   tanh(linear(ctx))            (nrms_v0.py:108) */
    float* w;              /* [M]      additive-attention softmax weights (nrms_v0.py:110-112) */
    void*  scratch;        /* nrms_encoder_fwd_scratch_bytes(desc) bytes: head-major W_qkv copy, bf16 weight planes,
                              token compaction lists */
    /* NRMS_PRECISION_FP16: x, ctx, t hold fp16 with the FIXED pitches KP = 320, DP = 320, QP = 224
     * (NRMS_FP16_KP / _DP / _QP):  x [M + 1, KP] (required for both encoders: gathered embeddings / the cast input),
     * ctx [Mp, DP] and t [Mp, QP] with Mp = n_seq * (seq_len <= 32 ? 32 : 64) rows (every sequence padded to whole
     * 32-row blocks, internal fragment order); w [M] fp32; qkv is unused (may be NULL); attn is unused unless
     * use_output_proj, then fp16 [Mp, DP] (the head concatenation in the operand order of the W_O tiles; read by the
     * backward's d(w_o) product). */
} nrms_encoder_acts;

/* Forward: embedding gather(+dropout) -> QKV projection -> per-head softmax(QK^T/sqrt(d_k))V
 * [-> output projection W_O] -> dropout -> tanh(linear)·q -> softmax over the sequence -> weighted sum.
 * Replaces model/nrms_v0.py:13-23,46-76,100-126,154-176,188-199 and, with use_output_proj / mask_mode,
 * model/nrms_v1.py:15-105,128-162,208-211.
 * out: [n_seq, d].  Exactly one of ids / x is used (by desc->vocab). */
size_t nrms_encoder_fwd_scratch_bytes(const nrms_encoder_desc* desc);
/* Size of acts.qkv under NRMS_FLAG_FUSED_SEQ64 (0 if the descriptor is not eligible for it). */
size_t nrms_encoder_fused_qkv_bytes(const nrms_encoder_desc* desc);
int nrms_encoder_fwd(const nrms_encoder_desc* desc, const nrms_encoder_weights* w,
                     const int64_t* ids, const float* x, const uint8_t* mask /* [n_seq, seq_len] or NULL */,
                     const nrms_encoder_acts* acts, float* out, void* stream);

/* Backward of the above (autograd through the same lines; `loss.backward()` train_eval.py:126).
 * dout: [n_seq, d].  grads: accumulated.  dx: [M, d] gradient w.r.t. `x` (user encoder), or
 * NULL for the news encoder, whose input gradient is scatter-added into grads->table
 * (the dense embedding gradient the reference builds 55x per step).
 * workspace: nrms_encoder_bwd_workspace_bytes(desc) bytes, 256-byte aligned.  Nothing is assumed about its contents on entry and
 * nothing outside those bytes is touched (tests/test_hip_buffer_contracts.py).  News encoder: its last segment is the scratch
 * of the table-gradient scatter, 2 (vocab + 64) + max(M, ceil(vocab / 1024)) + 64 ints -- the histogram and cursors over the
 * vocabulary, then one region that holds the block totals of the scan over the vocabulary (one per 1024 ids) and afterwards the M
 * token buckets -- so the query also covers a large vocabulary with a tiny batch (vocab = 300 000, M = 8). */
size_t nrms_encoder_bwd_workspace_bytes(const nrms_encoder_desc* desc);
int nrms_encoder_bwd(const nrms_encoder_desc* desc, const nrms_encoder_weights* w,
                     const int64_t* ids, const float* x, const uint8_t* mask,
                     const nrms_encoder_acts* acts, const float* dout,
                     const nrms_encoder_grads* grads, float* dx,
                     void* workspace, size_t workspace_bytes, void* stream);
/* nrms_encoder_bwd with NRMS_FLAG_TABLE_ADAM: the Adam operands of the embedding table (see nrms_adam_step for their meaning). */
typedef struct nrms_table_adam {
    float*   param;        /* [vocab, d] the table itself (w->table, writable) */
    float*   exp_avg;      /* [vocab, d] */
    float*   exp_avg_sq;   /* [vocab, d] */
    double   lr, beta1, beta2, eps;
    int32_t  step;         /* 1-based */
    float    grad_scale;
    int32_t* n_nonfinite;  /* device int32 counter: the guarded update (nrms_adam_step_guarded); NULL: nrms_adam_step */
} nrms_table_adam;
/* table_adam non-NULL exactly when desc->flags has NRMS_FLAG_TABLE_ADAM; with NULL this is nrms_encoder_bwd.  n_seq == 0: the
 * table still takes its step (gradient +0). */
int nrms_encoder_bwd_adam(const nrms_encoder_desc* desc, const nrms_encoder_weights* w,
                          const int64_t* ids, const float* x, const uint8_t* mask,
                          const nrms_encoder_acts* acts, const float* dout,
                          const nrms_encoder_grads* grads, float* dx,
                          void* workspace, size_t workspace_bytes, const nrms_table_adam* table_adam, void* stream);
/* Step 5 of the backward on its own: d(w_qkv), d(b_qkv) += dQKV^T [X | 1] from the dQKV left in `workspace`
 * by nrms_encoder_bwd(desc with NRMS_FLAG_DEFER_WQKV) -- same desc, ids / x, acts, grads, workspace. */
int nrms_encoder_bwd_wqkv(const nrms_encoder_desc* desc, const int64_t* ids, const float* x,
                          const nrms_encoder_acts* acts, const nrms_encoder_grads* grads,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Orders `stream` behind whatever an earlier nrms_encoder_bwd on it left running on the helper streams (NRMS_FLAG_DEFER_WQKV in
 * the fp16 mode, NRMS_FLAG_DEFER_USER_JOIN).  A no-op when nothing is outstanding. */
int nrms_encoder_join(void* stream);

/* Word ids must lie in [0, vocab) before they reach nrms_encoder_fwd / _bwd: the kernels index the table, the
 * token histogram and the placement lists with the raw id.  nn.Embedding raises on an out-of-range index
 * (nrms_v0.py:134-139,166); this is the device-side counterpart for untrusted input:
 * dst[i] = src[i] if 0 <= src[i] < vocab, else 0 (the padding id); *n_bad += number of ids replaced
 * (device int32 the caller zeroes and reads back when it chooses to synchronise).  dst may alias src. */
int nrms_sanitize_ids(const int64_t* src, int64_t* dst, int64_t n, int32_t vocab, int32_t* n_bad, void* stream);
/* The same from int32 ids (a feed that keeps its ids in 32 bits moves half the bytes; the encoder entry points take the
 * validated int64 copy either way). */
int nrms_sanitize_ids_i32(const int32_t* src, int64_t* dst, int64_t n, int32_t vocab, int32_t* n_bad, void* stream);

/* Evaluation encodes every DISTINCT title once (get_news_vector, nrms_v0.py:278-289, is the reference's hook for
 * caching news vectors; an impression padded to max_candidate_size = 300 slots, data_handler.py:174-177, is mostly
 * padding and repeats).  Exact grouping of the n_titles rows of ids [n_titles, seq_len] (seq_len = 1 groups plain news
 * ids): inverse[t] = index in [0, *n_unique) of the group of row t, rep_rows[u] = one row of group u (groups are
 * numbered in arrival order, which may differ between runs; the groups themselves do not).  table: caller-provided
 * workspace of table_size int32, a power of two >= 2 * n_titles.  *n_unique is a device int32. */
int nrms_title_dedup(const int64_t* ids, int64_t n_titles, int32_t seq_len, int32_t* table, int64_t table_size,
                     int32_t* inverse, int32_t* rep_rows, int32_t* n_unique, void* stream);

/* Click scores: bmm(cand [B,C,d], user [B,d,1]) then masked_fill(mask==0, -1e9)
 * (DotProductClickPredictor, nrms_v0.py:205-216; mask nrms_v0.py:272-274).  mask may be NULL. */
int nrms_click_score_fwd(int32_t B, int32_t C, int32_t d, const float* cand, const float* user,
                         const uint8_t* mask, float* scores, void* stream);
/* The same scores with the candidate vectors named by row index into a table of news vectors instead of being
 * materialised: scores[b][c] = <news_vec[index[b*C + c]], user[b]> (the evaluation path: 300 candidate slots per
 * impression over a few thousand distinct news).  index: int32 [B*C], every entry in [0, n_vec). */
int nrms_click_score_indexed(int32_t B, int32_t C, int32_t d, const float* news_vec, int64_t n_vec, const int32_t* index,
                             const float* user, const uint8_t* mask, float* scores, void* stream);
/* dscores [B,C] -> dcand [B,C,d], duser [B,d] (masked slots receive no gradient). */
int nrms_click_score_bwd(int32_t B, int32_t C, int32_t d, const float* cand, const float* user,
                         const uint8_t* mask, const float* dscores, float* dcand, float* duser,
                         void* stream);

/* nn.CrossEntropyLoss with every label 0 (train_eval.py:63,116-117):
 * loss_sum[0] += sum_b -log_softmax(scores[b])[0]   (caller divides by the global batch),
 * dscores = (softmax(scores) - onehot0) * grad_scale (grad_scale = 1/B_global).
 * dscores may be NULL (loss only). */
int nrms_ce_loss_fwd_bwd(int32_t B, int32_t C, const float* scores, float* loss_sum,
                         float* dscores, float grad_scale, void* stream);

/* torch.optim.Adam defaults (train_eval.py:48,127): one fused pass over a flat fp32 buffer.
 * g is multiplied by grad_scale first (1/world_size after a summing all-reduce).
 * step is 1-based.  lr / betas / eps are doubles, as torch holds them (1 - beta is rounded to fp32 once). */
int nrms_adam_step(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                   double lr, double beta1, double beta2, double eps, int32_t step, float grad_scale,
                   void* stream);

/* The same update, but an element whose (scaled) gradient is inf or nan is left out -- param, exp_avg and exp_avg_sq keep
 * their values there, so one overflowing fp16 backward cannot poison Adam's moments for the rest of training -- and counted:
 * *n_nonfinite (device int32, caller-zeroed) += number of elements skipped.  The caller reads the counter when it chooses to
 * (asynchronously) and lowers the fp16 loss scale (nrms_encoder_desc.loss_scale = -n).  Data parallel: every rank applies
 * this to the same reduced gradient and skips the same elements. */
int nrms_adam_step_guarded(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                           double lr, double beta1, double beta2, double eps, int32_t step, float grad_scale,
                           int32_t* n_nonfinite, void* stream);
/* The optimizer step of the parameters BEHIND a table that nrms_encoder_bwd_adam updated: nrms_adam_step (n_nonfinite NULL) or
 * nrms_adam_step_guarded (non-NULL), same kernels and bits; its launch is recorded under the timer "rest_adam" (timers are read by
 * prefix; "adam" is the table's fused kernel on that path). */
int nrms_adam_step_rest(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        double lr, double beta1, double beta2, double eps, int32_t step, float grad_scale,
                        int32_t* n_nonfinite, void* stream);
/* For callers that run their own optimizer (torch.optim.Adam on the autograd path, train_eval.py:126-127): inf / nan elements
 * of grad [n] are replaced by 0 in place and counted into *n_nonfinite (device int32, caller-zeroed). */
int nrms_grad_guard(size_t n, float* grad, int32_t* n_nonfinite, void* stream);

/* Per-impression AUC of evaluate() (train_eval.py:219-227,255-271 + evaluation.py:26-27):
 * scores, labels [n_imp, max_c] (padded), lens [n_imp] = candidates actually shown;
 * auc[i] = roc_auc_score(labels[i,:lens[i]], scores[i,:lens[i]]) in float64 (NaN if one class only). */
int nrms_impression_auc(int32_t n_imp, int32_t max_c, const float* scores, const uint8_t* labels,
                        const int32_t* lens, double* auc, void* stream);

/* The four MIND scores per impression and the submission ranks of test(), in one pass (same inputs as
 * nrms_impression_auc; only the prefix n = min(lens[i], max_c) of a row counts; a label != 0 is a positive).
 * Every output is a nullable device pointer; at least one must be given (n_imp = 0: a no-op, any pointer may be null).
 *   auc    [n_imp] f64: bit-identical to nrms_impression_auc (NaN when the prefix holds one class only).
 *   mrr    [n_imp] f64: sum over positives of 1 / rank_m, over n_pos.
 *   ndcg_a [n_imp] f64: sum over positives with rank_m <= k_a of 1 / log2(rank_m + 1), over
 *                       sum_{r=1}^{min(n_pos, k_a)} 1 / log2(r + 1)  (k_a > n: the whole prefix).  ndcg_b: k_b.
 *          MRR and nDCG are NaN when the prefix has no positive or holds a NaN score.
 *   ranks  [n_imp, max_c] i32: the rank (1 = best) of each shown candidate, 0 past the prefix.
 * Tie rule.  The metrics rank among equal scores the LATER slot first (np.argsort(s, kind="stable")[::-1], the
 * reference's mrr_score / ndcg_score whenever its sort keeps equal keys in index order):
 *     rank_m(i) = 1 + #{j : s_j > s_i} + #{j > i : s_j == s_i}.
 * The submission ranks put the EARLIER slot first (np.argsort(-s, kind="stable"), train_eval._cal_test), NaN after
 * every number and NaNs in slot order:  rank_s(i) = 1 + #{j : s_j > s_i} + #{j < i : s_j == s_i}.
 * Counts are integers and the f64 sums have a fixed order: two runs are bit-identical. */
int nrms_impression_metrics(int32_t n_imp, int32_t max_c, const float* scores, const uint8_t* labels,
                            const int32_t* lens, int32_t k_a, int32_t k_b, double* auc, double* mrr, double* ndcg_a,
                            double* ndcg_b, int32_t* ranks, void* stream);

/* ---- Top-k retrieval over a whole catalogue (serving: "which k of all N items should user b see?") ----
 * For each user b < B: the k catalogue items n of largest score s(b, n) = user[b] . items[n], never forming the [B, N]
 * score matrix.  user [B, d], items [N, d] fp32 row-major; exclude [B, n_exclude] int64, nullable: ids that user b must
 * not get (duplicates allowed; ids outside [0, N) are ignored); top_scores [B, k] fp32, top_ids [B, k] int64.
 * Score.  One fp32 chain per (b, n): a single accumulator over all of d on v_mfma_f32_32x32x2_f32, no split-K (k order
 *   32m, 32m+16, 32m+1, 32m+17, ... in each whole block of 32, then 8g, 8g+4, 8g+1, ... in groups of 8 for the rest).  A returned score therefore has the same bits for the same
 *   (user row, item row) whatever B, N, k, the row's position, the exclude list or the run.
 * Eligible: n is not in exclude[b, :] and s(b, n) is not NaN.
 * Order.  Score descending (+inf first); equal scores put the SMALLER n first; -0.0 equals +0.0 (and is returned as +0.0).
 * Output.  Row b holds the first min(k, #eligible) items in that order; the remaining slots hold id -1 and score -inf.
 * Limits: 1 <= k <= 256, d >= 1, 0 <= N <= 0x7FFF0000, B >= 0; B = 0 is a no-op, N = 0 writes all-padding rows.
 * Workspace: nrms_topk_dot_workspace_bytes(B, N, d, k) bytes, 8-byte aligned, O(B * slices * k) (0 = arguments rejected).
 * Two kernels on `stream`, no host synchronisation. */
size_t nrms_topk_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items, const int64_t* exclude,
                  int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);

/* Top-k with a query per (user, item group): the catalogue is split into G groups and user b scores item n with the query
 * row of n's group, s(b, n) = query[b, g(n)] . items[n] (HieRec's hierarchical matching, whose user side depends only on the
 * candidate's (topic, sub-topic) pair: nrms_hier_query).  query [B, G, d], items [N, d] fp32 row-major, stored group after
 * group: group g is rows [group_ptr[g], group_ptr[g + 1]) (group_ptr int64 [G + 1], nondecreasing from 0 to N; groups may be
 * empty or of any length, nothing is padded by the caller).  item_ids int32 [N]: the id of each row, distinct, in [0, 2^31),
 * in any order; exclude [B, n_exclude] int64, nullable: ids (not rows) user b must not get (duplicates and ids that are no
 * item's are ignored).  top_scores [B, k] fp32, top_ids [B, k] int64 (item ids).
 * The contract of nrms_topk_dot, with ids in place of rows:
 * Score.  The chain of nrms_topk_dot for (query row, item row): its bits do not depend on B, N, k, G, the grouping of the
 *   other items, the item's row or the run.  With G = 1 and item_ids[n] = n the result is bit-identical to nrms_topk_dot.
 * Eligible: the id is not in exclude[b, :] and s(b, n) is not NaN.  Order: score descending, equal scores put the SMALLER id
 *   first, -0.0 equals +0.0 (returned as +0.0).  Output: the first min(k, #eligible) items, then id -1 / score -inf.
 * Limits: 1 <= k <= 256, d >= 1, G >= 1, B >= 0, 0 <= N and N + 32 G <= 0x7FFF0000; B = 0 is a no-op, N = 0 writes
 *   all-padding rows.  A group_ptr outside its contract reads no row outside [0, N) (groups are clamped), but the result is
 *   then unspecified.
 * Workspace: nrms_topk_grouped_dot_workspace_bytes(B, N, d, k, G) bytes, 16-byte aligned (0 = arguments rejected): the tile
 *   table of the grouped layout (each group padded to whole 32-row tiles, at most N / 32 + G tiles) and O(B * slices * k).
 * Three kernels on `stream`, no host synchronisation. */
size_t nrms_topk_grouped_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G);
int nrms_topk_grouped_dot(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, const float* query, const float* items,
                          const int32_t* item_ids, const int64_t* group_ptr, const int64_t* exclude, int32_t n_exclude,
                          float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);

/* A sectioned front page: per user the k best items of EVERY section of the catalogue in one call (serving: "the best k of sports,
 * of finance, of health, ... for user b"; csrc/topksec.hip; PARITY UNPINNED, the reference scores shown candidates only).
 * user [B, d], items [N, d] fp32 row-major, stored section after section: section g is rows [section_ptr[g], section_ptr[g + 1])
 * (section_ptr int64 [G + 1], nondecreasing from 0 to N; sections may be empty or of any length, nothing is padded by the caller).
 * item_ids int32 [N]: the id of each row, distinct, in [0, 2^31), in any order; bias [N] fp32 BY ROW (not by id), 4-byte aligned,
 * NULLABLE; exclude [B, n_exclude] int64, nullable: ids (not rows) user b must not get (duplicates and ids that are no item's are
 * ignored).  top_scores [B, G, k] fp32, top_ids [B, G, k] int64 (item ids).
 * It is nrms_topk_grouped_dot's contract with these changes:
 * One query per user.  Every section is scored with the user's own row, s(b, n) = user[b] . items[n], on the chain of
 *   nrms_topk_dot: the same bits, whatever B, N, k, G, slice_tiles, the sections, the item's row or the run.
 * Optional prior.  With bias the score is s' = s + bias[row]: ONE fp32 add on the finished accumulator, under the rules of
 *   nrms_topk_dot_biased: a NaN sum removes the item, -inf puts it last, a NULL or all-zero bias gives the same ids and score bits.
 * Selection per (user, section).  Row (b, g) of the outputs holds the first min(k, #eligible in section g) items of section g,
 *   ordered by score descending (+inf first), equal scores by the SMALLER id, -0.0 equals +0.0 (returned as +0.0); then id -1 /
 *   score -inf.  Eligible: the id is not in exclude[b, :] and the (biased) score is not NaN.  An empty section gives an all-padding
 *   row.
 * Limits: 1 <= k <= 256, d >= 1, 1 <= G <= 4096, B >= 0, 0 <= N and N + 32 G <= 0x7FFF0000, (int64) B * G * k <= 0x7FFFFFFF;
 *   slice_tiles is 0 (the library chooses) or in [1, 1 << 20]: the 32-row tiles per slice of the launch geometry, for tests and
 *   tuning, and ceil((N + 31 G) / 32 / slice_tiles) + G must not pass 65535 (never with 0).  B = 0 is a no-op, N = 0 writes
 *   all-padding rows.  A section_ptr outside its contract reads no row outside [0, N) (sections are clamped), but the result is
 *   then unspecified.
 * Consequences.  With G = 1, item_ids[n] = n and bias NULL the result is bit-identical to nrms_topk_dot.  Row (b, g) equals
 *   nrms_topk_dot_biased for user b over the rows of section g alone, rows renamed to ids (with ids ascending inside the section
 *   even the tie order).  The result does not depend on slice_tiles, B, the user's position in the batch, the order of the sections,
 *   the order of rows inside a section, what other sections hold, what the workspace held or the run.  The first k' columns of a
 *   call with k are the call with k' <= k.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_sections_dot: ..."); an undersized workspace
 *   returns NRMS_EWORKSPACE.
 * Workspace: nrms_topk_sections_dot_workspace_bytes(B, N, d, k, G, slice_tiles) bytes, 16-byte aligned (0 = arguments rejected):
 *   the tile table, the slice table, the sections' slice ranges and O(B * slices * k), all sized from bounds (at most
 *   (N + 31 G) / 32 tiles and ceil(tiles / slice length) + G slices), since the section lengths live on the device.
 * Three kernels on `stream`, no host synchronisation, no allocation; plain vector loads and stores, no atomics beyond the integer
 *   LDS counters of nrms_topk_dot's slice kernel. */
size_t nrms_topk_sections_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, int32_t slice_tiles);
int nrms_topk_sections_dot(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, int32_t slice_tiles, const float* user,
                           const float* items /* section after section */, const int32_t* item_ids, const int64_t* section_ptr,
                           const float* bias /* [N], by row, nullable */, const int64_t* exclude, int32_t n_exclude,
                           float* top_scores /* [B, G, k] */, int64_t* top_ids /* [B, G, k] */, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Exact rank of given items in nrms_topk_dot's order over the whole catalogue (evaluation: "at which position of all N items
 * does the model put the item user b clicked next?"), again without the [B, N] score matrix.  user [B, d], items [N, d] fp32
 * row-major; targets [B, T] int64: the items to rank (-1 is the padding value callers use); exclude [B, n_exclude] int64,
 * nullable, as nrms_topk_dot's; ranks [B, T] int32; target_scores [B, T] fp32, nullable.
 * Score, eligibility and order are nrms_topk_dot's: the same fp32 chain on v_mfma_f32_32x32x2_f32 per (user row, item row),
 *   one accumulator over all of d in the same k order, so the same bits; n is eligible if it is not in exclude[b, :] and
 *   s(b, n) is not NaN; score descending, equal scores put the SMALLER n first, -0.0 equals +0.0.
 * Rank.  For a valid target t = targets[b, j]:  ranks[b, j] = 1 + #{eligible n : (s(b, n), n) precedes (s(b, t), t)}, the
 *   1-based position t would have in nrms_topk_dot's row b were k unbounded; target_scores[b, j] = s(b, t) (-0.0 as +0.0).
 *   Targets do not remove each other: each is ranked against the whole eligible catalogue, duplicates get equal ranks.
 * Invalid targets.  A target outside [0, N), an excluded one and one whose score is NaN get rank 0 and score -inf.
 * Limits: 1 <= T <= 32, d >= 1, 0 <= N <= 0x7FFF0000, B >= 0, n_exclude >= 0; B = 0 is a no-op, N = 0 writes rank 0 / -inf
 *   everywhere.
 * Counts are integers: two runs are bit-identical, and the result does not depend on B, the user's position in the batch, T,
 *   the other targets, the launch geometry or what the workspace held.
 * Workspace: nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude) bytes, 8-byte aligned, O(B * (T + n_exclude))
 *   (0 = arguments rejected).  Three kernels on `stream`, no host synchronisation, no allocation. */
size_t nrms_rank_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude);
int nrms_rank_dot(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items, const int64_t* targets,
                  const int64_t* exclude, int32_t n_exclude, int32_t* ranks, float* target_scores, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- A per-item additive prior in retrieval and ranking (serving: popularity, freshness, editorial boosts, a global block-list;
 * PARITY UNPINNED, the reference scores shown candidates only) ----
 * nrms_topk_dot and nrms_rank_dot over s'(b, n) = s(b, n) + bias[n].  bias [N] fp32, 4-byte aligned, NULLABLE; every other
 * argument is the unbiased call's.
 * Score.  s(b, n) is nrms_topk_dot's chain, the same code and the same bits.  s'(b, n) is ONE fp32 addition, round to nearest,
 *   of bias[n] to the finished accumulator; it is never folded into the chain.  top_scores and target_scores carry s'.
 * Eligible: n is not in exclude[b, :] and s'(b, n) is not NaN.  A NaN bias[n] therefore removes item n for every user: this is
 *   the global block-list, and it is part of the contract.  In ranking such a target gets rank 0 / score -inf, and such an
 *   excluded id is taken out of nothing.  +inf + -inf is NaN and falls under the same rule.  A -inf bias leaves the item
 *   eligible (unless s is +inf or NaN): it comes last, its score -inf, ties among such items by the smaller n.
 * Everything else is the unbiased call's: order (s' descending, +inf first, equal s' put the SMALLER n first), -0.0 equals
 *   +0.0 and is returned as +0.0 (the sum is not inspected before the entry is formed), padding (-1 / -inf), invalid targets,
 *   limits, workspace alignment, and independence of B, the row's position, k, T, the launch geometry, what the workspace held
 *   and the run.
 * Consequences.  bias == NULL is the unbiased call, bit for bit (the same kernels are launched).  An all-zero bias gives the
 *   same ids, ranks and score bits: s + 0.0 differs from s only for s = -0.0, which is returned as +0.0 anyway.  A bias that is
 *   constant over n leaves ids and ranks as they are whenever the addition maps distinct scores to distinct sums and equal
 *   scores to equal sums (always, when scores and the constant are exact in fp32 with an exact sum); rounding may otherwise
 *   merge neighbouring scores into ties, which the id rule then decides.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_biased: ...", "rank_dot_biased: ...");
 *   a bias that is not 4-byte aligned is one of them.
 * Workspace: the _biased_workspace_bytes queries return exactly nrms_topk_dot_workspace_bytes(B, N, d, k) and
 *   nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude) (0 = arguments rejected); 8-byte aligned.
 * The same kernel counts as the unbiased calls, on `stream`, no host synchronisation, no allocation; plain vector loads and
 *   stores, no atomics beyond the integer counters of the unbiased kernels. */
size_t nrms_topk_dot_biased_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_biased(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                         const float* bias /* [N], nullable */, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                         int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);
size_t nrms_rank_dot_biased_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude);
int nrms_rank_dot_biased(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                         const float* bias /* [N], nullable */, const int64_t* targets, const int64_t* exclude,
                         int32_t n_exclude, int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- A per-user time window on the catalogue in retrieval and ranking (news expires: evaluation against the news that were live
 * at the moment of the click, serving with a request time per user; PARITY UNPINNED, the reference scores shown candidates only) ----
 * nrms_topk_dot_biased and nrms_rank_dot_biased over the items whose timestamp lies in the user's own interval.  item_time [N]
 * int32: one tick per item (any unit the caller likes); window [B, 2] int32: user b's interval [lo, hi) = [window[b, 0], window[b, 1]);
 * both REQUIRED and 4-byte aligned.  bias [N] fp32, 4-byte aligned, NULLABLE: NULL means no prior, s' = s.  Every other argument is
 * the biased call's.
 * Eligible: item n is eligible for user b iff window[b, 0] <= item_time[n] < window[b, 1], n is not in exclude[b, :] and s'(b, n)
 *   is not NaN.  The interval is half-open and compared as signed int32.  lo >= hi is the EMPTY window: row b is all padding
 *   (id -1 / score -inf) and every target of user b gets rank 0 / score -inf.  An item whose time is INT32_MAX is never eligible,
 *   for any window (hi <= INT32_MAX): this is the "not published" value.  INT32_MIN is an ordinary, earliest, tick.
 * Score, order and output.  s and s' are the biased call's, the same code and the same bits: the window never touches a score.
 *   Order (s' descending, +inf first, equal s' put the SMALLER n first), -0.0 equals +0.0 (returned as +0.0), padding (-1 / -inf),
 *   invalid targets (outside [0, N), excluded, NaN s': rank 0 / -inf), limits (1 <= k <= 256, 1 <= T <= 32, d >= 1,
 *   0 <= N <= 0x7FFF0000, B >= 0; B = 0 is a no-op, N = 0 writes padding / rank 0) are nrms_topk_dot_biased's and
 *   nrms_rank_dot_biased's.
 * Targets.  A target whose time is outside its user's window is invalid: rank 0 / score -inf.  A valid target is ranked against
 *   the items eligible for its user, so ranks[b, j] = 1 + #{n eligible for b : (s'(b, n), n) precedes (s'(b, t), t)}.  An excluded
 *   id outside the window is taken out of nothing.
 * Consequences.
 *   (a) With every window [INT32_MIN, INT32_MAX) and every time below INT32_MAX, ids, ranks and score bits equal the _biased
 *       call's with the same bias (NULL: the unbiased call's).
 *   (b) Row b equals nrms_topk_dot_biased at B = 1 for user b with bias'[n] = bias[n] (0 when bias is NULL) where
 *       window[b, 0] <= item_time[n] < window[b, 1] and NaN elsewhere; the same holds for the ranks and target scores of
 *       nrms_rank_dot_biased.  (With bias NULL, s + 0.0 differs from s only for s = -0.0, which is returned as +0.0 anyway.)
 *   (c) The ids nrms_topk_dot_windowed returns for user b get ranks 1 .. k, in order, from nrms_rank_dot_windowed with the same
 *       arguments, and the same score bits.
 *   (d) The result does not depend on the row order of the catalogue (items, bias and item_time permuted together, ids mapped
 *       back; the tie rule then speaks of the mapped ids only when scores tie), on B, the user's position in the batch, k, T, the
 *       launch geometry, the run or what the workspace held.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_windowed: ...", "rank_dot_windowed: ...");
 *   a NULL or misaligned item_time (N > 0) or window is one of them.  An undersized workspace returns NRMS_EWORKSPACE.  Nothing is
 *   launched after an error.
 * Workspace: the _windowed_workspace_bytes queries return exactly nrms_topk_dot_workspace_bytes(B, N, d, k) and
 *   nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude) (0 = arguments rejected); 8-byte aligned.
 * The same kernel counts as the unwindowed calls, on `stream`, no host synchronisation, no allocation; plain vector loads and
 *   stores, no atomics beyond the integer counters of the unwindowed kernels.  A wave whose 64 items are closed to all 32 users of
 *   its block loads no item row and runs no MFMA for that step: with a catalogue stored in time order, a narrow window costs little
 *   more than the items inside it.  The results are the same with that skip compiled out (csrc/topk_entry.h TK_WINDOW_SKIP). */
size_t nrms_topk_dot_windowed_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_windowed(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                           const float* bias /* [N], nullable */, const int32_t* item_time /* [N] */,
                           const int32_t* window /* [B, 2] */, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                           int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);
size_t nrms_rank_dot_windowed_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude);
int nrms_rank_dot_windowed(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                           const float* bias /* [N], nullable */, const int32_t* item_time /* [N] */,
                           const int32_t* window /* [B, 2] */, const int64_t* targets, const int64_t* exclude,
                           int32_t n_exclude, int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- A per-user set of item tags on the catalogue in retrieval and ranking (muted topics, "only what I follow", an edition, a
 * publisher block; PARITY UNPINNED, the reference has no catalogue retrieval) ----
 * nrms_topk_dot_biased and nrms_rank_dot_biased over the items whose tag the user allows.  item_tag [N] int32: one tag per item;
 * allow [B, W] uint32, W = ceil(n_tags / 32): tag t is allowed for user b iff bit t & 31 of allow[b * W + (t >> 5)] is set; the bits of
 * the last word at positions >= n_tags are ignored; both REQUIRED and 4-byte aligned.  bias [N] fp32, 4-byte aligned, NULLABLE:
 * NULL means no prior, s' = s.  Every other argument is the biased call's.
 * Eligible: item n is eligible for user b iff 0 <= item_tag[n] < n_tags, that tag is allowed for b, n is not in exclude[b, :] and
 *   s'(b, n) is not NaN.  A tag outside [0, n_tags) is open to nobody: -1 is the "untagged, never served" value.  An all-zero allow
 *   row is the EMPTY set: row b is all padding (id -1 / score -inf) and every target of user b gets rank 0 / score -inf.
 * Score, order and output.  s and s' are the biased call's, the same code and the same bits: the tags never touch a score.
 *   Order (s' descending, +inf first, equal s' put the SMALLER n first), -0.0 equals +0.0 (returned as +0.0), padding (-1 / -inf),
 *   invalid targets (outside [0, N), excluded, NaN s': rank 0 / -inf), limits (1 <= k <= 256, 1 <= T <= 32, d >= 1,
 *   0 <= N <= 0x7FFF0000, B >= 0; B = 0 is a no-op, N = 0 writes padding / rank 0) are nrms_topk_dot_biased's and
 *   nrms_rank_dot_biased's; 1 <= n_tags <= 512.
 * Targets.  A target whose tag is closed to its user is invalid: rank 0 / score -inf.  A valid target is ranked against the items
 *   eligible for its user, so ranks[b, j] = 1 + #{n eligible for b : (s'(b, n), n) precedes (s'(b, t), t)}.  An excluded id that is
 *   closed was never counted and is taken out of nothing.
 * Consequences.
 *   (a) With every tag in [0, n_tags) and every bit below n_tags set, ids, ranks and score bits equal the _biased call's with the
 *       same bias (NULL: the unbiased call's).
 *   (b) Row b equals nrms_topk_dot_biased at B = 1 for user b with bias'[n] = bias[n] (0 when bias is NULL) where n is open to b
 *       and NaN where it is closed; the same holds for the ranks and target scores of nrms_rank_dot_biased.  (With bias NULL,
 *       s + 0.0 differs from s only for s = -0.0, which is returned as +0.0 anyway.)
 *   (c) Row b depends on user row b and allow row b only: not on B, the row's position in the batch, the other users' sets, the
 *       ignored bits, the launch geometry, what the workspace held or the run.
 *   (d) The first k' columns of a call with k are the call with k'.
 *   (e) The ids nrms_topk_dot_tagged returns for user b get ranks 1 .. k, in order, from nrms_rank_dot_tagged with the same
 *       arguments, and the same score bits.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_tagged: ...", "rank_dot_tagged: ...");
 *   n_tags outside [1, 512] and a NULL or misaligned item_tag (N > 0) or allow are among them.  An undersized workspace returns
 *   NRMS_EWORKSPACE.  Nothing is launched after an error.
 * Workspace: the _tagged_workspace_bytes queries return exactly nrms_topk_dot_workspace_bytes(B, N, d, k) and
 *   nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude) (0 = arguments rejected); 8-byte aligned.
 * The same kernel counts as the untagged calls (two for the top-k, three for the rank), on `stream`, no host synchronisation, no
 *   allocation; plain vector loads and stores, no atomics beyond the integer counters of the untagged kernels.  A block transposes its
 *   32 users' sets once into n_tags words of LDS, so a score costs one bit test; a wave whose 64 items are closed to all 32 users of
 *   its block loads no item row and runs no MFMA for that step.  The results are the same with that skip compiled out
 *   (csrc/topk_entry.h TK_TAGS_SKIP). */
size_t nrms_topk_dot_tagged_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_tagged(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                         const float* bias /* [N], nullable */, const int32_t* item_tag /* [N] */, int32_t n_tags,
                         const uint32_t* allow /* [B, W] */, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                         int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);
size_t nrms_rank_dot_tagged_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude);
int nrms_rank_dot_tagged(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                         const float* bias /* [N], nullable */, const int32_t* item_tag /* [N] */, int32_t n_tags,
                         const uint32_t* allow /* [B, W] */, const int64_t* targets, const int64_t* exclude, int32_t n_exclude,
                         int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Per-category caps on the served list (a front page: "at most two stories per category in my ten", "one politics story at
 * most for this user"; PARITY UNPINNED, the reference has no catalogue retrieval) ----
 * nrms_topk_dot_biased with a hard cap per item tag and user, exact, in one scan of the row-ordered catalogue.  item_tag [N] int32:
 * one tag per item; cap [B, n_tags] int32: the most items of tag t that row b may hold; both REQUIRED and 4-byte aligned.  bias [N]
 * fp32, 4-byte aligned, NULLABLE: NULL means no prior, s' = s.  Every other argument is the biased call's.
 * Greedy rule.  Walk user b's complete ranking under nrms_topk_dot_biased's rules: the same score bits s, one fp32 add for the prior
 *   (s' = s + bias[n]), a NaN s' removes the item, so does the exclude list, s' descending (+inf first), equal s' put the SMALLER n
 *   first, -0.0 equals +0.0 (returned as +0.0).  Item n with tag t = item_tag[n] is TAKEN iff 0 <= t < n_tags and fewer than
 *   cap[b, t] items of tag t were taken before it.  The first k taken items are row b, followed by id -1 / score -inf.
 * Tags and caps.  A tag outside [0, n_tags) is served to nobody (nrms_topk_dot_tagged's rule: -1 is "untagged, never served").
 *   cap <= 0 closes the tag for that user; cap >= k leaves it uncapped.
 * Limits: 1 <= k <= 256, 1 <= n_tags <= 512, N, d, B and n_exclude as in nrms_topk_dot; B = 0 is a no-op, N = 0 writes
 *   all-padding rows.
 * Consequences.
 *   (1) Every cap >= k gives nrms_topk_dot_tagged with all tags open, bit for bit; with every tag in [0, n_tags) that is the plain /
 *       biased call.
 *   (2) Every cap in {0} u [k, inf) (and every cap < 0 read as 0) gives nrms_topk_dot_tagged with allow = cap > 0, bit for bit.
 *   (3) The first k' columns of a call with k are the call with k': the greedy walk does not depend on k.
 *   (4) No row holds more than max(cap[b, t], 0) ids of tag t.
 *   (5) Row b depends on user row b and cap row b only: not on B, the row's position in the batch, the other rows' caps, the launch
 *       geometry, what the workspace held or the run.
 *   (6) For N <= 4096, row b equals the greedy walk over row b of nrms_topk_dot_deep (K = 4096) under the same prior and exclude
 *       list, ids and score bits alike.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_capped: ..."); n_tags outside [1, 512] and
 *   a NULL or misaligned item_tag (N > 0) or cap are among them.  An undersized workspace returns NRMS_EWORKSPACE.  Nothing is
 *   launched after an error.
 * Workspace: nrms_topk_dot_capped_workspace_bytes returns exactly nrms_topk_dot_workspace_bytes(B, N, d, k) (0 = arguments
 *   rejected); 8-byte aligned.
 * Two kernels on `stream` (the slices, the merge), no host synchronisation, no allocation, no [B, N] matrix; plain vector loads and
 *   stores, no atomics beyond the integer LDS counters of the uncapped slice kernel.  Why one scan is exact: with C(S) the capped
 *   list of a set S, C(S1 u S2) = C(C(S1) u C(S2)), and once the capped list of what a user has been shown holds
 *   k_b = min(k, sum_t min(max(cap[b, t], 0), k)) entries nothing below its smallest entry can enter. */
size_t nrms_topk_dot_capped_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_capped(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                         const float* bias /* [N], nullable */, const int32_t* item_tag /* [N] */, int32_t n_tags,
                         const int32_t* cap /* [B, n_tags] */, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                         int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Per-user score adjustments (impression discounting: "shown three times without a click: down by 3 beta"; per-user boosts: a
 * followed publisher, an editor's pin for a segment; a per-user block that is not the click history; PARITY UNPINNED, the reference
 * has no catalogue retrieval) ----
 * nrms_topk_dot_biased / nrms_rank_dot_biased with a short per-user list of (catalogue row, delta) pairs.  adj_ids int64 [B, E],
 * 8-byte aligned, and adj_delta fp32 [B, E], 4-byte aligned, E = n_adjust, 0 <= E <= 256 (NRMS_ADJ_MAX).  bias [N] fp32, 4-byte
 * aligned, NULLABLE: NULL means no prior, s' = s.  Every other argument is the biased call's.
 * Slots.  Slot (b, e) names catalogue row adj_ids[b, e]; a value outside [0, N) is an empty slot (-1 by convention).  The slot of
 *   pair (b, n) is the LOWEST e with adj_ids[b, e] == n; later slots of row b that name the same n are ignored.
 * Scores.  s'(b, n) is what the biased call would offer: the same score bits s, plus bias[n] when bias != NULL (one fp32 add).  A pair
 *   with a slot has s'' = s' + adj_delta[b, e]: one fp32 add on the finished s', after the prior's add, never folded into the chain.
 *   A pair without a slot keeps s'' = s', with no add performed.
 * Eligibility.  Item n is eligible for user b iff n is not in b's exclude row and s'' is not NaN.  So a NaN delta closes the item for
 *   that user alone; -inf and +inf deltas are ordinary values under the order (s'' descending, +inf first, equal s'' put the SMALLER n
 *   first, -0.0 equals +0.0 and is returned as +0.0).  An id that is both excluded and adjusted is excluded.
 * Everything else is nrms_topk_dot_biased's / nrms_rank_dot_biased's: entry order and tie rule, padding id -1 / score -inf, 1 <= k <=
 *   256, 1 <= T <= 32, the exclude list, invalid targets (out of range, excluded, NaN s'') give rank 0 / score -inf, ranks are exact
 *   integers, rank(b, t) = 1 + #{eligible n : (s''(b, n), n) precedes (s''(b, t), t)}.  The returned scores are s''.
 * Consequences.
 *   (a) E == 0, or adj_ids == NULL and adj_delta == NULL, is the biased (bias == NULL: the plain) call, bit for bit; so is a call
 *       whose slots are all empty.
 *   (b) With bias == NULL, row b equals nrms_topk_dot_biased / nrms_rank_dot_biased at B = 1 whose bias holds row b's deltas
 *       scattered by the lowest-slot rule and +0.0 elsewhere (adding +0.0 changes no score the order or the result can tell apart:
 *       -0.0 is returned as +0.0 either way): ids, ranks and returned score bits are equal.
 *   (c) Row b depends on user row b, adj row b and exclude row b only: not on B, the row's position in the batch, the other rows'
 *       slots, the launch geometry, what the workspace held or the run.
 *   (d) The first k' columns of a call with k are the call with k'.
 *   (e) The ids nrms_topk_dot_adjusted returns for user b get ranks 1 .. k, in order, from nrms_rank_dot_adjusted with the same
 *       arguments.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_adjusted: ...", "rank_dot_adjusted: ..."):
 *   n_adjust outside [0, 256], exactly one of adj_ids / adj_delta NULL with n_adjust > 0 and a misaligned list are among them.  An
 *   undersized workspace returns NRMS_EWORKSPACE.  Nothing is launched after an error.
 * Workspace: the _workspace_bytes queries return exactly nrms_topk_dot_workspace_bytes(B, N, d, k) / nrms_rank_dot_workspace_bytes(B,
 *   N, d, T, n_exclude) (0 = arguments rejected); 8-byte aligned.
 * The kernels of nrms_topk_dot / nrms_rank_dot on `stream`, no host synchronisation, no allocation, no [B, N] matrix.  A block stages
 *   the slots of its 32 users that fall into its catalogue slice in LDS (up to 2048 of them for k <= 192, 1024 above: every E <= 64 at
 *   k <= 192 is staged) and otherwise walks the lists in global memory: slower, never different. */
#define NRMS_ADJ_MAX 256
size_t nrms_topk_dot_adjusted_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_adjusted(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                           const float* bias /* [N], nullable */, const int64_t* adj_ids /* [B, E] */,
                           const float* adj_delta /* [B, E] */, int32_t n_adjust /* E */, const int64_t* exclude, int32_t n_exclude,
                           float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);
size_t nrms_rank_dot_adjusted_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude);
int nrms_rank_dot_adjusted(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                           const float* bias /* [N], nullable */, const int64_t* adj_ids /* [B, E] */,
                           const float* adj_delta /* [B, E] */, int32_t n_adjust /* E */, const int64_t* targets,
                           const int64_t* exclude, int32_t n_exclude, int32_t* ranks, float* target_scores, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- One request through several catalogue filters at once (a front page: news that is still live, outside the topics this user
 * muted, with what they were already shown pushed down, after the page they have just seen; PARITY UNPINNED, the reference has no
 * catalogue retrieval) ----
 * nrms_topk_dot_biased / nrms_rank_dot_biased with four optional PARTS, each a pair of pointers given both or neither:
 *   the window       item_time [N] int32, window [B, 2] int32          nrms_topk_dot_windowed's
 *   the tag set      item_tag [N] int32, allow [B, W] uint32, n_tags   nrms_topk_dot_tagged's
 *   the adjustments  adj_ids [B, E] int64, adj_delta [B, E] fp32, E    nrms_topk_dot_adjusted's
 *   the cursor       after_scores [B] fp32, after_ids [B] int64        nrms_topk_dot_after's (top-k only)
 * Every part is NULLABLE and keeps the rules its own call states, word for word: the window is half-open and signed, lo <= time <
 * hi, and a time of INT32_MAX is never eligible; a tag outside [0, n_tags) is served to nobody, 1 <= n_tags <= 512 (read only when
 * the tag set is given); E = n_adjust <= 256 (NRMS_ADJ_MAX), an id outside [0, N) is an empty slot, of several slots of one user
 * that name one row the LOWEST e counts, and n_adjust == 0 or two NULL lists mean no adjustments; after_ids[b] == NRMS_CURSOR_BEGIN
 * is no cursor for that row, any other negative id or a NaN after score is END.  bias [N] fp32, NULLABLE.
 * The composition.
 *   Scores.  s'' = (s + bias[n]) + delta: the same score bits s, then two fp32 additions in that order on the finished accumulator,
 *     the first only with a prior, the second only where the pair (b, n) has a slot; neither is folded into the chain.
 *   Eligibility.  Item n is eligible for user b iff ALL of these hold: n is not in b's exclude row; s'' is not NaN; b's window is
 *     open to item_time[n]; b allows item_tag[n].  An absent part closes nothing.
 *   Order, ties, -0.0, padding (id -1 / score -inf) and the returned scores (s'') are nrms_topk_dot_biased's.
 *   The cursor compares (s'', n): user b is offered the eligible items strictly after (after_scores[b], after_ids[b]) in that
 *     order.  A client that pages must pass the same adjustments on every page.
 *   Rank.  A target closed by any part, excluded or out of range gets rank 0 / score -inf; otherwise rank(b, t) = 1 + #{eligible n :
 *     (s''(b, n), n) precedes (s''(b, t), t)} and its score is s''.
 * Consequences.
 *   1. All parts given but neutral by value (the window (INT32_MIN, INT32_MAX) over times below INT32_MAX, every tag open, every
 *      slot -1, every cursor NRMS_CURSOR_BEGIN) is nrms_topk_dot_biased / nrms_rank_dot_biased, bit for bit.
 *   2. One part live, the rest neutral by value or NULL, is that part's own call, bit for bit: nrms_topk_dot_windowed, _tagged,
 *      _adjusted, _after and their rank forms.
 *   3. With bias == NULL, row b equals nrms_topk_dot_biased at B = 1 whose bias holds row b's deltas scattered by the lowest-slot
 *      rule, +0.0 elsewhere, and NaN where b's window or tag set closes the item.
 *   4. The ids nrms_topk_dot_request returns for user b (without a cursor) get ranks 1 .. k, in order, from nrms_rank_dot_request
 *      with the same parts.
 *   5. Pages chained by the cursor (each page's last column is the next page's cursor) are the prefix of the longer list and then
 *      padding: nothing is repeated or skipped across ties.
 *   6. Row b depends on user row b, the b-th row of every part and exclude row b only: not on B, the row's position in the batch,
 *      the other rows, the launch geometry, what the workspace held or the run.
 * Routing.  No part, and exactly one part, forward to the existing entry point (nrms_topk_dot_biased, _windowed, _tagged,
 *   _adjusted, _after and the rank forms), and the window with the cursor alone to nrms_topk_dot_after: the same device code, the
 *   same bytes.  Every other combination runs one kernel form that holds all parts and skips an absent one by a block-uniform
 *   branch.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_request: ...", "rank_dot_request: ..."): a
 *   half-given pair names its missing pointer ("window is null"), n_tags outside [1, 512] with a tag set, n_adjust outside [0, 256]
 *   and a misaligned array are among them.  An undersized workspace returns NRMS_EWORKSPACE.  Nothing is launched after an error.
 * Workspace: the _workspace_bytes queries return exactly nrms_topk_dot_workspace_bytes(B, N, d, k) / nrms_rank_dot_workspace_bytes(B,
 *   N, d, T, n_exclude) (0 = arguments rejected); 8-byte aligned.
 * The kernels of nrms_topk_dot / nrms_rank_dot on `stream`, no host synchronisation, no allocation, no [B, N] matrix.  A wave whose
 *   64 items are closed to its whole 32-user block by the window hull OR by the tag bitmap runs no score chain for that step.  A
 *   block stages the slots of its users that fall into its slice in LDS, up to 2048 of them for k <= 192 and 512 above (half of the
 *   adjusted call's: the tag bitmap, the windows and the cursor keys lie beside the list), and otherwise walks the lists in global
 *   memory: slower, never different.
 * Not composed here: the fp16 shortlist, sections, the diversity re-ranking, the log-partition, the attribution and the deep list;
 *   paging works through the cursor.  The per-tag caps are composed with every part in nrms_topk_dot_request_capped (below); there
 *   is no rank under caps. */
size_t nrms_topk_dot_request_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_request(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                          const float* bias /* [N], nullable */, const int32_t* item_time /* [N], nullable */,
                          const int32_t* window /* [B, 2], nullable */, const int32_t* item_tag /* [N], nullable */, int32_t n_tags,
                          const uint32_t* allow /* [B, W], nullable */, const int64_t* adj_ids /* [B, E], nullable */,
                          const float* adj_delta /* [B, E], nullable */, int32_t n_adjust /* E */,
                          const float* after_scores /* [B], nullable */, const int64_t* after_ids /* [B], nullable */,
                          const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t nrms_rank_dot_request_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude);
int nrms_rank_dot_request(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                          const float* bias /* [N], nullable */, const int32_t* item_time /* [N], nullable */,
                          const int32_t* window /* [B, 2], nullable */, const int32_t* item_tag /* [N], nullable */, int32_t n_tags,
                          const uint32_t* allow /* [B, W], nullable */, const int64_t* adj_ids /* [B, E], nullable */,
                          const float* adj_delta /* [B, E], nullable */, int32_t n_adjust /* E */, const int64_t* targets,
                          const int64_t* exclude, int32_t n_exclude, int32_t* ranks, float* target_scores, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- Per-category caps through the request (a rationed front page that expires news per user, mutes topics, pushes down what was
 * seen and serves page 2; PARITY UNPINNED, the reference has no catalogue retrieval) ----
 * nrms_topk_dot_request_capped: nrms_topk_dot_capped's greedy walk over the items nrms_topk_dot_request leaves eligible.
 * item_tag [N] int32 and cap [B, n_tags] int32 are REQUIRED (4-byte aligned), 1 <= n_tags <= 512.  Every other part is NULLABLE and
 * given as both pointers or neither, with the rules nrms_topk_dot_request states: the window (item_time, window), the adjustments
 * (adj_ids, adj_delta, n_adjust <= 256), the cursor (after_scores, after_ids); allow [B, W] uint32, W = ceil(n_tags / 32), is the
 * tag set over the same item_tag and n_tags (NULL: every tag in range is open).  bias [N] fp32, NULLABLE.  1 <= k <= 256.  An absent
 * part closes nothing.
 * Eligible set.  nrms_topk_dot_request's, word for word: the score is s'' = (s + bias[n]) + delta; item n is eligible for user b iff
 *   n is not in b's exclude row, s'' is not NaN, b's window is open to item_time[n], b allows item_tag[n] (if allow is given) and
 *   (s'', n) lies strictly after b's cursor (if one is given).
 * Greedy walk.  Walk that set in nrms_topk_dot_biased's order (s'' descending, then the smaller n, -0.0 equal to +0.0).  Item n with
 *   tag t = item_tag[n] is TAKEN iff 0 <= t < n_tags and fewer than cap[b, t] items of tag t were taken before it IN THIS CALL.  The
 *   first k taken items are row b, with their s''; then id -1 / score -inf.
 * Cap values.  cap <= 0 closes the tag, cap >= k leaves it uncapped; a tag is open iff cap > 0 and, with allow given, its bit is set.
 * Consequences.
 *   1. Every cap >= k is nrms_topk_dot_request with the same parts, bit for bit, its tag set being allow (allow == NULL: all tags
 *      in range open).
 *   2. No window, no adjustments, no cursor and allow == NULL is nrms_topk_dot_capped, bit for bit (the call is routed there).
 *   3. The first k' columns of a call with k are the call with k'.
 *   4. With no cursor and bias == NULL, row b equals nrms_topk_dot_capped at B = 1 whose bias holds row b's deltas scattered by the
 *      lowest-slot rule, +0.0 elsewhere, and NaN where b's window or allow closes the item; for N <= 4096 it is therefore also the
 *      greedy walk over nrms_topk_dot_deep with that bias.
 *   5. Paging.  Let page j + 1 be the call whose cursor is the last column of page j, whose cap is the original cap minus the
 *      per-tag counts of everything served on pages 1 .. j, and whose other parts are unchanged.  The pages laid end to end are the
 *      columns of ONE call with k = the sum of the page lengths (any total <= 256), then padding; nothing is repeated or skipped
 *      across ties.  (An item the walk skipped before the cursor belonged to a saturated tag and can never be taken later; every
 *      item after the cursor sees exactly the room that is left.)
 *   6. No row holds more than max(cap[b, t], 0) ids of tag t.
 *   7. Row b depends on user row b, the b-th row of every part, cap row b and exclude row b only: not on B, the row's position in
 *      the batch, the other rows, the launch geometry, what the workspace held or the run.
 * There is no rank form: the position of a target in a capped list is not a count of predecessors.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_request_capped: ..."): cap or item_tag NULL,
 *   a half-given pair (it names its missing pointer), n_tags outside [1, 512], n_adjust outside [0, 256] and a misaligned array are
 *   among them.  An undersized workspace returns NRMS_EWORKSPACE.  Nothing is launched after an error.
 * Workspace: the query returns exactly nrms_topk_dot_workspace_bytes(B, N, d, k) (0 = arguments rejected); 8-byte aligned.
 * One scan of the catalogue and one merge on `stream`, no host synchronisation, no allocation, no [B, N] matrix.  A block keeps a
 *   16-bit threshold per (user, tag) in the LDS its request parts leave free: every n_tags for k <= 64, n_tags <= 43 for k <= 192,
 *   none above; a call without the table gives the same results (what the table saves is measured for nrms_topk_dot_capped,
 *   DESIGN.md section 8m; section 8p has this call's figures). */
size_t nrms_topk_dot_request_capped_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_request_capped(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                 const float* bias /* [N], nullable */, const int32_t* item_time /* [N], nullable */,
                                 const int32_t* window /* [B, 2], nullable */, const int32_t* item_tag /* [N] */, int32_t n_tags,
                                 const uint32_t* allow /* [B, W], nullable */, const int32_t* cap /* [B, n_tags] */,
                                 const int64_t* adj_ids /* [B, E], nullable */, const float* adj_delta /* [B, E], nullable */,
                                 int32_t n_adjust /* E */, const float* after_scores /* [B], nullable */,
                                 const int64_t* after_ids /* [B], nullable */, const int64_t* exclude, int32_t n_exclude,
                                 float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Paging through the exact ranking: a cursor on the top-k, and lists up to 4096 (candidate generation for a re-ranker, a feed
 * that scrolls: "the next 20 after what I showed"; PARITY UNPINNED, the reference has no catalogue retrieval) ----
 * The order of nrms_topk_dot[_biased|_windowed] is total (s' descending, then the SMALLER n, -0.0 equal to +0.0) and a score's bits
 * do not depend on B, N, k, the row's position or the run, so "everything after (s, n) in user b's ranking" is well defined and a
 * page needs no state but the last (score, id) its reader saw.
 *
 * nrms_topk_dot_after: one page.  after_scores [B] fp32 and after_ids [B] int64, both REQUIRED, 4- / 8-byte aligned: user b's
 * cursor.  bias [N] fp32, NULLABLE, as nrms_topk_dot_biased's; item_time [N] int32 and window [B, 2] int32, NULLABLE, given both or
 * neither, as nrms_topk_dot_windowed's (NULL: no window).  Every other argument is nrms_topk_dot's; 1 <= k <= 256.
 * Eligible, score, order, padding: the uncursored call's (with the prior s' = s + bias[n], with the window its eligibility).
 * Cursor.  Row b holds, in order, the first k eligible items n with (s'(b, n), n) strictly AFTER (after_scores[b], after_ids[b])
 *   in that order: s' < after_scores[b], or s' equal to it and n > after_ids[b]; then -1 / -inf.
 *   after_ids[b] == -2 (NRMS_CURSOR_BEGIN): no cursor; after_scores[b] is not inspected, row b is the uncursored call's row, bit
 *     for bit.  Users on different pages, first pages included, can share one call.
 *   after_ids[b] == -1, any other negative id, or a NaN after_scores[b]: END, row b is all padding.  -1 / -inf is what a page
 *     leaves in the columns a list did not reach, so feeding the last column of a finished page back in yields padding again.
 *   after_ids[b] >= 0: a position in the order, not an item: the id need not be eligible, un-excluded, inside the window or below
 *     N.  Ids above 0x7FFF0000 are read as 0x7FFF0000, which follows every item at the same score.  -0.0 is +0.0; +inf and -inf
 *     are ordinary scores.
 *
 * nrms_topk_dot_deep: 1 <= K <= 4096; top_scores [B, K] fp32 and top_ids [B, K] int64, both REQUIRED, 4- / 8-byte aligned.  Row
 * b holds the first min(K, #eligible) items of user b's ranking in order, then -1 / -inf; every element is written.  It runs
 * ceil(K / 256) pages: the first is min(256, K) columns with no cursor, each later one min(256, rest) columns whose cursor is the
 * last column of the page before, read on the device.  Arguments as nrms_topk_dot_after's without the cursor.
 *
 * Consequences.
 *   (a) With every after_ids[b] == -2, nrms_topk_dot_after equals nrms_topk_dot / _biased / _windowed with the same arguments, bit
 *       for bit, ids and scores.
 *   (b) Chaining pages of any lengths, each from the last column of the page before, reproduces the uncursored list: no item is
 *       repeated or skipped, across runs of equal scores included, and a finished list returns padding from then on.
 *   (c) nrms_topk_dot_deep at K <= 256 equals nrms_topk_dot / _biased / _windowed at k = K, bit for bit (the same kernels).
 *   (d) The first K' columns of nrms_topk_dot_deep(K) are nrms_topk_dot_deep(K').
 *   (e) The ids of row b of nrms_topk_dot_deep get ranks 1, 2, ... from nrms_rank_dot / _biased / _windowed with the same
 *       arguments, and the same score bits.
 *   (f) The result does not depend on B, the row's position in the batch, the page lengths, the other rows' cursors, the launch
 *       geometry, what the workspace held or the run.
 * Argument errors return NRMS_EINVAL with a message that names the argument ("topk_dot_after: ...", "topk_dot_deep: ..."); a NULL
 *   or misaligned after_scores / after_ids, and an item_time (N > 0) without a window or a window without an item_time, are among
 *   them.  An undersized workspace returns NRMS_EWORKSPACE.  Nothing is launched after an error.  B = 0 is a no-op, N = 0 writes
 *   padding.
 * Workspace: nrms_topk_dot_after_workspace_bytes returns exactly nrms_topk_dot_workspace_bytes(B, N, d, k), and
 *   nrms_topk_dot_deep_workspace_bytes that of its longest page, nrms_topk_dot_workspace_bytes(B, N, d, min(K, 256)) (0 =
 *   arguments rejected); 8-byte aligned.
 * nrms_topk_dot_after launches the same kernel counts as the uncursored call, nrms_topk_dot_deep those of its pages one after the
 *   other; all on `stream`, no host synchronisation, no allocation; plain vector loads and stores, no atomics beyond the integer
 *   LDS counters of nrms_topk_dot's slice kernel.  A block of 32 users who are all at END loads no item row.  The results are the
 *   same with that exit compiled out (csrc/topk_entry.h TK_CURSOR_EXIT). */
#define NRMS_CURSOR_BEGIN (-2)
size_t nrms_topk_dot_after_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k);
int nrms_topk_dot_after(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                        const float* bias /* [N], nullable */, const int32_t* item_time /* [N], nullable */,
                        const int32_t* window /* [B, 2], nullable */, const float* after_scores /* [B] */,
                        const int64_t* after_ids /* [B] */, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                        int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream);
size_t nrms_topk_dot_deep_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t K);
int nrms_topk_dot_deep(int32_t B, int64_t N, int32_t d, int32_t K, const float* user, const float* items,
                       const float* bias /* [N], nullable */, const int32_t* item_time /* [N], nullable */,
                       const int32_t* window /* [B, 2], nullable */, const int64_t* exclude, int32_t n_exclude,
                       float* top_scores /* [B, K] */, int64_t* top_ids /* [B, K] */, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- The exact top-k through an fp16 shortlist with a certificate (csrc/topkcoarse.hip; serving: nrms_topk_dot's rows for less
 * than nrms_topk_dot's scan; PARITY UNPINNED, the reference has no catalogue retrieval) ----
 * A coarse pass over an fp16 copy of the catalogue on v_mfma_f32_32x32x16_f16 picks a shortlist of M items per user, the shortlist
 * is re-scored with nrms_topk_dot's exact chain, and a per-user certificate proves from norms formed beforehand that no item
 * outside the shortlist can reach the top k.
 * GUARANTEE: a row with certified[b] = 1 equals nrms_topk_dot's row b (same user, items, exclude, k) bit for bit, ids and
 *   scores.  A row with certified[b] = 0 is the exact top k of the shortlist only: send it through nrms_topk_dot.
 *
 * nrms_catalogue_f16_pitch(d) = 32 * ceil(d / 32): the halves per row of the packed copy (0 = d rejected).
 *
 * nrms_catalogue_pack_f16: items [N, d] fp32 -> items16 [N, pitch] uint16 (fp16 bits; 16-byte aligned; N * pitch * 2 bytes) and
 *   stats float [2] on the device (4-byte aligned).
 *   Element rule h(x): a magnitude above 65504 becomes +-65504, a magnitude below 2^-14 becomes +-0 (both decided on the fp32
 *     input), everything else is rounded to nearest even: no subnormal and no infinity is ever stored, so the MFMA's input-flush
 *     mode cannot matter.  Columns >= d are 0.  A row holding a NaN or an infinity is stored as zeros and makes stats[0] = +inf.
 *   stats[0] = NRM >= max_n ||items[n]||_2, stats[1] = ERR >= max_n ||items[n] - items16[n]||_2 (over the rows without NaN / inf):
 *     the sums are formed in fp64 and rounded UP to fp32; the maximum over the rows is an integer atomic max on the float's bits,
 *     so it has no order and two runs are bit-identical.  N = 0 gives stats = {0, 0}.
 *   One memset and one kernel on `stream`, no host synchronisation.  Pack again whenever items changes.
 *
 * nrms_topk_dot_coarse: user [B, d], items [N, d] fp32, items16 / stats as packed from THESE items; exclude, top_scores [B, k],
 *   top_ids [B, k] as nrms_topk_dot's; certified [B] uint8; short_scores [B, M] fp32 and short_ids [B, M] int64, both NULLABLE.
 *   Limits: 1 <= k <= M <= 256; every other limit, B = 0 (a no-op) and N = 0 (all-padding rows, certified) are nrms_topk_dot's.
 *   (a) Per user: u16 = h(user[b]) padded to the pitch, in the workspace, and in fp64, rounded up, un >= ||u||, un16 >= ||u16||,
 *       ue >= ||u - u16||.  A user row holding a NaN or an infinity is stored as zeros with infinite norms (never certified).
 *   (b) Coarse score c(b, n): ONE fp32 accumulator over the whole pitch on v_mfma_f32_32x32x16_f16, no split-K, each whole
 *       superblock sb of 64 halves in four instructions (halves 64 sb + 32 h + 8 s + j of lane half h, instruction s, element j),
 *       a last block of 32 halves in two (16 h + 8 s + j of it), the same fixed order for every (user, item): its bits do not
 *       depend on B, N, M, the item's row, the exclude list or the run.  Eligibility (exclude,
 *       NaN) and the order (score descending, smaller n first, -0.0 = +0.0) are nrms_topk_dot's, through the same filter.
 *   (c) The shortlist: the M eligible items of largest c(b, n) in that order, L = min(M, #eligible) real entries, then id -1 /
 *       score -inf; written to short_scores / short_ids when given.  It is nrms_topk_dot at k = M over the coarse scores.
 *   (d) Every shortlist entry's exact score s(b, n) is nrms_topk_dot's chain against the fp32 row it names (the same code, the same
 *       bits); row b of top_scores / top_ids is the first min(k, L) shortlist entries in nrms_topk_dot's order of their EXACT
 *       scores, then id -1 / score -inf.
 *   Certificate, in fp64 with every product and sum rounded up: certified[b] = 1 iff stats and the user's norms are finite,
 *       un * NRM <= 2^100, and either L < M (every eligible item is in the shortlist) or s_k > c_M + E_b strictly, s_k the k-th
 *       exact score of the row and c_M the M-th coarse score, with
 *         E_b = ue*NRM + un16*ERR + gamma_d*un*NRM + alpha_d*un16*(NRM + ERR) + d*2^-140,
 *         gamma_d = d*2^-24 / (1 - d*2^-24)  (the exact fmaf chain),   alpha_d = d*2^-21  (the fp16 MFMA's fp32 accumulation).
 *       Soundness: u.n - u16.n16 = (u - u16).n + u16.(n - n16), both terms bounded by Cauchy-Schwarz with the norms; an item outside
 *       a full shortlist has c <= c_M, so its exact score is <= c_M + E_b < s_k: it can neither enter the top k nor tie into it.
 *   Argument errors return NRMS_EINVAL with a message that starts "topk_dot_coarse: ..." and names the argument (items16 must be
 *     16-byte aligned, stats 4-byte); an undersized workspace returns NRMS_EWORKSPACE.  Nothing is launched after an error.
 *   Workspace: nrms_topk_dot_coarse_workspace_bytes(B, N, d, k, M) bytes, 8-byte aligned (0 = arguments rejected: k < 1, k > M,
 *     M > 256 and whatever nrms_topk_dot_workspace_bytes rejects).  What it holds on entry does not matter.
 *   Five kernels on `stream` (user, slices, merge, re-score, finish), no host synchronisation, no allocation; plain vector loads
 *     and stores, no atomics beyond the LDS counters of nrms_topk_dot's slice kernel. */
int32_t nrms_catalogue_f16_pitch(int32_t d);
int nrms_catalogue_pack_f16(int64_t N, int32_t d, const float* items, uint16_t* items16, float* stats, void* stream);
size_t nrms_topk_dot_coarse_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k, int32_t M);
int nrms_topk_dot_coarse(int32_t B, int64_t N, int32_t d, int32_t k, int32_t M, const float* user, const float* items,
                         const uint16_t* items16, const float* stats, const int64_t* exclude, int32_t n_exclude,
                         float* top_scores, int64_t* top_ids, uint8_t* certified, float* short_scores /* [B, M], nullable */,
                         int64_t* short_ids /* [B, M], nullable */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Negatives from the model's own softmax over the whole catalogue (csrc/softmaxsample.hip; training: "which S news does the
 * model itself confuse with the positive right now?"; PARITY UNPINNED, the reference draws its negatives offline) ----
 * For each user b < B: S items drawn WITHOUT replacement from softmax(s(b, .) * inv_temperature) over the eligible items, never
 * forming the [B, N] score matrix, as a pure function of the inputs.  By the Gumbel-top-S identity these are the S largest perturbed
 * keys s(b, n) * inv_temperature + g(b, n), g i.i.d. standard Gumbel: nrms_topk_dot with a keyed perturbation in its epilogue.
 * user [B, d], items [N, d] fp32 row-major; row_key [B] int64: what names row b's draw (e.g. a click's position in the log);
 * exclude [B, n_exclude] int64, nullable, as nrms_topk_dot's; ids [B, S] int64; keys [B, S] fp32, nullable.
 * Score.  s(b, n) is nrms_topk_dot's chain for (user row, item row): one fp32 accumulator over all of d on
 *   v_mfma_f32_32x32x2_f32 in the same k order, so the same bits (the kernels are the same code).
 * Noise.  An exact integer function of (seed, row_key[b], n), independent of B, N, the row's position and the launch geometry.  A
 *   48-bit row key and a 31-bit item id do not fit one 64-bit Philox counter, so the draw has two levels (philox4x32_7 and the
 *   counter layout of the dropout sites, csrc/common.h):
 *     r = philox4x32_7(seed, group = row_key[b], site 8);   row_seed = r[0] | (uint64) r[1] << 32
 *     w(b, n) = word n & 3 of philox4x32_7(row_seed, group = n >> 2, site 9)
 *   (four neighbouring items share one call on purpose: adjacent lanes of an MFMA column tile hold adjacent items, so the generator
 *   work can be quartered later without changing a draw).  m = w >> 9;  u = (2 m + 1) * 2^-24, exact in fp32 and strictly inside
 *   (0, 1);  g = -logf(-logf(u)) in fp32, below 17.4 for every u.
 * Key.  key(b, n) = fmaf(s(b, n), inv_temperature, g(b, n)) in fp32, inv_temperature = 1 / temperature finite and >= 0.  0 gives a
 *   uniform draw over the eligible items with finite scores (an infinite score times 0 is NaN); large values approach "the S
 *   hardest".
 * Eligible: n is not in exclude[b, :] and key(b, n) is not NaN.
 * Order.  Key descending; equal keys put the SMALLER n first; -0.0 equals +0.0 (returned as +0.0): nrms_topk_dot's order.
 * Output.  Row b holds the first min(S, #eligible) items in that order, which is the Plackett-Luce order: slot 0 is a draw from the
 *   softmax, slot 1 a draw from the rest, and so on; the remaining slots hold id -1 and key -inf.  keys carries the perturbed keys,
 *   not the plain scores.
 * Limits: 1 <= S <= 256, d >= 1, 0 <= N <= 0x7FFF0000, B >= 0, n_exclude >= 0, 0 <= row_key < 2^48; B = 0 is a no-op, N = 0
 *   writes all-padding rows.  Arguments outside the limits return NRMS_EINVAL (row keys are device data and are not inspected).
 * Workspace: nrms_softmax_sample_dot_workspace_bytes(B, N, d, S, n_exclude) bytes, 8-byte aligned, O(B * slices * S) (0 =
 *   arguments rejected).
 * Two kernels on `stream`, no host synchronisation, no allocation; plain vector stores only, no float atomics (the integer LDS
 *   counters of the slice buffers order insertions, never a result): two runs are bit-identical whatever the workspace held. */
size_t nrms_softmax_sample_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t S, int32_t n_exclude);
int nrms_softmax_sample_dot(int32_t B, int64_t N, int32_t d, int32_t S, const float* user, const float* items,
                            const int64_t* row_key /* [B] */, float inv_temperature, uint64_t seed,
                            const int64_t* exclude /* [B, n_exclude], nullable */, int32_t n_exclude, int64_t* ids /* [B, S] */,
                            float* keys /* [B, S], nullable */, void* workspace, size_t workspace_bytes, void* stream);
/* Test hook, like nrms_dropout_keep_mask: the whole [B, N] perturbation of nrms_softmax_sample_dot for small shapes, w(b, n) into
 * words and g(b, n) into gumbel (each nullable, not both; the same device function as the fused kernel's). */
int nrms_softmax_sample_noise(int32_t B, int64_t N, const int64_t* row_key /* [B] */, uint64_t seed,
                              uint32_t* words /* [B, N], nullable */, float* gumbel /* [B, N], nullable */, void* stream);

/* ---- The exact log-partition of the served softmax over the whole catalogue (csrc/lsedot.hip; evaluation and calibration: "how
 * much probability does the model put on this news?"; PARITY UNPINNED, the reference scores shown candidates only) ----
 * For each user b < B and each of J variants j: lse(b, j) = log sum over the eligible n of exp(z_j(b, n)), never forming the
 * [B, N] score matrix; the dot product, the expensive part, is shared by the J variants.  user [B, d], items [N, d] fp32 row-major;
 * bias [N] fp32, 4-byte aligned, NULLABLE (the prior of nrms_topk_dot_biased); inv_temperature [J] and bias_scale [J] (nullable =
 * all 1) are HOST arrays, read before the call returns; exclude [B, n_exclude] int64, nullable, as nrms_topk_dot's (duplicates and
 * ids outside [0, N) are ignored); lse [B, J] fp32; zmax [B, J] fp32 and n_eligible [B, J] int32, each nullable.
 * Score.  s(b, n) is nrms_topk_dot's chain for (user row, item row): the bits of nrms_topk_dot / nrms_rank_dot.
 * Logit.  z_j(b, n) = fmaf(s(b, n), inv_temperature[j], c_j(n)) in fp32; c_j(n) = bias_scale[j] * bias[n], one fp32 multiply, and
 *   +0.0 when bias is NULL.  inv_temperature[j] finite and >= 0 (0: the uniform distribution), bias_scale[j] finite.
 * Eligible (for variant j): n is not in exclude[b, :] and z_j(b, n) is not NaN.  So a NaN bias[n] removes item n for everybody
 *   (nrms_topk_dot_biased's block-list rule), a NaN score removes the pair, and so does a 0 * inf product (inv_temperature 0 and
 *   an infinite score, bias_scale 0 and an infinite bias).  A z of -inf stays eligible and contributes 0.  Exclusion is applied
 *   BEFORE the maximum and the sum, never taken back out afterwards: an excluded item, however high it scores, leaves no trace.
 * Output.  n_eligible(b, j) = the number of eligible pairs.  zmax(b, j) = the exact maximum of the eligible z_j, -inf when there
 *   is none, -0.0 returned as +0.0.  lse(b, j) = zmax + log(sum over eligible of exp(z_j - zmax)); -inf when nothing is eligible
 *   or zmax = -inf; +inf when zmax = +inf.
 * Reduction.  t = expf(z_j - zmax) lies in [0, 1] and is added up in fixed point, unit 2^-63, in two unsigned 64-bit limbs:
 *   hi += floor(t 2^31), lo += floor(frac(t 2^31) 2^32), by integer atomics.  Every fp32 t >= 2^-40 enters exactly, a smaller one
 *   truncated by less than 2^-63, and neither limb can overflow for N <= 0x7FFF0000.  The maximum term is expf(0) = 1, so
 *   mass = hi 2^-31 + lo 2^-63 >= 1 and the accumulation itself is short of the exact sum of the t by less than N 2^-63, which
 *   is below 2^-32 relative for every N.  lse = (float)((double) zmax + log(mass)) in fp64, rounded once.  What remains is the
 *   error of expf itself (docs/EXPERIMENTS.md measures it).
 * Invariance.  Integer addition is associative and a maximum is order-free, so lse, zmax and n_eligible of (b, j) are a pure
 *   function of user row b, the multiset of its eligible z_j and variant j's two parameters, bit for bit: not of B or the row's
 *   position, of the other rows or variants, of N when the extra rows are ineligible, of the order of the catalogue rows, of the
 *   launch geometry, of what the workspace held, or of the run.
 * Limits: 1 <= J <= 8, d >= 1, 0 <= N <= 0x7FFF0000, B >= 0, n_exclude >= 0; B = 0 is a no-op, N = 0 writes lse = zmax = -inf and
 *   n_eligible = 0.  Arguments outside the limits return NRMS_EINVAL with a message that names the argument ("logsumexp_dot: ...").
 * Workspace: nrms_logsumexp_dot_workspace_bytes(B, N, d, J, n_exclude) bytes, 8-byte aligned, O(B * J) (0 = arguments rejected);
 *   a smaller one returns NRMS_EWORKSPACE.
 * Four kernels on `stream` (init, the maxima, the masses, finish: two scans of the catalogue), no host synchronisation, no
 *   allocation; plain vector loads and stores, integer atomics only (LDS or, add and global max, add), no float atomics. */
size_t nrms_logsumexp_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t J, int32_t n_exclude);
int nrms_logsumexp_dot(int32_t B, int64_t N, int32_t d, int32_t J, const float* user /* [B, d] */, const float* items /* [N, d] */,
                       const float* bias /* [N], nullable */, const float* inv_temperature /* [J] host */,
                       const float* bias_scale /* [J] host, nullable = all 1 */,
                       const int64_t* exclude /* [B, n_exclude], nullable */, int32_t n_exclude, float* lse /* [B, J] */,
                       float* zmax /* [B, J], nullable */, int32_t* n_eligible /* [B, J], nullable */, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Test hook, like nrms_softmax_sample_noise: the raw integer mass of nrms_logsumexp_dot, mass[b, j] = (hi, lo) as above (the same
 * kernels; one item at the maximum weighs NRMS_LSE_MASS_ONE in hi and 0 in lo; all 0 where lse is infinite).  Same arguments,
 * workspace and errors ("logsumexp_dot_mass: ..."). */
#define NRMS_LSE_MASS_ONE 0x80000000ull
int nrms_logsumexp_dot_mass(int32_t B, int64_t N, int32_t d, int32_t J, const float* user, const float* items, const float* bias,
                            const float* inv_temperature, const float* bias_scale, const int64_t* exclude, int32_t n_exclude,
                            uint64_t* mass /* [B, J, 2] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Diversified re-ranking of a shortlist (csrc/mmr.hip; serving: "which k of these M candidates, so that the list is not k
 * articles about one story?"; PARITY UNPINNED, the reference has no such step) ----
 * For each user b < B: k entries of the row's shortlist, picked greedily by maximal marginal relevance (Carbonell & Goldstein),
 * and the intra-list diversity of the picks.  items [N, d] fp32 row-major (the catalogue); short_ids [B, M] int64 and
 * short_scores [B, M] fp32: the shortlist, e.g. nrms_topk_dot's output at k = M; out_ids [B, k] int64, out_scores [B, k] fp32,
 * out_value [B, k] fp32 (nullable), ild [B] fp32 (nullable).
 * Entries.  Entry i of row b is VALID if 0 <= short_ids[b, i] < N and short_scores[b, i] is finite.  Everything else is padding
 *   and is never selected: nrms_topk_dot's -1 / -inf tail, NaN and +-inf scores, ids outside the catalogue.  No id outside
 *   [0, N) is dereferenced.  An id that occurs twice makes two separate entries (their similarity is that of a row with itself).
 * Relevance, over the row's valid entries, in fp32: s_min and s_max are their smallest and largest score;
 *   rel_i = (s_i - s_min) / (s_max - s_min): one subtraction each and one IEEE division; rel_i = 0 for every i when
 *   s_max == s_min (-0.0 equals +0.0).
 * Similarity.  dot(i, j) is one fp32 accumulator over all of d on v_mfma_f32_32x32x2_f32 (k order 32m, 32m+16, 32m+1, 32m+17, ...
 *   in each whole block of 32, then 8g, 8g+4, 8g+1, ... in zero-padded groups of 8 for the rest), the same chain for every pair;
 *   r_i = 1 / sqrt(dot(i, i)), a correctly rounded square root and division, or 0 when dot(i, i) is 0 or not finite;
 *   cos(i, j) = dot(i, j) * (r_i * r_j), two roundings.  cos(i, j) and cos(j, i) have the same bits, and the value depends on the
 *   contents of the two item rows only (a zero row has cosine 0 with everything, itself included).
 * Greedy selection, for t = 0 .. k - 1: among the valid entries not picked yet, the one of largest
 *     v_i = (lambda * rel_i) - (c * maxsim_i),   c = 1 - lambda:
 *   one fp32 subtraction for c, two multiplications and one subtraction for v_i, nothing fused.  maxsim_i is 0 at t = 0 and
 *   afterwards the maximum of cos(i, p) over the entries p picked so far, formed in pick order by fmaxf (which skips a NaN
 *   cosine; only non-finite item rows or an overflowing dot make one).
 *   Order: v descending, -0.0 equals +0.0; equal v puts the SMALLER shortlist position first; a NaN v orders after every number.
 * Output.  Row b holds the min(k, #valid) picks in pick order: out_ids the id, out_scores the entry's short_scores bits,
 *   out_value v at the moment of the pick; the remaining slots hold -1 / -inf / -inf.
 * ILD.  ild[b] = 1 - (sum of cos over the unordered pairs of picks) / (number of pairs), NaN with fewer than two picks: one fp32
 *   accumulator from 0 over the pairs (p_u, p_t), t = 1, 2, ... and within t u = 0 .. t - 1 (pick order), one division, one
 *   subtraction.
 * Consequences.  lambda = 1 returns the valid entries in the order (score descending, then position): for a shortlist whose
 *   valid scores do not increase (nrms_topk_dot's) that is its first k valid entries in shortlist order, ids and score bits.
 *   Row b's result is a function of (its shortlist, the item rows it names, lambda, k) only: not of B, the row's position, N,
 *   what the workspace held, or the run.
 * Limits: 1 <= k <= M <= 256, d >= 1, 0 <= lambda <= 1, B >= 0, N >= 0; B = 0 is a no-op, N = 0 writes all-padding rows.
 *   Arguments outside the limits return NRMS_EINVAL with a message naming the argument.
 * Workspace: nrms_mmr_rerank_workspace_bytes(B, M, d, k) bytes, 16-byte aligned (0 = arguments rejected): the dot products
 *   [B, Mp, Mp] fp32, Mp = M rounded up to 64, so 256 KiB per user at M = 256; callers that must bound it split B (a row does
 *   not depend on B).
 * Two kernels on `stream` (the first once per 32 768 users), no host synchronisation, no allocation; plain vector stores only, no
 *   atomics: two runs are bit-identical whatever the workspace held. */
size_t nrms_mmr_rerank_workspace_bytes(int32_t B, int32_t M, int32_t d, int32_t k);
int nrms_mmr_rerank(int32_t B, int32_t M, int32_t d, int32_t k, int64_t N, float lambda,
                    const float* items /* [N, d] */, const int64_t* short_ids /* [B, M] */,
                    const float* short_scores /* [B, M] */,
                    int64_t* out_ids /* [B, k] */, float* out_scores /* [B, k] */,
                    float* out_value /* [B, k], nullable */, float* ild /* [B], nullable */,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- Why this item: a score split exactly over the clicks of the history (csrc/attribution.hip; serving: "because you read
 * ..."; PARITY UNPINNED, the reference explains nothing) ----
 * The user vector of the additive-attention user encoder is u[b] = sum_h w[b, h] ctx[b, h, :] (nrms_encoder_acts.w and .ctx,
 * nrms_v0.py:110-125), so the score of any item x splits over the H history slots: u[b] . x = sum_h w[b, h] (ctx[b, h, :] . x).
 * For each user b < B and each position j < K of the user's list, the H terms, their ordered sum, the m largest of them and the
 * part carried by the slots the caller cannot name.
 * ctx [B, H, d], w [B, H], items [N, d] fp32 row-major; ids [B, K] int64: catalogue rows, e.g. a row of nrms_topk_dot's or
 * nrms_mmr_rerank's output, padding included; slot_named [B, H] uint8, NULLABLE (null = every slot is named); contrib [B, K, H]
 * fp32, NULLABLE; total [B, K] fp32; top_slots [B, K, m] int32; top_contrib [B, K, m] fp32; unnamed_share [B, K] fp32, NULLABLE.
 * Term.  c(b, j, h) = w[b, h] * s(ctx[b, h, :], items[ids[b, j], :]): s is nrms_topk_dot's chain (one fp32 accumulator over all
 *   of d on v_mfma_f32_32x32x2_f32 in the same k order, csrc/topk_entry.h tk_chain), then ONE fp32 multiplication, rounded to
 *   nearest, nothing fused.  The bits of c depend on (the ctx row, the w value, the item row) only: not on B, K, H, m, the position
 *   in the list, the other ids or the run.  s(ctx row, item row) has the bits nrms_rank_dot returns as target_scores when that ctx
 *   row is given as a user row.
 * Total.  total[b, j] = the fp32 sum of c(b, j, h) over h = 0, 1, ..., H - 1 in that order, one sequential chain from +0.0.  It is
 *   the model's score of the item up to the rounding of the two orders of summation.
 * Reasons.  Slot h is ELIGIBLE when slot_named is NULL or slot_named[b, h] != 0, and c(b, j, h) is not NaN.  top_slots[b, j, :]
 *   holds the first min(m, #eligible) eligible slots by c descending, top_contrib their c; equal values put the SMALLER slot first;
 *   -0.0 equals +0.0 and is returned as +0.0 (nrms_topk_dot's order on (c, slot)).  The remaining places hold slot -1 and
 *   contribution -inf.  Negative contributions are listed like any other: the caller cuts at 0.
 * Unnamed share.  unnamed_share[b, j] = the fp32 sum, from +0.0 in slot order, of c(b, j, h) over the slots with slot_named[b, h]
 *   == 0; 0 when slot_named is NULL.  (nrms_v0 masks nothing: a padding slot of the history has a non-zero ctx row and carries part
 *   of the score.  This is that part.)
 * NaN.  A NaN in ctx[b, h, :] or w[b, h] makes c(b, j, h) NaN for every j: slot h is never a reason, total[b, j] is NaN for every
 *   valid j, and unnamed_share[b, j] is NaN if the slot is unnamed.  A NaN in an item row makes every term of the entries that name
 *   it NaN: no reasons, total NaN.  contrib carries the NaNs.  Infinities are ordinary values.
 * Invalid entries.  An entry whose ids[b, j] is outside [0, N) (-1 is the padding of every top-k call here) gets total -inf,
 *   unnamed_share 0, m reasons -1 / -inf and a contrib row of zeros.  No item row is read for it.  An id that occurs twice makes
 *   two entries with the same bits.
 * Limits: 1 <= H <= 64, 1 <= K <= 256, 1 <= m <= 8, d >= 1, 0 <= N <= 0x7FFF0000, B >= 0; B = 0 is a no-op (no pointer is
 *   inspected), N = 0 makes every entry invalid (items may be NULL).  Arguments outside the limits, a NULL required pointer, float /
 *   int32 pointers not 4-byte aligned or ids not 8-byte aligned return NRMS_EINVAL with a message "attribution_dot: ..." naming the
 *   argument; a workspace below the query's size returns NRMS_EWORKSPACE.  Nothing is launched after an error.
 * Every element of total, top_slots, top_contrib and of contrib / unnamed_share when given is written; nothing else is.
 * Workspace: nrms_attribution_dot_workspace_bytes(B, H, d, K, m) bytes, 8-byte aligned, required (0 = arguments rejected).  It is
 *   256 reserved bytes today: a chunk's terms stay in LDS and the call neither reads nor writes the workspace.
 * One kernel on `stream`, one wave per (user, 64 list positions); no host synchronisation, no allocation; plain vector loads and
 *   stores, no atomics: two runs are bit-identical.  Row (b, j) is a function of (ctx[b], w[b], slot_named[b], the item row, m). */
size_t nrms_attribution_dot_workspace_bytes(int32_t B, int32_t H, int32_t d, int32_t K, int32_t m);
int nrms_attribution_dot(int32_t B, int32_t H, int64_t N, int32_t d, int32_t K, int32_t m,
                         const float* ctx /* [B, H, d] */, const float* w /* [B, H] */,
                         const float* items /* [N, d] */, const int64_t* ids /* [B, K] */,
                         const uint8_t* slot_named /* [B, H], nullable */,
                         float* contrib /* [B, K, H], nullable */, float* total /* [B, K] */,
                         int32_t* top_slots /* [B, K, m] */, float* top_contrib /* [B, K, m] */,
                         float* unnamed_share /* [B, K], nullable */,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- nrms_naml pieces around the two encoder passes (model/nrms_naml.py) ----
 * LayerNorm over the last dimension (nn.LayerNorm(news_feature_size) on the history vectors, nrms_naml.py:207,238):
 * y = (x - mean) / sqrt(var + eps) * gamma + beta, biased variance.  stats [n_rows, 2] = (mean, 1/std) is written when
 * non-NULL (the backward needs it). */
int nrms_layernorm_fwd(int64_t n_rows, int32_t d, const float* x, const float* gamma, const float* beta, float eps,
                       float* y, float* stats, void* stream);
size_t nrms_layernorm_bwd_workspace_bytes(int32_t d);
/* dx [n_rows, d] is overwritten; d(gamma) [d] and d(beta) [d] are ACCUMULATED into dgamma_dbeta [2d] (gamma's gradient
 * first: norm.weight and norm.bias are adjacent in the caller's flat gradient buffer).  Reproducible (fixed-order sums). */
int nrms_layernorm_bwd(int64_t n_rows, int32_t d, const float* x, const float* gamma, const float* stats, const float* dy,
                       float* dx, float* dgamma_dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* News feature rows (NewsEncoder.forward, nrms_naml.py:168-175):
 * out[n] = dropout([title_vec[n] | abst_vec[n] | cat_table[categ[n]] | sub_table[subcateg[n]]]), dropout site 3 over
 * [n, 2 d_text + 2 d_cat].  categ / subcateg: int64 [n], already validated (nrms_sanitize_ids with the table's row count). */
typedef struct nrms_news_features {
    int64_t n;               /* slots: B*(H+C) */
    int32_t d_text;          /* config.word_embed_size */
    int32_t d_cat;           /* config.cate_embed_size */
    int32_t n_cat, n_sub;    /* config.category_nums, config.subcategory_nums (table rows; row 0 = padding_idx) */
    float   p_drop;          /* config.dropout in training, 0 in eval */
    uint64_t seed;
    const float* title_vec;  /* [n, d_text] */
    const float* abst_vec;   /* [n, d_text] */
    const float* cat_table;  /* [n_cat, d_cat] */
    const float* sub_table;  /* [n_sub, d_cat] */
    const int64_t* categ;    /* [n] */
    const int64_t* subcateg; /* [n] */
} nrms_news_features;
int nrms_news_features_fwd(const nrms_news_features* f, float* out, void* stream);
/* dout [n, 2 d_text + 2 d_cat] -> d_title_vec, d_abst_vec [n, d_text] (overwritten; d_title_vec also holds the table sums' per-chunk
 * partial results during the call); the table gradients are ACCUMULATED into d_cat_table / d_sub_table, row 0 (padding_idx = 0,
 * nrms_naml.py:107-108) untouched; atomic-free (slot chunks in ascending order). */
int nrms_news_features_bwd(const nrms_news_features* f, const float* dout, float* d_title_vec, float* d_abst_vec,
                           float* d_cat_table, float* d_sub_table, void* stream);

/* ---- Gather + additive-attention aggregate over variable-length segments (BASELINE configs 4-5) ----
 *   out[s] = sum_{k in [seg_ptr[s], seg_ptr[s+1])} alpha_k x[idx[k]],   alpha = softmax over the segment of
 *   q_vec . tanh(W_add x[idx[k]] + b_add)          -- AdditiveAttention (model/nrms_v0.py:100-126) over an index list.
 * It is the aggregation step of a HieRec-style hierarchical interest model (clicked news pooled per sub-topic, sub-topic interests
 * per topic, topic interests per user: each level is this call over a PARTITION of its rows) and of a user-news graph encoder
 * (neighbour gather + attention aggregate: segments = adjacency lists, a row may be a member of many segments).  The reference
 * holds no implementation of either (model/tanr.py is empty): the checker is a torch restatement of the formula
 * (oracle/segpool_oracle.py) -- PARITY UNPINNED.  An empty segment yields a zero row. */
#define NRMS_SEGPOOL_ROWS_UNIQUE 1   /* every row is a member of at most one segment: d(logit) and dx are then plain stores by the
                                        segment's wave; without the flag the backward sorts the list entries by row (stable) and
                                        adds a row's shares in ascending list position -- bit-reproducible either way */
typedef struct nrms_segpool_desc {
    int64_t n_rows;       /* rows of x */
    int64_t n_seg;        /* segments */
    int64_t nnz;          /* members in all segments = seg_ptr[n_seg] */
    int32_t d;            /* row width: multiple of 4, <= 1024 */
    int32_t q;            /* width of the additive attention: multiple of 4, <= 512 */
    int32_t precision;    /* NRMS_PRECISION_FP32 / _BF16X3 / _BF16: the arithmetic of the two projections (x W_add^T and dZ W_add, dZ^T x) */
    int32_t flags;        /* NRMS_SEGPOOL_* */
} nrms_segpool_desc;
size_t nrms_segment_pool_workspace_bytes(const nrms_segpool_desc* desc);
/* x [n_rows, d]; seg_ptr int32 [n_seg + 1] ascending from 0; idx int32 [nnz], every entry in [0, n_rows).  Saved for the backward:
 * t [n_rows, q] = tanh(x W_add^T + b_add), alpha [nnz]; logit [n_rows] is scratch the caller provides.  out [n_seg, d]. */
int nrms_segment_pool_fwd(const nrms_segpool_desc* desc, const float* x, const float* w_add, const float* b_add,
                          const float* q_vec, const int32_t* seg_ptr, const int32_t* idx, float* t, float* logit, float* alpha,
                          float* out, void* workspace, size_t workspace_bytes, void* stream);
/* dout [n_seg, d] -> dx [n_rows, d] (OVERWRITTEN: rows outside every segment get their projection gradient, i.e. zero);
 * dw_add [q, d], db_add [q], dq_vec [q] are ACCUMULATED. */
int nrms_segment_pool_bwd(const nrms_segpool_desc* desc, const float* x, const float* w_add, const float* q_vec,
                          const int32_t* seg_ptr, const int32_t* idx, const float* t, const float* alpha, const float* dout,
                          float* dx, float* dw_add, float* db_add, float* dq_vec, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Index lists from padded neighbour lists (a sampled sub-graph as [n_seg, K] int64 with -1 for "no neighbour"): entries inside
 * [0, n_rows) are kept in their order.  seg_ptr [n_seg + 1], idx [capacity n_seg * K]; pass nnz = n_seg * K (a capacity) in the
 * nrms_segpool_desc -- the lists' real length is seg_ptr[n_seg], on the device.  Without NRMS_SEGPOOL_ROWS_UNIQUE (a row listed
 * by several segments, as in a graph) the backward sorts the list entries by row (stable) and adds a row's contributions in
 * ascending list position: no atomics, the same bits on every run. */
int nrms_csr_from_padded(int64_t n_seg, int32_t K, const int64_t* lists, int64_t n_rows, int32_t* seg_ptr, int32_t* idx, void* stream);

/* ---- Click graph: neighbour sampling for the user-news graph encoder (csrc/graphsample.hip; click_graph.py; PARITY UNPINNED,
 * the reference has no graph model).  The bipartite user-news click graph of the WHOLE data set as two CSRs in HBM; every edge is
 * in both, a user's news and a news's users in ascending id, no duplicates; news id 0 (the padding slot) is never an edge. */
typedef struct nrms_click_graph {
    int64_t n_users, n_news, n_edges;     /* n_news = rows of the catalogue (ids 0 .. n_news - 1), < 2^31; n_users < 2^31 */
    const int64_t* user_ptr;              /* [n_users + 1] */
    const int32_t* user_news;             /* [n_edges] */
    const int64_t* news_ptr;              /* [n_news + 1] */
    const int32_t* news_users;            /* [n_edges] */
} nrms_click_graph;
/* neighbor_ids [n_slots, K] int32, 1 <= K <= 64, n_slots < 0x7f7f7f7f, n_slots * K < 2^31.  Draw t of a slot that shows news j = slot_ids[r]:
 *   r4 = philox4x32_7(seed, group = j * K + t, site 5)          (the counter layout of the dropout sites, csrc/common.h)
 *   deg = news_ptr[j + 1] - news_ptr[j];  -1 if deg == 0, j == 0 or j outside [0, n_news)
 *   u = news_users[news_ptr[j] + ((uint64) r4[0] * deg >> 32)]
 *   m = user_news[user_ptr[u] + ((uint64) r4[1] * deg(u) >> 32)]
 *   -1 if m == j, else m.
 * Repeated neighbours among the K draws are kept.  The result is a function of (graph, j, t, seed) alone: not of the slot, the
 * batch or the call.  Slot ids outside [0, n_news) are counted into *n_bad (device int32, as nrms_sanitize_ids counts).  One
 * kernel, no atomics on the results.  The call needs no workspace today (the query returns 0; workspace may be NULL). */
size_t nrms_graph_sample_workspace_bytes(int64_t n_slots, int32_t K);
int nrms_graph_sample_neighbors(const nrms_click_graph* graph, int64_t n_slots, int32_t K, const int64_t* slot_ids, uint64_t seed,
                                int32_t* neighbor_ids, int32_t* n_bad, void* workspace, size_t workspace_bytes, void* stream);
/* Neighbour news ids -> rows of the batch's numbering, neighbor_rows [n_slots, K] int64 (the input of nrms_csr_from_padded):
 *   a neighbour some slot of the batch shows -> the smallest such slot r (slot_ids[r] == id);
 *   any other neighbour                      -> n_slots + e, e = its rank among the batch's distinct out-of-batch neighbour ids in
 *                                               ascending order, while e < cap; -1 for e >= cap (so the largest ids go first);
 *   -1 (or an id outside (0, n_news))        -> -1.
 * extra_ids [cap] int32 = those distinct ids in ascending order, padded with 0; *n_extra (device int32) = how many are valid;
 * *n_dropped (device int32) += distinct ids of rank >= cap.  No host synchronisation; integer atomicMin / atomicOr only, so two
 * calls with the same inputs give the same bytes.  workspace: nrms_graph_resolve_workspace_bytes(n_news) bytes, 4-byte aligned
 * (two tables over the news ids; the call initialises them).  Intended range: the ranking pass is ONE 1 024-lane workgroup that walks
 * the n_news / 32 bitmap words (4 words per lane and 5 us at 130 000 news; about 0.2 ms at 10^7); larger catalogues stay correct but
 * that pass, and the two tables' memsets (4.1 bytes per news id), grow linearly with n_news, whatever the batch. */
size_t nrms_graph_resolve_workspace_bytes(int64_t n_news);
int nrms_graph_resolve_rows(int64_t n_slots, int32_t K, int64_t n_news, const int64_t* slot_ids, const int32_t* neighbor_ids, int32_t cap,
                            int64_t* neighbor_rows, int32_t* extra_ids, int32_t* n_extra, int32_t* n_dropped, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- Impression log: the negatives of every training row, redrawn per epoch (csrc/negsample.hip; data_handler.py ImpressionFeed).
 * The reference shuffles an impression's non-clicked news once, offline, and gives its i-th clicked item the slice
 * [i * sample_size, (i + 1) * sample_size) of that shuffle (MIND_2020/data_processor.py:519-528).  Here the log stays in HBM as a CSR
 * -- impression i shows shown[imp_ptr[i] .. imp_ptr[i + 1]) with labels label[...] (non-zero = clicked) -- and the shuffle is a
 * ranking by counter-based keys, so a call with another seed is another epoch's draw.  The impression's positives are its clicked
 * entries in shown order, p = 0, 1, ...; sample_ptr [n_imp + 1] is the exclusive scan of the impressions' positive counts, built
 * once by the caller: sample_ptr[i] is the first output row of impression i and n_samples = sample_ptr[n_imp].
 *   key of the entry at log position e = imp_ptr[i] + j:
 *     w(e) = word e & 3 of philox4x32_7(seed, group = e >> 2, site 6)      (the counter layout of the dropout sites, csrc/common.h)
 *   rank of negative j:  r(j) = #{negatives j' of the same impression : (w(e'), j') < (w(e), j)}      (equal words: the earlier position first)
 *   row sample_ptr[i] + p of cand [n_samples, S + 1] int64:
 *     slot 0 = the p-th positive; slots 1 .. = the negatives with p * S <= r < (p + 1) * S in ascending r; the remaining slots 0;
 *     clen [n_samples] int64 = 1 + the number of negatives written (a positive whose slice is empty still has its row, clen = 1).
 * Equal words are the only departure from a uniform shuffle: two of an impression's n negatives share a word with probability
 * below n^2 / 2^33 (5e-4 at n = 2048, 1e-5 at n = 300), and then the earlier one comes first.  The result is a function of (imp_ptr,
 * shown, label, S, seed) alone; every byte of cand and clen is written, with plain stores by one writer each, and nothing else is
 * (but the workspace and *n_bad): two calls with the same inputs give the same bytes.  1 <= S <= 64, 1 <= max_shown <= 2048,
 * n_imp < 2^31.  An impression longer than max_shown gets rows that hold its positives only (clen = 1) and adds one to *n_bad (device
 * int32, as nrms_sanitize_ids counts); so does, without writing anything, an impression whose extent leaves the log or whose rows in
 * sample_ptr are not as many as its positives.  Bad scalar arguments, null pointers and a workspace below
 * nrms_negative_sample_workspace_bytes(n_imp, nnz = imp_ptr[n_imp], S) bytes (4-byte aligned; the call initialises it; the query
 * returns 0 for arguments the call would refuse) return non-zero before any launch.  No host synchronisation.  An impression of at
 * most 64 entries is ranked by one wavefront, a longer one by one workgroup; the workspace lists the latter (an integer counter
 * orders that list, never a result). */
size_t nrms_negative_sample_workspace_bytes(int64_t n_imp, int64_t nnz, int32_t S);
int nrms_negative_sample(int64_t n_imp, const int64_t* imp_ptr /* [n_imp + 1] */, const int32_t* shown /* [nnz] */,
                         const uint8_t* label /* [nnz] */, const int64_t* sample_ptr /* [n_imp + 1] */, int32_t S, int32_t max_shown,
                         uint64_t seed, int64_t* cand /* [n_samples, S + 1] */, int64_t* clen /* [n_samples] */, int32_t* n_bad,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- Click log: negatives from the whole catalogue, redrawn per epoch (csrc/catneg.hip; data_handler.py ClickFeed; PARITY UNPINNED,
 * the reference trains on impressions only).  A data set that records who clicked what, and no impressions, has no non-clicked news
 * to draw from: row r (one click: a user, the clicked news row_pos[r], a key row_key[r] that names the click, e.g. its position in
 * the log) takes S negatives from the catalogue by integer weights.  set_ptr [n_users + 1] / set_news hold every user's distinct
 * clicked news in ascending id (the user side of nrms_click_graph); cum [n_news + 1] is the exclusive running sum of the
 * non-negative weights per news id: cum[0] = cum[1] = 0 (id 0 is the padding slot), nondecreasing, W = cum[n_news] in [1, 2^62].
 *   draw of row key k, slot s = 0 .. S - 1, attempt a = 0 .. 7:
 *     r4 = philox4x32_7(seed, group = ((k * 64 + s) << 2) | (a >> 1), site 7)      (the counter layout of the dropout sites, csrc/common.h)
 *     u = (uint64) r4[2 (a & 1)] << 32 | r4[2 (a & 1) + 1];   x = (u * W) >> 64      (the high half of the 128-bit product: x < W)
 *     n(s, a) = the id with cum[n] <= x < cum[n + 1]                               (an id of weight 0 is never drawn, ties in cum included)
 *   value of slot s = n(s, a) of the FIRST attempt a for which it is not 0, not in set_news[set_ptr[u] .. set_ptr[u + 1]) for
 *     u = row_user[r], and not the value of a slot s' < s of the same row; no value if all eight fail.  A slot depends on lower slots
 *     only: the values for S = 4 are the first four for S = 8.
 *   row r of cand [n_rows, S + 1] int64: slot 0 = row_pos[r], then the valued slots in slot order, packed to the front, then zeros;
 *     clen [n_rows] int64 = 1 + the number of valued slots; *n_short (device int32) += the slots left without a value (informational:
 *     a user whose set covers most of the weight, or a catalogue of fewer than S eligible ids).
 * A row whose user is outside [0, n_users) or whose positive is outside (0, n_news) writes cand = [0 ...], clen = 1, adds one to
 * *n_bad (device int32, as nrms_sanitize_ids counts) and nothing to *n_short.  Every byte of cand and clen is written, by one plain
 * store each; the only atomics are the two integer counters.  The result is a function of (row_key, row_user, row_pos, the sets, cum, S,
 * seed) alone: not of the row's position, n_rows, the launch geometry or what the workspace holds -- a row drawn alone, in another
 * order or on another rank has the same bytes.  1 <= S <= 64, 2 <= n_news < 2^31, 0 <= n_rows < 2^31 (0: nothing is launched),
 * 0 <= n_users < 2^31, 0 <= row_key < 2^48 (the group must not wrap).  Bad scalar arguments, null pointers and a workspace below
 * nrms_catalogue_negative_sample_workspace_bytes(n_rows, n_news, S) bytes (4-byte aligned; reserved, the call touches none of it today;
 * the query returns 0 for arguments the call would refuse) return non-zero before any launch.  No host synchronisation, no allocation.
 * One kernel: a row is a segment of P = next power of two >= S lanes of a wavefront; attempts 2 .. 7 are computed only by
 * wavefronts in which a slot has used up the attempts before them. */
size_t nrms_catalogue_negative_sample_workspace_bytes(int64_t n_rows, int64_t n_news, int32_t S);
int nrms_catalogue_negative_sample(int64_t n_rows, const int64_t* row_key /* [n_rows] */, const int32_t* row_user /* [n_rows] */,
                                   const int32_t* row_pos /* [n_rows] */, int64_t n_users, const int64_t* set_ptr /* [n_users + 1] */,
                                   const int32_t* set_news /* [set_ptr[n_users]] */, int64_t n_news, const int64_t* cum /* [n_news + 1] */,
                                   int32_t S, uint64_t seed, int64_t* cand /* [n_rows, S + 1] */, int64_t* clen /* [n_rows] */,
                                   int32_t* n_short, int32_t* n_bad, void* workspace, size_t workspace_bytes, void* stream);

/* ---- All-padding sequences of the output-projection topology in closed form (csrc/empty_seq.hip; nrms_naml's word-level
 * encoder, model/nrms_naml.py:42-100,121-177: 41 % of a MIND-shaped batch's title / abstract slots are history padding).  With a
 * zero padding row every Q | K | V row of such a sequence is the bias, so attention row i is b_v scaled per head by
 * c_ih = (kept keys of query i) / (seq_len (1 - p_drop_attn)), and W_O, the additive attention and their gradients collapse to
 * products with n_heads + 1 vectors that depend on the weights only.  The caller splits its sequences with nrms_sequence_partition
 * (order[0 .. counts[0]) = sequences with a real token, order[n_seq .. n_seq + counts[1]) = all-padding ones; counts holds
 * nrms_sequence_partition_count_ints(n_seq) ints, device), runs nrms_encoder_fwd / _bwd on the first list's sequences (gathered,
 * desc.seq_index = that list) and these two calls on the second: desc.n_seq = counts[1], seq_index = the second list, out / dout
 * [desc.n_seq, d_model] compact.  Same desc rules as the chain (use_output_proj = 1, no mask, no embedding / context dropout;
 * seq_len <= 64, n_heads <= 8, d_model <= 512, q_dim <= 256); gradients are ACCUMULATED into grads (w_add, b_add, q_vec, w_o, b_o,
 * and the V third of b_qkv; every other gradient of such a sequence is exactly zero), per-wave partial sums in a fixed order. */
size_t nrms_sequence_partition_count_ints(int32_t n_seq);
int nrms_sequence_partition(const int64_t* ids, int32_t n_seq, int32_t seq_len, int32_t* order /* [2 * n_seq] */, int32_t* counts, void* stream);
size_t nrms_encoder_empty_workspace_bytes(const nrms_encoder_desc* desc);
size_t nrms_encoder_empty_saved_bytes(const nrms_encoder_desc* desc);
/* saved: nrms_encoder_empty_saved_bytes(desc) bytes that the forward fills (the rows' kept-key factors and pooling weights) and the
 * backward of the same sequences reads; null in the forward = inference. */
int nrms_encoder_empty_fwd(const nrms_encoder_desc* desc, const nrms_encoder_weights* w, const int32_t* seq_index, float* out,
                           void* saved, void* workspace, size_t workspace_bytes, void* stream);
int nrms_encoder_empty_bwd(const nrms_encoder_desc* desc, const nrms_encoder_weights* w, const int32_t* seq_index, const float* dout,
                           const void* saved, const nrms_encoder_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Index side of a HieRec-style hierarchical interest model (BASELINE configs[3]; SURVEY f-4; PARITY UNPINNED: no reference
 * implementation, checked against oracle/segpool_oracle.py).  A user's clicked news (H <= 64 history slots, `valid` = the
 * batch dict's browsed_mask) are grouped by sub-topic id, the sub-topic groups by topic id, in order of first occurrence; every
 * level's groups live in fixed per-user slots b * H + g.  nrms_hier_tree_build writes the three index lists
 * nrms_segment_pool_fwd / _bwd aggregate over:
 *   level 1: rows = history slots b * H + k;       l1_ptr [B * H + 1], l1_idx [B * H]: one segment per sub-topic group slot
 *   level 2: rows = sub-topic group slots;         l2_ptr [B * H + 1], l2_idx [B * H]: one segment per topic group slot
 *   level 3: rows = topic group slots;             l3_ptr [B + 1],     l3_idx [B * H]: one segment per user
 * and per slot the ids and click counts (l1_sub, l1_top, l1_cnt, l2_top, l2_cnt: int32 [B * H]; count 0 = empty slot),
 * n_valid [B].  Every level partitions its rows (NRMS_SEGPOOL_ROWS_UNIQUE). */
size_t nrms_hier_tree_scratch_bytes(int32_t B, int32_t H);
int nrms_hier_tree_build(int32_t B, int32_t H, const uint8_t* valid, const int64_t* topic, const int64_t* subtopic,
                         int32_t* l1_ptr, int32_t* l1_idx, int32_t* l1_sub, int32_t* l1_top, int32_t* l1_cnt,
                         int32_t* l2_ptr, int32_t* l2_idx, int32_t* l2_top, int32_t* l2_cnt, int32_t* l3_ptr,
                         int32_t* l3_idx, int32_t* n_valid, void* scratch, size_t scratch_bytes, void* stream);
/* interest of an occupied slot = its aggregate + the embedding of its (sub-)topic: u[slot] += table[id[slot]] where cnt[slot] > 0
 * (table [n_ids, d]; an id outside it adds nothing and takes no gradient);
 * backward: dtable[r] += sum of du over the occupied slots with id == r, in a fixed order (per-chunk partial sums in `workspace`,
 * then the chunks in ascending order; no atomics). */
int nrms_hier_add_embedding_fwd(int64_t n_slots, int32_t d, int32_t n_ids, const int32_t* id, const int32_t* cnt, const float* table,
                                float* u, void* stream);
size_t nrms_hier_add_embedding_bwd_workspace_bytes(int64_t n_slots, int32_t d, int32_t n_ids);
int nrms_hier_add_embedding_bwd(int64_t n_slots, int32_t d, int32_t n_ids, const int32_t* id, const int32_t* cnt,
                                const float* du, float* dtable, void* workspace, size_t workspace_bytes, void* stream);
/* Hierarchical matching.  nrms_hier_match: for candidate (b, c) the user's sub-topic / topic group slot with the candidate's ids
 * (-1: the user never clicked there) and the share of the user's clicks in it.  nrms_hier_score_fwd:
 *   score = l_s f_s <n, u1[sub_slot]> + l_t f_t <n, u2[top_slot]> + (1 - l_s - l_t) <n, ug[b]>,  masked slots -1e9.
 * _bwd: dcand, dug overwritten; du1, du2 [B * H, d] ACCUMULATED (zero them first); one wavefront per user, no atomics. */
int nrms_hier_match(int32_t B, int32_t C, int32_t H, const int64_t* cand_topic, const int64_t* cand_subtopic,
                    const int32_t* l1_sub, const int32_t* l1_cnt, const int32_t* l2_top, const int32_t* l2_cnt,
                    const int32_t* n_valid, int32_t* sub_slot, float* sub_frac, int32_t* top_slot, float* top_frac, void* stream);
int nrms_hier_score_fwd(int32_t B, int32_t C, int32_t d, const float* cand, const float* u1, const float* u2, const float* ug,
                        const int32_t* sub_slot, const float* sub_frac, const int32_t* top_slot, const float* top_frac,
                        const uint8_t* mask, float lambda_sub, float lambda_top, float* scores, void* stream);
/* nrms_hier_query: the user side of nrms_hier_score_fwd per catalogue group.  Group g has the ids (group_topic[g],
 * group_subtopic[g]) (int64 [G] each); query [B, G, d] is written with
 *   query[b, g] = cs * u1[ss] + ct * u2[ts] + lg * ug[b],   cs = l_s f_s, ct = l_t f_t, lg = 1 - l_s - l_t,
 * where (ss, f_s) and (ts, f_t) are the slots and shares nrms_hier_match gives a candidate with group g's ids, and a term
 * whose slot is -1 is 0 -- the element expression of nrms_hier_score_fwd, so query[b, g] . n is user b's score for a news
 * vector n of group g.  1 <= H <= 64, G >= 1; B = 0 is a no-op.  One kernel on `stream`. */
int nrms_hier_query(int32_t B, int32_t H, int32_t G, int32_t d, const int64_t* group_topic, const int64_t* group_subtopic,
                    const int32_t* l1_sub, const int32_t* l1_cnt, const int32_t* l2_top, const int32_t* l2_cnt,
                    const int32_t* n_valid, const float* u1, const float* u2, const float* ug, float lambda_sub,
                    float lambda_top, float* query, void* stream);
int nrms_hier_score_bwd(int32_t B, int32_t C, int32_t d, const float* cand, const float* u1, const float* u2, const float* ug,
                        const int32_t* sub_slot, const float* sub_frac, const int32_t* top_slot, const float* top_frac,
                        const uint8_t* mask, float lambda_sub, float lambda_top, const float* dscores, float* dcand, float* du1,
                        float* du2, float* dug, void* stream);

/* The keep mask (1 = kept) the encoder kernels apply at a dropout site, for n_rows x d
 * elements: site 0 = embedding dropout (nrms_v0.py:137), site 1 = context dropout (:171-173), site 2 = attention
 * probabilities ([n_seq * n_heads * seq_len, seq_len], nrms_naml.py:36-39), site 3 = news feature rows (:175).
 * Lets a test replay a training step through the oracle with identical masks. */
#define NRMS_DROPOUT_FIELDS16 0x100   /* or-ed into `site`: the 16-bit-field scheme of the fp16 mode's context dropout --
                                        one Philox call per 8 elements of the flat [n_rows, d] layout, P(drop) = p rounded
                                        down to a multiple of 2^-16.  The fp16 kernels apply it over the padded [tokens, 320]
                                        layout with the two middle bits of a column's index inside its 32-column head block
                                        swapped: mask of column 16a + 8b + 4c + e = field at 16a + 8c + 4b + e */
int nrms_dropout_keep_mask(uint64_t seed, int32_t site, int64_t n_rows, int32_t d, float p_drop,
                           uint8_t* keep, void* stream);

/* nrms_bert's news-vector layer (BertNewsEncoder, model/nrms.py:216-256): slot s of a batch (B*H history slots, then B*C
 * candidate slots) holds news id ids[s]; its vector is dropout(table[ids[s]] W^T + b), table [n_rows, d] the fine-tuned
 * pretrained vectors (no padding row: id 0 is an ordinary row), W [d, d], b [d] (news_dense.0).  Dropout site 4 over the
 * [n_slots, d] output (nrms_dropout_keep_mask(seed, NRMS_DROPOUT_SITE_NEWSVEC, n_slots, d, p_drop) replays it). */
#define NRMS_DROPOUT_SITE_NEWSVEC 4
typedef struct nrms_newsvec_desc {
    int64_t  n_slots;      /* B * (H + C) */
    int32_t  n_rows;       /* rows of the table (news ids 0 .. n_rows - 1) */
    int32_t  d;            /* width E, a multiple of 4, <= 1024 */
    int32_t  precision;    /* NRMS_PRECISION_FP32, _BF16X3 or _BF16 (the dense products) */
    float    p_drop;       /* dropout on the slot vectors (model/nrms.py:254); 0 in eval */
    uint64_t seed;         /* counter-based RNG key of the step */
} nrms_newsvec_desc;
/* `saved`: caller-owned bytes the forward writes and the backward of the same batch reads (the distinct ids, ascending, and
 * the slot -> id-group maps); `workspace`: scratch of either direction.  Both 256-byte aligned. */
size_t nrms_newsvec_saved_bytes(const nrms_newsvec_desc* desc);
size_t nrms_newsvec_workspace_bytes(const nrms_newsvec_desc* desc);
/* Forward.  Ids outside [0, n_rows) are read as 0 and counted into *n_bad (device int32; may be NULL), as nrms_sanitize_ids
 * does.  The batch's distinct ids are grouped on the device (stable sort), each goes through the dense layer once, the slots
 * then receive their group's row through the dropout.  No host synchronisation.  out: [n_slots, d]. */
int nrms_newsvec_fwd(const nrms_newsvec_desc* desc, const int64_t* ids, const float* table, const float* w, const float* b,
                     float* out, void* saved, size_t saved_bytes, int32_t* n_bad, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Backward of the forward that filled `saved`: the slot gradients dout [n_slots, d] are undone through the dropout and summed
 * per distinct id in slot order (no atomics; bit-reproducible); d_w, d_b are ACCUMULATED from the distinct rows; the rows of
 * d_table [n_rows, d] of the batch's distinct ids are OVERWRITTEN with their gradient (plain stores), every other row is left
 * as it is (the caller zeroes the buffer: rows outside the batch have gradient 0). */
int nrms_newsvec_bwd(const nrms_newsvec_desc* desc, const float* table, const float* w, const float* dout, const void* saved,
                     size_t saved_bytes, float* d_table, float* d_w, float* d_b, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Device copies of what a forward left in `saved`: *n_unique (int32) and, if ids is not NULL, the distinct ids in ascending
 * order (ids [n_slots] int32, the first *n_unique valid). */
int nrms_newsvec_distinct(const nrms_newsvec_desc* desc, const void* saved, int32_t* n_unique, int32_t* ids, void* stream);
/* Every row of the table through the dense layer, no dropout (catalogue retrieval, evaluation): out [n_rows, d]. */
size_t nrms_newsvec_rows_workspace_bytes(int64_t n_rows, int32_t d, int32_t precision);
int nrms_newsvec_rows_fwd(int64_t n_rows, int32_t d, int32_t precision, const float* table, const float* w, const float* b,
                          float* out, void* workspace, size_t workspace_bytes, void* stream);

/* In-batch sampled softmax: every row of the batch is scored against the batch's whole candidate pool (csrc/poolce.hip).
 * M = B * C pool columns, cand [M, d] (row b's own candidates are columns b*C .. b*C + C - 1), own(b) = b*C the column of row
 * b's positive.  Column j is LIVE if cand_mask is NULL or cand_mask[j] != 0; row b is live if its own column is.  For a live row b,
 * column j is IN THE SOFTMAX OF b if j == own(b), or if j is live, cand_id[j] != cand_id[own(b)] and cand_id[j] is not among
 * reject[b, 0:R) (entries of reject that are <= 0 match nothing).  Duplicate ids in the pool count as often as they occur.
 *   z[b, j]   = <user[b], cand[j]> + col_bias[j]          fp32 products, fp32 accumulation in ascending k; col_bias NULL = 0
 *                                                          (the positive's column takes its bias too: the logQ correction of
 *                                                          Yi et al. 2019 is col_bias[j] = -log q(cand_id[j]))
 *   loss_b    = logsumexp_{j in the softmax of b} z[b, j] - z[b, own(b)]
 *   g[b, j]   = (softmax_b[j] - [j == own(b)]) * grad_scale for the columns in the softmax of b; every other entry, and every entry
 *               of a dead row, is exactly 0
 *   loss_sum[0] += sum over the live rows of loss_b        (the caller divides by the batch, as for nrms_ce_loss_fwd_bwd)
 *   duser[b]  = sum_j g[b, j] cand[j]                      written, not accumulated
 *   dcand[j]  = sum_b g[b, j] user[b]                      written, not accumulated
 *   n_pairs[0] += the number of pairs (b, j != own(b)) with j in the softmax of b      (device int64; may be NULL)
 * dcand and duser both NULL: the loss only.  Vectors at dead slots must be finite (they are multiplied by 0).
 * Domain: 1 <= B <= 4096, 1 <= C <= 64, B*C <= 32768, 1 <= d <= 1024, 0 <= R <= 256; reject is NULL exactly when R == 0.  Anything
 * else, a workspace smaller than the query's answer (which is 0 for a refused shape), or exactly one of dcand / duser being NULL
 * returns NRMS_EINVAL before any launch.  `workspace` holds the [B, M] fp32 matrix z, later g (materialised on purpose: 5 MB at
 * B = 512, C = 5), the row losses and the K slabs of duser; nothing is assumed about its contents.  Every sum has a fixed order
 * (the only atomic is the integer n_pairs), so two calls on the same inputs give the same bits.  The denominator, the log and the
 * reciprocal of a row are formed in double and rounded once, as in nrms_ce_loss_fwd_bwd.  No allocation, no host synchronisation;
 * up to six kernels on `stream`, each timed under a name that starts with "pooled_ce". */
size_t nrms_pooled_ce_workspace_bytes(int32_t B, int32_t C, int32_t d, int32_t R);
int nrms_pooled_ce_fwd_bwd(int32_t B, int32_t C, int32_t d, int32_t R, const float* cand, const float* user, const int64_t* cand_id,
                           const uint8_t* cand_mask, const int64_t* reject, const float* col_bias, float grad_scale, float* loss_sum,
                           float* dcand, float* duser, int64_t* n_pairs, void* workspace, size_t workspace_bytes, void* stream);

/* Per-kernel device timing (HIP events on the launch stream), for bench.py's roofline leg.
 * nrms_timing_read synchronises the recorded events; returns 0 and the accumulated
 * milliseconds / launch count of kernels whose name starts with `prefix`. */
void nrms_timing_enable(int enable);
void nrms_timing_reset(void);
int  nrms_timing_read(const char* prefix, double* total_ms, int64_t* launches);

const char* nrms_last_error(void);
const char* nrms_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NRMS_HIP_H */
