/*
 * libmmscore -- C ABI of the MI355X-native (gfx950) cross-modal pair scorer.
 *
 * The reference (zuokai/KDDCUP_2020_MultimodalitiesRecall_2nd_Place) has no FFI of its own: its
 * hot path is entered through three Python/TF1/PyTorch call surfaces.  Each entry point below
 * replaces one of them (paths relative to the reference root):
 *
 *   mms_score_zk      <- model_triple.model_attention_channel_e(...)  code/imagebert_zk/model_triple.py:162-214,
 *                        driven by sess.run([probs, ...])              code/imagebert_zk/evaluate_normal.py:227-238
 *   mms_score_lds     <- bertmodel(... features ...)                   code/imagebert_lds/src/run_pretraining_predict_score.py:288-336,
 *                        get_next_sentence_output                      :479-501, sess.run :566-570
 *   mms_score_lxmert  <- KDDModel.forward(...)                         code/lxmert/src/tasks/kdd_model.py:183-214,
 *                        called from KDD.predict                       :97-100
 *   mms_load_weight   <- tf.train.Saver.restore / load_state_dict      evaluate_normal.py:204-212,
 *                        run_pretraining_predict_score.py:558-563, kdd_model.py:131-152
 *                        (tensor names are the reference's own checkpoint variable names)
 *
 * Conventions
 *   - plain C, no torch / STL types; every function returns an int status (0 = MMS_OK) and never
 *     throws; mms_last_error(h) gives the message of the last failing call on that handle.
 *   - all batch pointers are DEVICE pointers (HBM-resident inputs) unless the field says host;
 *     the caller owns every input/output buffer, the handle owns weights and workspace.
 *   - one handle per GPU/stream; calls on one handle must be serialised by the caller; kernels are
 *     enqueued asynchronously on the hipStream_t passed as `stream` (NULL = default stream).
 *     Host synchronisation points inside a scoring call (each a 4-byte device->host read + hipStreamSynchronize of `stream`):
 *       * dense label ids (uniq_label_ids == NULL): the count of distinct label tuples, once per call;
 *       * lxmert / ensemble with pack_tokens = 1 and >= 2 pairs: the count of distinct (input_ids, input_mask) rows, once per call
 *         -- ALSO when the caller passes uniq_label_ids (the language layers run once per distinct query, api.hip lx_query_stage);
 *       * ensemble: the per-wave counts of pairs whose query the sen2forest rewrite changed, once per call;
 *       * a workspace that has to grow (first call, or a larger batch than any before) allocates, which synchronises the device.
 *     A zk / lds call with de-duplicated labels on a warmed-up handle is fully asynchronous.
 *     Memory: the workspace is sized for the largest launch wave seen (<= chunk_pairs pairs, ~1 MB per pair); lxmert additionally
 *     keeps the language rows of the distinct queries of the largest BATCH seen (Q x text_len x 768 x 4 bytes, Q <= B / 2) outside
 *     the per-wave workspace; nothing shrinks before mms_destroy.
 *   - integer dtypes are the reference feed dtypes (zk: int32 ids, int64 labels; lds/lxmert: int64).
 *   - the library reads no environment variable (A/B knobs and timing-only diagnostics live in the separate lab build,
 *     csrc/Makefile `make lab`, which the package never loads).
 */
#ifndef MMSCORE_H
#define MMSCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_OK 0
#define MMS_ERR_ARG 1
#define MMS_ERR_WEIGHT 2
#define MMS_ERR_HIP 3
#define MMS_ERR_STATE 4

#define MMS_MODEL_ZK 0
#define MMS_MODEL_LDS 1
#define MMS_MODEL_LXMERT 2

typedef struct mms_handle mms_handle;

typedef struct mms_config {
    int32_t model;            /* MMS_MODEL_* */
    int32_t layers;           /* zk/lds: encoder layers (12); lxmert: language layers (9) */
    int32_t r_layers;         /* lxmert: relational (vision) layers (5) */
    int32_t x_layers;         /* lxmert: cross-modality layers (5) */
    int32_t vocab;            /* 21128 */
    int32_t inter;            /* 3072, multiple of 128 */
    int32_t max_pos;          /* 512 */
    int32_t type_vocab;       /* 2 */
    int32_t text_len;         /* zk/lds 20, lxmert 23 */
    int32_t precision;        /* 1: bf16 activations, one MFMA pass; 2: split-bf16 activations (hi+lo), two passes, GEMM
                                 weights stored as bf16; 3: activations AND weights split (three passes): follows an
                                 arbitrary fp32 checkpoint to ~2e-5; 4: fp8 (OCP e4m3) weights with one fp32 scale per output
                                 channel and fp8 activations on the four big encoder GEMM classes (QKV, attention output,
                                 FFN up / down), fp8 MFMA -- BASELINE.json config 5; OUTSIDE the 1e-3 logit contract, its measured
                                 deviation is reported by the tests and bench.py.  The fp8 activation stores SATURATE: beyond +-448,
                                 infinities included, the largest finite code -- and a NaN becomes -448 (the clamp in front of the
                                 conversion drops it), so a NaN that arises inside a precision-4 forward is not visible in its logits */
    int32_t chunk_pairs;      /* max pairs per internal launch wave (0 = default 32768); a batch is cut into equal chunks */
    int32_t stop_after;       /* debug: run only the first n encoder layers (-1 = all) and skip nothing else */
    int32_t device;           /* HIP device ordinal */
    int32_t pack_tokens;      /* 1 = skip token rows that cannot change a logit; 0 = the reference's padded rows.
                                 zk / lxmert: padded tokens whose keys are masked are dropped (a masked key's softmax weight is
                                 exactly 0 in fp32).  lds has no mask (pixelmodel.py:189-190), but its feature and label tokens carry
                                 no position embedding, so identical rows of a pair (the zero-padded boxes, boxes of one class) stay
                                 identical through every layer: one representative is kept and its key carries log(multiplicity) --
                                 the same softmax and the same P V up to fp32 round-off */
    int32_t fuse_layernorm;   /* mask -- bit 0: the attention-output projections, bit 1: the FFN-down projections of launches with
                                 >= 16384 rows add bias + residual and apply the LayerNorm in their GEMM epilogue (gemm_pp_ln.h: the
                                 residual rides in as eight extra K stages against an identity built in registers, the three column
                                 tiles of a row panel exchange row statistics across workgroups; precision mode 2 only), instead of
                                 writing the fp32 sum for a separate LayerNorm kernel.  Same results to fp32 round-off (one-pass
                                 variance); 12 -> 6 KB of HBM traffic per row and LayerNorm, no LayerNorm launches; +1.5 % on the
                                 bench batch.  scorers.py passes 3; a launch whose workgroups are not all
                                 resident (GPU shared with another process) falls back to the two-kernel route by itself */
    int32_t fuse_attention;   /* 1: the self-attention sub-layers of launches with >= 16384 rows run the Q / K / V projection and the
                                 attention in ONE kernel (qkv_attn.hip: a workgroup projects one head of a 256-row tile, keeps the 192
                                 result columns in LDS and attends from there), so the fp32 [rows][2304] Q | K | V tensor never goes
                                 through HBM.  Precision modes 2 and 3 (mode 3: a 192-row tile variant with the weights' lo plane in the ring); context
                                 rows bit-identical to the two-kernel route.
                                 2: the attention's Q K^T and P V on split-bf16 MFMAs (hi + lo operands, three products, v_exp_f32 / v_rcp_f32 softmax)
                                 instead of exact-fp32 MFMAs: ~2^-16 relative on the scores.  Precision mode 2 runs the 8 x 1-wave kernel (Q operands
                                 straight from the accumulators, K / V staged as bf16 planes in LDS, 16-query tiles attended block-diagonally over the
                                 pairs they touch with an online softmax): any pair length that fits a 128-row sub-tile, lxmert's 10-token box stream
                                 included, and BOTH directions of lxmert's cross-attention (lxrt/modeling.py:460-464) in one launch per X layer.
                                 scorers.py's "auto": 2 in precision mode 2, 1 in mode 3 */
} mms_config;

/* zk feed, code/imagebert_zk/evaluate_normal.py:141-152.  np_idx_class_labels [B,10,8] is either passed as the reference
 * feeds it (`label_ids`, dense: the library finds the distinct 8-id tuples itself -- the label-text encoder depends on the
 * tuple only -- which costs one 4-byte device->host read on `stream` per call), or already de-duplicated by the caller:
 * uniq_label_ids [U,8] + label_index [B,10] (U = B*10 and index = arange reproduces the dense graph).  uniq_label_ids ==
 * NULL selects the dense form. */
typedef struct mms_zk_batch {
    int64_t n_pairs;
    const int32_t* num_boxes;      /* [B] */
    const float* boxes_5;          /* [B,10,5] */
    const float* feats;            /* [B,10,2048] */
    const int32_t* uniq_label_ids; /* [U,8] or NULL */
    int64_t n_uniq_labels;
    const int32_t* label_index;    /* [B,10] -> row of uniq_label_ids (values outside [0,U) are clamped) */
    const int32_t* query_ids;      /* [B,text_len] */
    const int32_t* len_query;      /* [B] */
    const int64_t* labels;         /* [B] (AM-softmax head is label dependent, model_triple.py:68-81) */
    const int32_t* segment_ids;    /* [B,text_len+10]; ids are clamped to [0, type_vocab) */
    const int32_t* label_ids;      /* [B,10,8] dense np_idx_class_labels, read when uniq_label_ids == NULL */
} mms_zk_batch;

/* lds feed, code/imagebert_lds/src/run_pretraining_predict_score.py:526-548 (boxes is unused there) */
typedef struct mms_lds_batch {
    int64_t n_pairs;
    const int64_t* input_ids;      /* [B,text_len] */
    const int64_t* segment_ids;    /* [B,text_len] */
    const float* features;         /* [B,10,2048] */
    const int64_t* labelfeat;      /* [B,10,8] */
} mms_lds_batch;

/* lxmert feed, code/lxmert/src/tasks/kdd_model.py:183-186 (label text dense or de-duplicated, as for zk) */
typedef struct mms_lxmert_batch {
    int64_t n_pairs;
    const int64_t* input_ids;      /* [B,text_len] */
    const int64_t* input_mask;     /* [B,text_len] */
    const int64_t* uniq_label_ids; /* [U,8] or NULL */
    int64_t n_uniq_labels;
    const int32_t* label_index;    /* [B,10] */
    const float* feats;            /* [B,10,2048] */
    const float* boxes;            /* [B,10,4] */
    const float* visual_attention_mask; /* [B,10] */
    const int64_t* label_ids;      /* [B,10,8] dense boxes_label_input_ids, read when uniq_label_ids == NULL */
    float* x_norm;                 /* optional OUTPUT, device fp32 [B,768]: pooled / max(||pooled||, 1e-12), the first element
                                      of KDDModel.forward's return tuple (kdd_model.py:204-205,214); NULL = not wanted */
} mms_lxmert_batch;

/* The three models on the SAME pairs in one call -- BASELINE.json config 5, what code/main.py:41-59 merges from four score files:
 * imagebert_zk on the query, imagebert_zk on its sen2forest rewrite (evaluate_normal_sen2fs.py, load_data_v4.py:153-154),
 * imagebert_lds and lxmert.  One TSV record feeds all of them (load_data_v4.py:133-163, load_data_pred.py:94-121,
 * lxmert/src/utils.py:23-59), so the image side is passed ONCE: the 2048-d box features are split into operand planes once per
 * launch wave, the class-name tuples are de-duplicated once, zk's image-token stage (label conv, kdd_conv2, kdd_dense1,
 * kdd_featureemb: model_triple.py:189-195, pixelbert.py:449-452) runs once for both query variants.  All ids are int32 here. */
typedef struct mms_ensemble_batch {
    int64_t n_pairs;
    const float* feats;            /* [B,10,2048] */
    const float* boxes_5;          /* [B,10,5] = corners/[h,w,h,w] + area (load_data_v4.py:141-147); lxmert reads the 4 corners */
    const int32_t* num_boxes;      /* [B]; lxmert's visual mask = box index < min(num_boxes, 10) */
    const int32_t* label_ids;      /* [B,10,8] */
    const int32_t* query_ids;      /* [B,zk.text_len]  zk + lds query ([CLS] .. [SEP], zero padded) */
    const int32_t* len_query;      /* [B] */
    const int32_t* s2f_query_ids;  /* [B,zk.text_len]  the sen2forest rewrite of the same query */
    const int32_t* s2f_len_query;  /* [B] */
    const int64_t* labels;         /* [B] zk AM-softmax label (1 on testB, ground truth on valid: load_data_v4.py:259-265) */
    const int32_t* lx_input_ids;   /* [B,lxmert.text_len]  lxmert tokenizer flavour */
    const int32_t* lx_input_mask;  /* [B,lxmert.text_len] */
} mms_ensemble_batch;

/* ABI revision of the structs and entry points declared in this header.  It changes whenever a struct gains a field or an entry
 * point changes its signature (r1: 1; r2 added mms_config.fuse_layernorm, mms_zk_batch.label_ids, mms_lxmert_batch.label_ids / x_norm
 * without bumping it; r3: 3, then 4 with mms_config.fuse_attention; r4: 5 -- mms_dbg_gemm takes the engine per call,
 * the process-global mms_set_gemm_variant and the lab engines' hooks left the product library, fuse_layernorm became a mask; r5: 6 -- mms_dbg_qkv_attn and mms_side_lane_flops added; r7: 7 -- mms_decode_feats_b64 added; r8: 8 -- mms_rank_workspace_bytes and mms_rank_submission added; r9: 9 -- mms_ndcg_workspace_bytes, mms_key_relevance and mms_ndcg_at_k added; r10: 10 -- mms_ndcg_sweep_workspace_bytes and mms_ndcg_weight_sweep added; r11: 11 -- mms_filter_sweep_workspace_bytes and mms_filter_sweep added; r12: 12 -- mms_joint_sweep_workspace_bytes and mms_joint_sweep added; r13: 13 -- mms_joint_sweep_codes, mms_resample_workspace_bytes and mms_resample_select added; r14: 14 -- mms_cascade_workspace_bytes, mms_cascade_select and mms_score_ensemble_cascade added; r15: 15 -- mms_normalize_workspace_bytes and mms_normalize_members added; r16: 16 -- mms_plan_stage, mms_score_ensemble_plan, mms_cascade_safe_workspace_bytes and mms_cascade_select_safe added).  A caller built against another revision would make the library read past its structs, so compare
 * BEFORE the first mms_create:  if (mms_version() != MMS_ABI_VERSION) abort();   (lib.py's load() does) */
#define MMS_ABI_VERSION 16
int mms_version(void);
const char* mms_global_error(void);              /* message of the last failing mms_create / mms_decode_feats_b64 / mms_rank_submission / mms_key_relevance / mms_ndcg_at_k / mms_ndcg_weight_sweep / mms_filter_sweep / mms_joint_sweep / mms_joint_sweep_codes / mms_resample_select / mms_cascade_select / mms_cascade_select_safe / mms_normalize_members */

int mms_create(const mms_config* cfg, mms_handle** out);
void mms_destroy(mms_handle* h);
const char* mms_last_error(const mms_handle* h);

/* host fp32 tensor, copied; names = reference checkpoint variable names (see weights.py) */
int mms_load_weight(mms_handle* h, const char* name, const float* host_data, const int64_t* shape, int32_t rank);
/* builds the device-resident model: bf16 [N][K] GEMM matrices (fused QKV), fp32 tables/vectors */
int mms_finalize(mms_handle* h);

/* logits / probs: device fp32 [B,2] (probs may be NULL).
 * Pairs are independent: how a caller groups them into calls (or mms_config.chunk_pairs into launch waves) changes a logit by fp32 summation
 * order at most (~1e-5 relative), and not at all between launches of the same SIZE REGIME.  A launch's regime is decided by its PADDED row bound
 * (pairs x sequence length of the stream; the live count stays on the device), per projection class -- every boundary that changes a summation order:
 * GENERATED REGIMES BEGIN (tools/gen_regime_doc.py from csrc/regimes.h -- do not edit)
 *   rows <= 128     SKINNY_ROWS      [speed choice only: bit-identical across it]  every projection on the skinny kernel (gemm_skinny.hip), K sliced
 *                                    exactly as the tile route of the same projection slices it
 *   rows <  1024    TINY_ROWS        wide projections (N >= 1536, K = 768: QKV, K | V, FFN-up): K in 4 slices, summed in fixed order
 *                                    (k_splitk_reduce)
 *   rows >= 1024    FUSED_ATTN_ROWS  mms_config.fuse_attention: a stream's QKV projection + attention in one kernel (qkv_attn.hip); 1 = the
 *                                    two-kernel route's arithmetic (bit-identical to it), 2 = split-bf16 attention over 16-query tiles of a packed
 *                                    sub-tile: a pair's logits depend on its place in the launch by fp32 round-off (<= 1e-4 relative)
 *   rows <  4096    TALL_ROWS        the long-K projections in front of the encoder (K >= 2048, N = 768: zk kdd_conv1 as im2col, kdd_conv2 / visn_fc
 *                                    / featureemb over the box rows): K in 8 slices
 *   rows >= 4096    SPLITK_HALF_ROWS the LayerNorm-followed K >= 2048 projections (FFN-down) of the split-K regime: 4 K slices instead of 8
 *   rows >= 5120    PP_WIDE_ROWS     [speed choice only: bit-identical across it]  wide projections (N >= 1536) on the persistent ping-pong engine
 *                                    instead of the 128 x 256 tiles (same contraction order per element)
 *   rows <  8192    SPLITK_ROWS      the N = 768 projections that a LayerNorm follows (attention output, FFN-down): K in 4 (K = 768) / 8 or 4 (K >=
 *                                    2048) slices, summed by the LayerNorm kernel
 *   rows >= 11264   SPLITK2_LO_ROWS  FFN-down (K = 3072) of launches below PP_ROWS: 2 K slices (one pass between SPLITK_ROWS and here)
 *   rows >= 16384   PP_ROWS          [speed choice only: bit-identical across it]  persistent ping-pong engines for every projection (same
 *                                    contraction order per element as the tiles: bit-identical, tested)
 *   rows >= 98304   LNF_ROWS         mms_config.fuse_layernorm: bias + residual + LayerNorm in the GEMM epilogue (one-pass variance) -- not in a call
 *                                    that runs on launch lanes, see LANE_ROWS / ENS_LANE_ROWS
 *   rows <  200000  ENS_LANE_ROWS    mms_score_ensemble: the three members of a launch wave (rows of its longest member; ~5000 pairs) side by side on
 *                                    three streams, every LayerNorm by its own kernel
 *   rows <  400000  LANE_ROWS        lxmert calls (pairs x (text_len + 10) rows; ~12 500 pairs): the two streams' launch chains on two lanes, every
 *                                    LayerNorm by its own kernel (with or without per-launch timing)
 * GENERATED REGIMES END
 * (below TINY_ROWS / SPLITK_ROWS / PP_ROWS a projection runs on the register-staged / LDS-DMA 128 x 256 tiles, one pass over K unless a line above says otherwise.)
 * Batch composition enters in two more places: lxmert with pack_tokens runs its language layers once per DISTINCT query when at least half of the pairs
 * share theirs (the rows of that stage = distinct queries x text_len), and label texts are encoded once per distinct 8-id tuple (rows = tuples).
 * mms_score_ensemble runs the three members of a launch wave of fewer than 5000 pairs side by side on three streams (same rule: every LayerNorm by its own kernel; a member's
 * scores equal the single-model call's bit for bit wherever that call would not have used the fused epilogue either, i.e. below 98304 token rows).
 * lxmert's two launch lanes (a side stream between fork / join events: the vision stream's sub-layers beside the language stream's between two cross attentions, the
 * distinct-query stage beside the box stream's layers) run the same kernels on the same operands: no numerical effect beyond the LayerNorm route named above.
 * Not numerical boundaries (same arithmetic, tested bit-identical): the ping-pong engine taken for the wide projections (N >= 1536) from 5120 rows on and for every
 * projection from 16384, the LDS-DMA tile variant taken when a launch has no more workgroups than CUs, the
 * read-back-free label de-duplication of calls of <= 51 pairs, packed vs. dense token layout.
 * A call is ~110 (zk, lds) to ~220 (lxmert) dependent launches: 0.6 - 1.1 ms at 1 pair, so batch thousands of pairs per call when
 * throughput matters ("Call sizes"). */
int mms_score_zk(mms_handle* h, const mms_zk_batch* b, float* logits, float* probs, void* stream);
int mms_score_lds(mms_handle* h, const mms_lds_batch* b, float* logits, float* probs, void* stream);
int mms_score_lxmert(mms_handle* h, const mms_lxmert_batch* b, float* logits, float* probs, void* stream);
/* merged[i] = w[0]*zk(query) + w[1]*zk(sen2forest query) + w[2]*lds + w[3]*lxmert, each member = softmax(logit)[1]
 * (main.py:59: w = 0.2, 0.2, 0.3, 0.3).  merged: device fp32 [B]; member_scores: optional device fp32 [4,B] (the four columns
 * main.py reads from the score files).  The three handles must live on the same device; zk and lds share text_len. */
int mms_score_ensemble(mms_handle* zk, mms_handle* lds, mms_handle* lxmert, const mms_ensemble_batch* b, const float* weights4,
                       float* merged, float* member_scores, void* stream);

/* Cascade form of mms_score_ensemble (opt-in, approximate by construction): the cheapest member prunes, the other three score what is left.
 * Inputs are those of mms_score_ensemble plus group_ids [B] (device int64: the query id of each pair; rows of a query need not be adjacent;
 * MMS_RANK_RESERVED_ID is reserved) and keep >= 1.
 *   Stage 1.  x[i] = the lxmert member's score, softmax(logit)[1], of EVERY pair, computed exactly as mms_score_ensemble computes member 3 for the
 *     same batch: bit-equal to member 3 of mms_score_ensemble on the same feed (and to mms_score_lxmert wherever the text above promises that).
 *   Selection (mms_cascade_select).  Within each query the rows are ordered by (x descending, row index ascending); -0.0 == +0.0: the comparison
 *     is made on the fp32 value widened exactly to double.  The first min(keep, rows) rows of that order are KEPT.  kept_list holds the kept row
 *     indices in ascending row order, n_kept is their number.
 *   Stage 2.  The kept rows are gathered, in kept_list order, into a batch of their own (a device copy of the eleven arrays of mms_ensemble_batch,
 *     the box features in 16-byte accesses), and members 0, 1, 2 are computed for it.  BIT-EQUALITY RULE: they are bit-equal to what
 *     mms_score_ensemble returns for that gathered batch passed as a call of its own -- the label de-duplication runs over the kept pairs, the launch
 *     waves, size regimes, lanes and LayerNorm route are those of a batch of n_kept pairs; nothing of stage 1 is reused.
 *   Output.   member_scores[0..2][i] = the stage-2 score of a kept pair, exactly 0.0f for a pruned pair; member_scores[3][i] = x[i] for both.
 *     merged[i] = ((w0 * m0 + w1 * m1) + w2 * m2) + w3 * m3 on these four values, every product and sum rounded to fp32 on its own (the merge of
 *     mms_score_ensemble); for a pruned pair that is ((w0 * 0 + w1 * 0) + w2 * 0) + w3 * x[i].  kept[i] (device uint8 [B]) = 1 / 0; *n_kept_out
 *     (host, optional) = the number of kept pairs.
 *   ORDERING GUARANTEE.  For non-negative weights and member scores in [0, 1], every kept pair of a query has merged >= every pruned pair of the same
 *     query: x(kept) >= x(pruned) by the selection, the other three terms are >= 0, and fp32 rounding is monotone.  The per-query top of `merged`
 *     therefore consists of kept pairs as long as the query has that many.
 *   Batch boundaries.  The call sees one batch: a query that the caller cuts across two calls is selected per part, and the union of the parts'
 *     selections contains the whole-query selection -- never fewer pairs kept than specified, only (rarely) more.
 *   Flags (first status word of mms_cascade_select): a non-finite x, a group id equal to MMS_RANK_RESERVED_ID, B > MMS_CASCADE_MAX_ROWS.  On any flag
 *     EVERY pair is kept, i.e. the call returns the full ensemble result (detected, served by the exact form).  With keep >= the rows of the largest
 *     query the result equals mms_score_ensemble's bit for bit, merged and member_scores.
 *   Cost.  Two label de-duplication read-backs (one per stage) and the second zk member's count read, as in mms_score_ensemble, plus ONE 16-byte device ->
 *     host read of the status word between the stages.  The buffers of the gathered batch and of the selection live in the zk handle and grow on
 *     demand: a warmed-up handle does not allocate.  The caller's current device is restored on return.
 * Returns MMS_ERR_ARG for keep < 1, a NULL group_ids / kept with B > 0, B >= 2^31, and whatever mms_score_ensemble rejects. */
int mms_score_ensemble_cascade(mms_handle* zk, mms_handle* lds, mms_handle* lxmert, const mms_ensemble_batch* b, const int64_t* group_ids,
                               int32_t keep, const float* weights4, float* merged, float* member_scores, uint8_t* kept, int64_t* n_kept_out,
                               void* stream);

/* The selection of the cascade alone, over two parallel device arrays of n rows (group_ids int64, score_f32): kept_u8 [n] = 1 for a kept row, 0
 * for a pruned one; kept_list_i32 [n]: the kept rows in ascending row order (the first n_kept entries are written); semantics as above.
 *   status: device int32 [4]:  [0] flags  [1] n_kept  [2] distinct queries  [3] rows of the largest query  ([2], [3]: over the rows without a flag)
 *   flags:  MMS_CASCADE_FLAG_NONFINITE  a non-finite score (NaN, +-inf)      MMS_CASCADE_FLAG_RESERVED_ID  a group id equal to MMS_RANK_RESERVED_ID
 *           MMS_CASCADE_FLAG_TOO_MANY   n > MMS_CASCADE_MAX_ROWS (nothing is ranked; [2] = [3] = 0)
 *   With a non-zero flag word every row is kept: kept_u8 all ones, kept_list = 0 .. n - 1, n_kept = n.
 *   workspace: device memory, 256-byte aligned, at least mms_cascade_workspace_bytes(n) bytes (no content expected, none preserved).
 * A row is kept iff fewer than `keep` rows of its query rank before it: no sort, no limit on the rows of a query or on keep (a query of more than
 * `keep` rows costs rows x min(rows, rank) comparisons, one wavefront per query; queries of at most `keep` rows cost none).
 * Only integer atomics whose result does not depend on arrival order: equal inputs give equal bytes on every run.
 * The call ONLY ENQUEUES on `stream` (three fills, nine kernels): no allocation, no synchronisation, no device -> host read.
 * Returns MMS_ERR_ARG (message in mms_global_error, nothing launched) for n < 0 or n >= 2^31, keep < 1, a NULL status, a NULL pointer with n > 0,
 * a workspace smaller than mms_cascade_workspace_bytes(n) or not 256-byte aligned.  n == 0 writes a zero status and returns 0.  Handle-free. */
#define MMS_CASCADE_MAX_ROWS (1 << 22)
#define MMS_CASCADE_FLAG_NONFINITE 1
#define MMS_CASCADE_FLAG_RESERVED_ID 2
#define MMS_CASCADE_FLAG_TOO_MANY 4
int64_t mms_cascade_workspace_bytes(int64_t n);   /* a multiple of 256; -1 for n < 0 or n >= 2^31 */
int mms_cascade_select(const int64_t* group_ids, const float* score_f32, int64_t n, int32_t keep, uint8_t* kept_u8, int32_t* kept_list_i32,
                       int32_t* status /* [4] */, void* workspace, int64_t workspace_bytes, void* stream);

/* Ensemble PLANS (opt-in): an ordered list of 1 .. MMS_PLAN_MAX_STAGES stages, each naming the members it computes and the rule that decides which
 * rows go on to the next stage.  mms_score_ensemble is the plan [(7, 0, 0)], mms_score_ensemble_cascade(keep) the plan [(LX, keep, 0), (ZK | LDS, 0, 0)],
 * and a member subset (e.g. without a member whose weight is zero) is a one-stage plan.
 *   Members.  MMS_MEMBER_ZK = members 0 and 1 together (one image-token stage), MMS_MEMBER_LDS = member 2, MMS_MEMBER_LX = member 3.
 *   Stage rules (all rejected with MMS_ERR_ARG before anything is launched): 1 <= n_stages <= MMS_PLAN_MAX_STAGES; every `members` a non-empty subset
 *     of 7; the stages pairwise disjoint (their union may be a strict subset of 7); reserved == 0; the last stage has keep == safe_k == 0; every other
 *     stage has exactly one of keep >= 1 / safe_k >= 1; a plan with a safe_k stage and a negative or non-finite weight; a NULL handle (all three are
 *     required even when a member is in no stage); a NULL group_ids unless the plan has one stage; a NULL reached with B > 0; B >= 2^31.
 *   Table.  T is fp32 [4][B] and starts as +0.0f.  A_0 = all rows.  Stage s computes its members on the rows A_s and writes them into T.
 *   Bounds.  L = ((w0 * T0 + w1 * T1) + w2 * T2) + w3 * T3, every product and sum rounded to fp32 on its own (the merge of mms_score_ensemble).  U = the
 *     same expression with the members of LATER stages set to 1.0f.  Members in no stage stay 0: they are never computed.
 *   Selection among the rows of A_s, per query (group_ids as for mms_score_ensemble_cascade):
 *     keep    the order of mms_cascade_select on L (L descending, original row index ascending, -0.0 == +0.0); the first min(keep, rows) go on.
 *     safe_k  row i is pruned iff at least safe_k OTHER rows j of A_s in its query have L_j > U_i (strict, on the fp32 values): mms_cascade_select_safe.
 *     A flag at any selection -- a non-finite bound, the reserved id, more than MMS_CASCADE_MAX_ROWS rows -- sends every row of A_s on.
 *   Output.  member_scores (optional, [4,B]) = T; merged = L of the final T; reached[i] (device uint8 [B]) = the number of stages row i went through
 *     (1 .. n_stages); n_scored_out[s] (host, optional, [n_stages]) = |A_s|.
 *   BIT-EQUALITY RULE.  Stage 0 computes its members on b itself.  Stage s > 0 runs on the eleven feed arrays gathered from the ORIGINAL batch through the
 *     ascending list of A_s; its members are bit-equal to what mms_score_ensemble returns for that gathered batch as a call of its own.  Nothing of an
 *     earlier stage is reused.  A member of a subset is bit-equal to the same member of mms_score_ensemble on the same batch.
 *   GUARANTEES, for weights >= 0 and member scores in [0, 1] (fp32 rounding is monotone):
 *     L <= final merged <= U, whatever values in [0, 1] the members not yet computed take.
 *     A row pruned by a safe_k stage has at least safe_k rows of its query strictly above it in `merged`: no query's top safe_k of `merged` changes.
 *     A row kept by a keep stage has merged >= every row of its query pruned at that stage.
 *     These concern each query's top k of `merged`.  The uniqueness filter of the submission reads every row's score across queries and is NOT covered:
 *     ensemble.plan_curve measures what a plan changes there.
 *   Equivalences, bit for bit: [(7, 0, 0)] and mms_score_ensemble (merged, members); [(LX, keep, 0), (ZK | LDS, 0, 0)] and mms_score_ensemble_cascade
 *     (merged, members, kept = reached == 2, n_kept) -- for w3 > 0, and as long as L = w3 * x separates the lxmert scores x that the cascade's selection
 *     separates (two scores one ulp apart may round to one L; the tie then goes to the smaller row).
 *   Cost.  What each stage's mms_score_ensemble costs on its rows, ONE 16-byte device -> host read of the status word per non-last stage, and the copy of
 *     the feed arrays of the later stages' rows (none while every row has gone on: such a stage runs on b itself, which is the gathered batch).  The buffers live in the zk handle and grow on demand: a warmed-up handle does not allocate.  The
 *     caller's current device is restored on return. */
#define MMS_MEMBER_ZK 1
#define MMS_MEMBER_LDS 2
#define MMS_MEMBER_LX 4
#define MMS_PLAN_MAX_STAGES 3
typedef struct mms_plan_stage { int32_t members; int32_t keep; int32_t safe_k; int32_t reserved; } mms_plan_stage;
int mms_score_ensemble_plan(mms_handle* zk, mms_handle* lds, mms_handle* lxmert, const mms_ensemble_batch* b, const int64_t* group_ids,
                            const mms_plan_stage* stages, int32_t n_stages, const float* weights4, float* merged, float* member_scores /* optional [4,B] */,
                            uint8_t* reached /* [B] */, int64_t* n_scored_out /* host, optional [n_stages] */, void* stream);

/* The safe selection alone, over three parallel device arrays of n rows (group_ids int64, lower_f32, upper_f32): row i is PRUNED iff at least k OTHER
 * rows j of its group have lower[j] > upper[i] (strict, the fp32 values widened exactly to double, -0.0 == +0.0); every other row is kept.  A group of at
 * most k rows is kept whole.  kept_u8, kept_list_i32, status, the flags (a non-finite lower OR upper), the workspace rules, "only enqueues" (three fills,
 * nine kernels), determinism and the argument errors are those of mms_cascade_select, with mms_cascade_safe_workspace_bytes; additionally MMS_ERR_ARG
 * for k < 1.  lower[i] > upper[i] on a finite row is the caller's error and is not checked.  One wavefront per group, a lane per row, rows x min(rows,
 * until k are found) comparisons; no limit on the rows of a group or on k.  Handle-free. */
int64_t mms_cascade_safe_workspace_bytes(int64_t n);   /* a multiple of 256; -1 for n < 0 or n >= 2^31 */
int mms_cascade_select_safe(const int64_t* group_ids, const float* lower_f32, const float* upper_f32, int64_t n, int32_t k, uint8_t* kept_u8,
                            int32_t* kept_list_i32, int32_t* status /* [4] as mms_cascade_select */, void* workspace, int64_t workspace_bytes,
                            void* stream);

/* Per-query normalisation of the member scores BEFORE a merge (opt-in): every member is put on a common per-query scale, so that the weight and
 * filter grids of the fits mean the same whatever scale a checkpoint emits.  query_id: device int64 [n]; members: device fp32 [n_members, n],
 * member-major (the layout mms_score_ensemble writes); out: device fp32 [n_members, n], which must not overlap members.
 *   A GROUP is all rows with the same query id, in any order, not necessarily adjacent; each member is treated on its own, group by group.  With c
 *   the rows of the group and x_r = (double)members[m][r] + 0.0 (-0.0 folded onto +0.0), all arithmetic in IEEE double, every operation rounded on
 *   its own (no fused multiply-add), the result rounded once to fp32:
 *     MMS_NORMALIZE_MINMAX  (x - lo) / (hi - lo), lo / hi the group's minimum / maximum; +0.0 for every row when hi == lo
 *     MMS_NORMALIZE_ZSCORE  (x - mean) / sd;  mean = S1 / c, S1 the sum of x_r taken SEQUENTIALLY IN ASCENDING ROW INDEX from +0.0;
 *                           sd = sqrt(S2 / c), S2 the sum of (x_r - mean) * (x_r - mean) taken the same way; +0.0 for every row unless sd > 0
 *     MMS_NORMALIZE_RANK    (c - 1 - g) / (c - 1), g the rows of the group whose x is strictly greater (ties share a value); +0.0 when c == 1
 *     MMS_NORMALIZE_NONE    a copy
 *   ensemble.normalize_members is the same definition in numpy; the two agree bit for bit.
 *   status: device int32 [4]:  [0] distinct queries  [1] rows of the largest query  ([0], [1]: over the rows without a flag)  [2] flags  [3] 0
 *           (MMS_NORMALIZE_NONE checks nothing: a zero status)
 *   flags:  MMS_NORMALIZE_FLAG_NONFINITE (bit 1)  a non-finite score (NaN, +-inf) in any row of any member
 *           MMS_NORMALIZE_FLAG_RESERVED_ID (bit 3)  a query id equal to MMS_RANK_RESERVED_ID          (the bits of mms_rank_submission)
 *   WITH A NON-ZERO FLAG WORD THE CONTENT OF out IS UNSPECIFIED (the transform is skipped): detected, not served -- a caller answers from the host
 *   form (ensemble.normalize_members_device does).
 *   workspace: device memory, 256-byte aligned, at least mms_normalize_workspace_bytes(n, n_members) bytes (no content expected, none preserved).
 * No sort: rows are grouped through a query table and a counting scatter, each list is put into ascending row order by a counting walk, and the
 * thread of an output element walks its group's list: rows x rows-of-the-query steps per member, no limit on the rows of a query.
 * Only integer atomics whose result does not depend on arrival order: equal inputs give equal bytes on every run.
 * The call ONLY ENQUEUES on `stream` (three fills, seven kernels; MMS_NORMALIZE_NONE: one fill, one copy): no allocation, no synchronisation, no
 * device -> host read.  The caller's current device is restored on return.
 * Returns MMS_ERR_ARG (message in mms_global_error, nothing launched) for n < 0 or n > MMS_NORMALIZE_MAX_ROWS, n_members outside
 * [1, MMS_NORMALIZE_MAX_MEMBERS], a mode outside [0, 3], a NULL status, a NULL pointer with n > 0, out overlapping members, a workspace smaller than
 * mms_normalize_workspace_bytes(n, n_members) or not 256-byte aligned.  n == 0 writes a zero status and returns 0.  Handle-free. */
#define MMS_NORMALIZE_MAX_ROWS (1 << 22)
#define MMS_NORMALIZE_MAX_MEMBERS 8
#define MMS_NORMALIZE_NONE 0
#define MMS_NORMALIZE_MINMAX 1
#define MMS_NORMALIZE_ZSCORE 2
#define MMS_NORMALIZE_RANK 3
#define MMS_NORMALIZE_FLAG_NONFINITE 2
#define MMS_NORMALIZE_FLAG_RESERVED_ID 8
int64_t mms_normalize_workspace_bytes(int64_t n, int32_t n_members);   /* a multiple of 256; -1 for n or n_members out of range */
int mms_normalize_members(const int64_t* query_id, const float* members, int32_t n_members, int64_t n, int32_t mode, float* out,
                          int32_t* status /* [4] */, void* workspace, int64_t workspace_bytes, void* stream);

/* Box features of B records from their base64 text (the TSV's 6th field: f32 [num_boxes, 2048] row-major), decoded on the device --
 * the host gathers the text (libmmfeat mmf_gather_spans) instead of decoding it, and the H2D copy carries ~42 KB per record instead of 80 KB.
 *   record i's text starts at chars + char_off[i], a multiple of 16 bytes from `chars` (itself 16-byte aligned); rows[i] = min(num_boxes, 10)
 *   (clamped to [0, 10] here).  The first ceil(rows[i] x 8192 x 4 / 3) characters are read, decoded in loads of 16.
 *   Padding rule: the last load of record i covers characters char_off[i] .. char_off[i] + round_up(ceil(rows[i] x 8192 x 4 / 3), 16) - 1,
 *   so the buffer behind `chars` must extend to at least that byte for every record (mmf_gather_spans's dst_off layout: an exclusive prefix
 *   sum of the lengths rounded up to 16, plus the last record's rounded length).
 *   feats[i, :rows[i]] = the decoded floats and feats[i, rows[i]:10] = 0: bit for bit what libmmfeat's host decoder writes (NaN payloads included).
 *   bad[i] = 1 if one of the characters read is outside the base64 alphabet ('=' included) -- where libmmfeat rejects the record -- or if
 *   char_off[i] is negative or not a multiple of 16 (nothing is read; the row is zeroed); 0 otherwise.  Characters past the count above
 *   (the rest of the last load, the text of rows past the 10th) are ignored.  A malformed record sets bad[i] and writes nothing outside feats[i].
 *   chars, char_off, rows, feats [B,10,2048] fp32 and bad [B] int32 are device pointers; one kernel, asynchronous on `stream`.
 *   Returns MMS_ERR_ARG (message in mms_global_error, nothing launched) for B < 0, a NULL pointer with B > 0, or a misaligned chars / feats;
 *   B == 0 launches nothing and returns 0.  Handle-free: it needs no model. */
int mms_decode_feats_b64(const char* chars, const int64_t* char_off, const int32_t* rows, int64_t B, float* feats, int32_t* bad, void* stream);

/* The last step of the job on the device: the global product-uniqueness filter and the per-query top-5 of code/main.py:64-104 over the merged
 * scores, given as three parallel device arrays of n rows (query_id, product_id int64; score as fp32 OR fp64 -- exactly one of score_f32 /
 * score_f64 is non-NULL).  Rows of a query may come in any order, interleaved with other queries; the table's query order is the order of
 * first appearance.  Every comparison is made in IEEE double on the scores converted to double (-0.0 == +0.0):
 *   per product, over all rows: best, and second = the 2nd entry of its descending score list (two rows at the maximum: second == best);
 *   keep_product = (rows of the product < 2) or not (best - second < gap);   survive(row) = keep_product and |score - best| < tie;
 *   a query with >= 5 survivors gets its 5 best survivors; one with 1..4 survivors the 5 best of ALL its rows (fewer if it has fewer); one
 *   with none gets no output row.  Inside a row: score descending, equal scores in row order.  Output rows: first the queries with >= 5
 *   survivors, then those with 1..4, each class in first-appearance order (what ensemble.top5 / ensemble.submission_rows produce).
 * n <= MMS_RANK_MAX_ROWS; no limit on the rows of one query.  Neither id may be MMS_RANK_RESERVED_ID (the empty mark of the hash tables).
 *   workspace: device memory, 256-byte aligned, at least mms_rank_workspace_bytes(n) bytes (no content expected, none preserved).
 *   out_query [max_queries], out_products [max_queries][5] (unused entries -1), out_count [max_queries] (products written per row, 1..5).
 *   status: device int32 [4]:  [0] output rows written  [1] how many of them are of the >= 5-survivor class (they come first)
 *                              [2] flags  [3] distinct queries seen
 *   flags:  bit 0  a (query, product) pair occurs more than once (the table semantics "last score wins, first position stays" are NOT
 *                  implemented here: use the host form)         bit 1  a non-finite score (NaN, +-inf)
 *           bit 2  more output rows than max_queries            bit 3  an id equal to MMS_RANK_RESERVED_ID
 *   With a non-zero flag word out_* are unspecified, but nothing is written outside them or outside the workspace.
 * Only integer atomics whose result does not depend on arrival order: equal inputs give bit-equal outputs on every run.
 * The call ONLY ENQUEUES on `stream` (three fills, eight kernels): no allocation, no synchronisation, no device -> host read.
 * Returns MMS_ERR_ARG (message in mms_global_error, nothing launched) for n < 0 or n > MMS_RANK_MAX_ROWS, a NULL pointer with n > 0 (status: always),
 * both or neither score pointer, a workspace smaller than mms_rank_workspace_bytes(n) or not 256-byte aligned, max_queries < 0.
 * n == 0 writes a zero status and returns 0.  Handle-free: it needs no model. */
#define MMS_RANK_MAX_ROWS (1 << 22)
#define MMS_RANK_RESERVED_ID (-1LL)
int64_t mms_rank_workspace_bytes(int64_t n);   /* bytes of device workspace mms_rank_submission needs for n rows; a multiple of 256; -1 for n < 0 or n > MMS_RANK_MAX_ROWS */
int mms_rank_submission(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int64_t n,
                        double gap, double tie, void* workspace, int64_t workspace_bytes, int64_t max_queries,
                        int64_t* out_query /* [max_queries] */, int64_t* out_products /* [max_queries][5], unused entries -1 */,
                        int32_t* out_count /* [max_queries]: products written per row, 1..5 */, int32_t* status /* [4] */, void* stream);

/* The valid half of the job on the device: the relevance labels and the nDCG@k decisions of the reference's evaluation (code/imagebert_lds/src/
 * evaluation.py:4-38; ndcg.ndcg_from_arrays) against an answer key given in CSR form as three device arrays: key_query [n_key_queries] int64,
 * key_off [n_key_queries + 1] int64 with key_off[0] = 0 and key_off[n_key_queries] = n_key_products, key_product [n_key_products] int64 (key
 * query i's truth list is key_product[key_off[i] .. key_off[i + 1]); it may be empty, and a product that is repeated in it counts once).
 * The rows are three parallel device arrays of n entries (query_id, product_id int64; score as fp32 OR fp64 -- exactly one of score_f32 /
 * score_f64 is non-NULL); rows of a query may come in any order, interleaved with other queries.  Rows whose query is not in the key are
 * ignored; a (query, product) row that occurs twice counts each time.  No id may be MMS_RANK_RESERVED_ID.
 *   mms_key_relevance: labels_out[r] = 1 when row r's product is in the truth list of row r's query, else 0 (also for a query outside the
 *   key) -- the ground-truth label the reference feeds on valid (load_data_v4.py:259-263).
 *   mms_ndcg_at_k, per key query i: its rows ranked by score descending, equal scores in row order (compared in IEEE double on the scores
 *   converted to double, -0.0 == +0.0: Python's stable sorted(..., reverse=True));
 *     mask = bit j set when the j-th ranked row is relevant (j < k);   ideal = min(distinct products of the truth list, k);
 *     out_code[i] = mask | ideal << 8, or -1 for a key query without rows;   out_topk[i][j] (optional) = the j-th ranked product, -1 past the
 *     query's rows;   hist[ideal << k | mask] += 1 over the key queries that have rows -- (k + 1) << k int64 bins, zeroed by the call.
 *   The metric is host arithmetic on these integers: the per-query nDCG is a function of the code alone, ndcg.ndcg_from_codes sums it in key
 *   order like the host form (bit-identical to it), ndcg.ndcg_from_hist sums bin count x value -- the histogram path differs from the
 *   sequential sum by summation order only.  Histograms of disjoint query shards add up to the whole table's, exactly.
 *   allow_missing != 0: key queries without rows are skipped (code -1, no histogram entry) -- what a rank's shard of the rows needs.
 *   workspace: device memory, 256-byte aligned, at least mms_ndcg_workspace_bytes(n, n_key_queries, n_key_products) bytes (no content
 *   expected, none preserved).  k in 1..MMS_NDCG_MAX_K.
 *   status: device int32 [4]:  [0] key queries evaluated (those with rows)   [1] rows that belong to a key query
 *                              [2] flags                                     [3] key queries without rows
 *   flags:  bit 0  a key query has no rows while allow_missing == 0 (the host form raises KeyError there; mms_key_relevance never sets it)
 *           bit 1  a non-finite score (NaN, +-inf)        bit 2  a key query occurs more than once in key_query
 *           bit 3  an id (row or key) equal to MMS_RANK_RESERVED_ID
 *   With a non-zero flag word the outputs are unspecified, but nothing is written outside them or outside the workspace.
 * Only integer atomics whose result does not depend on arrival order: equal inputs give bit-equal outputs on every run.  No kernel waits
 * on another workgroup.  Both calls ONLY ENQUEUE on `stream` (fills and five / eight kernels): no allocation, no synchronisation, no
 * device -> host read.  Both are handle-free: they need no model.
 * Return MMS_ERR_ARG (message in mms_global_error naming the function, nothing launched) for a negative count or one over its cap
 * (n, n_key_products <= MMS_NDCG_MAX_ROWS, n_key_queries <= MMS_NDCG_MAX_KEY_QUERIES), k outside 1..MMS_NDCG_MAX_K, a NULL pointer whose count is
 * non-zero (status and hist: always; out_topk may be NULL), key products without key queries, both or neither score pointer, a workspace that is
 * too small or not 256-byte aligned (needed when n_key_queries > 0).
 * n == 0 writes a zero histogram, status [0, 0, flags, n_key_queries] (bit 0 unless allow_missing) and every code -1; n_key_queries == 0 writes a
 * zero histogram and status (and zero labels). */
#define MMS_NDCG_MAX_ROWS (1 << 22)          /* also the cap on n_key_products */
#define MMS_NDCG_MAX_KEY_QUERIES (1 << 20)
#define MMS_NDCG_MAX_K 8
int64_t mms_ndcg_workspace_bytes(int64_t n, int64_t n_key_queries, int64_t n_key_products);   /* a multiple of 256; -1 outside the caps */
int mms_key_relevance(const int64_t* query_id, const int64_t* product_id, int64_t n, const int64_t* key_query, const int64_t* key_off,
                      const int64_t* key_product, int64_t n_key_queries, int64_t n_key_products, void* workspace, int64_t workspace_bytes,
                      int64_t* labels_out /* [n] 0 / 1 */, int32_t* status /* [4] */, void* stream);
int mms_ndcg_at_k(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int64_t n,
                  const int64_t* key_query, const int64_t* key_off, const int64_t* key_product, int64_t n_key_queries, int64_t n_key_products,
                  int32_t k, int32_t allow_missing, void* workspace, int64_t workspace_bytes, int32_t* out_code /* [n_key_queries] */,
                  int64_t* out_topk /* [n_key_queries][k] or NULL */, int64_t* hist /* [(k + 1) << k] */, int32_t* status /* [4] */, void* stream);

/* Fitting the ensemble weights on the valid set: the nDCG@k histogram -- and, optionally, the value -- of EVERY weight vector of a grid in one
 * call, over the member scores mms_score_ensemble leaves on the device.  Rows, answer key, k, allow_missing, status words and flag bits are
 * those of mms_ndcg_at_k; the score is replaced by n_members member scores, member-major in fp32 (members[m * n + r]: the member_scores layout
 * of mms_score_ensemble), and n_weights weight vectors (weights[v * n_members + m], device fp64).
 *   ARITHMETIC CONTRACT.  For weight vector v and row r
 *       score_v[r] = (...((w[v][0] * s0) + w[v][1] * s1) + ...) + w[v][n_members - 1] * s_{n_members - 1}
 *   in IEEE double: the members widened exactly, every product and every sum rounded on its own, left to right -- Python's evaluation of
 *   code/main.py:59, numpy's when written as separate ufunc calls; never a fused multiply-add.  hist_out[v] is by definition the histogram
 *   mms_ndcg_at_k yields for score_f64 = score_v: rows ranked by (image descending, row ascending) with -0.0 == +0.0, code = mask | ideal << 8,
 *   hist_out[v][ideal << k | mask] += 1 over the key queries that have rows ((k + 1) << k int64 bins per vector, zeroed by the call).
 *       value_out[v] = (sum over ALL bins b in bin order of double(hist_out[v][b]) * bin_value[b]) / n_key_queries_total
 *   each product, each sum and the division rounded on its own.  bin_value is the caller's table of the per-code nDCG (ndcg._code_value: the
 *   metric's arithmetic stays in one place), so value_out[v] is ndcg.ndcg_from_hist(hist_out[v], k, n_key_queries_total) bit for bit (an empty
 *   bin adds +0.0 to a non-negative sum).  value_out may be NULL; given, it needs bin_value and n_key_queries_total >= 1.
 *   A non-finite score_v[r] of a row that belongs to a key query sets flag bit 1 (a row outside the key is never read).  With a weight of 0 a
 *   member of +-inf gives NaN, as in Python.
 *   The value at w = (0.2, 0.2, 0.3, 0.3) is the DOUBLE merge of main.py; the merged output of mms_score_ensemble is the fp32 merge, whose
 *   ranking can differ on a near tie.
 *   workspace: device memory, 256-byte aligned, at least mms_ndcg_sweep_workspace_bytes(n, n_key_queries, n_key_products, n_members) bytes.
 * The score-independent stages of mms_ndcg_at_k (key tables, relevance of every row, scan, scatter) run once per call; then a wavefront takes a
 * key query and a tile of 64 weight vectors, a lane owning one vector (csrc/ndcg_sweep.hip).  Integer atomics only: equal inputs give bit-equal
 * outputs.  ONLY ENQUEUES on `stream` (fills and at most ten kernels): no allocation, no synchronisation, no device -> host read.  Handle-free.
 * Returns MMS_ERR_ARG (message in mms_global_error, nothing launched) for a count that is negative or over its cap (those of mms_ndcg_at_k;
 * n_members in 1..MMS_SWEEP_MAX_MEMBERS, n_weights <= MMS_SWEEP_MAX_WEIGHTS), k outside 1..MMS_NDCG_MAX_K, a NULL pointer whose count is non-zero
 * (status: always), value_out without bin_value, a workspace that is too small or not 256-byte aligned (needed when n_key_queries > 0).
 * n == 0, n_key_queries == 0: zero histograms, status as mms_ndcg_at_k (values 0); n_weights == 0: the status alone. */
#define MMS_SWEEP_MAX_MEMBERS 8
#define MMS_SWEEP_MAX_WEIGHTS (1 << 20)
int64_t mms_ndcg_sweep_workspace_bytes(int64_t n, int64_t n_key_queries, int64_t n_key_products, int32_t n_members);   /* a multiple of 256; -1 outside the caps */
int mms_ndcg_weight_sweep(const int64_t* query_id, const int64_t* product_id, const float* members /* [n_members][n] */, int32_t n_members, int64_t n,
                          const int64_t* key_query, const int64_t* key_off, const int64_t* key_product, int64_t n_key_queries, int64_t n_key_products,
                          const double* weights /* device [n_weights][n_members] */, int64_t n_weights, int32_t k, int32_t allow_missing,
                          const double* bin_value /* device [(k+1)<<k] or NULL */, int64_t n_key_queries_total /* divisor of value_out */,
                          void* workspace, int64_t workspace_bytes, int64_t* hist_out /* [n_weights][(k+1)<<k], zeroed by the call */,
                          double* value_out /* [n_weights] or NULL; needs bin_value */, int32_t* status /* [4] as mms_ndcg_at_k */, void* stream);

/* Fitting the uniqueness filter on the valid set: the nDCG@k histogram -- and, optionally, the value and the per-query codes -- of the SUBMISSION
 * rows (what mms_rank_submission writes: code/main.py:76-104) for EVERY (gap, tie) pair of a grid in one call.  Rows, answer key, allow_missing and
 * status words are those of mms_ndcg_at_k; the score is given as fp32 OR fp64 (exactly one of score_f32 / score_f64 is non-NULL); filters is a
 * device fp64 array [n_filters][2] with rows (gap, tie).  k in 1..MMS_FILTER_MAX_K: a submission row holds five products.
 *   ARITHMETIC CONTRACT, decision for decision that of mms_rank_submission and of ensemble.submission_rows, in IEEE double on the scores widened
 *   exactly, -0.0 == +0.0:
 *     per product, over ALL rows -- also rows of queries outside the key:  d = best - second, second = best when two rows share the maximum;
 *     keep_product = (rows of the product < 2) or not (d < gap);   survive(row) = keep_product and |score - best| < tie;
 *     per key query: >= 5 survivors -> its best survivors; 1..4 survivors -> its best rows overall; order: score descending, then row ascending.
 *   A NaN or +-inf gap / tie is no error: the two comparisons decide as they do in Python ((-inf, +inf) keeps every product and every row, so the
 *   output row is the unfiltered top-5 and the histogram is that of mms_ndcg_at_k).
 *   code_out[g][i] (optional), for filter g and key query i:  -1 when the query has no rows;  -2 when it has rows but no survivor (main.py writes
 *   no row for it; it scores 0);  otherwise mask | ideal << 8 with bit j of mask set when the j-th product of its output row is in its truth list
 *   (j < min(k, products written)) and ideal = min(distinct products of the truth list, k).  hist_out[g][ideal << k | mask] += 1 over the codes >= 0
 *   ((k + 1) << k int64 bins per filter, zeroed by the call) -- ndcg.submission_codes / ndcg.filter_sweep_host on the host.
 *       value_out[g] = (sum over ALL bins b in bin order of double(hist_out[g][b]) * bin_value[b]) / n_key_queries_total
 *   each product, each sum and the division rounded on its own, as in mms_ndcg_weight_sweep: ndcg.ndcg_from_hist(hist_out[g], k,
 *   n_key_queries_total) bit for bit.  The divisor is the caller's (the whole key's length): a dropped or missing query costs its share, as a
 *   grader of the submission file charges it.  value_out may be NULL; given, it needs bin_value and n_key_queries_total >= 1.
 *   The filter is global over the rows: histograms of query shards do NOT add up to the whole table's (a product's second best may sit in another
 *   shard).  Run the call on the gathered table.
 *   flags (status[2]):  bits 0-3 as mms_ndcg_at_k, but bit 1 covers a non-finite score in ANY row (the product statistics read every row);
 *           bit 4  a (query, product) pair occurs more than once (the table semantics "last score wins" stay with the host form, as in
 *                  mms_rank_submission)
 *   With a non-zero flag word (other than bit 0 under allow_missing, which is never set then) the outputs are unspecified, but nothing is written
 *   outside them or outside the workspace.
 *   workspace: device memory, 256-byte aligned, at least mms_filter_sweep_workspace_bytes(n, n_key_queries, n_key_products) bytes.
 * Everything but the two comparisons against (gap, tie) runs once per call: the score-independent stages of mms_ndcg_at_k, the product statistics
 * of mms_rank_submission, the records (score image, row, relevance, d, |score - best|) and the unfiltered top-k; then a wavefront takes a key query
 * and a tile of 64 filters, a lane owning one filter (csrc/filter_sweep.hip).  Integer atomics only: equal inputs give bit-equal outputs.  No kernel
 * waits on another workgroup.  ONLY ENQUEUES on `stream` (fills and at most fifteen kernels): no allocation, no synchronisation, no device -> host
 * read.  Handle-free.
 * Returns MMS_ERR_ARG (message in mms_global_error naming the function, nothing launched) for a count that is negative or over its cap (those of
 * mms_ndcg_at_k; n_filters <= MMS_FILTER_MAX), k outside 1..MMS_FILTER_MAX_K, a NULL pointer whose count is non-zero (status: always; filters and
 * hist_out with n_filters > 0; code_out may be NULL), key products without key queries, both or neither score pointer, value_out without bin_value
 * or with n_key_queries_total < 1, a workspace that is too small or not 256-byte aligned (needed when n_key_queries > 0).
 * n == 0: zero histograms, every code -1, status as mms_ndcg_at_k (values 0); n_key_queries == 0: zero histograms and status; n_filters == 0: the
 * status alone. */
#define MMS_FILTER_MAX (1 << 16)
#define MMS_FILTER_MAX_K 5
int64_t mms_filter_sweep_workspace_bytes(int64_t n, int64_t n_key_queries, int64_t n_key_products);   /* a multiple of 256; -1 outside the caps */
int mms_filter_sweep(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int64_t n,
                     const int64_t* key_query, const int64_t* key_off, const int64_t* key_product, int64_t n_key_queries, int64_t n_key_products,
                     const double* filters /* device [n_filters][2] = (gap, tie) */, int64_t n_filters, int32_t k /* 1..5 */, int32_t allow_missing,
                     const double* bin_value /* device [(k+1)<<k] or NULL */, int64_t n_key_queries_total /* divisor of value_out */,
                     void* workspace, int64_t workspace_bytes, int64_t* hist_out /* [n_filters][(k+1)<<k], zeroed by the call */,
                     double* value_out /* [n_filters] or NULL; needs bin_value */, int32_t* code_out /* [n_filters][n_key_queries] or NULL */,
                     int32_t* status /* [4] as mms_ndcg_at_k */, void* stream);

/* Fitting the ensemble weights and the uniqueness filter JOINTLY on the valid set: the nDCG@k histogram -- and, optionally, the value -- of the
 * SUBMISSION rows for EVERY (weight vector, filter) pair of two grids in one call.  Rows, answer key, allow_missing and status words are those of
 * mms_ndcg_at_k; members / n_members / weights are those of mms_ndcg_weight_sweep, filters / k those of mms_filter_sweep.
 *   ARITHMETIC CONTRACT: none of its own.  It composes the two existing contracts: item (v, g) -- hist_out[v][g], value_out[v][g] -- is by
 *   definition what mms_filter_sweep yields for filter g on score_f64 = score_v, the merge of mms_ndcg_weight_sweep for weight vector v (IEEE
 *   double, members widened exactly, every product and every sum rounded on its own, left to right, never a fused multiply-add).  So d, keep,
 *   survive, the >= 5 / 1..4 / 0 survivor cases, the order (score descending, then row ascending), -0.0 == +0.0, NaN / +-inf filters and the
 *   divisor n_key_queries_total are mms_filter_sweep's, unchanged: ndcg.joint_sweep_host on the host.  The product statistics (best, second) depend
 *   on the weights and are formed per weight vector.
 *   flags (status[2]): those of mms_filter_sweep.  Bit 1: a non-finite merged score in ANY row for ANY weight vector (or a non-finite first
 *   member); bit 4: a repeated (query, product) pair.  With a non-zero flag word (other than bit 0 under allow_missing, never set then) the
 *   outputs are unspecified, but nothing is written outside them or outside the workspace.
 *   hist_out may be NULL: only values are written, and the histograms of the vectors in flight live in the workspace (the full array is
 *   n_weights * n_filters * ((k + 1) << k) * 8 bytes: about 280 MB at 1 771 x 102, k = 5).  value_out may be NULL; given, it needs bin_value and
 *   n_key_queries_total >= 1.
 *   workspace: device memory, 256-byte aligned.  The weight vectors are processed in tiles of 64, and the tiles in CHUNKS, because the per-vector
 *   product statistics take 16 B x 64 x n per tile: mms_joint_sweep_workspace_bytes(n, n_key_queries, n_key_products, n_members, tiles_per_chunk)
 *   is the size for chunks of tiles_per_chunk tiles WITH hist_out; without hist_out add tiles_per_chunk * 64 * n_filters * ((k + 1) << k) * 8
 *   bytes, rounded up to a multiple of 256 per tile.  The call derives its chunk from workspace_bytes -- as many tiles as fit, one at least -- and
 *   the results do not depend on it.
 * Once per call: the score-independent stages of mms_ndcg_at_k, the product table of mms_rank_submission, the rows grouped by product and by key
 * query.  Per chunk: the product statistics per weight vector, the unfiltered top-k per (key query, vector), then a wavefront takes a tile of 64
 * weight vectors, ONE filter and a slab of key queries, a lane owning one vector (csrc/joint_sweep.hip).  Integer atomics only: equal inputs give
 * bit-equal outputs.  No kernel waits on another workgroup.  ONLY ENQUEUES on `stream` (fills and kernels): no allocation, no synchronisation, no
 * device -> host read.  Handle-free.
 * Returns MMS_ERR_ARG (message in mms_global_error naming the function, nothing launched) for a count that is negative or over its cap (those of
 * mms_ndcg_at_k; n_members in 1..MMS_SWEEP_MAX_MEMBERS, n_filters <= MMS_FILTER_MAX, n_weights and n_weights * n_filters <= MMS_JOINT_MAX_ITEMS), k
 * outside 1..MMS_FILTER_MAX_K, a NULL pointer whose count is non-zero (status: always; hist_out and value_out may be NULL), key products without
 * key queries, value_out without bin_value or with n_key_queries_total < 1, a workspace that is not 256-byte aligned or too small for a chunk of
 * ONE tile (needed when n_key_queries > 0; with n_weights == 0 or n_filters == 0 the part that does not grow with tiles_per_chunk is enough).
 * n == 0, n_key_queries == 0: zero histograms and values, status as mms_filter_sweep; n_weights == 0 or n_filters == 0: the status alone. */
#define MMS_JOINT_MAX_ITEMS (1 << 22)
int64_t mms_joint_sweep_workspace_bytes(int64_t n, int64_t n_key_queries, int64_t n_key_products, int32_t n_members,
                                        int64_t tiles_per_chunk /* >= 1 */);   /* a multiple of 256, monotone in tiles_per_chunk; -1 outside the caps */
int mms_joint_sweep(const int64_t* query_id, const int64_t* product_id, const float* members /* [n_members][n] */, int32_t n_members, int64_t n,
                    const int64_t* key_query, const int64_t* key_off, const int64_t* key_product, int64_t n_key_queries, int64_t n_key_products,
                    const double* weights /* device [n_weights][n_members] */, int64_t n_weights,
                    const double* filters /* device [n_filters][2] = (gap, tie) */, int64_t n_filters, int32_t k /* 1..5 */, int32_t allow_missing,
                    const double* bin_value /* device [(k+1)<<k] or NULL */, int64_t n_key_queries_total /* divisor of value_out */,
                    void* workspace, int64_t workspace_bytes, int64_t* hist_out /* [n_weights][n_filters][(k+1)<<k] or NULL; zeroed by the call */,
                    double* value_out /* [n_weights][n_filters] or NULL; needs bin_value */, int32_t* status /* [4] as mms_ndcg_at_k */, void* stream);

/* mms_joint_sweep that KEEPS the per-query codes: the same call -- launch sequence, histograms, values, status and workspace sizes, bit for bit and
 * whatever the chunk -- plus code_out, one byte per (filter g, key query i, weight vector v):
 *       code_out[(g * n_key_queries + i) * Wp + v],   Wp = 64 * ceil(n_weights / 64)
 *   ideal << 5 | mask   a graded query: the int32 code mask | ideal << 8 of mms_filter_sweep's code_out (k <= 5: mask < 32, ideal <= 5)
 *   0xFF                a key query without table rows (code -1)
 *   0xFE                a key query with rows but no output row (code -2)
 * The 64 lanes of a wavefront own 64 consecutive vectors, so the store is one aligned 64-byte line per (filter, key query, tile).  The call fills
 * the matrix with 0xFF first; bytes with v >= n_weights are unspecified and never read.  ndcg.joint_codes_host on the host.
 * code_bytes must equal n_filters * n_key_queries * Wp (0 with code_out == NULL, which makes the call mms_joint_sweep): MMS_ERR_ARG otherwise, nothing
 * launched.  The other arguments, errors and empty cases are mms_joint_sweep's. */
int mms_joint_sweep_codes(const int64_t* query_id, const int64_t* product_id, const float* members /* [n_members][n] */, int32_t n_members, int64_t n,
                          const int64_t* key_query, const int64_t* key_off, const int64_t* key_product, int64_t n_key_queries, int64_t n_key_products,
                          const double* weights /* device [n_weights][n_members] */, int64_t n_weights,
                          const double* filters /* device [n_filters][2] = (gap, tie) */, int64_t n_filters, int32_t k /* 1..5 */, int32_t allow_missing,
                          const double* bin_value /* device [(k+1)<<k] or NULL */, int64_t n_key_queries_total /* divisor of value_out */,
                          void* workspace, int64_t workspace_bytes, int64_t* hist_out /* [n_weights][n_filters][(k+1)<<k] or NULL; zeroed by the call */,
                          double* value_out /* [n_weights][n_filters] or NULL; needs bin_value */,
                          uint8_t* code_out /* [n_filters][n_key_queries][Wp] or NULL */, int64_t code_bytes, int32_t* status /* [4] as mms_ndcg_at_k */,
                          void* stream);

/* Resampling the joint fit: k-fold, repeated k-fold and bootstrap estimates of the HELD-OUT nDCG@k from the codes of ONE sweep.  The filter's product
 * statistics are taken over all rows of the table whatever the key, so the code of key query i under item (v, g) does not depend on which other key
 * queries are graded: a replicate is a row of small integer counts over the key queries, its value a count-weighted mean over the item's codes.
 *   code        device, the matrix of mms_joint_sweep_codes for n_weights x n_filters items and n_key_queries key queries; code_bytes as there
 *   count_fit / count_eval   device uint8 [n_replicates][n_key_queries]: how often key query i counts in the fit / in the evaluation of replicate r
 *   byte_value  device fp64 [256]: the value of a key query per code byte (ndcg.byte_values(k): ndcg._code_value of the byte's code; 0.0 for 0xFF, 0xFE
 *               and the bytes that cannot occur at this k).  PRECONDITION: finite and >= 0
 *   probe_item  device int64 [n_probes] (optional): items v * n_filters + g whose values are reported per replicate whoever wins
 *   ARITHMETIC CONTRACT, IEEE double, never a fused multiply-add:
 *       fit[r][item] = (sum over i = 0 .. n_key_queries - 1 of double(count_fit[r][i]) * byte_value[code[item][i]]) / double(sum over i of count_fit[r][i])
 *   the sum in key order from +0.0, every product, every sum and the division rounded on its own (a term with count 0 adds +0.0 to a sum that is never
 *   negative: the same bits as leaving it out; the divisor is the integer sum, converted once).  With all counts 1 this is ndcg.ndcg_from_codes of the
 *   item's codes term for term -- the sum evaluate_ndcg makes.  ndcg.resample_select_host on the host.
 *   best[r]        the SMALLEST item v * n_filters + g that attains the maximum of fit[r][.]: the first-at-maximum rule of ensemble.fit_joint
 *   fit_value[r]   that maximum;   eval_value[r]  the same sum with count_eval[r] on item best[r] (a zero count sum: NaN, from 0.0 / 0.0)
 *   probe_fit[r][p] / probe_eval[r][p]   the two sums on item probe_item[p] (an item outside [0, n_weights * n_filters): NaN, nothing is read)
 *   flags (status[2]): bit 5 (MMS_FLAG_EMPTY_FIT) is OR-ed in when count_fit of some replicate sums to zero: best[r] = -1, fit_value[r] and
 *   eval_value[r] NaN for that replicate.  Nothing else of status is written, so the status block of the sweep can be passed on and one read carries
 *   every flag; a caller without a sweep zeroes it.
 *   workspace: device memory, 256-byte aligned, mms_resample_workspace_bytes(n_weights, n_filters, n_key_queries, n_replicates) bytes.
 * The [n_replicates][items] value matrix is never stored: a lane owns an item and walks its codes in key order with the counts of 16 replicates in
 * scalar registers, a workgroup reduces its items to one (value, item) per replicate, and a second kernel picks per replicate by the total order
 * (value descending, item ascending) and walks the winner's and the probes' codes (csrc/resample.hip).  No floating-point atomics: equal inputs give
 * bit-equal outputs.  No kernel waits on another workgroup.  ONLY ENQUEUES on `stream` (four kernels): no allocation, no synchronisation, no
 * device -> host read.  Handle-free.
 * Returns MMS_ERR_ARG (message in mms_global_error naming the function, nothing launched) for a count that is negative or over its cap (n_weights and
 * n_weights * n_filters <= MMS_JOINT_MAX_ITEMS, n_filters <= MMS_FILTER_MAX, n_key_queries <= MMS_NDCG_MAX_KEY_QUERIES, n_replicates <=
 * MMS_RESAMPLE_MAX_REPLICATES, n_probes <= MMS_RESAMPLE_MAX_PROBES), a code_bytes other than n_filters * n_key_queries * Wp, a NULL pointer whose
 * count is non-zero (status: always), a workspace that is too small or not 256-byte aligned.  n_replicates == 0: nothing is written. */
#define MMS_RESAMPLE_MAX_REPLICATES (1 << 16)
#define MMS_RESAMPLE_MAX_PROBES 256
#define MMS_FLAG_EMPTY_FIT 32
int64_t mms_resample_workspace_bytes(int64_t n_weights, int64_t n_filters, int64_t n_key_queries, int64_t n_replicates);   /* a multiple of 256; -1 outside the caps */
int mms_resample_select(const uint8_t* code, int64_t code_bytes, int64_t n_weights, int64_t n_filters, int64_t n_key_queries,
                        const uint8_t* count_fit, const uint8_t* count_eval /* device [n_replicates][n_key_queries] */, int64_t n_replicates,
                        const double* byte_value /* device [256] */, const int64_t* probe_item /* device [n_probes] or NULL */, int64_t n_probes,
                        void* workspace, int64_t workspace_bytes, int64_t* best /* [n_replicates] */, double* fit_value, double* eval_value /* [n_replicates] */,
                        double* probe_fit, double* probe_eval /* [n_replicates][n_probes] */, int32_t* status /* [4]; [2] |= flags */, void* stream);

/* accumulated hipEvent time (ms) and launch count of the GEMM kernels since the last reset;
 * enable = 1 brackets every GEMM launch with events on its stream (bench / roofline only) */
int mms_gemm_timing(mms_handle* h, int32_t enable, int32_t reset, double* ms_out, int64_t* launches_out, double* flops_out);
/* the same, for one class of the timed GEMM launches: cls 0 = plain epilogue, 1 = fused bias + residual + LayerNorm epilogue
 * (mms_config.fuse_layernorm; their duration includes the residual stages and the LayerNorm work, their FLOP count the projection alone) */
int mms_gemm_timing_class(mms_handle* h, int32_t cls, double* ms_out, int64_t* launches_out, double* flops_out);
/* The fused QKV + attention launches (mms_config.fuse_attention) of the calls timed through mms_gemm_timing (enabled / reset there),
 * reported apart from the GEMM launches because their duration includes the attention of their pairs: total ms, launches, executed
 * projection FLOPs. */
int mms_fused_timing(mms_handle* h, double* ms_out, int64_t* launches_out, double* flops_out);
/* ... and the executed FLOPs of the launches that ran on a side lane (lxmert's distinct-query stage): counted, not timed -- a launch that shares the chip has no duration of its own */
int mms_side_lane_flops(mms_handle* h, double* flops_out);

/* ---- debug / test hooks: NOT part of the product ABI --------------------------------------------------------------------------------
 * The kernel-level parity tests and tools/ call the same kernels the scorers launch through these; they are built into libmmscore.so (the
 * tests must exercise the shipped binary) but may change with any revision and take no part in MMS_ABI_VERSION.  A host that scores pairs
 * does not define MMS_TEST_HOOKS and does not see them. */
#ifdef MMS_TEST_HOOKS
int mms_debug_read_x(mms_handle* h, float* dst_dev, int64_t rows, void* stream); /* current hidden state -> fp32 [rows,768] */
int mms_dbg_gemm(const float* a_f32, int64_t M, int64_t K, int64_t lda, const float* w_f32_nk, int64_t N,
                 const float* bias, const float* resid_f32, int32_t act, int32_t nsplit, int32_t out_planes,
                 int32_t engine /* enum Engine of csrc/regimes.h, per CALL, no global state:
 * GENERATED ENGINES BEGIN (tools/gen_regime_doc.py from csrc/regimes.h -- do not edit)
 *     0 ENG_AUTO          the per-shape choice of a forward (gemm_dispatch.hip pick_engine)
 *     1 ENG_TILE_128      gemm_tile.hip: register-staged 128 x 128 tile (the only tile for N % 256 != 0, and the three-pass tile of precision mode 3)
 *     3 ENG_TILE_DMA      gemm_tile.hip: 128 x 256 tile, LDS-DMA double buffered, one workgroup per CU (launches of no more workgroups than CUs)
 *     4 ENG_TILE          gemm_tile.hip: register-staged 128 x 256 tile, the default below PP_ROWS
 *     5 ENG_SKINNY        gemm_skinny.hip: <= 128 rows, one workgroup per 16 output columns, K sliced over its waves (GemmParams::wave_k_slices)
 *    16 ENG_TILE_256      gemm_tile.hip: 256 x 256 / 16 waves (kept for the kernel tests; no forward selects it since round 4)
 *    20 ENG_PP            gemm_pp.hip: 256 x 256 ping-pong phases, one tile per workgroup
 *    26 ENG_PP_PERSIST    gemm_pp.hip: the same, persistent workgroups (XCD-aware tile walk): launches of >= PP_ROWS rows
 *    27 ENG_PPW           gemm_ppw.hip: 256 x 128 three-pass ping-pong (precision mode 3, >= PP_ROWS rows)
 *    28 ENG_DW            lab build: gemm_dw.hip (128 x 256, two 4-wave workgroups per CU) -- measured and shelved
 *    54 ENG_SKINNY_K4     kernel tests: the skinny kernel with 4 wave-level K slices
 *    55 ENG_SKINNY_PARTS  gemm_skinny.hip with the K slices dealt to single-wave WORKGROUPS: GemmParams::k_splits fp32 partials (the split-K contract
 *                         of the tiles)
 *    58 ENG_SKINNY_K8     kernel tests: 8 wave-level K slices
 * GENERATED ENGINES END
 */,
                 float* c_f32, void* stream);
/* fp8 GEMM (precision 4, MX-scaled fp8 MFMA) on fp32 operands: A and W are quantised exactly as the forward does it (A: e4m3 RNE of the
 * value; W: per output channel the smallest POWER OF TWO scale with max|w| / scale <= 448, e4m3 RNE of w / scale; the scale is applied
 * by the MFMA instruction itself as the weight operand's e8m0 hardware scale).  N % 256 == 0, K % 128 == 0 */
/* The output addressing of a launch, opened up for the kernel tests (tests/test_gemm_addressing_gpu.py; the numpy statement of these fields is
 * tests/helpers.py gemm_rows_ref).  A row map {grp, stride, off} sends logical row r to physical row (r / grp) * stride + off + r % grp; grp == 0 is the
 * identity.  mms_dbg_gemm_rows reads every field; the hooks that take an OPTIONAL mms_rows_spec name the fields they read. */
typedef struct mms_rows_spec {
    int32_t M, N, K;
    int32_t nsplit;        /* 1, 2, 3: the precision modes of mms_dbg_gemm */
    int32_t engine;        /* ONE named engine (enum Engine), launched through its own launcher: a shape or field set it refuses is MMS_ERR_ARG, no fall-back */
    int32_t act, reverse;
    int32_t m_live;        /* >= 0: the device-side live-row count (rows >= min(M, m_live) are not written); -1: none */
    int32_t a_rows, lda;   /* A: fp32 [a_rows][lda], lda >= K, lda % 32 == 0 */
    int32_t amap[3];       /* logical row -> A row (ignored when a_index is given) */
    int32_t r_rows;        /* residual: fp32 [r_rows][N] */
    int32_t rmap[3];       /* logical row -> residual row (ignored when r_index is given) */
    int32_t out_kind;      /* 0: fp32 [c_rows][ldo], ldo >= N, ldo % 4 == 0;  1: split planes [c_rows][ldo], ldo >= N, ldo % 32 == 0, passed and returned as
                            * their fp32 image;  2: head-major fp32 [hm_blocks][hm_rows][64]: columns [64 g, 64 g + 64) of a row go to block hm_col0 / 64 + g */
    int32_t ldo, c_rows;
    int32_t cmap[3];       /* logical row -> output row (of c_rows, or of hm_rows for out_kind 2) */
    int32_t hm_rows, hm_col0, hm_blocks;     /* out_kind 2: hm_col0 % 64 == 0, (hm_col0 + N) / 64 <= hm_blocks */
} mms_rows_spec;
int mms_dbg_gemm_f8(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, int64_t N, const float* bias, int32_t act,
                    int32_t out_f8, float* c_f32, void* stream);
/* ... with `rows` (NULL = the dense call above): m_live, cmap, c_rows, ldo and -- with out_f8 == 0 -- out_kind 0 / 2 with hm_rows / hm_col0 / hm_blocks are
 * honoured; with out_f8 the e4m3 bytes are [c_rows][ldo], ldo % 32 == 0 (GemmParams::ldf8).  c_f32 is then the caller's PRE-FILLED physical image (for out_f8 it is
 * rounded to e4m3 bytes before the launch and the whole byte buffer is decoded back after it); every output row a logical row r < M can address is checked
 * against it on the host */
int mms_dbg_gemm_f8_rows(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, int64_t N, const float* bias, int32_t act,
                         int32_t out_f8, float* c_f32, const mms_rows_spec* rows, void* stream);
/* out = LayerNorm(A W^T + bias + resid) over N = 768 through the GEMM with the fused LayerNorm epilogue (gemm_pp_ln.h) and the
 * LayerNorm kernel queued behind it; *mode_out = 1 when the launch ran fused, 2 when it took the plain two-kernel route */
int mms_dbg_gemm_ln(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, const float* bias, const float* resid_f32,
                    const float* gamma, const float* beta, int32_t flags /* bit 0: fp8 operands (no such engine: MMS_ERR_ARG); bit 1: the row panels are walked from
 * the last one down, as every second big launch of a forward walks them (the ragged panel in the first persistent round) */, float* c_f32, int32_t* mode_out, void* stream);
/* the small-launch route of the same operation (calls of a few hundred pairs): register-staged tiles with the contraction split `splits`
 * ways into fp32 partials (K % (64 * splits) == 0; 1 = unsplit) + the LayerNorm kernel that sums them and adds bias + residual; splits < 0: |splits|
 * partials from the skinny kernel instead (K slices dealt to workgroups, M <= 512): bit-identical to the tile engine's */
int mms_dbg_proj_ln_splitk(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, const float* bias, const float* resid_f32,
                           const float* gamma, const float* beta, int32_t splits, float* c_f32, void* stream);
int mms_dbg_proj_ln_splitk_rows(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, const float* bias, const float* resid_f32,
                                const float* gamma, const float* beta, int32_t splits, float* c_f32,
                                const mms_rows_spec* rows /* optional: a_f32 is [a_rows][lda] read through amap / a_index (the split-K GEMM), resid_f32 [r_rows][768] read
 * through rmap / r_index (the LayerNorm that sums the partials); every row a logical row r < M can address is checked on the host */,
                                const int32_t* a_index, const int32_t* r_index, void* stream);
/* time one GEMM shape on random data (`what`: an engine as in mms_dbg_gemm, or 52: the MX-fp8 engine; 60 / 61: the LayerNorm kernel with / without
 * residual; 62 / 63: N = 768 projection + residual + LayerNorm as two kernels / as one launch with the fused epilogue -- api.hip enum BenchMode) */
int mms_dbg_gemm_bench(int64_t M, int64_t N, int64_t K, int32_t nsplit, int32_t act, int32_t out_planes, int32_t resid,
                       int32_t what, int32_t iters, float* ms_out);
int mms_dbg_attention(const float* q, const float* k, const float* v, int64_t B, int32_t Sq, int32_t Sk,
                      const float* key_add, float* out_f32, void* stream);
/* ONE fused QKV-projection + attention launch (qkv_attn.hip) on fp32 operands (all device pointers but n_sub_out): x [rows1 + rows2][768], the rows of stream 1
 * first; a pair's tokens are consecutive rows of a stream -- off / cnt [n_pairs] per stream (first row relative to the stream, tokens), or NULL = dense, S tokens per
 * pair; rows2 == 0: self-attention of stream 1, else CROSS attention: the queries of either stream attend the keys of the OTHER stream of their pair (lxmert X layers);
 * w_qkv [2304][768] = [Wq; Wk; Wv] in torch Linear layout, bias_qkv [2304]; key_add: additive key mask by stream row or NULL; mode 1: exact-fp32 attention MFMAs
 * (self-attention, pairs of <= 48 tokens), 2: the split-bf16 route (qkv_attn2_kernel).  ctx_f32 [rows1 + rows2][768]; *n_sub_out = sub-tiles the plan made */
int mms_dbg_qkv_attn(const float* x, int64_t rows1, int64_t rows2, const int32_t* off1, const int32_t* cnt1, const int32_t* off2, const int32_t* cnt2,
                     int64_t n_pairs, int32_t S1, int32_t S2, const float* w_qkv, const float* bias_qkv, const float* key_add1, const float* key_add2,
                     int32_t mode, float* ctx_f32, int32_t* n_sub_out, void* stream);
/* launch counters since mms_create: which = 0 -> fused QKV + attention launches (mms_config.fuse_attention took effect), 1 -> GEMM launches
 * with the fused LayerNorm epilogue (mms_config.fuse_layernorm), 2 -> split-K launches of the small-call routes, 3 -> skinny-GEMM launches (launches of <= 128
 * padded rows, precision modes 2 and 3), 4 -> fork / join pairs of the second launch lane (lxmert handles; on a zk handle: the member lanes of mms_score_ensemble);
 * 5 -> not a launch counter: the bytes of device memory the handle holds NOW (weights, workspaces, partials: the sum over its pools -- a warmed-up handle's figure
 * does not move from call to call); anything else: -1 */
int64_t mms_dbg_counter(mms_handle* h, int32_t which);
int mms_dbg_layernorm(const float* x, const float* gamma, const float* beta, int64_t M, float* out_f32, void* stream);
/* ONE launch of the small-sequence attention kernel (attn.hip) in the forms the forwards use.  q / k / v: device fp32, already in the layout `flags` names; B pairs;
 * Sq / Sk: the MAXIMUM tokens of a pair (tile selection, <= 48); q_rows / kv_rows: rows of the two streams.  q_off / q_cnt, kv_off / kv_cnt: int32 [B] first row and
 * live tokens of every pair (1 <= cnt <= S, rows inside the stream: checked on the host), or NULL = dense (row b * S, S tokens).  key_add: additive key mask by
 * kv-stream row, or NULL.  flags:
 *   bit 0  head-major operands: q = 12 blocks [q_rows][64], k and v = 12 blocks [kv_rows][64] each (the [Q | K | V] blocks of a forward's projection buffer);
 *          else row-major [rows][768]
 *   bit 1  reverse: the last pair first
 *   bit 2  CLS-only (the last layer before the pooler): q is a compact row-major [B][768] whatever bit 0 says, Sq == 1, q_rows == B, no q_off; output row b
 *   bit 3  the context leaves as e4m3 bytes (precision 4) instead of the split planes
 * out_f32 [q_rows (bit 2: B)][768]: the planes, or the decoded bytes; both are zero-filled before the launch, so a row no live query owns comes back 0 */
int mms_dbg_attention_ex(const float* q, const float* k, const float* v, int64_t B, int32_t Sq, int32_t Sk, int64_t q_rows, int64_t kv_rows,
                         const int32_t* q_off, const int32_t* q_cnt, const int32_t* kv_off, const int32_t* kv_cnt, const float* key_add,
                         int32_t flags, float* out_f32, void* stream);
/* ONE pack plan (rowops.hip) of n pairs with T text tokens, its raw tables written to the caller's device buffers.  kind:
 *   0  zk, the one-block route (n <= 1024)          in_a = len_query int32 [n], in_b = num_boxes int32 [n]
 *   1  zk, the three-launch route (token + box plan) same inputs
 *   2  lds                                           in_a = features fp32 [n][10][2048], in_b = labelfeat int64 [n][10][8]
 *   3  lxmert, both streams                          in_a = input_mask int64 [n][T], in_b = visual_attention_mask fp32 [n][10]
 *   4  lxmert, language stream only                  in_a = input_mask; in_b ignored
 * off / cnt [n], tok_src / key_add [n * (tokens of a dense pair)]: the token plan (lxmert: the language stream); rows_dev[0] = its live rows.
 * off2 / cnt2 [n], src2 [n * 10]: kinds 0, 1 the box plan, kind 3 the vision stream (with add2 [n * 10]); rows_dev[1] = its live rows.  Kind 2: src2 (optional)
 * receives the "box has a non-zero feature" flags [n * 10].  Kind 4 does not touch the second table */
int mms_dbg_pack_plan(int32_t kind, int64_t n, int32_t T, const void* in_a, const void* in_b, int32_t* off, int32_t* cnt, int32_t* tok_src, float* key_add,
                      int32_t* off2, int32_t* cnt2, int32_t* src2, float* add2, int32_t* rows_dev, void* stream);
/* ONE de-duplication (batchops.hip) with a workspace sized as a forward sizes it (hash table: the smallest power of two >= max(1024, 2 * rows)).  kind 0: label
 * tuples int32 [rows][8]; 1: int64 [rows][8]; 2: lxmert queries, ids / mask int64 [rows][T].  *count_out (host) = distinct keys; index [rows]; kinds 0, 1: uniq32 /
 * uniq64 [rows][8] (either may be NULL); kind 2: rows_of [rows], the first row of every distinct query */
int mms_dbg_dedup(int32_t kind, const void* ids, const int64_t* mask, int32_t T, int64_t rows, int32_t* count_out, int32_t* index, int32_t* uniq32,
                  int64_t* uniq64, int32_t* rows_of, void* stream);
/* the LayerNorm kernel with the fields mms_dbg_layernorm leaves at their defaults: out = LN(x + resid[r_index ? r_index[row] : row]).  resid_f32 [resid_rows][768] or
 * NULL; r_index int32 [M] (entries in [0, resid_rows): checked on the host) or NULL; m_live >= 0: the device-side row count (rows >= min(M, m_live) are not
 * written), < 0: none.  flags: bit 0 reverse, bit 1 also write the row as e4m3 bytes (decoded to out_f8 [M][768]), bit 2 the skip word is set (nothing is
 * written).  The planes and the bytes are zero-filled first */
int mms_dbg_layernorm_ex(const float* x, const float* gamma, const float* beta, int64_t M, const float* resid_f32, int64_t resid_rows, const int32_t* r_index,
                         int64_t m_live, int32_t flags, float* out_f32, float* out_f8, void* stream);
int mms_dbg_layernorm_rows(const float* x, const float* gamma, const float* beta, int64_t M, const float* resid_f32, int64_t resid_rows, const int32_t* r_index,
                           int64_t m_live, int32_t flags, float* out_f32, float* out_f8,
                           const int32_t* rmap /* optional host {grp, stride, off}: without r_index the residual row of row r is LnResid::rmap(r), checked on the host */, void* stream);
/* mms_dbg_gemm (two-pass bf16 planes, no residual) with a device-side live-row count and the head-major output of the QKV projections: m_live >= 0: rows >=
 * min(M, m_live) are not written, < 0: none.  out_kind 0: c_f32 [M][N]; 1: split planes, joined to fp32 [M][N]; 2: head-major fp32 [N / 64][M][64].
 * reverse 1: the tiles are walked from the last row tile down, as every second big launch of a forward walks them (the ragged tile first).  c_f32 is zero-filled first */
int mms_dbg_gemm_ex(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, int64_t N, const float* bias, int32_t act, int32_t out_kind,
                    int32_t engine, int64_t m_live, int32_t reverse, float* c_f32, void* stream);
/* one conversion launcher on n elements (n % 32 == 0).  kind 0: fp32 -> e4m3 bytes; 1: e4m3 bytes -> fp32; 2: fp32 -> split planes -> fp32 (round trip);
 * 3: fp32 -> split planes -> e4m3 bytes */
int mms_dbg_convert(int32_t kind, const void* in, void* out, int64_t n, void* stream);
/* ONE GEMM launch with the six addressing fields of GemmParams as a forward sets them: C[cmap(r)] = act(A[a_index ? a_index[r] : amap(r)] W^T + bias
 * (+ resid[r_index ? r_index[r] : rmap(r)])) for r < min(M, m_live).  a_index / r_index: device int32 [M] or NULL; resid_f32 NULL: no residual.  c_f32 is the
 * caller's PRE-FILLED physical output (mms_rows_spec::out_kind) and is never cleared: for planes its fp32 image is split into the plane buffer before the launch and
 * the WHOLE buffer is joined back after it, so the caller sees every element the kernel did or did not touch.  Before anything is launched the host checks that
 * every A row, residual row and output row (head-major: every block) that a logical row r < M -- M, not m_live -- can address lies inside the buffers the spec
 * describes: MMS_ERR_ARG otherwise, and MMS_ERR_ARG with c_f32 untouched when the named engine's launcher refuses the launch */
int mms_dbg_gemm_rows(const mms_rows_spec* spec, const float* a_f32, const int32_t* a_index, const float* w_f32_nk, const float* bias,
                      const float* resid_f32, const int32_t* r_index, float* c_f32, void* stream);
/* k_splitk_reduce alone: out = act(sum_s parts[s] + bias), parts device fp32 [S][M][N] (N % 4 == 0), rows r < min(M, m_live) (m_live < 0: M).  out_kind / ldo /
 * c_rows / hm_rows / hm_col0 / hm_blocks as in mms_rows_spec (the kernel has no row map: c_rows, hm_rows >= M); c_f32 is the caller's pre-filled physical image */
int mms_dbg_splitk_reduce(const float* parts, int32_t S, int64_t M, int64_t N, const float* bias, int32_t act, int64_t m_live, int32_t out_kind,
                          int32_t ldo, int64_t c_rows, int32_t hm_rows, int32_t hm_col0, int32_t hm_blocks, float* c_f32, void* stream);
#endif /* MMS_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif
