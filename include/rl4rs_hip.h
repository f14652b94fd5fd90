/*
 * rl4rs_hip.h — C ABI of librl4rs_hip.so: the MI355X (gfx950) implementation of the RL4RS batched
 * env.step() hot path (boundary row b).
 *
 * The reference is pure Python; it has no FFI.  Each entry point below replaces the Python call a
 * reference maintainer would bind through ctypes; the reference interface it
 * replaces is cited as rl4rs/<file>:<line>.
 *
 * Conventions
 *   - every function returns 0 on success, a negative RL4RS_E* code on failure; the message of the
 *     last failure on the calling thread is available from rl4rs_last_error().
 *   - "dev" pointers are device (HBM) addresses, "host" pointers are host addresses; the caller owns
 *     every buffer it passes in; handles own their internal state.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue work on
 *     that stream: no allocation, no host synchronisation inside step / forward calls.
 *   - a handle is bound to the HIP device that was current when it was created and is not thread-safe.
 *   - plain C types only: no torch / STL types cross this boundary.
 */
#ifndef RL4RS_HIP_H
#define RL4RS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL4RS_ABI_VERSION 1

enum {
    RL4RS_OK = 0,
    RL4RS_EINVAL = -1,   /* bad argument / configuration */
    RL4RS_EHIP = -2,     /* a HIP runtime call failed */
    RL4RS_ESTATE = -3,   /* call not valid in the handle's current state (e.g. step past the horizon) */
    RL4RS_ENOMEM = -4
};

const char* rl4rs_last_error(void);
int rl4rs_abi_version(void);
/* number of HIP devices visible; <0 on error.  The library never falls back to a CPU path. */
int rl4rs_device_count(void);

/* Async device-to-device copy on `stream` (lets a host binding snapshot env-owned buffers into
 * caller-owned ones without linking the HIP runtime itself). */
int rl4rs_copy_d2d(void* dst_dev, const void* src_dev, int64_t n_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Env state machine: SlateState / SeqSlateState (rl4rs/env/slate.py:8-214, rl4rs/env/seqslate.py:8-126)
 * ---------------------------------------------------------------------------------------------- */

typedef struct rl4rs_env rl4rs_env;

typedef struct rl4rs_env_cfg {
    int32_t batch_size;            /* config['batch_size']                       slate.py:11 */
    int32_t max_steps;             /* config['max_steps']                        slate.py:14 */
    int32_t action_size;           /* config['action_size']                      slate.py:12 */
    int32_t action_emb_size;       /* config['action_emb_size'] (32)             slate.py:13 */
    int32_t page_items;            /* config['page_items'] (9)                   seqslate.py:11 */
    int32_t item_dim;              /* len(item_vec) (40)                         slate.py:35 */
    int32_t user_dense_dim;        /* len(user_protrait[10:]) (32)               slate.py:78 */
    int32_t user_cat_dim;          /* len(user_protrait[:10]) (10)               slate.py:79 */
    int32_t maxlen;                /* config['maxlen'] (64)                      datautil.py:12 */
    int32_t dense_feature_num;     /* config['dense_feature_num'] (432)          datautil.py:15 */
    int32_t category_feature_num;  /* config['category_feature_num'] (21)        datautil.py:16 */
    int32_t log_steps;             /* columns of exposed_items / user_feedback in the loaded batch */
    int32_t is_seq;                /* 0 = SlateState rules, 1 = SeqSlateState rules */
    int32_t violation_zeroes_reward; /* slate.py:303-307 (always) / seqslate.py:154-157 (mask modes only) */
} rl4rs_env_cfg;

int rl4rs_env_create(const rl4rs_env_cfg* cfg, rl4rs_env** out);
int rl4rs_env_destroy(rl4rs_env* env);

/* Catalogue tables parsed on the host from item_info.csv
 * (SlateState.get_iteminfo_from_file slate.py:28-53, get_mask_from_file slate.py:55-65).
 *   item_vec_host     [action_size, item_dim] float32 (row 0 = zeros)
 *   price_host        [action_size] float64
 *   action_emb_host   [action_size, action_emb_size] float64
 *   is_special_host   [action_size] uint8
 *   location_mask_host[4, action_size] uint8
 */
int rl4rs_env_set_catalog(rl4rs_env* env, const float* item_vec_host, const double* price_host,
                          const double* action_emb_host, const uint8_t* is_special_host,
                          const uint8_t* location_mask_host, void* stream);

/* One sampled batch of log records in columnar form (RecDataBase.sample base.py:92-100 +
 * SlateState.records_to_state slate.py:67-83 + pad_sequences of the history, datautil.py:43-46).
 * Device pointers; copied into the env (async on `stream`).
 *   exposed_dev   [B, log_steps] int32      exposed_items
 *   feedback_dev  [B, log_steps] int32      user_feedback
 *   history_dev   [B, maxlen]    int32      user_seqfeature, pre-padded / pre-truncated
 *   user_dense_dev[B, user_dense_dim] float32
 *   user_cat_dev  [B, user_cat_dim]   int32
 */
int rl4rs_env_load_batch(rl4rs_env* env, const int32_t* exposed_dev, const int32_t* feedback_dev,
                         const int32_t* history_dev, const float* user_dense_dev,
                         const int32_t* user_cat_dev, void* stream);
/* The same as ONE launch when the log is resident on the device (rl4rs_amd LogStore: the sample file parsed once into
 * columnar tables of n_lines rows): gathers the sampled lines line_idx_dev int32 [B] (RecDataBase.sample, base.py:92-100) into
 * the batch buffers, writes the start-of-episode state (prev_actions = 0, both masks all ones; slate.py:8-27) so that the
 * following rl4rs_env_reset only builds the state rows, and - optionally - copies the histories of the batch's n_uniq DISTINCT
 * lines uniq_idx_dev int32 [n_uniq] to hist_unique_dev int32 [n_uniq, maxlen] (what the scorer encodes once per history).
 * store_*: exposed / feedback int32 [n_lines, log_steps], history int32 [n_lines, maxlen], user_dense float32
 * [n_lines, user_dense_dim], user_cat int32 [n_lines, user_cat_dim]. */
int rl4rs_env_load_lines(rl4rs_env* env, const int32_t* store_exposed, const int32_t* store_feedback, const int32_t* store_history,
                         const float* store_user_dense, const int32_t* store_user_cat, int32_t n_lines, int32_t store_log_steps,
                         const int32_t* line_idx_dev, const int32_t* uniq_idx_dev, int32_t n_uniq, int32_t* hist_unique_dev,
                         void* stream);

/* HOST-side parser of a text buffer of '\n'-separated '@'-records (blank lines skipped) into the columnar HOST
 * arrays above: FeatureUtil.record_split (datautil.py:20-32) + records_to_state (slate.py:67-83) + pad_sequences
 * of the history (datautil.py:43-46), for a whole sample file at once.  exposed/feedback are zero padded /
 * truncated to log_steps columns; exposed_len_host (optional) receives each record's true exposed_items count. */
int rl4rs_parse_records(const char* text, int64_t len, int32_t max_records, int32_t maxlen, int32_t log_steps,
                        int32_t user_dense_dim, int32_t user_cat_dim, int32_t* exposed_host, int32_t* feedback_host,
                        int32_t* history_host, float* user_dense_host, int32_t* user_cat_host,
                        int32_t* exposed_len_host, int32_t* n_parsed);

/* HOST-side CRC-32C (Castagnoli) of a byte range, continuing the running checksum `crc` (0 starts one): the
 * checksum of the TFRecord framing (tf.io behind FeatureUtil.to_tfrecord / read_tfrecord, datautil.py:71-230)
 * and of the tensor-bundle checkpoints tf.train.Saver writes (base.py:129,151; supervised_train.py:44-46). */
uint32_t rl4rs_crc32c(const void* data, int64_t len, uint32_t crc);

/* RecState.__init__ (base.py:27-31) + SlateState.__init__ (slate.py:15-19): zero prev_actions, masks
 * to all-ones, cur_steps = 0, feature rows = the un-acted state. */
int rl4rs_env_reset(rl4rs_env* env, void* stream);

/* SlateState.act / SeqSlateState.act with integer actions (slate.py:198-214, seqslate.py:98-126). */
int rl4rs_env_act_discrete(rl4rs_env* env, const int32_t* actions_dev, void* stream);

/* Continuous actions: masked K-NN argmax in float64 (slate.py:187-197, seqslate.py:93-97) followed by
 * act.  `actions_dev` is [B, action_emb_size] float32 (is_f64 = 0) or float64 (is_f64 = 1);
 * `chosen_dev` (optional) receives the item ids that were played. */
int rl4rs_env_act_conti(rl4rs_env* env, const void* actions_dev, int is_f64, int32_t* chosen_dev,
                        void* stream);

/* SlateState.get_nearest_neighbor / get_nearest_neighbor_with_mask (slate.py:180-191, static):
 * [n,E] -> [n].  mask_dev: optional uint8 [n, action_size] (0 = score forced to -2**31). */
int rl4rs_knn(const void* actions_dev, int is_f64, int32_t n, const double* action_emb_dev,
              int32_t action_size, int32_t emb_size, const uint8_t* mask_dev, int32_t* out_dev,
              void* stream);

/* get_complete_states + feature_extraction for the reward rows (slate.py:117-131,289-294;
 * seqslate.py:27-50,141-146): fills the env's complete-state buffers ([B*n, ...], env-major). */
int rl4rs_env_build_complete(rl4rs_env* env, void* stream);
/* Same, emitting only the first rows_per_env (<= complete_rows) rows of each env ([B*rows_per_env, ...]).
 * The LAST complete row of an env equals its current state row (same prev_actions, action = the item just
 * played; slate.py:205-212 vs :119-130), so a caller that already scored the state row can skip it. */
int rl4rs_env_build_complete_rows(rl4rs_env* env, int32_t rows_per_env, void* stream);
/* rows per env produced by build_complete: max_steps (Slate) or page_items (SeqSlate). */
int rl4rs_env_complete_rows(const rl4rs_env* env);
/* 1 when SlateRecEnv.forward / SeqSlateRecEnv.forward would call the reward net now
 * (slate.py:283, seqslate.py:138). */
int rl4rs_env_is_reward_step(const rl4rs_env* env);
int rl4rs_env_cur_steps(const rl4rs_env* env);

/* reward = sum_j price*prob in float64 (numpy pairwise order), zeroed on violation
 * (slate.py:298-307, seqslate.py:150-157).  probs_dev [B, n] float32, reward_dev [B] float64. */
int rl4rs_env_reward(rl4rs_env* env, const float* probs_dev, double* reward_dev, void* stream);

/* Same with the last row's probability supplied separately: probs_dev [B, n-1], p_last_dev [B] (NULL = probs_dev
 * holds all n). */
int rl4rs_env_reward_split(rl4rs_env* env, const float* probs_dev, const float* p_last_dev, double* reward_dev,
                           void* stream);

/* get_violation (slate.py:133-147, seqslate.py:52-69): out_dev [B] int32 in {0,1}. */
int rl4rs_env_violation(rl4rs_env* env, int32_t* out_dev, void* stream);

/* state['action_mask'] = action_mask & location_mask[layer(post-increment cur_steps)] & special_mask
 * (slate.py:92-97, seqslate.py:15-17).  out_dev [B, action_size]; dtype: 0=uint8 1=int32 2=int64 3=float32;
 * dtype 4: packed, out_dev [B, (action_size + 31) / 32] uint32 words, bit k & 31 of word k >> 5 = action k (the mask_bits
 * layout of rl4rs_policy_*) */
int rl4rs_env_obs_mask(rl4rs_env* env, void* out_dev, int dtype, void* stream);

/* offline_action (slate.py:149-162): ids_dev [B] int32, and/or emb_dev [B, E] float64 (conti mode). */
int rl4rs_env_offline_action(rl4rs_env* env, int32_t* ids_dev, double* emb_dev, void* stream);
/* offline_reward (slate.py:164-174, seqslate.py:71-86): out_dev [B] float64. */
int rl4rs_env_offline_reward(rl4rs_env* env, double* out_dev, void* stream);

/* policy_model.predict_with_mask (rl4rs/policy/policy_model.py:17-41; same mask rule as
 * CustomVectorEncoder.forward, rl4rs/nets/cql/encoder.py:42-67): masked argmax where the mask is re-derived
 * from the observation tail.  scores_dev [N, action_size] f32, prev_dev [N, prev_cols] int32 (the obs tail's
 * previous actions), cur_step_dev [N] int32, out_dev [N] int32.  Uses the env's catalogue tables only. */
int rl4rs_env_predict_with_mask(rl4rs_env* env, int32_t N, const float* scores_dev, const int32_t* prev_dev,
                                int32_t prev_cols, const int32_t* cur_step_dev, int32_t* out_dev, void* stream);

/* Kernel-path selection of one env handle (A/B measurements; same results): ROWS_VARIANT 0 [default] = the row kernels stage
 * the catalogue in LDS, 1 = they read it through L1 / L2. */
enum { RL4RS_ENV_OPT_ROWS_VARIANT = 0 };
int rl4rs_env_set_option(rl4rs_env* env, int32_t which, int32_t value);

/* The configuration the env was created with. */
int rl4rs_env_get_cfg(const rl4rs_env* env, rl4rs_env_cfg* out);

/* Device views of env-owned buffers (valid until destroy).  `which`: */
enum {
    RL4RS_BUF_PREV_ACTIONS = 0,   /* int32  [B, max_steps] */
    RL4RS_BUF_ACTION_MASK = 1,    /* uint32 [B, ceil(A/32)] bit k of word k/32 = action_mask[b,k] */
    RL4RS_BUF_SPECIAL_MASK = 2,   /* uint32 [B, ceil(A/32)] */
    RL4RS_BUF_DENSE = 3,          /* float32 [B, dense_feature_num]      feature_extraction()[1] */
    RL4RS_BUF_CATEGORY = 4,       /* int32  [B, category_feature_num]    feature_extraction()[2] */
    RL4RS_BUF_SEQ0 = 5,           /* int32  [B, maxlen]                  sequence 0 (history)     */
    RL4RS_BUF_SEQ1 = 6,           /* int32  [B, maxlen]                  sequence 1               */
    RL4RS_BUF_C_DENSE = 7,        /* float32 [B*n, dense_feature_num]    complete-state rows      */
    RL4RS_BUF_C_CATEGORY = 8,     /* int32  [B*n, category_feature_num] */
    RL4RS_BUF_ERROR_FLAG = 9      /* int32  [1]  sticky: 1 = an action id outside [0, action_size) */
};
int rl4rs_env_buffer(rl4rs_env* env, int which, void** dev_ptr, int64_t* n_bytes);

/* ------------------------------------------------------------------------------------------------
 * DIEN simulator net: rl4rs/nets/dien.py:8-45, rl4rs/nets/utils.py:16-25,48-54,100-129,
 * called from SlateRecEnv.obs_fn / forward (slate.py:265-267, 295-297) as obs_layer / reward_layer.
 * ---------------------------------------------------------------------------------------------- */

typedef struct rl4rs_dien rl4rs_dien;

typedef struct rl4rs_dien_cfg {
    int32_t maxlen;                /* 64  */
    int32_t emb_size;              /* 128 */
    int32_t hidden_units;          /* 128 */
    int32_t dense_feature_num;     /* 432 */
    int32_t category_feature_num;  /* 21  */
    int32_t category_hash_size;    /* 100000 */
    int32_t seq_num;               /* 2   */
    int32_t class_num;             /* 2   */
    int32_t max_rows;              /* largest R passed to rl4rs_dien_forward */
    int32_t max_slots;             /* sequence-cache slots per sequence input */
    int32_t scorer_mode;           /* RL4RS_SCORER_* : arithmetic of the AUGRU recurrence (the dominant kernel) */
    uint32_t kernel_opts;          /* RL4RS_DIEN_OPT_* bits, 0 = the defaults */
} rl4rs_dien_cfg;

/* Kernel-path selection of ONE scorer handle (A/B measurements, and parity tests that pin a path): configuration, never
 * process environment, so that handles with different paths can live side by side.  Every combination computes the same
 * function inside the parity bars of DESIGN.md 2; forms marked (=) are bit-identical to the default.
 *   AUGRU_H16       first-generation fp16x2 recurrence k_augru_h16 instead of k_augru_x
 *   AUGRU_ROWS32    k_augru_x: 32-row workgroups for every launch (=)
 *   AUGRU_ROWS64    k_augru_x: 64-row workgroups whenever the launch shape admits them (R % 64 == 0, rows in whole groups
 *                   of 8 per cache slot, or in groups of 9: 63 rows per workgroup), not only when that still fills the chip
 *                   twice over (=); see rl4rs_dien_set_augru_rows
 *   DIN_V1          first-generation attention-score kernel k_din_scores instead of k_din_x
 *   NO_DIN16 / NO_GRU16 / NO_GEMM16 / NO_CAT16   keep the exact-fp32 MFMA form of the attention MLP / first GRU / plain GEMMs /
 *                   category self-attention in fp16x2 mode
 *   NO_DENSE_CHAIN  dense tower as two GEMM launches instead of one chained launch (=)
 *   NO_HEAD_TABLES  head GEMM over all 3456 inputs instead of the per-category-slot tables
 *   NO_HEAD_FUSED   k_head_finish as its own launch instead of the table sums inside k_cat_attn
 *   CAT_V1          category branch through the first-generation k_cat_attn (full [Cn, E] LDS image per row: 12 rows in flight
 *                   per CU) instead of k_cat_attn2 (half-K image, 16+ rows per CU; E = 128 and Cn <= 24 only)
 *   NO_CAT_GROUP    launches whose rows come in groups of 8 or 9 per cache slot (the reward forward over the complete states):
 *                   category branch per row (k_cat_attn2) instead of one workgroup per group that gathers the category rows the
 *                   group shares once (k_cat_attn2g; a group that shares nothing takes the per-row body inside it) (=)
 *   NO_GEMM_GROUP   the chained dense tower and the q-side term of the DIN scores (independent GEMMs, half-chip grids at observation
 *                   size) as two launches instead of one grid that holds both problems' workgroups (k_gemm_h16_pair) (=)
 *   NO_ROW_DEDUP    k_din_x and k_augru_x over every row of a forward instead of one representative per set of bit-identical row
 *                   groups (equal cache slots, category ids and dense bit patterns: k_row_dedup finds them on the device at the top
 *                   of every forward, k_row_expand copies the representative's AUGRU states and attention scores to its duplicates
 *                   in front of the head GEMM).  Active only where k_din_x and k_augru_x are the selected kernels (=)
 *   DUP_STORE       row dedup: k_din_x and k_augru_x store every score / final-state piece of a representative to the same row of
 *                   its duplicates where it is produced (k_row_dedup then leaves the duplicates of every representative as a
 *                   list) and no k_row_expand is launched (=).  OFF by default: measured slower than the copy launch (building
 *                   the lists costs the one compacting workgroup more than the launch it saves)
 *   NO_DUP_STORE    pins that default: k_row_expand copies the representatives' rows to the duplicates (=)
 *   NO_TIER2_ROWS   row dedup: the category kernel, the dense tower / q-side GEMMs and the head GEMM over every row of a forward
 *                   instead of the representatives' rows only (they take the active list as k_din_x / k_augru_x do; k_row_expand
 *                   then runs behind the head GEMM and copies a duplicate's whole all-feature row, scores, query row and head
 *                   output).  The active-row form is used only with the default category / GEMM forms, without
 *                   DUP_STORE and DENSE_FORK, and not in a forward whose head GEMM writes a host mirror (=)
 *   DIN_ROWS16      k_din_x with 16 rows per workgroup whatever the row dedup left, instead of 8 (one row per wave) when the active
 *                   rows of an observation-sized launch fit one round that way (decided on the device) (=)
 *   NO_AUGRU_SHADOW an observation-sized forward (group == 1, 32-row k_augru_x, active-row second tier) keeps its seven launches:
 *                   category kernel and dense / q-side pair in front of k_din_x, instead of k_din_xq forming q and qa for its own
 *                   rows and the category branch and the dense tower running as a shadow plane of the AUGRU launch (k_augru_xs)
 *                   where ceil(G / 32) * (S + 1) workgroups fit the chip, G = rl4rs_dien_set_distinct_hint (=) */
enum {
    RL4RS_DIEN_OPT_AUGRU_H16 = 1 << 0,
    RL4RS_DIEN_OPT_AUGRU_ROWS32 = 1 << 1,
    RL4RS_DIEN_OPT_AUGRU_ROWS64 = 1 << 2,
    RL4RS_DIEN_OPT_DIN_V1 = 1 << 3,
    RL4RS_DIEN_OPT_NO_DIN16 = 1 << 4,
    RL4RS_DIEN_OPT_NO_GRU16 = 1 << 5,
    RL4RS_DIEN_OPT_NO_GEMM16 = 1 << 6,
    RL4RS_DIEN_OPT_NO_CAT16 = 1 << 7,
    RL4RS_DIEN_OPT_NO_DENSE_CHAIN = 1 << 8,
    RL4RS_DIEN_OPT_NO_HEAD_TABLES = 1 << 9,
    RL4RS_DIEN_OPT_NO_HEAD_FUSED = 1 << 10,
    RL4RS_DIEN_OPT_CAT_V1 = 1 << 11,
    RL4RS_DIEN_OPT_NO_CAT_GROUP = 1 << 12,
    RL4RS_DIEN_OPT_DENSE_FORK = 1 << 13,       /* the dense tower on a second stream of the handle, joined in front of the head GEMM */
    RL4RS_DIEN_OPT_NO_GRU_PAD = 1 << 14,       /* first GRU: compute the steps on leading zero ids (front padding) per row instead of
                                                  taking them from the handle's table of pad states (bit-identical either way) */
    RL4RS_DIEN_OPT_NO_GEMM_GROUP = 1 << 15,    /* fp16x2 mode: the dense tower and the q-side term of the DIN scores as two launches
                                                  instead of one grid that holds both problems' workgroups (bit-identical either way) */
    RL4RS_DIEN_OPT_NO_ROW_DEDUP = 1 << 16,     /* fp16x2 mode: k_din_x / k_augru_x score duplicate row groups of a forward too
                                                  (bit-identical either way) */
    RL4RS_DIEN_OPT_NO_DUP_STORE = 1 << 17,     /* row dedup: k_row_expand as its own launch (the default; bit-identical either way) */
    RL4RS_DIEN_OPT_DIN_ROWS16 = 1 << 18,       /* k_din_x: 16 rows per workgroup for every launch (bit-identical either way) */
    RL4RS_DIEN_OPT_DUP_STORE = 1 << 19,        /* row dedup: the duplicates' stores inside k_din_x / k_augru_x, no k_row_expand launch
                                                  (bit-identical either way) */
    RL4RS_DIEN_OPT_NO_TIER2_ROWS = 1 << 20,    /* row dedup: category kernel, dense / q-side GEMMs and head GEMM over all R rows, k_row_expand
                                                  in front of the head GEMM (bit-identical either way) */
    RL4RS_DIEN_OPT_NO_AUGRU_SHADOW = 1 << 21,  /* observation-sized forwards: category kernel and dense / q-side pair as launches of their own
                                                  in front of k_din_x, no shadow plane in the AUGRU launch (bit-identical either way) */
    RL4RS_DIEN_OPT_NO_LAZY_EXPAND = 1 << 22,   /* row dedup, second tier: k_row_expand behind the head GEMM in every forward, instead of
                                                  outputs that read the representative's row and internal rows completed by
                                                  rl4rs_dien_buffer (bit-identical either way) */
    RL4RS_DIEN_OPT_GRU_H16_V1 = 1 << 23,       /* fp16x2 mode, first GRU: the 4-wave k_gru_h16 and a k_h1_frag launch per encode instead of
                                                  k_gru_h16r (two wave roles per SIMD, writes the fragment-order copy itself;
                                                  bit-identical either way) */
    RL4RS_DIEN_OPT_ALL = (1 << 24) - 1
};

/* Every mode accumulates in fp32 and meets the fp32 parity bar against the fp64 oracle (same measured error):
 *   FP32   v_mfma_f32_32x32x2_f32, operands exact.
 *   FP16X2 operands split into fp16 hi + lo, 3 v_mfma_f32_32x32x16_f16 per product (hi*hi + hi*lo + lo*hi):
 *          ~2^-22 relative error per product, 2.3x faster.  No weight-range condition: a weight tile that would not fit
 *          fp16 (max |w| >= 2^14) is stored times a power of two and the accumulator divided by it, exactly (32-column tiles
 *          of the recurrent matrices, columns of the plain GEMMs).  Only NON-FINITE weights need FP32.  ACTIVATIONS are
 *          range-checked at run time: a row whose state / GEMM input leaves the fp16 range comes back NaN + status bit.
 *   AUTO   FP16X2 for every finite checkpoint, else FP32. */
enum { RL4RS_SCORER_AUTO = 0, RL4RS_SCORER_FP32 = 1, RL4RS_SCORER_FP16X2 = 2 };

/* Host pointers to float32 arrays, shapes in rl4rs_amd/nets/dien.py (dien_spec). seq arrays have
 * seq_num entries (max 4). */
typedef struct rl4rs_dien_weights {
    const float* cat_emb;
    const float* dense_w1; const float* dense_b1;
    const float* dense_w2; const float* dense_b2;
    const float* seq_emb;
    const float* gru_gate_w[4];   const float* gru_gate_b[4];
    const float* gru_cand_w[4];   const float* gru_cand_b[4];
    const float* att_w1[4]; const float* att_b1[4];
    const float* att_w2[4]; const float* att_b2[4];
    const float* att_w3[4]; const float* att_b3[4];
    const float* augru_gate_w[4]; const float* augru_gate_b[4];
    const float* augru_cand_w[4]; const float* augru_cand_b[4];
    const float* obs_w; const float* obs_b;
    const float* out_w; const float* out_b;
} rl4rs_dien_weights;

int rl4rs_dien_create(const rl4rs_dien_cfg* cfg, const rl4rs_dien_weights* w, void* stream,
                      rl4rs_dien** out);
int rl4rs_dien_destroy(rl4rs_dien* net);
/* The mode the handle resolved to (RL4RS_SCORER_FP32 or RL4RS_SCORER_FP16X2). */
int rl4rs_dien_scorer_mode(rl4rs_dien* net, int32_t* mode);
/* Row-tile form of k_augru_x for the following forwards of this handle: 0 automatic, 32, 64 (the AUGRU_ROWS* options above,
 * switchable on a live handle so that one cache can be scored by both forms). */
int rl4rs_dien_set_augru_rows(rl4rs_dien* net, int32_t rows);
/* Distinct row groups the row dedup is expected to leave in the following forwards of this handle (0 = no expectation: the rows of
 * the forward).  Only sizes decisions, never results: an observation-sized forward takes the shadow-plane order (NO_AUGRU_SHADOW above)
 * where ceil(min(n_groups, R) / 32) * (S + 1) workgroups fit the chip.  rl4rs_stepper_set_distinct_hint passes its hint on. */
int rl4rs_dien_set_distinct_hint(rl4rs_dien* net, int32_t n_groups);
/* Status bits since the last call (synchronises `stream`, then clears them).  RL4RS_DIEN_STATUS_FP16_RANGE: in
 * FP16X2 mode a recurrent state left the fp16 range (|h| >= 6e4, or NaN) - possible only when the attention scores
 * push the update gate outside [0, 1] until the state diverges; results of the affected forwards are invalid, use
 * RL4RS_SCORER_FP32 for such a model. */
enum { RL4RS_DIEN_STATUS_FP16_RANGE = 1 };
int rl4rs_dien_status(rl4rs_dien* net, int32_t* flags, void* stream);
/* The status word itself: device pointer to ONE int32 owned by the handle, != 0 <=> RL4RS_DIEN_STATUS_FP16_RANGE pending.  A
 * caller that copies a record to the host every step anyway (rl4rs_env_step_record) reads it there. */
int rl4rs_dien_status_word(rl4rs_dien* net, int32_t** word_dev);

/* Encode `n` id sequences of sequence input `s` into cache slots [slot_base, slot_base+n):
 * embedding lookup + first GRU over all maxlen steps (utils.py:119-120) and the input-side
 * projections of the attention MLP / AUGRU that depend only on it.  ids_dev [n, maxlen] int32.
 * Front padding (rl4rs/utils/datautil.py:44: pad_sequences pads in FRONT): the states after k leading zero ids are the same for
 * every sequence, so (FP16X2 mode, unless RL4RS_DIEN_OPT_NO_GRU_PAD) the handle keeps them in a table and in one extra cache slot
 * behind max_slots; encode starts every 32-row block at its shortest zero prefix and records each slot's prefix length, and the
 * forward's AUGRU / DIN kernels read the steps of a row's prefix from that one slot.  Bit-identical to computing them per row. */
int rl4rs_dien_encode(rl4rs_dien* net, int32_t s, const int32_t* ids_dev, int32_t n,
                      int32_t slot_base, void* stream);

/* Forward R rows (obs_layer / reward_layer, slate.py:265-267,295-297).
 *   dense_dev [R, dense_feature_num] f32, cat_dev [R, category_feature_num] i32
 *   slot_dev  [seq_num, R/group] int32: cache slot of sequence input s for each group of `group`
 *             consecutive rows (rows of one env share their sequences)
 *   obs_dev   [R, 256] f32  'simulator_obs' activations (may be NULL)
 *   prob_dev  [R] f32       softmax('simulator_reward')[:, 1] (may be NULL)
 */
int rl4rs_dien_forward(rl4rs_dien* net, int32_t R, int32_t group, const float* dense_dev,
                       const int32_t* cat_dev, const int32_t* slot_dev, float* obs_dev,
                       float* prob_dev, void* stream);

/* The NEXT rl4rs_dien_forward of this handle (one call, and one that returns probabilities) also stores the 'simulator_obs'
 * activations of the LAST row of each group: obs_last_dev [R / group, 256] f32 - without writing all R rows to the caller.  The
 * values are the head's own rows: bit-identical to a group-1 forward of that row.  NULL disarms. */
int rl4rs_dien_set_obs_last(rl4rs_dien* net, float* obs_last_dev);

/* The NEXT rl4rs_dien_forward of this handle (one call, as with rl4rs_dien_set_obs_last) takes the duplicate row groups of its
 * input from the caller instead of looking for them: it launches no k_row_dedup and hands the three buffers to everything that
 * reads the handle's own partition otherwise (k_din_x / k_din_xq, k_augru_x / k_augru_xs, the mapped GEMMs, the category kernels,
 * k_row_expand).  int32 device memory the caller owns and keeps unchanged until the forward has run:
 *   rep_dev      [n_groups]  representative of every row group; rep[g] == g: g is one
 *   active_dev   [n_active]  the representatives in processing order (rl4rs_dien_set_row_order; none: ascending)
 *   n_active_dev [1]         their number
 * That forward must have R / group == n_groups and the row dedup on (and not the dup_store form): anything else is an error.
 * The caller's contract, which the scorer does NOT check:
 *   - rep[rep[g]] == rep[g] for every g;
 *   - active lists exactly the groups with rep[g] == g, in processing order;
 *   - the rows of g and of rep[g] (category ids and dense values, `group` rows each) are bitwise equal and their cache slots are
 *     equal for every sequence input.
 * Under it the forward's outputs are bit-identical to those of a forward that compares the rows itself; a partition that merges
 * rows which differ gives the duplicates the representative's results.  rep_dev == NULL disarms.  rl4rs_env_step_* carry the
 * partition of the env batch from step to step this way (rl4rs_stepper_set_partition_carry). */
int rl4rs_dien_set_row_partition(rl4rs_dien* net, const int32_t* rep_dev, const int32_t* active_dev, const int32_t* n_active_dev,
                                 int32_t n_groups);
/* Forwards since the last rl4rs_dien_profile_reset that launched k_row_dedup / that took a caller's partition instead (host
 * counters, kept whether profiling is on or not; the profile class of k_row_dedup keeps one empty entry for a launch not issued,
 * so that its counts stay comparable between handles). */
int rl4rs_dien_dedup_counts(rl4rs_dien* net, int64_t* launched, int64_t* carried);

/* The launch plan of the last forward as one line of key=value tokens (which form every stage took: csrc/dien_plan.hpp,
 * dien_plan_str); "" before the first forward. */
int rl4rs_dien_last_plan(rl4rs_dien* net, char* buf, int32_t cap);

/* softmax(obs @ out_w + out_b)[:, 1] of already computed 'simulator_obs' activations (dien.py:36):
 * obs_dev [R, 256] -> prob_dev [R]. */
int rl4rs_dien_head_prob(rl4rs_dien* net, int32_t R, const float* obs_dev, float* prob_dev, void* stream);

/* Intermediate activations for parity tests; `which`: */
enum {
    RL4RS_DIEN_ALL_FEATURE = 0,   /* float32 [max_rows, ld] concat input of simulator_obs; ld = n_bytes / (4 max_rows):
                                     2E*seq_num + U + (Cn+1)E, or only the first 2E*seq_num + U + E columns when the
                                     Flatten(category_emb) part lives in the head tables */
    RL4RS_DIEN_SCORES = 1,        /* float32 [seq_num, max_rows, maxlen] attention scores */
    RL4RS_DIEN_QUERY = 2,         /* float32 [max_rows, E] */
    RL4RS_DIEN_H1 = 3,            /* float32 [seq_num, max_slots, maxlen, E] first-GRU states */
    RL4RS_DIEN_N_ACTIVE = 4,      /* int32 [1] row groups k_din_x / k_augru_x scored in the last forward (row dedup; an error
                                     on a handle where it is off) */
    RL4RS_DIEN_ROW_REP = 5,       /* int32 [max_rows] representative group of every row group of the last forward, first
                                     R / group entries (rep[g] == g: scored itself) */
    RL4RS_DIEN_ROW_ACTIVE = 6,    /* int32 [max_rows] the representatives of the last forward in processing order, first
                                     N_ACTIVE entries.  After a forward that took its partition from the caller
                                     (rl4rs_dien_set_row_partition) the three ids give the caller's buffers, n_bytes = 4 n_groups */
    RL4RS_DIEN_H1_FRAG = 7,       /* float32 [max_slots + 1, ceil(maxlen / 32), 8, 64, 8] sequence input 0's first-GRU states in the
                                     fragment order k_din_x reads (an error on a handle that keeps none) */
    RL4RS_DIEN_LEAD = 8           /* int32 [max_slots + 1] leading zero ids of sequence input 0's history in every cache slot (an
                                     error on a handle without the pad table) */
};
/* ALL_FEATURE, SCORES and QUERY: with the row dedup on, a forward computes these rows for the representatives only and (unless
 * RL4RS_DIEN_OPT_NO_LAZY_EXPAND, or a form of the forward that keeps k_row_expand) no longer copies them to the duplicates.
 * This call then issues that copy on the last forward's stream - once, a second call does nothing - before it returns the
 * pointer, so every row reads as before.  It must come before the handle's next forward and, for a handle driven by a stepper,
 * before the env's next act (the act rewrites the partition the forward ran on; the pending copy is then dropped and the
 * duplicates' internal rows stay what earlier forwards left there).  The forward's outputs (obs, prob, obs_last) are always
 * complete. */
int rl4rs_dien_buffer(rl4rs_dien* net, int which, void** dev_ptr, int64_t* n_bytes);

/* Processing order of the row groups (envs) of the following forwards: order_dev[i] = group handled at position i, a
 * permutation of 0..n_groups-1 in caller-owned device memory (NULL = identity).  A locality hint only (results per row are
 * unchanged): envs sorted by the cache slot of their history make duplicate histories share L2 lines
 * (RecDataBase.sample draws with replacement, rl4rs/env/base.py:92-100).  Applies when n_groups == R / group. */
int rl4rs_dien_set_row_order(rl4rs_dien* net, const int32_t* order_dev, int32_t n_groups);

/* Per-kernel HIP-event timing (bench.py roofline).  With profiling enabled every kernel class launched
 * by rl4rs_dien_encode / rl4rs_dien_forward is bracketed by an event pair on the caller's stream.
 * rl4rs_dien_profile_read synchronises on the recorded pairs and returns the cumulative milliseconds
 * and launch count of kernel class `which` since the last reset.
 * enable: 0 off; 1 every kernel class (~0.4 ms of event records per episode-batch of the bench workload: a breakdown
 * pass); 2 only the AUGRU recurrence, the dominant kernel (two records per forward: what a timed region can carry). */
int rl4rs_dien_set_profiling(rl4rs_dien* net, int enable);
int rl4rs_dien_kernel_count(void);
const char* rl4rs_dien_kernel_name(int which);
/* The kernel(s) THIS handle launches for class `which`, named as a rocprofv3 kernel trace shows them (they depend on the
 * scorer mode and the handle's kernel_opts; rl4rs_dien_kernel_name is the static class name).  NUL-terminated into buf[cap]. */
int rl4rs_dien_kernel_label(rl4rs_dien* net, int which, char* buf, int32_t cap);
int rl4rs_dien_profile_read(rl4rs_dien* net, int which, double* ms_total, int64_t* launches);
int rl4rs_dien_profile_reset(rl4rs_dien* net);

/* ------------------------------------------------------------------------------------------------
 * The reference's other simulator families behind the same 'simulator_obs' / 'simulator_reward' contract
 * (SlateRecEnv.get_model, rl4rs/env/slate.py:228-241: config['algo'] = 'dnn' | 'widedeep' | 'lstm'):
 *   DNN       rl4rs/nets/dnn.py:31-37       obs_dim 256
 *   WIDEDEEP  rl4rs/nets/widedeep.py:31-38  obs_dim 256 + hidden_units + category_feature_num * emb_size
 *   LSTM      rl4rs/nets/lstm.py:31-37      obs_dim 256 (keras GRU layers; needs emb_size == hidden_units == 128)
 * Same calling pattern as rl4rs_dien: `encode` caches the per-sequence feature of a cache slot (WIDEDEEP: mean of
 * the sequence embeddings, LSTM: final GRU state, DNN: nothing - that model never reads its sequences), `forward`
 * scores R rows whose groups of `group` consecutive rows share their slots.
 * Weight arrays (host float32, shapes in rl4rs_amd/nets/simnets.py); unused ones may be NULL.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rl4rs_simnet rl4rs_simnet;
enum { RL4RS_SIMNET_DNN = 1, RL4RS_SIMNET_WIDEDEEP = 2, RL4RS_SIMNET_LSTM = 3,
       RL4RS_SIMNET_ADVERSARIAL = 4 /* trainer only (rl4rs_simtrain_create_head with RL4RS_HEAD_ADVERSARIAL); no scorer */ };

typedef struct rl4rs_simnet_cfg {
    int32_t algo;                  /* RL4RS_SIMNET_* */
    int32_t maxlen;                /* 64  */
    int32_t emb_size;              /* 128 */
    int32_t hidden_units;          /* 128 */
    int32_t dense_feature_num;     /* 432 */
    int32_t category_feature_num;  /* 21  */
    int32_t category_hash_size;    /* 100000 */
    int32_t seq_num;               /* 2   */
    int32_t class_num;             /* 2   */
    int32_t max_rows;
    int32_t max_slots;
} rl4rs_simnet_cfg;

typedef struct rl4rs_simnet_weights {
    const float* cat_emb;
    const float* seq_emb;
    const float* dense_w1; const float* dense_b1;
    const float* dense_w2; const float* dense_b2;
    const float* fc_w; const float* fc_b;
    const float* obs_w; const float* obs_b;
    const float* out_w; const float* out_b;
    const float* cat_gru_kernel; const float* cat_gru_recurrent; const float* cat_gru_bias;
    const float* seq_gru_kernel[4]; const float* seq_gru_recurrent[4]; const float* seq_gru_bias[4];
} rl4rs_simnet_weights;

int rl4rs_simnet_create(const rl4rs_simnet_cfg* cfg, const rl4rs_simnet_weights* w, void* stream,
                        rl4rs_simnet** out);
int rl4rs_simnet_destroy(rl4rs_simnet* net);
int rl4rs_simnet_obs_dim(rl4rs_simnet* net, int32_t* dim);
/* ids_dev [n, maxlen] int32 -> cache slots [slot_base, slot_base + n) of sequence input s */
int rl4rs_simnet_encode(rl4rs_simnet* net, int32_t s, const int32_t* ids_dev, int32_t n, int32_t slot_base,
                        void* stream);
/* dense_dev [R, dense_feature_num] f32, cat_dev [R, category_feature_num] i32, slot_dev [seq_num, R/group] i32,
 * obs_dev [R, obs_dim] f32 (may be NULL), prob_dev [R] f32 = softmax('simulator_reward')[:, 1] (may be NULL) */
int rl4rs_simnet_forward(rl4rs_simnet* net, int32_t R, int32_t group, const float* dense_dev,
                         const int32_t* cat_dev, const int32_t* slot_dev, float* obs_dev, float* prob_dev,
                         void* stream);
/* softmax(obs @ out_w + out_b)[:, 1] of already computed 'simulator_obs' rows */
int rl4rs_simnet_head_prob(rl4rs_simnet* net, int32_t R, const float* obs_dev, float* prob_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One batched transition as ONE call: RecSimBase._step (rl4rs/env/base.py:157-170) = act -> obs_fn -> forward (reward
 * when due) -> done, for an env bound to its scorer.  Same kernels in the same order as calling rl4rs_env_act_* /
 * rl4rs_dien_forward / rl4rs_env_build_complete_rows / rl4rs_dien_head_prob / rl4rs_env_reward_split one by one
 * (bit-identical results); nothing is allocated, nothing synchronises inside.
 *   slots_dev  int32 [seq_num, batch_size]: cache slot of every env row per sequence input (caller-owned; the caller
 *              encodes the history sequences with rl4rs_dien_encode after every rl4rs_env_load_batch and keeps row 0
 *              current).  SeqSlate's second input (items of the previous pages, seqslate.py:107-108) is re-encoded here
 *              into slots [0, batch_size) on the first act of every page but the first; rows 1.. must then read
 *              0, 1, .., batch_size - 1.  On the first page of every episode it is the constant [0] and is NOT encoded
 *              here: the caller supplies it, either by encoding batch_size all-zero rows into slots [0, batch_size)
 *              after every rl4rs_env_load_batch, or (the Python wrapper's recipe) by encoding one all-zero row once into
 *              a spare slot (slot batch_size: the net needs max_slots >= batch_size + 1), pointing rows 1.. at it after
 *              every rl4rs_env_load_batch and writing 0 .. batch_size - 1 back before the first act of the second page
 *              (on the stream the steps run on).  Slate's second input is that constant [0] at every step
 *              (slate.py:77), supplied the same way.
 *   obs_dev    float32 [B, D]    'simulator_obs' of the new state (slate.py:265-267); D = 256 for the DIEN scorer,
 *              rl4rs_simnet_obs_dim() for an attached simnet (widedeep: 256 + hidden_units + Cn * emb_size)
 *   reward_dev float64 [B] (optional)  0 unless a reward is due (slate.py:283, seqslate.py:138)
 *   done_dev   uint8 [B] (optional)    1 once cur_steps (before the act) >= max_steps - 1 (base.py:165-168)
 *   mask_bits_dev uint32 [B, ceil(A/32)] (optional)  obs-side action mask of the NEXT slot (slate.py:92-97), packed as
 *              rl4rs_env_obs_mask dtype 4
 * ---------------------------------------------------------------------------------------------- */
typedef struct rl4rs_stepper rl4rs_stepper;
int rl4rs_env_attach_scorer(rl4rs_env* env, rl4rs_dien* net, const int32_t* slots_dev, int32_t seq_num,
                            rl4rs_stepper** out);
int rl4rs_env_attach_simnet(rl4rs_env* env, rl4rs_simnet* net, const int32_t* slots_dev, int32_t seq_num,
                            rl4rs_stepper** out);
int rl4rs_stepper_destroy(rl4rs_stepper* s);
int rl4rs_env_step_discrete(rl4rs_stepper* s, const int32_t* actions_dev, float* obs_dev, double* reward_dev,
                            uint8_t* done_dev, uint32_t* mask_bits_dev, void* stream);
/* rl4rs_env_step_discrete lets the act kernel write done_dev, the zero of reward_dev on a step on which no reward is due and the
 * logged item ids of the NEXT step (the rule of rl4rs_env_offline_action, past the horizon included) instead of launching a kernel
 * for the first two and leaving the third to a call between two steps.  rl4rs_stepper_next_offline_action: *step = the step whose
 * logged ids the last rl4rs_env_step_discrete wrote (-1: none - another kind of transition, or the option is off), *ids_dev =
 * int32 [B] device memory of the stepper holding them: a row of its own per step of an episode, rewritten by the same step of
 * the next one.  rl4rs_stepper_set_act_tail(s, 0): the launches as they were (k_step_tail, no next-step ids); bit-identical
 * outputs either way. */
int rl4rs_stepper_set_act_tail(rl4rs_stepper* s, int32_t on);
/* On a reward step of rl4rs_env_step_discrete / _conti with the DIEN scorer in fp16x2 mode (k_augru_x), the state row is scored
 * INSIDE the reward forward - one forward of n_complete rows per env that returns every row's probability and, through
 * rl4rs_dien_set_obs_last, the observation - instead of an observation forward followed by a forward of n_complete - 1 rows.
 * Taken only when that forward's k_augru_x launch runs 64-row workgroups (a batch large enough to fill the chip twice over, or the
 * form pinned) and needs no more rounds of workgroups over the chip than the smaller one, counted on
 * rl4rs_stepper_set_distinct_hint's number of envs the scorer's row dedup is expected to leave (default: the batch size; a
 * batch drawn with replacement passes its number of distinct log lines).  rl4rs_stepper_set_obs_fold(s, 0): the two-forward order
 * as it was; bit-identical outputs either way.  rl4rs_env_step_record* keep the two-forward order. */
int rl4rs_stepper_set_obs_fold(rl4rs_stepper* s, int32_t on);
int rl4rs_stepper_set_distinct_hint(rl4rs_stepper* s, int32_t n_distinct);
/* With the DIEN scorer and its row dedup on, rl4rs_env_step_* carry the duplicate-row partition of the env batch from one forward
 * of an episode to the next instead of letting every forward compare whole rows: two envs whose state rows were equal are equal
 * now iff they have just taken the same (resolved) action, so the act kernel refines the partition by one integer per env and the
 * forwards of the transition take it through rl4rs_dien_set_row_partition.  Seeded by the scorer's last content dedup when that
 * ran on exactly the env's current state rows (the reset observation forward); dropped - the next forward compares rows again -
 * by a reset, by any other call that writes the env's rows, by the first act of a SeqSlate page (the slot table changes) and by
 * a changed row order.  The slot table and the row order must not be rewritten in place between two steps of an episode.
 * Outputs are bit-identical either way.  rl4rs_stepper_set_partition_carry(s, 0): every forward launches k_row_dedup as before. */
int rl4rs_stepper_set_partition_carry(rl4rs_stepper* s, int32_t on);
/* Consecutive transitions on two streams (default on).  A transition of rl4rs_env_step_discrete that scores with the DIEN
 * on its k_augru_x path, carries the partition, has no reward due, asks for neither done_dev nor mask_bits_dev and whose
 * observation-sized launch leaves half of the chip free (2 * seq_num * ceil(distinct hint / 32) <= CUs) runs on one of two streams
 * of the stepper, in turn: its act waits for the previous transition's ACT only, so its forward runs beside the previous forward
 * when the caller hands back the logged-action row it was given (rl4rs_stepper_next_offline_action); any other action makes it
 * wait for the caller's stream first.  obs_dev / reward_dev are filled on the caller's stream, behind the lane's last launch:
 * what the caller sees on its stream is what it saw before, bit for bit.  Every other entry point of the stepper, its env and its
 * scorer first lets the stream it is given wait for both lanes (those that are given none: the host waits).
 * rl4rs_stepper_set_step_overlap(s, 0): every call runs on the caller's stream with the launches it had.
 * Cost: a stepper on a DIEN owns two streams, four events and 2 * B * 1032 bytes of device memory for its life, its scorer a second
 * scratch set of about 6 KB per env (reserved once per batch size, freed with the scorer).  Env, scorer and stepper may be destroyed
 * in any order. */
int rl4rs_stepper_set_step_overlap(rl4rs_stepper* s, int32_t on);
/* Lane transitions issued on each lane and joins carried out since the stepper was created (read-only; any pointer may be NULL). */
int rl4rs_stepper_lane_stats(const rl4rs_stepper* s, int64_t* lane0, int64_t* lane1, int64_t* joins);
/* The two ends of an episode on the same two lanes (default on where the step overlap is).
 * rl4rs_stepper_observe: the observation of the state behind a reset (cur_steps == 0) as a lane transition without an act.  Under the
 * rule of rl4rs_stepper_set_step_overlap (less the act's conditions) the scorer forward runs on a lane behind everything the caller's
 * stream holds, obs_dev [B, 256] is filled on the caller's stream, the logged action of step 0 is written to the row
 * rl4rs_stepper_next_offline_action then returns (step 0) and *taken = 1: a first transition that hands that row back starts beside
 * this forward.  *taken = 0: the rule says no, nothing was enqueued - compose the observation with rl4rs_dien_forward as before.
 * A reward step that scores the state row inside the reward forward (rl4rs_stepper_set_obs_fold) runs on lane 0 when the
 * transition before it is in flight on lane 1 (the scorer's second scratch set holds B rows only; the lane of the first transition
 * behind a join is chosen so that this is the case) and joins otherwise; its front kernels run beside that transition, its AUGRU
 * launch waits for that transition's last kernel (whole rounds over every CU).  rl4rs_stepper_set_reset_lane(s, 0) /
 * rl4rs_stepper_set_reward_lane(s, 0) turn each half off alone; rl4rs_stepper_set_step_overlap(s, 0) turns off both.
 * rl4rs_stepper_lane_stats_ex: reset forwards and reward steps issued on a lane (rl4rs_stepper_lane_stats counts neither). */
int rl4rs_stepper_observe(rl4rs_stepper* s, float* obs_dev, int32_t* taken, void* stream);
int rl4rs_stepper_set_reset_lane(rl4rs_stepper* s, int32_t on);
int rl4rs_stepper_set_reward_lane(rl4rs_stepper* s, int32_t on);
int rl4rs_stepper_lane_stats_ex(const rl4rs_stepper* s, int64_t* reset_runs, int64_t* reward_runs);
/* Replay-ahead (default on with a DIEN scorer).  When rl4rs_env_step_discrete of a Slate env is handed the stepper's own
 * logged-action row (rl4rs_stepper_next_offline_action) at act index c0 with n = max_steps - 1 - c0 equal to 8 or 9, neither done_dev
 * nor mask_bits_dev, and a forward of n rows per env runs the 64-row form of k_augru_x - by the automatic rule (on = 1, the default:
 * enough workgroups to fill the chip twice over) or also by the pin (on = 2; on = 0: never) -, the observation rows of the transitions
 * c0 .. max_steps - 2 under the logged actions are scored in ONE forward; every later transition that hands back the stepper's row again
 * runs its act alone and receives its row (and the zero reward).  Any other call - a foreign action pointer, another entry point of
 * the env, the scorer or the stepper, a reset - drops the rows not handed out yet and proceeds as without the switch: wasted work, the
 * same results.  rl4rs_stepper_replay_stats: forwards started, rows per env handed out, rows per env dropped, since attach. */
int rl4rs_stepper_set_replay_ahead(rl4rs_stepper* s, int32_t on);
/* The rows that forward scores, on their own (Slate envs, behind at least one act): row k of env b (out row b * n + k) is the state
 * row the act of step c0 + k builds when the env plays its logged actions from c0 + 1 on, c0 = cur_steps - 1 the act just taken;
 * dense_out [B * n, dense_feature_num] f32, cat_out [B * n, category_feature_num] i32, c0 + n <= max_steps.  Env state is not touched.
 * rep != NULL: the duplicate-row partition of the envs behind the act just taken (rep [B] with rep[rep[b]] == rep[b], active
 * [n_active[0]] the representatives, as rl4rs_dien_set_row_partition takes them) is copied to rep_out [B] / active_out [B] /
 * n_active_out [1] for a forward of these rows: an env whose logged actions c0 + 1 .. c0 + n - 1 differ from its representative's is
 * its own representative in the copy, appended to active_out behind the copied entries (in no fixed order) and counted. */
int rl4rs_env_build_ahead_rows(rl4rs_env* e, int32_t n, float* dense_out, int32_t* cat_out, const int32_t* rep, const int32_t* active,
                               const int32_t* n_active, int32_t* rep_out, int32_t* active_out, int32_t* n_active_out, void* stream);
int rl4rs_stepper_replay_stats(const rl4rs_stepper* s, int64_t* started, int64_t* handed, int64_t* dropped);
/* The reward step beside the replay-ahead forward (default on where the step overlap is).  The first transition that may
 * start a replay-ahead forward on the lanes also grows the scorer's second scratch set to B * n_complete rows (reserved once, freed with
 * the scorer; no memory for it: the switch stays off for good and nothing fails).  A folded reward step that rl4rs_stepper_set_reward_lane
 * would run on lane 0 then runs on lane 1 and that set when the forward in flight on lane 0 is a replay-ahead forward nothing has
 * joined since: its act, row builder and front kernels no longer wait for that forward, its AUGRU launch still does.  Same kernels, same
 * arguments but for the scratch pointers, same results.  on = 0: that reward step runs on lane 0 behind the forward, as it did.
 * rl4rs_stepper_reward_beside_stats: reward steps that took lane 1 since attach, and the bytes the scorer's second scratch set holds
 * now (read-only; either pointer may be NULL). */
int rl4rs_stepper_set_reward_beside(rl4rs_stepper* s, int32_t on);
int rl4rs_stepper_reward_beside_stats(const rl4rs_stepper* s, int64_t* ran, int64_t* scratch_bytes);
/* Click probabilities of the complete-state rows of the LAST reward step, slate order: out_dev [B, n_complete] f32 - the same
 * numbers in either order of the forwards (the record form's click_p part, for rl4rs_env_step_discrete / _conti). */
int rl4rs_stepper_click_probs(rl4rs_stepper* s, float* out_dev, void* stream);
/* Rows per env the reward forward of the last reward step scored: n_complete (the state row inside it), n_complete - 1 (the
 * two-forward order), 0 before the first reward step. */
int rl4rs_stepper_reward_rows(const rl4rs_stepper* s);
int rl4rs_stepper_next_offline_action(rl4rs_stepper* s, const int32_t** ids_dev, int32_t* step);
/* continuous actions: [B, action_emb_size] float32 / float64 resolved by the masked float64 K-NN first (slate.py:187-197);
 * chosen_dev (optional) receives the item ids played */
int rl4rs_env_step_conti(rl4rs_stepper* s, const void* actions_dev, int is_f64, int32_t* chosen_dev, float* obs_dev,
                         double* reward_dev, uint8_t* done_dev, uint32_t* mask_bits_dev, void* stream);

/* Reference-shaped form of the same transition (RecEnvBase.step hands lists / ndarrays to the caller, base.py:256-263,
 * slate.py:244-279): every output a host-returning caller needs is written into ONE device record, host-visible part first,
 * so the facade brings a whole transition back with a single device-to-host copy into pinned memory and ONE wait.
 * `want` selects the optional parts; offsets are bytes from the start of the record, -1 = absent; all parts 64-byte aligned.
 *   status          int32 [2]: [0] sticky bad-action flag of the env (RL4RS_BUF_ERROR_FLAG), [1] the scorer's fp16-range status
 *                   (RL4RS_DIEN_STATUS_FP16_RANGE; read and cleared)
 *   reward          float64 [B]                      done   uint8 [B]          chosen   int32 [B] item ids played
 *   obs             float32 [B, obs_dim]             'simulator_obs'  (behind host_bytes when D3RL_OBS is wanted)
 *   obs_d3rl        float64 [B, obs_dim + cols + 1]  support_d3rl_mask observation: obs | masked_actions | cur_steps
 *                   (slate.py:270-277; cols = max_steps, or page_items for SeqSlate: seqslate.py:18-23)
 *   mask_i64        int64 [B, action_size]           support_rllib_mask observation-side mask (slate.py:90-97)
 *   mask_bits       uint32 [B, ceil(A/32)]           the same mask packed
 *   click_p         float32 [B, n_complete]          simulator_info_fetch (slate.py:299-301); written on reward steps only
 *   offline_action  int32 [B] (discrete) / float64 [B, action_emb_size] (continuous): the logged action of the NEXT step
 *                   (slate.py:152-161); written while a next step exists
 * host_bytes: length of the prefix a host caller copies; total_bytes: size of the record buffer to allocate. */
enum {
    RL4RS_STEP_WANT_MASK_I64 = 1, RL4RS_STEP_WANT_MASK_BITS = 2, RL4RS_STEP_WANT_D3RL_OBS = 4, RL4RS_STEP_WANT_CLICK_P = 8,
    RL4RS_STEP_WANT_OFFLINE_ACTION = 16, RL4RS_STEP_WANT_ALL = 31
};
typedef struct rl4rs_step_record {
    int64_t status, reward, done, chosen, obs, obs_d3rl, mask_i64, mask_bits, click_p, offline_action;
    int64_t host_bytes, total_bytes;
    int32_t obs_dim, d3rl_cols;
} rl4rs_step_record;
int rl4rs_stepper_record_layout(rl4rs_stepper* s, uint32_t want, int32_t conti, rl4rs_step_record* out);
/* action_kind: 0 = int32 item ids [B]; 1 / 2 = float32 / float64 action embeddings [B, action_emb_size] (masked K-NN first) */
int rl4rs_env_step_record(rl4rs_stepper* s, const void* actions_dev, int32_t action_kind, uint32_t want, void* record_dev,
                          void* stream);
/* The same transition, and the record's host part brought home by the library: `record_host` = host_bytes of (pinned) host
 * memory, filled when `stream` has drained - ONE wait on `stream` by the caller.  The int64 mask (the bulk of a
 * support_rllib_mask record, B * action_size * 8 bytes, and a function of the act alone) leaves on a copy stream of the
 * stepper as soon as the act is done, beside the scorer's kernels; on a reward step the observation follows it as soon as the
 * observation forward is done, beside the reward forward; the rest is copied on `stream` after the last kernel. */
int rl4rs_env_step_record_host(rl4rs_stepper* s, const void* actions_dev, int32_t action_kind, uint32_t want, void* record_dev,
                               void* record_host, void* stream);
/* The record of the state the env is IN, without a transition - what RecSimBase.sample returns right after a reset
 * (base.py:172-175: obs_fn(samples.state)): obs / obs_d3rl / mask_i64 / mask_bits / offline_action (the logged action of the
 * CURRENT step) / status in the same layout (`conti` selects the offline_action form); reward, done and chosen are left alone.
 * The caller has encoded the batch's sequences (rl4rs_dien_encode).  record_host may be NULL (no copies). */
int rl4rs_env_observe_record_host(rl4rs_stepper* s, int32_t conti, uint32_t want, void* record_dev, void* record_host,
                                  void* stream);
/* On steps without a reward forward (and on resets) the float32 observation reaches `record_host` from the epilogue of the head
 * GEMM itself (device-visible pinned memory: hipHostGetDevicePointer must succeed on record_host, else the copy engine serves it
 * as before) - the copy would otherwise start only when the GPU has nothing left to run.  Process-wide switch, default 0: on the
 * boxes measured the mirror is no faster than the copy engine (13.2 against 13.1 ms per episode-batch); kept for A/B
 * measurements.  Replaces nothing in the reference (its observations never leave host memory: rl4rs/env/slate.py:244-279). */
int rl4rs_set_host_mirror(int32_t on);

/* ------------------------------------------------------------------------------------------------
 * Action-masked policy net: rl4rs/nets/rllib/rllib_mask_model.py:7-64 (FC obs->hidden(tanh)->action_size
 * logits, value head on the shared hidden layer, logits + max(log(action_mask), float32.min)).
 * Parameters, gradients and Adam state are ONE flat float32 buffer each:
 *   [ W1 (obs_dim x hidden) | b1 (hidden) | W2e (hidden x (action_size+1)) | b2e (action_size+1) ]
 * (column action_size of layer 2 is the value head), so a data-parallel trainer all-reduces one buffer.
 * mask_bits_dev: uint32 [N, ceil(action_size/32)] bit rows in the layout of RL4RS_BUF_ACTION_MASK, or NULL.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rl4rs_policy rl4rs_policy;

int rl4rs_policy_param_count(int32_t obs_dim, int32_t hidden, int32_t action_size);
/* Limits: obs_dim > 0, 0 < hidden <= 1024, action_size > 1, and 16 * (obs_dim + hidden + 2 * (action_size + 1)) bytes <= 160 KB,
 * the LDS of one workgroup that the one-wave training kernel needs (obs_dim 256 / hidden 64: action_size <= 4959); create refuses
 * other shapes.  The tiled kernels (hidden % 64 == 0, hidden / 32 in {2, 4, 8}, obs_dim % 32 == 0, ...) run an entry point only
 * where their own LDS for it fits too; elsewhere the one-wave kernels do. */
int rl4rs_policy_create(int32_t obs_dim, int32_t hidden, int32_t action_size, int32_t max_rows,
                        const float* params_host, void* stream, rl4rs_policy** out);
int rl4rs_policy_destroy(rl4rs_policy* pol);
/* device pointer of the flat parameter buffer (owned by the handle) */
int rl4rs_policy_params(rl4rs_policy* pol, float** params_dev, int32_t* count);

/* Sample actions ~ Categorical(softmax(masked logits)) by Gumbel-max with a counter-based RNG keyed on
 * (seed, step, row, action); outputs (each may be NULL except actions): log-prob of the draw, value, entropy,
 * masked logits [N, action_size]. */
int rl4rs_policy_act(rl4rs_policy* pol, int32_t N, const float* obs_dev, const uint32_t* mask_bits_dev,
                     uint32_t seed, uint32_t step, int32_t* actions_dev, float* logp_dev, float* value_dev,
                     float* entropy_dev, float* logits_dev, void* stream);
/* Same forward for GIVEN actions (no sampling). */
int rl4rs_policy_evaluate(rl4rs_policy* pol, int32_t N, const float* obs_dev, const uint32_t* mask_bits_dev,
                          const int32_t* actions_dev, float* logp_dev, float* value_dev, float* entropy_dev,
                          float* logits_dev, void* stream);

/* Loss + gradient over N samples into grad_dev (flat, same layout as the parameters).
 *   algo 0 = A2C (RLlib a3c_tf_policy: -sum(logp*adv) + vf_coeff*0.5*sum((V-R)^2) - ent_coeff*sum(H))
 *   algo 1 = PPO (RLlib ppo_tf_policy: mean(-min(adv*r, adv*clip(r,1-c,1+c)) + kl_coeff*KL(old||new)
 *                 + vf_coeff*max((V-R)^2, (Vclip-R)^2) - ent_coeff*H)); needs old_logp / old_value / old_logits
 * stats_dev (optional) float[4] = sums over samples of {policy loss, value loss, entropy, kl}.
 * Gradients are bit-reproducible (fixed sample chunks, fixed summation order). */
int rl4rs_policy_loss_grad(rl4rs_policy* pol, int32_t algo, int32_t N, const float* obs_dev,
                           const uint32_t* mask_bits_dev, const int32_t* actions_dev, const float* adv_dev,
                           const float* ret_dev, const float* old_logp_dev, const float* old_value_dev,
                           const float* old_logits_dev, float vf_coeff, float ent_coeff, float clip,
                           float vf_clip, float kl_coeff, float* grad_dev, float* stats_dev, void* stream);
/* Adam update of the handle's parameters from grad_dev (tf.train.AdamOptimizer form); grad_clip > 0 applies
 * tf.clip_by_global_norm first. */
int rl4rs_policy_adam_step(rl4rs_policy* pol, const float* grad_dev, float lr, float beta1, float beta2,
                           float eps, float grad_clip, void* stream);
/* One PPO SGD pass over N already shuffled samples in minibatches of `minibatch` consecutive rows (loss + backward
 * + Adam per minibatch; the trailing N % minibatch rows are dropped).  Identical arithmetic to
 * rl4rs_policy_loss_grad(algo 1) + rl4rs_policy_adam_step per minibatch, one host call (one persistent kernel when the
 * shapes fit and its grid can be co-resident on this device, checked against the runtime's occupancy answer).
 * stats_dev (optional) float[8]: [0..3] = sums of {policy loss, value loss, entropy, kl} over the LAST minibatch,
 * [4..7] = the same sums over every sample of the pass (RLlib reports the pass-mean KL and feeds it to its adaptive
 * kl_coeff rule: script/modelfree_train.py:189 kl_coeff, :216 kl_target). */
int rl4rs_policy_ppo_epoch(rl4rs_policy* pol, int32_t N, int32_t minibatch, const float* obs_dev,
                           const uint32_t* mask_bits_dev, const int32_t* actions_dev, const float* adv_dev,
                           const float* ret_dev, const float* old_logp_dev, const float* old_value_dev,
                           const float* old_logits_dev, float vf_coeff, float ent_coeff, float clip, float vf_clip,
                           float kl_coeff, float lr, float beta1, float beta2, float eps, float grad_clip,
                           float* grad_dev, float* stats_dev, void* stream);
/* Data-parallel form of the pass (gradient all-reduce only): the PPO gradient of minibatch `mb_index`
 * (rows [mb_index*minibatch, (mb_index+1)*minibatch) of the N shuffled samples) into grad_dev WITHOUT updating the
 * parameters.  Each rank calls it on its own shard, mean-all-reduces grad_dev and applies rl4rs_policy_adam_step.
 * stats_dev (optional) float[4] = sums over the minibatch. */
int rl4rs_policy_ppo_minibatch_grad(rl4rs_policy* pol, int32_t N, int32_t minibatch, int32_t mb_index,
                                    const float* obs_dev, const uint32_t* mask_bits_dev, const int32_t* actions_dev,
                                    const float* adv_dev, const float* ret_dev, const float* old_logp_dev,
                                    const float* old_value_dev, const float* old_logits_dev, float vf_coeff,
                                    float ent_coeff, float clip, float vf_clip, float kl_coeff, float* grad_dev,
                                    float* stats_dev, void* stream);
/* Status bits since the last call (synchronises `stream`, then clears them).  RL4RS_POLICY_STATUS_PASS_TIMEOUT: a grid
 * barrier of a persistent PPO pass timed out (workgroups not co-resident: another process holds compute units); the pass
 * stopped at the last completed minibatch and is incomplete. */
enum { RL4RS_POLICY_STATUS_PASS_TIMEOUT = 1 };
int rl4rs_policy_status(rl4rs_policy* pol, int32_t* flags, void* stream);
/* The same status word without a synchronisation: device pointer to 2 x uint32 owned by the handle, word [1] != 0 <=> a
 * persistent pass timed out.  A training loop copies it asynchronously together with its loss statistics and looks at it one
 * iteration later (rl4rs_amd/train.py), so that validating every pass costs no pipeline drain. */
int rl4rs_policy_status_words(rl4rs_policy* pol, uint32_t** words_dev);
/* Once a pass has timed out, rl4rs_policy_ppo_epoch / rl4rs_policy_ppo_minibatch_grad return RL4RS_ESTATE (nothing is
 * launched, the Adam step counter does not advance) until rl4rs_policy_status has reported and cleared the condition: the
 * kernel raises a pinned host word next to the device flag, which the launch path reads without synchronising.
 *
 * Kernel-path selection of ONE handle, for A/B measurements and tests (defaults in brackets):
 *   TILE          [1] 0 = one-wave-per-sample forward / loss kernels instead of k_policy_tile
 *   PPO_FUSED     [1] 0 = per-minibatch kernel chain instead of the persistent k_ppo_pass
 *   PPO_ROWS      [0 = automatic] samples per workgroup of k_ppo_pass: 8, 16 or 32 pin the all-runtime instantiation's (automatic: 8);
 *                     where the compile-time instantiation applies: 4 or 8 (automatic: 4 while MB / 4 <= 126 workgroups, else 8)
 *   RESIDENT_WGS [-1] >= 0: pretend the device holds only this many workgroups of k_ppo_pass at once (co-residency tests)
 *   PPO_STD       [1] 0 = the all-runtime instantiation of k_ppo_pass even at the default shape (256 -> 64 -> 284 + 1, 8 rows,
 *                     minibatch % 256 == 0), which otherwise runs the compile-time one (bit-identical results) */
enum { RL4RS_POLICY_OPT_TILE = 0, RL4RS_POLICY_OPT_PPO_FUSED = 1, RL4RS_POLICY_OPT_PPO_ROWS = 2, RL4RS_POLICY_OPT_RESIDENT_WGS = 3,
       RL4RS_POLICY_OPT_PPO_STD = 4 };
int rl4rs_policy_set_option(rl4rs_policy* pol, int32_t which, int32_t value);
/* Adam state of the handle (first / second moments, device pointers owned by the handle; same layout as the
 * parameters) and its step counter: a data-parallel trainer broadcasts rank 0's at start, a checkpoint saves them. */
int rl4rs_policy_adam_state(rl4rs_policy* pol, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_policy_set_adam_step(rl4rs_policy* pol, int64_t step);

/* ------------------------------------------------------------------------------------------------
 * On-device DQN on the action-masked net: script/modelfree_train.py:106-133 (algo "DQN": hiddens [], dueling False,
 * double_q True, n_step 1, target_network_update_freq 200, buffer_size 100000, custom_model mask_model).  With those settings the
 * Q values are the masked logits of rl4rs_policy, and RLlib's SoftQ exploration (temperature 1) is rl4rs_policy_act's draw.
 * RLlib 1.5.1's dqn_tf_policy and PrioritizedReplayBuffer are restated from their published form (ray is absent: parity unpinned).
 *
 * Replay memory (replaces ray's PrioritizedReplayBuffer behind modelfree_train.py:121 buffer_size): a ring of WHOLE rollouts in
 * the trainers' row order (r * T + t) * B + b.  A row holds obs float32 [obs_dim], packed mask words, action int32, reward float32,
 * done int32 and priority float64; the successor of a non-terminal row is row idx + B of the same rollout, so no next_obs is
 * stored.  Capacity is max(1, buffer_size / (T * B)) rollouts and the oldest rollout is evicted whole: the one deviation from
 * RLlib's per-timestep ring.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rl4rs_replay rl4rs_replay;

/* alpha: the priority exponent (RLlib prioritized_replay_alpha 0.6) */
int rl4rs_replay_create(int32_t obs_dim, int32_t action_size, int32_t max_steps, int32_t batch_size, int64_t buffer_size,
                        double alpha, rl4rs_replay** out);
int rl4rs_replay_destroy(rl4rs_replay* h);
/* filled rows n (always rows [0, n) of the buffers), capacity in rows, rollouts pushed so far; any may be NULL */
int rl4rs_replay_rows(rl4rs_replay* h, int32_t* rows, int32_t* capacity_rows, int64_t* pushes);
/* device address and element count of one column of the ring (tests, checkpoints) */
enum { RL4RS_REPLAY_BUF_OBS = 0, RL4RS_REPLAY_BUF_MASK = 1, RL4RS_REPLAY_BUF_ACTION = 2, RL4RS_REPLAY_BUF_REWARD = 3,
       RL4RS_REPLAY_BUF_DONE = 4, RL4RS_REPLAY_BUF_PRIORITY = 5, RL4RS_REPLAY_BUF_MAX_PRIORITY = 6,
       RL4RS_REPLAY_BUF_ACTION_F32 = 7 /* continuous ring only; MASK and ACTION are the discrete ring's */ };
int rl4rs_replay_buffer(rl4rs_replay* h, int32_t which, void** dev_out, int64_t* count_out);
/* Append one rollout (T * B rows in row order t * B + b) from device pointers, no host round trip: obs float32, mask words,
 * actions int32, rewards float64 (what the env returns; stored as float32).  done = (t == T - 1).  New rows get priority
 * max_priority ^ alpha; max_priority starts at 1.0 and is the largest |td| + 1e-6 ever set.
 * The obs column is, by contract, OPAQUE 32-bit words: push (a device-to-device copy) and sample (a word gather, on its 16-byte
 * path and on its scalar path alike) move them and do no arithmetic on them.  A ring created with obs_dim = REC therefore keeps
 * packed raw-state records (rl4rs_rawstate_pack) bit for bit, although their int32 ids read as float32 are denormals (small ids)
 * or NaNs (negative ids). */
int rl4rs_replay_push(rl4rs_replay* h, const float* obs_dev, const uint32_t* mask_bits_dev, const int32_t* action_dev,
                      const double* reward_dev, void* stream);
/* Draw M rows and gather them into contiguous minibatch buffers: obs / next obs float32 [M, obs_dim], next mask words [M, W],
 * action int32, reward float32, done int32, idx int32 (row in the ring), weight float32 (optional) and u float32 (optional: the
 * uniform variate of each draw = the policy net's counter RNG keyed (seed, step, draw, 0)).
 *   prioritized 0: idx = floor(u * n), weight 1.
 *   prioritized 1: RLlib's proportional buffer, not stratified: idx = the smallest i whose inclusive float64 prefix sum of the
 *     priorities exceeds u * total; weight = (n p_i / total)^-beta / (n p_min / total)^-beta.  Prefix sums, total and minimum are
 *     float64 reductions in a fixed order (per 1024-row tile, then over the tiles in order): bit-identical from run to run.
 * Next obs / next mask of a terminal row are a copy of the row itself (finite, never to be used). */
int rl4rs_replay_sample(rl4rs_replay* h, int32_t M, int32_t prioritized, double beta, uint32_t seed, uint32_t step,
                        float* obs_out, float* next_obs_out, uint32_t* next_mask_out, int32_t* action_out, float* reward_out,
                        int32_t* done_out, int32_t* idx_out, float* weight_out, float* u_out, void* stream);
/* priority[idx_i] = (|td_i| + 1e-6)^alpha; where idx repeats within the batch the HIGHEST batch position wins (deterministic);
 * max_priority = max(max_priority, |td_i| + 1e-6) over the whole batch.  A non-finite td leaves its row alone. */
int rl4rs_replay_update_priorities(rl4rs_replay* h, int32_t M, const int32_t* idx_dev, const float* td_dev, void* stream);
/* The same ring for the continuous-action env (support_conti_env: the action is a float32 vector of act_dim values in Box(-1, 1),
 * rl4rs/env/base.py:214-215): the same handle type, row order, successor rule, whole-rollout eviction, scans, draw rule and
 * rl4rs_replay_rows / _buffer / _update_priorities / _destroy; a row holds obs, action float32 [act_dim]
 * (RL4RS_REPLAY_BUF_ACTION_F32), reward, done and priority, and no mask words.  push_conti: obs float32, action float32
 * [T * B, act_dim], reward float64.  sample_conti: obs / next obs float32 [M, obs_dim], action float32 [M, act_dim], reward, done,
 * idx, weight (optional), u (optional).  The discrete push / sample on a continuous ring, or the reverse, is refused. */
int rl4rs_replay_create_conti(int32_t obs_dim, int32_t act_dim, int32_t max_steps, int32_t batch_size, int64_t buffer_size,
                              double alpha, rl4rs_replay** out);
int rl4rs_replay_push_conti(rl4rs_replay* h, const float* obs_dev, const float* action_dev, const double* reward_dev, void* stream);
int rl4rs_replay_sample_conti(rl4rs_replay* h, int32_t M, int32_t prioritized, double beta, uint32_t seed, uint32_t step,
                              float* obs_out, float* next_obs_out, float* action_out, float* reward_out, int32_t* done_out,
                              int32_t* idx_out, float* weight_out, float* u_out, void* stream);

/* DQN loss and gradient on the net of `pol` (replaces ray's dqn_tf_policy build_q_losses behind modelfree_train.py:106-133);
 * target_params_dev: the target net's parameters, a device buffer in the same flat layout.
 *   Q(s)[a] from the online net (a was legal: its mask term is 0)
 *   a* = first maximum of the masked online Q(s') (double_q 1) or of the masked target Q(s') (double_q 0)
 *   y  = r + gamma * Q_target(s')[a*] for a non-terminal row, r for a terminal one: a select, so nothing of a terminal row's
 *        successor (which may hold anything, NaN included) reaches the result
 *   td = Q(s)[a] - y,  loss = mean(w * huber(td, delta 1)),  w = weights_dev or 1
 * A NON-terminal row whose successor allows no action at all bootstraps nothing either: y = r, like a terminal row (every
 * Q(s') of it is the mask's -3.4e38, not a value).
 * Outputs: grad_dev (flat layout; the value-head column and every action nobody took get exactly 0), td_dev [N] for the
 * priority update, next_action_dev [N] (optional: a*, -1 for terminal rows), stats_dev float[4] (optional) = sums of
 * {w * huber, Q(s)[a], y, |td|}.  N <= max_rows; the first call allocates the loss's scratch on the handle.
 * Rank-sparse backward: one non-zero d loss / d Q per row, so dW2e is gathered column by column and the s' forwards are never
 * differentiated.  Bit-reproducible like rl4rs_policy_loss_grad (fixed sample chunks, fixed summation order).  The forwards
 * run as MFMA GEMMs for every shape rl4rs_policy_create admits; RL4RS_POLICY_OPT_TILE = 0 selects the one-wave-per-row kernel. */
int rl4rs_policy_dqn_loss_grad(rl4rs_policy* pol, const float* target_params_dev, int32_t N, const float* obs_dev,
                               const int32_t* actions_dev, const float* rewards_dev, const int32_t* dones_dev,
                               const float* next_obs_dev, const uint32_t* next_mask_bits_dev, const float* weights_dev,
                               float gamma, int32_t double_q, float* grad_dev, float* td_dev, int32_t* next_action_dev,
                               float* stats_dev, void* stream);
/* Greedy action (RLlib explore: False): the first maximum of the masked Q row; q_dev (optional) receives the masked row
 * [N, action_size].  A row that allows nothing returns action 0. */
int rl4rs_policy_greedy(rl4rs_policy* pol, int32_t N, const float* obs_dev, const uint32_t* mask_bits_dev,
                        int32_t* actions_dev, float* q_dev, void* stream);
/* forward exactly as rl4rs_policy_greedy's GEMM path (q_mode 1: the A logit columns; q_mode 0: all A + 1, column A = the value head),
 * then rl4rs_ope_greedy_rows on the handle's own [N, A + 1] buffer: q_mode 1 -> q = masked Q of the chosen action (DQN),
 * q_mode 0 -> q = V(s) (A2C / PPO / PG / IMPALA: 'vf_preds').  N <= max_rows; any shape rl4rs_policy_create admits. */
int rl4rs_policy_ope_step(rl4rs_policy* pol, int32_t N, const float* obs_dev, const uint32_t* mask_bits_dev, const int32_t* logged_dev,
                          int32_t q_mode, int32_t* actions_dev, double* pi_dev, double* q_dev, float* masked_out_dev, void* stream);
/* rl4rs_policy_adam_step with tf.clip_by_norm applied to EACH variable (W1, b1, W2e, b2e) by its own norm - RLlib DQN's
 * minimize_and_clip (grad_clip 40) - instead of the global norm; var_clip <= 0: no clipping. */
int rl4rs_policy_adam_step_clip_by_var(rl4rs_policy* pol, const float* grad_dev, float lr, float beta1, float beta2,
                                       float eps, float var_clip, void* stream);

/* ------------------------------------------------------------------------------------------------
 * On-device Rainbow: script/modelfree_train.py:50-53,146-178 (algo "RAINBOW": num_atoms 8 over [v_min 0, v_max 1000] on RLlib
 * 1.5.1's DQN defaults - dueling, double_q, n_step 3, gamma 1, no custom model, support_rllib_mask forced False).  RLlib's
 * dqn_tf_policy / distributional_q_tf_model are restated from their published form (ray is absent: parity unpinned).
 *
 * Network (RLlib's default model): obs -> Dense(trunk, tanh) -> Dense(trunk, tanh); advantage stream Dense(stream_hidden, relu) ->
 * Dense(A * atoms) with column a * atoms + j; value stream (dueling) Dense(stream_hidden, relu) -> Dense(atoms);
 *   logits[a, j] = V[j] + Adv[a, j] - mean_a' Adv[a', j]   (dueling 0: logits = Adv)
 *   p[a, :] = softmax_j logits[a, :],  z_j = v_min + j (v_max - v_min) / (atoms - 1),  Q[a] = sum_j z_j p[a, j]
 * Flat fp32 layout: W1, b1, W2, b2, Wa1, ba1, Wa2, ba2 [, Wv1, bv1, Wv2, bv2], every matrix [in, out] row-major.
 * The [rows, A * atoms] logits are never written to memory: acting and the double-Q argmax run one fused head kernel (fp32 MFMA
 * GEMM, dueling centring through the action-mean of Wa2, softmax over atoms, sum z p, then the draw or the first maximum), and an
 * update touches the logits of one action per row only.
 * Two deviations from the reference: the replay ring holds whole rollouts (above), and an OPTIONAL packed action mask (NULL = the
 * reference's unmasked behaviour) sets a disallowed action's Q to -3.4028235e38 before the draw / the maximum; the logits are not
 * altered.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rl4rs_distq rl4rs_distq;
typedef struct rl4rs_distq_cfg {
    int32_t obs_dim, action_size /* 2..512 */, atoms /* 2..64 */, trunk /* % 32 == 0 */, stream_hidden /* % 32 == 0, <= 256 */,
        dueling /* 0 / 1 */;
    float v_min, v_max;
    int32_t max_rows;                     /* most rows of one act / greedy / loss_grad call */
} rl4rs_distq_cfg;
/* floats of the flat layout, -1 for a config rl4rs_distq_create refuses */
int64_t rl4rs_distq_param_count(const rl4rs_distq_cfg* cfg);
int rl4rs_distq_create(const rl4rs_distq_cfg* cfg, const float* params_host, void* stream, rl4rs_distq** out);
int rl4rs_distq_destroy(rl4rs_distq* net);
/* device pointers owned by the handle (any may be NULL); like rl4rs_amlp_params / _copy_params / _adam_state */
int rl4rs_distq_params(rl4rs_distq* net, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_distq_copy_params(rl4rs_distq* dst, const rl4rs_distq* src, void* stream);
int rl4rs_distq_adam_state(rl4rs_distq* net, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_distq_set_adam_step(rl4rs_distq* net, int64_t step);
/* SoftQ exploration (RLlib's default for DQN): a draw from softmax(Q / temperature) over the allowed actions by inverse CDF,
 * action = the smallest a whose inclusive prefix sum of exp((Q - max Q) / temperature), in action order, exceeds u * total, with
 * u = the policy net's counter RNG keyed (seed, step, row, 0).  u_out [N], q_out [N, A] (masked Q) are optional.  A row whose mask
 * allows nothing returns action 0. */
int rl4rs_distq_act(rl4rs_distq* net, int32_t N, const float* obs_dev, const uint32_t* mask_bits_dev, float temperature, uint32_t seed,
                    uint32_t step, int32_t* actions_dev, float* u_out_dev, float* q_out_dev, void* stream);
/* Greedy action (explore: False): the first maximum of the masked Q row; a row that allows nothing returns 0. */
int rl4rs_distq_greedy(rl4rs_distq* net, int32_t N, const float* obs_dev, const uint32_t* mask_bits_dev, int32_t* actions_dev,
                       float* q_out_dev, void* stream);
/* Categorical (C51) loss and gradient of RLlib's QLoss with num_atoms > 1; target_params_dev: the target net, same flat layout.
 *   a*  = first maximum of the (masked) Q(s') of the online net (double_q 1) or of the target net (double_q 0)
 *   p'  = the target net's p(s')[a*, :]
 *   r_tau_j = clip(R + gamma_n * z_j, v_min, v_max) for a row that bootstraps, clip(R) for every j otherwise (terminal row, or a
 *             successor whose mask allows nothing): a select, nothing of such a row's successor - NaN included - reaches any output
 *   b_j = (r_tau_j - v_min) / dz, l = floor(b_j), u = ceil(b_j), eq = (u - l < 0.5)
 *   m[l] += p'_j (u - b_j + eq),  m[u] += p'_j (b_j - l)
 *   td = -sum_i m_i log_softmax(logits(s)[a, :])_i,   loss = mean(w * td),  w = weights_dev or 1
 * rewards_dev holds the n-step return R, dones_dev the n-step done, gamma_n = gamma ^ n_step (rl4rs_replay_sample_nstep).
 * Outputs: grad_dev (flat layout), td_dev [N] (the new priorities), next_action_dev [N] (optional: a*, -1 on terminal rows),
 * stats_dev float[4] (optional) = sums of {w * td, Q(s)[a], sum_i z_i m_i, td}.  N <= max_rows.  Fixed sample chunks and a fixed
 * summation order: bit-identical from run to run. */
int rl4rs_distq_loss_grad(rl4rs_distq* net, const float* target_params_dev, int32_t N, const float* obs_dev, const int32_t* actions_dev,
                          const float* rewards_dev, const int32_t* dones_dev, const float* next_obs_dev,
                          const uint32_t* next_mask_bits_dev, const float* weights_dev, float gamma_n, int32_t double_q, float* grad_dev,
                          float* td_dev, int32_t* next_action_dev, float* stats_dev, void* stream);
/* Adam (tf.train.AdamOptimizer form) with tf.clip_by_norm on each of the 8 (12 with dueling) variables; var_clip <= 0: no clipping */
int rl4rs_distq_adam_step_clip_by_var(rl4rs_distq* net, const float* grad_dev, float lr, float beta1, float beta2, float eps,
                                      float var_clip, void* stream);
/* rl4rs_replay_sample with RLlib's adjust_nstep on the discrete ring's complete episodes.  The index draw and the weights are
 * rl4rs_replay_sample's; for a row at step t of its T-step rollout, k = min(n_step, T - t):
 *   reward = sum_{j < k} gamma^j r_{t + j} (the ring's float32 rewards, accumulated in float64 in step order, stored float32)
 *   done   = (t + n_step >= T);  next obs / next mask = row idx + k * B when not done (a copy of the row itself otherwise)
 * n_step = 1 is rl4rs_replay_sample bit for bit.  The bootstrap factor of the loss is gamma ^ n_step, not gamma ^ k. */
int rl4rs_replay_sample_nstep(rl4rs_replay* h, int32_t M, int32_t n_step, double gamma, int32_t prioritized, double beta, uint32_t seed,
                              uint32_t step, float* obs_out, float* next_obs_out, uint32_t* next_mask_out, int32_t* action_out,
                              float* reward_out, int32_t* done_out, int32_t* idx_out, float* weight_out, float* u_out, void* stream);

/* --------------------------------------------------------------------------------------------------
 * V-trace (the off-policy correction of script/modelfree_train.py:345-390, algo "IMPALA"; restates RLlib 1.5.1's
 * vtrace_tf.from_importance_weights, parity unpinned).  All arrays are time-major [T, B] with row stride B; T is the number of
 * steps the loss runs over (RLlib's "drop the last step, bootstrap from its value" is the caller's business: pass T - 1 and
 * the dropped step's values as bootstrap_value).
 *   rho_t    = exp(target_logp_t - behaviour_logp_t)
 *   disc_t   = gamma * (1 - done_t)
 *   V_{t+1}  = values_{t+1} (t < T-1), bootstrap_value (t = T-1)
 *   delta_t  = min(clip_rho, rho_t) * (r_t + disc_t * V_{t+1} - V_t)
 *   acc_t    = delta_t + disc_t * min(1, rho_t) * acc_{t+1},   acc_T = 0
 *   vs_t     = V_t + acc_t
 *   vs_{t+1} = vs at t+1 (t < T-1), bootstrap_value (t = T-1)
 *   pg_adv_t = min(clip_pg_rho, rho_t) * (r_t + disc_t * vs_{t+1} - V_t)
 * bootstrap_value [B] (NULL = zeros), rewards float64 (the env's), dones int32 (NULL = none).  The scan runs in float64 and
 * rounds once on the store.  stats_out (optional) double[4] = {sum rho, sum min(rho, clip_rho), sum vs_out, sum pg_adv_out}
 * over all T * B entries, summed in a fixed order: bit-identical from run to run.  Refuses T < 1, B < 1, null required pointers. */
int rl4rs_vtrace(int32_t T, int32_t B, const float* behaviour_logp, const float* target_logp, const float* values,
                 const float* bootstrap_value, const double* rewards, const int32_t* dones, float gamma, float clip_rho,
                 float clip_pg_rho, float* vs_out, float* pg_adv_out, double* stats_out, void* stream);
/* V-trace loss and gradient on the net of `pol` in one call (RLlib 1.5.1's VTraceLoss).  Rows are [R, T, B]: R rollouts of T
 * time-major steps of B envs, row (r * T + t) * B + b; R * T * B <= max_rows.
 *   1. target_logp, values = the forward of rl4rs_policy_evaluate on every row
 *   2. rl4rs_vtrace per rollout.  drop_last 1 (RLlib): the loss runs over steps 0 .. T-2, the bootstrap is values[T-1] and
 *      nothing else of step T-1 is seen (T = 1 is refused); drop_last 0: all T steps, zero bootstrap
 *   3. rl4rs_policy_loss_grad(algo 0) on the kept rows with adv = pg_adv, ret = vs (both constants):
 *      -sum(logp * pg_adv) + vf_coeff * 0.5 * sum((V - vs)^2) - ent_coeff * sum(H)
 * The rows of a dropped step contribute nothing to grad_dev, the entropy sum or stats_dev (float[4] as rl4rs_policy_loss_grad).
 * vtrace_stats_dev (optional) double[4]: rl4rs_vtrace's sums, added up over the R rollouts.  vs_out / pg_adv_out (optional)
 * float [R * T * B]: the V-trace outputs in row order, zeros on dropped rows.  No Adam step inside: a data-parallel trainer
 * all-reduces grad_dev first.  The first call allocates the scratch on the handle.  behaviour_logp_dev float32, rewards_dev
 * float64, dones_dev int32 or NULL. */
int rl4rs_policy_vtrace_loss_grad(rl4rs_policy* pol, int32_t R, int32_t T, int32_t B, const float* obs_dev,
                                  const uint32_t* mask_bits_dev, const int32_t* actions_dev, const float* behaviour_logp_dev,
                                  const double* rewards_dev, const int32_t* dones_dev, float gamma, float clip_rho,
                                  float clip_pg_rho, int32_t drop_last, float vf_coeff, float ent_coeff, float* grad_dev,
                                  float* stats_dev, double* vtrace_stats_dev, float* vs_out, float* pg_adv_out, void* stream);

/* Raw-state policy encoder: rl4rs/nets/rllib/rllib_rawstate_model.py:25-86 (and its action-mask wrapper,
 * rllib_mask_model.py:67-115) for envs with config['rawstate_as_obs'] (rl4rs/env/slate.py:250-262):
 *   context = ELU([mean seq emb (per sequence, one shared table) | dense tower | mean category emb] @ ctx_w + ctx_b)  (256)
 *   logits  = context @ out_w + out_b (+ max(log(mask), float32.min)),   value = context @ value_w + value_b
 * Forward only (act / evaluate with the outputs of rl4rs_policy_act / rl4rs_policy_evaluate); shapes of the host
 * float32 weights in rl4rs_amd/nets/rawpolicy.py.  seq_dev: seq_num device pointers, each int32 [N, maxlen]. */
typedef struct rl4rs_rawpolicy rl4rs_rawpolicy;
typedef struct rl4rs_rawpolicy_cfg {
    int32_t maxlen, emb_size, hidden_units, dense_feature_num, category_feature_num, category_hash_size, seq_num,
        action_size, max_rows;
} rl4rs_rawpolicy_cfg;
typedef struct rl4rs_rawpolicy_weights {
    const float* cat_emb; const float* seq_emb;
    const float* dense_w1; const float* dense_b1; const float* dense_w2; const float* dense_b2;
    const float* ctx_w; const float* ctx_b;
    const float* out_w; const float* out_b;
    const float* value_w; const float* value_b;
} rl4rs_rawpolicy_weights;
int rl4rs_rawpolicy_create(const rl4rs_rawpolicy_cfg* cfg, const rl4rs_rawpolicy_weights* w, void* stream,
                           rl4rs_rawpolicy** out);
int rl4rs_rawpolicy_destroy(rl4rs_rawpolicy* pol);
int rl4rs_rawpolicy_act(rl4rs_rawpolicy* pol, int32_t N, const int32_t* cat_dev, const float* dense_dev,
                        const int32_t* const* seq_dev, const uint32_t* mask_bits_dev, uint32_t seed, uint32_t step,
                        int32_t* actions_dev, float* logp_dev, float* value_dev, float* entropy_dev, float* logits_dev,
                        void* stream);
int rl4rs_rawpolicy_evaluate(rl4rs_rawpolicy* pol, int32_t N, const int32_t* cat_dev, const float* dense_dev,
                             const int32_t* const* seq_dev, const uint32_t* mask_bits_dev, const int32_t* actions_dev,
                             float* logp_dev, float* value_dev, float* entropy_dev, float* logits_dev, void* stream);

/* Trainable raw-state policy: the model of rl4rs_rawpolicy with RLlib's A2C / PPO losses (rl4rs_policy_loss_grad semantics),
 * backward through both heads, the context layer, the dense tower and the mean-pooled embeddings, Adam.  Flat parameter /
 * gradient layout: [ cat_emb | seq_emb | dense_w1 | dense_b1 | dense_w2 | dense_b2 | ctx_w | ctx_b |
 *                    head_w 256 x (A+1) = [out_w | value_w] | head_b (A+1) ].  act / evaluate as rl4rs_rawpolicy_*. */
typedef struct rl4rs_rawtrain rl4rs_rawtrain;
int rl4rs_rawtrain_create(const rl4rs_rawpolicy_cfg* cfg, const rl4rs_rawpolicy_weights* w, void* stream, rl4rs_rawtrain** out);
int rl4rs_rawtrain_destroy(rl4rs_rawtrain* pol);
int rl4rs_rawtrain_params(rl4rs_rawtrain* pol, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_rawtrain_act(rl4rs_rawtrain* pol, int32_t N, const int32_t* cat_dev, const float* dense_dev,
                       const int32_t* const* seq_dev, const uint32_t* mask_bits_dev, uint32_t seed, uint32_t step,
                       int32_t* actions_dev, float* logp_dev, float* value_dev, float* entropy_dev, float* logits_dev,
                       void* stream);
int rl4rs_rawtrain_evaluate(rl4rs_rawtrain* pol, int32_t N, const int32_t* cat_dev, const float* dense_dev,
                            const int32_t* const* seq_dev, const uint32_t* mask_bits_dev, const int32_t* actions_dev,
                            float* logp_dev, float* value_dev, float* entropy_dev, float* logits_dev, void* stream);
int rl4rs_rawtrain_loss_grad(rl4rs_rawtrain* pol, int32_t algo, int32_t N, const int32_t* cat_dev, const float* dense_dev,
                             const int32_t* const* seq_dev, const uint32_t* mask_bits_dev, const int32_t* actions_dev,
                             const float* adv_dev, const float* ret_dev, const float* old_logp_dev,
                             const float* old_value_dev, const float* old_logits_dev, float vf_coeff, float ent_coeff,
                             float clip, float vf_clip, float kl_coeff, float* stats_dev, void* stream);
int rl4rs_rawtrain_adam_step(rl4rs_rawtrain* pol, float lr, float beta1, float beta2, float eps, float grad_clip,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * On-device raw-state DQN: script/modelfree_train.py:55-56,63-66,106-133 (algo "DQN_rawstate": the DQN settings above on
 * mask_model_rawstate, rllib_mask_model.py:67-115 over rllib_rawstate_model.py:25-86).  The Q values are the masked logits of the
 * rl4rs_rawtrain net; its value head takes no part.  RLlib parity is unpinned as for DQN.  Out of scope: RAINBOW_rawstate, the
 * continuous model_rawstate learners (TD3 / DDPG / *_conti), PG / IMPALA on the raw handle.
 *
 * Packed raw-state record: one observation row as REC 32-bit words
 *   [ dense: Dn float32 | cat: Cn int32 | seq_0: L int32 | ... | seq_{S-1}: L int32 | zero pad to a multiple of 4 words ]
 * (Dn = dense_feature_num, Cn = category_feature_num, L = maxlen, S = seq_num; 432 + 21 + 2 * 64 = 581 -> REC 584 at the default
 * configuration).  Dense comes first, so the dense part of a batch of records is a GEMM operand with lda = REC, 16-byte aligned.
 * Ids are stored as they come, not clamped: every forward clamps them to [0, category_hash_size) where it uses them.  The
 * buffer is typed float* only because the replay ring's obs column is; rl4rs_replay_* with obs_dim = REC stores such records
 * unchanged (see rl4rs_replay_push). */
int32_t rl4rs_rawstate_record_words(const rl4rs_rawpolicy_cfg* cfg);      /* REC; 0 for a NULL / impossible configuration */
/* rec_out_dev [N, REC] from cat_dev int32 [N, Cn], dense_dev float32 [N, Dn], seq_dev: S device pointers of int32 [N, L].  One
 * launch; only cfg's five layout fields are read. */
int rl4rs_rawstate_pack(const rl4rs_rawpolicy_cfg* cfg, int32_t N, const int32_t* cat_dev, const float* dense_dev,
                        const int32_t* const* seq_dev, float* rec_out_dev, void* stream);
/* rl4rs_policy_dqn_loss_grad with the raw-state model as the network: the same a*, y (a select: nothing of a terminal row's
 * successor record - NaN dense values, ids out of range - reaches any output), no bootstrap from a successor that allows no action,
 * td, Huber loss (delta 1), loss = mean(w * huber), td_dev [N], next_action_dev [N] (optional: a*, -1 on terminal rows) and
 * stats_dev float[4] (optional) = sums of {w * huber, Q(s)[a], y, |td|}.
 *   rec_dev / next_rec_dev   float [N, REC]: the records of s and s', read in place (no unpacked copy is made)
 *   target_params_dev        the target net: a device buffer in the handle's flat layout (rl4rs_rawtrain_params gives the count),
 *                            with its own copy of the two embedding tables
 * The gradient goes into the handle's flat gradient buffer, as in rl4rs_rawtrain_loss_grad: the value-head column and every
 * action column nobody took are exactly 0, and so is every table row no id of the minibatch touches.  N <= max_rows; the first
 * call allocates the scratch of the two s' forwards on the handle.
 * Three forwards (s online, s' target, s' online when double_q), each one pooling launch for all S + 1 id fields and the GEMMs
 * with lda = REC; one wave per row then picks a*, takes Q(s)[a] and Q_target(s')[a*] as single-column products over the 256-wide
 * context and writes d loss / d (context pre-activation) = g * head_w[:, a] * ELU'(context) directly - no [N, A + 1] head gradient,
 * no GEMM back through the head.  The head's gradient is gathered column by column; below the context layer the backward is
 * rl4rs_rawtrain_loss_grad's, with one embedding scatter launch reading the ids from the records.
 * Reproducibility: td, stats, a* and the gradients of the eight dense variables are bit-identical from run to run (fixed
 * summation orders); the embedding scatter keeps the handle's float atomics, so the two tables' gradients are not. */
int rl4rs_rawtrain_dqn_loss_grad(rl4rs_rawtrain* pol, const float* target_params_dev, int32_t N, const float* rec_dev,
                                 const int32_t* actions_dev, const float* rewards_dev, const int32_t* dones_dev,
                                 const float* next_rec_dev, const uint32_t* next_mask_bits_dev, const float* weights_dev,
                                 float gamma, int32_t double_q, float* td_dev, int32_t* next_action_dev, float* stats_dev,
                                 void* stream);
/* Greedy action: the forward of rl4rs_rawtrain_act, then the first maximum of the masked Q row; q_dev (optional) receives the
 * masked row [N, action_size].  A row that allows nothing returns action 0. */
int rl4rs_rawtrain_greedy(rl4rs_rawtrain* pol, int32_t N, const int32_t* cat_dev, const float* dense_dev,
                          const int32_t* const* seq_dev, const uint32_t* mask_bits_dev, int32_t* actions_dev, float* q_dev,
                          void* stream);
/* TF-form Adam on the handle's gradient with tf.clip_by_norm applied to EACH of the ten variables of the flat layout by its own
 * norm (RLlib DQN's minimize_and_clip, grad_clip 40); var_clip <= 0: no clipping, bit-identical to rl4rs_rawtrain_adam_step with
 * grad_clip 0.  The ten sums of squares are one two-stage pass: tiles of 16384 elements over as many workgroups (a tile that
 * straddles variable boundaries gives one partial sum per variable it meets), then the tiles of a variable added in tile order -
 * bit-identical from run to run for the same gradient buffer.  (rl4rs_rawtrain_adam_step's global-norm clip still reduces in one
 * workgroup.) */
int rl4rs_rawtrain_adam_step_clip_by_var(rl4rs_rawtrain* pol, float lr, float beta1, float beta2, float eps, float var_clip,
                                         void* stream);
/* Measurement aid (tools/rawdqn_rate.py): with profiling on, rl4rs_rawtrain_dqn_loss_grad and ..._adam_step_clip_by_var record
 * events at their stage boundaries; rl4rs_rawtrain_profile waits for the last call of each and returns float[5] milliseconds:
 * the three forwards, the row kernel, the backward (head gradient, chain, statistics), the sums of squares, the Adam kernel.
 * Both calls must have run since profiling was switched on. */
int rl4rs_rawtrain_set_profiling(rl4rs_rawtrain* pol, int32_t on);
int rl4rs_rawtrain_profile(rl4rs_rawtrain* pol, float* ms_out);

/* Supervised training of the 'dnn' / 'widedeep' / 'lstm' simulators (rl4rs/nets/dnn.py, widedeep.py, lstm.py) on the device: what
 * script/supervised_train.py:37-42 does with model.compile(loss='binary_crossentropy', optimizer='adam') + model.fit -
 * forward in training mode (Dropout after each dense-tower layer, utils.py:48-54), keras binary_crossentropy of the
 * softmax output against the one-hot label, backward (BPTT through the keras GRUs of the lstm family), Adam.
 * cfg->algo = RL4RS_SIMNET_DNN, RL4RS_SIMNET_WIDEDEEP or RL4RS_SIMNET_LSTM.
 * Parameters, gradients and Adam state are flat float32 buffers (arrays a family does not have are skipped):
 *   [ cat_emb | seq_emb | dense_w1 | dense_b1 | dense_w2 | dense_b2 | fc_w | fc_b | obs_w | obs_b | out_w | out_b |
 *     lstm: cat_gru kernel, recurrent, bias | seq0_gru kernel, recurrent, bias | seq1_gru ... ]
 * dense_dev [N, dense_feature_num] f32, cat_dev [N, category_feature_num] i32, seq_dev: seq_num pointers of int32
 * [N, maxlen] (widedeep, lstm; may be NULL for dnn), labels_dev [N] i32 in [0, class_num); the dropout masks are a pure
 * function of (seed, step, row, column). */
typedef struct rl4rs_simtrain rl4rs_simtrain;
int rl4rs_simtrain_create(const rl4rs_simnet_cfg* cfg, const rl4rs_simnet_weights* w, int32_t max_batch, void* stream,
                          rl4rs_simtrain** out);
int rl4rs_simtrain_destroy(rl4rs_simtrain* tr);
/* device pointers of the flat parameter / gradient buffers (owned by the handle) and their length */
int rl4rs_simtrain_params(rl4rs_simtrain* tr, float** params_dev, float** grad_dev, int64_t* count);
/* the dropout keep-masks (uint8 [N, hidden_units] each) of the last grad / step call (for gradient checks) */
int rl4rs_simtrain_masks(rl4rs_simtrain* tr, uint8_t** mask1_dev, uint8_t** mask2_dev);
/* forward + loss + backward into the gradient buffer; loss_dev[0] = mean loss (may be NULL) */
int rl4rs_simtrain_grad(rl4rs_simtrain* tr, int32_t N, const float* dense_dev, const int32_t* cat_dev,
                        const int32_t* const* seq_dev, const int32_t* labels_dev, float dropout_rate, uint32_t seed,
                        uint32_t step, float* loss_dev, void* stream);
/* rl4rs_simtrain_grad + one Adam update (keras defaults: lr 1e-3, beta 0.9 / 0.999, epsilon 1e-7) */
int rl4rs_simtrain_step(rl4rs_simtrain* tr, int32_t N, const float* dense_dev, const int32_t* cat_dev,
                        const int32_t* const* seq_dev, const int32_t* labels_dev, float lr, float beta1, float beta2,
                        float eps, float dropout_rate, uint32_t seed, uint32_t step, float* loss_dev, void* stream);

/* The slate-wise models of script/supervised_train.py (rl4rs/nets/{dnn,widedeep,lstm,dien}_slate.py, *_slate_multiclass.py,
 * adversarial_slate.py): the item-wise trunk with another output layer and loss, one sample per page.
 *   ITEM              the handle of rl4rs_simtrain_create / rl4rs_dientrain_create (labels_dev [N] in [0, class_num))
 *   SLATE             Dense(9, sigmoid) + binary_crossentropy: row loss = mean_j [max(x,0) - x y + log1p(exp(-|x|))] of the logits x
 *   SLATE_MULTICLASS  Dense(22, softmax) + categorical crossentropy of class c = sum_j y_j [1,2,4,1,2,4,1,2,4][j]:
 *                     row loss = logsumexp(x) - x[c]
 *   ADVERSARIAL       rl4rs_simtrain only, cfg->algo = RL4RS_SIMNET_ADVERSARIAL: features [mean of each sequence's embeddings
 *                     (seq_num * E) | dense tower (U) | mean of the category embeddings of the first category_feature_num - 1 ids (E)]
 *                     -> Dense(9); s = sigmoid(x), row loss = 0.1 * (the SLATE loss) + sum_j softmax(s)_j (1 - y_j).
 *                     Arrays: cat_emb, seq_emb, dense_w1, dense_b1, dense_w2, dense_b2, out_w, out_b.
 * For every head but ITEM the output layer is [obs_dim, 9] / [obs_dim, 22] whatever cfg->class_num says (only out_w / out_b change
 * width in the flat layout) and labels_dev of grad / step / eval is int32 [N, 9] of 0 / 1.  All losses are taken from the logits
 * (keras does so for a Sigmoid / Softmax output op), so nothing is clipped. */
enum { RL4RS_HEAD_ITEM = 0, RL4RS_HEAD_SLATE = 1, RL4RS_HEAD_SLATE_MULTICLASS = 2, RL4RS_HEAD_ADVERSARIAL = 3 };
int rl4rs_simtrain_create_head(const rl4rs_simnet_cfg* cfg, const rl4rs_simnet_weights* w, int32_t head, int32_t max_batch,
                               void* stream, rl4rs_simtrain** out);
/* device pointers of the Adam moments (owned by the handle) and the number of steps taken */
int rl4rs_simtrain_adam_state(rl4rs_simtrain* tr, float** m_dev, float** v_dev, int64_t* step);
/* Inference pass on a trainer handle (validation): forward without dropout, no backward; parameters, gradient buffer and Adam state
 * are left untouched.  pred_dev [N, K] f32 = the model output (softmax for ITEM with K = class_num and SLATE_MULTICLASS with K = 22,
 * sigmoid with K = 9 otherwise); loss_rows_dev [N] (may be NULL) = the head's row losses, which need labels_dev (else may be NULL). */
int rl4rs_simtrain_eval(rl4rs_simtrain* tr, int32_t N, const float* dense_dev, const int32_t* cat_dev,
                        const int32_t* const* seq_dev, const int32_t* labels_dev, float* pred_dev, float* loss_rows_dev,
                        void* stream);

/* Supervised training of the DIEN simulator (rl4rs/nets/dien.py; script/supervised_train.py with model_type='dien') on the
 * device: training-mode forward (Dropout after each dense-tower layer), keras binary_crossentropy, backward through the
 * head, the category self-attention, the dense tower and, per sequence input, the DIN attention MLP, the AUGRU and the
 * first GRU (explicit BPTT), Adam.  Weights as for rl4rs_dien_create (max_rows, max_slots, scorer_mode unused).  The
 * trainer's own size limits, refused at create: emb_size = 128 (the recurrences are built for widths 128 / 256),
 * 10 <= category_feature_num <= 32, 1 <= seq_num <= 4, 2 <= class_num <= 8, 1 <= maxlen <= 64 (the persistent training
 * recurrences; no step-by-step form), and max_batch * maxlen * 3 * 256 * 4 < 2^31 (the AUGRU's pre-activations:
 * max_batch <= 10922 at maxlen 64).
 * Flat parameter / gradient layout:
 *   [ cat_emb | seq_emb | dense_w1 | dense_b1 | dense_w2 | dense_b2 | obs_w | obs_b | out_w | out_b |
 *     per sequence input: gru_gate_w, gru_gate_b, gru_cand_w, gru_cand_b, att_w1, att_b1, att_w2, att_b2, att_w3, att_b3,
 *                         augru_gate_w, augru_gate_b, augru_cand_w, augru_cand_b ]
 * Arguments of grad / step as for rl4rs_simtrain_grad / rl4rs_simtrain_step (seq_dev is required). */
/* Row-tile form of the persistent training recurrences (the GRU / AUGRU layers of rl4rs_dientrain_* and of the lstm family of
 * rl4rs_simtrain_*; reference: model.fit with batch_size 256, script/supervised_train.py:12-46): 0 = automatic (8-row workgroups
 * on v_mfma_f32_4x4x1 while 32-row ones would occupy fewer than half of the CUs - a 256-sample minibatch is 64 workgroups
 * instead of 16; hidden width 256 goes on to 4-row workgroups - 128 of them - while the 8-row ones would), 4 (hidden width 256;
 * other widths take 8), 8 or 32 = pinned.  Process-wide; same arithmetic up to the summation order of a dot product. */
int rl4rs_recur_train_set_rows(int32_t rows);

typedef struct rl4rs_dientrain rl4rs_dientrain;
int rl4rs_dientrain_create(const rl4rs_dien_cfg* cfg, const rl4rs_dien_weights* w, int32_t max_batch, void* stream,
                           rl4rs_dientrain** out);
/* head: RL4RS_HEAD_ITEM (= rl4rs_dientrain_create), RL4RS_HEAD_SLATE or RL4RS_HEAD_SLATE_MULTICLASS (dien_slate.py,
 * dien_slate_multiclass.py); _adam_state and _eval as for rl4rs_simtrain_* */
int rl4rs_dientrain_create_head(const rl4rs_dien_cfg* cfg, const rl4rs_dien_weights* w, int32_t head, int32_t max_batch,
                                void* stream, rl4rs_dientrain** out);
int rl4rs_dientrain_adam_state(rl4rs_dientrain* tr, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_dientrain_eval(rl4rs_dientrain* tr, int32_t N, const float* dense_dev, const int32_t* cat_dev,
                         const int32_t* const* seq_dev, const int32_t* labels_dev, float* pred_dev, float* loss_rows_dev,
                         void* stream);
int rl4rs_dientrain_destroy(rl4rs_dientrain* tr);
/* The launch chains that follow a recurrent layer (parameter-gradient reductions, the attention MLP's forward / backward) of the
 * ODD sequence inputs run on a second stream of the handle, beside the even inputs' (each ~35 small launches; own scratch; joined in
 * front of the next recurrent launch).  Process-wide switch, default 1; 0 = everything on the caller's stream (A/B measurements).
 * Same kernels on the same operands either way (the embedding-table gradient takes float atomics from both). */
int rl4rs_dientrain_set_fork(int32_t on);
int rl4rs_dientrain_params(rl4rs_dientrain* tr, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_dientrain_masks(rl4rs_dientrain* tr, uint8_t** mask1_dev, uint8_t** mask2_dev);
int rl4rs_dientrain_grad(rl4rs_dientrain* tr, int32_t N, const float* dense_dev, const int32_t* cat_dev,
                         const int32_t* const* seq_dev, const int32_t* labels_dev, float dropout_rate, uint32_t seed,
                         uint32_t step, float* loss_dev, void* stream);
int rl4rs_dientrain_step(rl4rs_dientrain* tr, int32_t N, const float* dense_dev, const int32_t* cat_dev,
                         const int32_t* const* seq_dev, const int32_t* labels_dev, float lr, float beta1, float beta2,
                         float eps, float dropout_rate, uint32_t seed, uint32_t step, float* loss_dev, void* stream);

/* Streaming classifier metrics (script/supervised_train.py:38-42 and the slate models' compile calls: keras AUC, Precision, Recall,
 * 'acc', categorical accuracy): int64 confusion counts on the device, integer atomics only - exact, and the same from run to run.
 * No update waits for the host.  thresholds: host float32 [num_thresholds], non-decreasing - for keras AUC(num_thresholds = T) the table
 * [-1e-7] + [(i + 1) / (T - 1) for i in range(T - 2)] + [1 + 1e-7].  A prediction counts as positive at a threshold iff pred > thr in
 * float32 (a NaN never does).
 *   update_binary      n elements: pred_dev f32 [n], label_dev i32 [n] (non-zero = positive); TP / FP / TN / FN at every threshold
 *                      and at 0.5 (Precision, Recall, binary accuracy)
 *   update_multiclass  pred_dev f32 [N, K], label_dev i32 [N]: rows whose first maximum is the label, and rows
 *   read               waits for the stream; counts_host int64 [4 T + 6] = TP [T] | FP [T] | TN [T] | FN [T] | tp, fp, tn, fn at 0.5 |
 *                      multiclass correct, rows.  The metrics themselves are the host's (rl4rs_amd/metrics.py). */
typedef struct rl4rs_clfmetrics rl4rs_clfmetrics;
int rl4rs_clfmetrics_create(int32_t num_thresholds, const float* thresholds, void* stream, rl4rs_clfmetrics** out);
int rl4rs_clfmetrics_destroy(rl4rs_clfmetrics* m);
int rl4rs_clfmetrics_reset(rl4rs_clfmetrics* m, void* stream);
int rl4rs_clfmetrics_update_binary(rl4rs_clfmetrics* m, int64_t n, const float* pred_dev, const int32_t* label_dev, void* stream);
int rl4rs_clfmetrics_update_multiclass(rl4rs_clfmetrics* m, int64_t N, int32_t K, const float* pred_dev, const int32_t* label_dev,
                                       void* stream);
int rl4rs_clfmetrics_read(rl4rs_clfmetrics* m, int64_t* counts_host, void* stream);

/* Offline-RL learner networks and losses: what script/batchrl_trainer.py:34-90 trains with d3rlpy (DiscreteBC, DiscreteBCQ,
 * DiscreteCQL) on the logged-policy dataset, BASELINE configs[4].  A qnet is one encoder + d3rlpy's Linear head:
 *   mask_size = page_items + 1 > 0: CustomVectorEncoder of rl4rs/nets/cql/encoder.py:9-67 (with_q=True):
 *       relu(fc1(x)) | Embedding(action_size, emb_size)(x[-mask_size:]) -> fc2 -> [action_size], entries whose mask is 0 set to 0
 *       (mask = location_mask[cur_step % 9 // 3], previous actions and - once one was chosen - special items removed), then
 *       head Linear(action_size, action_size);
 *   mask_size = 0: d3rlpy VectorEncoder relu(fc1) -> relu(fc2) [hidden2], head Linear(hidden2, action_size).
 * Flat float32 parameter / gradient layout, matrices stored [in, out]:
 *   [ fc1_w obs_dim x hidden1 | fc1_b | emb action_size x emb_size (custom only) | fc2_w | fc2_b | head_w | head_b ]
 * params_host, location_mask [n_layers, action_size] and is_special [action_size] are HOST pointers (the masks may be NULL for
 * the plain encoder).  forward keeps the activations in the handle; backward must follow the forward of the SAME rows and
 * writes the gradient of sum(out * dout_dev).  adam_step is torch.optim.Adam.  status: bit 0 = an id in an observation tail
 * or an action was out of range (torch would raise IndexError), bit 1 = mask layer out of range. */
typedef struct rl4rs_qnet rl4rs_qnet;
typedef struct rl4rs_qnet_cfg {
    int32_t obs_dim;
    int32_t action_size;
    int32_t mask_size;
    int32_t emb_size;
    int32_t hidden1;
    int32_t hidden2;
    int32_t n_layers;
    int32_t max_rows;
} rl4rs_qnet_cfg;
int rl4rs_qnet_create(const rl4rs_qnet_cfg* cfg, const float* params_host, const uint8_t* location_mask,
                      const uint8_t* is_special, void* stream, rl4rs_qnet** out);
int rl4rs_qnet_destroy(rl4rs_qnet* net);
int rl4rs_qnet_params(rl4rs_qnet* net, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_qnet_copy_params(rl4rs_qnet* dst, const rl4rs_qnet* src, void* stream);
/* Adam moments (device pointers, `count` floats each) and step count of the handle: checkpointing (d3rlpy save_model / load_model,
 * script/batchrl_train.py:132,141). */
int rl4rs_qnet_adam_state(rl4rs_qnet* net, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_qnet_set_adam_step(rl4rs_qnet* net, int64_t step);
int rl4rs_qnet_status(rl4rs_qnet* net, int32_t* flags, void* stream);
int rl4rs_qnet_forward(rl4rs_qnet* net, int32_t N, const float* obs_dev, float* out_dev, void* stream);
int rl4rs_qnet_backward(rl4rs_qnet* net, int32_t N, const float* obs_dev, const float* dout_dev, void* stream);
int rl4rs_qnet_adam_step(rl4rs_qnet* net, float lr, float beta1, float beta2, float eps, void* stream);
/* Greedy action per row [N]: argmax q (first maximum), or - with imitator logits - the DiscreteBCQ rule
 * argmax (q - min q) * [log pi - max log pi > log(action_flexibility)]. */
int rl4rs_q_best_action(int32_t N, int32_t A, const float* q_dev, const float* imitator_logits_dev,
                        float action_flexibility, int32_t* actions_dev, void* stream);
/* DiscreteImitator.compute_error: loss2_dev = {mean nll_loss(log_softmax(logits), a), mean_n sum_k logits^2}; dlogits_dev =
 * gradient of nll + beta * mean(logits^2).  rows_scratch_dev: [N, 2] float32. */
int rl4rs_qloss_imitation(rl4rs_qnet* net, int32_t N, const float* logits_dev, const int32_t* actions_dev, float beta,
                          float* dlogits_dev, float* rows_scratch_dev, float* loss2_dev, void* stream);
/* DoubleDQN temporal-difference loss (+ DiscreteCQL's conservative term when cql_alpha > 0): the next action is chosen
 * from q_next_dev by rl4rs_q_best_action's rule (imitator_next_logits_dev NULL = argmax), evaluated on q_next_target_dev;
 * loss2_dev = {mean huber(r + gamma * Q_targ(s')[a*] * (1 - terminal) - Q(s)[a]), mean(logsumexp Q(s) - Q(s)[a])};
 * dq_dev = gradient of td + cql_alpha * conservative wrt q_t_dev.  best_next_action_dev (optional) receives a*. */
int rl4rs_qloss_dqn(rl4rs_qnet* net, int32_t N, const float* q_t_dev, const int32_t* actions_dev, const float* rewards_dev,
                    const float* terminals_dev, const float* q_next_dev, const float* q_next_target_dev,
                    const float* imitator_next_logits_dev, float action_flexibility, float gamma, float cql_alpha,
                    float* dq_dev, float* rows_scratch_dev, float* loss2_dev, int32_t* best_next_action_dev, void* stream);

/* Continuous-action offline-RL learners: what script/batchrl_trainer.py:61-73 ('BCQ-conti', d3rlpy.algos.BCQ) and :91-107
 * ('CQL-conti', d3rlpy.algos.CQL) train on the continuous dataset of data_generate_rl4rs_a_conti (:220-270, actions = 32-d item
 * embeddings), BASELINE configs[4].  Both leave the custom encoder factory commented out, so every network is d3rlpy's default
 * VectorEncoderWithAction([256, 256], relu) on cat([x, action]) + one Linear head = an "amlp":
 *     h1 = relu([x | a] W1 + b1);  h2 = relu(h1 W2 + b2);  out = head_act(h2 W3 + b3)      (act_dim = 0: plain VectorEncoder)
 * head_act: the activation codes of rl4rs_gemm_f32 (0 none, 3 tanh ...).
 * Flat float32 parameter / gradient layout, matrices stored [in, out]:
 *     [ W1 (obs_dim + act_dim) x hidden1 (observation rows first, like torch.cat([x, action])) | b1 | W2 | b2 | W3 | b3 ]
 * forward: obs_dev [N / rep, obs_dim] - row r is the observation of rows r*rep .. r*rep + rep - 1 of act_dev [N, act_dim]
 * (rep sampled actions per observation: the observation side of the first layer is computed once per observation);
 * out_dev [N, out_dim].  The activations stay in the handle: backward must follow the forward of the SAME rows, takes the
 * gradient wrt the head's PRE-activation output (the loss entry points below fold the head activation in), writes every
 * parameter gradient into the handle when want_param_grad, and the gradient wrt act_dev into dact_dev when that is not NULL.
 * N <= max_rows for forward, N <= max_grad_rows for backward.  adam_step is torch.optim.Adam; soft_update is d3rlpy's
 * soft_sync  targ = (1 - tau) * targ + tau * src. */
typedef struct rl4rs_amlp rl4rs_amlp;
typedef struct rl4rs_amlp_cfg {
    int32_t obs_dim;
    int32_t act_dim;
    int32_t hidden1;
    int32_t hidden2;
    int32_t out_dim;
    int32_t head_act;
    int32_t max_rows;
    int32_t max_grad_rows;
} rl4rs_amlp_cfg;
int rl4rs_amlp_create(const rl4rs_amlp_cfg* cfg, const float* params_host, void* stream, rl4rs_amlp** out);
int rl4rs_amlp_destroy(rl4rs_amlp* net);
int rl4rs_amlp_params(rl4rs_amlp* net, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_amlp_copy_params(rl4rs_amlp* dst, const rl4rs_amlp* src, void* stream);
int rl4rs_amlp_adam_state(rl4rs_amlp* net, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_amlp_set_adam_step(rl4rs_amlp* net, int64_t step);
int rl4rs_amlp_soft_update(rl4rs_amlp* targ, const rl4rs_amlp* src, float tau, void* stream);
int rl4rs_amlp_forward(rl4rs_amlp* net, int32_t N, int32_t rep, const float* obs_dev, const float* act_dev, float* out_dev,
                       void* stream);
/* The same forward for rows that never see a backward (target values, greedy evaluation: batch x n_action_samples rows), in
 * fp16x2 arithmetic (operands as fp16 hi + lo, three f16 MFMAs per product, fp32 accumulation - the scorer's form) as ONE launch
 * for the three layers behind the observation-side projection.  rl4rs_amlp_h16_ok: 1 when the network's shape has this form
 * (hidden 256 x 256, act_dim 8..64 in multiples of 8, out_dim <= 64).  The fp16 planes are rebuilt from the current fp32
 * parameters in front of every call; rows whose activations leave the fp16 range come back NaN; a following
 * rl4rs_amlp_backward is refused (no activations are kept).  Replaces the torch.no_grad() forwards of
 * d3rlpy BCQImpl.compute_target / _predict_best_action (script/batchrl_trainer.py:61-73 trains and evaluates through them). */
int rl4rs_amlp_h16_ok(const rl4rs_amlp* net);
int rl4rs_amlp_forward_h16(rl4rs_amlp* net, int32_t N, int32_t rep, const float* obs_dev, const float* act_dev, float* out_dev,
                           void* stream);
int rl4rs_amlp_backward(rl4rs_amlp* net, int32_t N, int32_t rep, const float* obs_dev, const float* act_dev,
                        const float* dout_dev, float* dact_dev, int32_t want_param_grad, void* stream);
int rl4rs_amlp_adam_step(rl4rs_amlp* net, float lr, float beta1, float beta2, float eps, void* stream);
/* The optimiser of ONE phase of an update as one launch: torch.optim.Adam for the n <= 8 networks with do_adam[i] != 0 (learning
 * rate lr[i]) and, for every i with targets[i] != NULL, d3rlpy's soft_sync targets[i] = (1 - tau) targets[i] + tau nets[i] computed
 * from the parameters AFTER this call's step (do_adam[i] = 0: soft update only).  targets may be NULL.  Element for element the
 * arithmetic of rl4rs_amlp_adam_step / rl4rs_amlp_soft_update. */
int rl4rs_amlp_adam_multi(int32_t n, rl4rs_amlp* const* nets, const float* lr, const int32_t* do_adam, rl4rs_amlp* const* targets,
                          float beta1, float beta2, float eps, float tau, void* stream);
/* Minibatch-sized rl4rs_amlp_forward / rl4rs_amlp_backward calls (hidden 256 x 256, out_dim / act_dim <= 64, rep = 1, N <= 2048 /
 * 1024) run as fused launches - one for the three layers forwards; transposes + input-gradient chain + all parameter gradients
 * backwards - instead of one launch per layer and product.  on = 0 restores the per-layer launches, 2 selects the 8-rows-per-
 * workgroup form of the fused kernels (measured slower at 256 rows; default 1 = 4 rows).  Process-wide; tests, A/B. */
int rl4rs_amlp_set_fused(int32_t on);
/* n <= 4 networks with the same input widths on the SAME rows (d3rlpy's twin critics: both Q functions see (s, a)) - forward /
 * backward of all of them as one launch each way when the call has the fused form, otherwise one rl4rs_amlp_forward / _backward
 * per network.  rep = 1.  outs_dev[i] [N, out_dim_i]; douts_dev[i] as for rl4rs_amlp_backward; dacts_dev (or its entries) may be NULL. */
int rl4rs_amlp_forward_multi(int32_t n, rl4rs_amlp* const* nets, int32_t N, const float* obs_dev, const float* act_dev,
                             float* const* outs_dev, void* stream);
int rl4rs_amlp_backward_multi(int32_t n, rl4rs_amlp* const* nets, int32_t N, const float* obs_dev, const float* act_dev,
                              const float* const* douts_dev, float* const* dacts_dev, int32_t want_param_grad, void* stream);
/* d3rlpy ConditionalVAE (the BCQ imitator).  enc_out_dev [N, 2L] = [mu | logstd] (the encoder amlp's two Linear heads side by
 * side); sample: z = mu + exp(clamp(logstd, min, max)) * eps (Normal.rsample with the caller's noise).
 * loss (compute_error): decoded_dev [N, E] = tanh output of the decoder amlp on (x, z); loss2_dev = {mean_n sum_e (y - a)^2,
 * mean_n sum_l KL(N(mu, sigma) || N(0, 1))} - the loss is loss2[0] / E + beta * loss2[1] / L; d_dec_pre_dev = gradient of the
 * mse term wrt the decoder's pre-tanh output.  rows_scratch_dev: [N, 2] float32.
 * encoder_grad: d_enc_out_dev [N, 2L] from dz_dev (the decoder's action-input gradient) and the beta-weighted KL term. */
int rl4rs_cvae_sample(int32_t N, int32_t L, const float* enc_out_dev, const float* eps_dev, float min_logstd, float max_logstd,
                      float* z_dev, void* stream);
int rl4rs_cvae_loss(int32_t N, int32_t E, int32_t L, const float* decoded_dev, const float* actions_dev, const float* enc_out_dev,
                    float min_logstd, float max_logstd, float* d_dec_pre_dev, float* rows_scratch_dev, float* loss2_dev,
                    void* stream);
int rl4rs_cvae_encoder_grad(int32_t N, int32_t L, const float* enc_out_dev, const float* eps_dev, const float* dz_dev, float beta,
                            float min_logstd, float max_logstd, float* d_enc_out_dev, void* stream);
/* d3rlpy DeterministicResidualPolicy: out = clamp(action + scale * tanh_out, -1, 1) with tanh_out_dev [N, E] the tanh head
 * of the policy amlp on (x, action); residual_grad: gradient wrt the policy head's pre-tanh output given d_out_dev. */
int rl4rs_residual_action(int32_t N, int32_t E, const float* action_dev, const float* tanh_out_dev, float scale, float* out_dev,
                          void* stream);
int rl4rs_residual_grad(int32_t N, int32_t E, const float* action_dev, const float* tanh_out_dev, float scale,
                        const float* d_out_dev, float* d_pre_dev, void* stream);
/* BCQ target (d3rlpy compute_max_with_n_actions): per row b the value max_j [(1 - lam) max(q1, q2) + lam min(q1, q2)] over its n
 * sampled actions (q*_dev [B * n]); y_dev [B] = rewards + gamma * value * (1 - terminals), or the bare value when rewards_dev
 * is NULL; best_dev [B] (optional) = the first maximising j.  q2_dev NULL: the value is q1 (the greedy pick of predict). */
int rl4rs_bcq_target(int32_t B, int32_t n, const float* q1_dev, const float* q2_dev, float lam, const float* rewards_dev,
                     const float* terminals_dev, float gamma, float* y_dev, int32_t* best_dev, void* stream);
/* out_dev [B, E] = rows_dev [b * n + best_dev[b], :] */
int rl4rs_pick_rows(int32_t B, int32_t n, int32_t E, const float* rows_dev, const int32_t* best_dev, float* out_dev, void* stream);
/* Twin ContinuousMeanQFunction error: loss2_dev = {mean (q1 - y)^2, mean (q2 - y)^2} (the critic loss is their sum),
 * dq*_dev = 2 (q* - y) / N. */
int rl4rs_critic_mse(int32_t N, const float* q1_dev, const float* q2_dev, const float* y_dev, float* dq1_dev, float* dq2_dev,
                     float* loss2_dev, void* stream);

/* Continuous CQL (d3rlpy.algos.CQL = SAC + the conservative critic term; 'CQL-conti', script/batchrl_trainer.py:91-107).
 * squashed_sample: d3rlpy SquashedNormalPolicy.sample(_n)_with_log_prob.  head_dev [N / rep, 2A] = [mu | logstd] (the policy
 * amlp's two Linear heads side by side, act_dim = 0), eps_dev [N, A] the caller's Gaussian noise (NULL: the deterministic
 * best_action a = tanh(mu), no log-prob).  u = mu + exp(clamp(logstd)) * eps, a = tanh(u), logp = sum_e [Normal log-prob of u
 * - 2 (log 2 - u - softplus(-2u))].  Sample i of observation r is written to destination row r * out_rep + out_off + i % rep of
 * act_out_dev [.., A] and logp_out_dev (so several sample groups of an observation can sit side by side).
 * sac_actor_grad: gradient of mean_b [exp(log_temp) * logp_b - Qmin(s_b, a_b)] wrt the head, given g_act_dev [B, A] = gradient
 * of -mean Qmin wrt the action (the critics' rl4rs_amlp_backward dact, 1 / B included); log_temp_dev: device scalar.
 * twin_min: qmin = min(q1, q2) and (optional) the selector dq_c = -1/B on the smaller critic (q1 on ties).
 * cql_critic_loss: rows laid out [B][m], column 0 = the dataset action, columns 1..m-1 = sampled actions with importance
 * offsets offs_dev (log-prob of a policy sample, A * log 0.5 of a uniform one):
 *   sums6_dev = {sum_b (q1[b,0] - y_b)^2, same for q2, sum_b logsumexp_j (q1[b,j] - offs[b,j]), same for q2, sum_b q1[b,0], sum_b q2[b,0]}
 *   dq_c[b,0] = 2 (q_c[b,0] - y_b) / B - aw / (2B),  dq_c[b,j>0] = aw / (2B) * softmax_j,  aw = *alpha_w_dev (clipped alpha *
 *   conservative weight, device scalar).  y_dev NULL: sums only (the alpha update).  rows_scratch_dev: [B, 6] float32. */
int rl4rs_squashed_sample(int32_t N, int32_t rep, int32_t A, const float* head_dev, const float* eps_dev, float min_logstd,
                          float max_logstd, int32_t out_rep, int32_t out_off, float* act_out_dev, float* logp_out_dev, void* stream);
int rl4rs_sac_actor_grad(int32_t B, int32_t A, const float* head_dev, const float* eps_dev, const float* act_dev,
                         const float* g_act_dev, const float* log_temp_dev, float min_logstd, float max_logstd, float* d_head_dev,
                         void* stream);
int rl4rs_twin_min(int32_t B, const float* q1_dev, const float* q2_dev, float* qmin_dev, float* dq1_dev, float* dq2_dev, void* stream);
int rl4rs_cql_critic_loss(int32_t B, int32_t m, const float* q1_dev, const float* q2_dev, const float* offs_dev, const float* y_dev,
                          const float* alpha_w_dev, float* dq1_dev, float* dq2_dev, float* rows_scratch_dev, float* sums6_dev,
                          void* stream);

/* One whole BCQ update (d3rlpy BCQ._update: imitator step, critic step, actor step, soft target updates - the sequence of
 * rl4rs_amlp_* / rl4rs_cvae_* / rl4rs_residual_* / rl4rs_bcq_target / rl4rs_critic_mse calls rl4rs_amd/offline_rl.py::BCQ.update
 * makes, with the same arguments, as ONE host call: after the fused kernels an update was bound by the ~55 Python -> C calls it
 * takes, not by the GPU).  Single-process only: the data-parallel learner keeps the per-phase calls around its all-reduces.
 *   noise_dev      (B + B * n + B) * L floats of N(0, 1): eps [B, L] | z_target [B * n, L] | z_actor [B, L]; the two z parts are
 *                  clamped to +-0.5 IN PLACE (BCQImpl: the decoder's latent is clipped when actions are sampled)
 *   workspace_dev  rl4rs_bcq_workspace_floats(B, n, E, L) floats, 16-byte aligned
 *   metrics_dev    float[3] = {imitator loss, critic loss, actor loss} (entries of skipped phases are left alone)
 *   do_rl / do_actor   total_step >= rl_start_step / total_step % update_actor_interval == 0;  nograd_h16: the B * n target rows
 *                  through rl4rs_amlp_forward_h16 where the network and the row count allow (the learner's nograd_precision) */
typedef struct rl4rs_bcq_step {
    rl4rs_amlp *imit_enc, *imit_dec, *policy, *policy_targ, *q1, *q2, *q1_targ, *q2_targ;
    int32_t B, n, E, L;
    float beta, action_flexibility, lam, gamma, tau, imitator_lr, critic_lr, actor_lr;
    int32_t do_rl, do_actor, nograd_h16, h16_min_rows;
    const float *obs_dev, *act_dev, *rew_dev, *nxt_dev, *ter_dev;
    float* noise_dev;
    float* workspace_dev;
    float* metrics_dev;
} rl4rs_bcq_step;
int64_t rl4rs_bcq_workspace_floats(int32_t B, int32_t n, int32_t E, int32_t L);
int rl4rs_bcq_update(const rl4rs_bcq_step* step, void* stream);

/* One whole continuous-CQL update (d3rlpy CQL._update as 'CQL-conti' runs it: temperature step, alpha step, critic step with the
 * conservative term over m = 1 + 3 n rows per transition, actor step, soft critic-target updates) as ONE host call - the sequence
 * rl4rs_amd/offline_rl.py::CQL.update issues, with the two learned scalars' Adam on the device.  Single-process only.
 *   log_temp / log_alpha   device float[3] each = {value, Adam m, Adam v}; *_step = the number of Adam steps taken so far (host)
 *   normal_dev   N(0, 1): eps_temp [B, A] | alpha eps_t [B n, A] | alpha eps_tp1 [B n, A] | critic eps_t | critic eps_tp1 | eps_actor [B, A]
 *   uniform_dev  U[-1, 1): alpha [B, n, A] | critic [B, n, A]
 *   rew_dev      rewards as the critic sees them (the caller applies the reward scaler)
 *   workspace_dev  rl4rs_cql_workspace_floats(B, n, A) floats, 16-byte aligned;  metrics_dev float[4] = {critic, actor, temp, alpha loss} */
typedef struct rl4rs_cql_step {
    rl4rs_amlp *policy, *q1, *q2, *q1_targ, *q2_targ;
    int32_t B, n, A;
    float gamma, tau, actor_lr, critic_lr, temp_lr, alpha_lr, alpha_threshold, conservative_weight;
    int32_t nograd_h16, h16_min_rows;
    int64_t temp_step, alpha_step;
    float* log_temp_dev;
    float* log_alpha_dev;
    const float *obs_dev, *act_dev, *rew_dev, *nxt_dev, *ter_dev;
    const float* normal_dev;
    const float* uniform_dev;
    float* workspace_dev;
    float* metrics_dev;
} rl4rs_cql_step;
int64_t rl4rs_cql_workspace_floats(int32_t B, int32_t n, int32_t A);
int rl4rs_cql_update(const rl4rs_cql_step* step, void* stream);

/* COMBO (d3rlpy.algos.COMBO, 'COMBO' of script/batchrl_trainer.py:130-151: SAC + a conservative critic term over a minibatch of
 * n_real real rows followed by F = B - n_real model-generated rows; d3rlpy absent, PARITY UNPINNED).  The critic step runs two
 * passes through the twin critics: pass T = the B rows (s, a) (rep = 1), pass C = the F * k sample rows of the generated
 * observations (k = 3 n_action_samples, rep = k); csrc/combo.hpp says why.
 * amlp_grad_stash: the join of the two passes (rl4rs_amlp_backward WRITES a handle's flat gradient).  For n <= 4 handles in ONE
 * launch: mode 0 copies each handle's flat gradient to bufs_dev[i] (its parameter count floats), mode 1 adds bufs_dev[i] into it. */
int rl4rs_amlp_grad_stash(int32_t n, rl4rs_amlp* const* nets, float* const* bufs_dev, int32_t mode, void* stream);
/* combo_critic_loss: both gradient sets and the six sums of the critic loss
 *     sum_c mean_b (q_c[b] - y_b)^2 + w [ sum_c mean_f logsumexp_j (q_c[f,j] - offs[f,j]) - sum_c mean_{b < n_real} q_c[b] ].
 *   pass-T half  q*t_dev, y_dev [B] -> dq*t_dev [B] = 2 (q - y) / B - [b < n_real] w / n_real   (one thread per row)
 *   pass-C half  q*c_dev, offs_dev [F, k] -> dq*c_dev [F, k] = (w / F) softmax_j                  (one wave per generated row)
 *   sums6_dev = {sum_b (q1 - y)^2, same for q2, sum_f logsumexp for q1, for q2, sum_{b < n_real} q1, same for q2}, reduced in a
 *   fixed order (no atomics) from rows_scratch_dev [4 B + 2 F].
 * Either half may be left out by passing ALL of its pointers NULL: a forward of pass C overwrites the activations pass T's backward
 * needs, so an update calls the T half after forward T and the C half after forward C with the SAME rows_scratch_dev; the sums are
 * written by the call that has the C half.  w_dev: the conservative weight, a device scalar.  n_real <= 0, n_real >= B and k < 1
 * are refused (d3rlpy's mean over an empty half is NaN), each with its own message, before anything touches a device. */
int rl4rs_combo_critic_loss(int32_t B, int32_t n_real, int32_t k, const float* q1t_dev, const float* q2t_dev, const float* y_dev,
                            const float* q1c_dev, const float* q2c_dev, const float* offs_dev, const float* w_dev, float* dq1t_dev,
                            float* dq2t_dev, float* dq1c_dev, float* dq2c_dev, float* rows_scratch_dev, float* sums6_dev, void* stream);
/* One whole COMBO update as ONE host call: target, critic step (forward T, backward T, stash, forward C, backward C, add, Adam) and,
 * when do_actor (total_step % update_actor_interval == 0), the SAC actor step, the temperature step on the STEPPED policy and the
 * soft critic-target update - the sequence rl4rs_amd/offline_rl.py::COMBO.update issues.  Single-process only.  Rows 0 .. n_real - 1
 * of the five transition columns are real, the rest generated.
 *   log_temp_dev   device float[3] = {value, Adam m, Adam v}; temp_step = the number of its Adam steps so far (host)
 *   normal_dev     N(0, 1), 16-byte aligned: eps_t [F n, A] | eps_tp1 [F n, A] | eps_actor [B, A] | eps_temp [B, A]
 *   uniform_dev    U[-1, 1): [F, n, A]
 *   rew_dev        rewards as the critic sees them (the caller applies the reward scaler)
 *   stash_dev      2 * round_up(critic parameter count, 4) floats, 16-byte aligned: pass T's gradients while pass C runs
 *   workspace_dev  rl4rs_combo_workspace_floats(B, n_real, n, A) floats (-1: bad sizes), 16-byte aligned
 *   metrics_dev    float[4] = {critic loss, actor loss, temp loss, conservative term} (entries of skipped phases are left alone)
 * Refused with a message each, before any device is needed: n_real <= 0, n_real >= B, n < 1, a null handle, a misaligned workspace. */
typedef struct rl4rs_combo_step {
    rl4rs_amlp *policy, *q1, *q2, *q1_targ, *q2_targ;
    int32_t B, n_real, n, A;
    float gamma, tau, actor_lr, critic_lr, temp_lr, conservative_weight;
    int32_t do_actor, reserved;
    int64_t temp_step;
    float* log_temp_dev;
    const float *obs_dev, *act_dev, *rew_dev, *nxt_dev, *ter_dev;
    const float* normal_dev;
    const float* uniform_dev;
    float* stash_dev;
    float* workspace_dev;
    float* metrics_dev;
} rl4rs_combo_step;
int64_t rl4rs_combo_workspace_floats(int32_t B, int32_t n_real, int32_t n, int32_t A);
/* where the last update left its target y [B] (what = 0) and the six sums of rl4rs_combo_critic_loss (what = 1): offsets in floats
 * into workspace_dev (tests, tools); -1: bad sizes / what */
int64_t rl4rs_combo_workspace_offset(int32_t B, int32_t n_real, int32_t n, int32_t A, int32_t what);
int rl4rs_combo_update(const rl4rs_combo_step* step, void* stream);

/* ------------------------------------------------------------------------------------------------
 * On-device TD3 / DDPG on the continuous-action env: script/modelfree_train.py:46-48,79-105 (algo "TD3" / "DDPG" with
 * support_conti_env; rl4rs/env/base.py:214-215 Box(-1, 1) of action_emb_size values, resolved by the env's masked K-NN).  RLlib
 * 1.5.1's ddpg_tf_policy / ddpg_tf_model / OrnsteinUhlenbeckNoise are restated from their published form (ray is absent: PARITY
 * UNPINNED, checked against the fp64 restatement of tests/td3_ref.py).  The reference driver's DDPG branch is an `if` in front of
 * a separate `if TD3 / elif ... / else: raise` chain, so algo "DDPG" raises there; DDPG here is TD3 with the twin critic, the
 * policy delay and the target smoothing off.
 * Networks: two kinds of rl4rs_amlp.  Actor obs -> Dense relu -> Dense relu -> Dense(E), then RLlib's sigmoid(2x) * (high - low)
 * + low, which on Box(-1, 1) is tanh(x): head_act tanh, act_dim 0.  Critics cat([obs, action]) -> relu -> relu -> 1.
 * ---------------------------------------------------------------------------------------------- */
/* RLlib OrnsteinUhlenbeckNoise on a deterministic action det_action_dev [N, E]:
 *   eps ~ N(0, 1) by Box-Muller on the policy net's counter RNG keyed (seed, step, state row, column); written to eps_out_dev
 *   [N, E] when that is not NULL
 *   ou_state += theta * (-ou_state) + sigma * eps
 *   action = clip(det_action + scale * ou_state * (high - low), -1, 1), high - low = 2; scale = ou_base_scale * the annealed scale
 * random_phase 1 (RLlib random_timesteps): action = 2u - 1 with u uniform from the same RNG keyed (seed, step, row, column); the
 * state does not advance and eps_out_dev is not written.
 * state_rows N: ou_state_dev [N, E], one state per row.  state_rows 1: ou_state_dev [E] is shared by all rows (RLlib's single
 * variable shaped like one action): eps is keyed by column only and the state advances once per call, not once per row. */
int rl4rs_explore_ou(int32_t N, int32_t E, int32_t state_rows, const float* det_action_dev, float* ou_state_dev, float theta,
                     float sigma, float scale, uint32_t seed, uint32_t step, int32_t random_phase, float* action_out_dev,
                     float* eps_out_dev, void* stream);
/* TD3 target-policy smoothing: out = clip(action + clip(target_noise * eps, -noise_clip, noise_clip), -1, 1); eps_dev [N, E] is
 * the caller's N(0, 1).  out_dev may be action_dev. */
int rl4rs_td3_smooth_action(int32_t N, int32_t E, const float* action_dev, const float* eps_dev, float target_noise,
                            float noise_clip, float* out_dev, void* stream);
/* RLlib ddpg_tf_policy's critic loss.  q' = min(q1_targ, q2_targ) (q2_targ_dev NULL: q1_targ); y = r for a terminal row
 * (dones_dev int32 != 0) and r + gamma * q' otherwise - a select, so nothing of a terminal row's target Q (NaN included) reaches
 * any output; td_c = q_c - y; per-row error huber(td1, threshold) + huber(td2, threshold) (use_huber) or 0.5 td1^2 + 0.5 td2^2
 * (q2_dev / dq2_dev NULL: the single critic's one term); loss = mean(w * error), w = weights_dev or 1; dq_c = its gradient wrt q_c.
 * y_out_dev / td_out_dev (optional) [N]: y and the FIRST critic's td (what the priorities use).  stats4_dev (optional) = sums of
 * {w * error, q1, y, |td1|}; one workgroup, fixed order: bit-identical from run to run. */
int rl4rs_td3_critic_loss(int32_t N, const float* q1_dev, const float* q2_dev, const float* q1_targ_dev, const float* q2_targ_dev,
                          const float* rewards_dev, const int32_t* dones_dev, const float* weights_dev, float gamma,
                          int32_t use_huber, float huber_threshold, float* dq1_dev, float* dq2_dev, float* y_out_dev,
                          float* td_out_dev, float* stats4_dev, void* stream);
/* d_pre = d_out * (1 - tanh_out^2): the gradient wrt a tanh head's pre-activation (what rl4rs_amlp_backward takes) */
int rl4rs_tanh_head_grad(int32_t N, int32_t E, const float* tanh_out_dev, const float* d_out_dev, float* d_pre_dev, void* stream);
/* grad += l2 * W on the three weight matrices of the handle's gradient, biases untouched: the gradient of RLlib's
 * l2_reg * tf.nn.l2_loss(var) over the non-bias variables.  l2 = 0: nothing is launched. */
int rl4rs_amlp_add_l2(rl4rs_amlp* net, float l2, void* stream);

/* One whole TD3 / DDPG update as ONE host call; both gradients come from the parameters BEFORE the step, as in RLlib's TF policy:
 *   1. a' = actor_targ(s'), smoothed with noise_dev [M, E] (N(0, 1)) when smooth_target_policy
 *   2. q' from the target critics on (s', a')                                            (one rl4rs_amlp_forward_multi)
 *   3. q1, q2 on (s, a), rl4rs_td3_critic_loss, backward of both critics, L2 on both
 *   4. do_actor: a_pi = actor(s); q1(s, a_pi) forward, backward with dout = -1 / M for the action gradient only; tanh head; actor
 *      backward; L2 on the actor
 *   5. ONE rl4rs_amlp_adam_multi for {q1, q2, actor} (the actor steps only when do_actor) with the soft updates of ALL THREE targets
 *      (RLlib update_target at target_network_update_freq 0: the actor's target moves even when the actor did not step); Adam
 *      beta 0.9 / 0.999, eps 1e-7 (tf.keras's value, in rl4rs_amlp_adam_step's form)
 * q2 / q2_targ NULL: DDPG's single critic.  weights_dev NULL: 1.  td_out_dev [M]: the first critic's TD errors.
 * metrics_dev float[6] = {sum w * error, sum q1, sum y, sum |td1|, -sum q1(s, a_pi) (written only when do_actor), spare}; the L2
 * terms are not part of them.  workspace_dev: rl4rs_td3_workspace_floats(M, E) floats, 16-byte aligned.  Single process only:
 * the data-parallel trainer issues the same sequence as per-phase calls around its all-reduce. */
typedef struct rl4rs_td3_step {
    rl4rs_amlp *actor, *actor_targ, *q1, *q2, *q1_targ, *q2_targ;
    int32_t M, E;
    float gamma, tau, actor_lr, critic_lr, target_noise, target_noise_clip, l2_reg, huber_threshold;
    int32_t smooth_target_policy, use_huber, do_actor, reserved;
    const float *obs_dev, *act_dev, *rew_dev;
    const int32_t* done_dev;
    const float *nxt_dev, *weights_dev, *noise_dev;
    float* workspace_dev;
    float* td_out_dev;
    float* metrics_dev;
} rl4rs_td3_step;
int64_t rl4rs_td3_workspace_floats(int32_t M, int32_t E);
int rl4rs_td3_update(const rl4rs_td3_step* step, void* stream);

/* Plain fp32 GEMM used by the scorer, exposed for tests: C[M,N] = act(A[M,K] @ W[K,N] + bias).
 * act: 0 none, 1 ELU, 2 sigmoid, 3 tanh, 4 ReLU. */
int rl4rs_gemm_f32(const float* a_dev, int64_t lda, const float* w_dev, int64_t ldw,
                   const float* bias_dev, float* c_dev, int64_t ldc, int32_t M, int32_t N, int32_t K,
                   int act, void* stream);

/* Same GEMM through the pre-packed-weight kernel the scorer uses (w_host is a HOST pointer; packs, uploads,
 * runs and synchronises: test entry point only). */
int rl4rs_gemm_f32_packed(const float* a_dev, int64_t lda, const float* w_host, int64_t ldw,
                          const float* bias_dev, float* c_dev, int64_t ldc, int32_t M, int32_t N, int32_t K,
                          int act, void* stream);

/* The fp16x2 form of that GEMM (scorer_mode RL4RS_SCORER_FP16X2: operands as fp16 hi + lo pairs, three f16 MFMAs per
 * product, fp32 accumulation; an activation outside the fp16 range turns its output row into NaN).  Test entry point. */
int rl4rs_gemm_h16_packed(const float* a_dev, int64_t lda, const float* w_host, int64_t ldw,
                          const float* bias_dev, float* c_dev, int64_t ldc, int32_t M, int32_t N, int32_t K,
                          int act, void* stream);
/* Test hook: the device-side fragment packer (k_pack_h16_dev, used in front of rl4rs_amlp_forward_h16) against the host one
 * (pack_gemm_weight_h16, used when a scorer is loaded): number of 32-bit words that differ, 0 = bit-identical. */
int rl4rs_pack_h16_selftest(const float* w_host, int64_t ldw, int32_t K, int32_t N, int64_t* mismatches, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Off-policy evaluation: the estimators of rl4rs/utils/offline_policy_metrics.py:8-184 over the per-step log that
 * script/offline_evaluation.py:16-36 (ope_eval) collects, and the propensity rules of rl4rs/policy/policy_model.py:75-83 and
 * rl4rs/policy/behavior_model.py:44-58.  The reference pulls a [B, A] probability matrix to the host at every step and runs its
 * numpy passes over [B, T] arrays per epoch; here one step's record is a few [B] columns written into a [T, B] float64 log
 * owned by the handle, and one epoch's estimate is four launches that end in one vector of float64 statistics.  All arithmetic
 * is float64; sums over episodes are reduced per wave, per block, then over the block partials in a fixed order (no atomics): the
 * result is bit-identical from run to run and the same for the handle and the array forms.  Variances are two-pass.
 * ---------------------------------------------------------------------------------------------- */

typedef struct rl4rs_ope rl4rs_ope;

/* columns of the handle's log, each [T, B] float64 */
enum {
    RL4RS_OPE_COL_PI = 0,         /* evaluated policy's probability of the logged action   offline_evaluation.py:27-30 */
    RL4RS_OPE_COL_MU = 1,         /* logged policy's probability of the logged action      offline_evaluation.py:31-32 */
    RL4RS_OPE_COL_Q = 2,          /* policy.predict_q(obs, action)                         offline_evaluation.py:29 */
    RL4RS_OPE_COL_REWARD = 3,     /* the simulator's reward of the evaluated action        offline_evaluation.py:33,35 */
    RL4RS_OPE_COL_LOGGED_REWARD = 4, /* eval_env.offline_reward                            offline_evaluation.py:34 */
    RL4RS_OPE_N_COLS = 5
};

/* slots of the statistics vector (host double[RL4RS_OPE_N_STATS]); a slot whose inputs were not given is NaN */
enum {
    RL4RS_OPE_CIPS = 0,           /* eval_CIPS: E_t over ratios clipped to [0.1, 10]       offline_policy_metrics.py:69-94 */
    RL4RS_OPE_CIPS_C = 1,         /*   its confidence half-width cv * stddev / sqrt(int(n_e)) */
    RL4RS_OPE_IPS = 2,            /* eval_IPS (unclipped ratios, their own n_e and cv)     offline_policy_metrics.py:47-66 */
    RL4RS_OPE_IPS_C = 3,
    RL4RS_OPE_SNIPS = 4,          /* eval_SNIPS                                            offline_policy_metrics.py:97-122 */
    RL4RS_OPE_SNIPS_C = 5,
    RL4RS_OPE_DR = 6,             /* eval_doubly_robust: mean(dr) / mean(rewards)          offline_policy_metrics.py:145-162 */
    RL4RS_OPE_DR_SE = 7,          /*   scipy.stats.sem(dr) (ddof = 1; NaN for one episode) */
    RL4RS_OPE_WIPS = 8,           /* eval_WIPS(gamma)                                      offline_policy_metrics.py:125-142 */
    RL4RS_OPE_WIPS_2 = 9,         /*   the reference's constant second element, 0 */
    RL4RS_OPE_SEQDR = 10,         /* eval_seq_doubly_robust                                offline_policy_metrics.py:165-184 */
    RL4RS_OPE_SEQDR_2 = 11,       /*   0 */
    RL4RS_OPE_N_E = 12,           /* effective sample size of the clipped ratios           offline_policy_metrics.py:34 */
    RL4RS_OPE_CV = 13,            /* t.ppf(1 - 0.00125, int(n_e) - 1) for it               offline_policy_metrics.py:37-38 */
    RL4RS_OPE_N_E_RAW = 14,       /* the same two for the unclipped ratios (eval_IPS) */
    RL4RS_OPE_CV_RAW = 15,
    RL4RS_OPE_SIM_REWARD = 16,    /* mean over episodes of the summed simulator reward     offline_evaluation.py:38-39 */
    RL4RS_OPE_N_STATS = 17
};

/* scipy.stats.t.ppf(p, df) (offline_policy_metrics.py:38): quantile of Student's t, host arithmetic (regularised incomplete
 * beta, bisection); NaN for df <= 0 or p outside [0, 1] like scipy, and for df = +inf (scipy: the normal quantile; the
 * estimators never get there, df < 2^28).  Needs no device. */
double rl4rs_student_t_ppf(double p, double df);

/* A log for up to max_batch episodes of up to max_steps steps (max_steps <= 256: one lane walks an episode's steps). */
int rl4rs_ope_create(int32_t max_batch, int32_t max_steps, rl4rs_ope** out);
int rl4rs_ope_destroy(rl4rs_ope* h);
/* Start an epoch of B episodes x T steps (offline_evaluation.py:17-20): forgets what was recorded. */
int rl4rs_ope_begin(rl4rs_ope* h, int32_t B, int32_t T);

/* pi[t, b] from the learner's score matrix scores_dev [B, A] float32 (row stride ld floats) and the logged action action_dev [B]
 * int32 (offline_evaluation.py:27-28: action_prob[range(batch_size), off_action]).  is_logits = 0: the scores are probabilities,
 * taken as they are; 1: Q values / logits, pi = softmax(scores[b])[a] (policy_model.py:78-82) computed per row in float64
 * without the [B, A] softmax.  An action outside [0, A) gives NaN (the reference raises IndexError). */
int rl4rs_ope_record_policy(rl4rs_ope* h, int32_t t, const float* scores_dev, int32_t A, int64_t ld, const int32_t* action_dev,
                            int32_t is_logits, void* stream);
/* mu[t, b] = y[b, lo + clip(a - lo, 0, hi - lo - 1)] / sum(y[b, lo:hi]) from a behaviour score matrix y_dev [B, A_b] float32
 * (behavior_model.py:49-58; the caller maps `layer` to [lo, hi)).  is_logits = 1: exp(y_a - m) / sum_{[lo, hi)} exp(y - m), m the
 * maximum over the range: a full softmax followed by the reference's renormalisation, without the intermediate. */
int rl4rs_ope_record_behavior(rl4rs_ope* h, int32_t t, const float* y_dev, int32_t A_b, int64_t ld, int32_t lo, int32_t hi,
                              const int32_t* action_dev, int32_t is_logits, void* stream);
/* Column `col` (RL4RS_OPE_COL_*) of step t from a device array src_dev [B], float32 (src_is_f64 = 0) or float64 (1). */
int rl4rs_ope_record_column(rl4rs_ope* h, int32_t t, int32_t col, const void* src_dev, int32_t src_is_f64, void* stream);
/* Q[t, b] = scores_dev[b, action_dev[b]] (AlgoBase.predict_value of a discrete Q learner, policy_model.py:55-61) */
int rl4rs_ope_record_q(rl4rs_ope* h, int32_t t, const float* scores_dev, int32_t A, int64_t ld, const int32_t* action_dev,
                       void* stream);
/* Device address of one column's [T, B] float64 log (T, B of the last rl4rs_ope_begin). */
int rl4rs_ope_log(rl4rs_ope* h, int32_t col, double** dev_out, int64_t* n_out);
/* Step t of column col was written through rl4rs_ope_log's address (+ t * B) by the caller - rl4rs_ope_greedy_rows /
 * rl4rs_policy_ope_step take such addresses as pi_dev and q_dev: rl4rs_ope_estimate counts it as recorded.  Host state only. */
int rl4rs_ope_mark_recorded(rl4rs_ope* h, int32_t t, int32_t col);

/* One epoch's estimators from the log, assembled like offline_evaluation.py:38-67: the per-episode products of probs * 100, the
 * summed logged reward, the summed simulator reward as DR's action_rhat_rewards and the per-episode mean Q as its
 * state_rewards.  Waits for `stream`; stats_host double[RL4RS_OPE_N_STATS].  Slots whose columns are incomplete are NaN. */
int rl4rs_ope_estimate(rl4rs_ope* h, double gamma, double* stats_host, void* stream);

/* The same estimators on caller-supplied float64 device arrays, without a handle (they allocate their scratch).
 * Per-episode arrays [B]: eval_IPS / eval_CIPS / eval_SNIPS(rewards, policy_prob, behavior_prob) and
 * eval_doubly_robust(action_rhat_rewards, state_rewards, rewards, ...); rhat_dev / state_dev may be NULL (DR slots NaN). */
int rl4rs_ope_episode_stats(int32_t B, const double* rewards_dev, const double* policy_prob_dev, const double* behavior_prob_dev,
                            const double* rhat_dev, const double* state_dev, double* stats_host, void* stream);
/* Per-step arrays [B, T] row-major: eval_WIPS(step_rewards, policy_prob, behavior_prob, gamma) and
 * eval_seq_doubly_robust(action_rhat_rewards, state_rewards, rewards = step_rewards, ...); rhat / state may be NULL. */
int rl4rs_ope_step_stats(int32_t B, int32_t T, const double* step_rewards_dev, const double* policy_prob_dev,
                         const double* behavior_prob_dev, const double* rhat_dev, const double* state_dev, double gamma,
                         double* stats_host, void* stream);

/* One OPE step of a score-matrix policy: what ope_eval needs of the evaluated policy per episode (offline_evaluation.py:24-29,
 * policy_model.py:43-87, RLlib-trainer branch), one launch, no handle.
 * One wave per row, four rows per workgroup.  m[c] = scores[b, c], or for a column the mask forbids
 *   mask_set 0: scores[b, c] + (-3.4028235e38f) in float32 (the mask-model rule, as k_greedy_rows / rl4rs_policy_evaluate form it)
 *   mask_set 1: -3.4028235e38f                              (the Rainbow rule)
 * actions[b] = first maximum of m (a row that allows nothing: 0)
 * pi[b]      = exp(m[l] - max) / sum_c exp(m[c] - max) in float64, l = logged[b]; l outside [0, A): NaN
 * q[b]       = value_dev ? (double)value_dev[b * value_ld] : (double)m[actions[b]]
 * masked_out (optional, [N, A] float32) receives m: what the tests recompute everything from.
 * mask_bits_dev (optional): (A + 31) / 32 words per row, bit c of a row = column c is allowed.  pi_dev, q_dev, logged_dev are
 * optional (pi_dev needs logged_dev).  A row of up to 4092 columns is read from memory once; a longer one twice. */
int rl4rs_ope_greedy_rows(int32_t N, const float* scores_dev, int32_t A, int64_t ld, const uint32_t* mask_bits_dev, int32_t mask_set,
                          const int32_t* logged_dev, const float* value_dev, int64_t value_ld, int32_t* actions_dev,
                          double* pi_dev, double* q_dev, float* masked_out_dev, void* stream);

/* ---- Offline scorers (d3rlpy 0.91 metrics/scorer.py as published - parity unpinned; rl4rs/utils/d3rlpy_scorer.py) ----
 *
 * One pass over evaluation episodes: the caller runs each network once per row and hands the score rows to rl4rs_score_rows, which
 * writes the few scalars every scorer needs; rl4rs_score_episodes turns those columns into every score at once.
 *
 * rl4rs_score_rows: one wave per row, four rows per workgroup; scores_dev [N, A] float32 with row stride ld (Q values, or the
 * imitator's logits for a learner without Q).  A row (and its imitator row) of up to 4096 floats together is read from memory once.
 *   a_pi[n]   the learners' greedy rule (rl4rs_q_best_action's own device function): first maximum of the row, or the BCQ rule
 *             when imitator_dev [N, A] (row stride imitator_ld) and action_flexibility are given
 *   qp[n]     scores[n, a_pi[n]]
 *   qd[n]     scores[n, logged[n]]; a logged action outside [0, A) gives NaN
 *   a_mask[n] rl4rs_env_predict_with_mask on the same row: the catalogue tables of `env`, the previous actions and cur_step taken
 *             from the last page_items + 1 columns of the observation row obs_dev[n * obs_ld .. + obs_dim), converted by truncation
 * Every output is optional (NULL); qd needs logged_dev, a_mask needs env and obs_dev. */
int rl4rs_score_rows(int32_t N, const float* scores_dev, int32_t A, int64_t ld, const float* imitator_dev, int64_t imitator_ld,
                     float action_flexibility, const int32_t* logged_dev, const rl4rs_env* env, const float* obs_dev, int32_t obs_dim,
                     int64_t obs_ld, float* qd_dev, int32_t* a_pi_dev, float* qp_dev, int32_t* a_mask_dev, void* stream);
/* diff[n] = sum_k (actions[n, k] - predicted[n, k])^2 in float64 (continuous_action_diff_scorer); both [N, E] float32, contiguous */
int rl4rs_score_action_diff(int32_t N, int32_t E, const float* actions_dev, const float* predicted_dev, double* diff_dev, void* stream);

/* The per-transition columns of a pass, device arrays of `rows` entries; any may be NULL (the slots that need it are NaN). */
typedef struct rl4rs_score_cols {
    const float* qd;       /* Q(o, a), reverse-transformed by the caller where the learner has a reward scaler */
    const float* qp;       /* Q(o, pi(o)) */
    const float* qn;       /* Q(o', pi(o')) */
    const float* r_td;     /* next reward on the scale the critic was trained on */
    const float* r_raw;    /* next reward as logged */
    const float* ter;      /* terminal flag */
    const int32_t* a;      /* logged action */
    const int32_t* a_pi;   /* predict(o) */
    const int32_t* a_mask; /* predict_with_mask(o) */
    const double* diff;    /* rl4rs_score_action_diff */
} rl4rs_score_cols;
enum {
    RL4RS_SCORE_TD_ERROR = 0,          /* mean (qd - (r_td + gamma qn (1 - ter)))^2                       td_error_scorer */
    RL4RS_SCORE_DSA = 1,               /* mean S, S_last = adv, S_j = adv_j + gamma S_{j+1} inside each window of 1024 rows of an
                                          episode, adv = qd - qp                                           discounted_sum_of_advantage_scorer */
    RL4RS_SCORE_AVG_VALUE = 2,         /* mean qp                                                         average_value_estimation_scorer */
    RL4RS_SCORE_INIT_VALUE = 3,        /* mean over episodes of qp at the episode's first row            initial_state_value_estimation_scorer */
    RL4RS_SCORE_SOFT_OPC = 4,          /* mean qd over rows of episodes with return >= threshold - mean qd; NaN when none succeeds */
    RL4RS_SCORE_ACTION_MATCH = 5,      /* mean [a_pi == a]                                                d3rlpy's discrete_action_match_scorer */
    RL4RS_SCORE_ACTION_MATCH_MASK = 6, /* mean [a_mask == a]                                              the reference's */
    RL4RS_SCORE_ACTION_DIFF = 7,       /* mean diff                                                       continuous_action_diff_scorer */
    RL4RS_SCORE_N_ROWS = 8,
    RL4RS_SCORE_N_EPISODES = 9,
    RL4RS_SCORE_N_SUCCESS_ROWS = 10,   /* rows of successful episodes (NaN without a threshold) */
    RL4RS_SCORE_N_STATS = 11
};
/* Every score of E episodes at once: episode e is rows [starts[e], starts[e + 1]) of the columns (starts_dev int64 [E + 1],
 * clamped to [0, rows]).  One lane walks an episode of any length: its return (the float64 sum of r_raw), the success flag, the
 * first-row value and the backward scan with its 1024-row restarts, all float64; then a fixed-order float64 reduction (lane, wave,
 * block, blocks in order - no float atomics), so two runs give the same bytes.  Waits for `stream`; stats_host
 * double[RL4RS_SCORE_N_STATS].  A slot whose columns were not supplied is NaN. */
int rl4rs_score_episodes(int32_t E, const int64_t* starts_dev, int64_t rows, const rl4rs_score_cols* cols, double gamma,
                         int32_t has_threshold, double threshold, double* stats_host, void* stream);

/* ---- On-device Exact-K (rl4rs/nets/exact_k, script/exact_k_train.py): the pointer-network slate generator and its critic ----
 *
 * Generator: enc_user = relu(obs W + b) [hidden]; enc[n, a] = dropout(concat(enc_user[n], item_table[a] * sqrt(hidden))) over the
 * ONE shared candidate list 0..action_size-1 (both reference scripts feed the identity list; only the first action_size table rows
 * are used and trained); `blocks` blocks of multi-head self-attention (relu Q / K / V, key and query masking on an exactly-zero row
 * sum, dropout on the probabilities, residual, layer norm with population variance and eps 1e-8 under the root) + feed-forward
 * (D -> 4 hidden relu -> D, residual, layer norm), D = 2 hidden; TF LSTMCell(D) pointer decoder with trainable initial state and
 * first input, intra-attention over the earlier cell outputs, one glimpse over all candidates and the pointer scores; candidates
 * outside the allowed set of step t get -2^32 + 1:  allowed = not yet picked, in location_mask[t / 3], and no special item once a
 * special item has been picked (the env's own action mask).  Slate length 9.
 *
 * Flat parameter layout (float32):
 *   user W [obs_dim, H], b [H] | item table [vocab, H] |
 *   per block: Wq [D, D], bq, Wk, bk, Wv, bv | ln1 gamma, beta | W1 [D, 4H], b1 | W2 [4H, D], b2 | ln2 gamma, beta |
 *   LSTM kernel [2D, 4D] (gates i, j, f, o), bias [4D] | init c [D], init h [D], first input [D] |
 *   intra: W_b [D, D], v_dec [D], W_bef [D, D], bias_dec [D] |
 *   glimpse: W_q [D, D], W_dec [D, D], v [D], bias [D], W_ref [D, D] | pointer: the same five.
 *
 * Dropout keep masks are a pure function of the policy net's counter RNG: an element is kept when
 *   uniform01(seed, step, row, site * 65536 + col) >= rate   and then scaled by 1 / (1 - rate),
 * site = 32 * pass + 0 for enc (row = n * A + a, col = feature) and 32 * pass + 1 + block for the attention probabilities
 * (row = (n * heads + head) * A + query, col = key); pass = 0 in rl4rs_exactk_loss_grad and 1 in rl4rs_exactk_decode, so a rollout
 * and the update draw different masks from the same (seed, step).  Dropout is on in every call, greedy decoding included (the
 * reference builds its generator with is_training = True for its eval stage too).
 *
 * Refused by rl4rs_exactk_create (and rl4rs_exactk_param_count = -1), before a device is looked for: hidden not a multiple of 16,
 * a head width D / heads that is not a multiple of 8, action_size > vocab, a max_rows whose [max_rows * action_size, 4 hidden] fp32
 * activations (or, for small action_size, the decoder's [9 * max_rows, 8 hidden] gates) reach 2^31 bytes, shapes whose kernels need more than 160 KiB of LDS, and a location mask with fewer than 9 allowed
 * non-special items (9 keep every position's allowed set non-empty). */
typedef struct rl4rs_exactk rl4rs_exactk;
typedef struct rl4rs_exactk_critic rl4rs_exactk_critic;
typedef struct rl4rs_exactk_cfg {
    int32_t obs_dim, hidden /* H */, heads, blocks, action_size /* A */, vocab, max_rows;
    float dropout_rate;
} rl4rs_exactk_cfg;
int64_t rl4rs_exactk_param_count(const rl4rs_exactk_cfg* cfg);
/* location_mask_host uint8 [3, A], is_special_host uint8 [A] */
int rl4rs_exactk_create(const rl4rs_exactk_cfg* cfg, const float* params_host, const uint8_t* location_mask_host,
                        const uint8_t* is_special_host, void* stream, rl4rs_exactk** out);
int rl4rs_exactk_destroy(rl4rs_exactk* net);
int rl4rs_exactk_params(rl4rs_exactk* net, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_exactk_adam_state(rl4rs_exactk* net, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_exactk_set_adam_step(rl4rs_exactk* net, int64_t step);
/* A slate per row from obs_dev [N, obs_dim] -> path_dev int32 [N, 9] (candidate indices).  greedy = 0: one inverse-CDF draw per
 * step from softmax(logits): the smallest allowed a whose inclusive prefix sum of exp(logit - max), in candidate order, exceeds
 * u * total, u = uniform01(seed, step, row, t); greedy = 1: the first maximum.  logits_out_dev [N, 9, A] optional. */
int rl4rs_exactk_decode(rl4rs_exactk* net, int32_t N, const float* obs_dev, int32_t greedy, uint32_t seed, uint32_t step,
                        int32_t* path_dev, float* logits_out_dev, void* stream);
/* Beam search over the pointer decoder: path_dev int32 [N, beam, 9], score_dev float [N, beam] (sum of the 9 log-probabilities,
 * descending; ties by parent * A + token).  Optional trace, each [N, 9, beam]: parent_dev int32 (index of the beam of step t - 1
 * that beam k of step t extends; 0 at t = 0), token_dev int32, step_score_dev float.  Dropout pass 1, masks of rl4rs_exactk_decode.
 * The beams of a row share the encoder output; each carries its own LSTM state, intra-attention history and prefix, hence its own
 * allowed set.  Step t scores every allowed candidate a of every live beam b as acc[b] + logit[b, a] - logsumexp_allowed(logit[b, :])
 * and keeps the best `beam`; one beam is live at step 0, so the first picks are distinct.  1 <= beam <= 8.  The per-beam decoder
 * arrays are the handle's own, allocated on the first call (and again by a call with a larger N * beam), apart from what the other
 * calls use.  Refused: beam outside [1, 8], N outside [1, max_rows], a null path_dev / score_dev, a (beam, action_size, hidden)
 * whose per-user kernels need more than 160 KiB of LDS. */
int rl4rs_exactk_decode_beam(rl4rs_exactk* net, int32_t N, const float* obs_dev, int32_t beam, uint32_t seed, uint32_t step,
                             int32_t* path_dev, float* score_dev, int32_t* parent_dev, int32_t* token_dev, float* step_score_dev,
                             void* stream);
/* Teacher-forced forward along path_dev [N, 9], loss = mean_n(w_n * sum_t CE(logits[n, t], path[n, t])) and its full gradient into
 * the handle's flat gradient buffer (bit-identical between identical calls).  loss_dev float[2] = {loss, number of (row, step)
 * targets outside the allowed set (such a path is the caller's error; indices are clamped into range)}. */
int rl4rs_exactk_loss_grad(rl4rs_exactk* net, int32_t N, const float* obs_dev, const int32_t* path_dev, const float* weights_dev,
                           uint32_t seed, uint32_t step, float* logits_out_dev, float* loss_dev, void* stream);
/* Adam in tf.train.AdamOptimizer's form on the handle's gradient.  skip_dev (optional) int32[1] on the device: non-zero = leave
 * parameters and moments alone (the step counter still advances). */
int rl4rs_exactk_adam_step(rl4rs_exactk* net, float lr, float beta1, float beta2, float eps, const int32_t* skip_dev, void* stream);
/* Critic (the reference's Discriminator): obs -> hidden relu -> hidden relu -> hidden relu -> 1; flat layout W1, b1, W2, b2, W3, b3,
 * W4 [hidden, 1], b4.  loss_grad: the gradient of the SUM over rows of (value - target)^2 (TF's minimize of a vector loss);
 * value_out_dev [N] (the values BEFORE any update) and err_out_dev [N] (squared errors) are optional. */
int64_t rl4rs_exactk_critic_param_count(int32_t obs_dim, int32_t hidden);
int rl4rs_exactk_critic_create(int32_t obs_dim, int32_t hidden, int32_t max_rows, const float* params_host, void* stream,
                               rl4rs_exactk_critic** out);
int rl4rs_exactk_critic_destroy(rl4rs_exactk_critic* net);
int rl4rs_exactk_critic_params(rl4rs_exactk_critic* net, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_exactk_critic_adam_state(rl4rs_exactk_critic* net, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_exactk_critic_set_adam_step(rl4rs_exactk_critic* net, int64_t step);
int rl4rs_exactk_critic_forward(rl4rs_exactk_critic* net, int32_t N, const float* obs_dev, float* value_dev, void* stream);
int rl4rs_exactk_critic_loss_grad(rl4rs_exactk_critic* net, int32_t N, const float* obs_dev, const float* target_dev,
                                  float* value_out_dev, float* err_out_dev, void* stream);
int rl4rs_exactk_critic_adam_step(rl4rs_exactk_critic* net, float lr, float beta1, float beta2, float eps, void* stream);

/* ---- On-device ensemble dynamics model (d3rlpy 0.91's ProbabilisticEnsembleDynamics as restated in DESIGN.md; parity unpinned) ----
 * `members` networks on the shared input xa = [scaled x | a] (continuous actions only):
 *   h1 = dropout(bn1(relu(xa W1 + b1)));  h2 = dropout(bn2(relu([h1 | xa] W2 + b2)))   (use_dense = 0: h1 W2)
 *   mu = h2 Wmu + bmu;  ls = h2 Wls + bls;  ls = max_ls - softplus(max_ls - ls);  ls = min_ls + softplus(ls - min_ls)
 * with O = obs_dim + 1 outputs per head (the change of the scaled observation, then the scaled reward).  W1, W2 and Wmu are spectrally
 * normalised (spectral_norm = 1): a training forward runs one power iteration on the stored u / v and every product is scaled by
 * 1 / sigma; W / sigma is never materialised.  Batch norm is torch.nn.BatchNorm1d (eps 1e-5, momentum 0.1).  The dropout keep mask of
 * member m, layer l (0 / 1) is  uniform01(seed, step, row, (2 m + l) * 65536 + col) >= rate,  kept values scaled by 1 / (1 - rate).
 *
 * Flat parameters, members consecutive, matrices [in, out]:  W1 [D + E, H1], b1, bn1 weight, bn1 bias, W2 [H1 + D + E, H2] (rows of
 * h1 first; [H1, H2] without use_dense), b2, bn2 weight, bn2 bias, Wh [H2, 2 O] = [Wmu | Wls], bh [2 O], max_ls [O], min_ls [O].
 * Non-trained state, members consecutive: u1 [H1], v1 [D + E], u2 [H2], v2 [rows of W2], u3 [O], v3 [H2], running mean1, var1 [H1],
 * running mean2, var2 [H2]; after the last member the scaler constants: observation min [D], observation range max - min [D] (0: a
 * constant column, which maps to 0), reward mean, reward scale (std + eps).  No scaler = min 0, range 1, mean 0, scale 1.
 * Statistics of the last forward, per member: sigma [3], batch mean1, biased batch var1 [H1], mean2, var2 [H2].
 *
 * rl4rs_dyn_create refuses (and the *_count functions return -1), before a device is looked for: more than 16 members, widths
 * outside [1, 65536], a max_rows whose widest fp32 scratch array [members, max_rows, max(2 O, D + E, H1, H2)] would reach 2^31
 * bytes, and shapes whose power-iteration or loss kernels would need more than 160 KiB of LDS. */
typedef struct rl4rs_dyn rl4rs_dyn;
typedef struct rl4rs_dyn_cfg {
    int32_t obs_dim /* D */, act_dim /* E */, hidden1, hidden2, members, max_rows, max_grad_rows, use_batch_norm, use_dense, spectral_norm;
    float dropout_rate;
} rl4rs_dyn_cfg;
int64_t rl4rs_dyn_param_count(const rl4rs_dyn_cfg* cfg);
int64_t rl4rs_dyn_state_count(const rl4rs_dyn_cfg* cfg);
int64_t rl4rs_dyn_stats_count(const rl4rs_dyn_cfg* cfg);
int rl4rs_dyn_create(const rl4rs_dyn_cfg* cfg, const float* params_host, const float* state_host, void* stream, rl4rs_dyn** out);
int rl4rs_dyn_destroy(rl4rs_dyn* net);
int rl4rs_dyn_params(rl4rs_dyn* net, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_dyn_adam_state(rl4rs_dyn* net, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_dyn_set_adam_step(rl4rs_dyn* net, int64_t step);
int rl4rs_dyn_state(rl4rs_dyn* net, float** state_dev, int64_t* count, float** stats_dev, int64_t* stats_count);
/* x_dev [N, D] and a_dev [N, E] in raw units -> out_dev [members, N, 2 O] = [mu | bounded ls].  train != 0: batch statistics,
 * dropout, one power iteration; u / v and the running statistics move. */
int rl4rs_dyn_forward(rl4rs_dyn* net, int32_t N, const float* x_dev, const float* a_dev, int32_t train, uint32_t seed, uint32_t step,
                      float* out_dev, void* stream);
/* Training forward, then per member i:  loss_i = mean_b(mask[i, b] * (like_b + sum_o ls[b, o] + 0.01 (sum max_ls - sum min_ls))),
 * like_b = mean_d((x + mu[:D] - o')^2 exp(-ls[:D])) + (mu[D] - r')^2 exp(-ls[D])  on the scaled targets of next_x_dev [N, D] and
 * next_r_dev [N]; loss_dev [members]; the gradient of sum_i loss_i goes to the handle's flat gradient (bit-identical between
 * identical calls from the same state).  mask_dev float [members, N]. */
int rl4rs_dyn_loss_grad(rl4rs_dyn* net, int32_t N, const float* x_dev, const float* a_dev, const float* next_x_dev,
                        const float* next_r_dev, const float* mask_dev, uint32_t seed, uint32_t step, float* loss_dev, void* stream);
/* torch.optim.Adam on the handle's gradient, all members at once */
int rl4rs_dyn_adam_step(rl4rs_dyn* net, float lr, float beta1, float beta2, float eps, void* stream);
/* Eval forward, then per row the prediction of ONE member: indices_dev int32 [N] or NULL = floor(uniform01(seed, step, row,
 * 1000 * 65536) * members); pred = mu + exp(ls) * eps with eps = noise_dev [members, N, O], or NULL = Box-Muller of
 * uniform01(seed, step, row, (1001 + 2 m) * 65536 + o) and (1002 + 2 m) * 65536 + o, or 0 (deterministic).  next_x_dev [N, D] and
 * reward_dev [N] are reverse-scaled; variance_dev [N] stays in scaled units: variance_type 0 = max over members of sum_o exp(2 ls),
 * 1 = sum_o of the unbiased variance over members of their sampled [next x | reward].  penalise != 0: reward -= lam * variance
 * (MOPO).  indices_out_dev (optional) receives the member used. */
int rl4rs_dyn_predict(rl4rs_dyn* net, int32_t N, const float* x_dev, const float* a_dev, const int32_t* indices_dev,
                      const float* noise_dev, uint32_t seed, uint32_t step, int32_t deterministic, int32_t variance_type,
                      int32_t penalise, float lam, float* next_x_dev, float* reward_dev, float* variance_dev, int32_t* indices_out_dev,
                      void* stream);
/* SAC's soft target  y = r + gamma (1 - terminal) (min(q1, q2) - exp(log_temp[0]) logp),  all arrays float [N] on the device */
int rl4rs_sac_target(const float* q1_dev, const float* q2_dev, const float* logp_dev, const float* log_temp_dev, const float* rew_dev,
                     const float* ter_dev, float gamma, int32_t N, float* y_dev, void* stream);

/* The MDP checker's model (script/mdpchecker/mdp_checker.py:93-102, keras_transformer.get_model with encoder_num = decoder_num =
 * head_num = 1, use_same_embed = False), its training pass and its beam search (rl4rs/mdpchecker/decoder.py:50-82).  The model is restated
 * from the published form of keras_transformer in DESIGN 33; parity with it is unpinned, the beam search is pinned to the
 * reference's own function.  Tokens: 0 = <PAD>, 1 = <START>, 2 = <END>.
 *
 * Embedding + trigonometric position (added, no sqrt(d) scale; column 2 i = sin(pos / 10000^(2 i / d)), 2 i + 1 = cos); every block
 * is LayerNorm(x + f(x)) with the biased variance and eps 1e-14 under the root; attention has one head of width d, scores / sqrt(d),
 * e = exp(s - max over all keys), e = 0 at a PAD key (and behind the query in the decoder's self-attention), e / (sum e + 1e-7);
 * feed-forward d -> hidden_dim relu -> d; output softmax(h E_dec^T + b), tied to the decoder table.
 * Flat float32 parameters, matrices stored [in, out]:
 *     [ E_enc [V, d] | E_dec [V, d] | enc attention | enc ffn | dec self-attention | dec cross-attention | dec ffn | out bias [V] ]
 *     attention = Wq bq Wk bk Wv bv Wo bo gamma beta;   ffn = W1 [d, hidden] b1 W2 [hidden, d] b2 gamma beta
 * max_rows bounds the rows of every activation matrix of a call: N * max(L, src_len) of a forward, N * max(beam, src_len) of a
 * beam search (the caller splits its users into chunks).  Refused by rl4rs_seq2seq_create (rl4rs_seq2seq_param_count = -1), before a
 * device is looked for: token_num < 4, an odd embed_dim, src_len or tgt_len outside [1, 64], a max_rows whose widest fp32
 * activation row set [max_rows, max(token_num, 2 embed_dim, hidden_dim)] reaches 2^31 bytes, max_rows * 64 >= 2^31. */
typedef struct rl4rs_seq2seq rl4rs_seq2seq;
typedef struct rl4rs_seq2seq_cfg {
    int32_t token_num /* V */, embed_dim /* d */, hidden_dim, src_len, tgt_len /* most decoder positions */, max_rows;
} rl4rs_seq2seq_cfg;
int64_t rl4rs_seq2seq_param_count(const rl4rs_seq2seq_cfg* cfg);
int rl4rs_seq2seq_create(const rl4rs_seq2seq_cfg* cfg, const float* params_host, void* stream, rl4rs_seq2seq** out);
int rl4rs_seq2seq_destroy(rl4rs_seq2seq* net);
int rl4rs_seq2seq_params(rl4rs_seq2seq* net, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_seq2seq_adam_state(rl4rs_seq2seq* net, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_seq2seq_set_adam_step(rl4rs_seq2seq* net, int64_t step);
/* Teacher-forced training pass: dec_in_dev / dec_out_dev int32 [N, L]; loss_dev float[1] = mean over the positions whose decoder
 * INPUT token is not PAD of -log p[dec_out] (no clipping of p), and its full gradient into the handle's flat gradient buffer
 * (hand-written reverse pass; fixed-order reductions, no float atomics: two identical calls give identical bits, both tables'
 * row gradients included; the tied decoder table sums its output-layer and its embedding term).  Dropout as keras_transformer's
 * block wrapper, LayerNorm(x + Dropout(f(x))): element (row, col) of the [rows, d] output of block `site` (0 encoder attention,
 * 1 encoder ffn, 2 decoder self-attention, 3 decoder cross-attention, 4 decoder ffn) is kept when
 * uniform01(seed, step, row, site * 65536 + col) >= dropout_rate and then scaled by 1 / (1 - dropout_rate).  The training
 * activations are allocated by the first call ([max_rows, .] each).  N * max(L, src_len) <= max_rows. */
int rl4rs_seq2seq_loss_grad(rl4rs_seq2seq* net, int32_t N, const int32_t* enc_tokens_dev, const int32_t* dec_in_dev,
                            const int32_t* dec_out_dev, int32_t L, float dropout_rate, uint32_t seed, uint32_t step, float* loss_dev,
                            void* stream);
/* Adam in tf.train.AdamOptimizer's form (= Keras 'adam': lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), p -= lr_t m / (sqrt(v) + eps)) on
 * the handle's gradient; Keras' defaults are lr 1e-3, 0.9, 0.999, eps 1e-7. */
int rl4rs_seq2seq_adam_step(rl4rs_seq2seq* net, float lr, float beta1, float beta2, float eps, void* stream);
/* enc_tokens_dev int32 [N, src_len], dec_tokens_dev int32 [N, L] -> probs_dev float [N, L, V] (position l: the distribution of the
 * token after dec_tokens[:, :l + 1]).  No dropout. */
int rl4rs_seq2seq_forward(rl4rs_seq2seq* net, int32_t N, const int32_t* enc_tokens_dev, const int32_t* dec_tokens_dev, int32_t L,
                          float* probs_dev, void* stream);
/* Beam search as the reference's beam_search runs it: one live beam (<START>) at step 0, at every step the `beam` best of all
 * live * V continuations, score = PRODUCT of the probabilities carried in float64, beam 0 the best, equal scores by the smaller
 * beam * V + token; <END> and <PAD> are ordinary tokens, nothing ends early.  paths_dev int32 [N, beam, target_len + 1] (column 0 =
 * 1), scores_dev double [N, beam], step_probs_dev (optional) float [N, beam, target_len]: the probability of each chosen token along
 * the surviving path (their product is the score).  cand_bits_dev (optional) uint32 [N, ceil(V / 32)]: bit v of user n clear =
 * the probability of token v counts as 0 from step 1 on (step 0 is unmasked, as in the reference).
 * Refused: beam outside [1, 128], beam >= V, target_len outside [1, min(tgt_len, 63)], N * max(beam, src_len) > max_rows, a user whose
 * candidate bits hold fewer than `beam` tokens (candidates_size < beam; the bits are counted on the device and the count read back,
 * so a call with candidates synchronises the stream once before it decodes). */
int rl4rs_seq2seq_beam(rl4rs_seq2seq* net, int32_t N, const int32_t* enc_tokens_dev, int32_t beam, int32_t target_len,
                       const uint32_t* cand_bits_dev, int32_t* paths_dev, double* scores_dev, float* step_probs_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gaussian policy: the stochastic continuous actor-critic of the on-policy learners on support_conti_env
 * (script/modelfree_train.py:219-234,271-286,315-330,362-377, the `is_conti` branches of A2C / PPO / PG / IMPALA).  RLlib 1.5.1's
 * FullyConnectedNetwork under MODEL_DEFAULTS and its DiagGaussian are restated from their published form (ray is absent: parity
 * unpinned), checked against tests/gauss_ref.py.
 *   actor   head = tanh(tanh(x W1 + b1) W2 + b2) W3 + b3 = [mean (E) | log_std (E)]      critic  V = tanh(tanh(x V1 + c1) V2 + c2) V3 + c3
 *   flat    [W1 | b1 | W2 | b2 | W3 (H x 2E) | b3 | V1 | c1 | V2 | c2 | V3 (H x 1) | c3], matrices [in, out], float32
 *   with z = (a - mean) exp(-log_std):   logp = sum_e (-z^2 / 2 - log_std) - E log(2 pi) / 2,   entropy = sum_e (log_std + log(2 pi e) / 2),
 *   KL(old || new) = sum_e [ls_n - ls_o + (exp(2 ls_o) + (mu_o - mu_n)^2) / (2 exp(2 ls_n)) - 1 / 2];   log_std is not clamped.
 * Limits: 1 <= obs_dim <= 4096, hidden in {64, 128, 256}, 1 <= act_dim <= 64; create refuses other shapes.  Every call takes at most
 * max_rows rows.  All arithmetic is fp32 (f32 MFMA); gradients and statistics are bit-identical from call to call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rl4rs_gpolicy rl4rs_gpolicy;

int64_t rl4rs_gpolicy_param_count(int32_t obs_dim, int32_t hidden, int32_t act_dim);
int rl4rs_gpolicy_create(int32_t obs_dim, int32_t hidden, int32_t act_dim, int32_t max_rows, const float* params_host, void* stream,
                         rl4rs_gpolicy** out);
int rl4rs_gpolicy_destroy(rl4rs_gpolicy* pol);
/* Flat parameters (grad_dev receives NULL: the gradient is the caller's buffer), the Adam moments and step counter. */
int rl4rs_gpolicy_params(rl4rs_gpolicy* pol, float** params_dev, float** grad_dev, int64_t* count);
int rl4rs_gpolicy_adam_state(rl4rs_gpolicy* pol, float** m_dev, float** v_dev, int64_t* step);
int rl4rs_gpolicy_set_adam_step(rl4rs_gpolicy* pol, int64_t step);
/* dst's parameters <- src's (IMPALA's learner -> actor broadcast); the handles must have one shape. */
int rl4rs_gpolicy_copy_params(rl4rs_gpolicy* dst, const rl4rs_gpolicy* src, void* stream);
/* One launch: a = mean + exp(log_std) * normal01(seed, step, row, e) (row = position in the call; deterministic != 0: a = mean).
 * action_dev [N, E] is the unclipped draw, env_action_dev [N, E] = clip(a, -1, 1) is what the env receives; logp / value / entropy
 * [N], head_dev [N, 2E] = [mean | log_std], eps_dev [N, E] the noise.  Every output but action_dev may be NULL. */
int rl4rs_gpolicy_act(rl4rs_gpolicy* pol, int32_t N, const float* obs_dev, uint32_t seed, uint32_t step, int32_t deterministic,
                      float* action_dev, float* env_action_dev, float* logp_dev, float* value_dev, float* entropy_dev, float* head_dev,
                      float* eps_dev, void* stream);
/* The same forward for given (unclipped) actions [N, E]; on rl4rs_gpolicy_act's own actions logp is bit-identical to its logp. */
int rl4rs_gpolicy_evaluate(rl4rs_gpolicy* pol, int32_t N, const float* obs_dev, const float* actions_dev, float* logp_dev,
                           float* value_dev, float* entropy_dev, float* head_dev, void* stream);
/* Loss and flat gradient, the formulas of rl4rs_policy_loss_grad with this distribution: algo 0 = A2C (sums over rows), algo 1 = PPO
 * (means; KL(old || new); value clipping around old_value; needs old_logp [N], old_value [N], old_head [N, 2E]).
 * stats_dev (optional) float[4] = sums of {policy loss, value loss, entropy, kl}. */
int rl4rs_gpolicy_loss_grad(rl4rs_gpolicy* pol, int32_t algo, int32_t N, const float* obs_dev, const float* actions_dev,
                            const float* adv_dev, const float* ret_dev, const float* old_logp_dev, const float* old_value_dev,
                            const float* old_head_dev, float vf_coeff, float ent_coeff, float clip, float vf_clip, float kl_coeff,
                            float* grad_dev, float* stats_dev, void* stream);
/* Adam (tf.train.AdamOptimizer form) from grad_dev; grad_clip > 0 applies tf.clip_by_global_norm first. */
int rl4rs_gpolicy_adam_step(rl4rs_gpolicy* pol, const float* grad_dev, float lr, float beta1, float beta2, float eps, float grad_clip,
                            void* stream);
/* One PPO pass over N shuffled rows in minibatches of `minibatch` consecutive rows (the trailing N % minibatch rows are dropped): one
 * host call, bit-identical to rl4rs_gpolicy_loss_grad(algo 1) + rl4rs_gpolicy_adam_step per minibatch.  stats_dev (optional)
 * float[8] as rl4rs_policy_ppo_epoch: [0..3] sums over the LAST minibatch, [4..7] sums over every row of the pass. */
int rl4rs_gpolicy_ppo_epoch(rl4rs_gpolicy* pol, int32_t N, int32_t minibatch, const float* obs_dev, const float* actions_dev,
                            const float* adv_dev, const float* ret_dev, const float* old_logp_dev, const float* old_value_dev,
                            const float* old_head_dev, float vf_coeff, float ent_coeff, float clip, float vf_clip, float kl_coeff,
                            float lr, float beta1, float beta2, float eps, float grad_clip, float* grad_dev, float* stats_dev,
                            void* stream);
/* One-call IMPALA update as rl4rs_policy_vtrace_loss_grad: evaluate every row of R rollouts of [T, B] time-major rows, the float64
 * scan of rl4rs_vtrace per rollout (no dones: episodes end with the rollout), then the A2C-form loss with adv = pg_adv, ret = vs on
 * the kept rows (drop_last: the last step only supplies the bootstrap value).  rewards_dev float64; stats_dev float[4];
 * vtrace_stats_dev (optional) double[4] = sums of {rho, min(rho, clip_rho), vs, pg_adv}. */
int rl4rs_gpolicy_vtrace_loss_grad(rl4rs_gpolicy* pol, int32_t R, int32_t T, int32_t B, const float* obs_dev, const float* actions_dev,
                                   const float* behaviour_logp_dev, const double* rewards_dev, float gamma, float clip_rho,
                                   float clip_pg_rho, int32_t drop_last, float vf_coeff, float ent_coeff, float* grad_dev,
                                   float* stats_dev, double* vtrace_stats_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RL4RS_HIP_H */
