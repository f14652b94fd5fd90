// The launch plan of one scorer forward (rl4rs_dien_forward): which form every stage takes, derived ONCE from the handle's
// traits and the call - the stages in dien.hip switch on these fields and read no option.  Host code only, nothing from HIP: the
// plan of any handle and shape can be computed (and printed: dien_plan_str) without a device (tests/test_dien_plan_host.py).
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace rl4rs {

// ---- k_augru_x row tiles: the only copy of the rule (the grids of augru_x_launch / augru_xs_launch, the forward's automatic choice,
// dien_augru_rounds for step.hip).  32-row form: a tile is 32 rows.  64-row form: 64 rows, or - rows in groups of 9, the reward
// forward that also scores the state row - 7 groups = 63 stored rows.
inline int64_t augru_tiles(bool rows64, int64_t rows, int group) {
    if (!rows64) return (rows + 31) / 32;
    return group == 9 ? (rows / 9 + 6) / 7 : (rows + 63) / 64;
}
// 64-row workgroups when the rows come in whole groups of 8 per cache slot (the reward forward) or in groups of 9, and there are
// enough workgroups to fill the chip twice over; 32-row workgroups otherwise (obs-sized launches: one 32-row tile per CU).
// pin = 32 / 64 fixes the form where the shape admits it (rl4rs_dien_cfg.kernel_opts, rl4rs_dien_set_augru_rows), 0 = automatic
inline bool augru_rows64(int pin, int R, int group, int S, int n_cu) {
    if (pin == 32 || !(group == 9 || (group % 8 == 0 && R % 64 == 0))) return false;
    return pin == 64 || augru_tiles(true, R, group) * S >= 2 * (int64_t)n_cu;
}
// room rule of the shadow plane: the expected 32-row tiles * (S + 1) workgroups, one per CU, fit the chip.  The
// distinct hint counts only where it is below the forward's groups
inline bool augru_shadow_room(int hint, int n_groups, int S, int n_cu) {
    const int g = hint > 0 && hint < n_groups ? hint : n_groups;
    return augru_tiles(false, g, 1) * (S + 1) <= n_cu;
}
// the shadow plane's dense tile addresses `dense` and allf through one buffer descriptor each (as k_gemm_h16_map does)
inline bool g16_shadow_fits(int R, int Dn, int F, int U) {
    return ((int64_t)R - 1) * Dn + Dn < ((int64_t)1 << 29) && ((int64_t)R - 1) * F + U < ((int64_t)1 << 29);
}
// the gather form of the head GEMM (k_gemm_h16_gather) addresses allf, the table addend and the 256-wide output the same way
inline bool g16_gather_fits(int R, int F, int Kh) {
    return ((int64_t)R - 1) * F + Kh < ((int64_t)1 << 29) && (int64_t)R * 256 < ((int64_t)1 << 29);
}

// ---- what rl4rs_dien_create fixes
struct DienTraits {
    // modes, after option parsing and the weight-range checks
    bool fp16x2;           // scorer arithmetic
    bool gemm16;           // the plain GEMMs through k_gemm_h16 (else k_gemm_pk)
    bool din16;            // the DIN layer-1 operands fit fp16 too
    bool cat16;            // the Gram matrix of the category kernels in the split form
    bool augru_x;          // k_augru_x (default) or the first-generation k_augru_h16 (RL4RS_DIEN_OPT_AUGRU_H16)
    bool din_x;            // DIN scores through k_din_x (RL4RS_DIEN_OPT_DIN_V1: k_din_scores<*, true>)
    bool din_rows_auto;    // k_din_x at group == 1 picks 8 or 16 rows per workgroup on the device (RL4RS_DIEN_OPT_DIN_ROWS16: always 16)
    bool cat_v2;           // category branch through k_cat_attn2 when the shape allows (RL4RS_DIEN_OPT_CAT_V1: first form)
    bool cat_group;        // rows in groups of 8 / 9: k_cat_attn2g, one workgroup per group (RL4RS_DIEN_OPT_NO_CAT_GROUP: per row)
    bool dense_chain;      // both dense-tower layers in one launch (RL4RS_DIEN_OPT_NO_DENSE_CHAIN: two GEMMs)
    bool gemm_group;       // the chained dense tower and the q-side term in one launch (RL4RS_DIEN_OPT_NO_GEMM_GROUP: two)
    bool dense_fork;       // RL4RS_DIEN_OPT_DENSE_FORK: the dense tower on the handle's side stream
    bool row_dedup;        // k_din_x and k_augru_x score one representative per set of identical row groups; on only
                           // where both are the selected kernels: implies fp16x2, augru_x, din16, din_x and h1f
    bool dup_store;        // row dedup: the kernels store a representative's rows to its duplicates (default: k_row_expand)
    bool tier2_rows;       // row dedup: second tier on the active rows
    bool augru_shadow;     // observation-sized forwards may take the shadow-plane order
    bool h1f;              // the fragment-order copy of the first-GRU states exists (what k_din_x reads)
    bool lazy_expand;      // second tier: no k_row_expand behind the head - the outputs read the representative's row, the duplicates'
                           // internal rows are completed when somebody asks for them (RL4RS_DIEN_OPT_NO_LAZY_EXPAND: off)
    bool ptab, tsum;       // head tables built / their per-row sum buffer exists
    int E, U, L, S, Cn, Dn, Fld, NH2, n_cu, max_rows;

    // the derived predicates, each in this one place
    bool dense_chained() const { return gemm16 && dense_chain && U <= 128 && U % 16 == 0; }       // the tower is one chained launch
    bool dense_grouped() const { return fp16x2 && dense_chained() && gemm_group && !dense_fork; } // ... issued as a pair with the q-side term
    // ... and that pair as ONE grid (k_gemm_h16_pair).  launch_gemm_h16_pair needs both problems one block of columns wide
    // (gemm_h16_route: up to 128 columns; the q-side term is S * 64 wide) and loading their rows alike (dense rows of Dn % 4 != 0
    // take scalar loads, the query rows never do); otherwise it issues its two launches, bit-identical.  An unaligned `dense`
    // pointer of a call does the same to that call.
    bool pair_one_grid() const { return dense_grouped() && S * 64 <= 128 && (Dn & 3) == 0; }
    bool din_h16() const { return fp16x2 && din16; }
    bool din_x_selected() const { return din_h16() && h1f; }
    bool cat_v2_shape() const { return cat_v2 && E == 128 && Cn <= 24; }
    bool head_tsum() const { return ptab && tsum; }                                                // head: table addend built by the category kernel
};

// ---- what varies per forward
struct DienCall {
    int R, group;
    bool obs, prob;        // the caller gave an obs buffer / wants probabilities
    bool mirror, obs_last; // rl4rs::dien_set_obs_mirror / rl4rs_dien_set_obs_last armed for this forward
    bool carried;          // rl4rs_dien_set_row_partition armed ...
    int part_groups;       // ... for this many groups
    bool row_order;        // a row order of R / group entries is set
    int augru_rows;        // 0 / 32 / 64: the pin of the k_augru_x row-tile form
    int distinct_hint;     // rl4rs_dien_set_distinct_hint (0 = none)
    bool dense_vec;        // `dense` and Dn admit 16-byte loads (AugruShadowArgs::vec)
    bool rows_differ;      // rl4rs::dien_set_group_rows armed: the rows of a group share the cache slot but not the category
                           // columns - the group kernels k_cat_attn2g (every id but the last shared) are not selected
};

enum class PlanDedup { None, Launch, Carried };
enum class PlanCat { Shadow, V1, V2_21, V2_24, G8, G9 };
enum class PlanDense { Shadow, Pair, Chain, TwoGemm };
enum class PlanQside { InPair, InDinXq, MappedH16, ScorerGemm };
enum class PlanDin { Xq, XAuto, X16, Scores };
enum class PlanAugru { Xs, X32, X64, H16, Recur32 };
enum class PlanExpand { None, Front, Behind, Lazy };
enum class PlanHead { TsumH16, TsumH16Mirror, TsumPacked, TablesFinish, Plain };

struct DienPlan {
    bool tier2;            // the category kernel, the dense / q-side GEMMs and the head GEMM take the active-row map
    bool shadow;           // shadow-plane order: k_din_xq, k_augru_xs
    PlanDedup dedup;
    bool dup_lists;        // k_row_dedup builds, k_din_x / k_augru_x follow the duplicate lists (dup_store)
    PlanCat cat;
    bool cat_h16;          // the category kernels' Gram matrix in the split form
    PlanDense dense;       // Chain / TwoGemm: ...
    bool dense_side;       // ... on the side stream, forked at the top of the forward and joined in front of the head
    bool dense_vec;
    PlanQside qside;
    PlanDin din;
    bool din_stage, din_h16; int din_waves;      // k_din_scores<STAGE, H16> and its waves per workgroup
    PlanAugru augru;
    PlanExpand expand; int expand_ncol;          // k_row_expand and the columns of allf it copies (Lazy: not launched by the forward -
                                                 // group == 1: the head GEMM computes every row from its representative's all-feature
                                                 // row; group > 1: k_head_prob_rep reads the representative's head output)
    PlanHead head;
    bool prob;
};

inline DienPlan dien_plan(const DienTraits& t, const DienCall& c) {
    DienPlan p{};
    const int n_groups = c.R / c.group;
    const bool rows64 = augru_rows64(c.augru_rows, c.R, c.group, t.S, t.n_cu);
    p.dedup = !t.row_dedup ? PlanDedup::None : (c.carried ? PlanDedup::Carried : PlanDedup::Launch);
    p.dup_lists = t.dup_store;
    // second tier: only in the default forms of the launches that take the map, never with the head's host mirror armed
    p.tier2 = t.row_dedup && t.tier2_rows && !t.dup_store && !t.dense_fork && !(c.obs && c.mirror) && t.gemm16 && t.head_tsum() &&
              t.cat_v2_shape() && t.dense_chained();
    // shadow plane: on top of the second tier (so k_din_x and k_augru_x are the selected kernels), observation-shaped,
    // every launch involved in its default form, the 32-row AUGRU form not pinned away, room on the chip
    p.shadow = p.tier2 && t.augru_shadow && c.group == 1 && t.Cn == 21 && t.S <= 2 && t.din_rows_auto && t.dense_grouped() && !rows64 &&
               c.augru_rows != 64 && augru_shadow_room(c.distinct_hint, n_groups, t.S, t.n_cu) && g16_shadow_fits(c.R, t.Dn, t.Fld, t.U);
    p.cat_h16 = t.fp16x2 && t.cat16;
    if (p.shadow) p.cat = PlanCat::Shadow;
    else if (t.cat_v2_shape() && t.cat_group && t.Cn >= 11 && (c.group == 8 || c.group == 9) && !c.rows_differ) p.cat = c.group == 8 ? PlanCat::G8 : PlanCat::G9;
    else if (t.cat_v2_shape()) p.cat = t.Cn == 21 ? PlanCat::V2_21 : PlanCat::V2_24;
    else p.cat = PlanCat::V1;
    p.dense_side = t.dense_fork;
    p.dense_vec = c.dense_vec;
    if (p.shadow) p.dense = PlanDense::Shadow;
    else if (t.dense_grouped()) p.dense = PlanDense::Pair;
    else p.dense = t.dense_chained() ? PlanDense::Chain : PlanDense::TwoGemm;
    if (p.shadow) p.qside = PlanQside::InDinXq;
    else if (p.dense == PlanDense::Pair) p.qside = PlanQside::InPair;
    else p.qside = p.tier2 ? PlanQside::MappedH16 : PlanQside::ScorerGemm;
    p.din_h16 = t.din_h16();
    p.din_stage = c.group != 1;
    p.din_waves = c.group == 1 ? 4 : (c.group % 4 == 0 ? 4 : (c.group % 3 == 0 ? 3 : (c.group % 2 == 0 ? 2 : (c.group < 4 ? c.group : 4))));
    if (p.shadow) p.din = PlanDin::Xq;
    else if (t.din_x_selected()) p.din = (c.group == 1 && t.din_rows_auto) ? PlanDin::XAuto : PlanDin::X16;
    else p.din = PlanDin::Scores;
    if (!t.fp16x2) p.augru = PlanAugru::Recur32;
    else if (p.shadow) p.augru = PlanAugru::Xs;
    else if (t.augru_x) p.augru = rows64 ? PlanAugru::X64 : PlanAugru::X32;
    else p.augru = PlanAugru::H16;
    // the duplicates' rows: in front of the head GEMM (AUGRU states and attention scores), or - second tier - behind it (the whole
    // all-feature row, the scores, q and the head output)
    if (p.dedup == PlanDedup::None || t.dup_store) p.expand = PlanExpand::None;
    else p.expand = p.tier2 ? PlanExpand::Behind : PlanExpand::Front;
    p.expand_ncol = p.expand == PlanExpand::None ? 0 : (p.tier2 ? t.S * t.NH2 + t.U + t.E : t.S * t.NH2);
    // lazy form, only in place of Behind (so: second tier, the head is the mapped k_gemm_h16 with the table addend and
    // no mirror): observation-shaped forwards - the head's gather form addresses allf, the addend and the output through one
    // buffer descriptor each - and reward-shaped forwards whose head output stays inside the handle
    if (p.expand == PlanExpand::Behind && t.lazy_expand &&
        (c.group == 1 ? g16_gather_fits(c.R, t.Fld, p.expand_ncol) : !c.obs))
        p.expand = PlanExpand::Lazy;
    if (t.head_tsum()) p.head = !t.gemm16 ? PlanHead::TsumPacked : ((c.obs && c.mirror) ? PlanHead::TsumH16Mirror : PlanHead::TsumH16);
    else p.head = t.ptab ? PlanHead::TablesFinish : PlanHead::Plain;
    p.prob = c.prob;
    return p;
}

// one line per plan, for logs and the host test
inline int dien_plan_str(const DienPlan& p, char* buf, size_t cap) {
    static const char* const dd[] = {"none", "k_row_dedup", "carried"};
    static const char* const ct[] = {"shadow", "k_cat_attn", "k_cat_attn2<21,true>", "k_cat_attn2<24,false>", "k_cat_attn2g<8,8>", "k_cat_attn2g<9>"};
    static const char* const dn[] = {"shadow", "pair", "chain", "two_gemms"};
    static const char* const qs[] = {"in_pair", "in_k_din_xq", "mapped_k_gemm_h16", "scorer_gemm"};
    static const char* const di[] = {"k_din_xq", "k_din_x_auto", "k_din_x_16", "k_din_scores"};
    static const char* const au[] = {"k_augru_xs", "k_augru_x_32", "k_augru_x_64", "k_augru_h16", "k_recur_fp32"};
    static const char* const ex[] = {"none", "front", "behind", "lazy"};
    static const char* const hd[] = {"tsum+k_gemm_h16", "tsum+k_gemm_h16+mirror", "tsum+packed", "tables+k_head_finish", "plain"};
    char din[48];
    if (p.din == PlanDin::Scores) snprintf(din, sizeof(din), "k_din_scores<%d,%d>x%d", (int)p.din_stage, (int)p.din_h16, p.din_waves);
    else snprintf(din, sizeof(din), "%s", di[(int)p.din]);
    return snprintf(buf, cap, "tier2=%d shadow=%d dedup=%s%s cat=%s dense=%s%s qside=%s din=%s augru=%s expand=%s:%d head=%s prob=%d",
                    (int)p.tier2, (int)p.shadow, dd[(int)p.dedup], p.dup_lists ? "+dup_lists" : "", ct[(int)p.cat], dn[(int)p.dense],
                    p.dense_side ? "@side" : "", qs[(int)p.qside], din, au[(int)p.augru], ex[(int)p.expand], p.expand_ncol,
                    hd[(int)p.head], (int)p.prob);
}

}  // namespace rl4rs
