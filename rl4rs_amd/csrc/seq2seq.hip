// The MDP checker's model on gfx950: a one-layer, one-head encoder-decoder transformer over item tokens (inference) and the beam
// search the checker's two experiments decode with.
//
// Reference: script/mdpchecker/mdp_checker.py:93-102 (keras_transformer.get_model) and rl4rs/mdpchecker/decoder.py:50-82
// (beam_search).  keras_transformer and the three packages under it are not available: the model is restated in DESIGN 33
// [from memory], parity with it is unpinned, the yardstick is the float64 restatement tests/mdp_ref.py.  beam_search is plain numpy
// and IS pinned: the golden files under tests/golden/mdp_beam_*.npz are its own output.
//
// Every dense product goes through the fp32 MFMA GEMMs of gemm.hip.  The kernels here are what has no counterpart there: the
// embedding + position sum, attention over at most 64 keys under PAD / causal masks with keras_multi_head's "+ 1e-7" normaliser,
// add + layer norm with eps 1e-14, the row softmax of the tied output layer and the wide-beam top-K.
//
// Beam layout.  Decoder rows are r = n * live + b (live = 1 at step 0, beam afterwards).  A step runs ONLY the last position of
// every row.  The encoder output and the cross-attention K / V are computed once per user and read by all of its beams (row r reads
// user r / live).  With one decoder layer the self-attention K / V of a prefix position are a function of (token, position), and a
// LINEAR one: (E[tok] + pos[j]) W + b = E[tok] W + (pos[j] W + b).  So a beam call projects the decoder table once (EKV [V, 2d]) and
// the position table once (PKV [64, 2d]); a beam carries nothing but its token prefix, and a selection copies target_len + 1 ints
// per beam instead of reordering a per-beam cache.  The two-term sum rounds differently from the one-GEMM form of the
// teacher-forced forward (fp32 rounding only).
//
// Selection.  Scores are products of probabilities carried in float64 (the reference multiplies float32 probabilities into a
// float64 array).  The best `beam` of a user's live * V continuations are found in two stages: each row's own best `beam`, in order
// (k_s2s_topk / k_s2s_topk_wave; no more than that many of one row can survive), then a merge of the user's `live` sorted lists
// (k_s2s_merge).  Order: larger score first, equal scores by the smaller flat index b * V + token - in both stages, so the result is
// that of one search over the flat list.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "optim.hpp"

namespace rl4rs {

namespace {

constexpr int S2S_MAXLEN = 64;                 // positions of either sequence: one lane per key
constexpr int S2S_BEAM_MAX = 128;
constexpr float S2S_LN_EPS = 1e-14f;           // keras_layer_normalization: K.epsilon()^2, under the root
constexpr float S2S_ATT_EPS = 1e-7f;           // keras_multi_head: e / (sum e + K.epsilon())

struct S2sAtt { size_t Wq, bq, Wk, bk, Wv, bv, Wo, bo, g, b; };
struct S2sFfn { size_t W1, b1, W2, b2, g, b; };
// flat parameter layout, matrices [in, out]:
//   E_enc [V, d] | E_dec [V, d] | encoder attention | encoder ffn | decoder self-attention | decoder cross-attention | decoder ffn | out bias [V]
//   attention = Wq bq Wk bk Wv bv Wo bo gamma beta;  ffn = W1 [d, h] b1 W2 [h, d] b2 gamma beta
struct S2sLayout { size_t Eenc, Edec; S2sAtt ea; S2sFfn ef; S2sAtt ds, dc; S2sFfn df; size_t ob, total; };

static S2sLayout s2s_layout(int V, int d, int h) {
    S2sLayout L;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += n; return at; };
    auto att = [&](S2sAtt& a) {
        a.Wq = take((size_t)d * d); a.bq = take(d); a.Wk = take((size_t)d * d); a.bk = take(d);
        a.Wv = take((size_t)d * d); a.bv = take(d); a.Wo = take((size_t)d * d); a.bo = take(d); a.g = take(d); a.b = take(d);
    };
    auto ffn = [&](S2sFfn& f) {
        f.W1 = take((size_t)d * h); f.b1 = take(h); f.W2 = take((size_t)h * d); f.b2 = take(d); f.g = take(d); f.b = take(d);
    };
    L.Eenc = take((size_t)V * d); L.Edec = take((size_t)V * d);
    att(L.ea); ffn(L.ef); att(L.ds); att(L.dc); ffn(L.df);
    L.ob = take(V);
    L.total = o;
    return L;
}

__device__ __forceinline__ float s2s_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float s2s_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// X[m, :] = E[token of row m] + pos[pos0 + m % L]; the token of row m is tok[(m / L) * tok_ld + tok_off + m % L], clamped into the table
__global__ void k_s2s_embed(const int32_t* __restrict__ tok, int tok_ld, int tok_off, int L, int pos0, const float* __restrict__ E,
                            const float* __restrict__ pos, float* __restrict__ X, int M, int D, int V) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)M * D) return;
    const int m = (int)(i / D), c = (int)(i - (size_t)m * D), n = m / L, j = m - n * L;
    const int t = min(max(tok[(size_t)n * tok_ld + tok_off + j], 0), V - 1);
    X[i] = E[(size_t)t * D + c] + pos[(size_t)(pos0 + j) * D + c];
}

// One query row per wave, one key per lane (Lk <= 64):  s = q . k / sqrt(D);  e = exp(s - max over ALL keys);  e = 0 at a PAD key and,
// causal, at a key behind the query;  a = e / (sum e + 1e-7);  O = a V.  Query row r = (n, q) of Lq rows per sequence.
// TABLE = false: keys / values are rows (n / qdiv) * Lk + k of K / V (row stride ldkv), their tokens ktok[(n / qdiv) * Lk + k].
// TABLE = true (a beam row's own prefix, Lq = 1): key k is K[tok] + PK[k] with tok = ktok[r * ktok_ld + k], values alike.
template <bool TABLE>
__global__ __launch_bounds__(256) void k_s2s_attn(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                  int ldkv, const float* __restrict__ PK, const float* __restrict__ PV,
                                                  const int32_t* __restrict__ ktok, int ktok_ld, float* __restrict__ O, int Mq, int Lq,
                                                  int Lk, int qdiv, int D, int causal, int vocab, float* __restrict__ Asave = nullptr) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= Mq) return;                       // whole waves leave; no block-wide barrier below
    const int n = r / Lq, q = r - n * Lq, kb = n / qdiv;
    const float* qr = Q + (size_t)r * D;
    int my_tok = 0;
    if (lane < Lk) my_tok = TABLE ? ktok[(size_t)r * ktok_ld + lane] : ktok[(size_t)kb * Lk + lane];
    float mine = 0.f;
    for (int k = 0; k < Lk; ++k) {
        const int tk = __shfl(my_tok, k);
        const size_t row = TABLE ? (size_t)min(max(tk, 0), vocab - 1) : (size_t)kb * Lk + k;
        const float* kr = K + row * ldkv;
        float s = 0.f;
        if (TABLE) {
            const float* pk = PK + (size_t)k * ldkv;
            for (int d = lane; d < D; d += 64) s = fmaf(qr[d], kr[d] + pk[d], s);
        } else {
            for (int d = lane; d < D; d += 64) s = fmaf(qr[d], kr[d], s);
        }
        s = s2s_wave_sum(s);
        if (lane == k) mine = s;
    }
    mine = mine / sqrtf((float)D);
    const float mx = s2s_wave_max(lane < Lk ? mine : -3.4028235e38f);
    const bool open = lane < Lk && my_tok != 0 && (!causal || lane <= q);
    const float e = open ? expf(mine - mx) : 0.f;
    const float a = e / (s2s_wave_sum(e) + S2S_ATT_EPS);
    if (Asave) {                               // training: the reverse pass reads a and the key the max came from (65 floats per row)
        const unsigned long long top = __ballot(lane < Lk && mine == mx);
        if (lane < Lk) Asave[(size_t)r * 65 + lane] = a;
        if (lane == 0) Asave[(size_t)r * 65 + 64] = (float)(__ffsll((long long)top) - 1);
    }
    for (int d0 = 0; d0 < D; d0 += 64) {
        const int d = d0 + lane;
        float o = 0.f;
        for (int k = 0; k < Lk; ++k) {
            const float ak = __shfl(a, k);     // every lane takes part in the exchange, also one past D
            const int tk = __shfl(my_tok, k);
            if (d < D) {
                const size_t row = TABLE ? (size_t)min(max(tk, 0), vocab - 1) : (size_t)kb * Lk + k;
                float v = V[row * ldkv + d];
                if (TABLE) v += PV[(size_t)k * ldkv + d];
                o = fmaf(ak, v, o);
            }
        }
        if (d < D) O[(size_t)r * D + d] = o;
    }
}

// Y = gamma * (s - mean) / sqrt(var + 1e-14) + beta, s = X + R, population variance; one wave per row
__global__ __launch_bounds__(256) void k_s2s_add_ln(const float* __restrict__ X, const float* __restrict__ R, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ Y, int M, int D) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const size_t o = (size_t)r * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += X[o + d] + R[o + d];
    const float mean = s2s_wave_sum(s) / (float)D;
    float v = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float c = X[o + d] + R[o + d] - mean;
        v += c * c;
    }
    const float sd = sqrtf(s2s_wave_sum(v) / (float)D + S2S_LN_EPS);
    for (int d = lane; d < D; d += 64) Y[o + d] = gamma[d] * ((X[o + d] + R[o + d] - mean) / sd) + beta[d];
}

// P[r, :V] = softmax(P[r, :V]) in place (the bias is already in: GEMM epilogue); one workgroup per row
__global__ __launch_bounds__(256) void k_s2s_softmax(float* __restrict__ P, int64_t ld, int V) {
    __shared__ float red[8];
    float* p = P + (size_t)blockIdx.x * ld;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float mx = -3.4028235e38f;
    for (int v = threadIdx.x; v < V; v += 256) mx = fmaxf(mx, p[v]);
    mx = s2s_wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float se = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) se += expf(p[v] - mx);
    se = s2s_wave_sum(se);
    if (lane == 0) red[4 + wave] = se;
    __syncthreads();
    se = (red[4] + red[5]) + (red[6] + red[7]);
    for (int v = threadIdx.x; v < V; v += 256) p[v] = expf(p[v] - mx) / se;
}

// T [D, ldt] = E [V, D]^T through a 32 x 33 LDS tile (both sides coalesced); block (32, 8)
__global__ void k_s2s_transpose(const float* __restrict__ E, float* __restrict__ T, int V, int D, int ldt) {
    __shared__ float tile[32][33];
    const int v0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int v = v0 + i, c = c0 + threadIdx.x;
        tile[i][threadIdx.x] = (v < V && c < D) ? E[(size_t)v * D + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int c = c0 + i, v = v0 + threadIdx.x;
        if (c < D && v < V) T[(size_t)c * ldt + v] = tile[threadIdx.x][i];
    }
}

// flag[0] = 1 when some user's candidate bits hold fewer than `beam` tokens below V (one thread per user)
__global__ void k_s2s_cand_check(const uint32_t* __restrict__ cand, int N, int W, int V, int beam, int32_t* __restrict__ flag) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int c = 0;
    for (int w = 0; w < W; ++w) {
        uint32_t x = cand[(size_t)n * W + w];
        if (w == W - 1 && (V & 31)) x &= (1u << (V & 31)) - 1u;
        c += __popc(x);
    }
    if (c < beam) flag[0] = 1;
}

// both prefix buffers: column 0 = <START>, the rest 0
__global__ void k_s2s_beam_init(int32_t* __restrict__ a, int32_t* __restrict__ b, int n, int T1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = (i % T1) == 0 ? 1 : 0;
    a[i] = v;
    b[i] = v;
}

// the larger (value, then smaller index) of two candidates
__device__ __forceinline__ void s2s_better(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// Stage one, any V: the best Kb items of beam row r = blockIdx.x, descending, equal values by the smaller token.  Item v has value
// score[r] * P[r, v] (score = NULL: 1; times 0 where the candidate bits of user r / live, cand [users, cand_ld], do not hold v)
// -> cval / cidx [r, Kb].  A round scans for the largest item that comes AFTER the previous pick in that order: P stays read-only.
__global__ __launch_bounds__(256) void k_s2s_topk(const float* __restrict__ P, int64_t ldp, int V, int Kb, int live,
                                                  const double* __restrict__ score, const uint32_t* __restrict__ cand, int cand_ld,
                                                  double* __restrict__ cval, int32_t* __restrict__ cidx) {
    __shared__ double s_wv[2][4];
    __shared__ int s_wi[2][4];
    const int r = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* p = P + (size_t)r * ldp;
    const double sc = score ? score[r] : 1.0;
    const uint32_t* bits = cand ? cand + (size_t)(r / live) * cand_ld : nullptr;
    double prev_v = INFINITY;
    int prev_i = -1;
    for (int k = 0; k < Kb; ++k) {
        double best = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = threadIdx.x; v < V; v += 256) {
            double x = sc * (double)p[v];
            if (bits && !((bits[v >> 5] >> (v & 31)) & 1u)) x = 0.0;
            const bool after = x < prev_v || (x == prev_v && v > prev_i);
            if (after && (x > best || (x == best && v < bi))) { best = x; bi = v; }
        }
        for (int o = 32; o > 0; o >>= 1) s2s_better(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
        if (lane == 0) { s_wv[k & 1][wave] = best; s_wi[k & 1][wave] = bi; }
        __syncthreads();                       // slots alternate: the next round's writes cannot overtake this round's reads
        best = s_wv[k & 1][0];
        bi = s_wi[k & 1][0];
        for (int w = 1; w < 4; ++w) s2s_better(best, bi, s_wv[k & 1][w], s_wi[k & 1][w]);
        if (bi == 0x7fffffff) { best = 0.0; bi = 0; }      // nothing left to pick (NaN scores): a valid index all the same
        prev_v = best;
        prev_i = bi;
        if (threadIdx.x == 0) {
            cval[(size_t)r * Kb + k] = best;
            cidx[(size_t)r * Kb + k] = bi;
        }
    }
}

// Stage two: the best Kb of user n = blockIdx.x among the live * Kb survivors cval / cidx [n * live + b, k], index b * V + token.
// Every row's list is already in (value, index) order, so this is a merge of `live` sorted lists: one wave per user, lane l holds
// the heads of rows l and l + 64 (live <= 128), a round is one wave-wide arg-max and one advance by the owner.  The picks become
// the user's new beams: prefix_out[n, k] = prefix_in[n, parent] + token, score_out[n, k], and the chosen tokens' (masked)
// probabilities sp_out[n, k, 0..t] when sp_out is not NULL.  T1 = target_len + 1 ints per prefix, T1 - 1 floats per sp row.
__global__ __launch_bounds__(64) void k_s2s_merge(const float* __restrict__ P, int64_t ldp, int V, int Kb, int live,
                                                  const uint32_t* __restrict__ cand, int cand_ld, const double* __restrict__ cval,
                                                  const int32_t* __restrict__ cidx, int t, int T1, const int32_t* __restrict__ prefix_in,
                                                  int32_t* __restrict__ prefix_out, double* __restrict__ score_out,
                                                  const float* __restrict__ sp_in, float* __restrict__ sp_out) {
    __shared__ double s_val[S2S_BEAM_MAX];
    __shared__ int s_idx[S2S_BEAM_MAX];
    const int n = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)n * live * Kb;
    double cur[2];                             // head of the lane's two rows; -1: no such row, or the row is used up
    int cid[2], head[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int b = lane + 64 * s;
        head[s] = 0;
        cur[s] = b < live ? cval[base + (size_t)b * Kb] : -1.0;
        cid[s] = b < live ? b * V + cidx[base + (size_t)b * Kb] : 0x7fffffff;
    }
    for (int k = 0; k < Kb; ++k) {
        double best = cur[0];
        int bi = cid[0];
        s2s_better(best, bi, cur[1], cid[1]);
        for (int o = 32; o > 0; o >>= 1) s2s_better(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (cur[s] >= 0.0 && cid[s] == bi) {
                const int b = lane + 64 * s;
                ++head[s];
                const bool more = head[s] < Kb;
                cur[s] = more ? cval[base + (size_t)b * Kb + head[s]] : -1.0;
                cid[s] = more ? b * V + cidx[base + (size_t)b * Kb + head[s]] : 0x7fffffff;
            }
        if (lane == 0) {
            const bool none = best < 0.0 || bi == 0x7fffffff;               // cannot happen with live * Kb >= Kb finite items
            s_val[k] = none ? 0.0 : best;
            s_idx[k] = none ? 0 : bi;
        }
    }
    __syncthreads();
    for (int k = lane; k < Kb; k += 64) {
        const int par = min(s_idx[k] / V, live - 1), tok = s_idx[k] - (s_idx[k] / V) * V;
        const size_t ri = (size_t)n * live + par, ro = (size_t)n * Kb + k;
        for (int j = 0; j <= t; ++j) prefix_out[ro * T1 + j] = prefix_in[ri * T1 + j];
        prefix_out[ro * T1 + t + 1] = tok;
        score_out[ro] = s_val[k];
        if (sp_out) {
            const int T = T1 - 1;
            for (int j = 0; j < t; ++j) sp_out[ro * T + j] = sp_in[ri * T + j];
            float pr = P[ri * (size_t)ldp + tok];
            if (cand && !((cand[(size_t)n * cand_ld + (tok >> 5)] >> (tok & 31)) & 1u)) pr = 0.f;
            sp_out[ro * T + t] = pr;
        }
    }
}

// k_s2s_topk for V <= 64 * S2S_WAVE_ITEMS: one row per WAVE, the row's products in registers (item v in lane v % 64, slot
// v / 64), a pick is struck out by its owner, no block-wide barrier.  Same values, same order, same output as the workgroup form,
// which pays a barrier per pick: 2048 users x 100 beams over V = 287 took 117 ms with it and 53.6 ms with this.
constexpr int S2S_WAVE_ITEMS = 8;
__global__ __launch_bounds__(256) void k_s2s_topk_wave(const float* __restrict__ P, int64_t ldp, int V, int Kb, int live, int R,
                                                       const double* __restrict__ score, const uint32_t* __restrict__ cand, int cand_ld,
                                                       double* __restrict__ cval, int32_t* __restrict__ cidx) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;
    const double sc = score ? score[r] : 1.0;
    const uint32_t* bits = cand ? cand + (size_t)(r / live) * cand_ld : nullptr;
    const float* p = P + (size_t)r * ldp;
    double x[S2S_WAVE_ITEMS];                  // -1: past V or already picked (products are >= 0)
#pragma unroll
    for (int j = 0; j < S2S_WAVE_ITEMS; ++j) {
        const int v = j * 64 + lane;
        double y = -1.0;
        if (v < V) {
            y = sc * (double)p[v];
            if (bits && !((bits[v >> 5] >> (v & 31)) & 1u)) y = 0.0;
        }
        x[j] = y;
    }
    for (int k = 0; k < Kb; ++k) {
        double best = -1.0;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < S2S_WAVE_ITEMS; ++j)
            if (x[j] > best) { best = x[j]; bi = j * 64 + lane; }          // ascending index: the first of equals stays
        for (int o = 32; o > 0; o >>= 1) s2s_better(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
#pragma unroll
        for (int j = 0; j < S2S_WAVE_ITEMS; ++j)
            if (bi == j * 64 + lane) x[j] = -1.0;
        if (lane == 0) {
            const bool none = bi == 0x7fffffff;                             // nothing left to pick (NaN scores): a valid index all the same
            cval[(size_t)r * Kb + k] = none ? 0.0 : best;
            cidx[(size_t)r * Kb + k] = none ? 0 : bi;
        }
    }
}

}  // namespace

}  // namespace rl4rs

using namespace rl4rs;

#include "seq2seq_train.hpp"

namespace {
struct S2sAttSave { float *Q, *Pa, *AO, *xhat, *rstd, *H; };
struct S2sFfnSave { float *F, *xhat, *rstd, *H; };
struct S2sTrain {
    void* arena;
    float *Xe, *KVe, *Xd, *KVs, *CKV, *Pr;                       // embeddings, keys / values, probabilities [R, V]
    S2sAttSave ea, ds, dc;
    S2sFfnSave ef, df;
    float *T[5], *G[3], *GKV, *GP, *GF, *dWt, *part, *part_b, *rowloss, *cnt;   // reverse-pass scratch
};
}  // namespace

struct rl4rs_seq2seq {
    rl4rs_seq2seq_cfg c;
    S2sLayout L;
    int Vp;                                     // row stride of the transposed decoder table (multiple of 4)
    void* arena;
    float *params, *pos;
    // activations, [max_rows, .]
    float *X, *Q, *KV, *A, *O, *H1, *H2, *F, *Enc, *CKV, *P;
    // beam tables and state
    float *EKV, *PKV, *EdT, *sp[2];
    int32_t *prefix[2], *cidx;
    double *score[2], *cval;
    OptBlock opt;                               // params (the same pointer), gradient, Adam moments
    S2sTrain tr;                                // training activations and scratch, allocated by the first loss_grad
};

namespace {

#define S2S_TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

static int s2s_check_cfg(const rl4rs_seq2seq_cfg* c) {
    RL4RS_REQUIRE(c, "seq2seq: null cfg");
    RL4RS_REQUIRE(c->token_num >= 4 && c->embed_dim >= 2 && c->embed_dim % 2 == 0 && c->hidden_dim >= 1,
                  "seq2seq: token_num %d (>= 4), embed_dim %d (even, >= 2), hidden_dim %d (>= 1)", c->token_num, c->embed_dim,
                  c->hidden_dim);
    RL4RS_REQUIRE(c->src_len >= 1 && c->src_len <= S2S_MAXLEN && c->tgt_len >= 1 && c->tgt_len <= S2S_MAXLEN,
                  "seq2seq: src_len %d, tgt_len %d outside [1, %d]", c->src_len, c->tgt_len, S2S_MAXLEN);
    RL4RS_REQUIRE(c->max_rows >= 1 && (int64_t)c->max_rows * S2S_MAXLEN < ((int64_t)1 << 31),
                  "seq2seq: max_rows %d outside [1, 2^31 / %d) (the beams' prefix cells are counted in 32 bits)", c->max_rows, S2S_MAXLEN);
    const int64_t widest = std::max<int64_t>(std::max(c->token_num + 3, 2 * c->embed_dim), c->hidden_dim);
    RL4RS_REQUIRE((int64_t)c->max_rows * widest * 4 < ((int64_t)1 << 31),
                  "seq2seq: max_rows %d x widest activation row %lld floats reaches 2^31 bytes; largest admitted max_rows is %lld",
                  c->max_rows, (long long)widest, (long long)((((int64_t)1 << 31) - 1) / (widest * 4)));
    RL4RS_REQUIRE((int64_t)c->token_num * 2 * c->embed_dim * 4 < ((int64_t)1 << 31), "seq2seq: token_num %d x 2 embed_dim %d reaches 2^31 bytes",
                  c->token_num, c->embed_dim);
    return RL4RS_OK;
}

static int s2s_embed(rl4rs_seq2seq* p, const int32_t* tok, int tok_ld, int tok_off, int L, int pos0, size_t table, float* X, int M,
                     hipStream_t st) {
    const int D = p->c.embed_dim;
    const size_t n = (size_t)M * D;
    hipLaunchKernelGGL(k_s2s_embed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tok, tok_ld, tok_off, L, pos0, p->params + table,
                       p->pos, X, M, D, p->c.token_num);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}
static int s2s_add_ln(rl4rs_seq2seq* p, const float* X, const float* R, size_t g, size_t b, float* Y, int M, hipStream_t st) {
    hipLaunchKernelGGL(k_s2s_add_ln, dim3((M + 3) / 4), dim3(256), 0, st, X, R, p->params + g, p->params + b, Y, M, p->c.embed_dim);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}
static int s2s_lin(rl4rs_seq2seq* p, const float* a, size_t W, size_t b, float* c, int64_t ldc, int M, int N, int K, int act, hipStream_t st) {
    return launch_gemm_f32(a, K, p->params + W, N, p->params + b, c, ldc, M, N, K, act, st);
}
// H = LN(Hin + relu(Hin W1 + b1) W2 + b2); O is scratch
static int s2s_ffn(rl4rs_seq2seq* p, const S2sFfn& f, const float* Hin, float* Hout, int M, hipStream_t st) {
    const int D = p->c.embed_dim, Hd = p->c.hidden_dim;
    S2S_TRY(s2s_lin(p, Hin, f.W1, f.b1, p->F, Hd, M, Hd, D, ACT_RELU, st));
    S2S_TRY(s2s_lin(p, p->F, f.W2, f.b2, p->O, D, M, D, Hd, ACT_NONE, st));
    return s2s_add_ln(p, Hin, p->O, f.g, f.b, Hout, M, st);
}
// keys / values of `M` rows of Xkv into KVout [M, 2 D] = [K | V]
static int s2s_kv(rl4rs_seq2seq* p, const S2sAtt& a, const float* Xkv, float* KVout, int M, hipStream_t st) {
    const int D = p->c.embed_dim;
    S2S_TRY(s2s_lin(p, Xkv, a.Wk, a.bk, KVout, 2 * D, M, D, D, ACT_NONE, st));
    return s2s_lin(p, Xkv, a.Wv, a.bv, KVout + D, 2 * D, M, D, D, ACT_NONE, st);
}
// Hout = LN(Xq + (attention of Xq's rows over KVsrc) Wo + bo); Q, A, O are scratch
static int s2s_att_block(rl4rs_seq2seq* p, const S2sAtt& a, const float* Xq, int Mq, int Lq, const float* KVsrc, const int32_t* ktok, int Lk,
                         int qdiv, int causal, float* Hout, hipStream_t st) {
    const int D = p->c.embed_dim;
    S2S_TRY(s2s_lin(p, Xq, a.Wq, a.bq, p->Q, D, Mq, D, D, ACT_NONE, st));
    hipLaunchKernelGGL(k_s2s_attn<false>, dim3((Mq + 3) / 4), dim3(256), 0, st, p->Q, KVsrc, KVsrc + D, 2 * D, nullptr, nullptr, ktok, 0,
                       p->A, Mq, Lq, Lk, qdiv, D, causal, p->c.token_num);
    RL4RS_LAUNCH_CHECK();
    S2S_TRY(s2s_lin(p, p->A, a.Wo, a.bo, p->O, D, Mq, D, D, ACT_NONE, st));
    return s2s_add_ln(p, Xq, p->O, a.g, a.b, Hout, Mq, st);
}
// encoder of N sequences -> Enc [N * S, D] and the decoder's cross-attention keys / values CKV [N * S, 2 D]
static int s2s_encode(rl4rs_seq2seq* p, int N, const int32_t* enc_tok, hipStream_t st) {
    const int S = p->c.src_len, M = N * S;
    S2S_TRY(s2s_embed(p, enc_tok, S, 0, S, 0, p->L.Eenc, p->X, M, st));
    S2S_TRY(s2s_kv(p, p->L.ea, p->X, p->KV, M, st));
    S2S_TRY(s2s_att_block(p, p->L.ea, p->X, M, S, p->KV, enc_tok, S, 1, 0, p->H1, st));
    S2S_TRY(s2s_ffn(p, p->L.ef, p->H1, p->Enc, M, st));
    return s2s_kv(p, p->L.dc, p->Enc, p->CKV, M, st);
}
static int s2s_transposed_table(rl4rs_seq2seq* p, hipStream_t st) {
    const int V = p->c.token_num, D = p->c.embed_dim;
    hipLaunchKernelGGL(k_s2s_transpose, dim3((V + 31) / 32, (D + 31) / 32), dim3(32, 8), 0, st, p->params + p->L.Edec, p->EdT, V, D, p->Vp);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}
// probabilities of M decoder rows H [M, D] -> out [M, ld]
static int s2s_output(rl4rs_seq2seq* p, const float* H, float* out, int64_t ld, int M, hipStream_t st) {
    const int V = p->c.token_num, D = p->c.embed_dim;
    S2S_TRY(launch_gemm_f32(H, D, p->EdT, p->Vp, p->params + p->L.ob, out, ld, M, V, D, ACT_NONE, st));
    hipLaunchKernelGGL(k_s2s_softmax, dim3(M), dim3(256), 0, st, out, ld, V);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// ---------------------------------------------------------------- training
constexpr size_t S2S_NO_BIAS = ~(size_t)0;
static int s2s_chunk(int Ns) { return std::max(256, (Ns + 15) / 16); }            // at most 16 partials
static int s2s_tn(rl4rs_seq2seq* p, const float* A_, int lda, int M, const float* B_, int ldb, int Nc, int Ns, size_t dW, size_t db,
                  hipStream_t st) {
    return launch_gemm_tn(A_, lda, M, B_, ldb, Nc, Ns, s2s_chunk(Ns), p->tr.part, p->tr.part_b, p->opt.grad + dW,
                          db == S2S_NO_BIAS ? nullptr : p->opt.grad + db, st);
}
static int s2s_nt(rl4rs_seq2seq* p, const float* dy, int64_t ldy, size_t W, float* dx, int M, int Kin, int Nout, hipStream_t st,
                  const float* relu_of = nullptr) {
    return launch_gemm_nt(dy, ldy, p->params + W, Nout, dx, Kin, M, Kin, Nout, st, relu_of, Kin);
}
static int s2s_sum(float* y, const float* a, const float* b, const float* c, const float* e, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_s2s_sum4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, y, a, b, c, e, n);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

static int s2s_train_reserve(rl4rs_seq2seq* p) {
    if (p->tr.arena) return RL4RS_OK;
    S2sTrain& t = p->tr;
    const size_t R = (size_t)p->c.max_rows, D = p->c.embed_dim, Hd = p->c.hidden_dim, V = p->c.token_num;
    std::vector<std::pair<void**, size_t>> reqs;
    auto req = [&](float** slot, size_t n) { reqs.emplace_back(reinterpret_cast<void**>(slot), n * sizeof(float)); };
    req(&t.Xe, R * D); req(&t.KVe, R * 2 * D); req(&t.Xd, R * D); req(&t.KVs, R * 2 * D); req(&t.CKV, R * 2 * D); req(&t.Pr, R * V);
    for (S2sAttSave* a : {&t.ea, &t.ds, &t.dc}) {
        req(&a->Q, R * D); req(&a->Pa, R * S2S_PA); req(&a->AO, R * D); req(&a->xhat, R * D); req(&a->rstd, R); req(&a->H, R * D);
    }
    for (S2sFfnSave* f : {&t.ef, &t.df}) { req(&f->F, R * Hd); req(&f->xhat, R * D); req(&f->rstd, R); req(&f->H, R * D); }
    for (auto& x : t.T) req(&x, R * D);
    for (auto& x : t.G) req(&x, R * D);
    req(&t.GKV, R * 2 * D); req(&t.GP, R * S2S_PA); req(&t.GF, R * Hd); req(&t.dWt, D * V);
    req(&t.part, 16 * D * std::max(std::max(V, D), Hd)); req(&t.part_b, 16 * std::max(std::max(V, 2 * D), Hd));
    req(&t.rowloss, R); req(&t.cnt, 1);
    size_t total = 0;
    for (auto& r : reqs) total += (r.second + 255) / 256 * 256;
    hipError_t e = hipMalloc(&t.arena, total);
    if (e != hipSuccess) {
        set_error("seq2seq_loss_grad: hipMalloc(%zu bytes) failed: %s", total, hipGetErrorString(e));
        t.arena = nullptr;
        return RL4RS_ENOMEM;
    }
    size_t off = 0;
    for (auto& r : reqs) { *r.first = static_cast<char*>(t.arena) + off; off += (r.second + 255) / 256 * 256; }
    return RL4RS_OK;
}

struct S2sDrop { float rate; uint32_t seed, step; };

// forward of an attention block that keeps Q, the probabilities, the attention output and the normalised sum
static int s2s_att_fwd_train(rl4rs_seq2seq* p, const S2sAtt& a, S2sAttSave& sv, const float* Xq, int Mq, int Lq, const float* KV,
                             const int32_t* ktok, int Lk, int causal, const S2sDrop& dr, uint32_t site, hipStream_t st) {
    const int D = p->c.embed_dim;
    S2S_TRY(s2s_lin(p, Xq, a.Wq, a.bq, sv.Q, D, Mq, D, D, ACT_NONE, st));
    hipLaunchKernelGGL(k_s2s_attn<false>, dim3((Mq + 3) / 4), dim3(256), 0, st, sv.Q, KV, KV + D, 2 * D, nullptr, nullptr, ktok, 0, sv.AO, Mq,
                       Lq, Lk, 1, D, causal, p->c.token_num, sv.Pa);
    RL4RS_LAUNCH_CHECK();
    S2S_TRY(s2s_lin(p, sv.AO, a.Wo, a.bo, p->O, D, Mq, D, D, ACT_NONE, st));
    hipLaunchKernelGGL(k_s2s_add_ln_train, dim3((Mq + 3) / 4), dim3(256), 0, st, Xq, p->O, p->params + a.g, p->params + a.b, sv.H, sv.xhat,
                       sv.rstd, Mq, D, dr.rate, dr.seed, dr.step, site);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}
static int s2s_ffn_fwd_train(rl4rs_seq2seq* p, const S2sFfn& f, S2sFfnSave& sv, const float* Hin, int M, const S2sDrop& dr, uint32_t site,
                             hipStream_t st) {
    const int D = p->c.embed_dim, Hd = p->c.hidden_dim;
    S2S_TRY(s2s_lin(p, Hin, f.W1, f.b1, sv.F, Hd, M, Hd, D, ACT_RELU, st));
    S2S_TRY(s2s_lin(p, sv.F, f.W2, f.b2, p->O, D, M, D, Hd, ACT_NONE, st));
    hipLaunchKernelGGL(k_s2s_add_ln_train, dim3((M + 3) / 4), dim3(256), 0, st, Hin, p->O, p->params + f.g, p->params + f.b, sv.H, sv.xhat,
                       sv.rstd, M, D, dr.rate, dr.seed, dr.step, site);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}
// layer norm of a block in reverse: dS -> T[0], dO -> T[1], d gamma / d beta into the gradient
static int s2s_ln_bwd(rl4rs_seq2seq* p, const float* dY, const float* xhat, const float* rstd, size_t g, int M, const S2sDrop& dr,
                      uint32_t site, hipStream_t st) {
    const int D = p->c.embed_dim, chunk = s2s_chunk(M), nz = (M + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_s2s_ln_bwd, dim3((M + 3) / 4), dim3(256), 0, st, dY, xhat, rstd, p->params + g, p->tr.T[0], p->tr.T[1], M, D, dr.rate,
                       dr.seed, dr.step, site);
    hipLaunchKernelGGL(k_s2s_ln_colsum, dim3((D + 63) / 64, nz), dim3(64), 0, st, dY, xhat, M, D, chunk, p->tr.part_b);
    hipLaunchKernelGGL(k_reduce_chunks, dim3((2 * D + 255) / 256), dim3(256), 0, st, p->tr.part_b, 2 * D, nz, p->opt.grad + g);   // gamma | beta
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}
// reverse of an attention block: dY [Mq, D] -> dXq (residual + query side; + key / value side when the block attends over its own
// input, dXkv = NULL) and dXkv (cross-attention: the gradient of the rows the keys / values were projected from)
static int s2s_att_bwd(rl4rs_seq2seq* p, const S2sAtt& a, const S2sAttSave& sv, const float* Xq, int Mq, int Lq, const float* Xkv, int Mk,
                       int Lk, const float* KV, const float* dY, float* dXq, float* dXkv, const S2sDrop& dr, uint32_t site, hipStream_t st) {
    const int D = p->c.embed_dim;
    S2sTrain& t = p->tr;
    S2S_TRY(s2s_ln_bwd(p, dY, sv.xhat, sv.rstd, a.g, Mq, dr, site, st));
    S2S_TRY(s2s_nt(p, t.T[1], D, a.Wo, t.T[2], Mq, D, D, st));                               // dAO
    S2S_TRY(s2s_tn(p, sv.AO, D, D, t.T[1], D, D, Mq, a.Wo, a.bo, st));
    hipLaunchKernelGGL(k_s2s_attn_bwd_q, dim3((Mq + 3) / 4), dim3(256), 0, st, KV, KV + D, 2 * D, sv.Pa, t.T[2], t.GP, t.T[3], Mq, Lq, Lk, D);
    hipLaunchKernelGGL(k_s2s_attn_bwd_kv, dim3((Mk + 3) / 4), dim3(256), 0, st, sv.Q, sv.Pa, t.GP, t.T[2], t.GKV, Mk, Lq, Lk, D);
    RL4RS_LAUNCH_CHECK();
    S2S_TRY(s2s_tn(p, Xq, D, D, t.T[3], D, D, Mq, a.Wq, a.bq, st));
    S2S_TRY(s2s_tn(p, Xkv, D, D, t.GKV, 2 * D, D, Mk, a.Wk, S2S_NO_BIAS, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->opt.grad + a.bk, 0, (size_t)D * 4, st));      // exactly zero: k_s2s_attn_bwd_q
    S2S_TRY(s2s_tn(p, Xkv, D, D, t.GKV + D, 2 * D, D, Mk, a.Wv, a.bv, st));
    S2S_TRY(s2s_nt(p, t.T[3], D, a.Wq, t.T[2], Mq, D, D, st));
    S2S_TRY(s2s_nt(p, t.GKV, 2 * D, a.Wk, t.T[1], Mk, D, D, st));
    S2S_TRY(s2s_nt(p, t.GKV + D, 2 * D, a.Wv, t.T[4], Mk, D, D, st));
    if (dXkv) {
        S2S_TRY(s2s_sum(dXq, t.T[0], t.T[2], nullptr, nullptr, (size_t)Mq * D, st));
        return s2s_sum(dXkv, t.T[1], t.T[4], nullptr, nullptr, (size_t)Mk * D, st);
    }
    return s2s_sum(dXq, t.T[0], t.T[2], t.T[1], t.T[4], (size_t)Mq * D, st);
}
static int s2s_ffn_bwd(rl4rs_seq2seq* p, const S2sFfn& f, const S2sFfnSave& sv, const float* Hin, int M, const float* dY, float* dHin,
                       const S2sDrop& dr, uint32_t site, hipStream_t st) {
    const int D = p->c.embed_dim, Hd = p->c.hidden_dim;
    S2sTrain& t = p->tr;
    S2S_TRY(s2s_ln_bwd(p, dY, sv.xhat, sv.rstd, f.g, M, dr, site, st));
    S2S_TRY(s2s_nt(p, t.T[1], D, f.W2, t.GF, M, Hd, D, st, sv.F));                          // dF, zero where the relu was
    S2S_TRY(s2s_tn(p, sv.F, Hd, Hd, t.T[1], D, D, M, f.W2, f.b2, st));
    S2S_TRY(s2s_tn(p, Hin, D, D, t.GF, Hd, Hd, M, f.W1, f.b1, st));
    S2S_TRY(s2s_nt(p, t.GF, Hd, f.W1, t.T[2], M, D, Hd, st));
    return s2s_sum(dHin, t.T[0], t.T[2], nullptr, nullptr, (size_t)M * D, st);
}

static int s2s_loss_grad(rl4rs_seq2seq* p, int N, const int32_t* enc, const int32_t* dec_in, const int32_t* dec_out, int L, float rate,
                         uint32_t seed, uint32_t step, float* loss_dev, hipStream_t st) {
    const int S = p->c.src_len, D = p->c.embed_dim, V = p->c.token_num, Me = N * S, Md = N * L;
    S2sTrain& t = p->tr;
    const S2sLayout& Y = p->L;
    const S2sDrop dr{rate, seed, step};
    // forward
    S2S_TRY(s2s_embed(p, enc, S, 0, S, 0, Y.Eenc, t.Xe, Me, st));
    S2S_TRY(s2s_kv(p, Y.ea, t.Xe, t.KVe, Me, st));
    S2S_TRY(s2s_att_fwd_train(p, Y.ea, t.ea, t.Xe, Me, S, t.KVe, enc, S, 0, dr, 0, st));
    S2S_TRY(s2s_ffn_fwd_train(p, Y.ef, t.ef, t.ea.H, Me, dr, 1, st));
    S2S_TRY(s2s_kv(p, Y.dc, t.ef.H, t.CKV, Me, st));
    S2S_TRY(s2s_transposed_table(p, st));
    S2S_TRY(s2s_embed(p, dec_in, L, 0, L, 0, Y.Edec, t.Xd, Md, st));
    S2S_TRY(s2s_kv(p, Y.ds, t.Xd, t.KVs, Md, st));
    S2S_TRY(s2s_att_fwd_train(p, Y.ds, t.ds, t.Xd, Md, L, t.KVs, dec_in, L, 1, dr, 2, st));
    S2S_TRY(s2s_att_fwd_train(p, Y.dc, t.dc, t.ds.H, Md, L, t.CKV, enc, S, 0, dr, 3, st));
    S2S_TRY(s2s_ffn_fwd_train(p, Y.df, t.df, t.dc.H, Md, dr, 4, st));
    S2S_TRY(s2s_output(p, t.df.H, t.Pr, V, Md, st));
    // loss and d logits (in place)
    hipLaunchKernelGGL(k_s2s_count, dim3(1), dim3(256), 0, st, dec_in, Md, t.cnt);
    hipLaunchKernelGGL(k_s2s_ce, dim3(Md), dim3(256), 0, st, t.Pr, (int64_t)V, V, dec_in, dec_out, t.cnt, t.rowloss);
    hipLaunchKernelGGL(k_s2s_loss, dim3(1), dim3(256), 0, st, t.rowloss, Md, t.cnt, loss_dev);
    RL4RS_LAUNCH_CHECK();
    // tied output layer: d h = dlogits E_dec; d E_dec (first term) = (h^T dlogits)^T; d bias = column sums of dlogits
    S2S_TRY(launch_gemm_f32(t.Pr, V, p->params + Y.Edec, D, nullptr, t.G[0], D, Md, D, V, ACT_NONE, st));
    S2S_TRY(launch_gemm_tn(t.df.H, D, D, t.Pr, V, V, Md, s2s_chunk(Md), t.part, t.part_b, t.dWt, p->opt.grad + Y.ob, st));
    hipLaunchKernelGGL(k_s2s_transpose, dim3((D + 31) / 32, (V + 31) / 32), dim3(32, 8), 0, st, t.dWt, p->opt.grad + Y.Edec, D, V, D);
    RL4RS_LAUNCH_CHECK();
    // decoder in reverse; G[2] collects the encoder output's gradient
    S2S_TRY(s2s_ffn_bwd(p, Y.df, t.df, t.dc.H, Md, t.G[0], t.G[1], dr, 4, st));
    S2S_TRY(s2s_att_bwd(p, Y.dc, t.dc, t.ds.H, Md, L, t.ef.H, Me, S, t.CKV, t.G[1], t.G[0], t.G[2], dr, 3, st));
    S2S_TRY(s2s_att_bwd(p, Y.ds, t.ds, t.Xd, Md, L, t.Xd, Md, L, t.KVs, t.G[0], t.G[1], nullptr, dr, 2, st));
    hipLaunchKernelGGL(k_s2s_embed_bwd, dim3(V), dim3(256), 0, st, dec_in, Md, t.G[1], p->opt.grad + Y.Edec, D, V, 1);
    RL4RS_LAUNCH_CHECK();
    // encoder in reverse
    S2S_TRY(s2s_ffn_bwd(p, Y.ef, t.ef, t.ea.H, Me, t.G[2], t.G[0], dr, 1, st));
    S2S_TRY(s2s_att_bwd(p, Y.ea, t.ea, t.Xe, Me, S, t.Xe, Me, S, t.KVe, t.G[0], t.G[1], nullptr, dr, 0, st));
    hipLaunchKernelGGL(k_s2s_embed_bwd, dim3(V), dim3(256), 0, st, enc, Me, t.G[1], p->opt.grad + Y.Eenc, D, V, 0);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // namespace

extern "C" {

int64_t rl4rs_seq2seq_param_count(const rl4rs_seq2seq_cfg* cfg) {
    if (s2s_check_cfg(cfg)) return -1;
    return (int64_t)s2s_layout(cfg->token_num, cfg->embed_dim, cfg->hidden_dim).total;
}

int rl4rs_seq2seq_destroy(rl4rs_seq2seq* p) {
    if (!p) return RL4RS_OK;
    if (p->arena) (void)hipFree(p->arena);
    if (p->tr.arena) (void)hipFree(p->tr.arena);
    delete p;
    return RL4RS_OK;
}

int rl4rs_seq2seq_create(const rl4rs_seq2seq_cfg* cfg, const float* params_host, void* stream, rl4rs_seq2seq** out) {
    int rc = s2s_check_cfg(cfg);
    if (rc) return rc;
    RL4RS_REQUIRE(params_host && out, "seq2seq_create: null argument");
    *out = nullptr;
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    rl4rs_seq2seq* p = new rl4rs_seq2seq();
    p->c = *cfg;
    p->L = s2s_layout(cfg->token_num, cfg->embed_dim, cfg->hidden_dim);
    p->Vp = (cfg->token_num + 3) & ~3;
    p->arena = nullptr;
    p->tr.arena = nullptr;
    const size_t R = (size_t)cfg->max_rows, D = cfg->embed_dim, Hd = cfg->hidden_dim, V = cfg->token_num, T1 = S2S_MAXLEN;
    std::vector<std::pair<void**, size_t>> reqs;                 // (pointer slot, bytes)
    auto req = [&](auto** slot, size_t n) { reqs.emplace_back(reinterpret_cast<void**>(slot), n * sizeof(**slot)); };
    req(&p->params, p->L.total); req(&p->pos, (size_t)S2S_MAXLEN * D);
    req(&p->opt.grad, p->L.total); req(&p->opt.m, p->L.total); req(&p->opt.v, p->L.total);
    req(&p->X, R * D); req(&p->Q, R * D); req(&p->KV, R * 2 * D); req(&p->A, R * D); req(&p->O, R * D); req(&p->H1, R * D);
    req(&p->H2, R * D); req(&p->F, R * Hd); req(&p->Enc, R * D); req(&p->CKV, R * 2 * D); req(&p->P, R * V);
    req(&p->EKV, V * 2 * D); req(&p->PKV, (size_t)S2S_MAXLEN * 2 * D); req(&p->EdT, D * (size_t)p->Vp);
    for (int i = 0; i < 2; ++i) { req(&p->sp[i], R * T1); req(&p->prefix[i], R * T1); req(&p->score[i], R); }
    req(&p->cidx, R * S2S_BEAM_MAX); req(&p->cval, R * S2S_BEAM_MAX);
    size_t total = 0;
    for (auto& r : reqs) total += (r.second + 255) / 256 * 256;
    hipError_t e = hipMalloc(&p->arena, total);
    if (e != hipSuccess) {
        set_error("seq2seq_create: hipMalloc(%zu bytes) failed: %s", total, hipGetErrorString(e));
        p->arena = nullptr;
        rl4rs_seq2seq_destroy(p);
        return RL4RS_ENOMEM;
    }
    size_t off = 0;
    for (auto& r : reqs) { *r.first = static_cast<char*>(p->arena) + off; off += (r.second + 255) / 256 * 256; }
    // trigonometric position table: column 2 i = sin(pos / 10000^(2 i / D)), column 2 i + 1 = cos of the same angle
    std::vector<float> pos((size_t)S2S_MAXLEN * D);
    for (int j = 0; j < S2S_MAXLEN; ++j)
        for (size_t c = 0; c < D; ++c) {
            const double ang = (double)j / std::pow(10000.0, (double)(2 * (c / 2)) / (double)D);
            pos[(size_t)j * D + c] = (float)((c & 1) ? std::cos(ang) : std::sin(ang));
        }
    hipStream_t st = (hipStream_t)stream;
    e = hipMemcpyAsync(p->params, params_host, p->L.total * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->EdT, 0, D * (size_t)p->Vp * 4, st);      // the pad columns stay 0
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.grad, 0, p->L.total * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.m, 0, p->L.total * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.v, 0, p->L.total * 4, st);
    if (e == hipSuccess) e = hipMemcpyAsync(p->pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);           // pos is a local: the copy has to be over before it goes
    if (e != hipSuccess) {
        set_error("seq2seq_create: initialisation failed: %s", hipGetErrorString(e));
        rl4rs_seq2seq_destroy(p);
        return RL4RS_EHIP;
    }
    p->opt.params = p->params; p->opt.n = (int64_t)p->L.total; p->opt.t = 0;
    *out = p;
    return RL4RS_OK;
}

int rl4rs_seq2seq_params(rl4rs_seq2seq* p, float** params_dev, float** grad_dev, int64_t* count) {
    return opt_params(RL4RS_OPT(p), params_dev, grad_dev, count, "seq2seq_params");
}
int rl4rs_seq2seq_adam_state(rl4rs_seq2seq* p, float** m_dev, float** v_dev, int64_t* step) {
    return opt_adam_state(RL4RS_OPT(p), m_dev, v_dev, step, "seq2seq_adam_state");
}
int rl4rs_seq2seq_set_adam_step(rl4rs_seq2seq* p, int64_t step) {
    return opt_set_adam_step(RL4RS_OPT(p), step, "seq2seq_set_adam_step");
}
int rl4rs_seq2seq_adam_step(rl4rs_seq2seq* p, float lr, float beta1, float beta2, float eps, void* stream) {
    RL4RS_REQUIRE(p, "seq2seq_adam_step: null handle");
    adam_step(p->opt, p->opt.grad, ADAM_TF, lr, beta1, beta2, eps, nullptr, 0.f, nullptr, (hipStream_t)stream);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_seq2seq_loss_grad(rl4rs_seq2seq* p, int32_t N, const int32_t* enc_tokens_dev, const int32_t* dec_in_dev, const int32_t* dec_out_dev,
                            int32_t L, float dropout_rate, uint32_t seed, uint32_t step, float* loss_dev, void* stream) {
    RL4RS_REQUIRE(p && enc_tokens_dev && dec_in_dev && dec_out_dev && loss_dev, "seq2seq_loss_grad: null argument");
    RL4RS_REQUIRE(L >= 1 && L <= p->c.tgt_len, "seq2seq_loss_grad: L %d outside [1, tgt_len = %d]", L, p->c.tgt_len);
    RL4RS_REQUIRE(N >= 1 && (int64_t)N * std::max(L, p->c.src_len) <= p->c.max_rows,
                  "seq2seq_loss_grad: N %d x max(L %d, src_len %d) rows exceed max_rows %d", N, L, p->c.src_len, p->c.max_rows);
    RL4RS_REQUIRE(dropout_rate >= 0.f && dropout_rate < 1.f, "seq2seq_loss_grad: dropout_rate %g outside [0, 1)", (double)dropout_rate);
    S2S_TRY(s2s_train_reserve(p));
    return s2s_loss_grad(p, N, enc_tokens_dev, dec_in_dev, dec_out_dev, L, dropout_rate, seed, step, loss_dev, (hipStream_t)stream);
}

int rl4rs_seq2seq_forward(rl4rs_seq2seq* p, int32_t N, const int32_t* enc_tokens_dev, const int32_t* dec_tokens_dev, int32_t L,
                          float* probs_dev, void* stream) {
    RL4RS_REQUIRE(p && enc_tokens_dev && dec_tokens_dev && probs_dev, "seq2seq_forward: null argument");
    RL4RS_REQUIRE(L >= 1 && L <= p->c.tgt_len, "seq2seq_forward: L %d outside [1, tgt_len = %d]", L, p->c.tgt_len);
    RL4RS_REQUIRE(N >= 1 && (int64_t)N * std::max(L, p->c.src_len) <= p->c.max_rows,
                  "seq2seq_forward: N %d x max(L %d, src_len %d) rows exceed max_rows %d", N, L, p->c.src_len, p->c.max_rows);
    hipStream_t st = (hipStream_t)stream;
    const int S = p->c.src_len, M = N * L;
    S2S_TRY(s2s_encode(p, N, enc_tokens_dev, st));
    S2S_TRY(s2s_transposed_table(p, st));
    S2S_TRY(s2s_embed(p, dec_tokens_dev, L, 0, L, 0, p->L.Edec, p->X, M, st));
    S2S_TRY(s2s_kv(p, p->L.ds, p->X, p->KV, M, st));
    S2S_TRY(s2s_att_block(p, p->L.ds, p->X, M, L, p->KV, dec_tokens_dev, L, 1, 1, p->H1, st));
    S2S_TRY(s2s_att_block(p, p->L.dc, p->H1, M, L, p->CKV, enc_tokens_dev, S, 1, 0, p->H2, st));
    S2S_TRY(s2s_ffn(p, p->L.df, p->H2, p->X, M, st));
    return s2s_output(p, p->X, probs_dev, p->c.token_num, M, st);
}

int rl4rs_seq2seq_beam(rl4rs_seq2seq* p, int32_t N, const int32_t* enc_tokens_dev, int32_t beam, int32_t target_len,
                       const uint32_t* cand_bits_dev, int32_t* paths_dev, double* scores_dev, float* step_probs_dev, void* stream) {
    RL4RS_REQUIRE(p && enc_tokens_dev && paths_dev && scores_dev, "seq2seq_beam: null argument");
    const int V = p->c.token_num, D = p->c.embed_dim, S = p->c.src_len, B = beam, T = target_len, T1 = T + 1;
    RL4RS_REQUIRE(B >= 1 && B <= S2S_BEAM_MAX, "seq2seq_beam: beam %d outside [1, %d]", B, S2S_BEAM_MAX);
    RL4RS_REQUIRE(B < V, "seq2seq_beam: beam %d is not below token_num %d", B, V);
    RL4RS_REQUIRE(T >= 1 && T <= p->c.tgt_len && T1 <= S2S_MAXLEN, "seq2seq_beam: target_len %d outside [1, min(tgt_len = %d, %d)]", T,
                  p->c.tgt_len, S2S_MAXLEN - 1);
    RL4RS_REQUIRE(N >= 1 && (int64_t)N * std::max(B, S) <= p->c.max_rows, "seq2seq_beam: N %d x max(beam %d, src_len %d) rows exceed max_rows %d",
                  N, B, S, p->c.max_rows);
    hipStream_t st = (hipStream_t)stream;
    const S2sAtt& ds = p->L.ds;
    const int W = (V + 31) / 32;
    if (cand_bits_dev) {                       // candidates_size >= beam, per user: read back before anything is decoded
        int32_t few = 0;
        RL4RS_HIP_TRY(hipMemsetAsync(p->cidx, 0, 4, st));
        hipLaunchKernelGGL(k_s2s_cand_check, dim3((N + 255) / 256), dim3(256), 0, st, cand_bits_dev, N, W, V, B, p->cidx);
        RL4RS_LAUNCH_CHECK();
        RL4RS_HIP_TRY(hipMemcpyAsync(&few, p->cidx, 4, hipMemcpyDeviceToHost, st));
        RL4RS_HIP_TRY(hipStreamSynchronize(st));
        RL4RS_REQUIRE(!few, "seq2seq_beam: a user's candidate set holds fewer tokens than beam %d (candidates_size >= beam)", B);
    }
    S2S_TRY(s2s_encode(p, N, enc_tokens_dev, st));
    S2S_TRY(s2s_transposed_table(p, st));
    // EKV = E_dec [Wk | Wv] (no bias), PKV = pos [Wk | Wv] + [bk | bv]
    S2S_TRY(launch_gemm_f32(p->params + p->L.Edec, D, p->params + ds.Wk, D, nullptr, p->EKV, 2 * D, V, D, D, ACT_NONE, st));
    S2S_TRY(launch_gemm_f32(p->params + p->L.Edec, D, p->params + ds.Wv, D, nullptr, p->EKV + D, 2 * D, V, D, D, ACT_NONE, st));
    S2S_TRY(launch_gemm_f32(p->pos, D, p->params + ds.Wk, D, p->params + ds.bk, p->PKV, 2 * D, T1, D, D, ACT_NONE, st));
    S2S_TRY(launch_gemm_f32(p->pos, D, p->params + ds.Wv, D, p->params + ds.bv, p->PKV + D, 2 * D, T1, D, D, ACT_NONE, st));
    const int cells = N * B * T1;
    hipLaunchKernelGGL(k_s2s_beam_init, dim3((cells + 255) / 256), dim3(256), 0, st, p->prefix[0], p->prefix[1], cells, T1);
    RL4RS_LAUNCH_CHECK();
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        const int live = t == 0 ? 1 : B, R = N * live;
        const uint32_t* bits = t == 0 ? nullptr : cand_bits_dev;             // the reference's first step is unmasked
        // step 0 reads rows 0 .. N - 1 of the [N * B, T1] prefixes as its N rows: every row starts as <START>
        const int tok_ld = T1;
        S2S_TRY(s2s_embed(p, p->prefix[cur], tok_ld, t, 1, t, p->L.Edec, p->X, R, st));
        S2S_TRY(s2s_lin(p, p->X, ds.Wq, ds.bq, p->Q, D, R, D, D, ACT_NONE, st));
        hipLaunchKernelGGL(k_s2s_attn<true>, dim3((R + 3) / 4), dim3(256), 0, st, p->Q, p->EKV, p->EKV + D, 2 * D, p->PKV, p->PKV + D,
                           p->prefix[cur], tok_ld, p->A, R, 1, t + 1, 1, D, 0, V);
        RL4RS_LAUNCH_CHECK();
        S2S_TRY(s2s_lin(p, p->A, ds.Wo, ds.bo, p->O, D, R, D, D, ACT_NONE, st));
        S2S_TRY(s2s_add_ln(p, p->X, p->O, ds.g, ds.b, p->H1, R, st));
        S2S_TRY(s2s_att_block(p, p->L.dc, p->H1, R, 1, p->CKV, enc_tokens_dev, S, live, 0, p->H2, st));
        S2S_TRY(s2s_ffn(p, p->L.df, p->H2, p->X, R, st));
        S2S_TRY(s2s_output(p, p->X, p->P, V, R, st));
        const double* sc = t == 0 ? nullptr : p->score[cur];
        if (V <= 64 * S2S_WAVE_ITEMS)
            hipLaunchKernelGGL(k_s2s_topk_wave, dim3((R + 3) / 4), dim3(256), 0, st, p->P, (int64_t)V, V, B, live, R, sc, bits, W, p->cval,
                               p->cidx);
        else
            hipLaunchKernelGGL(k_s2s_topk, dim3(R), dim3(256), 0, st, p->P, (int64_t)V, V, B, live, sc, bits, W, p->cval, p->cidx);
        RL4RS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_s2s_merge, dim3(N), dim3(64), 0, st, p->P, (int64_t)V, V, B, live, bits, W, p->cval, p->cidx, t, T1,
                           p->prefix[cur], p->prefix[cur ^ 1], p->score[cur ^ 1], p->sp[cur], step_probs_dev ? p->sp[cur ^ 1] : nullptr);
        RL4RS_LAUNCH_CHECK();
        cur ^= 1;
    }
    RL4RS_HIP_TRY(hipMemcpyAsync(paths_dev, p->prefix[cur], (size_t)N * B * T1 * 4, hipMemcpyDeviceToDevice, st));
    RL4RS_HIP_TRY(hipMemcpyAsync(scores_dev, p->score[cur], (size_t)N * B * 8, hipMemcpyDeviceToDevice, st));
    if (step_probs_dev) RL4RS_HIP_TRY(hipMemcpyAsync(step_probs_dev, p->sp[cur], (size_t)N * B * T * 4, hipMemcpyDeviceToDevice, st));
    return RL4RS_OK;
}

}  // extern "C"
