// Beam search over Exact-K's pointer decoder: the kernels that serve ONE USER PER WORKGROUP with all of its live beams.
// Included by exactk.hip inside its namespace, after the single-path decoder kernels whose arithmetic these repeat per beam
// (same summation orders: a beam of width 1 computes the logits of the greedy decode).
//
// The B beams of a user share enc and the encoded references R = enc W_ref; each beam has its own query vector c_b.  A workgroup
// reads every R row (and every enc row) once and forms the B sums from it, where N * B replicated rows would read it B times.
// Decoder rows: r = n * live + b, live = 1 at step 0 (one beam per user is live) and B afterwards.
//
// Per-beam history.  The intra-attention of step t reads the cell outputs Hout[j] and their W_bef products Bef[j] of the beam's own
// ancestors, j < t.  They stay where step j wrote them; an ancestor table anc[j][r] (int32 [9, N * B]) names the row of step j that
// row r descends from, and every selection rewrites the 9 ints per beam instead of copying up to 2 * 8 * D floats per beam.
#pragma once

constexpr int XK_BEAM_MAX = 8;
constexpr float XK_NEG = -3.4028235e38f;       // a candidate that is disallowed or already taken

// sc[b * A + a] = sum_d v[d] tanh(R[n, a, d] + c_b[d]) for the live beams; a wave per candidate, every R row read once
__device__ __forceinline__ void xk_beam_scores(const float* __restrict__ Rn, const float* cs, const float* vs, float* sc, int A, int D,
                                               int live) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int a = wave; a < A; a += 4) {
        const float* r = Rn + (size_t)a * D;
        float s[XK_BEAM_MAX];
#pragma unroll
        for (int b = 0; b < XK_BEAM_MAX; ++b) s[b] = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float rv = r[d], vv = vs[d];
#pragma unroll
            for (int b = 0; b < XK_BEAM_MAX; ++b)
                if (b < live) s[b] += vv * tanhf(rv + cs[b * D + d]);
        }
#pragma unroll
        for (int b = 0; b < XK_BEAM_MAX; ++b)
            if (b < live) {
                const float w = xk_wave_sum(s[b]);
                if (lane == 0) sc[b * A + a] = w;
            }
    }
}
// max and sum of exp(sc - max) of every live beam, a wave per beam -> red[2 b], red[2 b + 1]
__device__ __forceinline__ void xk_beam_softmax_stats(const float* sc, int A, int live, float* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = wave; b < live; b += 4) {
        const float* s = sc + b * A;
        float mx = XK_NEG;
        for (int a = lane; a < A; a += 64) mx = fmaxf(mx, s[a]);
        mx = xk_wave_max(mx);
        float se = 0.f;
        for (int a = lane; a < A; a += 64) se += expf(s[a] - mx);
        se = xk_wave_sum(se);
        if (lane == 0) { red[2 * b] = mx; red[2 * b + 1] = se; }
    }
}

// x_t and the parent's state of every beam row (t >= 1): XH[r] = [enc[r / B, prefix[r][t - 1]] | h of the parent], Cin[r] = c of the parent
__global__ void k_xk_beam_gather(int t, int rows, int B, int stride, int A, int D, const float* __restrict__ enc,
                                 const int32_t* __restrict__ prefix, const int32_t* __restrict__ anc, const float* __restrict__ Hprev,
                                 const float* __restrict__ Cprev, float* __restrict__ XH, float* __restrict__ Cin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * D) return;
    const int r = i / D, d = i - r * D, n = r / B;
    const int a = min(max(prefix[r * XK_T + t - 1], 0), A - 1);
    const int pr = anc[(size_t)(t - 1) * stride + r];
    float* row = XH + (size_t)r * 2 * D;
    row[d] = enc[((size_t)n * A + a) * D + d];
    row[D + d] = Hprev[(size_t)pr * D + d];
    Cin[i] = Cprev[(size_t)pr * D + d];
}

// k_xk_intra_fwd along the beam's own ancestors: Hout, Bef [T][stride][D] as the steps wrote them, Qb and intra [rows][D] of this step
__global__ __launch_bounds__(256) void k_xk_beam_intra(int t, int stride, int D, const float* __restrict__ Bef, const float* __restrict__ Qb,
                                                       const float* __restrict__ Hout, const int32_t* __restrict__ anc,
                                                       const float* __restrict__ v_dec, float* __restrict__ intra) {
    __shared__ float s_sc[XK_T];
    __shared__ int s_row[XK_T];
    const int r = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* out = intra + (size_t)r * D;
    if (t == 0) {
        for (int d = threadIdx.x; d < D; d += 256) out[d] = 0.f;
        return;
    }
    if ((int)threadIdx.x < t) s_row[threadIdx.x] = anc[(size_t)threadIdx.x * stride + r];
    __syncthreads();
    if (t == 1) {
        for (int d = threadIdx.x; d < D; d += 256) out[d] = Hout[(size_t)s_row[0] * D + d];
        return;
    }
    const float* qb = Qb + (size_t)r * D;
    for (int j = wave; j < t; j += 4) {
        const float* bef = Bef + ((size_t)j * stride + s_row[j]) * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += v_dec[d] * tanhf(bef[d] + qb[d]);
        s = xk_wave_sum(s);
        if (lane == 0) s_sc[j] = s;
    }
    __syncthreads();
    float mx = s_sc[0];
    for (int j = 1; j < t; ++j) mx = fmaxf(mx, s_sc[j]);
    float p[XK_T], se = 0.f;
    for (int j = 0; j < t; ++j) { p[j] = expf(s_sc[j] - mx); se += p[j]; }
    for (int j = 0; j < t; ++j) p[j] = p[j] / se;
    for (int d = threadIdx.x; d < D; d += 256) {
        float s = 0.f;
        for (int j = 0; j < t; ++j) s += p[j] * Hout[((size_t)j * stride + s_row[j]) * D + d];
        out[d] = s;
    }
}

// LDS of the two per-user kernels: sc [live * A] | cs [live * D] | vs [D] | red [16] | acc [parts * live * D] (glimpse)
// glimpse of the live beams of user n: p_b = softmax over ALL candidates, q_b = sum_a p_b[a] enc[n, a]; R and enc rows read once
__global__ __launch_bounds__(256) void k_xk_beam_glimpse(int A, int D, int live, const float* __restrict__ R, const float* __restrict__ Cg,
                                                         const float* __restrict__ v, const float* __restrict__ enc,
                                                         float* __restrict__ qout) {
    extern __shared__ float sm[];
    float *sc = sm, *cs = sc + live * A, *vs = cs + live * D, *red = vs + D, *acc = red + 16;
    const int n = blockIdx.x;
    for (int i = threadIdx.x; i < live * D; i += 256) cs[i] = Cg[(size_t)n * live * D + i];
    for (int d = threadIdx.x; d < D; d += 256) vs[d] = v[d];
    __syncthreads();
    xk_beam_scores(R + (size_t)n * A * D, cs, vs, sc, A, D, live);
    __syncthreads();
    xk_beam_softmax_stats(sc, A, live, red);
    __syncthreads();
    for (int i = threadIdx.x; i < live * A; i += 256) {
        const int b = i / A;
        sc[i] = expf(sc[i] - red[2 * b]) / red[2 * b + 1];
    }
    __syncthreads();
    const int parts = D >= 256 ? 1 : 256 / D, Dw = D >= 256 ? 256 : D;
    const int part = threadIdx.x / Dw, dl = threadIdx.x - part * Dw;
    const float* en = enc + (size_t)n * A * D;
    if (part < parts)
        for (int d = dl; d < D; d += Dw) {
            float s[XK_BEAM_MAX];
#pragma unroll
            for (int b = 0; b < XK_BEAM_MAX; ++b) s[b] = 0.f;
            for (int a = part; a < A; a += parts) {
                const float e = en[(size_t)a * D + d];
#pragma unroll
                for (int b = 0; b < XK_BEAM_MAX; ++b)
                    if (b < live) s[b] = fmaf(sc[b * A + a], e, s[b]);
            }
#pragma unroll
            for (int b = 0; b < XK_BEAM_MAX; ++b)
                if (b < live) acc[(part * live + b) * D + d] = s[b];
        }
    __syncthreads();
    for (int i = threadIdx.x; i < live * D; i += 256) {
        const int b = i / D, d = i - b * D;
        float s = 0.f;
        for (int pp = 0; pp < parts; ++pp) s += acc[(pp * live + b) * D + d];
        qout[(size_t)n * live * D + i] = s;
    }
}

// Pointer scores of the live beams of user n, each beam's own allowed set, the candidate scores
//   acc[b] + (logit[b, a] - logsumexp_allowed(logit[b, :]))
// and the best B of them in descending order, equal scores by the smaller flat index b * A + a (B rounds of a block-wide arg-max
// over LDS: wave reductions, then the four waves' winners).  New beam k takes its parent's prefix and ancestor row; row indices of
// the in-arrays are n * live + b, of the out-arrays n * B + k.  Trace pointers [N, 9, B] are optional.
__global__ __launch_bounds__(256) void k_xk_beam_select(int t, int A, int D, int live, int B, int stride, const float* __restrict__ R,
                                                        const float* __restrict__ Cp, const float* __restrict__ v,
                                                        const uint8_t* __restrict__ loc, const uint8_t* __restrict__ special,
                                                        const int32_t* __restrict__ prefix_in, const float* __restrict__ acc_in,
                                                        const int32_t* __restrict__ anc_in, int32_t* __restrict__ prefix_out,
                                                        float* __restrict__ acc_out, int32_t* __restrict__ anc_out,
                                                        int32_t* __restrict__ parent_tr, int32_t* __restrict__ token_tr,
                                                        float* __restrict__ score_tr) {
    extern __shared__ float sm[];
    float *sc = sm, *cs = sc + live * A, *vs = cs + live * D, *red = vs + D;
    __shared__ int s_prev[XK_BEAM_MAX][XK_T];
    __shared__ int s_any[XK_BEAM_MAX];
    __shared__ float s_acc[XK_BEAM_MAX];
    __shared__ float s_wv[4];
    __shared__ int s_wi[4];
    __shared__ float s_selv[XK_BEAM_MAX];
    __shared__ int s_sel[XK_BEAM_MAX];
    const int n = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int LA = live * A;
    for (int i = threadIdx.x; i < live * D; i += 256) cs[i] = Cp[(size_t)n * live * D + i];
    for (int d = threadIdx.x; d < D; d += 256) vs[d] = v[d];
    if ((int)threadIdx.x < live) {
        const int b = threadIdx.x, r = n * live + b;
        int any = 0;
        for (int j = 0; j < t; ++j) {
            const int a = min(max(prefix_in[r * XK_T + j], 0), A - 1);
            s_prev[b][j] = a;
            any |= special[a];
        }
        s_any[b] = any;
        s_acc[b] = t == 0 ? 0.f : acc_in[r];
    }
    __syncthreads();
    xk_beam_scores(R + (size_t)n * A * D, cs, vs, sc, A, D, live);
    __syncthreads();
    for (int i = threadIdx.x; i < LA; i += 256) {
        const int b = i / A, a = i - b * A;
        if (!xk_allowed(a, t, A, loc, special, s_prev[b], s_any[b] != 0)) sc[i] = XK_PAD;
    }
    __syncthreads();
    xk_beam_softmax_stats(sc, A, live, red);
    __syncthreads();
    for (int i = threadIdx.x; i < LA; i += 256) {
        const int b = i / A;
        const float l = sc[i];
        sc[i] = l == XK_PAD ? XK_NEG : s_acc[b] + (l - (logf(red[2 * b + 1]) + red[2 * b]));
    }
    __syncthreads();
    for (int k = 0; k < B; ++k) {
        float best = XK_NEG;
        int bi = 0x7fffffff;
        for (int i = threadIdx.x; i < LA; i += 256)
            if (sc[i] > best) { best = sc[i]; bi = i; }
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { s_wv[wave] = best; s_wi[wave] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            best = s_wv[0];
            bi = s_wi[0];
            for (int w = 1; w < 4; ++w)
                if (s_wv[w] > best || (s_wv[w] == best && s_wi[w] < bi)) { best = s_wv[w]; bi = s_wi[w]; }
            bi = min(bi, LA - 1);              // (the allowed sets hold B candidates: create's 9 usable items per location)
            s_sel[k] = bi;
            s_selv[k] = best;
            sc[bi] = XK_NEG;
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < B) {
        const int k = threadIdx.x, f = s_sel[k], par = f / A, tok = f - par * A;
        const int ro = n * B + k, ri = n * live + par;
        for (int j = 0; j < t; ++j) {
            prefix_out[ro * XK_T + j] = s_prev[par][j];
            anc_out[(size_t)j * stride + ro] = anc_in[(size_t)j * stride + ri];
        }
        prefix_out[ro * XK_T + t] = tok;
        anc_out[(size_t)t * stride + ro] = ri;
        acc_out[ro] = s_selv[k];
        const size_t o = ((size_t)n * XK_T + t) * B + k;
        if (parent_tr) parent_tr[o] = par;
        if (token_tr) token_tr[o] = tok;
        if (score_tr) score_tr[o] = s_selv[k];
    }
}
