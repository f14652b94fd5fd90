// Streaming classifier metrics on the device: the confusion counts behind keras' AUC(num_thresholds), Precision, Recall, binary accuracy
// and categorical accuracy (script/supervised_train.py:38-42 fits with them), accumulated over any number of updates without a host wait.
// Every accumulator is an int64 fed by integer atomics only, so the counts are exact and the same from run to run.
//
// Binary update: `pred > thr[i]` (float32, thresholds non-decreasing) holds for a prefix of the table, so an element is binned ONCE: its
// bin b = the number of thresholds below it (binary search of the table in LDS; a NaN is above no threshold: b = 0).  A workgroup keeps
// a positives' and a negatives' histogram over b in LDS and flushes the non-zero bins with 64-bit global atomics; read() turns them into
// TP / FP / TN / FN per threshold by suffix sums (TP[i] = positives with b > i).  Included at the end of policy.hip.
#pragma once

namespace rl4rs {

// counts layout: [ pos_hist T+1 | neg_hist T+1 | tp, fp, tn, fn at 0.5 | multiclass correct, rows ]
__global__ __launch_bounds__(256) void k_clf_binary(const float* __restrict__ pred, const int32_t* __restrict__ label, int64_t n,
                                                    const float* __restrict__ thr, int T, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int clf_sm[];
    float* sthr = reinterpret_cast<float*>(clf_sm);              // [T]
    unsigned int* hist = clf_sm + T;                             // [2 (T + 1) + 4]
    const int nb = 2 * (T + 1) + 4;
    for (int i = threadIdx.x; i < T; i += blockDim.x) sthr[i] = thr[i];
    for (int i = threadIdx.x; i < nb; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pred[i];
        const bool pos = label[i] != 0;
        int lo = 0, hi = T;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p > sthr[mid]) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&hist[(pos ? 0 : T + 1) + lo], 1u);
        const bool hit = p > 0.5f;
        atomicAdd(&hist[2 * (T + 1) + (pos ? (hit ? 0 : 3) : (hit ? 1 : 2))], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += blockDim.x)
        if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
}

// categorical accuracy: rows whose FIRST maximum (tf.argmax's tie rule) is the label
__global__ __launch_bounds__(256) void k_clf_multiclass(const float* __restrict__ pred, const int32_t* __restrict__ label, int64_t N, int K,
                                                        unsigned long long* __restrict__ counts) {
    __shared__ unsigned int sm[2];
    if (threadIdx.x < 2) sm[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int ok = 0u, rows = 0u;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const float* x = pred + r * K;
        int best = 0;
        float bv = x[0];
        for (int k = 1; k < K; ++k)
            if (x[k] > bv) { bv = x[k]; best = k; }
        ok += best == label[r] ? 1u : 0u;
        rows += 1u;
    }
    if (ok) atomicAdd(&sm[0], ok);
    if (rows) atomicAdd(&sm[1], rows);
    __syncthreads();
    if (threadIdx.x < 2 && sm[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)sm[threadIdx.x]);
}

}  // namespace rl4rs

struct rl4rs_clfmetrics {
    int T;
    int64_t n_counts;
    float* thr;
    unsigned long long* counts;
};

extern "C" {

int rl4rs_clfmetrics_destroy(rl4rs_clfmetrics* m) {
    if (!m) return RL4RS_OK;
    if (m->thr) (void)hipFree(m->thr);
    if (m->counts) (void)hipFree(m->counts);
    delete m;
    return RL4RS_OK;
}

int rl4rs_clfmetrics_create(int32_t num_thresholds, const float* thresholds, void* stream, rl4rs_clfmetrics** out) {
    RL4RS_REQUIRE(out && thresholds && num_thresholds >= 2 && num_thresholds <= 4096,
                  "clfmetrics_create: num_thresholds must be in [2, 4096] (got %d) and the table non-null", num_thresholds);
    for (int i = 1; i < num_thresholds; ++i)
        RL4RS_REQUIRE(thresholds[i] >= thresholds[i - 1], "clfmetrics_create: the threshold table must not decrease (entry %d)", i);
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    hipStream_t st = (hipStream_t)stream;
    rl4rs_clfmetrics* m = new rl4rs_clfmetrics();
    m->T = num_thresholds;
    m->n_counts = 2 * ((int64_t)num_thresholds + 1) + 4 + 2;
    m->thr = nullptr;
    m->counts = nullptr;
    int rc;
    if ((rc = dev_alloc(&m->thr, (size_t)m->T)) || (rc = dev_alloc(&m->counts, (size_t)m->n_counts))) { rl4rs_clfmetrics_destroy(m); return rc; }
    hipError_t e = hipMemcpyAsync(m->thr, thresholds, (size_t)m->T * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(m->counts, 0, (size_t)m->n_counts * 8, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);               // the table is the caller's
    if (e != hipSuccess) {
        set_error("clfmetrics_create: %s", hipGetErrorString(e));
        rl4rs_clfmetrics_destroy(m);
        return RL4RS_EHIP;
    }
    *out = m;
    return RL4RS_OK;
}

int rl4rs_clfmetrics_reset(rl4rs_clfmetrics* m, void* stream) {
    RL4RS_REQUIRE(m, "clfmetrics_reset: null handle");
    RL4RS_HIP_TRY(hipMemsetAsync(m->counts, 0, (size_t)m->n_counts * 8, (hipStream_t)stream));
    return RL4RS_OK;
}

int rl4rs_clfmetrics_update_binary(rl4rs_clfmetrics* m, int64_t n, const float* pred_dev, const int32_t* label_dev, void* stream) {
    RL4RS_REQUIRE(m && pred_dev && label_dev && n > 0, "clfmetrics_update_binary: bad argument");
    const int64_t blocks = (n + 255) / 256;
    const size_t sm = (size_t)(m->T + 2 * (m->T + 1) + 4) * 4;
    hipLaunchKernelGGL(k_clf_binary, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), sm, (hipStream_t)stream, pred_dev, label_dev, n,
                       m->thr, m->T, m->counts);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_clfmetrics_update_multiclass(rl4rs_clfmetrics* m, int64_t N, int32_t K, const float* pred_dev, const int32_t* label_dev,
                                       void* stream) {
    RL4RS_REQUIRE(m && pred_dev && label_dev && N > 0 && K > 0, "clfmetrics_update_multiclass: bad argument");
    const int64_t blocks = (N + 255) / 256;
    hipLaunchKernelGGL(k_clf_multiclass, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, pred_dev, label_dev, N,
                       K, m->counts + 2 * (m->T + 1) + 4);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// counts_host [4 T + 6] int64: TP [T] | FP [T] | TN [T] | FN [T] | tp, fp, tn, fn at 0.5 | multiclass correct, rows.  Waits for the stream.
int rl4rs_clfmetrics_read(rl4rs_clfmetrics* m, int64_t* counts_host, void* stream) {
    RL4RS_REQUIRE(m && counts_host, "clfmetrics_read: null argument");
    std::vector<unsigned long long> raw((size_t)m->n_counts);
    RL4RS_HIP_TRY(hipMemcpyAsync(raw.data(), m->counts, raw.size() * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    RL4RS_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const int T = m->T;
    int64_t P = 0, Nn = 0;
    for (int b = 0; b <= T; ++b) { P += (int64_t)raw[b]; Nn += (int64_t)raw[T + 1 + b]; }
    int64_t tp = 0, fp = 0;
    for (int i = T - 1; i >= 0; --i) {          // TP[i] = positives above threshold i = those in bins b > i
        tp += (int64_t)raw[i + 1];
        fp += (int64_t)raw[T + 1 + i + 1];
        counts_host[i] = tp;
        counts_host[T + i] = fp;
        counts_host[2 * T + i] = Nn - fp;
        counts_host[3 * T + i] = P - tp;
    }
    for (int k = 0; k < 6; ++k) counts_host[4 * T + k] = (int64_t)raw[2 * (T + 1) + k];
    return RL4RS_OK;
}

}  // extern "C"
