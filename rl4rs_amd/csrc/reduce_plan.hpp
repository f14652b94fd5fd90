// Which form the sample-axis reductions of simtrain.hpp (st_tn / st_cs / st_tn_cs / st_back) take for a call, and how many floats of
// the caller's scratch (TrainCtx::part, TrainCtx::wt) that form writes.  No HIP in here: the launch code includes it for the
// selection, a handle's create for its sizing, and a host test compiles it alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

// sample-axis reductions / transposed-weight GEMM over an explicit number of samples
struct TrainCtx { int chunk; float* part; float* wt; size_t part_cap = 0; };       // part_cap: floats behind `part` (0 = sized for `chunk` only)

// Long reductions with wide outputs go through the LDS-tiled 128 x 128 form (k_gemm_tn_t128, policy.hip); the chunk count is chosen
// to give every CU a workgroup (at most 64 chunks: the partials are summed by k_reduce_chunks4) within what `part` holds.  Returns the chunk count, 0 = not applicable (caller: k_gemm_tn).
inline int tn_t128_plan(const TrainCtx& x, const float* A, int lda, int M, const float* B, int ldb, int Nc, int Ns, bool bias, int* chunk_out) {
    if (Ns < 4096 || M < 64 || Nc < 64 || (lda | ldb | M | Nc) % 4 != 0 || ((uintptr_t)A | (uintptr_t)B) % 16 != 0) return 0;
    const int tiles = ((M + 127) / 128) * ((Nc + 127) / 128);
    int nz = (256 + tiles - 1) / tiles;
    if (nz > 64) nz = 64;
    const size_t per = (size_t)M * Nc + (bias ? Nc : 0);
    const size_t cap = x.part_cap ? x.part_cap : (size_t)((Ns + x.chunk - 1) / x.chunk) * per;
    if ((size_t)nz * per > cap) nz = (int)(cap / per);
    if (nz < 1) return 0;
    int chunk = (((Ns + nz - 1) / nz) + 15) / 16 * 16;
    if (chunk < 64) chunk = 64;
    *chunk_out = chunk;
    return (Ns + chunk - 1) / chunk;
}
constexpr int TN4_MAX_SAMPLES = 1024;      // up to here the whole sample axis is one workgroup's (four waves x Ns / 4 samples)

// floats of x.part that st_tn (bias = false) / st_tn_cs (bias = true) write for this call: one partial per chunk, none when a single
// workgroup or a single chunk writes the destination itself
inline size_t st_tn_part_floats(const TrainCtx& x, const float* A, int lda, int M, const float* B, int ldb, int Nc, int Ns, bool bias) {
    if (Ns <= TN4_MAX_SAMPLES) return 0;
    const size_t per = (size_t)M * Nc + (bias ? Nc : 0);
    int big_chunk = 0;
    if (const int bz = tn_t128_plan(x, A, lda, M, B, ldb, Nc, Ns, bias, &big_chunk)) return bz > 1 ? (size_t)bz * per : 0;
    const int nz = (Ns + x.chunk - 1) / x.chunk;
    return nz > 1 ? (size_t)nz * per : 0;
}
inline size_t st_cs_part_floats(const TrainCtx& x, int Nc, int Ns) {
    const int nz = (Ns + x.chunk - 1) / x.chunk;
    return nz > 1 ? (size_t)nz * Nc : 0;
}
// st_back: minibatch-sized calls need no transposed weight copy (k_gemm_nt, 32 x 32 tiles); the others transpose W [Kin, Nout] into
// x.wt.  (The bound is on the ROW count as well - the 16 384-row input gradients of the simulator trainers' recurrent layers took
// the k_gemm_nt form at up to 94 us a call)
inline bool st_back_transposes(int Ns, int Kin) {
    return !(Ns <= 2048 && (int64_t)((Ns + 127) / 128) * ((Kin + 63) / 64) < 512);
}
inline size_t st_back_wt_floats(int Ns, int Kin, int Nout) { return st_back_transposes(Ns, Kin) ? (size_t)Kin * Nout : 0; }

}  // namespace
