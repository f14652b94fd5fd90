// Sizes of the raw-state training handle (rawtrain.hpp, rawdqn.hpp): its ten variables and the two scratch buffers its backward
// shares with the sample-axis reductions of simtrain.hpp - cx.part (chunk partials of a weight or bias gradient) and cx.wt (the
// transposed weight of a long st_back).  No HIP in here: rl4rs_rawtrain_create sizes the handle from it and a host test compiles it
// alone against every call the backward issues.
#pragma once

#include <initializer_list>

#include "reduce_plan.hpp"

enum { RT_CAT_EMB = 0, RT_SEQ_EMB, RT_DW1, RT_DB1, RT_DW2, RT_DB2, RT_CTX_W, RT_CTX_B, RT_HEAD_W, RT_HEAD_B, RT_COUNT };

namespace {

constexpr int RAWTRAIN_CHUNK = 512;      // rows per chunk of the k_gemm_tn / k_colsum forms on this handle

struct RawTrainDims { int64_t E, U, H, S, Dn, Cn, L, A, max_rows; };

struct RawTrainScratch {
    int64_t F, AE, REC;
    int64_t sizes[RT_COUNT];
    int64_t wmax;              // the widest weight: [F, 256], [Dn, U], [U, U] or [256, AE]
    int64_t wt_floats;         // behind cx.wt: one transposed weight
    int64_t part_floats;       // behind cx.part: one partial of the widest weight per RAWTRAIN_CHUNK rows of max_rows
};

inline RawTrainScratch rawtrain_scratch(const RawTrainDims& d) {
    RawTrainScratch s;
    s.F = d.S * d.E + d.U + d.E;
    s.AE = d.A + 1;
    s.REC = (d.Dn + d.Cn + d.S * d.L + 3) / 4 * 4;
    const int64_t sizes[RT_COUNT] = {d.H * d.E, d.H * d.E, d.Dn * d.U, d.U, d.U * d.U, d.U, s.F * 256, 256, 256 * s.AE, s.AE};
    for (int i = 0; i < RT_COUNT; ++i) s.sizes[i] = sizes[i];
    // every [M, Nc] a weight gradient reduces and every [Kin, Nout] a st_back transposes is one of the four weights; the bias
    // gradients' partials (256, U, AE columns) are narrower than any of them
    s.wmax = 0;
    for (int i : {RT_DW1, RT_DW2, RT_CTX_W, RT_HEAD_W})
        if (sizes[i] > s.wmax) s.wmax = sizes[i];
    s.wt_floats = s.wmax;
    s.part_floats = (d.max_rows + RAWTRAIN_CHUNK - 1) / RAWTRAIN_CHUNK * s.wmax;
    return s;
}

// What one backward over N rows writes into the two buffers: the largest of the four weight gradients (head, context, dense_w2,
// dense_w1 - the calls of rl4rs_rawtrain_loss_grad and rawtrain_backward_from_ctx with their leading dimensions; ldd = Dn from
// unpacked arrays, REC from records), the four bias gradients and the three st_back calls.  `aligned`: whether the operands sit
// on 16-byte boundaries (the 128 x 128 form needs them to).
struct RawTrainNeed { size_t part[8], wt[3]; };      // part: {weight, bias} x {head, ctx, dense_w2, dense_w1}; wt: head, ctx, dense_w2
inline RawTrainNeed rawtrain_need(const RawTrainDims& d, int N, int ldd, bool aligned) {
    const RawTrainScratch s = rawtrain_scratch(d);
    const int F = (int)s.F, AE = (int)s.AE, U = (int)d.U, Dn = (int)d.Dn;
    const TrainCtx x{RAWTRAIN_CHUNK, nullptr, nullptr, 0};
    const float* p = reinterpret_cast<const float*>((uintptr_t)(aligned ? 16 : 4));
    return RawTrainNeed{{st_tn_part_floats(x, p, 256, 256, p, AE, AE, N, false), st_cs_part_floats(x, AE, N),
                         st_tn_part_floats(x, p, F, F, p, 256, 256, N, false), st_cs_part_floats(x, 256, N),
                         st_tn_part_floats(x, p, U, U, p, F, U, N, false), st_cs_part_floats(x, U, N),
                         st_tn_part_floats(x, p, ldd, Dn, p, U, U, N, false), st_cs_part_floats(x, U, N)},
                        {st_back_wt_floats(N, 256, AE), st_back_wt_floats(N, F, 256), st_back_wt_floats(N, U, U)}};
}

}  // namespace
