// Device helpers of the fp16x2 GEMM tile (gemm_h16_tile.inc) shared by gemm.hip and by the shadow plane of the observation-sized
// AUGRU launch (augru_xs.hpp), which runs the same tile text.
#pragma once
#include "common.hpp"

namespace rl4rs {

__device__ __forceinline__ float apply_act(float x, int act) {
    switch (act) {
        case ACT_ELU: return x > 0.f ? x : expm1f(x);
        case ACT_SIGMOID: return 1.f / (1.f + expf(-x));
        case ACT_TANH: return tanhf(x);
        case ACT_RELU: return fmaxf(x, 0.f);
        default: return x;
    }
}

struct f4bits_g { float x, y, z, w; };
__device__ __forceinline__ float4 gbuf_load4(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);   // result must be bit_cast (see dien.hip)
    f4bits_g f = __builtin_bit_cast(f4bits_g, v);
    return make_float4(f.x, f.y, f.z, f.w);
}

typedef _Float16 ghalf8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ ghalf8_t gbuf_load_h8(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
    return __builtin_bit_cast(ghalf8_t, v);
}


// Optional second layer chained onto the first (the dense tower: Dense+ELU twice, utils.py:48-54): when the first layer's N
// fits one workgroup (N <= 128, a multiple of 16) its activated output tile never leaves the CU - it is split into the LDS
// planes the main loop has finished with and multiplied by the second weight matrix (K2 = N, N2 <= 128).  Same values, same
// k-blocks and the same MFMA sequence as two launches with the intermediate in HBM: bit-identical results, one launch less.
struct G16Chain {
    const char* wp2; int kb2; const float* bias2; float* c2; int64_t ldc2; int n2; int act2;
    // (unchained launches) second destination of the SAME output elements, row stride ldm: device-visible pinned HOST memory - the
    // observation of a reference-shaped step leaves for the host from the head GEMM's epilogue, as its tiles finish, instead of
    // through a device-to-host copy that can only start when the whole GEMM has ended
    float* mirror; int64_t ldm;
};

}  // namespace rl4rs
