// Store address map of k_gru_h16r (gru_roles.hpp): which piece of a workgroup's 32 x 128 state tile every u-role thread writes at step
// t, and where it lands in the h1 cache [slot][L][128] and in its fragment-order copy h1f [slot][NT][8][64][8] (din_x.hpp).  Plain
// constexpr functions, so that tests/test_gru_frag_map_host.py compiles this very file with the host compiler and replays it.
#pragma once

#if defined(__HIPCC__)
#define GFM_FN __host__ __device__ constexpr
#else
#define GFM_FN constexpr
#endif

namespace gfm {

constexpr int NH = 128;            // hidden columns
constexpr int LDH = NH + 4;        // leading dimension (floats) of the fp32 state plane in LDS
constexpr int THREADS = 256;       // u-role threads of a workgroup (waves 4..7), j = tid - 256
constexpr int PIECES = 4;          // 16-byte pieces per thread and step: 32 rows x 32 pieces of a row

// piece i of u-role thread j: row of the tile, 4-column group of the row
GFM_FN int piece_row(int j, int i) { return (i * THREADS + j) >> 5; }
GFM_FN int piece_c4(int j, int i) { return (i * THREADS + j) & 31; }

// byte offset of columns [4 c4, 4 c4 + 4) of (tile row, step t) from the tile's first slot in h1
GFM_FN int h1_off(int row, int t, int c4, int L) { return ((row * L + t) * NH + c4 * 4) * 4; }

// ... and in h1f: [row][n = t / 32][kb = e / 16][lane = t % 32 + 32 * ((e % 16) / 8)][e % 8], e = 4 c4
GFM_FN int h1f_off(int row, int t, int c4, int NT) {
    const int e = c4 * 4, n = t >> 5, kb = e >> 4, lane = (t & 31) + 32 * ((e & 15) >> 3);
    return ((((row * NT + n) * 8 + kb) * 64 + lane) * 8 + (e & 7)) * 4;
}
// Both are sums of a (row, c4) part and a step part: the kernel keeps the first per lane and adds the second as a scalar offset.
GFM_FN int h1_lane(int row, int c4, int L) { return h1_off(row, 0, c4, L); }
GFM_FN int h1_step(int t, int L) { return h1_off(0, t, 0, L); }
GFM_FN int h1f_lane(int row, int c4, int NT) { return h1f_off(row, 0, c4, NT); }
GFM_FN int h1f_step(int t, int NT) { return h1f_off(0, t, 0, NT); }

// The zero tail (steps L .. 32 NT - 1 of the last step tile, which k_h1_frag leaves zero): zero piece z of the tile,
// z in [0, (32 NT - L) * 1024), is (row, step, c4) =
GFM_FN int tail_row(int z) { return (z >> 5) & 31; }
GFM_FN int tail_t(int z, int L) { return L + (z >> 10); }
GFM_FN int tail_c4(int z) { return z & 31; }

}  // namespace gfm
