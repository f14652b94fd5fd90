// Translation unit of k_augru_xs alone (augru_xs.hpp): k_augru_x's 32-row form with the shadow plane of an observation-sized
// forward.  Its own unit so that the four instantiations of augru_x.hip are not compiled beside it and keep their code (instantiations
// of one template compiled together move each other's register allocation).  Built like augru_x.hip; floating-point contraction is
// off in every unit, so the category branch and the GEMM tile compute here what they compute in dien.hip and gemm.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "augru_xs.hpp"
#include "dien_plan.hpp"      // augru_tiles: the row-tile rule

namespace rl4rs {

int augru_xs_prepare() {
    int rc;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_augru_xs<false>), augru_x_smem(1)))) return rc;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_augru_xs<true>), augru_x_smem(1)))) return rc;
    return 0;
}

// grid (32-row tiles, S + 1); the caller has checked the conditions (dien_plan: shadow)
void augru_xs_launch(int n_seq, hipStream_t st, const RecurArgs& a, const AugruShadowArgs& sh) {
    const dim3 grid((unsigned)augru_tiles(false, a.n_rows, 1), n_seq + 1), block(512);
    if (a.lead[0]) hipLaunchKernelGGL((k_augru_xs<true>), grid, block, augru_x_smem(1), st, a, sh);
    else hipLaunchKernelGGL((k_augru_xs<false>), grid, block, augru_x_smem(1), st, a, sh);
}

}  // namespace rl4rs
