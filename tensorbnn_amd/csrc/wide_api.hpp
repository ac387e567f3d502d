// Workgroup plan of the wide-layer path (kernels_wide.hpp): what FusedOps::plan fills and FusedOps::wlaunch reads.
#pragma once
#include <hip/hip_runtime.h>
#include "common.hpp"

// (id, fwd_ok: no longer read; they keep the layout the run-time libraries of TBNN_JIT_ABI 6 were built against)
struct WidePlan {
    int id = -1;
    int gridA = 0;               // k_chain_wide workgroups (= entries of pstat)
    int gridB = 0;               // k_dw_wide workgroups
    int wg_lo[TBNN_MAX_LAYERS + 1] = {0};
    size_t store_floats = 0;     // a_l / delta_l blocks
    size_t slabA_floats = 0;     // gridA x compact slab (first + last layer)
    size_t slabB_floats = 0;     // gridB x middle-layer slab
    int img_floats = 0;
    int fwd_ok = 0;
};
