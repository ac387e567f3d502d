// The ahead-of-time kernel instantiations, one translation unit per family (tbnn_narrow.hip, tbnn_mid.hip, tbnn_wide.hip,
// tbnn_tall.hip), compiled side by side: each family's shapes as FusedOps tables, the interface a run-time compiled kernel
// library registers.
#pragma once
#include "common.hpp"
#include "fused_ops.hpp"

// null: no ahead-of-time instantiation of the family covers this network
const FusedOps* narrow_find(const NetDev& nd);
const FusedOps* mid_find(const NetDev& nd);
const FusedOps* wide_find(const NetDev& nd);
const FusedOps* tall_find(const NetDev& nd);
// diagnostic (tbnn_debug_stamps): one launch of a narrow_find table's kernel that writes workgroup 0's stamps (-1: not such a table)
int narrow_launch_stamped(const FusedOps* o, int grid, hipStream_t st, const NetDev& nd, const float* qimg, const float* eta, const float* X,
                          const float* Y, long n, float* slabs, int pitch, double* pstat, unsigned long long* stamps);
#ifdef TBNN_TILE_STAMPS
// diagnostic build only: tbnn_narrow.hip's copy of the shader-clock stamps (jit_narrow.hpp)
extern "C" int tbnn_jit_tile_stamps(unsigned long long* out64);
#endif
