// Registry of the ahead-of-time instantiations of the narrow fused kernels (kernels_fast.hpp, kernels_fast3.hpp, kernels_traj.hpp):
// shapes of BASELINE.json's configs and the tests.
#include <hip/hip_runtime.h>
#include <mutex>
#include "jit_narrow.hpp"
#include "aot_ops.hpp"

using ShapeC2 = Shape<TBNN_ACT_RELU, TBNN_ACT_NONE, false, 5, 50, 50, 50, 1>;      // configs[1], configs[2]
using ShapeC1 = Shape<TBNN_ACT_RELU, TBNN_ACT_NONE, false, 1, 10, 10, 1>;          // configs[0]
using ShapeTR = Shape<TBNN_ACT_TANH, TBNN_ACT_NONE, false, 1, 10, 10, 10, 1>;      // Examples/trainRegression.py
using ShapeT3 = Shape<TBNN_ACT_SIGMOID, TBNN_ACT_NONE, false, 4, 7, 3>;            // test shape: last layer on the MFMA path

typedef int (*StampedLaunch)(int, hipStream_t, const NetDev*, const float*, const float*, const float*, const float*, long, float*, int, double*,
                             int, ChainStride, unsigned long long*);
static FusedOps g_narrow[4];
static const StampedLaunch g_stamped[4] = {&JitNarrow<ShapeC2, true>::launch_stamped, &JitNarrow<ShapeC1, true>::launch_stamped,
                                           &JitNarrow<ShapeTR, true>::launch_stamped, &JitNarrow<ShapeT3, false>::launch_stamped};
static std::once_flag g_narrow_once;

const FusedOps* narrow_find(const NetDev& nd) {
    std::call_once(g_narrow_once, [] {
        JitNarrow<ShapeC2, true>::fill(&g_narrow[0], "fast3<relu;5,50,50,50,1>");
        JitNarrow<ShapeC1, true>::fill(&g_narrow[1], "fast3<relu;1,10,10,1>");
        JitNarrow<ShapeTR, true>::fill(&g_narrow[2], "fast3<tanh;1,10,10,10,1>");
        JitNarrow<ShapeT3, false>::fill(&g_narrow[3], "fast<sigmoid;4,7,3>");
    });
    for (const FusedOps& o : g_narrow) if (fused_ops_match(o, nd)) return &o;
    return nullptr;
}

int narrow_launch_stamped(const FusedOps* o, int grid, hipStream_t st, const NetDev& nd, const float* qimg, const float* eta, const float* X,
                          const float* Y, long n, float* slabs, int pitch, double* pstat, unsigned long long* stamps) {
    for (int i = 0; i < 4; ++i)
        if (o == &g_narrow[i]) return g_stamped[i](grid, st, &nd, qimg, eta, X, Y, n, slabs, pitch, pstat, 1, ChainStride{0, 0, 0, nullptr, 0}, stamps);
    return -1;
}
