// Registry of the ahead-of-time instantiations of the mid-width fused kernel (kernels_mid.hpp).
#include <hip/hip_runtime.h>
#include <mutex>
#include "jit_mid.hpp"
#include "aot_ops.hpp"

using MShapeC5 = Shape<TBNN_ACT_RELU, TBNN_ACT_SIGMOID, true, 20, 100, 100, 2>;         // BASELINE configs[4]
using MShapeT1 = Shape<TBNN_ACT_TANH, TBNN_ACT_NONE, false, 4, 24, 40, 1>;              // test: ragged widths, one middle layer
using MShapeT2 = Shape<TBNN_ACT_SIGMOID, TBNN_ACT_SIGMOID, true, 20, 32, 48, 2>;        // test: widths % 16 == 0 (ones slot in its own tile)
using MShapeT3 = Shape<TBNN_ACT_RELU, TBNN_ACT_NONE, false, 7, 33, 18, 50, 2>;          // test: two middle layers

static FusedOps g_mid[4];
static std::once_flag g_mid_once;

const FusedOps* mid_find(const NetDev& nd) {
    std::call_once(g_mid_once, [] {
        JitMid<MShapeC5>::fill(&g_mid[0], "mid<relu,sigmoid,bernoulli;20,100,100,2>");
        JitMid<MShapeT1>::fill(&g_mid[1], "mid<tanh;4,24,40,1>");
        JitMid<MShapeT2>::fill(&g_mid[2], "mid<sigmoid,sigmoid,bernoulli;20,32,48,2>");
        JitMid<MShapeT3>::fill(&g_mid[3], "mid<relu;7,33,18,50,2>");
    });
    for (const FusedOps& o : g_mid) if (fused_ops_match(o, nd)) return &o;
    return nullptr;
}

#ifdef MID_STAMPS
extern "C" int tbnn_debug_mid_stamps(unsigned long long* out64) {
    return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_mid_stamps), 64 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
