// Registry of the ahead-of-time instantiations of the wide-layer kernels (kernels_wide.hpp).
#include <hip/hip_runtime.h>
#include <mutex>
#include "jit_wide.hpp"
#include "aot_ops.hpp"

using WShapeC4 = Shape<TBNN_ACT_RELU, TBNN_ACT_NONE, false, 10, 200, 200, 200, 1>;      // BASELINE configs[3]
using WShapeC5 = Shape<TBNN_ACT_RELU, TBNN_ACT_SIGMOID, true, 20, 100, 100, 2>;         // BASELINE configs[4]
using WShapeT1 = Shape<TBNN_ACT_TANH, TBNN_ACT_NONE, false, 3, 20, 36, 2>;              // test: ragged widths, one middle layer
using WShapeT2 = Shape<TBNN_ACT_SIGMOID, TBNN_ACT_SIGMOID, true, 20, 32, 16, 48, 2>;    // test: widths % 16 == 0 (ones slot in its own tile)

template <> struct WideForceStream<WShapeT2> { static constexpr bool value = true; };   // keeps the ring path under the small-shape tests

static FusedOps g_wide[4];
static std::once_flag g_wide_once;

const FusedOps* wide_find(const NetDev& nd) {
    std::call_once(g_wide_once, [] {
        JitWide<WShapeC4>::fill(&g_wide[0], "wide<relu;10,200,200,200,1>");
        JitWide<WShapeC5>::fill(&g_wide[1], "wide<relu,sigmoid,bernoulli;20,100,100,2>");
        JitWide<WShapeT1>::fill(&g_wide[2], "wide<tanh;3,20,36,2>");
        JitWide<WShapeT2>::fill(&g_wide[3], "wide<sigmoid,sigmoid,bernoulli;20,32,16,48,2>");
    });
    for (const FusedOps& o : g_wide) if (fused_ops_match(o, nd)) return &o;
    return nullptr;
}

#ifdef WIDE_STAMPS
extern "C" int tbnn_debug_wide_stamps(unsigned long long* out256) {
    return hipMemcpyFromSymbol(out256, HIP_SYMBOL(g_wide_stamps), 256 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
