// instantiations of the Winograd F(2x2,3x3) relevance conv on the exact bf16 splits (conv_wino_b6.h): 56 / 28 / 14-pixel maps
#include "conv_launch.h"
#include "conv_wino_b6.h"
namespace lrpx {
// LRPX_B6_WINO / lrpx_set_b6_wino bit 8 (on by default): every staging thread fetches its whole patch; off: column sharing between lanes
#define WINO_LEGACY (b6_wino_bits() & 8)
int launch_b6_56_wino(const ConvArgs& a, hipStream_t s) { return WINO_LEGACY ? launch_conv_wino_b6<56, false>(a, s) : launch_conv_wino_b6<56, true>(a, s); }
int launch_b6_28_wino(const ConvArgs& a, hipStream_t s) { return WINO_LEGACY ? launch_conv_wino_b6<28, false>(a, s) : launch_conv_wino_b6<28, true>(a, s); }
int launch_b6_14_wino(const ConvArgs& a, hipStream_t s) { return WINO_LEGACY ? launch_conv_wino_b6<14, false>(a, s) : launch_conv_wino_b6<14, true>(a, s); }
#undef WINO_LEGACY
}
