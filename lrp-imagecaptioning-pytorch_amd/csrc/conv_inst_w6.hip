// instantiations of the Winograd F(2x2,3x3) relevance conv on the exact bf16 splits (conv_wino_b6.h): 56 / 28 / 14-pixel maps
#include "conv_launch.h"
#include "conv_wino_b6.h"
namespace lrpx {
int launch_b6_56_wino(const ConvArgs& a, hipStream_t s) { return launch_conv_wino_b6<56>(a, s); }
int launch_b6_28_wino(const ConvArgs& a, hipStream_t s) { return launch_conv_wino_b6<28>(a, s); }
int launch_b6_14_wino(const ConvArgs& a, hipStream_t s) { return launch_conv_wino_b6<14>(a, s); }
}
