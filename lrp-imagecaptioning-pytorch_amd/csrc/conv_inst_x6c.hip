// instantiations of the fp32-accurate bf16x6 convolution (conv_bf16x6.h): 224-pixel relevance pass
#include "conv_launch.h"
#include "conv_bf16x6.h"
namespace lrpx {
int launch_x6_224_rel(const ConvArgs& a, hipStream_t s) { return launch_conv_bf16x6<224, 4, 2, false, EPI_REL>(a, s); }
}
