// instantiation list of conv_mfma_kernel (see conv_launch.h): the sizes only the general alpha-beta rule needs
#include "conv_launch.h"
namespace lrpx {
int launch_conv_224_8_1_4_9_plain(const ConvArgs& a, hipStream_t s) { return launch_conv_cfg<224, 8, 1, 4, 9, EPI_PLAIN>(a, s); }
}
