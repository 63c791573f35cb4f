// libosgpu: the halo-reuse 3x3 convolution with the weights resident as uint8 CODES (W8A16, round 6): the WQ = 1 instantiations of conv3x3_kernel
// (osg_conv3x3_kernel.h; the list: osg_gemm_routes.h).  The [BN][64] weight tile streams HBM -> L2 -> LDS as codes -- half the bytes of the operand the 8 x 8 / 16 x 16
// levels are bound by -- and becomes halves between LDS and the MFMA (osg_gemm_common.h w8_frag: exact integers q - zp, the scale applied once to the f32
// accumulators).  Tile choice, split-K, fold, statistics sinks, output views: those of the f16 kernel (osg_conv3x3.hip drives both).  Reference: get_tensor_data
// dequantises a uint8 weight when it is loaded, src/onnxstream.cpp:2887-2891 -> Model::dequantize :3353; the convolution itself :1292-1534.
#include "osg_conv3x3_kernel.h"

template <>
int osg_mm::launch3_unit<1>(int entry, osg_ctx* ctx, GemmParams& p) { return launch3_in_unit<1>(entry, ctx, p); }
