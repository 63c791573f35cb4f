// libosgpu: W8A16 contractions with the weight CODES resident (round 6 rewrite): the WQ = 1 instantiations of the direct-to-LDS contraction kernel (gemm2_kernel,
// osg_gemm2.h; the list: osg_gemm_routes.h) for Linear / MatMul / Gemm and the 1 x 1 convolutions; the implicit-GEMM convolutions are in osg_gemm_w8_conv.hip, the
// halo-reuse 3 x 3 convolution in osg_conv3x3_w8.hip.
//
// Reference semantics (src/onnxstream.cpp:2887-2891 -> Model::dequantize :3353): a uint8 weight with (scale, zero_point) becomes w = f16((float)((int)q - zp) * scale)
// when it is LOADED and the f16 GEMM / convolution then runs as usual.  Here the codes stay uint8 in HBM (half the footprint), stream through L2 and the LDS ring as
// codes (half the bytes of the weight operand on every hop -- the operand the 8 x 8 / 16 x 16 levels of the UNet are bound by, and half the bytes through the LDS
// port the k loop is bound by), and become halves between the LDS tile and the MFMA: the integer q - zp exactly (osg_gemm_common.h w8_frag), the scale applied once to
// the f32 accumulators.  Tiles, rings, split-K, the in-kernel fold, GEGLU, output views, statistics sinks: those of the f16 kernel -- osg_gemm.hip drives both,
// W8 shapes have rows of their own in the tune table (flag 1024 of the key).  Rounds 3-5 had a lean 512-thread kernel here that dequantised in its loader waves
// (register staging, ds_write): 1.6 x the f16 plan on the SD 1.5 pass.
#include "osg_gemm2.h"

template <>
int osg_mm::launch_v2_unit<2>(int entry, osg_ctx* ctx, GemmParams& p, int batch) { return launch_v2_in_unit<2>(entry, ctx, p, batch); }
