// libosgpu: the implicit-GEMM convolutions with the weight codes resident (W8A16; see osg_gemm_w8.hip): WQ = 1, CONV instantiations of gemm2_kernel -- the
// stride-2 downsampling convolutions and every 3 x 3 shape the halo-reuse kernel does not take.
#include "osg_gemm2.h"

template <>
int osg_mm::launch_v2_unit<3>(int entry, osg_ctx* ctx, GemmParams& p, int batch) { return launch_v2_in_unit<3>(entry, ctx, p, batch); }
