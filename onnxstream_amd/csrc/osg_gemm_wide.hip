// libosgpu: the 160- and 80-column tiles of the direct-to-LDS contraction kernel (round 6; kernel and launcher: osg_gemm2.h, instantiations and choice:
// osg_gemm_routes.h, osg_gemm.hip).
//
// Why: every output width of the SD / SDXL UNets is a multiple of 320 (320 ... 10 240, 960 / 1 920 / 3 840 for the merged Q|K|V projections), none but 640 x 2^n
// a multiple of 128 -- and a batch-2 layer is about ONE tile per CU, so how the tile grid divides the 256 CUs decides a launch more than the k loop does:
// the GEGLU projection of the 16 x 16 level (512 x 10 240 x 1 280) is 4 x 80 = 320 tiles of 128 x 128 (two rounds on 64 CUs, one on the rest) but 4 x 64 = 256
// tiles of 128 x 160; the one of the 32 x 32 level (2 048 x 5 120 x 640) is 1 280 tiles of 128 x 64 on 768 resident slots but 512 of 128 x 160 on 512; a
// 2 048 x 640 output is 320 tiles of 64 x 64 but 256 of 64 x 80.  The wider tile also fetches fewer bytes per MFMA (128 x 160: 71 FLOP per byte, 128 x 64: 43).
//   tile 4: 128 x 160, waves 4 x 1 (32 rows x 160 columns each: 10 column blocks, even -- the GEGLU pairing works)
//   tile 5: 128 x  80, waves 4 x 1 (the halo convolution's wave tile, 32 x 80)
//   tile 6:  64 x  80, waves 4 x 1 (16 x 80)
//   tile 7:  64 x 160, waves 2 x 2 (32 x 80)
// Measured candidates only (osg_tune.h): the cost-model plans of the parity tests never take them.  Arithmetic: the same MFMA sequence per output element as every
// other tile (k ascending in steps of 32, f32 accumulate, one rounding) -- a tile choice changes no bits unless it changes the split of K.
#include "osg_gemm2.h"

template <>
int osg_mm::launch_v2_unit<1>(int entry, osg_ctx* ctx, GemmParams& p, int batch) { return launch_v2_in_unit<1>(entry, ctx, p, batch); }
