// libosgpu: what the reference application does on the host around the VAE decoder pass, moved next to it so that latents become an image
// without leaving the device:
//   osg_decode_gather <- slice_and_inf and the latent scaling (reference src/sd.cpp:1261-1279, :2363, :2401-2418; untiled :1193-1194)
//   osg_decode_blend  <- blend, substract_mean_normalize(-1, 127.5) and Mat::to_pixels (src/sd.cpp:1300-1326, :2449-2478, :322-364; untiled :1251-1253)
// fp32 throughout, in the host's operation order with every quotient, product, sum and difference rounded on its own (no fma contraction, see
// osg_sampler.hip), so the device image equals Txt2Img.decode / decode_tiled bit for bit (tests/test_decode_device_gpu.py).
// Both are bandwidth kernels: a thread moves 4 neighbouring pixels of a row -- 16-byte loads and stores of the fp32 planes, one 12-byte store of
// the packed RGB bytes -- wherever the extents and addresses allow it (PX = 4), and single elements otherwise (PX = 1).
#include "osg_common.h"

namespace {

// the tile grid of include/osgpu.h: number of origins along an axis of n latent pixels, and origin k
__host__ __device__ inline int decode_tiles_along(int n, int tile) {
    const int step = tile * 3 / 4;
    return n == tile ? 1 : (n - tile + step - 1) / step + 1;
}
__device__ __forceinline__ int decode_origin(int k, int n, int tile) {
    const int o = k * (tile * 3 / 4);
    return o < n - tile ? o : n - tile;
}

template <int PX>
__global__ __launch_bounds__(256) void decode_gather_kernel(const float* __restrict__ lat, float* __restrict__ tiles, int images, int H, int W, int tile,
                                                            int Ty, int Tx, float factor) {
#pragma clang fp contract(off)
    const int xg = tile / PX;                                            // thread groups per tile row
    const long total = (long)images * Ty * Tx * 4 * tile * xg;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % xg) * PX;
    long r = i / xg;
    const int y = (int)(r % tile);
    r /= tile;
    const int c = (int)(r % 4);
    r /= 4;                                                              // sample p*T + k
    const int kx = (int)(r % Tx);
    r /= Tx;
    const int ky = (int)(r % Ty);
    const long p = r / Ty;
    const int oy = decode_origin(ky, H, tile), ox = decode_origin(kx, W, tile);
    const float* src = lat + ((p * 4 + c) * H + oy + y) * W + ox + x;
    float* dst = tiles + i * PX;
    if constexpr (PX == 4) {
        f32x4 v;
        if (((uintptr_t)src & 15) == 0) v = *(const f32x4*)src;          // (an origin such as 6 of tile 8, or W % 4 != 0: element loads)
        else v = f32x4{src[0], src[1], src[2], src[3]};
        *(f32x4*)dst = f32x4{v[0] * factor, v[1] * factor, v[2] * factor, v[3] * factor};
    } else {
        *dst = *src * factor;
    }
}

struct __attribute__((packed, aligned(4))) rgb4 {                       // 4 packed RGB pixels: three whole 32-bit words, one 12-byte store
    unsigned int w[3];
};

// min(max((int)v, 0), 255) with the clamp done in float first: defined for every v (NaN -> 0 through fmaxf)
__device__ __forceinline__ unsigned int decode_pixel(float v) { return (unsigned int)(int)fminf(fmaxf(v, 0.f), 255.f); }

template <int PX>
__global__ __launch_bounds__(256) void decode_blend_kernel(const float* __restrict__ tiles, float* __restrict__ image, unsigned char* __restrict__ pixels,
                                                           int images, int H, int W, int tile, int up, int Ty, int Tx) {
#pragma clang fp contract(off)
    const int oh = H * up, ow = W * up, ts = tile * up;                   // output rows / columns, tile side in output pixels
    const int xg = ow / PX;
    const long total = (long)images * oh * xg;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int X = (int)(i % xg) * PX;
    const long r = i / xg;
    const int Y = (int)(r % oh);
    const long p = r / oh;
    const int ramp_i = 2 * tile * up / 8;
    const float ramp = (float)ramp_i;
    float d[3][PX];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < PX; j++) d[c][j] = 0.f;
    // every tile that covers the pixels, in raster order (more than two per axis where the last origin is pulled back to the border).  With PX = 4
    // up % 4 == 0, so the tile borders are multiples of 4 and the four pixels of a thread lie in the same tiles.
    for (int ky = 0; ky < Ty; ky++) {
        const int ly = Y - decode_origin(ky, H, tile) * up;
        if (ly < 0 || ly >= ts) continue;
        // (origin != 0 <=> k != 0: the step 3 * tile / 4 is >= 1, since decode_check refuses a tile below 2 over larger latents)
        const float qy = (ky != 0 && ly < ramp_i) ? (float)ly / ramp : 1.f;
        for (int kx = 0; kx < Tx; kx++) {
            const int lx = X - decode_origin(kx, W, tile) * up;
            if (lx < 0 || lx >= ts) continue;
            float f[PX], g[PX];
#pragma unroll
            for (int j = 0; j < PX; j++) {
                const float qx = (kx != 0 && lx + j < ramp_i) ? (float)(lx + j) / ramp : 1.f;
                f[j] = qy * qx;
                g[j] = 1.f - f[j];
            }
            const float* src = tiles + (((p * Ty + ky) * Tx + kx) * 3 * ts + ly) * (long)ts + lx;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float s[PX];
                if constexpr (PX == 4) {
                    const f32x4 v = *(const f32x4*)(src + (long)c * ts * ts);
                    s[0] = v[0]; s[1] = v[1]; s[2] = v[2]; s[3] = v[3];
                } else {
                    s[0] = src[(long)c * ts * ts];
                }
#pragma unroll
                for (int j = 0; j < PX; j++) {
                    const float a = s[j] * f[j];
                    const float b = d[c][j] * g[j];
                    d[c][j] = a + b;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const float a = d[c][j] + 1.f;
            d[c][j] = a * 127.5f;
        }
    if (image) {
        float* dst = image + ((p * 3) * oh + Y) * (long)ow + X;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if constexpr (PX == 4) *(f32x4*)(dst + (long)c * oh * ow) = f32x4{d[c][0], d[c][1], d[c][2], d[c][3]};
            else dst[(long)c * oh * ow] = d[c][0];
        }
    }
    if (pixels) {
        unsigned char* dst = pixels + ((p * oh + Y) * (long)ow + X) * 3;
        if constexpr (PX == 4) {
            unsigned int b[12];
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int c = 0; c < 3; c++) b[j * 3 + c] = decode_pixel(d[c][j]);
            rgb4 o;
#pragma unroll
            for (int w = 0; w < 3; w++) o.w[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
            *(rgb4*)dst = o;
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) dst[c] = (unsigned char)decode_pixel(d[c][0]);
        }
    }
}

// the checks the two entry points share; 0 = fine
int decode_check(osg_ctx* ctx, const char* who, int images, int H, int W, int tile, int up) {
    if (images < 0 || tile < 1 || up < 1 || H < tile || W < tile)
        OSG_FAIL(ctx, std::string(who) + ": needs images >= 0, up >= 1 and H, W >= tile >= 1.");
    if (tile < 2 && (H != tile || W != tile)) OSG_FAIL(ctx, std::string(who) + ": a tile of 1 has no step; it only serves H == W == 1.");
    if ((long)H * up > (1 << 24) || (long)W * up > (1 << 24)) OSG_FAIL(ctx, std::string(who) + ": an image side above 2^24 pixels is not exact in fp32.");
    return 0;
}

}  // namespace

extern "C" {

int osg_decode_gather(osg_ctx* ctx, const float* latents, float* tiles, int images, int H, int W, int tile, float factor) {
    if (decode_check(ctx, "osg_decode_gather", images, H, W, tile, 1)) return 1;
    if (images == 0) return 0;
    const int Ty = decode_tiles_along(H, tile), Tx = decode_tiles_along(W, tile);
    const long elems = (long)images * Ty * Tx * 4 * tile * tile;
    const bool wide = tile % 4 == 0 && ((uintptr_t)tiles & 15) == 0;
    const long threads = wide ? elems / 4 : elems;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    if (wide) hipLaunchKernelGGL(decode_gather_kernel<4>, grid, block, 0, ctx->compute, latents, tiles, images, H, W, tile, Ty, Tx, factor);
    else hipLaunchKernelGGL(decode_gather_kernel<1>, grid, block, 0, ctx->compute, latents, tiles, images, H, W, tile, Ty, Tx, factor);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_decode_blend(osg_ctx* ctx, const float* tiles, float* image, unsigned char* pixels, int images, int H, int W, int tile, int up) {
    if (decode_check(ctx, "osg_decode_blend", images, H, W, tile, up)) return 1;
    if (images == 0 || (!image && !pixels)) return 0;
    const int Ty = decode_tiles_along(H, tile), Tx = decode_tiles_along(W, tile);
    const long px = (long)images * H * up * W * up;
    // four pixels per thread: tile borders and row starts on multiples of 4 pixels, every base address on the width of its access
    const bool wide = up % 4 == 0 && ((uintptr_t)tiles & 15) == 0 && ((uintptr_t)image & 15) == 0 && ((uintptr_t)pixels & 3) == 0;
    const long threads = wide ? px / 4 : px;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    if (wide) hipLaunchKernelGGL(decode_blend_kernel<4>, grid, block, 0, ctx->compute, tiles, image, pixels, images, H, W, tile, up, Ty, Tx);
    else hipLaunchKernelGGL(decode_blend_kernel<1>, grid, block, 0, ctx->compute, tiles, image, pixels, images, H, W, tile, up, Ty, Tx);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

}  // extern "C"
