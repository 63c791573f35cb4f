// libosgpu: the per-step host arithmetic of the reference's denoising loop, moved next to the UNet so that a whole 20-step image can be
// enqueued without one host round trip:
//   osg_sampler_prepare     <- CFGDenoiser_CompVisDenoiser's input scaling  x * c_in  and the timestep broadcast (reference src/sd.cpp:1427-1470)
//   osg_sampler_cfg_euler_a <- eps -> denoised (x + eps * c_out), the CFG combine (uncond + g * (cond - uncond), src/sd.cpp:1545-1556) and
//                              the Euler-Ancestral update (src/samplers.h:1430-1449: the branch the shipped `#define ORIGINAL_SAMPLER_ALGORITHMS 1`,
//                              samplers.h:66, selects:  x = x + ((x - d) / sigma_i) * (sigma_down - sigma_i) + r * sigma_up)
//   osg_sampler_cfg_multistep   <- the same CFG combine, then one step of DPM++ 2M / 2M v2, iPNDM / iPNDM_v / iPNDM_vo, Taylor3 or DDIM
//                                  (src/samplers.h:339-377, :543-582, :688-940, :942-1034, :1078-1100) with a history ring per prompt
//   osg_sampler_cfg_stochastic  <- the same CFG combine, then one step of DDPM(-a), DDIM-a, TCD(-a), LCM or DPM++ 3M SDE(-a) with the step's noise add
//                                  (src/samplers.h:1039-1076, :1102-1158, :1160-1223, :1406-1428, :412-541)
//   osg_sampler_prepare_rescale <- osg_sampler_prepare after DDIM's in-place prescale of x (prescale_sample, src/samplers.h:27-59)
//   osg_sampler_*_single        <- the same three steps without the guidance pair: CFGDenoiser_CompVisDenoiser returns the cond branch alone in
//                                  Turbo mode (src/sd.cpp:1537-1541), so the pass holds ONE sample per prompt and den = eps[p]*c_out + x
// Every kernel is a template on B, the UNet samples ("branches") per prompt: 2 = the cond / uncond pair with the CFG combine, 1 = single.  The
// update arithmetic after `den` has one body for both.
// fp32 throughout, in the reference's operation order with every multiply and add rounded separately (no fma contraction), so the device
// loop reproduces the host loop bit for bit (tests/test_pipeline.py).
#include "osg_common.h"

// HIP compiles with -ffp-contract=fast (and its __fmul_rn/__fadd_rn are plain operators defined in a header): without the pragma inside
// the kernels a*b+c becomes one fma (one rounding) and the loop drifts from the host arithmetic by an ulp per step.

namespace {

// eps -> denoised for element e of prompt p (i = p * L + e): B == 2 the CFG combine of the pair eps[2p], eps[2p+1] (src/sd.cpp:1545-1556), B == 1 eps[p] alone
template <int B>
__device__ __forceinline__ float sampler_denoised(const float* __restrict__ eps, long p, long L, long e, float xv, float c_out, float guidance) {
#pragma clang fp contract(off)
    static_assert(B == 1 || B == 2, "one sample per prompt, or the cond / uncond pair");
    if constexpr (B == 1) {
        const float pc = eps[p * L + e] * c_out;
        return pc + xv;
    } else {
        const float pc = eps[(2 * p) * L + e] * c_out, pu = eps[(2 * p + 1) * L + e] * c_out;
        const float den_c = pc + xv;
        const float den_u = pu + xv;
        const float gd = guidance * (den_c - den_u);
        return den_u + gd;
    }
}

// the input side of a step.  RESCALE: DDIM's prescale (src/samplers.h:27-59) folded in: x *= x_scale in place first, the UNet input is the rescaled x.
// One body; the two kernels below differ in their argument lists only (the plain one has no x_scale and reads x through a const pointer).
template <int B, bool RESCALE>
__device__ __forceinline__ void sampler_prepare_body(std::conditional_t<RESCALE, float, const float>* __restrict__ x, float* __restrict__ sample,
                                                     float* __restrict__ timestep, int prompts, long L, float x_scale, float c_in, float t,
                                                     long t_per_sample) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)prompts * L;
    if (i < total) {
        const long p = i / L, e = i - p * L;
        float xs = x[i];
        if constexpr (RESCALE) {
            xs = xs * x_scale;
            x[i] = xs;
        }
        const float v = xs * c_in;
        if constexpr (B == 1) {
            sample[i] = v;
        } else {
            sample[(2 * p) * L + e] = v;          // pushes 2p (cond) and 2p+1 (uncond) see the same scaled latent
            sample[(2 * p + 1) * L + e] = v;
        }
    }
    if (i < (long)B * prompts * t_per_sample) timestep[i] = t;
}

template <int B>
__global__ __launch_bounds__(256) void sampler_prepare_kernel(const float* __restrict__ x, float* __restrict__ sample, float* __restrict__ timestep,
                                                              int prompts, long L, float c_in, float t, long t_per_sample) {
    sampler_prepare_body<B, false>(x, sample, timestep, prompts, L, 1.f, c_in, t, t_per_sample);
}

template <int B>
__global__ __launch_bounds__(256) void sampler_prepare_rescale_kernel(float* __restrict__ x, float* __restrict__ sample, float* __restrict__ timestep,
                                                                      int prompts, long L, float x_scale, float c_in, float t, long t_per_sample) {
    sampler_prepare_body<B, true>(x, sample, timestep, prompts, L, x_scale, c_in, t, t_per_sample);
}

template <int B>
__global__ __launch_bounds__(256) void sampler_cfg_euler_a_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                                  int prompts, long L, float c_out, float guidance, float sigma, float d_sigma, float sigma_up, float clip) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)prompts * L) return;
    const long p = i / L, e = i - p * L;
    const float xv = x[i];
    const float den = sampler_denoised<B>(eps, p, L, e, xv, c_out, guidance);
    const float dd = (xv - den) / sigma;          // IEEE division (hipcc keeps fp32 divides correctly rounded), one rounding per operation
    const float st = dd * d_sigma;
    float nx = xv + st;
    if (noise) {
        const float nz = noise[i] * sigma_up;
        nx = nx + nz;
    }
    if (clip > 0.f) nx = fminf(fmaxf(nx, -clip), clip);
    x[i] = nx;
}

// The multistep samplers of src/samplers.h (ORIGINAL_SAMPLER_ALGORITHMS branch): the same den as above, then one of the update forms
// of include/osgpu.h (osg_multistep_form), each its own straight-line instantiation.  h0 receives this step's history entry (the denoised
// latent for DPM++, the derivative d otherwise); h1..h3 are the entries of the previous steps (ring slots chosen by the host, never copied).
// For DPM++ 2M h1 == h0 (one slot, read before it is overwritten), so the history pointers carry no __restrict__.
template <int F, int B>
__global__ __launch_bounds__(256) void sampler_cfg_multistep_kernel(float* __restrict__ x, const float* __restrict__ eps, float* h0, const float* h1,
                                                                    const float* h2, const float* h3, int prompts, long L, float c_out, float guidance,
                                                                    float sigma, float k0, float k1, float k2, float k3, float k4, double da, double db) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)prompts * L) return;
    const long p = i / L, e = i - p * L;
    const float xv = x[i];
    const float den = sampler_denoised<B>(eps, p, L, e, xv, c_out, guidance);
    if constexpr (F == OSG_MS_DDIM) {
        const double ax = (double)xv * da;
        const double bd = (double)den * db;
        x[i] = (float)(ax + bd);
    } else if constexpr (F == OSG_MS_DPMPP_FIRST || F == OSG_MS_DPMPP_2M) {
        float dv = den;
        if constexpr (F == OSG_MS_DPMPP_2M) {
            const float u = k2 * den;
            const float w = k3 * h1[i];
            dv = u - w;
        }
        const float ax = k0 * xv;
        const float bd = k1 * dv;
        h0[i] = den;
        x[i] = ax - bd;
    } else {
        const float d = (xv - den) / sigma;
        float s;
        if constexpr (F == OSG_MS_EULER_D) {
            s = k0 * d;
        } else if constexpr (F == OSG_MS_IPNDM1) {
            const float t = 3.f * d;
            const float u = t - h1[i];
            const float v = k0 * u;
            s = v / 2.f;
        } else if constexpr (F == OSG_MS_IPNDM_V1) {
            const float t = k1 * d;
            const float w = k2 * h1[i];
            const float u = t - w;
            const float v = k0 * u;
            s = v / 2.f;
        } else if constexpr (F == OSG_MS_IPNDM2) {
            const float t = 23.f * d;
            const float w1 = 16.f * h1[i];
            const float w2 = 5.f * h2[i];
            const float u = t - w1;
            const float u2 = u + w2;
            const float v = k0 * u2;
            s = v / 12.f;
        } else if constexpr (F == OSG_MS_IPNDM3) {
            const float t = 55.f * d;
            const float w1 = 59.f * h1[i];
            const float w2 = 37.f * h2[i];
            const float w3 = 9.f * h3[i];
            const float u = t - w1;
            const float u2 = u + w2;
            const float u3 = u2 - w3;
            const float v = k0 * u3;
            s = v / 24.f;
        } else if constexpr (F == OSG_MS_IPNDM_VO1) {
            const float t = k1 * d;
            const float w = k2 * h1[i];
            const float u = t + w;
            s = k0 * u;
        } else if constexpr (F == OSG_MS_IPNDM_VO2) {
            const float t = k1 * d;
            const float w1 = k2 * h1[i];
            const float w2 = k3 * h2[i];
            const float u = t + w1;
            const float u2 = u + w2;
            s = k0 * u2;
        } else if constexpr (F == OSG_MS_IPNDM_VO3) {
            const float t = k1 * d;
            const float w1 = k2 * h1[i];
            const float w2 = k3 * h2[i];
            const float w3 = k4 * h3[i];
            const float u = t + w1;
            const float u2 = u + w2;
            const float u3 = u2 + w3;
            s = k0 * u3;
        } else if constexpr (F == OSG_MS_TAYLOR1) {
            const float dd = d - h1[i];
            const float d2 = dd * k1;
            const float t = k0 * d;
            const float w = k2 * d2;
            s = t + w;
        } else {
            static_assert(F == OSG_MS_TAYLOR2, "unknown multistep form");
            const float dd = d - h1[i];
            const float d2 = dd * k1;
            const float dd3 = d2 - h2[i];
            const float d3 = dd3 * k1;
            const float t = k0 * d;
            const float w2 = k2 * d2;
            const float w3 = k3 * d3;
            const float u = t + w2;
            s = u + w3;
        }
        h0[i] = d;
        x[i] = xv + s;
    }
}

// The one-evaluation samplers of src/samplers.h that add fresh noise per step (DDPM, DDIM-a, TCD, LCM, DPM++ 3M SDE; ORIGINAL_SAMPLER_ALGORITHMS
// branch): the same den, one of the update forms of include/osgpu.h (osg_stochastic_form), each its own straight-line instantiation, then the
// reference's noise add when `noise` is given.  History holds den: the SDE forms write h0 and read h1, h2 (other ring slots, never h0).
template <int F, int B>
__global__ __launch_bounds__(256) void sampler_cfg_stochastic_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                                     float* __restrict__ h0, const float* __restrict__ h1, const float* __restrict__ h2,
                                                                     int prompts, long L, float c_out, float guidance, float sigma, float k0, float k1,
                                                                     float k2, float k3, float k4, float k5, float k6, float n0, float n1) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)prompts * L) return;
    const long p = i / L, e = i - p * L;
    const float xv = x[i];
    const float den = sampler_denoised<B>(eps, p, L, e, xv, c_out, guidance);
    float nx;
    if constexpr (F == OSG_ST_LINEAR) {
        const float ax = xv * k0;
        const float bd = den * k1;
        nx = ax + bd;
    } else if constexpr (F == OSG_ST_DEN) {
        nx = den;
    } else if constexpr (F == OSG_ST_EULER) {
        const float d = (xv - den) / sigma;
        const float s = d * k0;
        nx = xv + s;
    } else if constexpr (F == OSG_ST_DDIM_A) {
        const float az = k0 + xv;
        const float mo = (az - den) / sigma;
        const float xa = xv * k1;
        const float mb = mo * k2;
        const float po = (xa - mb) / k1;
        const float u = k3 * po;
        const float w = mo * k4;
        nx = u + w;
    } else if constexpr (F == OSG_ST_TCD) {
        const float mo = (xv - den) / sigma;
        const float km = k0 * mo;
        const float po = xv - km;
        const float u = k1 * po;
        const float w = k2 * mo;
        nx = u + w;
    } else {
        static_assert(F == OSG_ST_SDE0 || F == OSG_ST_SDE1 || F == OSG_ST_SDE2, "unknown stochastic form");
        h0[i] = den;
        const float ax = k0 * xv;
        const float bd = k1 * den;
        nx = ax - bd;
        if constexpr (F == OSG_ST_SDE1) {
            const float d1 = (den - h1[i]) / k2;
            const float w = k3 * d1;
            nx = nx + w;
        } else if constexpr (F == OSG_ST_SDE2) {
            const float b1 = h1[i];
            const float d10 = (den - b1) / k2;
            const float d11 = (b1 - h2[i]) / k3;
            const float df = d10 - d11;
            const float dr = df * k2;
            const float d1 = d10 + dr / k4;
            const float d2 = df / k4;
            const float u = k5 * d1;
            const float w = k6 * d2;
            nx = nx + (u - w);
        }
    }
    if (noise) {
        if constexpr (F == OSG_ST_TCD) {
            const float a = n1 * nx;
            const float b = n0 * noise[i];
            nx = a + b;
        } else {
            const float nz = noise[i] * n0;
            nx = nx + nz;
        }
    }
    x[i] = nx;
}

// the launches behind the entry points, one per step of the loop, each for both branch counts; `fn` names the entry point in error texts
// x_scale == 1 is the launch without DDIM's prescale: x is not written
template <int B>
int launch_prepare(osg_ctx* ctx, float* x, float* sample, float* timestep, int prompts, long L, float x_scale, float c_in, float t, long t_per_sample,
                   bool rescale) {
    if (prompts <= 0 || L <= 0) return 0;
    const long total = (long)prompts * L;
    const long n = total > (long)B * prompts * t_per_sample ? total : (long)B * prompts * t_per_sample;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (rescale)
        hipLaunchKernelGGL(sampler_prepare_rescale_kernel<B>, grid, block, 0, ctx->compute, x, sample, timestep, prompts, L, x_scale, c_in, t, t_per_sample);
    else
        hipLaunchKernelGGL(sampler_prepare_kernel<B>, grid, block, 0, ctx->compute, (const float*)x, sample, timestep, prompts, L, c_in, t, t_per_sample);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

template <int B>
int launch_euler_a(osg_ctx* ctx, float* x, const float* eps, const float* noise, int prompts, long L, float c_out, float guidance, float sigma,
                   float d_sigma, float sigma_up, float clip) {
    if (prompts <= 0 || L <= 0) return 0;
    const long total = (long)prompts * L;
    hipLaunchKernelGGL(sampler_cfg_euler_a_kernel<B>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->compute, x, eps, noise, prompts, L, c_out,
                       guidance, sigma, d_sigma, sigma_up, clip);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

template <int B>
int launch_multistep(osg_ctx* ctx, const char* fn, int form, float* x, const float* eps, float* h0, const float* h1, const float* h2, const float* h3,
                     int prompts, long L, float c_out, float guidance, float sigma, float k0, float k1, float k2, float k3, float k4, double da,
                     double db) {
    if (form < 0 || form >= OSG_MS_FORMS) OSG_FAIL(ctx, std::string(fn) + ": unknown form " + std::to_string(form));
    const int need = form == OSG_MS_DDIM ? 0 : form == OSG_MS_IPNDM3 || form == OSG_MS_IPNDM_VO3 ? 4
                   : form == OSG_MS_IPNDM2 || form == OSG_MS_IPNDM_VO2 || form == OSG_MS_TAYLOR2 ? 3
                   : form == OSG_MS_DPMPP_FIRST || form == OSG_MS_EULER_D ? 1 : 2;    // history pointers the form touches: h0 .. h(need-1)
    const float* hs[4] = {h0, h1, h2, h3};
    for (int k = 0; k < need; k++)
        if (!hs[k]) OSG_FAIL(ctx, std::string(fn) + ": form " + std::to_string(form) + " needs history pointer h" + std::to_string(k));
    if (prompts <= 0 || L <= 0) return 0;
    const long total = (long)prompts * L;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define OSG_MS_CASE(F)                                                                                                                              \
    case F:                                                                                                                                         \
        hipLaunchKernelGGL((sampler_cfg_multistep_kernel<F, B>), grid, block, 0, ctx->compute, x, eps, h0, h1, h2, h3, prompts, L, c_out, guidance, \
                           sigma, k0, k1, k2, k3, k4, da, db);                                                                                      \
        break;
    switch (form) {
        OSG_MS_CASE(OSG_MS_DPMPP_FIRST) OSG_MS_CASE(OSG_MS_DPMPP_2M) OSG_MS_CASE(OSG_MS_EULER_D) OSG_MS_CASE(OSG_MS_IPNDM1)
        OSG_MS_CASE(OSG_MS_IPNDM_V1) OSG_MS_CASE(OSG_MS_IPNDM2) OSG_MS_CASE(OSG_MS_IPNDM3) OSG_MS_CASE(OSG_MS_IPNDM_VO1)
        OSG_MS_CASE(OSG_MS_IPNDM_VO2) OSG_MS_CASE(OSG_MS_IPNDM_VO3) OSG_MS_CASE(OSG_MS_TAYLOR1) OSG_MS_CASE(OSG_MS_TAYLOR2)
        OSG_MS_CASE(OSG_MS_DDIM)
    }
#undef OSG_MS_CASE
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

template <int B>
int launch_stochastic(osg_ctx* ctx, const char* fn, int form, float* x, const float* eps, const float* noise, float* h0, const float* h1, const float* h2,
                      int prompts, long L, float c_out, float guidance, float sigma, float k0, float k1, float k2, float k3, float k4, float k5, float k6,
                      float n0, float n1) {
    if (form < 0 || form >= OSG_ST_FORMS) OSG_FAIL(ctx, std::string(fn) + ": unknown form " + std::to_string(form));
    const int need = form == OSG_ST_SDE2 ? 3 : form == OSG_ST_SDE1 ? 2 : form == OSG_ST_SDE0 ? 1 : 0;    // history pointers the form touches: h0 .. h(need-1)
    const float* hs[3] = {h0, h1, h2};
    for (int k = 0; k < need; k++)
        if (!hs[k]) OSG_FAIL(ctx, std::string(fn) + ": form " + std::to_string(form) + " needs history pointer h" + std::to_string(k));
    if (prompts <= 0 || L <= 0) return 0;
    const long total = (long)prompts * L;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define OSG_ST_CASE(F)                                                                                                                                  \
    case F:                                                                                                                                             \
        hipLaunchKernelGGL((sampler_cfg_stochastic_kernel<F, B>), grid, block, 0, ctx->compute, x, eps, noise, h0, h1, h2, prompts, L, c_out, guidance, \
                           sigma, k0, k1, k2, k3, k4, k5, k6, n0, n1);                                                                                  \
        break;
    switch (form) {
        OSG_ST_CASE(OSG_ST_LINEAR) OSG_ST_CASE(OSG_ST_DEN) OSG_ST_CASE(OSG_ST_EULER) OSG_ST_CASE(OSG_ST_DDIM_A) OSG_ST_CASE(OSG_ST_TCD)
        OSG_ST_CASE(OSG_ST_SDE0) OSG_ST_CASE(OSG_ST_SDE1) OSG_ST_CASE(OSG_ST_SDE2)
    }
#undef OSG_ST_CASE
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

}  // namespace

extern "C" {

int osg_sampler_prepare(osg_ctx* ctx, const float* x, float* sample, float* timestep, int prompts, long L, float c_in, float t, long t_per_sample) {
    return launch_prepare<2>(ctx, const_cast<float*>(x), sample, timestep, prompts, L, 1.f, c_in, t, t_per_sample, false);
}

int osg_sampler_prepare_rescale(osg_ctx* ctx, float* x, float* sample, float* timestep, int prompts, long L, float x_scale, float c_in, float t,
                                long t_per_sample) {
    return launch_prepare<2>(ctx, x, sample, timestep, prompts, L, x_scale, c_in, t, t_per_sample, true);
}

int osg_sampler_prepare_single(osg_ctx* ctx, float* x, float* sample, float* timestep, int prompts, long L, float x_scale, float c_in, float t,
                               long t_per_sample) {
    return launch_prepare<1>(ctx, x, sample, timestep, prompts, L, x_scale, c_in, t, t_per_sample, x_scale != 1.f);
}

int osg_sampler_cfg_euler_a(osg_ctx* ctx, float* x, const float* eps, const float* noise, int prompts, long L, float c_out, float guidance,
                            float sigma, float d_sigma, float sigma_up, float clip) {
    return launch_euler_a<2>(ctx, x, eps, noise, prompts, L, c_out, guidance, sigma, d_sigma, sigma_up, clip);
}

int osg_sampler_euler_a_single(osg_ctx* ctx, float* x, const float* eps, const float* noise, int prompts, long L, float c_out, float sigma,
                               float d_sigma, float sigma_up, float clip) {
    return launch_euler_a<1>(ctx, x, eps, noise, prompts, L, c_out, 0.f, sigma, d_sigma, sigma_up, clip);
}

int osg_sampler_cfg_multistep(osg_ctx* ctx, int form, float* x, const float* eps, float* h0, const float* h1, const float* h2, const float* h3,
                              int prompts, long L, float c_out, float guidance, float sigma, float k0, float k1, float k2, float k3, float k4,
                              double da, double db) {
    return launch_multistep<2>(ctx, "osg_sampler_cfg_multistep", form, x, eps, h0, h1, h2, h3, prompts, L, c_out, guidance, sigma, k0, k1, k2, k3, k4,
                               da, db);
}

int osg_sampler_multistep_single(osg_ctx* ctx, int form, float* x, const float* eps, float* h0, const float* h1, const float* h2, const float* h3,
                                 int prompts, long L, float c_out, float sigma, float k0, float k1, float k2, float k3, float k4, double da,
                                 double db) {
    return launch_multistep<1>(ctx, "osg_sampler_multistep_single", form, x, eps, h0, h1, h2, h3, prompts, L, c_out, 0.f, sigma, k0, k1, k2, k3, k4,
                               da, db);
}

int osg_sampler_cfg_stochastic(osg_ctx* ctx, int form, float* x, const float* eps, const float* noise, float* h0, const float* h1, const float* h2,
                               int prompts, long L, float c_out, float guidance, float sigma, float k0, float k1, float k2, float k3, float k4, float k5,
                               float k6, float n0, float n1) {
    return launch_stochastic<2>(ctx, "osg_sampler_cfg_stochastic", form, x, eps, noise, h0, h1, h2, prompts, L, c_out, guidance, sigma, k0, k1, k2, k3, k4,
                                k5, k6, n0, n1);
}

int osg_sampler_stochastic_single(osg_ctx* ctx, int form, float* x, const float* eps, const float* noise, float* h0, const float* h1, const float* h2,
                                  int prompts, long L, float c_out, float sigma, float k0, float k1, float k2, float k3, float k4, float k5, float k6,
                                  float n0, float n1) {
    return launch_stochastic<1>(ctx, "osg_sampler_stochastic_single", form, x, eps, noise, h0, h1, h2, prompts, L, c_out, 0.f, sigma, k0, k1, k2, k3, k4,
                                k5, k6, n0, n1);
}

}  // extern "C"
