// TEST INFRASTRUCTURE ONLY (fixture generator, tools/make_golden_sdxl_loop.py).  Never linked into the product libraries.
//
// The reference's txt2img application (src/sd.cpp + src/samplers.h, #included WHERE THEY LIE, as oracle/ref_sd.cpp and tools/ref_sd_samplers.cpp do)
// driven through its SDXL branch: the application's own mode switches (`--xl`, `--turbo`), latent size (`--res`) and sampler (`--sampler NAME`, chosen
// through its sampler_name[] table) are set, an SDXLParams is filled from the caller's arrays, and diffusion_solver runs.  Nothing of the reference is
// restated here.  Compiled by make_golden_sdxl_loop.py with oracle/Makefile's CXXFLAGS and linked against the oracle's objects (everything but
// ref_sd.o, whose symbols it would duplicate).
#define CPUINFO_H
static inline bool cpuinfo_initialize() { return true; }
static inline bool cpuinfo_has_x86_avx2() { return true; }
static inline bool cpuinfo_has_arm_neon_fp16_arith() { return false; }

#define USE_ONNXSTREAM 1
#define main onnxstream_reference_sd_main
#include "sd.cpp"
#undef main

extern "C" {

// diffusion_solver with the sampler `name` for one image: final latents [1,4,lath,latw].
//   pooled != NULL: the SDXL branch.  embeds / embeds_neg: [77,2048], pooled / pooled_neg: [1280] fp32; xl, turbo: the application's mode switches.  The
//                   UNet is read from <models>/sdxl_unet_fp16/ or, in Turbo mode, <models>/sdxl_unet_anyshape_fp16/.
//   pooled == NULL: the SD 1.5 branch (what tools/ref_sd_samplers.cpp runs): embeds / embeds_neg are the contexts [77,768], the latent is 64 x 64.
// Returns NULL or the error text.
const char* ref_sdxl_solve(const char* name, const char* models_path_with_slash, int xl, int turbo, int seed, int steps, unsigned latw, unsigned lath,
                           unsigned threads, const float* embeds, const float* embeds_neg, const float* pooled, const float* pooled_neg,
                           float* latents_out) {
    static thread_local std::string err;
    try {
        int k = 0;
        while (k < NUM_OF_SAMPLERS && sampler_name[k] != name) k++;
        if (k == NUM_OF_SAMPLERS) throw std::invalid_argument(std::string("unknown sampler: ") + name);
        g_main_args.m_path_with_slash = models_path_with_slash;
        g_main_args.m_xl = xl != 0;
        g_main_args.m_turbo = turbo != 0;
        g_main_args.m_latw = latw;
        g_main_args.m_lath = lath;
        g_main_args.m_num = "1";
        g_main_args.m_sampler = (sampler_type)k;
        n_threads = threads;
        std::vector<ncnn::Mat> samples;
        if (pooled) {
            SDXLParams params;
            params.m_prompt_embeds.assign(embeds, embeds + 77 * 2048);
            params.m_prompt_embeds_neg.assign(embeds_neg, embeds_neg + 77 * 2048);
            params.m_pooled_prompt_embeds.assign(pooled, pooled + 1280);
            params.m_pooled_prompt_embeds_neg.assign(pooled_neg, pooled_neg + 1280);
            SDCoroState coro_state;
            samples = coro_state.run<ncnn::Mat>([&]() { return diffusion_solver(seed, steps, ncnn::Mat(), ncnn::Mat(), std::string(), &params, coro_state); });
        } else {
            ncnn::Mat c(768, 77, 1, (void*)embeds), uc(768, 77, 1, (void*)embeds_neg);
            SDCoroState coro_state;
            samples = coro_state.run<ncnn::Mat>([&]() { return diffusion_solver(seed, steps, c, uc, std::string(), nullptr, coro_state); });
        }
        memcpy(latents_out, (float*)samples[0], (size_t)4 * lath * latw * sizeof(float));
        return nullptr;
    } catch (const std::exception& e) {
        err = e.what();
        return err.c_str();
    }
}

// the noise the application draws for a latent of this size: randn_4_w_h(seed, w, h) -> [4,h,w]
void ref_sdxl_randn(int seed, int w, int h, float* out) {
    ncnn::Mat m = randn_4_w_h(seed, w, h);
    memcpy(out, (float*)m, (size_t)4 * w * h * sizeof(float));
}

// the rand() stream process_sample consumes for the ancestral noise: srand(seed of the step), rand() % 1000
int ref_sdxl_step_noise_seed(int seed_at_step) {
    std::srand(seed_at_step);
    return rand() % 1000;
}

}  // extern "C"
