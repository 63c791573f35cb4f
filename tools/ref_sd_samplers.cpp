// TEST INFRASTRUCTURE ONLY (fixture generator, tools/make_golden_samplers.py).  Never linked into the product libraries.
//
// The reference's txt2img application (src/sd.cpp + src/samplers.h, #included WHERE THEY LIE, as oracle/ref_sd.cpp does) with the sampler
// chosen BY NAME through the application's own sampler_name[] table (src/sd.cpp:100), i.e. what `--sampler NAME` selects (:2963-2973).
// oracle/ref_sd.cpp only switches between euler_a and euler; this shim lets the fixture tool run the multistep samplers of src/samplers.h
// as compiled reference code.  It is compiled by make_golden_samplers.py with oracle/Makefile's CXXFLAGS and linked against the oracle's
// objects (everything but ref_sd.o, whose symbols it would duplicate).
#define CPUINFO_H
static inline bool cpuinfo_initialize() { return true; }
static inline bool cpuinfo_has_x86_avx2() { return true; }
static inline bool cpuinfo_has_arm_neon_fp16_arith() { return false; }

#define USE_ONNXSTREAM 1
#define main onnxstream_reference_sd_main
#include "sd.cpp"
#undef main

extern "C" {

// diffusion_solver (src/sd.cpp:1574-1780) with the sampler `name`, CFG 7, for `num` images batched like `--num`: final latents [num,4,64,64].
// cond / uncond: [77,768] fp32.  Returns NULL or the error text.
const char* ref_sd_samplers_solve(const char* name, const char* models_path_with_slash, int seed, int steps, int num, unsigned threads, const float* cond,
                                  const float* uncond, float* latents_out) {
    static thread_local std::string err;
    try {
        int k = 0;
        while (k < NUM_OF_SAMPLERS && sampler_name[k] != name) k++;
        if (k == NUM_OF_SAMPLERS) throw std::invalid_argument(std::string("unknown sampler: ") + name);
        g_main_args.m_path_with_slash = models_path_with_slash;
        g_main_args.m_latw = g_main_args.m_lath = 64;
        g_main_args.m_num = std::to_string(num);
        g_main_args.m_sampler = (sampler_type)k;
        n_threads = threads;
        ncnn::Mat c(768, 77, 1, (void*)cond), uc(768, 77, 1, (void*)uncond);
        std::vector<ncnn::Mat> samples;
        {
            SDCoroState coro_state;
            samples = coro_state.run<ncnn::Mat>([&]() { return diffusion_solver(seed + (int)coro_state.batch_index, steps, c, uc, std::string(), nullptr, coro_state); });
        }
        for (size_t i = 0; i < samples.size(); i++) memcpy(latents_out + i * 4 * 64 * 64, (float*)samples[i], 4 * 64 * 64 * sizeof(float));
        return nullptr;
    } catch (const std::exception& e) {
        err = e.what();
        return err.c_str();
    }
}

}  // extern "C"
