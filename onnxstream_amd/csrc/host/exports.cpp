// exports.cpp -- the flat C API over Model that foreign-language bindings use.  Names, argument order, ownership and
// error conventions are those of the reference's src/exports.cpp (model_new :42, model_new_2 :62, model_delete :87,
// model_read_string :92, model_read_file :98, model_get_weights_names :111, model_add_weights_file :150,
// model_add_tensor :169, model_get_tensor :205, model_get_all_tensor_names :235, model_run :245, model_run_2 :258,
// model_clear_tensors :271, model_set_option :276, model_add_extra_output :303, model_free_buffer :308): errors come back
// as malloc'd C strings the caller releases with model_free_buffer.  Extra entry points for this backend carry a
// `model_hip_` prefix.
#include <cstdio>
#include <cstring>

#include "onnxstream.h"
#include "plan.h"

using namespace onnxstream;

namespace {

char* dup_cstr(const std::string& s) {
    char* p = (char*)std::malloc(s.size() + 1);
    std::memcpy(p, s.c_str(), s.size() + 1);
    return p;
}

struct Handle {
    explicit Handle(int threads) : model(threads) {}
    Model model;
    std::string definition;
    std::string provider;
};

const char* dtype_name(TensorDataType t) {
    switch (t) {
        case TensorDataType::uint8: return "uint8";
        case TensorDataType::float16: return "float16";
        case TensorDataType::float32: return "float32";
        case TensorDataType::int64: return "int64";
        default: throw std::invalid_argument("Unsupported tensor data format.");
    }
}

// the error convention of the char*-returning exports: run `f`; NULL on success, the exception's text (malloc'd) otherwise.  With `ms`, f returns the
// device time that *ms (may be NULL) receives.
template <class F>
char* guarded(F&& f) {
    try {
        f();
        return nullptr;
    } catch (const std::exception& e) {
        return dup_cstr(e.what());
    }
}
template <class F>
char* guarded(double* ms, F&& f) {
    return guarded([&] {
        const double v = f();
        if (ms) *ms = v;
    });
}

// the three sampler loops on the Model's plan; each pair of exports (model_hip_sampler_loop*, *_single) differs in `branches` and `guidance` alone
char* euler_a_loop(Handle* h, int branches, float guidance, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, float* x,
                   const float* noise, const float* c_in, const float* c_out, const float* t, const float* sigma, const float* d_sigma, const float* sigma_up,
                   const float* clip, double* ms) {
    return guarded(ms, [&] {
        return Plan::on_plan_of(h->model, branches == 2 ? "Model::hip_sampler_loop" : "Model::hip_sampler_loop_single", [&](Plan& p) {
            return p.sampler_loop(sample_name, timestep_name, out_name, steps, prompts, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, guidance, clip, branches);
        });
    });
}
char* multistep_loop(Handle* h, int branches, float guidance, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, int sampler,
                     float* x, const float* c_in, const float* c_out, const float* t, const float* sigma, const int* order, const float* coef,
                     unsigned long long n_coef, const double* dcoef, unsigned long long n_dcoef, double* ms) {
    return guarded(ms, [&] {
        return Plan::on_plan_of(h->model, branches == 2 ? "Model::hip_sampler_loop_multistep" : "Model::hip_sampler_loop_multistep_single", [&](Plan& p) {
            return p.sampler_loop_multistep(sample_name, timestep_name, out_name, steps, prompts, sampler, x, c_in, c_out, t, sigma, order, coef, (size_t)n_coef,
                                            dcoef, (size_t)n_dcoef, guidance, branches);
        });
    });
}
char* stochastic_loop(Handle* h, int branches, float guidance, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, float* x,
                      const float* c_in, const float* c_out, const float* t, const float* sigma, const int* form, const int* draws, const float* coef,
                      unsigned long long n_coef, const float* noise, double* ms) {
    return guarded(ms, [&] {
        return Plan::on_plan_of(h->model, branches == 2 ? "Model::hip_sampler_loop_stochastic" : "Model::hip_sampler_loop_stochastic_single", [&](Plan& p) {
            return p.sampler_loop_stochastic(sample_name, timestep_name, out_name, steps, prompts, x, c_in, c_out, t, sigma, form, draws, coef, (size_t)n_coef,
                                             noise, guidance, branches);
        });
    });
}

}  // namespace

extern "C" {

Handle* model_new_2(int threads_count, char* wp_name) {
    Handle* h = new Handle(threads_count);
    h->provider = wp_name;
    const std::string& w = h->provider;
    if (w == "ram") h->model.set_weights_provider(RamWeightsProvider<WeightsProvider>());
    else if (w == "nocache") h->model.set_weights_provider(DiskNoCacheWeightsProvider());
    else if (w == "prefetch") h->model.set_weights_provider(DiskPrefetchWeightsProvider());
    else if (w == "ram+nocache") h->model.set_weights_provider(RamWeightsProvider<DiskNoCacheWeightsProvider>(DiskNoCacheWeightsProvider()));
    else if (w == "ram+prefetch") h->model.set_weights_provider(RamWeightsProvider<DiskPrefetchWeightsProvider>(DiskPrefetchWeightsProvider()));
    else {
        delete h;
        return nullptr;
    }
    return h;
}

Handle* model_new() {
    static char ram[] = "ram";
    return model_new_2(0, ram);
}

void model_delete(Handle* h) { delete h; }

void model_read_string(Handle* h, char* str) {
    h->definition = str;
    h->model.read_string(str);
}

char* model_read_file(Handle* h, char* fn) {
    return guarded([&] { h->model.read_file(fn); });
}

char* model_get_weights_names(Handle* h) {
    Model probe(-1);
    probe.m_support_dynamic_shapes = true;
    probe.set_weights_provider(CollectNamesWeightsProvider(true));
    probe.read_string(h->definition.c_str());
    probe.init();
    std::string out;
    for (auto& e : probe.get_weights_provider<CollectNamesWeightsProvider>().m_names_vec) {
        std::string fn = e.m_name;
        auto pos = fn.find("_nchw.bin");
        if (pos != std::string::npos) fn = fn.substr(0, pos) + "_nhwc.bin";
        if (!out.empty()) out += "|";
        out += std::string(dtype_name(e.m_type)) + ":" + fn;
    }
    return dup_cstr(out);
}

// 64-bit size variant (bindings that pass size_t need not truncate: a buffer of 4 GiB or more handed to the 32-bit entry point would
// be allocated short and overrun by the caller); the reference's 32-bit entry point (src/exports.cpp:139) forwards to it
void* model_hip_add_weights_file(Handle* h, const char* type, const char* name, unsigned long long size) {
    if (h->provider != "ram") return nullptr;
    auto& wp = h->model.get_weights_provider<RamWeightsProvider<WeightsProvider>>();
    const std::string t = type;
    if (t == "uint8") return wp.add_empty_and_return_ptr<uint8_t>(name, (size_t)size / sizeof(uint8_t));
    if (t == "float16") return wp.add_empty_and_return_ptr<uint16_t>(name, (size_t)size / sizeof(uint16_t));
    if (t == "float32") return wp.add_empty_and_return_ptr<float>(name, (size_t)size / sizeof(float));
    if (t == "int64") return wp.add_empty_and_return_ptr<int64_t>(name, (size_t)size / sizeof(int64_t));
    throw std::invalid_argument("Unsupported tensor data format.");
}

void* model_add_weights_file(Handle* h, char* type, char* name, unsigned int size) {
    return model_hip_add_weights_file(h, type, name, (unsigned long long)size);
}

void* model_add_tensor(Handle* h, char* type, char* name, unsigned int dims_num, unsigned int* dims) {
    Tensor t;
    t.m_name = name;
    size_t n = 1;
    for (unsigned i = 0; i < dims_num; i++) {
        t.m_shape.push_back(dims[i]);
        n *= dims[i];
    }
    const std::string ty = type;
    void* ptr = nullptr;
    if (ty == "float32") {
        tensor_vector<float> v(n);
        ptr = v.data();  // the heap block moves with the vector into the tensor
        t.set_vector(std::move(v));
    } else if (ty == "int64") {
        tensor_vector<int64_t> v(n);
        ptr = v.data();
        t.set_vector(std::move(v));
    } else {
        throw std::invalid_argument("Unsupported tensor data format.");
    }
    h->model.push_tensor(std::move(t));
    return ptr;
}

void* model_get_tensor(Handle* h, char* name) {
    struct Ret {
        size_t dims_num;
        size_t* dims;
        size_t data_num;
        float* data;
    };
    for (auto& t : h->model.m_data)
        if (t.m_name == name) {
            if (t.m_type != TensorDataType::float32) return nullptr;
            Ret* r = (Ret*)std::malloc(sizeof(Ret));
            r->dims_num = t.m_shape.size();
            r->dims = t.m_shape.data();
            r->data_num = t.get_vector<float>().size();
            r->data = t.get_vector<float>().data();
            return r;
        }
    return nullptr;
}

// sample `index` of a tensor that was produced for several pushed samples (index 0 == model_get_tensor); the reference app reaches
// the same data through Tensor::m_batch (src/sd.cpp:1098-1161 SDCoroState::get_result)
void* model_hip_get_tensor_batch(Handle* h, char* name, unsigned int index) {
    struct Ret {
        size_t dims_num;
        size_t* dims;
        size_t data_num;
        float* data;
    };
    for (auto& t : h->model.m_data)
        if (t.m_name == name) {
            Tensor* src = &t;
            if (index > 0) {
                if (!t.m_batch || index - 1 >= t.m_batch->size()) return nullptr;
                src = &(*t.m_batch)[index - 1];
            }
            if (src->m_type != TensorDataType::float32) return nullptr;
            Ret* r = (Ret*)std::malloc(sizeof(Ret));
            r->dims_num = src->m_shape.size();
            r->dims = src->m_shape.data();
            r->data_num = src->get_vector<float>().size();
            r->data = src->get_vector<float>().data();
            return r;
        }
    return nullptr;
}

char* model_get_all_tensor_names(Handle* h) {
    std::string out;
    for (auto& t : h->model.m_data) out += (out.empty() ? "" : "|") + t.m_name;
    return dup_cstr(out);
}

void model_run(Handle* h) {
    try {
        h->model.run();
    } catch (const std::exception& e) {
        printf("=== ERROR === %s\n", e.what());
        throw;
    }
}

char* model_run_2(Handle* h) {
    return guarded([&] { h->model.run(); });
}

void model_clear_tensors(Handle* h) { h->model.m_data.clear(); }

void model_set_option(Handle* h, char* name, unsigned int value) {
    Model& m = h->model;
    const std::string n = name;
    const bool b = value != 0;
    if (n == "use_fp16_arithmetic") m.m_use_fp16_arithmetic = b;
    else if (n == "use_uint8_qdq") m.m_use_uint8_qdq = b;
    else if (n == "use_uint8_arithmetic") m.m_use_uint8_arithmetic = b;
    else if (n == "fuse_ops_in_attention") m.m_fuse_ops_in_attention = b;
    else if (n == "force_fp16_storage") m.m_force_fp16_storage = b;
    else if (n == "support_dynamic_shapes") m.m_support_dynamic_shapes = b;
    else if (n == "use_ops_cache") m.m_use_ops_cache = b;
    else if (n == "use_scaled_dp_attn_op") m.m_use_scaled_dp_attn_op = b;
    else if (n == "use_next_op_cache") m.m_use_next_op_cache = b;
    else if (n == "ops_printf") m.m_ops_printf = b;
    else if (n == "ops_times_printf") m.m_ops_times_printf = b;
    else if (n == "use_nchw_convs") m.m_use_nchw_convs = b;
    else if (n == "range_data_calibrate") m.m_range_data_calibrate = b;
    // ---- backend additions ----
    else if (n == "attention_fused_ops_parts") m.m_attention_fused_ops_parts = value;
    else if (n == "hip_device") m.m_hip_device = (int)value;
    else if (n == "hip_fusion_level") m.m_hip_fusion_level = (int)value;
    else if (n == "hip_use_graph") m.m_hip_use_graph = b;
    else if (n == "hip_autotune") m.m_hip_autotune = b;
    else if (n == "hip_fuse_ln_gemm") m.m_hip_fuse_ln_gemm = b;
    else if (n == "hip_concat_views") m.m_hip_concat_views = b;
    else if (n == "hip_fuse_tblock") m.m_hip_fuse_tblock = b;
    else if (n == "hip_fuse_shortcut") Plan::plan_options(m).fuse_shortcut = b;
    else if (n == "hip_gn_stats") m.m_hip_gn_stats = (int)value;
    else if (n == "hip_loop_hoist") Plan::loop_options(m).hoist = b;
    else if (n == "hip_loop_hoist_rows") Plan::loop_options(m).rows = (int)value;
    else if (n == "hip_stream_weights") m.m_hip_stream_weights = b;
    else if (n == "hip_w8_resident") m.m_hip_w8_resident = b;
    else if (n == "hip_resident_outputs") m.m_hip_resident_outputs = b;
    else {
        const char* err = "model_set_option: 'name' not found.";
        printf("=== ERROR === %s\n", err);
        throw std::invalid_argument(err);
    }
}

void model_add_extra_output(Handle* h, char* name) { h->model.m_extra_outputs.emplace_back(name); }

void model_free_buffer(void* ptr) { std::free(ptr); }

// ---- backend additions -------------------------------------------------------------------------------------------
double model_hip_last_pass_ms(Handle* h) { return h->model.hip_last_pass_ms(); }
unsigned long long model_hip_last_kernel_count(Handle* h) { return h->model.hip_last_kernel_count(); }
void model_hip_invalidate_plan(Handle* h) { h->model.hip_invalidate_plan(); }
unsigned long long model_hip_plans_built(Handle* h) { return h->model.hip_plans_built(); }
// bytes the last pass pulled through the WeightsProvider and streamed host->device (0 in resident mode)
unsigned long long model_hip_streamed_bytes(Handle* h) { return h->model.hip_streamed_bytes(); }
unsigned long long model_hip_resident_weight_bytes(Handle* h) { return h->model.hip_resident_weight_bytes(); }
// CudaOptions::m_vram_to_use through the C API (the reference sets it from C++ only: src/llm.cpp set_cuda_options)
void model_hip_set_vram_budget(Handle* h, unsigned long long bytes) { h->model.set_cuda_options(CudaOptions(bytes, false)); }
// Model::m_requires_upcast is a std::function (set from C++ by src/llm.cpp:379-383: ops whose NAME contains "/input_layernorm/" or
// "/post_attention_layernorm/" run in fp32): through the C API as a '|'-separated list of substrings of the op name; "" clears it
void model_hip_set_upcast_substrings(Handle* h, const char* list) {
    std::vector<std::string> subs;
    std::string cur;
    for (const char* p = list ? list : ""; ; p++) {
        if (*p == '|' || *p == 0) {
            if (!cur.empty()) subs.push_back(cur);
            cur.clear();
            if (!*p) break;
        } else cur.push_back(*p);
    }
    if (subs.empty()) h->model.m_requires_upcast = nullptr;
    else
        h->model.m_requires_upcast = [subs](const std::string&, const std::string& name) {
            for (auto& s : subs)
                if (name.find(s) != std::string::npos) return true;
            return false;
        };
    h->model.hip_invalidate_plan();
}
// What src/llm.cpp does to Model::m_data and m_outputs_convert_set from C++ between two calls (:366, :403-407): keep an output out of the
// fp32 conversion, and hand an output of the last run back as an input of the next one under another name
void model_hip_add_outputs_convert(Handle* h, char* name) { h->model.m_outputs_convert_set.insert(name); }
int model_hip_drop_tensor(Handle* h, char* name) {   // (llm.cpp's get_output moves a result out of m_data, :342-353)
    auto& d = h->model.m_data;
    for (size_t i = 0; i < d.size(); i++)
        if (d[i].m_name == name) { d.erase(d.begin() + i); return 1; }
    return 0;
}
// bring a device-resident tensor (hip_resident_outputs) to the host; returns an error string or NULL
char* model_hip_fetch_tensor(Handle* h, char* name) {
    return guarded([&] { h->model.hip_fetch_tensor(name); });
}
// the bits of a float16 tensor of m_data (an output kept out of m_outputs_convert_set: the LLM flow's caches), which model_get_tensor cannot hand out.
// shape: [8] (receives the dims), *rank their number; dst (may be NULL: shape only) receives dst_elems halves, which must be the tensor's element count.
// A device-resident tensor is read where it lies and stays there.
char* model_hip_get_tensor_f16(Handle* h, char* name, unsigned short* dst, unsigned long long dst_elems, unsigned long long* shape, int* rank) {
    return guarded([&] {
        for (auto& t : h->model.m_data)
            if (t.m_name == name) {
                if (t.m_type != TensorDataType::float16) throw std::invalid_argument("Model::hip_get_tensor_f16: tensor is not float16: " + std::string(name));
                if (t.m_shape.size() > 8) throw std::invalid_argument("Model::hip_get_tensor_f16: rank > 8.");
                size_t n = 1;
                for (size_t k = 0; k < t.m_shape.size(); k++) { shape[k] = t.m_shape[k]; n *= t.m_shape[k]; }
                *rank = (int)t.m_shape.size();
                if (!dst) return;
                if (dst_elems != n) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
                if (t.m_hip_resident) {
                    if (t.m_hip_resident_bytes != n * 2) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
                    Plan::read_resident(h->model, t, dst);
                } else {
                    if (t.get_vector<uint16_t>().size() != n) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
                    std::memcpy(dst, t.get_vector<uint16_t>().data(), n * 2);
                }
                return;
            }
        throw std::invalid_argument("Model::hip_get_tensor_f16: tensor not found: " + std::string(name));
    });
}
int model_hip_rename_tensor(Handle* h, char* from, char* to) {
    for (auto& t : h->model.m_data)
        if (t.m_name == from) { t.m_name = to; return 1; }
    return 0;
}
// relaunch the captured pass n times on the resident inputs; ms_each (may be NULL) receives per-launch device times
char* model_hip_replay(Handle* h, int n, float* ms_each) {
    return guarded([&] { h->model.hip_replay(n, ms_each); });
}
// refresh sample `index` of a resident graph input (fp32, `count` elements) without running a pass
char* model_hip_set_input(Handle* h, char* name, long long index, const float* data, unsigned long long count) {
    return guarded([&] { h->model.hip_set_input(name, (long)index, data, (size_t)count); });
}
// the timestep values (n floats) of the schedule the following sampler-loop calls walk: the first of them computes their timestep-only launches ahead of step 0
char* model_hip_sampler_schedule(Handle* h, const float* t, unsigned long long n) { return guarded([&] { Plan::sampler_schedule(h->model, t, (size_t)n); }); }
// the loop hoist of the current plan: out[8], see Plan::loop_hoist_stats; the text of Plan::hoist_info (malloc'ed, free with model_free_buffer; "ERROR: ..." on error)
void model_hip_loop_hoist_stats(Handle* h, unsigned long long* out) { Plan::loop_hoist_stats(h->model, out); }
char* model_hip_loop_hoist_info(Handle* h) {
    try {
        return dup_cstr(Plan::loop_hoist_info(h->model));
    } catch (const std::exception& e) {
        return dup_cstr(std::string("ERROR: ") + e.what());
    }
}
// the reference app's denoising loop (CFG combine + Euler-Ancestral, src/sd.cpp:1397-1559, src/samplers.h:1430-1472) enqueued on the device
// without per-step host round trips.  x:[prompts,L] fp32 is updated in place; noise:[steps,prompts,L]; the five per-step scalar arrays
// have `steps` entries; clip (may be NULL) is a sixth: per-step clamp of the new latents, 0 = none.  *ms (may be NULL) receives the device time of the loop.
char* model_hip_sampler_loop(Handle* h, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, float* x, const float* noise,
                             const float* c_in, const float* c_out, const float* t, const float* sigma, const float* d_sigma, const float* sigma_up, float guidance, const float* clip,
                             double* ms) {
    return euler_a_loop(h, 2, guidance, sample_name, timestep_name, out_name, steps, prompts, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, clip, ms);
}
// the same loop with a one-evaluation multistep sampler of src/samplers.h.  sampler: 0 = dpm++2m / dpm++2mv2, 1 = ipndm, 2 = ipndm_v, 3 = ipndm_vo,
// 4 = taylor3, 5 = ddim; order: [steps] int (0 = the sampler's first-step form; <= step index; sampler 0 also takes 2 = the plain Euler step of the
// reference's SDXL last-step rule, src/sd.cpp:1705-1719, at any step); coef: [steps, 6] float = k0..k4 of the step's
// osg_multistep_form (include/osgpu.h) and DDIM's prescale factor of x; dcoef: [steps, 2] double = DDIM's (da, db); n_coef / n_dcoef: their lengths.
char* model_hip_sampler_loop_multistep(Handle* h, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, int sampler, float* x,
                                       const float* c_in, const float* c_out, const float* t, const float* sigma, const int* order, const float* coef,
                                       unsigned long long n_coef, const double* dcoef, unsigned long long n_dcoef, float guidance, double* ms) {
    return multistep_loop(h, 2, guidance, sample_name, timestep_name, out_name, steps, prompts, sampler, x, c_in, c_out, t, sigma, order, coef, n_coef, dcoef, n_dcoef, ms);
}
// the two loops above for a plan that holds ONE sample per prompt (SDXL Turbo: CFGDenoiser_CompVisDenoiser returns the cond branch alone, src/sd.cpp:1537-1541):
// den = eps*c_out + x, no guidance.  The arguments of their siblings without `guidance`; the plan's batch must be `prompts`.
char* model_hip_sampler_loop_single(Handle* h, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, float* x, const float* noise,
                                    const float* c_in, const float* c_out, const float* t, const float* sigma, const float* d_sigma, const float* sigma_up,
                                    const float* clip, double* ms) {
    return euler_a_loop(h, 1, 0.f, sample_name, timestep_name, out_name, steps, prompts, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, clip, ms);
}
char* model_hip_sampler_loop_multistep_single(Handle* h, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, int sampler, float* x,
                                              const float* c_in, const float* c_out, const float* t, const float* sigma, const int* order, const float* coef,
                                              unsigned long long n_coef, const double* dcoef, unsigned long long n_dcoef, double* ms) {
    return multistep_loop(h, 1, 0.f, sample_name, timestep_name, out_name, steps, prompts, sampler, x, c_in, c_out, t, sigma, order, coef, n_coef, dcoef, n_dcoef, ms);
}
// the same loop with a one-evaluation sampler that adds fresh noise per step (ddpm, ddpm_a, ddim_a, tcd, tcd_a, lcm, dpm++3msde, dpm++3msde_a;
// src/samplers.h:1039-1223, :1406-1428, :412-541).  form: [steps] int, the osg_stochastic_form (include/osgpu.h) of each step; draws: [steps] int,
// != 0 where the step adds noise; coef: [steps, 10] float = k0..k6, n0, n1 of the form and the prescale factor of x (prescale_sample, :38-60; 1 = none);
// n_coef: its length; noise: [steps, prompts, L] or NULL when no step draws.  The *_single form is for a plan with one sample per prompt.
char* model_hip_sampler_loop_stochastic(Handle* h, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, float* x,
                                        const float* c_in, const float* c_out, const float* t, const float* sigma, const int* form, const int* draws,
                                        const float* coef, unsigned long long n_coef, const float* noise, float guidance, double* ms) {
    return stochastic_loop(h, 2, guidance, sample_name, timestep_name, out_name, steps, prompts, x, c_in, c_out, t, sigma, form, draws, coef, n_coef, noise, ms);
}
char* model_hip_sampler_loop_stochastic_single(Handle* h, char* sample_name, char* timestep_name, char* out_name, int steps, int prompts, float* x,
                                               const float* c_in, const float* c_out, const float* t, const float* sigma, const int* form,
                                               const int* draws, const float* coef, unsigned long long n_coef, const float* noise, double* ms) {
    return stochastic_loop(h, 1, 0.f, sample_name, timestep_name, out_name, steps, prompts, x, c_in, c_out, t, sigma, form, draws, coef, n_coef, noise, ms);
}
// latents -> image on the device (decoder_solver / sd_tiled_decoder / sdxl_decoder around the VAE pass, src/sd.cpp:1174-1346, :2357-2516, and Mat::to_pixels
// :340-364): latents [images, 4, h, w] fp32 host -> image [images, 3, u*h, u*w] fp32 and / or pixels [images, u*h, u*w, 3] uint8, either may be NULL (not
// made, not downloaded).  The tile size and u come from the plan's input / output shapes; the plan must have been built by a run() with images * tiles pushes
// (tiles: origins 0, 3t/4, ... and a last one flush with the border, per axis).  image_elems / pixels_elems: the elements the two buffers hold -- a buffer of
// another size than the decode writes is refused, since u is the plan's to know.  *ms (may be NULL) receives the device time from gather to blend.
char* model_hip_decode(Handle* h, char* in_name, char* out_name, int images, int lat_h, int lat_w, float factor, const float* latents, float* image,
                       unsigned long long image_elems, unsigned char* pixels, unsigned long long pixels_elems, double* ms) {
    return guarded(ms, [&] {
        return Plan::on_plan_of(h->model, "Model::hip_decode", [&](Plan& p) {
            return p.decode_tiles(in_name, out_name, images, lat_h, lat_w, factor, latents, image, (size_t)image_elems, pixels, (size_t)pixels_elems);
        });
    });
}
// the reference LLM app's greedy token loop (src/llm.cpp:472-496) on the device: one call, one plan, one synchronisation for up to max_new tokens.  The Model is
// configured as the app configures it (dynamic shapes, fp16 arithmetic, m_use_scaled_dp_attn_op, `logits_name` the only converted output, the caches extra
// outputs) and a run() over the prompt has left the fp32 logits [1, T, V] and the fp16 caches <cache_out_prefix><i> [1, Hkv, P, d], i < n_caches, in m_data (host
// tensors, or device-resident under hip_resident_outputs).  The call computes what this host loop computes:
//     L = last row of logits
//     for n in 0 .. max_new-1:
//         tok = argmax(L)                    the app's scan, src/llm.cpp:355-370: starts at -1.0f, takes v >= prev (the LAST of equal maxima; NaN never; -1 if none)
//         if tok < 0:        stop = 2; break
//         if tok == eos_id:  stop = 1; break      (eos_id < 0: never)
//         tokens[n_tokens++] = tok
//         rename <cache_out_prefix><i> -> <cache_in_prefix><i>; push ids_name = [[tok]], pos_name = [[P]], mask_name = ones(1, P+1); run()
//         P += 1;  L = last row of logits
//     stop = 0 when the budget ran out
// and leaves m_data as that loop would: the caches [1, Hkv, P_final, d] where they were (host or device), logits [1, 1, V] of the last pass that ran (both
// untouched if none ran).  tokens: [max_new] int64; logits_trace (may be NULL): [max_new, V] fp32, row n = the logits of pass n (copied on the device per pass,
// downloaded once).  sync_every > 0: the host reads the stop code after every sync_every passes and ends early; 0: everything is enqueued, one wait at the
// end.  *ms (may be NULL) receives the device time of the loop.  The T = 1 plan behind it is built on the first call and kept while its cache capacity
// (>= P + max_new) and the options suffice; run()'s own plan is not touched.
char* model_hip_generate(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name, const char* cache_in_prefix,
                         const char* cache_out_prefix, int n_caches, int max_new, long long eos_id, int sync_every, long long* tokens, int* n_tokens, int* stop,
                         float* logits_trace, double* ms) {
    return guarded(ms, [&] {
        Plan::DecodeSpec spec;
        spec.ids = ids_name; spec.pos = pos_name; spec.mask = mask_name; spec.logits = logits_name;
        spec.cache_in = cache_in_prefix; spec.cache_out = cache_out_prefix; spec.n_caches = n_caches;
        static_assert(sizeof(long long) == sizeof(int64_t), "tokens are int64");
        return Plan::generate(h->model, spec, max_new, eos_id, sync_every, (int64_t*)tokens, n_tokens, stop, logits_trace, Plan::SampleRule());
    });
}
// repetition, presence and frequency penalties, min-p and the token history they count over (include/osgpu.h states steps 0 and 3b of the rule): the last
// argument of the three _ext calls below.  NULL is the call without the suffix.  The history is what the caller passes -- model_hip_turn_ext does not add
// the prompt by itself; every sequence of a batch starts from the same history.  Refused, each with the call's own prefix: a repetition penalty that is
// NaN, <= 0, infinite or whose fp32 reciprocal is not finite; a presence or frequency penalty that is NaN or infinite (negative values are allowed); min_p
// NaN, < 0 or > 1; min_p > 0 with temperature == 0; a history token outside [0, V); n_history < 0, or history == NULL with n_history > 0;
// n_history + max_new >= 2^24.  With a penalty active and temperature == 0 the greedy pick runs over the adjusted logits.  logits_trace keeps the raw logits.
struct model_hip_sample_ext {
    float repetition_penalty, presence_penalty, frequency_penalty, min_p;
    const long long* history;
    long long n_history;
};
static void apply_ext(Plan::SampleRule& rule, const model_hip_sample_ext* ext) {
    if (!ext) return;
    rule.repetition = ext->repetition_penalty; rule.presence = ext->presence_penalty; rule.frequency = ext->frequency_penalty; rule.min_p = ext->min_p;
    rule.history = ext->history; rule.n_history = ext->n_history;
}
char* model_hip_generate_sampled_ext(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name,
                                     const char* cache_in_prefix, const char* cache_out_prefix, int n_caches, int max_new, long long eos_id, int sync_every,
                                     long long* tokens, int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature, long long top_k, float top_p,
                                     unsigned long long seed, unsigned long long draw_base, const model_hip_sample_ext* ext);
char* model_hip_generate_batch_ext(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name,
                                   const char* cache_in_prefix, const char* cache_out_prefix, int n_caches, int n_seq, int max_new, long long eos_id,
                                   int sync_every, long long* tokens, int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature,
                                   long long top_k, float top_p, const unsigned long long* seeds, unsigned long long draw_base, const model_hip_sample_ext* ext);
char* model_hip_turn_ext(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name, const char* cache_in_prefix,
                         const char* cache_out_prefix, int n_caches, const long long* prompt, int n_prompt, int chunk, long long capacity, int max_new,
                         long long eos_id, int sync_every, long long* tokens, int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature,
                         long long top_k, float top_p, unsigned long long seed, unsigned long long draw_base, const model_hip_sample_ext* ext);
// model_hip_generate with a sampling rule in the argmax's place (osg_decode_sample, include/osgpu.h states the rule in full): temperature > 0 divides the
// logits, top_k > 0 keeps the k largest, top_p < 1 the shortest prefix that holds that share of the mass, and the token is drawn with Philox4x32-10 keyed by
// `seed` at draw index draw_base + n_tokens -- so a call of N tokens equals calls of a and N - a tokens, the second with draw_base = a.  temperature = 0
// is model_hip_generate itself (the other four arguments are still checked).  Refused, each with "Model::hip_generate: ": a temperature that is negative, NaN,
// infinite or so small that 1 / temperature is not finite in fp32; top_k < 0; top_p NaN, <= 0 or > 1.  The decode plan is the one model_hip_generate builds
// and keeps: a sampled and a greedy call share it.
char* model_hip_generate_sampled(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name, const char* cache_in_prefix,
                                 const char* cache_out_prefix, int n_caches, int max_new, long long eos_id, int sync_every, long long* tokens, int* n_tokens,
                                 int* stop, float* logits_trace, double* ms, float temperature, long long top_k, float top_p, unsigned long long seed,
                                 unsigned long long draw_base) {
    return model_hip_generate_sampled_ext(h, ids_name, pos_name, mask_name, logits_name, cache_in_prefix, cache_out_prefix, n_caches, max_new, eos_id, sync_every,
                                          tokens, n_tokens, stop, logits_trace, ms, temperature, top_k, top_p, seed, draw_base, nullptr);
}
char* model_hip_generate_sampled_ext(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name,
                                     const char* cache_in_prefix, const char* cache_out_prefix, int n_caches, int max_new, long long eos_id, int sync_every,
                                     long long* tokens, int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature, long long top_k, float top_p,
                                     unsigned long long seed, unsigned long long draw_base, const model_hip_sample_ext* ext) {
    return guarded(ms, [&] {
        Plan::DecodeSpec spec;
        spec.ids = ids_name; spec.pos = pos_name; spec.mask = mask_name; spec.logits = logits_name;
        spec.cache_in = cache_in_prefix; spec.cache_out = cache_out_prefix; spec.n_caches = n_caches;
        Plan::SampleRule rule;
        rule.temperature = temperature; rule.top_k = (long)top_k; rule.top_p = top_p; rule.seed = seed; rule.draw_base = draw_base;
        apply_ext(rule, ext);
        return Plan::generate(h->model, spec, max_new, eos_id, sync_every, (int64_t*)tokens, n_tokens, stop, logits_trace, rule);
    });
}
// n_seq sampled continuations of ONE prompt in one call: after the same batch-1 run() over the prompt, sequence s is exactly the loop of
// model_hip_generate_sampled with seed = seeds[s] (draw index draw_base + n_tokens[s]), on copies of the prompt's caches of its own and with a state of its
// own.  The n_seq sequences share every pass: a decode plan of batch n_seq (n_seq is part of its key; a call with another n_seq rebuilds it), whose weights
// are read once per pass for all of them.  A sequence that stops (eos_id, an invalid row, the budget) stops alone: its picks become no-ops and its slot of
// the pass recomputes its last token's pass, as the single loop does after a stop; nothing on the device waits.  tokens: [n_seq][max_new] int64; n_tokens,
// stop: [n_seq]; logits_trace (may be NULL): [n_seq][max_new][V] fp32, rows [s][0 .. n_tokens[s]) are written.  sync_every > 0 ends the call early only once
// EVERY sequence has stopped.  m_data is left untouched -- the prompt's logits and caches are as before the call, and the caller carries on through run() with
// the continuation it picks.  Refused, each with "Model::hip_generate_batch: ": what model_hip_generate_sampled refuses, n_seq < 1, seeds == NULL, and
// temperature == 0 (n_seq greedy sequences are one sequence n_seq times: model_hip_generate gives it).
char* model_hip_generate_batch(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name, const char* cache_in_prefix,
                               const char* cache_out_prefix, int n_caches, int n_seq, int max_new, long long eos_id, int sync_every, long long* tokens,
                               int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature, long long top_k, float top_p,
                               const unsigned long long* seeds, unsigned long long draw_base) {
    return model_hip_generate_batch_ext(h, ids_name, pos_name, mask_name, logits_name, cache_in_prefix, cache_out_prefix, n_caches, n_seq, max_new, eos_id,
                                        sync_every, tokens, n_tokens, stop, logits_trace, ms, temperature, top_k, top_p, seeds, draw_base, nullptr);
}
char* model_hip_generate_batch_ext(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name,
                                   const char* cache_in_prefix, const char* cache_out_prefix, int n_caches, int n_seq, int max_new, long long eos_id,
                                   int sync_every, long long* tokens, int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature,
                                   long long top_k, float top_p, const unsigned long long* seeds, unsigned long long draw_base, const model_hip_sample_ext* ext) {
    return guarded(ms, [&] {
        Plan::DecodeSpec spec;
        spec.ids = ids_name; spec.pos = pos_name; spec.mask = mask_name; spec.logits = logits_name;
        spec.cache_in = cache_in_prefix; spec.cache_out = cache_out_prefix; spec.n_caches = n_caches;
        Plan::SampleRule rule;
        rule.temperature = temperature; rule.top_k = (long)top_k; rule.top_p = top_p; rule.draw_base = draw_base;
        apply_ext(rule, ext);
        return Plan::generate(h->model, spec, max_new, eos_id, sync_every, (int64_t*)tokens, n_tokens, stop, logits_trace, rule, n_seq, seeds, true);
    });
}
// One chat turn of the reference's second application (src/llm.cpp:456-497) as one call: prompt tokens in, generated tokens out.  A run() has happened before
// (the app's weight-loading pass counts), and the conversation so far is the caches <cache_out_prefix><i> [1, Hkv, P, d] fp16 in m_data (host or
// device-resident) or, where those are absent, <cache_in_prefix><i> as the caller pushed them; P = 0 rows is the app's first turn (:400-412).  Neither
// present: refused.  The call computes what this host flow computes, the prompt fed in pieces of `chunk` tokens:
//     for each piece j:  forward(piece_j, positions P + j * chunk ..., mask ones)          (run() with the caches renamed, as the app does)
//     then the token loop of model_hip_generate (temperature == 0: the greedy pick) or model_hip_generate_sampled, from the last row of the last piece's logits
// A last piece of r < chunk tokens runs as a full chunk whose tail rows hold padding (token 0, position 0): they are appended behind the valid length
// P + n_prompt and never count -- the first generated token overwrites the first of them, and no real row sees one, since every padding row stands behind
// every real row and the attention is causal.  On the device: one upload of the prompt, then per piece osg_prefill_stage + the pass of the resident chunk
// plan (osg_kv_append_rows_at, osg_sdpa_chunk over capacity buffers), the first token picked from the prefill's own logits row on the device; between the
// first chunk and the end of the turn the host waits for the device only where sync_every > 0 says so.
// It leaves in m_data: the caches <cache_out_prefix><i> [1, Hkv, P + n_prompt + n_tokens, d] where they were (host or device; an empty cache counts as
// device-resident under hip_resident_outputs) and `logits` [1, 1, V], the row of the last pass that ran -- for max_new == 0, or when the first pick stops the
// loop, the last real row of the prefill.  (run() leaves [1, T, V]; the app reads the last row only.)  The caches it started from are consumed.
// capacity: rows of the capacity buffers; at least max(P + ceil(n_prompt / chunk) * chunk, P + n_prompt + max_new) are taken, rounded up to 64, and
// capacity > 0 asks for at least that many, so that later turns rebuild nothing.  Both plans are kept across turns while their key and capacity suffice.
// tokens / n_tokens / stop / logits_trace / sync_every / the sampling rule: as model_hip_generate_sampled.  *ms: device time of the whole turn.
// Refused, each with "Model::hip_turn: ": what model_hip_generate_sampled refuses, n_prompt < 1, chunk outside [1, 512], capacity < 0, positions or token
// ids (the prompt's included) beyond the smallest table they index.
char* model_hip_turn(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name, const char* cache_in_prefix,
                     const char* cache_out_prefix, int n_caches, const long long* prompt, int n_prompt, int chunk, long long capacity, int max_new,
                     long long eos_id, int sync_every, long long* tokens, int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature,
                     long long top_k, float top_p, unsigned long long seed, unsigned long long draw_base) {
    return model_hip_turn_ext(h, ids_name, pos_name, mask_name, logits_name, cache_in_prefix, cache_out_prefix, n_caches, prompt, n_prompt, chunk, capacity,
                              max_new, eos_id, sync_every, tokens, n_tokens, stop, logits_trace, ms, temperature, top_k, top_p, seed, draw_base, nullptr);
}
char* model_hip_turn_ext(Handle* h, const char* ids_name, const char* pos_name, const char* mask_name, const char* logits_name, const char* cache_in_prefix,
                         const char* cache_out_prefix, int n_caches, const long long* prompt, int n_prompt, int chunk, long long capacity, int max_new,
                         long long eos_id, int sync_every, long long* tokens, int* n_tokens, int* stop, float* logits_trace, double* ms, float temperature,
                         long long top_k, float top_p, unsigned long long seed, unsigned long long draw_base, const model_hip_sample_ext* ext) {
    return guarded(ms, [&] {
        Plan::DecodeSpec spec;
        spec.ids = ids_name; spec.pos = pos_name; spec.mask = mask_name; spec.logits = logits_name;
        spec.cache_in = cache_in_prefix; spec.cache_out = cache_out_prefix; spec.n_caches = n_caches;
        Plan::SampleRule rule;
        rule.temperature = temperature; rule.top_k = (long)top_k; rule.top_p = top_p; rule.seed = seed; rule.draw_base = draw_base;
        apply_ext(rule, ext);
        return Plan::turn(h->model, spec, prompt, n_prompt, chunk, capacity, max_new, eos_id, sync_every, (int64_t*)tokens, n_tokens, stop, logits_trace, rule);
    });
}
// steps of the chunk plan model_hip_turn built, as model_hip_plan_info gives them, after a first line "prefill chunk <C> capacity <CAP>"; "ERROR: ..." on error
char* model_hip_prefill_plan_info(Handle* h) {
    try {
        return dup_cstr(Plan::prefill_info(h->model));
    } catch (const std::exception& e) {
        return dup_cstr(std::string("ERROR: ") + e.what());
    }
}
// steps of the decode plan model_hip_generate built, as model_hip_plan_info gives them, after a first line "decode capacity <CAP>" (a plan of n_seq > 1
// sequences: "decode capacity <CAP> sequences <n_seq>"); "ERROR: ..." on error
char* model_hip_decode_plan_info(Handle* h) {
    try {
        return dup_cstr(Plan::decode_info(h->model));
    } catch (const std::exception& e) {
        return dup_cstr(std::string("ERROR: ") + e.what());
    }
}
// steps and arena placement of the current plan (malloc'ed text, free with model_free_buffer); "ERROR: ..." on error
char* model_hip_plan_info(Handle* h) {
    try {
        return dup_cstr(h->model.hip_plan_info());
    } catch (const std::exception& e) {
        return dup_cstr(std::string("ERROR: ") + e.what());
    }
}
// per-step timing report (malloc'ed text, free with model_free_buffer); on error the text starts with "ERROR: "
char* model_hip_profile(Handle* h, int reps) {
    try {
        return dup_cstr(h->model.hip_profile(reps));
    } catch (const std::exception& e) {
        return dup_cstr(std::string("ERROR: ") + e.what());
    }
}

// range_data.txt (per-op output ranges of a calibration run; src/sd.cpp:1214 reads it before the uint8 VAE decode, :1241 writes it after
// --decoder-calibrate): Model::read_range_data / write_range_data have no export in the reference's C API (the app links the class)
char* model_hip_read_range_data(Handle* h, const char* filename) {
    return guarded([&] { h->model.read_range_data(filename); });
}
char* model_hip_write_range_data(Handle* h, const char* filename) {
    return guarded([&] { h->model.write_range_data(filename); });
}

}  // extern "C"
