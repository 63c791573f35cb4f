// plan.h -- the device execution plan behind Model::run().
//
// The reference interprets the graph op by op on the host, allocating every output and converting layouts/dtypes
// around each call (reference src/onnxstream.cpp:3550-8269).  On MI355X that shape of execution is launch- and
// PCIe-bound, so this backend lowers the WHOLE graph once:
//   parse (model.cpp) -> fetch weights through the WeightsProvider in model order and make them resident in HBM
//   -> graph-level fusion (SiLU, GroupNorm, LayerNorm, GEGLU, Linear+bias+residual, attention incl. head split/merge)
//   -> lowering to a list of kernel launches over device-resident f16 activations (NHWC around convolutions)
//   -> liveness-based packing of all activations into one HBM arena
//   -> eager first pass, then capture into a hipGraph that later passes replay.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <unordered_map>
#include <set>
#include <string>
#include <vector>

#include "backend.h"
#include "onnxstream.h"

namespace onnxstream {

enum class Lay { plain, nhwc };

struct Val {
    std::string name;
    std::vector<long> shape;      // logical (ONNX) shape of ONE sample
    osg_dtype dtype = OSG_F16;
    Lay lay = Lay::plain;         // nhwc: 4-D logical [n,C,H,W] stored as [n,H,W,C]
    bool batched = false;         // one copy per pushed sample, stacked contiguously
    bool is_const = false;        // resident weight / constant
    int root = -1;                // >=0: alias sharing the storage of another val
    void* dptr = nullptr;         // constants & pinned buffers: own allocation
    size_t offset = 0;            // activations: offset inside the arena
    bool pinned = false;          // graph input/output staging: never recycled
    int first = 1 << 30, last = -1;
    std::vector<float> host_f;    // small constants, available at plan time
    std::vector<int64_t> host_i;
    bool host_valid = false;
    bool up32 = false;            // fp32 result of an op the Model's m_requires_upcast flags (LLM layer norms): rounded to f16 when an unflagged op reads it
    bool host_only = false;       // value computed at plan time (Shape / Gather / Cast / Concat chains over shapes): no device storage until a launch asks for it
    int as_plain = -1, as_nhwc = -1, as_dense = -1;
    // column-slice view of a wider 2-D buffer (merged projections): rows are `ld` elements apart, starting `view_off` bytes into the root
    long ld = 0;
    size_t view_off = 0;
    float qscale = 1.f;           // dtype == OSG_U8: value = (q - qzp) * qscale  (weights: from model.txt; uint8 activations: from range_data / the
    int qzp = 0;                  //   dynamic quantisation of a pushed input)
    int qsrc = -1;                // >= 0: the val whose (qscale, qzp) this one shares (Reshape / Transpose / Resize carry them over) -- read at RUN time
    bool qdyn = false;            // parameters change from run to run (a pushed input and what merely re-arranges it)
    bool qown = false;            // an alias with parameters of its OWN, not its root's (Squeeze / Unsqueeze: the reference hands the codes on without their parameters)
    int as_nk_u8 = -1;            // [N,K] twin of a [K,N] uint8 matrix
    // a VIRTUAL Expand (grouped-query attention's repeat_kv: [1,Hkv,1,S,d] -> [1,Hkv,rep,S,d], read only by ScaledDotProductAttention through a Reshape):
    // never materialised -- the attention launch reads `rep_src` with Hkv heads (plan.cpp lower_expand / lower_sdpa)
    int rep_src = -1;
    long rep = 1;
    // decode plans (Plan::generate): an int64 graph input whose VALUE lives on the device only (input_ids / position_ids, written by osg_decode_pick):
    // a Gather reads it as its index buffer, nothing may evaluate it at plan time
    bool dev_int = false;
    // decode plans: a key/value cache in its capacity buffer [Hkv][CAP][d] -- valid rows are counted on the device (Plan::dec_state)
    bool kv_cap = false;
    long numel() const { long n = 1; for (auto d : shape) n *= d; return n; }
};

struct Step {
    std::string what;
    std::function<void()> run;
    std::vector<int> reads, writes;
    double flops = 0;             // algorithmic 2*MAC count of a contraction step (0 for memory-bound steps)
    bool side = false;            // touches memory outside its declared lists (the GroupNorm statistics block): never hoisted out of the sampler step
};

struct Lowering;

// Device-resident constants that outlive a Plan (owned by the Model, next to the backend): a plan is rebuilt when the number of pushed
// samples, the input shapes or a hip_* option change, and a rebuild must not go back to the WeightsProvider -- by then a strictly
// sequential provider is exhausted and, with m_use_ops_cache, the host copies were remove()d (reference: the ops cache keeps the packed
// weights across runs, src/onnxstream.cpp:4556-4569).  `base` = weights as pulled through the provider ("file|dtype"), `derived` = the
// re-laid-out / merged / folded copies the lowering makes of them, by tag.  Not used in streamed-weights mode.
struct ConstPool {
    struct Base {
        void* dptr = nullptr;
        size_t bytes = 0;
        std::vector<float> host_f;
        std::vector<int64_t> host_i;
        bool host_valid = false;
    };
    std::map<std::string, Base> base;
    std::map<std::string, std::pair<void*, size_t>> derived;
    std::vector<TensorDataType> occ_types;   // resolved storage type of every weight occurrence, model order
    bool complete = false;                   // every occurrence of the graph went through the provider once
    size_t bytes = 0;
    // the op list AFTER the fusion passes, for models that re-plan on every call (m_support_dynamic_shapes: the LLM flow): the passes match graph
    // structure, constants and declared shapes -- none of which change between calls -- so their result is reused while `fused_key` (every option
    // they read, the extra outputs, the per-op m_requires_upcast answers) and the number of constant vals stay the same
    std::string fused_key;
    std::vector<Operation> fused_ops;
    size_t fused_const_vals = 0;
    bool fused_valid = false;
    std::vector<Val> snap_vals;              // the constant vals load_weights() builds from `base`, as they are right after it (same validity as fused_ops)
    size_t snap_weight_bytes = 0;
    std::vector<std::string> in_names;       // the graph's input names (consumed, never produced), in discovery order
    // device buffers (arena, small-allocation slabs) of a destroyed plan of such a model, handed to the next one: a hipMalloc + hipFree pair per buffer
    // and call otherwise
    std::vector<std::pair<void*, size_t>> spare;
    void* take(size_t bytes, size_t* got) {
        int best = -1;
        for (size_t i = 0; i < spare.size(); i++)
            if (spare[i].second >= bytes && (best < 0 || spare[i].second < spare[best].second)) best = (int)i;
        if (best < 0 || spare[best].second > 4 * bytes + ((size_t)8 << 20)) return nullptr;   // (no 1 GiB arena for a 1 MiB request)
        void* p = spare[best].first;
        *got = spare[best].second;
        spare.erase(spare.begin() + best);
        return p;
    }
    // ... and the buffers of device-resident outputs (Model::m_hip_resident_outputs), by size class: a cache grows by one row per call, so its buffer is
    // sized to the next power of two and the buffers of the call before last (released when their plan goes) serve the call that comes
    std::map<size_t, std::vector<void*>> spare_class;
    static size_t size_class(size_t bytes) {
        size_t c = 4096;
        while (c < bytes) c <<= 1;
        return c;
    }
    void* take_class(HipBackend& be, size_t cls) {
        auto it = spare_class.find(cls);
        if (it != spare_class.end() && !it->second.empty()) {
            void* p = it->second.back();
            it->second.pop_back();
            return p;
        }
        return be.malloc(cls);
    }
    void give_class(HipBackend& be, void* p, size_t cls) {
        auto& v = spare_class[cls];
        if (v.size() >= 512) be.free(p);
        else v.push_back(p);
    }
    void give(HipBackend& be, void* p, size_t bytes) {
        if (spare.size() >= 8) {   // keep the newest: drop the smallest
            size_t k = 0;
            for (size_t i = 1; i < spare.size(); i++)
                if (spare[i].second < spare[k].second) k = i;
            be.free(spare[k].first);
            spare.erase(spare.begin() + k);
        }
        spare.push_back({p, bytes});
    }
    // what the Model is told about its sampler loops (option hip_loop_hoist, model_hip_sampler_schedule): kept here, with the other state a Model keeps for
    // its plans, and reached through Plan::loop_options -- onnxstream.h, the header the reference application is compiled against, stays as it is.  Not
    // touched by clear(): another model file does not change what the caller asked for
    struct LoopOptions {
        bool hoist = true;                 // hip_loop_hoist: the loops launch per step only what depends on the latent (Plan::Hoist); false: the whole pass
        int rows = 64;                     // hip_loop_hoist_rows: rows of the timestep table; lowered by tests to reach the table-full path
        std::vector<float> schedule;       // the timestep values the next loop calls walk; a plan fills their rows once per serial
        unsigned long long schedule_serial = 0;
    };
    LoopOptions loop;
    // planner options added after the reference application was compiled against onnxstream.h (which therefore stays as it is), reached through Plan::plan_options.
    // Not touched by clear() either
    struct PlanOptions {
        // hip_fuse_shortcut: a ResNet's 1x1 conv_shortcut runs as a second K segment of its 3x3 conv2 (osg_conv2d_nhwc_cat), no launch of its own.  Off by
        // default: the output loses one f16 rounding, so its bits are not the un-fused plan's
        bool fuse_shortcut = false;
    };
    PlanOptions opts;
    // the resident decode plan of the Model (Plan::generate): T = 1 over key/value caches of a fixed capacity, kept across generate calls while the
    // capacity and the options it was built with (`decode_key`) still fit
    Plan* decode_plan = nullptr;
    std::string decode_key;
    void drop_decode();          // (plan_llm.cpp: Plan is incomplete here)
    // the resident chunk plan beside it (Plan::turn): T = C rows of a prompt over caches of the same kind, keyed as the decode plan plus C
    Plan* prefill_plan = nullptr;
    std::string prefill_key;
    void drop_prefill();
    void clear(HipBackend& be) {
        drop_decode();           // (first: its buffers go back to the lists freed below)
        drop_prefill();
        for (auto& kv : base) be.free(kv.second.dptr);
        for (auto& kv : derived) be.free(kv.second.first);
        for (auto& sp : spare) be.free(sp.first);
        spare.clear();
        for (auto& kv : spare_class)
            for (void* p : kv.second) be.free(p);
        spare_class.clear();
        base.clear(); derived.clear(); occ_types.clear();
        complete = false; bytes = 0;
        fused_valid = false; fused_ops.clear(); fused_key.clear(); snap_vals.clear(); snap_weight_bytes = 0; in_names.clear();
    }
};

// f16 bits -> float (host side: constants, folded weights, the sampler's table); shared by plan.cpp and plan_run.cpp
inline float half_to_float(uint16_t h) {
    uint32_t sign = (h >> 15) & 1, exp = (h >> 10) & 0x1f, man = h & 0x3ff;
    float v;
    if (exp == 0) v = std::ldexp((float)man, -24);
    else if (exp == 31) v = man ? NAN : INFINITY;
    else v = std::ldexp((float)(man | 0x400), (int)exp - 25);
    return sign ? -v : v;
}

// Plan::in_flight from the first enqueue to the wait at the end of the scope; an exception on the way leaves it set (the plan's destructor then waits for the device)
struct FlightGuard {
    bool& f;
    explicit FlightGuard(bool& f_) : f(f_) { f = true; }
    ~FlightGuard() { if (!std::uncaught_exceptions()) f = false; }
};

struct Plan {
    Plan(Model& m, HipBackend& be, ConstPool& pool, size_t batch);
    ~Plan();
    void build();
    // while_device_runs: host work the caller wants done between "the pass is enqueued" and "wait for it" (Model::run destroys the plan it replaced there:
    // the LLM flow re-plans on every call, and tearing the old plan down took 0.8 ms of every call's critical path)
    void execute(const std::function<void()>& while_device_runs = nullptr);
    // relaunch the captured pass `n` times on the inputs already resident in HBM; per-launch device ms (HIP events)
    void replay(int n, float* ms_each);
    // overwrite sample `index` of a graph input in its device staging (what run() does for every pushed tensor) without running a pass
    void set_input(const std::string& name, long index, const float* data, size_t count);
    // ---- the device sampler loops ----
    // branches (all three loops): UNet samples per prompt in the plan's batch.  2 = the cond / uncond pair with the CFG combine: the plan's batch must be
    // 2*prompts (push 2p = cond, 2p+1 = uncond of prompt p).  1 = one sample per prompt and den = eps*c_out + x, what CFGDenoiser_CompVisDenoiser returns
    // in Turbo mode (src/sd.cpp:1537-1541): the plan's batch must be `prompts`, guidance is unused and the osg_sampler_*_single kernels run (the
    // model_hip_sampler_loop*_single exports).
    //
    // the reference app's denoising loop with the CFG combine and the Euler-Ancestral update on the device: `steps` passes enqueued
    // back to back, one host sync at the end.  Every other input (context, ...) must already be resident from an earlier run().  Per-step scalars come
    // from the caller (who owns the schedule): c_in, c_out, t, sigma = sigma_i, d_sigma = sigma_down - sigma_i, sigma_up, clip (NULL or per-step clamp of
    // the new latents, 0 = none).  x: [prompts, L] fp32 host, updated in place; noise: [steps, prompts, L] fp32 host.  Returns the device time of the
    // whole loop in ms.
    double sampler_loop(const std::string& sample_name, const std::string& timestep_name, const std::string& out_name, int n_steps, int prompts,
                        float* x, const float* noise, const float* c_in, const float* c_out, const float* t, const float* sigma, const float* d_sigma,
                        const float* sigma_up, float guidance, const float* clip, int branches = 2);
    // the same loop with one of the one-evaluation multistep samplers of src/samplers.h (DPM++ 2M / 2M v2, iPNDM, iPNDM_v, iPNDM_vo, Taylor3, DDIM):
    // per step a prepare launch (DDIM: with its in-place prescale of x), the pass, and one osg_sampler_cfg_multistep launch whose form follows
    // from `sampler` (OSG_LOOP_* of exports.cpp) and order[i].  coef: [steps, 6] float (k0..k4 of the form, then DDIM's prescale factor),
    // dcoef: [steps, 2] double (DDIM's da, db); n_coef / n_dcoef are their lengths.  The history ring [H, prompts, L] is allocated once and
    // reused; order[i] <= i is required, so a call never reads an entry an earlier image left behind.  Order 2 of sampler 0 is the Euler step of the
    // reference's SDXL last-step rule (src/sd.cpp:1705-1719); it reads no history and is legal at any step.
    double sampler_loop_multistep(const std::string& sample_name, const std::string& timestep_name, const std::string& out_name, int n_steps, int prompts,
                                  int sampler, float* x, const float* c_in, const float* c_out, const float* t, const float* sigma, const int* order,
                                  const float* coef, size_t n_coef, const double* dcoef, size_t n_dcoef, float guidance, int branches = 2);
    // the same loop with one of the one-evaluation samplers that add fresh noise per step (DDPM(-a), DDIM-a, TCD(-a), LCM, DPM++ 3M SDE(-a);
    // src/samplers.h:1039-1223, :1406-1428, :412-541): per step a prepare launch (with the in-place prescale of x where coef[i][9] != 1, prescale_sample
    // :38-60), the pass, and one osg_sampler_cfg_stochastic / osg_sampler_stochastic_single launch of form[i] (osg_stochastic_form).  coef: [steps, 10]
    // float = k0..k6, n0, n1 of the form and the prescale factor; n_coef its length; noise: [steps, prompts, L] fp32 host or NULL, row i is read
    // when draws[i].  The history ring [3, prompts, L] (create_buffers, :14) exists when an SDE form occurs; OSG_ST_SDE1 / OSG_ST_SDE2 must follow one /
    // two steps that wrote history, so a call never reads an entry an earlier image left behind.
    double sampler_loop_stochastic(const std::string& sample_name, const std::string& timestep_name, const std::string& out_name, int n_steps, int prompts,
                                   float* x, const float* c_in, const float* c_out, const float* t, const float* sigma, const int* form, const int* draws,
                                   const float* coef, size_t n_coef, const float* noise, float guidance, int branches = 2);
    // latents -> image without leaving the device (the VAE decoder plan): upload the latents [images, 4, H, W], osg_decode_gather cuts and scales the
    // tiles into the input staging, the pass (captured, or eager while no graph exists), osg_decode_blend folds the tiles and makes the fp32 image
    // [images, 3, u*H, u*W] and / or the packed uint8 image [images, u*H, u*W, 3]; only the one(s) asked for (non-NULL) come back.  Tile size t and
    // upscale factor u are the plan's own input / output shapes; the plan's batch must be images * tiles.  Returns the device ms from gather to blend.
    // image_elems / pixels_elems: what the caller's buffers hold; a non-NULL buffer of another size than the decode writes is refused (the caller cannot know u).
    double decode_tiles(const std::string& in_name, const std::string& out_name, int images, int H, int W, float factor, const float* latents, float* image,
                        size_t image_elems, uint8_t* pixels, size_t pixels_elems);
    // run(plan) on Model m's plan, recording its last-pass time in the Model; `fn` is the "Model::hip_..." name for the text thrown when there is no plan.
    // The one way from a Model to its plan for the exports (the sampler loops, model_hip_decode).  A static member of Plan, Model's friend, so that
    // onnxstream.h -- the header the reference application is compiled against for the drop-in link (oracle/Makefile) -- stays as it is.
    template <class Run>
    static double on_plan_of(Model& m, const char* fn, Run&& run) {
        if (!m.m_plan) throw std::runtime_error(std::string(fn) + ": no plan (call run() first).");
        const double ms = run(*m.m_plan);
        m.m_last_ms = m.m_plan->last_ms();
        return ms;
    }
    // eager pass with HIP events around every step, `reps` times; "ms<TAB>flops<TAB>bytes<TAB>what" per line (ms = mean)
    std::string profile(int reps);
    // plan introspection for the CPU tests of the host logic (tests/test_planner_cpu.py): one line per step
    //   "step <i> reads=<v,...> writes=<v,...> | <what>"   (val ids are ROOT vals)
    // and per arena val  "val <id> offset=<o> bytes=<b> first=<f> last=<l>", then "arena <bytes>".
    std::string info() const;
    bool compatible(Model& m, size_t batch) const;
    size_t kernel_count() const { return steps.size(); }
    double last_ms() const { return m_last_ms; }

    Model& m;
    HipBackend& be;
    ConstPool& pool;
    long N;  // batch (number of samples pushed under each input name)

    std::vector<Operation> ops;  // working copy of the graph (mutated by the fusion passes)
    std::vector<Val> vals;
    std::unordered_map<std::string, int> by_name;
    std::vector<Step> steps;
    std::vector<char> io_block;   // host side of the gathered input upload / output download of execute()
    size_t gathered_up = 0, gathered_down = 0;   // bytes the last execute() moved that way (0: buffer by buffer)
    std::vector<std::pair<char*, size_t>> slabs;   // the small-allocation slabs of this plan
    bool in_one_slab(const char* lo, const char* hi) const;
    std::vector<void*> owned;     // device allocations owned by the plan (weights, staging, outputs)
    std::vector<std::pair<void*, size_t>> recyclable;   // ... those that go back to the pool's spare list when the model re-plans on every call (slabs, arena)
    bool recycle = false, arena_pooled = false;
    void* pooled_malloc(size_t bytes);
    // small per-plan buffers (input staging, pinned outputs, index / ones / mask constants) are carved out of 8 MiB slabs: a plan of the LLM flow
    // has ~100 of them and is rebuilt on every call -- one hipMalloc each was 2/3 of the rebuild time
    void* small_alloc(size_t bytes);
    char* slab = nullptr;
    size_t slab_left = 0;
    void* arena = nullptr;
    size_t arena_bytes = 0, weight_bytes = 0;

    // streamed-weights mode: how each resident constant is (re)filled from the provider, in the provider's (model) order
    struct WRecipe {
        int val = -1;                 // -1: a repeated occurrence -- fetched (providers serve strictly in order) but not uploaded
        std::string fn;
        TensorDataType ty = TensorDataType::none;
        osg_dtype have = OSG_F16, want = OSG_F16;
        long count = 0;
        float scale = 1.f;
        int zp = 0;
        void* raw = nullptr;          // device staging for weights that need a dtype conversion after the copy
        bool resident = false;        // VRAM-budget mode: inside the budget -- uploaded once, later passes only fetch it from the provider
        bool ring = false;            // VRAM-budget mode: over the budget -- lives in the streaming ring, re-sent every pass
    };
    // ---- VRAM budget (CudaOptions::m_vram_to_use) ----
    size_t vram_budget = 0, resident_bytes = 0, ring_weight_bytes = 0;
    bool budgeted = false;
    void* ring = nullptr;
    size_t ring_bytes = 0, ring_head = 0;
    struct RingOcc { size_t off, size; int last; int marker; };
    std::vector<RingOcc> ring_occ;
    int next_marker = 0, cur_step = 0;
    std::vector<WRecipe> recipes;
    std::vector<size_t> flush_upto;             // per step: how many leading recipes must have been pulled / sent before it runs
    std::map<const void*, size_t> registered;   // provider host buffers page-locked for zero-copy DMA
    size_t streamed_bytes = 0;
    void restream(const WRecipe& r);

    // ivals: an int64 graph input (LLM graphs: input_ids, position_ids, attention_mask) is a PLAN-TIME value -- its numbers feed Gather indices and
    // mask subgraphs that are evaluated while the plan is built, so a plan is only reused for the same numbers (Plan::compatible)
    struct In {
        std::string name; int val; int staging; TensorDataType host_type; std::vector<size_t> shape; std::vector<int64_t> ivals;
        std::shared_ptr<void> resident;   // a device-resident tensor (Tensor::m_hip_resident) read where it lies; kept alive by the plan that reads it
    };
    struct Out {
        std::string name; int val; int f32val; std::vector<size_t> shape; bool raw16 = false;
        void* dev = nullptr;              // m_hip_resident_outputs: the buffer this output is left in (handed to the Tensor in m_data after the pass)
        size_t dev_bytes = 0;
    };
    bool resident_outputs = false;
    struct Calib { int step; std::string op; int val; };   // m_range_data_calibrate: val is measured after `step`, range kept under the op's name
    std::vector<Calib> calib;
    std::vector<In> inputs;
    std::vector<Out> outputs;

    void* samp_x = nullptr;       // sampler_loop state: latents [prompts, L] and the pre-drawn noise [steps, prompts, L], device fp32
    void* samp_noise = nullptr;
    void* samp_hist = nullptr;    // sampler_loop_multistep, sampler_loop_stochastic: history ring [H, prompts, L], device fp32
    size_t samp_x_bytes = 0, samp_noise_bytes = 0, samp_hist_bytes = 0;
    // what the sampler loops share (plan_run.cpp): state and batch checks, the tensors a loop reads and writes, and the frame around the per-step launches
    struct SamplerIO { const In* in_s = nullptr; const In* in_t = nullptr; const Out* out = nullptr; long L = 0, TL = 0; };
    struct SamplerPrescale { bool rescale; float x_scale; };
    void sampler_check_state(const std::string& fn, int prompts, int branches) const;
    SamplerIO sampler_io(const std::string& fn, const std::string& sample_name, const std::string& timestep_name, const std::string& out_name) const;
    template <class Prescale, class Update>
    double sampler_frame(const std::string& fn, const std::string& sample_name, const std::string& timestep_name, const std::string& out_name, int n_steps,
                         int prompts, int branches, float* x, const float* c_in, const float* t, int H, const float* noise, Prescale&& prescale,
                         Update&& update);
    // a grow-only device buffer: (p, have) is reallocated when it holds fewer than `need` bytes; the contents are not kept
    void grow_buffer(void*& p, size_t& have, size_t need);
    void* dec_lat = nullptr;      // decode_tiles state: latents [images, 4, H, W] fp32, image [images, 3, uH, uW] fp32, pixels [images, uH, uW, 3] uint8
    void* dec_img = nullptr;
    void* dec_pix = nullptr;
    size_t dec_lat_bytes = 0, dec_img_bytes = 0, dec_pix_bytes = 0;

    // ---- decode mode: the resident T = 1 plan of the token loop (generate, below) ----
    // Built by the ordinary lowering over `build_inputs` (stand-ins for the graph inputs: one token, caches of CAP - 1 rows, a mask of CAP ones) instead of
    // m.m_data.  input_ids / position_ids are device values (Val::dev_int), the cache inputs live in capacity buffers [Hkv][CAP][d] (Val::kv_cap), a cache
    // Concat is osg_kv_append_at in place and the attention over it osg_sdpa_len: the pass is the same launches for every token and every cache length.
    // chunk plans (Plan::turn): the same build with `chunk` = C > 0 rows per pass -- stand-in caches of CAP - C rows, C tokens and positions, dec_state[0] the
    // row the chunk starts at (osg_prefill_stage writes it); a cache Concat is osg_kv_append_rows_at, the attention osg_sdpa_chunk, which works the causal
    // bound out of that row: the plan-time mask [C][CAP] is checked to be exactly causal and dropped.  dec_tokens holds the prompt (device int64).
    struct DecodeSpec { std::string ids, pos, mask, logits, cache_in, cache_out; int n_caches = 0; long cap = 0; long chunk = 0; };
    const char* dec_fn() const { return dspec.chunk > 0 ? "Model::hip_turn: " : "Model::hip_generate: "; }
    bool decode = false;
    DecodeSpec dspec;
    std::vector<Tensor>* build_inputs = nullptr;
    int* dec_state = nullptr;                 // device int32[4] per sequence (N of them): row, len, n_tokens, stop (include/osgpu.h, osg_decode_pick)
    long dec_pos_limit = 1L << 62, dec_tok_limit = 1L << 62;   // rows of the smallest table a Gather indexes with position_ids / input_ids
    void* dec_tokens = nullptr;               // device int64 [N][max_new]
    void* dec_trace = nullptr;                // device fp32 [N][max_new, V]
    void* dec_seeds = nullptr;                // device uint64 [N]: the seeds of a generate_batch call
    size_t dec_tokens_bytes = 0, dec_trace_bytes = 0, dec_seeds_bytes = 0;
    // penalties and min-p (SampleRule below): kept with the decode plan, allocated by the first call that needs them, no part of its key, capture or text
    void* dec_counts = nullptr;               // device int32 [N][V]: how often sequence s has seen token i (history + what it appended)
    void* dec_adjusted = nullptr;             // device fp32 [N][V]: the logits after step 0 (osg_decode_penalize), what the pick / sample then reads
    void* dec_history = nullptr;              // device int64 [n_history]: the caller's history, uploaded per call
    size_t dec_counts_bytes = 0, dec_adjusted_bytes = 0, dec_history_bytes = 0;
    int cache_index(const std::string& name, const std::string& prefix) const;   // i of "<prefix><i>", i < n_caches; -1 otherwise
    // ---- the LLM calls (plan_llm.cpp): generate and turn below, built from the steps they share.  Members here: what both refuse (check_loop_call), the kept
    // plan (resident_plan) and one pass of it (run_pass, plan_run.cpp, beside capture); file-local there: the plan's loop bindings, the table limits, the
    // host-cache scratch with staging in and publishing out, the choice of pick launch ----
    using CacheGeo = std::vector<std::array<long, 2>>;      // (Hkv, d) per cache
    // what differs between the Model's two resident plans: the decode plan (T = 1, one sequence per sample of the batch) and the chunk plan (T = C, batch 1)
    struct ResidentKind {
        Plan*& slot; std::string& slot_key;       // where the ConstPool keeps it: decode_plan / decode_key, prefill_plan / prefill_key
        long chunk;                               // DecodeSpec::chunk: 0 = T is 1; C = T is C, and the ids / pos staging starts out zeroed (padding rows)
        long batch;                               // samples of the plan (part of the key)
        long key_dim;                             // the key's one field of the call: V, which a decode plan's logits must have; C for a chunk plan
        std::vector<const char*> appends;         // what the steps that append to a cache in place are called in such a plan
        std::function<bool(long)> logits_ok;      // whether an fp32 logits output of that many elements per sample is the loop's ...
        std::string logits_want;                  // ... and what to call it when none is
    };
    static Plan* resident_plan(Model& m, const std::string& fn, const DecodeSpec& names, const CacheGeo& geo, long min_cap, const ResidentKind& k);
    void run_pass();
    // a Tensor that owns the device buffer `dev` of `bytes` bytes (execute()'s resident outputs, the caches generate and turn publish); plan_run.cpp
    static Tensor resident_tensor(Model& m, const std::string& name, std::vector<size_t> shape, void* dev, size_t bytes);
    // the reference app's token loop (src/llm.cpp:472-496) on the device: see model_hip_generate (exports.cpp) for the contract.  A static member of Plan
    // for the reason given at on_plan_of; the decode plan itself is kept in the Model's ConstPool.
    // how a token is taken from the logits: default-constructed = greedy, the app's argmax (osg_decode_pick); temperature > 0 = the sampling rule of
    // include/osgpu.h (osg_decode_sample).  Sampling is outside the decode plan: the plan, its capacity, its capture and its text are the same either way.
    // repetition / presence / frequency / min_p and the history (host int64 [n_history]): step 0 and step 3b of the rule.  counted() = the loop keeps the
    // count table and hands it to the _ext entry points; penalized() = step 0 changes a logit, so osg_decode_penalize runs before every pick.
    struct SampleRule {
        float temperature = 0.0f; long top_k = 0; float top_p = 1.0f; unsigned long long seed = 0, draw_base = 0;
        float repetition = 1.0f, presence = 0.0f, frequency = 0.0f, min_p = 0.0f;
        const long long* history = nullptr; long long n_history = 0;
        bool penalized() const { return repetition != 1.0f || presence != 0.0f || frequency != 0.0f; }
        bool extended() const { return penalized() || min_p != 0.0f; }
        // what every call refuses, `fn` its prefix; V < 0: the vocabulary is not known yet (the history's tokens are checked once it is)
        void check(const std::string& fn, long long max_new, long V) const;
    };
    // run_first_why: the caller's reason inside "run() once first (...)" -- generate starts from a run()'s logits and caches, a turn only needs its weights
    static void check_loop_call(Model& m, const std::string& fn, const DecodeSpec& names, int max_new, const int64_t* tokens, const SampleRule& rule,
                                const char* run_first_why);
    // batch (model_hip_generate_batch): n_seq sampled sequences from the one prompt in a decode plan of batch n_seq, sequence s with seeds[s] and its own
    // state, caches and stop; the outputs are arrays over the sequences and m_data is left untouched.  n_seq is part of the decode plan's key.
    // entry (Plan::turn): the loop starts from what a prefill leaves on the device instead of from m_data -- caches of P rows in capacity buffers of
    // `cap` rows per head, the logits row the first token is picked from; `prefill` enqueues that work (it starts the timer) after the loop's own
    // uploads, so that the host waits for nothing between the first chunk and the end of the loop.  V, the shape of the logits tensor to leave, and
    // whether cache i was device-resident come with it; nothing of it is read from m_data.
    struct TurnEntry {
        long P = 0, cap = 0, V = 0, min_cap = 0;
        CacheGeo geo;
        std::vector<const void*> caches;             // capacity buffers [Hkv][cap][d]
        std::vector<char> was_resident;
        std::vector<size_t> logits_shape;            // [1, T, V]: the rank to keep
        std::function<const float*()> prefill;       // enqueues the chunks, returns the device address of the last real logits row
    };
    static double generate(Model& m, const DecodeSpec& names, int max_new, long long eos_id, int sync_every, int64_t* tokens, int* n_tokens, int* stop,
                           float* logits_trace, const SampleRule& rule, int n_seq = 1, const unsigned long long* seeds = nullptr, bool batch = false,
                           const TurnEntry* entry = nullptr);
    static std::string decode_info(Model& m);
    // one chat turn on the device (model_hip_turn, exports.cpp states the contract): the prompt in chunks through the resident chunk plan, then the loop above
    static double turn(Model& m, const DecodeSpec& names, const long long* prompt, int n_prompt, int chunk, long long capacity, int max_new, long long eos_id,
                       int sync_every, int64_t* tokens, int* n_tokens, int* stop, float* logits_trace, const SampleRule& rule);
    static std::string prefill_info(Model& m);
    // a copy of a device-resident tensor's bytes (Tensor::m_hip_resident) for the host; the tensor stays where it is (model_hip_get_tensor_f16)
    static void read_resident(Model& m, const Tensor& t, void* dst);

    osg_graph* graph = nullptr;
    // ---- loop hoist (option hip_loop_hoist): the launches of the pass that do not depend on the latent leave the sampler step ----
    // Classes, from two taint bits propagated through the declared reads / writes: per-step (reads something `sample` reaches), T (the timestep but not
    // the sample), P (neither: the prompt, constants).  A P or T step is hoisted when it is the only writer of everything it writes and everything it
    // reads is a constant, a graph input or the product of hoisted steps.  Everything a hoisted step writes moves out of the arena (which recycles by
    // step index within ONE pass) into an allocation of its own; the captured passes are then recorded anew on the new addresses.
    // P steps run eagerly once per loop call, before step 0.  T steps run on a miss of the row table: a row = the T values the per-step part reads,
    // for one timestep value (keyed by the bits of t); a hit is one osg_copy per such value.
    enum : char { CLS_STEP = 0, CLS_P = 1, CLS_T = 2 };
    struct HoistLive { int val; size_t bytes, off; };           // a root val T steps write and others read: `off` inside a row
    struct Hoist {
        bool ready = false;
        std::string sample, timestep;
        std::vector<char> cls;                // per step, hoisted steps only: CLS_P / CLS_T, everything else CLS_STEP
        size_t n_p = 0, n_t = 0;
        std::vector<int> moved;               // the root vals that got their own allocation
        std::vector<HoistLive> live;
        size_t row_bytes = 0, extra_bytes = 0;
        bool epoch_keyed = false;             // T reads something besides the timestep and constants: rows are valid for one input epoch only
        char* table = nullptr;
        long cap = 0;
        std::vector<uint32_t> keys;           // keys[r]: bit pattern of t of filled row r
        unsigned long long table_epoch = 0, schedule_seen = 0;
        void* tvals = nullptr;                // the schedule's timestep broadcasts [n][N * TL] fp32, device (what fills rows ahead of step 0)
        size_t tvals_bytes = 0;
        unsigned long long hits = 0, misses = 0;   // of the last loop call
    };
    Hoist hoist;
    bool loop_hoist = true;        // ConstPool::LoopOptions as they were when the plan was built
    long loop_hoist_rows = 64;
    // the Model's loop options (created with its pool on first use), and what the exports make of them: the schedule call, out[0..7] = launches of the
    // per-step graph, hoisted prompt-only steps, hoisted timestep-only steps, device bytes the hoist added, table hits and misses of the last loop call,
    // the input epoch, filled table rows (all 0 before the first loop call and with the option off, but the epoch), and hoist_info() of the Model's plan.
    // Static members of Plan for the reason given at on_plan_of
    static ConstPool::LoopOptions& loop_options(Model& m);
    static ConstPool::PlanOptions& plan_options(Model& m);
    static void sampler_schedule(Model& m, const float* t, size_t n);
    static void loop_hoist_stats(Model& m, unsigned long long out[8]);
    static std::string loop_hoist_info(Model& m);
    osg_graph* step_graph = nullptr;          // the per-step class alone; what sampler_frame launches once the hoist is ready
    unsigned long long input_epoch = 0;       // bumped by every upload of an input other than the loop's sample / timestep
    void drop_graphs();
    osg_graph* capture(int cls);              // record run_steps(dyn_end, end, cls) into a new graph
    void hoist_prepare(const SamplerIO& io, const std::string& sample_name, const std::string& timestep_name);
    void hoist_fill_row(const float* tstep_src, float t, float* tstep, size_t tbytes);
    long hoist_find(float t) const;
    std::string hoist_info() const;           // "hoist P|T step <i> | <what>", "hoist val <id> ptr=.. bytes=..", "hoist live ..", table / epoch state
    Lowering* lowering = nullptr;  // kept alive: the launch closures capture it
    int runs = 0;
    bool in_capture = false;      // run_steps() is recording the hipGraph (no synchronisation allowed inside)
    double m_last_ms = 0;
    // options the plan was built with
    bool fp16 = true;
    bool u8_qdq = false, autotune = false, calibrate = false, fuse_attn = false, sdp_attn = false;
    std::set<std::string> outputs_convert_set;
    bool u8 = false;               // m_use_uint8_arithmetic: uint8 activations (the reference's W8A8 path, VAE decoder)
    bool stream_weights = false;
    bool fuse_ln_gemm = false;
    bool concat_views = true;     // m_hip_concat_views
    bool fuse_tblock = true;      // m_hip_fuse_tblock
    bool fuse_shortcut = false;   // hip_fuse_shortcut (ConstPool::PlanOptions)
    bool in_flight = false;       // a pass of this plan may still be running on the device (set while execute() / replay() are between enqueue and wait)
    bool gn_stats_on = false;
    int gn_stats_req = 2;          // m_hip_gn_stats as requested (0 off, 1 all eligible, 2 large tensors only)
    long gn_stats_min_elems = 0;   // m_hip_gn_stats: GroupNorm statistics from the producing convolutions' epilogues (plan.cpp lower_group_norm)
    char* gn_stats = nullptr;      // the pass's statistics block: one [N][G][2] int64 table per such GroupNorm, zeroed at the start of every pass
    size_t gn_stats_bytes = 0;
    void zero_gn_stats();
    // steps [begin, end); cls >= 0: only the steps of that hoist class (the GroupNorm statistics are zeroed with the per-step class)
    void run_steps(size_t begin = 0, size_t end = (size_t)-1, int cls = -1);
    // uint8 plans: steps [0, dyn_end) read values quantised per run (a pushed input and what merely re-arranges its codes): they run eagerly every
    // pass with the parameters of that pass, the steps after them only see range-data parameters and are captured like any other plan
    size_t dyn_end = 0;
    bool w8_resident = false;      // uint8 Conv/MatMul/Gemm weights kept as codes, dequantised inside the kernels (osg_*_w8)   // m_hip_stream_weights: weights are re-pulled from the WeightsProvider and re-streamed H2D every pass
    int fusion = 2;
    int fusion_req = 2;            // m_hip_fusion_level as the Model had it when the plan was built (build() lowers `fusion` to 0 for uint8 / calibration plans:
                                   // compatible() compares the REQUEST -- comparing the effective level re-planned every uint8 call, round 3)
    std::vector<std::string> extra_outputs;

    // ---- helpers used by the lowering code (plan.cpp) ----
    int new_val(const std::string& name, const std::vector<long>& shape, osg_dtype dt, Lay lay, bool batched);
    int alias(int v, const std::vector<long>& shape, Lay lay, const std::string& name = "");
    int root_of(int v) const;
    void* ptr(int v) const;
    size_t val_bytes(int v) const;
    long total_elems(int v) const;
    void add_step(const std::string& what, std::vector<int> reads, std::vector<int> writes, std::function<void()> fn);
    const Val& qv(int v) const;    // the val holding v's quantisation parameters
    void share_q(int dst, int src); // dst carries src's quantisation parameters
    void own_q(int v, float scale, int zp);   // v (an alias) gets fixed parameters of its own
    int ensure_plain(int v);
    int ensure_nhwc(int v);
    // a device constant that survives this plan (ConstPool::derived) -- *fresh tells the caller to fill it; plan-owned (always fresh) in
    // streamed-weights mode or with an empty tag
    void* const_alloc(const std::string& tag, size_t bytes, bool* fresh);
    int ensure_dense(int v);   // materialise a strided column view as a dense tensor (for consumers that cannot take a leading dimension)
};

}  // namespace onnxstream
