// plan_run.cpp -- the RUN-TIME half of Plan (round 6: split out of plan.cpp, which keeps construction, fusion and lowering): replaying the steps eagerly or as a
// captured hipGraph, input upload / output download, weight re-streaming under a VRAM budget, the device sampler loop, the per-step profile.  The LLM calls
// (the device token loop, the chat turn) stand on run_pass() and live in plan_llm.cpp.
#include "plan.h"
#include "qu8.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <string_view>
#include <unordered_map>
#include <unordered_set>

namespace onnxstream {

// the producers' epilogues ADD to the statistics tables of the GroupNorms that read them (lower_group_norm): a pass starts from zero
void Plan::zero_gn_stats() {
    if (gn_stats_bytes) be.check(be.api.osg_memset(be.ctx, gn_stats, 0, gn_stats_bytes), "osg_memset");
}

void Plan::run_steps(size_t begin, size_t end, int cls) {
    // measurement aid (tools/skip_probe.sh): OSG_PLAN_SKIP=<prefix>[,<prefix>...] leaves out every step whose description starts with one of
    // the prefixes -- the pass computes garbage, its captured-graph time shows what that class of launches really costs inside the chain
    static const std::vector<std::string> skip = [] {
        std::vector<std::string> v;
        if (const char* e = std::getenv("OSG_PLAN_SKIP")) {
            std::string t = e;
            size_t b0 = 0;
            while (b0 <= t.size()) {
                size_t e0 = t.find(',', b0);
                if (e0 == std::string::npos) e0 = t.size();
                if (e0 > b0) v.push_back(t.substr(b0, e0 - b0));
                b0 = e0 + 1;
            }
        }
        return v;
    }();
    end = std::min(end, steps.size());
    if (begin == 0 && cls <= CLS_STEP) zero_gn_stats();
    for (size_t si_ = begin; si_ < end; si_++) {
        if (cls >= 0 && hoist.cls[si_] != cls) continue;
        Step& s = steps[si_];
        if (!skip.empty()) {
            bool sk = false;
            for (auto& pre : skip) sk |= s.what.rfind(pre, 0) == 0;
            if (sk) continue;
        }
        static const bool roctx_on = std::getenv("OSG_ROCTX") != nullptr;
        struct Range {
            HipBackend& b; bool on;
            Range(HipBackend& b_, bool on_, const char* n) : b(b_), on(on_) { if (on) b.api.osg_range_push(n); }
            ~Range() { if (on) b.api.osg_range_pop(); }
        } range(be, roctx_on, s.what.c_str());
        s.run();
        // measurement aid (round 6): OSG_PROBE_EXTRA_TRIVIAL=<k> puts k trivial launches (a 4-element convert on a private buffer) behind EVERY
        // step of the pass -- eager, captured and replayed alike: (replayed pass time with k) - (without) over k x steps = what a trivial node costs INSIDE this pass
        static const int extra_trivial = std::getenv("OSG_PROBE_EXTRA_TRIVIAL") ? atoi(std::getenv("OSG_PROBE_EXTRA_TRIVIAL")) : 0;
        if (extra_trivial > 0) {
            static void* probe = nullptr;          // (first used in the eager first pass: never allocated inside a capture; a process-lifetime 4 KiB)
            if (!probe) be.check(be.api.osg_malloc(be.ctx, 4096, &probe), "osg_malloc");
            for (int k = 0; k < extra_trivial; k++)
                be.check(be.api.osg_convert(be.ctx, OSG_F32, OSG_F16, probe, (char*)probe + 2048, 4, 1.0f, 0), "osg_convert");
        }
        // OSG_PLAN_TRACE=1 (debugging aid, eager passes only): name every step on stderr and wait for it -- a device fault then points at its launch
        static const bool trace = std::getenv("OSG_PLAN_TRACE") != nullptr;
        if (trace && !in_capture) {
            fprintf(stderr, "[step] %s\n", s.what.c_str());
            be.check(be.api.osg_sync(be.ctx), "osg_sync");
        }
    }
}

void Plan::execute(const std::function<void()>& while_device_runs) {
    // ---- m_hip_resident_outputs: the buffers of the previous execute() of THIS plan now belong to the Tensors it published (or to copies the caller
    // kept): a plan that runs again writes into buffers of its own.  (advisor, round 2: the second execute() of a compatible plan overwrote the
    // buffer the first call's Tensor owned.)  The launch closures read ptr() at run time; a captured graph has the old addresses baked in and is dropped.
    {
        bool moved = false;
        for (auto& o : outputs)
            if (o.dev_bytes && !o.dev) {
                o.dev = pool.take_class(be, ConstPool::size_class(o.dev_bytes));
                vals[o.f32val].dptr = o.dev;
                moved = true;
            }
        if (moved) drop_graphs();
    }
    static const bool exec_times = getenv("OSG_EXEC_TIMES") != nullptr;    // developer probe: host milliseconds of the phases of this call, to stderr
    const auto t_exec = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    double ms_stage = 0, ms_enqueue = 0, ms_wait = 0;
    // ---- stage the inputs (host fp32, N samples stacked) -------------------------------------------------------------
    // Many small fp16 inputs (the LLM flow feeds 2 x layers key/value caches back every call) go up in ONE transfer when their device buffers are
    // neighbours in a small-allocation slab (they are carved out one after the other): gathered into a host block with the device's own spacing.
    char* up_lo = nullptr;
    char* up_hi = nullptr;
    {
        size_t sum = 0, cnt = 0;
        for (auto& in : inputs) {
            if (in.host_type != TensorDataType::float16 || vals[in.staging].numel() == 0 || in.resident) continue;
            char* p = (char*)ptr(in.val);
            const size_t nb = val_bytes(in.val);
            if (!up_lo || p < up_lo) up_lo = p;
            if (!up_hi || p + nb > up_hi) up_hi = p + nb;
            sum += (nb + 255) & ~(size_t)255;   // (what small_alloc hands out)
            cnt++;
        }
        // only a gap-free run inside ONE slab qualifies: nothing else may live in the range that is overwritten
        if (cnt < 4 || (size_t)(up_hi - up_lo) > sum || !in_one_slab(up_lo, up_hi)) up_lo = up_hi = nullptr;
        else io_block.assign((size_t)(up_hi - up_lo), 0);
    }
    bool new_epoch = false;
    for (auto& in : inputs) {
        Tensor* src = nullptr;
        for (auto& t : m.m_data)
            if (t.m_name == in.name) { src = &t; break; }
        if (!src) throw std::invalid_argument("Model::get_tensor_data: input tensor not found: " + in.name);
        if (src->m_type != in.host_type || src->m_shape != in.shape)
            throw std::invalid_argument("Model::run: input '" + in.name + "' changed type or shape since the plan was built.");
        if (!(hoist.ready && (in.name == hoist.sample || in.name == hoist.timestep))) new_epoch = true;   // (what the timestep rows may have been computed from)
        if (in.host_type == TensorDataType::int64 || vals[in.staging].numel() == 0) continue;   // plan-time value / empty tensor: nothing to stage
        if (in.resident) {   // on the device already; the tensor must still be the one the plan was built on
            if (src->m_hip_resident != in.resident) throw std::invalid_argument("Model::run: input '" + in.name + "' changed since the plan was built.");
            continue;
        }
        if (in.host_type == TensorDataType::float16) {
            if (src->m_hip_resident) throw std::invalid_argument("Model::run: input '" + in.name + "' changed since the plan was built.");
            auto& vec = src->get_vector<uint16_t>();
            if (vec.size() != (size_t)vals[in.val].numel()) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
            if (up_lo) std::memcpy(io_block.data() + ((char*)ptr(in.val) - up_lo), vec.data(), vec.size() * 2);
            else be.check(be.api.osg_upload(be.ctx, ptr(in.val), vec.data(), vec.size() * 2), "osg_upload");
            continue;
        }
        const size_t per = vals[in.staging].numel() * sizeof(float);
        auto upload = [&](Tensor& t, long idx) {
            auto& vec = t.get_vector<float>();
            if (vec.size() * sizeof(float) != per) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
            if (u8) {
                std::vector<uint8_t> codes(vec.size());
                qu8::QParams qp;
                if (!qu8::quantize_dynamic(vec.data(), vec.size(), m.m_threads, codes.data(), &qp))
                    throw std::invalid_argument("Model::quantize: unable to compute the percentiles of input '" + in.name + "'.");
                vals[in.val].qscale = qp.scale;
                vals[in.val].qzp = (int)qp.zero_point;
                be.check(be.api.osg_upload(be.ctx, ptr(in.val), codes.data(), codes.size()), "osg_upload");
                return;
            }
            be.check(be.api.osg_upload(be.ctx, (char*)ptr(in.staging) + idx * per, vec.data(), per), "osg_upload");
        };
        upload(*src, 0);
        const long extra = src->m_batch ? (long)src->m_batch->size() : 0;
        if (extra + 1 != N) throw std::invalid_argument("Model::run: inconsistent m_batch.size() across two or more tensors.");
        for (long i = 0; i < extra; i++) upload((*src->m_batch)[i], i + 1);
    }
    if (new_epoch) input_epoch++;
    gathered_up = up_lo ? io_block.size() : 0;
    if (up_lo) be.check(be.api.osg_upload(be.ctx, up_lo, io_block.data(), io_block.size()), "osg_upload");
    ms_stage = ms_since(t_exec);
    in_flight = true;
    // ---- run the pass -------------------------------------------------------------------------------------------------
    const bool stream_pass = stream_weights && (runs >= 1 || budgeted);
    if (m.m_ops_times_printf && stream_pass)
        throw std::invalid_argument("Model::run: m_ops_times_printf is not available with streamed weights (hip_stream_weights / a VRAM budget) on the HIP backend.");
    const bool times = m.m_ops_times_printf && !calibrate && !stream_pass;
    if (!times) be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
    const bool print = m.m_ops_printf;
    float times_total = 0;
    if (times) {
        // m_ops_times_printf (reference :3810-3815, :8199-8214: wall milliseconds per op TYPE, printed after the last op of the pass): here the
        // DEVICE milliseconds (HIP events on the compute stream) of the launches each graph op type was lowered to, eager pass, same line format
        std::map<std::string, double> per_type;
        int idx = 0;
        zero_gn_stats();
        for (auto& s : steps) {
            if (print) printf("#%i) %s\n", idx++, s.what.c_str());
            be.api.osg_range_push(s.what.c_str());
            be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
            s.run();
            float ms1 = 0;
            be.check(be.api.osg_timer_stop(be.ctx, &ms1), "osg_timer_stop");
            be.api.osg_range_pop();
            std::string ty = s.what.substr(0, s.what.find(' '));
            const size_t plus = ty.find('+');
            if (plus != std::string::npos) ty = ty.substr(0, plus);
            per_type[ty] += ms1;
            times_total += ms1;
        }
        printf("\033[7m > \033[0m");
        for (auto& e : per_type) printf(" %s:%f,", e.first.c_str(), e.second);
        printf("\n");
        fflush(stdout);
    } else
    if (stream_pass) {
        if (budgeted && runs == 0) m.get_wp()->on_restart();   // the plan build pulled the whole sequence once; the first pass pulls it again
        // ---- streamed-weights pass: every weight is pulled from the provider again, in model order, and sent H2D on the COPY stream
        // (pinned double-buffered staging, or straight out of a RAM provider's page-locked buffer) while the compute stream works on
        // the previous steps; a step is launched right after the uploads of ITS weights were enqueued (the compute stream waits on
        // their events), so upload(i+1) overlaps compute(i).  No hipGraph: host-side copies interleave with the launches.
        streamed_bytes = 0;
        size_t ri = 0;
        ring_occ.clear();
        ring_head = 0;
        for (size_t si = 0; si < steps.size(); si++) {
            cur_step = (int)si;
            while (ri < flush_upto[si]) restream(recipes[ri++]);
            be.check(be.api.osg_copy_fence(be.ctx), "osg_copy_fence");
            steps[si].run();
            // ring occupants whose last reader has just been enqueued: mark the compute stream here, the slot may be overwritten after it
            for (auto& o : ring_occ)
                if (o.marker < 0 && o.last <= (int)si) {
                    o.marker = next_marker;
                    next_marker = (next_marker + 1) % 256;
                    be.check(be.api.osg_marker_record(be.ctx, o.marker), "osg_marker_record");
                }
        }
        cur_step = (int)steps.size();
        while (ri < recipes.size()) restream(recipes[ri++]);   // keep the provider's sequence complete
    } else
    if (graph && !print && !calibrate) {
        if (dyn_end) run_steps(0, dyn_end);
        be.check(be.api.osg_graph_launch(be.ctx, graph), "osg_graph_launch");
    } else if (runs >= 1 && m.m_hip_use_graph && !print && !graph && !calibrate) {
        // (uint8 plans: the steps that read per-run quantisation parameters run eagerly first, see dyn_end; the rest is captured)
        if (dyn_end) run_steps(0, dyn_end);
        graph = capture(-1);
        be.check(be.api.osg_graph_launch(be.ctx, graph), "osg_graph_launch");
    } else if (calibrate) {
        // Model::push_tensor's calibration hook (reference :2983-3003): the 0.1 % percentiles of every tensor an op pushes widen the range
        // recorded under the OP's name.  The tensors live on the device: each is read back right after its producer (the arena recycles
        // it later) and measured by the host restatement of get_percentiles (qu8.h), chunked by the Model's thread count like the reference's.
        size_t ci = 0;
        std::vector<uint16_t> h16;
        std::vector<float> h32;
        static const std::vector<float> half_table = [] {
            std::vector<float> t(65536);
            for (unsigned k = 0; k < 65536; k++) t[k] = half_to_float((uint16_t)k);
            return t;
        }();
        const size_t workers = std::max(1u, std::thread::hardware_concurrency());
        for (size_t si = 0; si < steps.size(); si++) {
            steps[si].run();
            for (; ci < calib.size() && calib[ci].step <= (int)si; ci++) {
                const Calib& c = calib[ci];
                const size_t n = (size_t)total_elems(c.val);
                h16.resize(n);
                h32.resize(n);
                be.check(be.api.osg_download(be.ctx, h16.data(), ptr(c.val), n * 2), "osg_download");
                for (size_t k = 0; k < n; k++) h32[k] = half_table[h16[k]];
                auto r = qu8::percentiles_fast(h32.data(), n, 0.001f, 0.001f, m.m_threads, workers);
                if (!r) continue;
                auto it = m.m_range_data.find(c.op);
                if (it == m.m_range_data.end()) m.m_range_data[c.op] = *r;
                else {
                    if (r->first < it->second.first) it->second.first = r->first;
                    if (r->second > it->second.second) it->second.second = r->second;
                }
            }
        }
    } else if (!print) {
        run_steps();
    } else {
        int idx = 0;
        zero_gn_stats();
        for (auto& s : steps) {
            printf("#%i) %s\n", idx++, s.what.c_str());
            be.api.osg_range_push(s.what.c_str());
            s.run();
            be.api.osg_range_pop();
        }
    }
    float ms = times_total;
    ms_enqueue = ms_since(t_exec);
    if (while_device_runs) while_device_runs();
    if (!times) be.check(be.api.osg_timer_stop(be.ctx, &ms), "osg_timer_stop");
    in_flight = false;
    ms_wait = ms_since(t_exec);
    m_last_ms = ms;
    runs++;
    // ---- consume the inputs, publish the outputs as fp32 host tensors in the logical (NCHW) layout (reference :8217-8263) --
    for (auto& in : inputs)
        for (size_t i = 0; i < m.m_data.size(); i++)
            if (m.m_data[i].m_name == in.name) { m.m_data.erase(m.m_data.begin() + i); break; }
    // ... the same for many small outputs (the new caches): one transfer of the slab range that holds their staging buffers, split on the host
    char* dn_lo = nullptr;
    char* dn_hi = nullptr;
    if (outputs.size() >= 4) {
        size_t sum = 0;
        for (auto& o : outputs) {
            if (o.dev) continue;
            char* p = (char*)ptr(o.f32val);
            const size_t nb = val_bytes(o.f32val);   // (all N samples)
            if (!dn_lo || p < dn_lo) dn_lo = p;
            if (!dn_hi || p + nb > dn_hi) dn_hi = p + nb;
            sum += (nb + 255) & ~(size_t)255;
        }
        if ((size_t)(dn_hi - dn_lo) > sum || !in_one_slab(dn_lo, dn_hi)) dn_lo = dn_hi = nullptr;
        else {
            io_block.resize((size_t)(dn_hi - dn_lo));
            be.check(be.api.osg_download(be.ctx, io_block.data(), dn_lo, io_block.size()), "osg_download");
        }
    }
    gathered_down = dn_lo ? io_block.size() : 0;
    auto fetch = [&](void* host, const char* dev, size_t bytes) {
        if (dn_lo) std::memcpy(host, io_block.data() + (dev - dn_lo), bytes);
        else be.check(be.api.osg_download(be.ctx, host, dev, bytes), "osg_download");
    };
    for (auto& o : outputs) {
        if (o.dev) {
            // m_hip_resident_outputs: the Tensor in m_data owns the device buffer from here on
            Tensor t = resident_tensor(m, o.name, o.shape, o.dev, o.dev_bytes);
            o.dev = nullptr;
            for (size_t i = 0; i < m.m_data.size(); i++)
                if (m.m_data[i].m_name == o.name) { m.m_data.erase(m.m_data.begin() + i); break; }
            m.m_data.push_back(std::move(t));
            continue;
        }
        const size_t per_elems = (size_t)vals[o.f32val].numel();
        const long nb = vals[o.f32val].batched ? N : 1;
        Tensor first;
        for (long i = 0; i < nb; i++) {
            Tensor t;
            t.m_name = o.name;
            t.m_shape = o.shape;
            if (o.raw16) {
                tensor_vector<uint16_t> host(per_elems);
                fetch(host.data(), (char*)ptr(o.f32val) + i * per_elems * 2, per_elems * 2);
                t.set_vector(std::move(host));
            } else {
                tensor_vector<float> host(per_elems);
                fetch(host.data(), (char*)ptr(o.f32val) + i * per_elems * sizeof(float), per_elems * sizeof(float));
                t.set_vector(std::move(host));
            }
            if (i == 0) first = std::move(t);
            else {
                if (!first.m_batch) first.m_batch = std::make_shared<std::vector<Tensor>>();
                first.m_batch->push_back(std::move(t));
            }
        }
        for (size_t i = 0; i < m.m_data.size(); i++)
            if (m.m_data[i].m_name == o.name) { m.m_data.erase(m.m_data.begin() + i); break; }
        m.m_data.push_back(std::move(first));
    }
    if (exec_times)
        fprintf(stderr, "[exec] inputs staged %.3f ms, pass enqueued +%.3f, device done +%.3f (device %.3f), outputs published +%.3f\n", ms_stage, ms_enqueue - ms_stage,
                ms_wait - ms_enqueue, (double)m_last_ms, ms_since(t_exec) - ms_wait);
}

void Plan::restream(const WRecipe& r) {
    WeightsProvider* wp = m.get_wp();
    detail::dispatch_dtype(r.ty, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const size_t bytes = (size_t)r.count * sizeof(T);
        auto send = [&](const T* host, bool stable) {
            if (r.val < 0 || r.resident) return;        // fetched to keep the provider's sequence; already on the device
            if (r.ring) {
                if (vals[r.val].last < 0) return;       // nobody reads it in this plan
                // FIFO slot in the ring; whatever it overlaps must have been read by launches that are at least enqueued (else the ring
                // is too small for one step's weights) and the COPY stream waits for those launches before it overwrites them
                const size_t need = (bytes + 255) & ~(size_t)255;
                if (need > ring_bytes) throw std::runtime_error("Model::run: a weight is larger than the VRAM streaming ring.");
                if (ring_head + need > ring_bytes) ring_head = 0;
                for (size_t k = 0; k < ring_occ.size();) {
                    RingOcc& o = ring_occ[k];
                    if (o.off < ring_head + need && ring_head < o.off + o.size) {
                        if (o.last >= cur_step) throw std::runtime_error("Model::run: the VRAM budget leaves no room for the weights one step reads (raise m_vram_to_use).");
                        if (o.marker >= 0) be.check(be.api.osg_copy_wait_marker(be.ctx, o.marker), "osg_copy_wait_marker");
                        ring_occ.erase(ring_occ.begin() + k);
                    } else
                        k++;
                }
                vals[r.val].dptr = (char*)ring + ring_head;
                ring_occ.push_back(RingOcc{ring_head, need, vals[r.val].last, -1});
                ring_head += need;
            }
            void* dst = r.raw ? r.raw : vals[r.val].dptr;
            if (stable) {   // provider-owned memory that outlives the pass: page-lock once, DMA without a staging copy
                auto it = registered.find(host);
                if (it == registered.end()) {
                    be.check(be.api.osg_host_register(be.ctx, (void*)host, bytes), "osg_host_register");
                    registered[host] = bytes;
                }
                be.check(be.api.osg_upload_pinned_async(be.ctx, dst, host, bytes), "osg_upload_pinned_async");   // (fenced once per step, Plan::execute)
                if (r.raw) be.check(be.api.osg_copy_fence(be.ctx), "osg_copy_fence");
            } else {
                be.check(be.api.osg_upload(be.ctx, dst, host, bytes), "osg_upload");
            }
            if (r.raw) be.check(be.api.osg_convert(be.ctx, r.have, r.want, r.raw, vals[r.val].dptr, r.count, r.scale, r.zp), "osg_convert");
            streamed_bytes += bytes;
        };
        if (wp->supports_getptr()) {
            std::shared_ptr<tensor_vector<T>> sp;
            if constexpr (std::is_same_v<T, uint8_t>) sp = wp->getptr_uint8(r.fn);
            else if constexpr (std::is_same_v<T, uint16_t>) sp = wp->getptr_float16(r.fn);
            else if constexpr (std::is_same_v<T, float>) sp = wp->getptr_float32(r.fn);
            else sp = wp->getptr_int64(r.fn);
            if (r.val >= 0 && (long)sp->size() != r.count) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
            send(sp->data(), true);
        } else {
            tensor_vector<T> data;
            if constexpr (std::is_same_v<T, uint8_t>) data = wp->get_uint8(r.fn);
            else if constexpr (std::is_same_v<T, uint16_t>) data = wp->get_float16(r.fn);
            else if constexpr (std::is_same_v<T, float>) data = wp->get_float32(r.fn);
            else data = wp->get_int64(r.fn);
            if (r.val >= 0 && (long)data.size() != r.count) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
            send(data.data(), false);   // osg_upload copies into pinned staging before returning: `data` may die here
        }
    });
}

void Plan::replay(int n, float* ms_each) {
    if (!graph) throw std::runtime_error("Model::hip_replay: no captured pass yet (run() at least twice with hip_use_graph on).");
    FlightGuard flight(in_flight);
    if (!ms_each) {  // back-to-back launches, one event pair around all of them
        be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
        for (int i = 0; i < n; i++) be.check(be.api.osg_graph_launch(be.ctx, graph), "osg_graph_launch");
        float ms = 0;
        be.check(be.api.osg_timer_stop(be.ctx, &ms), "osg_timer_stop");
        m_last_ms = n > 0 ? ms / n : 0;
        return;
    }
    for (int i = 0; i < n; i++) {
        be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
        be.check(be.api.osg_graph_launch(be.ctx, graph), "osg_graph_launch");
        float ms = 0;
        be.check(be.api.osg_timer_stop(be.ctx, &ms), "osg_timer_stop");
        ms_each[i] = ms;
        m_last_ms = ms;
    }
}

void Plan::set_input(const std::string& name, long index, const float* data, size_t count) {
    if (u8) throw std::runtime_error("Model::hip_set_input: not available with uint8 arithmetic (inputs are quantised per run).");
    for (auto& in : inputs)
        if (in.name == name) {
            const size_t per = (size_t)vals[in.staging].numel();
            if (count != per) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
            if (index < 0 || index >= N) throw std::invalid_argument("Model::hip_set_input: sample index out of range.");
            be.check(be.api.osg_upload(be.ctx, (char*)ptr(in.staging) + index * per * sizeof(float), data, per * sizeof(float)), "osg_upload");
            if (!(hoist.ready && (name == hoist.sample || name == hoist.timestep))) input_epoch++;
            return;
        }
    throw std::invalid_argument("Model::get_tensor_data: input tensor not found: " + name);
}

// what the sampler loops check (sampler_check_state) and look up (sampler_io) before they enqueue anything; `fn` is the "Model::hip_sampler_loop...: " prefix
// of the caller's error texts.  branches: see plan.h.
void Plan::sampler_check_state(const std::string& fn, int prompts, int branches) const {
    if (runs < 1) throw std::runtime_error(fn + "run() once first (the context inputs must be resident).");
    if (stream_weights) throw std::runtime_error(fn + "not available in streamed-weights mode.");
    if (u8) throw std::runtime_error(fn + "not available with uint8 arithmetic.");
    if (branches == 2 && (prompts <= 0 || 2L * prompts != N))
        throw std::invalid_argument(fn + "the plan's batch must be 2 * prompts (cond, uncond per prompt).");
    if (branches != 2 && (prompts <= 0 || (long)prompts != N))
        throw std::invalid_argument(fn + "the plan's batch must be prompts (one sample per prompt: this loop runs no guidance pair).");
}

Plan::SamplerIO Plan::sampler_io(const std::string& fn, const std::string& sample_name, const std::string& timestep_name,
                                 const std::string& out_name) const {
    SamplerIO io;
    for (auto& in : inputs) {
        if (in.name == sample_name) io.in_s = &in;
        if (in.name == timestep_name) io.in_t = &in;
    }
    for (auto& o : outputs)
        if (o.name == out_name) io.out = &o;
    if (!io.in_s || !io.in_t || !io.out) throw std::invalid_argument(fn + "input/output tensor not found.");
    if (io.out->raw16) throw std::invalid_argument(fn + "the output is excluded from the fp32 conversion (m_outputs_convert_set).");
    io.L = vals[io.in_s->staging].numel();
    io.TL = vals[io.in_t->staging].numel();
    if (vals[io.out->f32val].numel() != io.L || !vals[io.out->f32val].batched)
        throw std::invalid_argument(fn + "the output must have the shape of the sample input.");
    return io;
}

void Plan::grow_buffer(void*& p, size_t& have, size_t need) {
    if (have >= need) return;
    if (p) be.check(be.api.osg_free(be.ctx, p), "osg_free");
    p = nullptr;
    have = 0;
    be.check(be.api.osg_malloc(be.ctx, need, &p), "osg_malloc");
    have = need;
}

// ---- loop hoist (plan.h: Plan::Hoist) ------------------------------------------------------------------------------------------------------------------
void Plan::drop_graphs() {
    if (graph) be.api.osg_graph_destroy(graph);
    if (step_graph) be.api.osg_graph_destroy(step_graph);
    graph = step_graph = nullptr;
}

osg_graph* Plan::capture(int cls) {
    be.check(be.api.osg_graph_begin(be.ctx), "osg_graph_begin");
    in_capture = true;
    osg_graph* g = nullptr;
    try {
        run_steps(dyn_end, (size_t)-1, cls);
        in_capture = false;
    } catch (...) {
        in_capture = false;
        be.api.osg_graph_end(be.ctx, &g);
        if (g) be.api.osg_graph_destroy(g);
        throw;
    }
    be.check(be.api.osg_graph_end(be.ctx, &g), "osg_graph_end");
    return g;
}

// one pass of a resident LLM plan (the token loop, the prefill loop): eager the first time, captured the second, replayed from then on.  With m_hip_use_graph
// off every pass is eager, a graph an earlier call captured included: it stays for the call that switches the option on again
void Plan::run_pass() {
    const bool use_graph = m.m_hip_use_graph;
    if (!graph && use_graph && runs >= 1) graph = capture(-1);
    if (graph && use_graph) be.check(be.api.osg_graph_launch(be.ctx, graph), "osg_graph_launch");
    else run_steps();
    runs++;
}

// Classify the steps for the loop's (sample, timestep) pair, give what the hoisted ones write a home outside the arena and record the passes anew.  Runs
// on the first loop call (and again should a later call name other inputs); nothing is enqueued, the plan's passes have all been waited for.
void Plan::hoist_prepare(const SamplerIO& io, const std::string& sample_name, const std::string& timestep_name) {
    if (!loop_hoist || (hoist.ready && hoist.sample == sample_name && hoist.timestep == timestep_name)) return;
    Hoist& h = hoist;
    const int rs = root_of(io.in_s->staging), rt = root_of(io.in_t->staging);
    std::vector<char> taint(vals.size(), 0), home(vals.size(), 0);      // home[r]: the class of the hoisted step that writes root r
    std::vector<int> writers(vals.size(), 0);
    taint[rs] |= 1;
    taint[rt] |= 2;
    for (auto& s : steps) {
        std::set<int> ws;
        for (int w : s.writes)
            if (w >= 0) ws.insert(root_of(w));
        for (int w : ws) writers[w]++;
    }
    std::set<int> out_vals;
    for (auto& o : outputs) out_vals.insert(root_of(o.f32val));
    h.cls.assign(steps.size(), CLS_STEP);
    h.n_p = h.n_t = 0;
    for (size_t si = 0; si < steps.size(); si++) {
        const Step& s = steps[si];
        char bits = 0;
        for (int r : s.reads)
            if (r >= 0) bits |= taint[root_of(r)];
        for (int w : s.writes)
            if (w >= 0) taint[root_of(w)] |= bits;
        if ((bits & 1) || s.side || s.writes.empty() || si < dyn_end) continue;
        const char c = (bits & 2) ? CLS_T : CLS_P;
        bool ok = true;
        for (int w : s.writes) {
            if (w < 0) continue;
            const int r = root_of(w);
            ok = ok && writers[r] == 1 && !vals[r].is_const && !vals[r].host_only && val_bytes(r) > 0;
        }
        for (int v : s.reads) {
            if (v < 0) continue;
            const int r = root_of(v);
            // a constant, a graph input (nothing writes it), or what a hoisted step leaves in a buffer of its own: never a value the per-step part computes
            ok = ok && (vals[r].is_const || vals[r].host_only || writers[r] == 0 || home[r] != 0);
        }
        if (!ok) continue;
        h.cls[si] = c;
        (c == CLS_T ? h.n_t : h.n_p)++;
        for (int w : s.writes)
            if (w >= 0) home[root_of(w)] = c;
    }
    // out of the arena: its packing lets a later step of the SAME pass reuse the bytes, a hoisted value must outlive the pass
    auto aligned = [](size_t b) { return (b + 255) & ~(size_t)255; };
    for (size_t r = 0; r < vals.size(); r++)
        if (home[r] && vals[r].root < 0 && !vals[r].dptr) {
            vals[r].dptr = small_alloc(val_bytes((int)r));
            vals[r].pinned = true;
            h.moved.push_back((int)r);
            h.extra_bytes += aligned(val_bytes((int)r));
        }
    // a row of the table: what T steps write and anything else reads
    h.live.clear();
    h.row_bytes = 0;
    h.epoch_keyed = false;
    std::vector<char> live(vals.size(), 0);
    for (size_t si = 0; si < steps.size(); si++)
        for (int v : steps[si].reads) {
            if (v < 0) continue;
            const int r = root_of(v);
            if (h.cls[si] != CLS_T && home[r] == CLS_T) live[r] = 1;
            if (h.cls[si] == CLS_T && r != rt && !vals[r].is_const && !vals[r].host_only && home[r] != CLS_T) h.epoch_keyed = true;
        }
    for (int r : out_vals)
        if (home[r] == CLS_T) live[r] = 1;
    for (size_t r = 0; r < vals.size(); r++)
        if (live[r]) {
            h.live.push_back(HoistLive{(int)r, val_bytes((int)r), h.row_bytes});
            h.row_bytes += aligned(val_bytes((int)r));
        }
    h.keys.clear();
    h.cap = std::max(0L, std::min(64L, loop_hoist_rows));
    h.table = nullptr;
    if (h.row_bytes && h.cap) {
        h.table = (char*)be.malloc(h.row_bytes * (size_t)h.cap);
        owned.push_back(h.table);
        h.extra_bytes += h.row_bytes * (size_t)h.cap;
    } else
        h.cap = 0;
    h.table_epoch = input_epoch;
    h.schedule_seen = 0;
    h.sample = sample_name;
    h.timestep = timestep_name;
    h.ready = true;
    // the recorded passes hold the old addresses
    const bool had = graph != nullptr;
    drop_graphs();
    if (had) graph = capture(-1);
}

ConstPool::LoopOptions& Plan::loop_options(Model& m) {
    if (!m.m_pool) m.m_pool = new ConstPool();
    return m.m_pool->loop;
}

ConstPool::PlanOptions& Plan::plan_options(Model& m) {
    if (!m.m_pool) m.m_pool = new ConstPool();
    return m.m_pool->opts;
}

void Plan::sampler_schedule(Model& m, const float* t, size_t n) {
    if (n && !t) throw std::invalid_argument("model_hip_sampler_schedule: no timestep values given.");
    ConstPool::LoopOptions& o = loop_options(m);
    o.schedule.assign(t, t + n);
    o.schedule_serial++;
}

void Plan::loop_hoist_stats(Model& m, unsigned long long out[8]) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (!m.m_plan) return;
    const Hoist& h = m.m_plan->hoist;
    out[6] = m.m_plan->input_epoch;
    if (!h.ready) return;
    out[0] = m.m_plan->kernel_count() - h.n_p - h.n_t;
    out[1] = h.n_p;
    out[2] = h.n_t;
    out[3] = h.extra_bytes;
    out[4] = h.hits;
    out[5] = h.misses;
    out[7] = h.keys.size();
}

std::string Plan::loop_hoist_info(Model& m) {
    if (!m.m_plan) throw std::runtime_error("model_hip_loop_hoist_info: no plan (call run() first).");
    return m.m_plan->hoist_info();
}

long Plan::hoist_find(float t) const {
    uint32_t key;
    std::memcpy(&key, &t, 4);
    for (size_t r = 0; r < hoist.keys.size(); r++)
        if (hoist.keys[r] == key) return (long)r;
    return -1;
}

// the T steps for the timestep now in the staging buffer -- today's launches in today's order -- and, while the table has room, their row
void Plan::hoist_fill_row(const float* tstep_src, float t, float* tstep, size_t tbytes) {
    if (tstep_src) be.check(be.api.osg_copy(be.ctx, tstep, tstep_src, tbytes), "osg_copy");
    run_steps(0, (size_t)-1, CLS_T);
    if ((long)hoist.keys.size() >= hoist.cap) return;
    char* row = hoist.table + hoist.keys.size() * hoist.row_bytes;
    for (auto& l : hoist.live) be.check(be.api.osg_copy(be.ctx, row + l.off, ptr(l.val), l.bytes), "osg_copy");
    uint32_t key;
    std::memcpy(&key, &t, 4);
    hoist.keys.push_back(key);
}

std::string Plan::hoist_info() const {
    std::string out;
    char buf[256];
    snprintf(buf, sizeof buf, "hoist ready=%d option=%d p=%zu t=%zu extra_bytes=%zu row_bytes=%zu cap=%ld rows=%zu epoch_keyed=%d epoch=%llu\n", (int)hoist.ready,
             (int)loop_hoist, hoist.n_p, hoist.n_t, hoist.extra_bytes, hoist.row_bytes, hoist.cap, hoist.keys.size(), (int)hoist.epoch_keyed, input_epoch);
    out += buf;
    snprintf(buf, sizeof buf, "arena base=%zu bytes=%zu\n", (size_t)(uintptr_t)arena, arena_bytes);
    out += buf;
    if (!hoist.ready) return out;
    for (size_t i = 0; i < steps.size(); i++)
        if (hoist.cls[i] != CLS_STEP) {
            snprintf(buf, sizeof buf, "hoist %c step %zu | ", hoist.cls[i] == CLS_T ? 'T' : 'P', i);
            out += buf + steps[i].what + "\n";
        }
    for (size_t i = 0; i < steps.size(); i++)
        if (hoist.cls[i] != CLS_STEP)
            for (int w : steps[i].writes) {
                if (w < 0) continue;
                const int r = root_of(w);
                snprintf(buf, sizeof buf, "hoist val %d step %zu base=%zu bytes=%zu moved=%d\n", r, i, (size_t)(uintptr_t)ptr(r), val_bytes(r),
                         (int)(std::find(hoist.moved.begin(), hoist.moved.end(), r) != hoist.moved.end()));
                out += buf;
            }
    for (auto& l : hoist.live) {
        snprintf(buf, sizeof buf, "hoist live %d bytes=%zu off=%zu\n", l.val, l.bytes, l.off);
        out += buf;
    }
    return out;
}

// The frame the three sampler loops share: everything between a loop's own table checks and its return.  H: depth of the history ring the loop needs
// (0: none); noise: [steps, prompts, L] host, uploaded when non-NULL.  Per step one prepare launch, the pass, one update launch:
//   prescale(i) -> {rescale, x_scale}: the pair launches osg_sampler_prepare_rescale with x_scale where `rescale` and osg_sampler_prepare otherwise; the
//       single form hands x_scale to osg_sampler_prepare_single.
//   update(i, x, eps, nz, L, slot): the loop's update launch.  nz: row i of the uploaded noise, NULL when none was uploaded.  slot(k): history entry k of
//       step i (k = 0: written now, k >= 1: written k steps ago), which lives in ring slot (i - k) mod H -- the reference's shift of
//       sampler_history_buffer (src/samplers.h:422, :695 and alike) becomes a rotation of the pointers; NULL without a ring.
template <class Prescale, class Update>
double Plan::sampler_frame(const std::string& fn, const std::string& sample_name, const std::string& timestep_name, const std::string& out_name,
                           int n_steps, int prompts, int branches, float* x, const float* c_in, const float* t, int H, const float* noise,
                           Prescale&& prescale, Update&& update) {
    FlightGuard flight(in_flight);
    const SamplerIO io = sampler_io(fn, sample_name, timestep_name, out_name);
    const long L = io.L;
    float *sample = (float*)ptr(io.in_s->staging), *tstep = (float*)ptr(io.in_t->staging);
    const float* eps = (const float*)ptr(io.out->f32val);
    const size_t row = (size_t)prompts * L, xb = row * sizeof(float), nb = (size_t)n_steps * xb;
    grow_buffer(samp_x, samp_x_bytes, xb);
    if (noise) grow_buffer(samp_noise, samp_noise_bytes, nb);
    if (H) grow_buffer(samp_hist, samp_hist_bytes, (size_t)H * xb);
    be.check(be.api.osg_upload(be.ctx, samp_x, x, xb), "osg_upload");
    if (noise) be.check(be.api.osg_upload(be.ctx, samp_noise, noise, nb), "osg_upload");
    float* const sx = (float*)samp_x;
    // ---- loop hoist: only the per-step class is launched per step.  The prompt-only steps run here, once per call (nothing of them is kept across calls: a
    // run() or hip_set_input in between may have changed what they read); the timestep-only steps run where the table has no row for t[i]
    hoist_prepare(io, sample_name, timestep_name);
    Hoist& hz = hoist;
    const bool hoisted = loop_hoist && hz.ready && hz.n_p + hz.n_t > 0;
    if (hoisted && graph && !step_graph) step_graph = capture(CLS_STEP);
    const size_t tbytes = val_bytes(io.in_t->staging);
    if (hoisted && hz.n_t && hz.cap && pool.loop.schedule_serial != hz.schedule_seen && !pool.loop.schedule.empty()) {
        // the schedule's timestep broadcasts, as osg_sampler_prepare* writes them, on the device before anything of this call is enqueued
        const size_t per = tbytes / sizeof(float);
        std::vector<float> bc(pool.loop.schedule.size() * per);
        for (size_t k = 0; k < pool.loop.schedule.size(); k++) std::fill(bc.begin() + k * per, bc.begin() + (k + 1) * per, pool.loop.schedule[k]);
        grow_buffer(hz.tvals, hz.tvals_bytes, bc.size() * sizeof(float));
        be.check(be.api.osg_upload(be.ctx, hz.tvals, bc.data(), bc.size() * sizeof(float)), "osg_upload");
    }
    be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
    if (hoisted) {
        hz.hits = hz.misses = 0;
        if (hz.n_p) run_steps(0, (size_t)-1, CLS_P);
        if (hz.n_t && hz.epoch_keyed && hz.table_epoch != input_epoch) {   // rows computed from other inputs than are resident now
            hz.keys.clear();
            hz.table_epoch = input_epoch;
        }
        if (hz.n_t && hz.cap && pool.loop.schedule_serial != hz.schedule_seen) {
            for (size_t k = 0; k < pool.loop.schedule.size(); k++)
                if (hoist_find(pool.loop.schedule[k]) < 0 && (long)hz.keys.size() < hz.cap)
                    hoist_fill_row((const float*)((const char*)hz.tvals + k * tbytes), pool.loop.schedule[k], tstep, tbytes);
            hz.schedule_seen = pool.loop.schedule_serial;
        }
    }
    for (int i = 0; i < n_steps; i++) {
        const SamplerPrescale ps = prescale(i);
        if (branches != 2)
            be.check(be.api.osg_sampler_prepare_single(be.ctx, sx, sample, tstep, prompts, L, ps.x_scale, c_in[i], t[i], io.TL), "osg_sampler_prepare_single");
        else if (ps.rescale)
            be.check(be.api.osg_sampler_prepare_rescale(be.ctx, sx, sample, tstep, prompts, L, ps.x_scale, c_in[i], t[i], io.TL), "osg_sampler_prepare_rescale");
        else
            be.check(be.api.osg_sampler_prepare(be.ctx, sx, sample, tstep, prompts, L, c_in[i], t[i], io.TL), "osg_sampler_prepare");
        if (hoisted && hz.n_t) {
            const long r = hoist_find(t[i]);
            if (r >= 0) {
                hz.hits++;
                for (auto& l : hz.live) be.check(be.api.osg_copy(be.ctx, ptr(l.val), hz.table + (size_t)r * hz.row_bytes + l.off, l.bytes), "osg_copy");
            } else {
                hz.misses++;
                hoist_fill_row(nullptr, t[i], tstep, tbytes);
            }
        }
        if (hoisted && step_graph) be.check(be.api.osg_graph_launch(be.ctx, step_graph), "osg_graph_launch");
        else if (hoisted) run_steps(0, (size_t)-1, CLS_STEP);
        else if (graph) be.check(be.api.osg_graph_launch(be.ctx, graph), "osg_graph_launch");
        else run_steps();
        const float* nz = noise ? (const float*)samp_noise + (size_t)i * row : nullptr;
        auto slot = [&](int k) -> float* { return H ? (float*)samp_hist + (size_t)(((i - k) % H + H) % H) * row : nullptr; };
        update(i, sx, eps, nz, L, slot);
    }
    float ms = 0;
    be.check(be.api.osg_timer_stop(be.ctx, &ms), "osg_timer_stop");
    be.check(be.api.osg_download(be.ctx, x, samp_x, xb), "osg_download");
    runs += n_steps;
    m_last_ms = n_steps > 0 ? ms / n_steps : 0;
    return ms;
}

double Plan::sampler_loop(const std::string& sample_name, const std::string& timestep_name, const std::string& out_name, int n_steps, int prompts,
                          float* x, const float* noise, const float* c_in, const float* c_out, const float* t, const float* sigma, const float* d_sigma,
                          const float* sigma_up, float guidance, const float* clip, int branches) {
    const bool pair = branches == 2;
    const std::string fn = pair ? "Model::hip_sampler_loop: " : "Model::hip_sampler_loop_single: ";
    sampler_check_state(fn, prompts, branches);
    return sampler_frame(
        fn, sample_name, timestep_name, out_name, n_steps, prompts, branches, x, c_in, t, 0, noise,
        [](int) { return SamplerPrescale{false, 1.f}; },   // Euler-A never rescales x
        [&](int i, float* sx, const float* eps, const float* nz, long L, auto&&) {
            const float cl = clip ? clip[i] : 0.f;
            if (pair)
                be.check(be.api.osg_sampler_cfg_euler_a(be.ctx, sx, eps, nz, prompts, L, c_out[i], guidance, sigma[i], d_sigma[i], sigma_up[i], cl),
                         "osg_sampler_cfg_euler_a");
            else
                be.check(be.api.osg_sampler_euler_a_single(be.ctx, sx, eps, nz, prompts, L, c_out[i], sigma[i], d_sigma[i], sigma_up[i], cl),
                         "osg_sampler_euler_a_single");
        });
}

double Plan::sampler_loop_multistep(const std::string& sample_name, const std::string& timestep_name, const std::string& out_name, int n_steps,
                                   int prompts, int sampler, float* x, const float* c_in, const float* c_out, const float* t, const float* sigma,
                                   const int* order, const float* coef, size_t n_coef, const double* dcoef, size_t n_dcoef, float guidance,
                                   int branches) {
    const bool pair = branches == 2;
    const std::string fn = pair ? "Model::hip_sampler_loop_multistep: " : "Model::hip_sampler_loop_multistep_single: ";
    sampler_check_state(fn, prompts, branches);
    // per sampler: history depth (create_buffers, src/samplers.h:5-24), and the kernel form of each order.  Order 2 of the DPM++ pair is the plain
    // Euler step the reference substitutes on the last step of an SDXL image (src/sd.cpp:1705-1719)
    static const int forms[6][4] = {
        {OSG_MS_DPMPP_FIRST, OSG_MS_DPMPP_2M, OSG_MS_EULER_D, -1},        // 0: DPM++ 2M and 2M v2 (they differ in the host coefficients only)
        {OSG_MS_EULER_D, OSG_MS_IPNDM1, OSG_MS_IPNDM2, OSG_MS_IPNDM3},    // 1: iPNDM
        {OSG_MS_EULER_D, OSG_MS_IPNDM_V1, OSG_MS_IPNDM2, OSG_MS_IPNDM3},  // 2: iPNDM_v
        {OSG_MS_EULER_D, OSG_MS_IPNDM_VO1, OSG_MS_IPNDM_VO2, OSG_MS_IPNDM_VO3},  // 3: iPNDM_vo
        {OSG_MS_EULER_D, OSG_MS_TAYLOR1, OSG_MS_TAYLOR2, -1},             // 4: Taylor3
        {OSG_MS_DDIM, -1, -1, -1},                                        // 5: DDIM
    };
    static const int depth[6] = {1, 4, 4, 4, 3, 0};
    // entries of earlier steps (h1..) that order o reads: o itself, except for that Euler step, which reads none and so is legal at step 0 too -- a
    // one-step image is first and last step at once
    auto reads = [&](int o) { return sampler == 0 && o == 2 ? 0 : o; };
    if (sampler < 0 || sampler >= 6) throw std::invalid_argument(fn + "unknown sampler form " + std::to_string(sampler) + ".");
    if (n_steps < 0 || n_coef != (size_t)n_steps * 6 || n_dcoef != (size_t)n_steps * 2)
        throw std::invalid_argument(fn + "the coefficient tables must hold steps * 6 floats and steps * 2 doubles.");
    for (int i = 0; i < n_steps; i++)
        if (order[i] < 0 || order[i] > 3 || forms[sampler][order[i]] < 0 || reads(order[i]) > i)
            throw std::invalid_argument(fn + "order " + std::to_string(order[i]) + " at step " + std::to_string(i) + " is not available.");
    return sampler_frame(
        fn, sample_name, timestep_name, out_name, n_steps, prompts, branches, x, c_in, t, depth[sampler], nullptr,
        // DDIM alone prescales x, by coef[i][5]: its pair takes the rescaling launch even where the factor is 1
        [&](int i) { return SamplerPrescale{sampler == 5, sampler == 5 ? coef[(size_t)i * 6 + 5] : 1.f}; },
        [&](int i, float* sx, const float* eps, const float*, long L, auto&& slot) {
            const float* k = coef + (size_t)i * 6;
            const int form = forms[sampler][order[i]], r = reads(order[i]);
            float* h0 = slot(0);
            const float *h1 = r >= 1 ? slot(1) : nullptr, *h2 = r >= 2 ? slot(2) : nullptr, *h3 = r >= 3 ? slot(3) : nullptr;
            if (pair)
                be.check(be.api.osg_sampler_cfg_multistep(be.ctx, form, sx, eps, h0, h1, h2, h3, prompts, L, c_out[i], guidance, sigma[i], k[0], k[1], k[2],
                                                          k[3], k[4], dcoef[2 * i], dcoef[2 * i + 1]),
                         "osg_sampler_cfg_multistep");
            else
                be.check(be.api.osg_sampler_multistep_single(be.ctx, form, sx, eps, h0, h1, h2, h3, prompts, L, c_out[i], sigma[i], k[0], k[1], k[2], k[3],
                                                             k[4], dcoef[2 * i], dcoef[2 * i + 1]),
                         "osg_sampler_multistep_single");
        });
}

double Plan::sampler_loop_stochastic(const std::string& sample_name, const std::string& timestep_name, const std::string& out_name, int n_steps,
                                     int prompts, float* x, const float* c_in, const float* c_out, const float* t, const float* sigma, const int* form,
                                     const int* draws, const float* coef, size_t n_coef, const float* noise, float guidance, int branches) {
    const bool pair = branches == 2;
    const std::string fn = pair ? "Model::hip_sampler_loop_stochastic: " : "Model::hip_sampler_loop_stochastic_single: ";
    sampler_check_state(fn, prompts, branches);
    if (n_steps < 0 || n_coef != (size_t)n_steps * 10) throw std::invalid_argument(fn + "the coefficient table must hold steps * 10 floats.");
    auto sde = [](int f) { return f == OSG_ST_SDE0 || f == OSG_ST_SDE1 || f == OSG_ST_SDE2; };
    bool ring = false, any_draw = false;
    for (int i = 0; i < n_steps; i++) {
        if (form[i] < 0 || form[i] >= OSG_ST_FORMS) throw std::invalid_argument(fn + "unknown form " + std::to_string(form[i]) + " at step " + std::to_string(i) + ".");
        // entries of earlier steps (h1, h2) the form reads: each must have been written by an SDE form of this image
        const int r = form[i] == OSG_ST_SDE2 ? 2 : form[i] == OSG_ST_SDE1 ? 1 : 0;
        for (int k = 1; k <= r; k++)
            if (i - k < 0 || !sde(form[i - k]))
                throw std::invalid_argument(fn + "form " + std::to_string(form[i]) + " at step " + std::to_string(i) + " is not available.");
        ring = ring || sde(form[i]);
        any_draw = any_draw || draws[i];
    }
    if (any_draw && !noise) throw std::invalid_argument(fn + "a step draws noise but no noise was given.");
    return sampler_frame(
        fn, sample_name, timestep_name, out_name, n_steps, prompts, branches, x, c_in, t, ring ? 3 : 0 /* create_buffers, src/samplers.h:14 */,
        any_draw ? noise : nullptr,
        // coef[i][9] prescales x: the pair takes the rescaling launch only where it is not 1
        [&](int i) { const float s = coef[(size_t)i * 10 + 9]; return SamplerPrescale{s != 1.f, s}; },
        [&](int i, float* sx, const float* eps, const float* nz, long L, auto&& slot) {
            const float* k = coef + (size_t)i * 10;
            const int f = form[i];
            float* h0 = sde(f) ? slot(0) : nullptr;
            const float *h1 = f == OSG_ST_SDE1 || f == OSG_ST_SDE2 ? slot(1) : nullptr, *h2 = f == OSG_ST_SDE2 ? slot(2) : nullptr;
            if (!draws[i]) nz = nullptr;
            if (pair)
                be.check(be.api.osg_sampler_cfg_stochastic(be.ctx, f, sx, eps, nz, h0, h1, h2, prompts, L, c_out[i], guidance, sigma[i], k[0], k[1], k[2], k[3],
                                                           k[4], k[5], k[6], k[7], k[8]),
                         "osg_sampler_cfg_stochastic");
            else
                be.check(be.api.osg_sampler_stochastic_single(be.ctx, f, sx, eps, nz, h0, h1, h2, prompts, L, c_out[i], sigma[i], k[0], k[1], k[2], k[3], k[4],
                                                              k[5], k[6], k[7], k[8]),
                         "osg_sampler_stochastic_single");
        });
}

double Plan::decode_tiles(const std::string& in_name, const std::string& out_name, int images, int H, int W, float factor, const float* latents,
                          float* image, size_t image_elems, uint8_t* pixels, size_t pixels_elems) {
    static const char* fn = "Model::hip_decode: ";
    if (runs < 1) throw std::runtime_error(std::string(fn) + "run() once first (the plan must have run a pass of this batch).");
    if (stream_weights) throw std::runtime_error(std::string(fn) + "not available in streamed-weights mode.");
    if (u8) throw std::runtime_error(std::string(fn) + "not available with uint8 arithmetic.");
    const In* in = nullptr;
    for (auto& i : inputs)
        if (i.name == in_name) in = &i;
    const Out* out = nullptr;
    for (auto& o : outputs)
        if (o.name == out_name) out = &o;
    if (!in || !out) throw std::invalid_argument(std::string(fn) + "input/output tensor not found.");
    if (out->raw16) throw std::invalid_argument(std::string(fn) + "the output is excluded from the fp32 conversion (m_outputs_convert_set).");
    // tile size and upscale factor are the plan's own: input [1, 4, t, t] fp32, output [1, 3, u*t, u*t]
    const auto& is = in->shape;
    const auto& os = out->shape;
    if (in->host_type != TensorDataType::float32 || is.size() != 4 || is[0] != 1 || is[1] != 4 || is[2] != is[3] || is[2] < 1)
        throw std::invalid_argument(std::string(fn) + "the input must be a float32 tensor [1, 4, t, t].");
    if (os.size() != 4 || os[0] != 1 || os[1] != 3 || os[2] != os[3] || !vals[out->f32val].batched)
        throw std::invalid_argument(std::string(fn) + "the output must be a tensor [1, 3, s, s] per sample.");
    const long t = (long)is[2], s = (long)os[2];
    if (s < t || s % t)
        throw std::invalid_argument(std::string(fn) + "the output's spatial size " + std::to_string(s) + " is not an integer multiple of the tile " + std::to_string(t) + ".");
    const long up = s / t;
    if (images < 1) throw std::invalid_argument(std::string(fn) + "needs at least one image.");
    if (H < t || W < t)
        throw std::invalid_argument(std::string(fn) + "latents of " + std::to_string(H) + " x " + std::to_string(W) + " are smaller than the tile " + std::to_string(t) + ".");
    if (t < 2 && (H != t || W != t)) throw std::invalid_argument(std::string(fn) + "a tile of 1 cannot be stepped over larger latents.");
    // the tile grid of osg_decode_gather / osg_decode_blend (include/osgpu.h): origins min(k * (3t/4), n - t)
    auto along = [&](long n) { const long step = t * 3 / 4; return n == t ? 1L : (n - t + step - 1) / step + 1; };
    const long T = along(H) * along(W);
    if ((long)images * T != N)
        throw std::invalid_argument(std::string(fn) + "the plan's batch is " + std::to_string(N) + ", the decode needs images * tiles = " + std::to_string(images) + " * " +
                                    std::to_string(T) + " = " + std::to_string((long)images * T) + " samples.");
    const size_t lb = (size_t)images * 4 * H * W * sizeof(float), px = (size_t)images * 3 * (H * up) * (W * up);
    if (image && image_elems != px)
        throw std::invalid_argument(std::string(fn) + "the image buffer holds " + std::to_string(image_elems) + " elements, the decode writes " + std::to_string(px) +
                                    " (upscale factor " + std::to_string(up) + ").");
    if (pixels && pixels_elems != px)
        throw std::invalid_argument(std::string(fn) + "the pixel buffer holds " + std::to_string(pixels_elems) + " elements, the decode writes " + std::to_string(px) +
                                    " (upscale factor " + std::to_string(up) + ").");
    if (!image && !pixels) return 0.0;
    FlightGuard flight(in_flight);
    grow_buffer(dec_lat, dec_lat_bytes, lb);
    if (image) grow_buffer(dec_img, dec_img_bytes, px * sizeof(float));
    if (pixels) grow_buffer(dec_pix, dec_pix_bytes, px);
    be.check(be.api.osg_upload(be.ctx, dec_lat, latents, lb), "osg_upload");
    be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
    be.check(be.api.osg_decode_gather(be.ctx, (const float*)dec_lat, (float*)ptr(in->staging), images, H, W, (int)t, factor), "osg_decode_gather");
    if (graph) be.check(be.api.osg_graph_launch(be.ctx, graph), "osg_graph_launch");
    else run_steps();
    be.check(be.api.osg_decode_blend(be.ctx, (const float*)ptr(out->f32val), image ? (float*)dec_img : nullptr, pixels ? (unsigned char*)dec_pix : nullptr, images, H, W,
                                     (int)t, (int)up),
             "osg_decode_blend");
    float ms = 0;
    be.check(be.api.osg_timer_stop(be.ctx, &ms), "osg_timer_stop");
    if (image) be.check(be.api.osg_download(be.ctx, image, dec_img, px * sizeof(float)), "osg_download");
    if (pixels) be.check(be.api.osg_download(be.ctx, pixels, dec_pix, px), "osg_download");
    runs++;
    m_last_ms = ms;
    return ms;
}

// a tensor whose data stays on the device in `dev` (m_hip_resident_outputs, the caches the LLM calls leave): the Tensor owns the buffer from here on -- freed with
// its last copy, as long as the Model lives -- and its host vector stays empty
Tensor Plan::resident_tensor(Model& m, const std::string& name, std::vector<size_t> shape, void* dev, size_t bytes) {
    Tensor t;
    t.m_name = name;
    t.m_shape = std::move(shape);
    t.set_vector(tensor_vector<uint16_t>());
    HipBackend* bp = m.m_backend;
    ConstPool* pp = m.m_pool;
    const size_t cls = ConstPool::size_class(bytes);
    t.m_hip_resident = std::shared_ptr<void>(dev, [alive = std::weak_ptr<bool>(m.m_alive), bp, pp, cls](void* p) {
        if (alive.lock()) pp->give_class(*bp, p, cls);     // (back to the Model's pool: the call after next takes it again)
    });
    t.m_hip_resident_bytes = bytes;
    return t;
}

void Plan::read_resident(Model& m, const Tensor& t, void* dst) {
    if (!m.m_backend) throw std::runtime_error("Model::hip_get_tensor_f16: no backend.");
    m.m_backend->check(m.m_backend->api.osg_download(m.m_backend->ctx, dst, t.m_hip_resident.get(), t.m_hip_resident_bytes), "osg_download");
}

std::string Plan::info() const {
    std::string out;
    char buf[128];
    if (decode && dspec.chunk > 0) out += "prefill chunk " + std::to_string(dspec.chunk) + " capacity " + std::to_string(dspec.cap) + "\n";
    else if (decode) out += "decode capacity " + std::to_string(dspec.cap) + (N > 1 ? " sequences " + std::to_string(N) : "") + "\n";
    for (size_t i = 0; i < steps.size(); i++) {
        const Step& s = steps[i];
        snprintf(buf, sizeof buf, "step %zu reads=", i);
        out += buf;
        for (size_t k = 0; k < s.reads.size(); k++) out += (k ? "," : "") + std::to_string(root_of(s.reads[k]));
        out += " writes=";
        for (size_t k = 0; k < s.writes.size(); k++) out += (k ? "," : "") + std::to_string(root_of(s.writes[k]));
        out += " | " + s.what + "\n";
    }
    for (size_t v = 0; v < vals.size(); v++) {
        const Val& r = vals[v];
        if (r.root >= 0 || r.dptr || r.is_const || r.last < 0) continue;
        snprintf(buf, sizeof buf, "val %zu offset=%zu bytes=%zu first=%d last=%d\n", v, r.offset, val_bytes((int)v), r.first, r.last);
        out += buf;
    }
    out += "arena " + std::to_string(arena_bytes) + "\n";
    return out;
}

std::string Plan::profile(int reps) {
    if (runs < 1) throw std::runtime_error("Model::hip_profile: run() once first (inputs must be resident).");
    FlightGuard flight(in_flight);
    std::vector<double> acc(steps.size(), 0.0);
    // every step between two timestamps on the compute stream, the whole pass enqueued back to back (the queue stays full, as inside the
    // captured graph): a step's figure = its kernels + the dependency gap to its predecessor, no idle-launch latency from host round trips.
    // Passes of more than 4000 steps fall back to one synchronised measurement per step.
    const bool chained = steps.size() < 4000 && !stream_weights;
    for (int r = 0; r < reps; r++) {
        zero_gn_stats();
        if (chained) {
            be.check(be.api.osg_timer_mark(be.ctx, 0), "osg_timer_mark");
            for (size_t i = 0; i < steps.size(); i++) {
                steps[i].run();
                be.check(be.api.osg_timer_mark(be.ctx, (int)i + 1), "osg_timer_mark");
            }
            for (size_t i = 0; i < steps.size(); i++) {
                float ms = 0;
                be.check(be.api.osg_timer_between(be.ctx, (int)i, (int)i + 1, &ms), "osg_timer_between");
                acc[i] += ms;
            }
        } else
            for (size_t i = 0; i < steps.size(); i++) {
                be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
                steps[i].run();
                float ms = 0;
                be.check(be.api.osg_timer_stop(be.ctx, &ms), "osg_timer_stop");
                acc[i] += ms;
            }
    }
    std::string out;
    char buf[256];
    for (size_t i = 0; i < steps.size(); i++) {
        double bytes = 0;
        for (int v : steps[i].reads) bytes += (double)val_bytes(v);
        for (int v : steps[i].writes) bytes += (double)val_bytes(v);
        snprintf(buf, sizeof buf, "%.6f\t%.0f\t%.0f\t", acc[i] / reps, steps[i].flops, bytes);
        out += buf;
        out += steps[i].what;
        out += "\n";
    }
    return out;
}

}  // namespace onnxstream
