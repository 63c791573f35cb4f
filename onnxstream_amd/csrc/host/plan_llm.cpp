// plan_llm.cpp -- the LLM calls of Plan: the device token loop (generate) and the chat turn (turn) over the Model's two resident plans, and the steps they share.
// Each shared step lives once (plan.h lists them; run_pass and resident_tensor are in plan_run.cpp, beside capture and execute); what differs between the two
// callers on purpose is an argument at the call site.
#include "plan.h"

#include <algorithm>
#include <array>
#include <cmath>

namespace onnxstream {

void ConstPool::drop_decode() {
    delete decode_plan;
    decode_plan = nullptr;
    decode_key.clear();
}

void ConstPool::drop_prefill() {
    delete prefill_plan;
    prefill_plan = nullptr;
    prefill_key.clear();
}

std::string Plan::decode_info(Model& m) {
    if (!m.m_pool || !m.m_pool->decode_plan) throw std::runtime_error("Model::hip_decode_plan_info: no decode plan (call model_hip_generate first).");
    return m.m_pool->decode_plan->info();
}

std::string Plan::prefill_info(Model& m) {
    if (!m.m_pool || !m.m_pool->prefill_plan) throw std::runtime_error("Model::hip_prefill_plan_info: no chunk plan (call model_hip_turn first).");
    return m.m_pool->prefill_plan->info();
}

// what model_hip_generate_sampled_ext, _batch_ext and model_hip_turn_ext refuse of the four controls and the history (exports.cpp lists it)
void Plan::SampleRule::check(const std::string& fn, long long max_new, long V) const {
    if (!(repetition > 0.0f) || std::isinf(repetition) || !std::isfinite(1.0f / repetition))
        throw std::invalid_argument(fn + "repetition_penalty must be > 0 and finite, with a finite 1 / repetition_penalty (1 = off).");
    if (!std::isfinite(presence)) throw std::invalid_argument(fn + "presence_penalty must be finite (0 = off).");
    if (!std::isfinite(frequency)) throw std::invalid_argument(fn + "frequency_penalty must be finite (0 = off).");
    if (!(min_p >= 0.0f) || !(min_p <= 1.0f)) throw std::invalid_argument(fn + "min_p must be in [0, 1] (0 = off).");
    if (min_p > 0.0f && temperature == 0.0f) throw std::invalid_argument(fn + "min_p needs temperature > 0 (the greedy pick keeps one token anyway).");
    if (n_history < 0) throw std::invalid_argument(fn + "n_history must be >= 0.");
    if (n_history > 0 && !history) throw std::invalid_argument(fn + "no history tokens (n_history > 0).");
    if (n_history + std::max(max_new, 0LL) >= (1LL << 24))
        throw std::invalid_argument(fn + "n_history + max_new must be below 2^24 (a count must stay exact in fp32).");
    for (long long i = 0; i < n_history && V >= 0; i++)
        if (history[i] < 0 || history[i] >= V)
            throw std::invalid_argument(fn + "history token " + std::to_string(history[i]) + " at " + std::to_string(i) + " is outside [0, " + std::to_string(V) + ").");
}

// what generate and turn both refuse before they look at the Model's tensors; `run_first_why` is the caller's reason inside "run() once first (...)"
void Plan::check_loop_call(Model& m, const std::string& fn, const DecodeSpec& names, int max_new, const int64_t* tokens, const SampleRule& rule,
                           const char* run_first_why) {
    if (max_new < 0) throw std::invalid_argument(fn + "max_new must be >= 0.");
    if (!(rule.temperature >= 0.0f) || std::isinf(rule.temperature)) throw std::invalid_argument(fn + "temperature must be finite and >= 0 (0 = greedy).");
    if (rule.temperature > 0.0f && std::isinf(1.0f / rule.temperature)) throw std::invalid_argument(fn + "temperature is too small: 1 / temperature is not finite.");
    if (rule.top_k < 0) throw std::invalid_argument(fn + "top_k must be >= 0 (0 = off).");
    if (!(rule.top_p > 0.0f) || !(rule.top_p <= 1.0f)) throw std::invalid_argument(fn + "top_p must be in (0, 1] (1 = off).");
    rule.check(fn, max_new, -1);
    if (names.n_caches <= 0) throw std::invalid_argument(fn + "needs at least one key/value cache.");
    if (!m.m_plan || !m.m_backend || !m.m_pool || m.m_plan->runs < 1) throw std::runtime_error(fn + "run() once first (" + run_first_why + ").");
    if (m.m_use_uint8_arithmetic) throw std::runtime_error(fn + "not available with uint8 arithmetic.");
    if (m.m_hip_stream_weights || m.m_cuda_options.m_vram_to_use > 0) throw std::runtime_error(fn + "not available in streamed-weights mode.");
    if (!m.m_use_fp16_arithmetic) throw std::runtime_error(fn + "needs fp16 arithmetic (m_use_fp16_arithmetic).");
    if (!m.m_use_scaled_dp_attn_op)
        throw std::runtime_error(fn + "needs m_use_scaled_dp_attn_op (the op-by-op attention chain is not implemented in the device token loop).");
    if (!m.m_support_dynamic_shapes) throw std::runtime_error(fn + "needs m_support_dynamic_shapes.");
    if (tokens == nullptr && max_new > 0) throw std::invalid_argument(fn + "no buffer for the tokens.");
}

// The Model's resident plan of kind `k` (plan.h: ResidentKind) with room for min_cap rows: the kept one while its key -- the names, k.key_dim, every option the
// build reads, the cache geometry, the extra outputs, the convert set, k.batch, the upcast answers -- and its capacity still fit, else a new one, built by the
// ordinary lowering over stand-ins for the graph inputs (shapes and types, the mask's ones; tokens and positions have no plan-time value) and checked to be the loop's.
Plan* Plan::resident_plan(Model& m, const std::string& fn, const DecodeSpec& names, const CacheGeo& geo, long min_cap, const ResidentKind& k) {
    HipBackend& be = *m.m_backend;
    std::string key = names.ids + "|" + names.pos + "|" + names.mask + "|" + names.logits + "|" + names.cache_in + "|" + names.cache_out + "|" + std::to_string(names.n_caches) +
                      "|" + std::to_string(k.key_dim) + "|" + std::to_string(m.m_hip_fusion_level) + (m.m_hip_fuse_ln_gemm ? "l" : "-") + (m.m_hip_concat_views ? "c" : "-") +
                      (m.m_hip_fuse_tblock ? "t" : "-") + (m.m_hip_autotune ? "a" : "-") + (m.m_hip_w8_resident ? "8" : "-") + (m.m_fuse_ops_in_attention ? "f" : "-") +
                      (m.m_hip_resident_outputs ? "r" : "-") + "|" + std::to_string(m.m_hip_gn_stats) + "|";
    for (auto& g : geo) key += std::to_string(g[0]) + "x" + std::to_string(g[1]) + ",";
    key += "|";
    for (auto& e : m.m_extra_outputs) key += e + ",";
    key += "|";
    for (auto& e : m.m_outputs_convert_set) key += e + ",";
    key += "|" + std::to_string(k.batch) + "|";
    if (m.m_requires_upcast)
        for (auto& op : m.m_ops) key += m.m_requires_upcast(op.m_type, op.m_name) ? '1' : '0';
    if (k.slot && (k.slot_key != key || k.slot->dspec.cap < min_cap)) {
        delete k.slot;
        k.slot = nullptr;
        k.slot_key.clear();
    }
    if (k.slot) return k.slot;
    const size_t cap = (size_t)((min_cap + 63) / 64 * 64), T = k.chunk > 0 ? (size_t)k.chunk : 1;
    std::vector<Tensor> fake;
    auto push_i64 = [&](const std::string& name, std::vector<size_t> shape, size_t n, int64_t v) {
        Tensor t;
        t.m_name = name;
        t.m_shape = std::move(shape);
        t.set_vector(tensor_vector<int64_t>(n, v));
        fake.push_back(std::move(t));
    };
    push_i64(names.ids, {1, T}, T, 0);
    push_i64(names.pos, {1, T}, T, 0);
    push_i64(names.mask, {1, cap}, cap, 1);
    for (int i = 0; i < names.n_caches; i++) {
        Tensor t;
        t.m_name = names.cache_in + std::to_string(i);
        t.m_shape = {1, (size_t)geo[i][0], cap - T, (size_t)geo[i][1]};
        t.set_vector(tensor_vector<uint16_t>());
        fake.push_back(std::move(t));
    }
    Plan* p = new Plan(m, be, *m.m_pool, (size_t)k.batch);
    p->decode = true;
    p->dspec = names;
    p->dspec.cap = (long)cap;
    if (k.chunk > 0) p->dspec.chunk = k.chunk;
    p->build_inputs = &fake;
    m.m_plans_built++;
    try {
        p->dec_state = (int*)be.malloc(16 * (size_t)k.batch);
        p->build();
        p->build_inputs = nullptr;
        // the plan must really be the loop's: one in-place append per cache, the token and position inputs, the logits as an fp32 output
        size_t appends = 0;
        for (auto& s : p->steps)
            for (const char* label : k.appends) appends += s.what.rfind(label, 0) == 0;
        if (appends != (size_t)names.n_caches)
            throw std::invalid_argument(fn + "the graph appends to " + std::to_string(appends) + " caches named '" + names.cache_in + "<i>' -> '" + names.cache_out +
                                        "<i>', the call names " + std::to_string(names.n_caches) + ".");
        bool has_ids = false, has_pos = false, has_logits = false;
        for (auto& in : p->inputs) { has_ids |= in.name == names.ids; has_pos |= in.name == names.pos; }
        for (auto& o : p->outputs) has_logits |= o.name == names.logits && !o.raw16 && k.logits_ok(p->vals[o.f32val].numel());
        if (!has_ids) throw std::invalid_argument(fn + "tensor not found: " + names.ids);
        if (!has_pos) throw std::invalid_argument(fn + "tensor not found: " + names.pos);
        if (!has_logits) throw std::invalid_argument(fn + "the graph has no fp32 output '" + names.logits + "' of " + k.logits_want + ".");
        if (k.chunk > 0) {      // (a chunk plan's staging starts out as padding rows; osg_prefill_stage writes it before every pass)
            const std::vector<int64_t> zeros(T, 0);
            for (auto& in : p->inputs)
                if (in.name == names.ids || in.name == names.pos) be.check(be.api.osg_upload(be.ctx, p->ptr(in.staging), zeros.data(), zeros.size() * 8), "osg_upload");
        }
    } catch (...) {
        delete p;
        throw;
    }
    k.slot = p;
    k.slot_key = key;
    return p;
}

namespace {

using In = Plan::In;
using Out = Plan::Out;

// what a loop reads and writes in its resident plan
struct LoopBindings {
    const In *in_ids = nullptr, *in_pos = nullptr;
    const Out* out_lg = nullptr;
    std::vector<const In*> in_cache;
};

LoopBindings loop_bindings(const Plan& p, const std::string& fn, const Plan::DecodeSpec& names) {
    LoopBindings b;
    b.in_cache.assign((size_t)names.n_caches, nullptr);
    for (auto& in : p.inputs) {
        if (in.name == names.ids) b.in_ids = &in;
        if (in.name == names.pos) b.in_pos = &in;
        const int ci = p.cache_index(in.name, names.cache_in);
        if (ci >= 0) b.in_cache[(size_t)ci] = &in;
    }
    for (auto& o : p.outputs)
        if (o.name == names.logits) b.out_lg = &o;
    for (auto* c : b.in_cache)
        if (!c) throw std::invalid_argument(fn + "tensor not found: " + names.cache_in + "<i>");
    return b;
}

// positions [0, positions) and tokens [0, V) against the smallest table the plan's Gathers index with them
void check_tables(const Plan& p, const std::string& fn, const Plan::DecodeSpec& names, long positions, long V) {
    if (positions > p.dec_pos_limit)
        throw std::invalid_argument(fn + "positions up to " + std::to_string(positions - 1) + " are needed, the smallest table indexed by '" + names.pos + "' has " +
                                    std::to_string(p.dec_pos_limit) + " rows.");
    if (V > p.dec_tok_limit)
        throw std::invalid_argument(fn + "the logits name " + std::to_string(V) + " tokens, the smallest table indexed by '" + names.ids + "' has " +
                                    std::to_string(p.dec_tok_limit) + " rows.");
}

// device scratch for host-side caches on their way into the capacity buffers and out of them: one 256-byte-aligned slot of `rows` rows per cache, allocated when
// the first host-side cache asks for it, freed with the call
struct CacheScratch {
    HipBackend& be;
    std::vector<size_t> slot;
    void* p = nullptr;
    CacheScratch(HipBackend& be_, const Plan::CacheGeo& geo, long rows) : be(be_), slot(geo.size() + 1, 0) {
        for (size_t i = 0; i < geo.size(); i++) slot[i + 1] = slot[i] + (((size_t)geo[i][0] * rows * geo[i][1] * 2 + 255) & ~(size_t)255);
    }
    CacheScratch(const CacheScratch&) = delete;
    ~CacheScratch() { if (p) be.free(p); }
    void* at(size_t i) {
        if (!p) p = be.malloc(slot.back());
        return (char*)p + slot[i];
    }
};

// cache i of the conversation so far ([Hkv][P][d], on the host or device-resident) into the capacity buffers [n_seq][Hkv][cap][d]: every sequence starts from a
// copy of its own
void stage_cache(HipBackend& be, CacheScratch& scratch, size_t i, Tensor& c, long Hkv, long P, long d, void* capbuf, long cap, int n_seq) {
    const void* src = c.m_hip_resident.get();
    if (!src) {
        void* up = scratch.at(i);
        be.check(be.api.osg_upload(be.ctx, up, c.get_vector<uint16_t>().data(), (size_t)Hkv * P * d * 2), "osg_upload");
        src = up;
    }
    for (int s = 0; s < n_seq; s++)
        be.check(be.api.osg_copy_2d(be.ctx, 2, src, P * d, 0, (char*)capbuf + (size_t)s * Hkv * cap * d * 2, cap * d, 0, Hkv, P * d), "osg_copy_2d");
}

void erase_tensor(Model& m, const std::string& name) {
    for (size_t i = 0; i < m.m_data.size(); i++)
        if (m.m_data[i].m_name == name) { m.m_data.erase(m.m_data.begin() + i); return; }
}

// m_data as the host loop would have left it: the logits `row` as [.., 1, V], then the first `rows` rows of every cache of plan p's capacity buffers as
// <cache_out><i> [1, Hkv, rows, d] -- device-resident where the cache was (a buffer of the Model's pool), else compacted in the scratch and downloaded.  A
// tensor of the same name is erased first, the new one goes to the end.
void publish(Model& m, HipBackend& be, ConstPool& pool, const Plan& p, const LoopBindings& io, const Plan::CacheGeo& geo, const std::vector<char>& was_resident,
             CacheScratch& scratch, std::vector<size_t> logits_shape, const float* row, long V, long rows) {
    auto replace = [&](Tensor&& t) {
        erase_tensor(m, t.m_name);
        m.m_data.push_back(std::move(t));
    };
    {
        Tensor t;
        t.m_name = p.dspec.logits;
        t.m_shape = std::move(logits_shape);
        t.m_shape[t.m_shape.size() - 2] = 1;
        tensor_vector<float> host((size_t)V);
        be.check(be.api.osg_download(be.ctx, host.data(), row, (size_t)V * sizeof(float)), "osg_download");
        t.set_vector(std::move(host));
        replace(std::move(t));
    }
    const long cap = p.dspec.cap;
    for (size_t i = 0; i < geo.size(); i++) {
        const long Hkv = geo[i][0], d = geo[i][1];
        const size_t bytes = (size_t)Hkv * rows * d * 2;
        const void* capbuf = p.ptr(io.in_cache[i]->val);
        const std::string name = p.dspec.cache_out + std::to_string(i);
        const std::vector<size_t> shape = {1, (size_t)Hkv, (size_t)rows, (size_t)d};
        if (was_resident[i]) {
            void* dev = pool.take_class(be, ConstPool::size_class(bytes));
            Tensor t = Plan::resident_tensor(m, name, shape, dev, bytes);
            be.check(be.api.osg_copy_2d(be.ctx, 2, capbuf, cap * d, 0, dev, rows * d, 0, Hkv, rows * d), "osg_copy_2d");
            replace(std::move(t));
        } else {
            void* tmp = scratch.at(i);
            be.check(be.api.osg_copy_2d(be.ctx, 2, capbuf, cap * d, 0, tmp, rows * d, 0, Hkv, rows * d), "osg_copy_2d");
            tensor_vector<uint16_t> host(bytes / 2);
            be.check(be.api.osg_download(be.ctx, host.data(), tmp, bytes), "osg_download");
            Tensor t;
            t.m_name = name;
            t.m_shape = shape;
            t.set_vector(std::move(host));
            replace(std::move(t));
        }
    }
    be.check(be.api.osg_sync(be.ctx), "osg_sync");
}

// the launch that takes the next token of every sequence from `from` ([n_seq][V]: the logits, or the penalised rows): sampled per sequence in a batch call,
// sampled when temperature > 0, else the argmax; the _ext entry points only when a control is on (they take min_p and keep the count table)
void launch_pick(HipBackend& be, const Plan& dp, const Plan::SampleRule& rule, bool batch, const float* from, long V, int n_seq, long long eos_id, int64_t* ids,
                 int64_t* pos, int max_new, int* counts) {
    int64_t* toks = (int64_t*)dp.dec_tokens;
    const unsigned long long* seeds = (const unsigned long long*)dp.dec_seeds;
    const bool ext = rule.extended(), sampled = rule.temperature > 0.0f;
    if (batch && ext)
        be.check(be.api.osg_decode_sample_batch_ext(be.ctx, from, V, n_seq, eos_id, dp.dec_state, ids, pos, toks, max_new, rule.temperature, rule.top_k, rule.top_p, seeds,
                                                    rule.draw_base, rule.min_p, counts),
                 "osg_decode_sample_batch_ext");
    else if (ext && sampled)
        be.check(be.api.osg_decode_sample_ext(be.ctx, from, 1, V, eos_id, dp.dec_state, ids, pos, toks, max_new, rule.temperature, rule.top_k, rule.top_p, rule.seed,
                                              rule.draw_base, rule.min_p, counts),
                 "osg_decode_sample_ext");
    else if (ext)
        be.check(be.api.osg_decode_pick_ext(be.ctx, from, 1, V, eos_id, dp.dec_state, ids, pos, toks, max_new, counts), "osg_decode_pick_ext");
    else if (batch)
        be.check(be.api.osg_decode_sample_batch(be.ctx, from, V, n_seq, eos_id, dp.dec_state, ids, pos, toks, max_new, rule.temperature, rule.top_k, rule.top_p, seeds,
                                                rule.draw_base),
                 "osg_decode_sample_batch");
    else if (sampled)
        be.check(be.api.osg_decode_sample(be.ctx, from, 1, V, eos_id, dp.dec_state, ids, pos, toks, max_new, rule.temperature, rule.top_k, rule.top_p, rule.seed,
                                          rule.draw_base),
                 "osg_decode_sample");
    else
        be.check(be.api.osg_decode_pick(be.ctx, from, 1, V, eos_id, dp.dec_state, ids, pos, toks, max_new), "osg_decode_pick");
}

}  // namespace

// The reference app's token loop (src/llm.cpp:472-496) with the argmax, the cache append and the cache length on the device: max_new x (osg_decode_pick + the
// T = 1 pass of the Model's resident decode plan) enqueued back to back.  model_hip_generate (exports.cpp) states the contract.  With a sampling rule
// (model_hip_generate_sampled) osg_decode_sample stands where the pick stands; nothing else differs.
// n_seq / seeds (model_hip_generate_batch, `batch` set): n_seq sequences from the one prompt, side by side in a decode plan of batch n_seq -- tokens
// [n_seq][max_new], n_tokens / stop [n_seq], logits_trace [n_seq][max_new][V], sequence s sampled with seeds[s]; m_data is left as it was.
double Plan::generate(Model& m, const DecodeSpec& names, int max_new, long long eos_id, int sync_every, int64_t* tokens, int* n_tokens, int* stop,
                      float* logits_trace, const SampleRule& rule, int n_seq, const unsigned long long* seeds, bool batch, const TurnEntry* entry) {
    const std::string fn = entry ? "Model::hip_turn: " : batch ? "Model::hip_generate_batch: " : "Model::hip_generate: ";
    if (batch && n_seq < 1) throw std::invalid_argument(fn + "n_seq must be >= 1.");
    for (int s = 0; s < n_seq; s++) {
        if (n_tokens) n_tokens[s] = 0;
        if (stop) stop[s] = 0;
    }
    if (batch && !seeds) throw std::invalid_argument(fn + "no seeds (one per sequence).");
    if (batch && rule.temperature == 0.0f)
        throw std::invalid_argument(fn + "temperature must be > 0: greedy sequences from one prompt are all the same sequence (model_hip_generate gives it).");
    check_loop_call(m, fn, names, max_new, tokens, rule, "the prompt's logits and key/value caches must be in the Model");      // (the loop starts from them)
    auto find = [&](const std::string& name) -> Tensor& {
        for (auto& t : m.m_data)
            if (t.m_name == name) return t;
        throw std::invalid_argument(fn + "tensor not found: " + name);
    };
    // ---- what the previous run() left: the logits [1, T, V] fp32 and the caches [1, Hkv, P, d] fp16 (host or device-resident) ----
    // (a turn: what its prefill leaves on the device -- `entry` says it all, Plan::turn has checked m_data)
    Tensor no_logits;
    Tensor& lg = entry ? no_logits : find(names.logits);
    long T0 = 1, V = entry ? entry->V : 0, P = entry ? entry->P : -1;
    CacheGeo geo;
    if (entry) geo = entry->geo;
    else {
        if (lg.m_type != TensorDataType::float32)
            throw std::invalid_argument(fn + "the logits tensor '" + names.logits + "' must be float32 (list it in m_outputs_convert_set).");
        if (lg.m_shape.size() < 2) throw std::invalid_argument(fn + "the logits tensor '" + names.logits + "' must be [1, T, V].");
        size_t lead = 1;
        for (size_t k = 0; k + 2 < lg.m_shape.size(); k++) lead *= lg.m_shape[k];
        if (lead != 1 || lg.m_batch) throw std::invalid_argument(fn + "the batch must be 1.");
        T0 = (long)lg.m_shape[lg.m_shape.size() - 2];
        V = (long)lg.m_shape.back();
        if (T0 < 1 || V < 1 || lg.get_vector<float>().size() != (size_t)(T0 * V)) throw std::invalid_argument(fn + "the logits tensor '" + names.logits + "' is empty.");
        for (int i = 0; i < names.n_caches; i++) {
            const std::string cn = names.cache_out + std::to_string(i);
            Tensor& c = find(cn);
            if (c.m_type != TensorDataType::float16) throw std::invalid_argument(fn + "cache '" + cn + "' must be float16 (keep it out of m_outputs_convert_set).");
            if (c.m_shape.size() != 4) throw std::invalid_argument(fn + "cache '" + cn + "' must be a [1, Hkv, P, d] tensor.");
            if (c.m_shape[0] != 1 || c.m_batch) throw std::invalid_argument(fn + "the batch must be 1.");
            if (P >= 0 && (long)c.m_shape[2] != P) throw std::invalid_argument(fn + "the caches differ in length.");
            P = (long)c.m_shape[2];
            const size_t bytes = c.m_shape[1] * c.m_shape[2] * c.m_shape[3] * 2;
            if (P < 1 || bytes == 0 || (c.m_hip_resident ? c.m_hip_resident_bytes : c.get_vector<uint16_t>().size() * 2) != bytes)
                throw std::invalid_argument(fn + "cache '" + cn + "' is empty or its data does not match its shape.");
            geo.push_back({(long)c.m_shape[1], (long)c.m_shape[3]});
        }
    }
    rule.check(fn, max_new, V);      // (the history's tokens, now that V is known)
    if (max_new == 0) return 0.0;
    HipBackend& be = *m.m_backend;
    ConstPool& pool = *m.m_pool;
    // ---- the resident decode plan (T = 1, one sequence per sample of its batch): kept while its capacity and the options it was built with still fit ----
    const long min_cap = std::max(P + max_new, entry ? entry->min_cap : 0L);      // (a turn may ask for room for the turns to come)
    Plan* dp = resident_plan(m, fn, names, geo, min_cap,
                             {pool.decode_plan, pool.decode_key, 0, n_seq, V, {"KVAppend ", "KVAppend(batch) "}, [V](long numel) { return numel == V; },
                              std::to_string(V) + " elements per token"});
    check_tables(*dp, fn, names, P + max_new, V);
    const LoopBindings io = loop_bindings(*dp, fn, names);
    const long cap = dp->dspec.cap;
    FlightGuard flight(dp->in_flight);
    // ---- entry: state, the caches into their capacity buffers (strided copies), the last row of the prompt's logits into the pass's logits buffer ----
    dp->grow_buffer(dp->dec_tokens, dp->dec_tokens_bytes, (size_t)n_seq * max_new * 8);
    if (logits_trace) dp->grow_buffer(dp->dec_trace, dp->dec_trace_bytes, (size_t)n_seq * max_new * V * sizeof(float));
    if (batch) dp->grow_buffer(dp->dec_seeds, dp->dec_seeds_bytes, (size_t)n_seq * 8);
    CacheScratch scratch(be, geo, P + max_new);      // (P rows on the way in, up to P + max_new on the way out)
    std::vector<char> was_resident((size_t)names.n_caches, 0);
    // (a loop that stops at its first pick still runs its passes: they append nowhere -- row -1 -- and gather row 0 of the tables)
    std::vector<int> st((size_t)n_seq * 4, 0);
    for (int s = 0; s < n_seq; s++) { st[4 * (size_t)s] = -1; st[4 * (size_t)s + 1] = (int)P; }
    be.check(be.api.osg_upload(be.ctx, dp->dec_state, st.data(), st.size() * sizeof(int)), "osg_upload");
    if (batch) be.check(be.api.osg_upload(be.ctx, dp->dec_seeds, seeds, (size_t)n_seq * 8), "osg_upload");
    // penalties: the count table [n_seq][V], zeroed and filled from the history per call (every sequence starts from the same history), and the row
    // step 0 writes; min-p alone needs neither.  With all four controls off nothing here runs and the loop below launches what it always launched.
    const bool penalized = rule.penalized();
    int* counts = nullptr;
    float* adjusted = nullptr;
    if (penalized) {
        dp->grow_buffer(dp->dec_counts, dp->dec_counts_bytes, (size_t)n_seq * V * sizeof(int));
        dp->grow_buffer(dp->dec_adjusted, dp->dec_adjusted_bytes, (size_t)n_seq * V * sizeof(float));
        counts = (int*)dp->dec_counts;
        adjusted = (float*)dp->dec_adjusted;
        be.check(be.api.osg_memset(be.ctx, counts, 0, (size_t)n_seq * V * sizeof(int)), "osg_memset");
        if (rule.n_history > 0) {
            dp->grow_buffer(dp->dec_history, dp->dec_history_bytes, (size_t)rule.n_history * 8);
            be.check(be.api.osg_upload(be.ctx, dp->dec_history, rule.history, (size_t)rule.n_history * 8), "osg_upload");
            for (int s = 0; s < n_seq; s++)
                be.check(be.api.osg_decode_count(be.ctx, (const int64_t*)dp->dec_history, (long)rule.n_history, counts + (size_t)s * V, V), "osg_decode_count");
        }
    }
    const float inv_r = 1.0f / rule.repetition;
    int64_t *ids_dev = (int64_t*)dp->ptr(io.in_ids->staging), *pos_dev = (int64_t*)dp->ptr(io.in_pos->staging);
    const std::vector<int64_t> zeros((size_t)n_seq, 0);
    be.check(be.api.osg_upload(be.ctx, ids_dev, zeros.data(), zeros.size() * 8), "osg_upload");
    be.check(be.api.osg_upload(be.ctx, pos_dev, zeros.data(), zeros.size() * 8), "osg_upload");
    // a turn: the chunks are enqueued here, behind the uploads above; from now on the host waits for nothing until the loop is through
    const float* entry_row = entry ? entry->prefill() : nullptr;
    for (int i = 0; i < names.n_caches; i++) {
        const long Hkv = geo[i][0], d = geo[i][1];
        void* capbuf = dp->ptr(io.in_cache[(size_t)i]->val);
        if (entry) {      // one strided device copy per cache: the prefill's capacity buffers into the loop's
            was_resident[(size_t)i] = entry->was_resident[(size_t)i];
            if (P > 0) be.check(be.api.osg_copy_2d(be.ctx, 2, entry->caches[(size_t)i], entry->cap * d, 0, capbuf, cap * d, 0, Hkv, P * d), "osg_copy_2d");
        } else {
            Tensor& c = find(names.cache_out + std::to_string(i));
            was_resident[(size_t)i] = c.m_hip_resident != nullptr;
            stage_cache(be, scratch, (size_t)i, c, Hkv, P, d, capbuf, cap, n_seq);
        }
    }
    float* lg_dev = (float*)dp->ptr(io.out_lg->f32val);      // [n_seq][V]
    if (entry) be.check(be.api.osg_copy(be.ctx, lg_dev, entry_row, (size_t)V * sizeof(float)), "osg_copy");
    for (int s = 0; s < n_seq && !entry; s++)
        be.check(be.api.osg_upload(be.ctx, lg_dev + (size_t)s * V, lg.get_vector<float>().data() + (size_t)(T0 - 1) * V, (size_t)V * sizeof(float)), "osg_upload");
    // ---- the loop: nothing on the device waits -- once the stop code is set, a pick is a no-op and a pass recomputes the last token's pass (same inputs, same row) ----
    auto all_stopped = [&] {
        for (int s = 0; s < n_seq; s++)
            if (!st[4 * (size_t)s + 3]) return false;
        return true;
    };
    std::fill(st.begin(), st.end(), 0);
    int passes = 0;
    if (!entry) be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");      // (a turn's time starts at its first chunk)
    for (int n = 0; n < max_new; n++) {
        if (penalized)      // step 0 into the scratch rows; the logits buffer (and with it the trace) keeps what the model computed
            be.check(be.api.osg_decode_penalize(be.ctx, lg_dev, V, V, n_seq, counts, adjusted, rule.repetition, inv_r, rule.presence, rule.frequency),
                     "osg_decode_penalize");
        launch_pick(be, *dp, rule, batch, penalized ? adjusted : lg_dev, V, n_seq, eos_id, ids_dev, pos_dev, max_new, counts);
        dp->run_pass();
        passes++;
        if (logits_trace && n_seq == 1)
            be.check(be.api.osg_copy(be.ctx, (char*)dp->dec_trace + (size_t)n * V * sizeof(float), lg_dev, (size_t)V * sizeof(float)), "osg_copy");
        else if (logits_trace)      // row n of every sequence's trace [max_new][V] in one strided copy
            be.check(be.api.osg_copy_2d(be.ctx, 4, lg_dev, V, 0, dp->dec_trace, (long)max_new * V, (long)n * V, n_seq, V), "osg_copy_2d");
        if (sync_every > 0 && (n + 1) % sync_every == 0 && n + 1 < max_new) {
            be.check(be.api.osg_download(be.ctx, st.data(), dp->dec_state, st.size() * sizeof(int)), "osg_download");
            if (all_stopped()) break;
        }
    }
    float ms = 0;
    be.check(be.api.osg_timer_stop(be.ctx, &ms), "osg_timer_stop");
    // ---- exit: the state, the tokens, the trace; then m_data as the host loop would have left it ----
    be.check(be.api.osg_download(be.ctx, st.data(), dp->dec_state, st.size() * sizeof(int)), "osg_download");
    for (int s = 0; s < n_seq; s++) {
        const int* q = &st[4 * (size_t)s];
        if (q[2] < 0 || q[2] > max_new || q[1] != P + q[2]) throw std::runtime_error(fn + "the device-side loop state is inconsistent.");
    }
    dp->m_last_ms = passes ? ms / passes : 0;
    m.m_last_ms = dp->m_last_ms;
    m.m_last_kernels = dp->kernel_count();
    for (int s = 0; s < n_seq; s++) {      // every sequence's tokens and trace rows up to its own count
        const size_t nt = (size_t)st[4 * (size_t)s + 2], at = (size_t)s * max_new;
        if (nt) be.check(be.api.osg_download(be.ctx, tokens + at, (char*)dp->dec_tokens + at * 8, nt * 8), "osg_download");
        if (nt && logits_trace)
            be.check(be.api.osg_download(be.ctx, logits_trace + at * V, (char*)dp->dec_trace + at * V * sizeof(float), nt * V * sizeof(float)), "osg_download");
        if (n_tokens) n_tokens[s] = (int)nt;
        if (stop) stop[s] = st[4 * (size_t)s + 3];
    }
    if (batch) {      // m_data stays as it was -- the caller carries on from the continuation it picks
        be.check(be.api.osg_sync(be.ctx), "osg_sync");
        return ms;
    }
    const int nt = st[2];
    if (nt == 0) return ms;          // no pass of the host loop ran: logits and caches stay as they are
    publish(m, be, pool, *dp, io, geo, was_resident, scratch, entry ? entry->logits_shape : lg.m_shape, lg_dev, V, P + nt);      // (`lg` is gone from here on)
    return ms;
}

// One chat turn (src/llm.cpp:456-497) as one call: the prompt in chunks of `chunk` rows through the Model's resident chunk plan, which appends to capacity
// buffers at a device-side row, then the token loop above from the prefill's own last real logits row.  model_hip_turn (exports.cpp) states the contract.
// The chunk plan and the decode plan keep capacity buffers of their own; one strided device copy per cache moves the P + n_prompt rows across per turn
// (DESIGN.md 4.5 says why).
double Plan::turn(Model& m, const DecodeSpec& names, const long long* prompt, int n_prompt, int chunk, long long capacity, int max_new, long long eos_id,
                  int sync_every, int64_t* tokens, int* n_tokens, int* stop, float* logits_trace, const SampleRule& rule) {
    const std::string fn = "Model::hip_turn: ";
    if (n_tokens) *n_tokens = 0;
    if (stop) *stop = 0;
    if (n_prompt < 1 || !prompt) throw std::invalid_argument(fn + "n_prompt must be >= 1 (a turn without a prompt is model_hip_generate).");
    if (chunk < 1 || chunk > 512) throw std::invalid_argument(fn + "chunk must be in [1, 512].");
    if (capacity < 0) throw std::invalid_argument(fn + "capacity must be >= 0 (0 = as many rows as this turn needs).");
    // (generate runs these again when the loop starts; a turn of max_new = 0 never gets there.  A turn needs no logits or caches of a run(), only its weights)
    check_loop_call(m, fn, names, max_new, tokens, rule, "the weights must be on the device; the app's weight-loading pass counts");
    auto lookup = [&](const std::string& name) -> Tensor* {
        for (auto& t : m.m_data)
            if (t.m_name == name) return &t;
        return nullptr;
    };
    // ---- the conversation so far: <cache_out><i> as a run() or a turn left them, else <cache_in><i> as the caller pushed them (P = 0 rows: the first turn) ----
    const bool from_out = lookup(names.cache_out + "0") != nullptr;
    const std::string& prefix = from_out ? names.cache_out : names.cache_in;
    long P = -1;
    TurnEntry entry;
    std::vector<Tensor*> src((size_t)names.n_caches, nullptr);
    for (int i = 0; i < names.n_caches; i++) {
        const std::string cn = prefix + std::to_string(i);
        Tensor* c = lookup(cn);
        if (!c) throw std::invalid_argument(fn + "tensor not found: " + cn + " (the conversation so far: '" + names.cache_out + "<i>', or '" + names.cache_in + "<i>' as pushed).");
        if (c->m_shape.size() != 4) throw std::invalid_argument(fn + "cache '" + cn + "' must be a [1, Hkv, P, d] tensor.");
        if (c->m_shape[0] != 1 || c->m_batch) throw std::invalid_argument(fn + "the batch must be 1.");
        if (P >= 0 && (long)c->m_shape[2] != P) throw std::invalid_argument(fn + "the caches differ in length.");
        P = (long)c->m_shape[2];
        const size_t elems = c->m_shape[1] * c->m_shape[2] * c->m_shape[3];
        // (an empty cache may be of any type: the app pushes its zero-length caches before fp16 arithmetic is switched on)
        if (elems && c->m_type != TensorDataType::float16) throw std::invalid_argument(fn + "cache '" + cn + "' must be float16 (keep it out of m_outputs_convert_set).");
        if (c->m_shape[1] < 1 || c->m_shape[3] < 1 || (elems && (c->m_hip_resident ? c->m_hip_resident_bytes : c->get_vector<uint16_t>().size() * 2) != elems * 2))
            throw std::invalid_argument(fn + "cache '" + cn + "' is empty or its data does not match its shape.");
        entry.geo.push_back({(long)c->m_shape[1], (long)c->m_shape[3]});
        entry.was_resident.push_back(c->m_hip_resident != nullptr || (elems == 0 && m.m_hip_resident_outputs));
        src[(size_t)i] = c;
    }
    const long C = chunk, n_chunks = (n_prompt + C - 1) / C, Pn = P + n_prompt;
    const long need = std::max(P + n_chunks * C, Pn + max_new);
    HipBackend& be = *m.m_backend;
    ConstPool& pool = *m.m_pool;
    // ---- the resident chunk plan (T = C, batch 1): keyed as the decode plan is, with C where that has V; its logits are C rows of a V it reports itself ----
    Plan* cp = resident_plan(m, fn, names, entry.geo, std::max(need, (long)capacity),
                             {pool.prefill_plan, pool.prefill_key, C, 1, C, {"KVAppend(rows) "}, [C](long numel) { return numel % C == 0; }, "one row per token"});
    const LoopBindings io = loop_bindings(*cp, fn, names);
    const long V = cp->vals[io.out_lg->f32val].numel() / C, cap = cp->dspec.cap;
    check_tables(*cp, fn, names, Pn + max_new, V);      // (over the prompt as well: a padding row gathers row 0)
    rule.check(fn, max_new, V);
    for (int i = 0; i < n_prompt; i++)
        if (prompt[i] < 0 || prompt[i] >= cp->dec_tok_limit)
            throw std::invalid_argument(fn + "prompt token " + std::to_string(prompt[i]) + " at " + std::to_string(i) + " is outside the smallest table indexed by '" + names.ids +
                                        "' (" + std::to_string(cp->dec_tok_limit) + " rows).");
    // ---- entry: the prompt and the caches so far into the chunk plan's buffers (uploads and strided copies, all before the first chunk) ----
    FlightGuard flight(cp->in_flight);
    cp->grow_buffer(cp->dec_tokens, cp->dec_tokens_bytes, (size_t)n_prompt * 8);
    be.check(be.api.osg_upload(be.ctx, cp->dec_tokens, prompt, (size_t)n_prompt * 8), "osg_upload");
    CacheScratch scratch(be, entry.geo, Pn);      // (P rows on the way in, P + n_prompt on the way out)
    for (int i = 0; i < names.n_caches && P > 0; i++)
        stage_cache(be, scratch, (size_t)i, *src[(size_t)i], entry.geo[i][0], P, entry.geo[i][1], cp->ptr(io.in_cache[(size_t)i]->val), cap, 1);
    int64_t *ids_dev = (int64_t*)cp->ptr(io.in_ids->staging), *pos_dev = (int64_t*)cp->ptr(io.in_pos->staging);
    float* lg_dev = (float*)cp->ptr(io.out_lg->f32val);      // [C][V]
    const float* last_row = lg_dev + (size_t)((n_prompt - 1) % C) * V;
    // ---- the chunks: stage (tokens, positions, first row), then the pass ----
    auto prefill = [&]() -> const float* {
        be.check(be.api.osg_timer_start(be.ctx), "osg_timer_start");
        for (long j = 0; j < n_chunks; j++) {
            be.check(be.api.osg_prefill_stage(be.ctx, (const int64_t*)cp->dec_tokens, n_prompt, j * C, P + j * C, (int)C, ids_dev, pos_dev, cp->dec_state), "osg_prefill_stage");
            cp->run_pass();
        }
        return last_row;
    };
    entry.P = Pn;
    entry.cap = cap;
    entry.V = V;
    entry.min_cap = (long)capacity;
    for (auto* c : io.in_cache) entry.caches.push_back(cp->ptr(c->val));
    {
        Tensor* lg = lookup(names.logits);
        if (lg && lg->m_shape.size() >= 2) entry.logits_shape = lg->m_shape;
        else entry.logits_shape = {1, 1, (size_t)V};
        entry.logits_shape.back() = (size_t)V;
    }
    entry.prefill = prefill;
    double ms = 0;
    int nt = 0, st = 0;
    if (max_new > 0) {
        ms = generate(m, names, max_new, eos_id, sync_every, tokens, &nt, &st, logits_trace, rule, 1, nullptr, false, &entry);
        m.m_last_ms = ms / (double)(n_chunks + std::max(nt, 1));
    } else {
        prefill();
        float t = 0;
        be.check(be.api.osg_timer_stop(be.ctx, &t), "osg_timer_stop");
        ms = t;
        m.m_last_ms = ms / (double)n_chunks;
        m.m_last_kernels = cp->kernel_count();
    }
    cp->m_last_ms = ms;
    if (n_tokens) *n_tokens = nt;
    if (stop) *stop = st;
    // ---- m_data: the loop has left the logits of its last pass and the caches of P + n_prompt + nt rows; when no pass of it ran, the prefill's are left here ----
    if (!from_out)      // (consumed, as a run() consumes its inputs)
        for (int i = 0; i < names.n_caches; i++) erase_tensor(m, names.cache_in + std::to_string(i));
    if (nt == 0) publish(m, be, pool, *cp, io, entry.geo, entry.was_resident, scratch, entry.logits_shape, last_row, V, Pn);
    return ms;
}

}  // namespace onnxstream
