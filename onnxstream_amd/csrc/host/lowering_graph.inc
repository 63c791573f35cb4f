// part of struct Lowering (plan.cpp): the weights pass (Phase B), the graph index, the FUSION PASSES of fusion levels 1 / 2 and plan-time evaluation of shape subgraphs.
// Included inside the struct body: one translation unit, three files by concern (round 6; the run-time half of Plan lives in plan_run.cpp).
    // ------------------------------------------------------------------------------------------------------------------
    // Phase B: pull every weight occurrence through the WeightsProvider in model order and make it resident.
    // dtype policy (reference get_tensor_data :2885-2909): u8 -> dequantised; f16/f32 -> the arithmetic type, except
    // operands the reference forces to float (InstanceNormalization scale/bias :4802, Pow exponent :5485, Resize scales).
    // ------------------------------------------------------------------------------------------------------------------
    static bool wants_f32(const Operation& op, size_t idx) {
        if (op.m_type == "InstanceNormalization" && (idx == 1 || idx == 2)) return true;
        if (op.m_type == "Resize") return true;
        if (op.m_type == "Pow" && idx == 1) return true;
        return false;
    }

    template <typename T>
    tensor_vector<T> fetch(WeightsProvider* wp, const std::string& fn) {
        if constexpr (std::is_same_v<T, uint8_t>) return wp->get_uint8(fn);
        else if constexpr (std::is_same_v<T, uint16_t>) return wp->get_float16(fn);
        else if constexpr (std::is_same_v<T, float>) return wp->get_float32(fn);
        else return wp->get_int64(fn);
    }

    // what one weight occurrence resolves to: the file actually read, its layout / shape, the dtype it is kept in on the device
    struct Occ { std::string fn, key; Shape shape; Lay lay; osg_dtype want; long count; };
    Occ resolve(const Operation& op, size_t i, const Tensor& t, TensorDataType ty) const {
        Occ o;
        o.fn = t.m_name;
        o.shape = to_shape(t.m_shape);
        o.lay = Lay::plain;
        auto pos = o.fn.find("_nchw.bin");
        if (pos != std::string::npos) {
            // conv weight: model.txt names the OIHW file, the runtime loads the OHWI twin (reference :2666-2692)
            if (o.shape.size() == 3) o.shape.push_back(1);  // Conv1D lifted to 2-D
            if (o.shape.size() != 4) throw std::invalid_argument("Model::get_tensor_data: layout is nhwc but invalid shape.");
            o.fn = o.fn.substr(0, pos) + "_nhwc.bin";
            o.lay = Lay::nhwc;
        }
        const bool f32 = wants_f32(op, i) || !P.fp16 || P.u8;
        // W8A16: the weight operand of a contraction stays uint8 when the on-chip dequantising kernels take its shape;
        // W8A8 (m_use_uint8_arithmetic): every uint8 weight stays uint8 -- the integer kernels consume the codes
        bool keep_u8 = false;
        if (ty == TensorDataType::uint8 && P.u8) keep_u8 = true;
        else if (ty == TensorDataType::uint8 && !f32) {
            if (P.w8_resident && i == 1) {
                if (op.m_type == "Conv") keep_u8 = o.shape.size() == 4 && o.shape[1] % 64 == 0;                      // [O,I,kh,kw]: Cin % 64
                else if (op.m_type == "MatMul" || op.m_type == "Gemm") keep_u8 = o.shape.size() == 2 && o.shape[0] % 64 == 0;   // [K,N]
            }
        }
        o.want = keep_u8 ? OSG_U8 : ty == TensorDataType::int64 ? OSG_I64 : (f32 ? OSG_F32 : OSG_F16);
        o.key = o.fn + (o.want == OSG_F32 ? "|f32" : o.want == OSG_F16 ? "|f16" : o.want == OSG_U8 ? "|u8" : "|i64");
        o.count = prod(o.shape);
        return o;
    }

    void load_weights() {
        WeightsProvider* wp = m.get_wp();
        ConstPool& pool = P.pool;
        const bool use_pool = !P.stream_weights;
        // a rebuilt plan (other batch size / input shapes / options) is served from the Model's pool: the provider is not touched
        // again -- it is exhausted by now and, with m_use_ops_cache, no longer holds the weights.  Only when a different device format
        // is wanted (fp16 arithmetic / hip_w8_resident toggled) the whole sequence is pulled once more, from a restarted provider.
        bool fetch_all = true;
        std::vector<Occ> resolved;   // of the pool check below, reused by the main loop (a plan of the LLM flow is rebuilt on every call)
        if (use_pool && pool.complete) {
            fetch_all = false;
            size_t occ = 0;
            resolved.reserve(pool.occ_types.size());
            for (auto& op : ops())
                for (size_t i = 0; i < op.m_input.size() && !fetch_all; i++) {
                    const Tensor& t = op.m_input[i];
                    if (!is_const_tensor(t)) continue;
                    if (occ >= pool.occ_types.size()) fetch_all = true;
                    else {
                        resolved.push_back(resolve(op, i, t, pool.occ_types[occ]));
                        if (!pool.base.count(resolved.back().key)) fetch_all = true;
                    }
                    occ++;
                }
            if (fetch_all) resolved.clear();
            if (fetch_all) {
                wp->on_restart();
                pool.occ_types.clear();
                pool.complete = false;
            }
        }
        size_t occ = 0;
        for (auto& op : ops())
            for (size_t i = 0; i < op.m_input.size(); i++) {
                Tensor& t = op.m_input[i];
                if (!is_const_tensor(t)) continue;
                TensorDataType ty = t.m_type;
                if (fetch_all) {
                    TensorDataType nt = wp->get_type_of_next();
                    if (nt != TensorDataType::none) ty = nt;
                    if (use_pool) pool.occ_types.push_back(ty);
                } else
                    ty = pool.occ_types[occ];
                occ++;
                const Occ o_fresh = fetch_all ? resolve(op, i, t, ty) : Occ{};
                const Occ& o = fetch_all ? o_fresh : resolved[occ - 1];
                const std::string& fn = o.fn;
                const osg_dtype want = o.want;
                const long count = o.count;
                int v = -1;
                auto it = const_cache.find(o.key);
                auto new_const = [&](void* dptr) {
                    v = P.new_val("", o.shape, want, o.lay, false);
                    Val& val = V(v);
                    val.is_const = true;
                    val.name = fn;
                    val.qscale = t.m_scale;
                    val.qzp = (int)t.m_zero_point;
                    val.dptr = dptr;
                    const_cache[o.key] = v;
                };
                if (!fetch_all) {
                    if (it != const_cache.end()) v = it->second;
                    else {
                        const ConstPool::Base& b = pool.base.at(o.key);
                        new_const(b.dptr);
                        V(v).host_f = b.host_f;
                        V(v).host_i = b.host_i;
                        V(v).host_valid = b.host_valid;
                        P.weight_bytes += b.bytes;
                    }
                    t.m_name = "#" + std::to_string(v);
                    continue;
                }
                detail::dispatch_dtype(ty, [&](auto tag) {
                    using T = typename decltype(tag)::type;
                    tensor_vector<T> data = fetch<T>(wp, fn);  // always fetched: providers serve strictly in order
                    if ((long)data.size() != count) throw std::invalid_argument("Model::get_tensor_data: mismatch between tensor shape and data size.");
                    if (it != const_cache.end()) {
                        v = it->second;
                        if (P.stream_weights) {
                            Plan::WRecipe r;
                            r.fn = fn; r.ty = ty;
                            P.recipes.push_back(r);
                        }
                        return;
                    }
                    const size_t bytes = (size_t)count * esize(want);
                    // small constants stay readable on the host for the planner (shapes, axes, eps, scales ...)
                    constexpr osg_dtype have = std::is_same_v<T, uint8_t> ? OSG_U8 : std::is_same_v<T, uint16_t> ? OSG_F16
                                               : std::is_same_v<T, float> ? OSG_F32 : OSG_I64;
                    std::vector<float> host_f;
                    std::vector<int64_t> host_i;
                    bool host_valid = false;
                    if (have == OSG_I64) {
                        host_i.assign((const int64_t*)data.data(), (const int64_t*)data.data() + count);
                        host_valid = true;
                    } else if (count <= 4096 && want != OSG_U8) {
                        host_f.resize(count);
                        for (long k = 0; k < count; k++) {
                            if constexpr (std::is_same_v<T, uint8_t>) host_f[k] = (float)((int)data[k] - (int)t.m_zero_point) * t.m_scale;
                            else if constexpr (std::is_same_v<T, uint16_t>) host_f[k] = half_to_float(data[k]);
                            else if constexpr (std::is_same_v<T, float>) host_f[k] = data[k];
                        }
                        host_valid = true;
                    }
                    auto pit = use_pool ? pool.base.find(o.key) : pool.base.end();
                    if (pit != pool.base.end()) {   // (a partial reload: this format is resident already)
                        new_const(pit->second.dptr);
                    } else if (P.budgeted && have == want && have != OSG_I64 && !host_valid && P.resident_bytes + bytes > P.vram_budget) {
                        // over the VRAM budget: this weight gets no buffer of its own -- every pass (the first one included) it is pulled from
                        // the provider again and lands in the streaming ring right before the step that reads it (Plan::restream)
                        new_const(nullptr);
                        Plan::WRecipe rec;
                        rec.val = v; rec.fn = fn; rec.ty = ty; rec.have = have; rec.want = want; rec.count = count;
                        rec.scale = t.m_scale; rec.zp = (int)t.m_zero_point;
                        rec.ring = true;
                        P.recipes.push_back(rec);
                        P.ring_weight_bytes += bytes;
                    } else {
                        new_const(be.malloc(bytes));
                        P.resident_bytes += bytes;
                        if (use_pool) {
                            ConstPool::Base b;
                            b.dptr = V(v).dptr; b.bytes = bytes; b.host_f = host_f; b.host_i = host_i; b.host_valid = host_valid;
                            pool.base[o.key] = std::move(b);
                            pool.bytes += bytes;
                        } else
                            P.owned.push_back(V(v).dptr);
                        Plan::WRecipe rec;
                        rec.val = v; rec.fn = fn; rec.ty = ty; rec.have = have; rec.want = want; rec.count = count;
                        rec.scale = t.m_scale; rec.zp = (int)t.m_zero_point;
                        if (have == want) {
                            be.check(be.api.osg_upload(be.ctx, V(v).dptr, data.data(), bytes), "osg_upload");
                        } else {
                            if (have == OSG_I64 || want == OSG_I64) throw std::invalid_argument("Model::get_tensor_data: unsupported tensor data format.");
                            void* tmp = be.malloc((size_t)count * sizeof(T));
                            be.check(be.api.osg_upload(be.ctx, tmp, data.data(), (size_t)count * sizeof(T)), "osg_upload");
                            be.check(be.api.osg_convert(be.ctx, have, want, tmp, V(v).dptr, count, t.m_scale, (int)t.m_zero_point), "osg_convert");
                            be.check(be.api.osg_sync(be.ctx), "osg_sync");
                            if (P.stream_weights) { rec.raw = tmp; P.owned.push_back(tmp); }
                            else be.free(tmp);
                        }
                        // budget mode: resident weights are fetched (providers serve strictly in order) but not re-sent.  Streamed mode: the same for the
                        // vectors small enough to stay readable on the host (biases, norm gains: <= 16 KiB each, 0.1 % of the bytes but half of the copies)
                        static const bool resend_small = getenv("OSG_STREAM_RESEND_SMALL") != nullptr;
                        rec.resident = P.budgeted || (host_valid && !resend_small);
                        if (P.stream_weights) P.recipes.push_back(rec);
                    }
                    P.weight_bytes += bytes;
                    V(v).host_f = std::move(host_f);
                    V(v).host_i = std::move(host_i);
                    V(v).host_valid = host_valid;
                });
                if (m.m_use_ops_cache && !P.stream_weights && !m.m_weights_exclusion_set.count(fn)) {
                    // resident from now on: drop the provider's host copy, like the reference's ops cache does (:4556-4569)
                    try { wp->remove(fn); } catch (const std::exception&) {}
                    m.m_weights_exclusion_set.insert(fn);
                }
                t.m_name = "#" + std::to_string(v);  // from here on the tensor names its resident val
            }
        be.check(be.api.osg_sync(be.ctx), "osg_sync");
        if (use_pool) pool.complete = true;
    }

    int const_val(const Tensor& t) const { return std::stoi(t.m_name.substr(1)); }

    // ------------------------------------------------------------------------------------------------------------------
    // graph indices for the fusion passes
    // ------------------------------------------------------------------------------------------------------------------
    void index_graph() {
        uses.clear(); producer.clear(); consumers.clear();
        uses.reserve(ops().size() * 2); producer.reserve(ops().size() * 2); consumers.reserve(ops().size() * 2);
        for (size_t i = 0; i < ops().size(); i++) {
            if (dead[i]) continue;
            for (auto& in : ops()[i].m_input)
                if (!in.m_name.empty() && in.m_type == TensorDataType::none) {
                    uses[in.m_name]++;
                    consumers[in.m_name].push_back((int)i);
                }
            for (auto& out : ops()[i].m_output) producer[out.m_name] = (int)i;
        }
        for (auto& n : P.extra_outputs) uses[n] += 1000;  // never fuse away something the caller wants to read
    }
    bool act(const Tensor& t) const { return !t.m_name.empty() && t.m_type == TensorDataType::none; }
    int prod_of(const Tensor& t) const {
        if (!act(t)) return -1;
        auto it = producer.find(t.m_name);
        return it == producer.end() ? -1 : it->second;
    }
    int use_count(const std::string& n) const { auto it = uses.find(n); return it == uses.end() ? 0 : it->second; }
    int sole_consumer(const Tensor& t) const {
        if (use_count(t.m_name) != 1) return -1;
        auto it = consumers.find(t.m_name);
        return it == consumers.end() || it->second.size() != 1 ? -1 : it->second[0];
    }
    bool is(int i, const char* type) const { return i >= 0 && !dead[i] && P.ops[i].m_type == type; }
    const Val* cval(const Tensor& t) const { return is_const_tensor(t) ? &P.vals[const_val(t)] : nullptr; }
    bool const_scalar(const Tensor& t, float* out) const {
        const Val* v = cval(t);
        if (!v || v->numel() != 1 || !v->host_valid || v->host_f.empty()) return false;
        *out = v->host_f[0];
        return true;
    }
    // the other operand of a commutative binary op
    int other(const Operation& op, const std::string& name) const { return op.m_input[0].m_name == name ? 1 : 0; }

    // a pass whose anchor op type does not occur in the (live) graph is skipped together with its re-indexing: the LLM flow re-plans on every call
    // and a 1 200-op llama graph spent 2/3 of its plan time re-indexing for passes that had nothing to match
    bool has_type(const char* type) const {
        for (size_t i = 0; i < P.ops.size(); i++)
            if (!dead[i] && P.ops[i].m_type == type) return true;
        return false;
    }
    // uint8 arithmetic: Reshape[1,G,L] -> InstanceNormalization -> Reshape[x.shape] over a 4-D tensor ==> osg.qu8.InstanceNormNHWC.  Not a fusion of
    // arithmetic (the two Reshapes carry codes and parameters through unchanged, the normalisation is one table lookup per code either way):
    // it only keeps the tensor in the convolutions' NHWC layout instead of copying it to NCHW and back (62 of the VAE decoder's launches).
    void fuse_u8_instance_norm_nhwc() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "InstanceNormalization")) continue;
            Operation& in = ops()[i];
            if (in.m_input.size() != 3 || in.m_output.size() != 1) continue;
            const int r0 = prod_of(in.m_input[0]);
            if (!is(r0, "Reshape") || use_count(in.m_input[0].m_name) != 1) continue;
            const Tensor x = ops()[r0].m_input[0];
            if (!act(x) || x.m_shape.size() != 4 || x.m_shape[0] != 1) continue;
            const auto& gs = in.m_input[0].m_shape;
            if (gs.size() != 3 || gs[0] != 1 || gs[1] == 0) continue;
            const long G = (long)gs[1], C = (long)x.m_shape[1], HW = (long)x.m_shape[2] * (long)x.m_shape[3];
            if (C % G || (long)gs[2] != (C / G) * HW || G > 56) continue;
            const int r1 = sole_consumer(in.m_output[0]);
            if (!is(r1, "Reshape") || ops()[r1].m_output[0].m_shape != x.m_shape) continue;
            Operation f;
            f.m_name = in.m_name;                 // (the op's range data is looked up under the InstanceNormalization's name)
            f.m_type = "osg.qu8.InstanceNormNHWC";
            f.m_input = {x, in.m_input[1], in.m_input[2]};
            f.m_output = {ops()[r1].m_output[0]};
            f.m_attributes = in.m_attributes;
            f.m_attributes.emplace_back("groups", std::to_string(G));
            dead[r0] = dead[i] = 1;
            ops()[r1] = std::move(f);
        }
    }

    // uint8 arithmetic: Mul(x, gamma[C]) -> Add(., beta[C]) [-> Sigmoid -> Mul(., sigmoid)] over a 4-D tensor ==> osg.qu8.AffineAct.  One pass
    // over the tensor instead of two / four; every stage re-quantises with ITS op's range exactly as the separate launches do (the fused op keeps
    // the four op names for the range lookups), so the codes are unchanged.
    void fuse_u8_affine_act() {
        auto chan_const = [&](const Tensor& t, long C) {
            const Val* v = cval(t);
            if (!v || v->dtype != OSG_U8 || v->numel() != C) return false;
            const Shape& sh = v->shape;
            return (sh.size() == 3 && sh[0] == C) || (sh.size() == 4 && sh[1] == C);
        };
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Mul")) continue;
            Operation& mu = ops()[i];
            if (mu.m_input.size() != 2 || mu.m_output.size() != 1) continue;
            int xi = -1;
            for (int k = 0; k < 2; k++)
                if (act(mu.m_input[k]) && mu.m_input[k].m_shape.size() == 4 && mu.m_input[k].m_shape[0] == 1 && chan_const(mu.m_input[1 - k], (long)mu.m_input[k].m_shape[1])) xi = k;
            if (xi < 0) continue;
            const Tensor x = mu.m_input[xi], gam = mu.m_input[1 - xi];
            const long C = (long)x.m_shape[1];
            const int ad = sole_consumer(mu.m_output[0]);
            if (!is(ad, "Add") || ops()[ad].m_input.size() != 2) continue;
            const int bidx = other(ops()[ad], mu.m_output[0].m_name);
            if (!chan_const(ops()[ad].m_input[bidx], C)) continue;
            const Tensor bet = ops()[ad].m_input[bidx];
            // optional SiLU: the Add feeds exactly a Sigmoid and the Mul that multiplies it back
            int sg = -1, m2 = -1;
            const std::string& an = ops()[ad].m_output[0].m_name;
            if (use_count(an) == 2) {
                auto it = consumers.find(an);
                if (it != consumers.end() && it->second.size() == 2) {
                    for (int c : it->second)
                        if (is(c, "Sigmoid")) sg = c;
                        else if (is(c, "Mul")) m2 = c;
                    if (sg >= 0 && m2 >= 0 && sole_consumer(ops()[sg].m_output[0]) == m2 && ops()[m2].m_input.size() == 2) {
                        const std::string &p0 = ops()[m2].m_input[0].m_name, &p1 = ops()[m2].m_input[1].m_name, &sn = ops()[sg].m_output[0].m_name;
                        if (!((p0 == an && p1 == sn) || (p0 == sn && p1 == an))) sg = m2 = -1;
                    } else
                        sg = m2 = -1;
                }
            }
            const bool silu = sg >= 0 && m2 >= 0;
            if (!silu && use_count(an) != 1) {
                // (the Add's result is read by several ops and they are not the SiLU pair: still one pass for Mul + Add)
            }
            Operation f;
            const int last = silu ? m2 : ad;
            f.m_name = ops()[last].m_name;
            f.m_type = "osg.qu8.AffineAct";
            f.m_input = {x, gam, bet};
            f.m_output = {ops()[last].m_output[0]};
            f.m_attributes = {{"mul", mu.m_name}, {"add", ops()[ad].m_name}};
            if (silu) {
                f.m_attributes.emplace_back("sigmoid", ops()[sg].m_name);
                f.m_attributes.emplace_back("mul2", ops()[m2].m_name);
            }
            // the normalisation right in front (already in its NHWC form): its table lookup rides in this pass
            const int nrm = prod_of(x);
            if (is(nrm, "osg.qu8.InstanceNormNHWC") && use_count(x.m_name) == 1) {
                f.m_type = "osg.qu8.NormAffineAct";
                f.m_input = {ops()[nrm].m_input[0], gam, bet, ops()[nrm].m_input[1], ops()[nrm].m_input[2]};
                f.m_attributes.emplace_back("norm", ops()[nrm].m_name);
                for (auto& a : ops()[nrm].m_attributes) f.m_attributes.emplace_back("norm_" + a.first, a.second);
                dead[nrm] = 1;
            }
            dead[i] = 1;
            if (silu) dead[ad] = dead[sg] = 1;
            ops()[last] = std::move(f);
        }
    }

    void run_fusions() {
        dead.assign(ops().size(), 0);
        if (P.u8 && m.m_hip_fusion_level >= 1 && has_type("InstanceNormalization")) { index_graph(); fuse_u8_instance_norm_nhwc(); }
        if (P.u8 && m.m_hip_fusion_level >= 1 && has_type("Mul") && has_type("Add")) { index_graph(); fuse_u8_affine_act(); }
        if (m.m_use_scaled_dp_attn_op && has_type("Softmax")) { index_graph(); fuse_sdpa(); }   // (a Model option of the reference, independent of hip_fusion_level)
        if (P.fusion >= 1) {
            if (m.m_requires_upcast && has_type("Pow") && has_type("ReduceMean")) { index_graph(); fuse_rms_norm(); }
            if (has_type("Neg") && has_type("Slice")) { index_graph(); fuse_rope(); }
            if (has_type("Sigmoid")) { index_graph(); fuse_silu(); }
            if (has_type("InstanceNormalization")) { index_graph(); fuse_group_norm(); }
            if (has_type("ReduceMean") && has_type("Sub")) { index_graph(); fuse_layer_norm(); }
            if (has_type("Erf")) { index_graph(); fuse_geglu(); }
        }
        if (P.fusion >= 2) {
            if (has_type("Softmax")) { index_graph(); fuse_attention(true); }
            if (has_type("MatMul")) { index_graph(); fuse_linear(); }
            if (has_type("Conv") || has_type("osg.Linear")) { index_graph(); fuse_residual(); }
            if (has_type("Conv")) { index_graph(); fuse_conv_act(); }
            if (has_type("osg.GEGLU")) { index_graph(); fuse_linear_geglu(); }
            if (has_type("osg.Attention") && has_type("osg.LayerNorm")) { index_graph(); fuse_tblock_tail(); }
            if (has_type("osg.SiLU")) { index_graph(); cse_silu(); }
            if (has_type("osg.SiLU") && has_type("Gemm")) { index_graph(); fuse_gemm_act(); }   // (after the CSE: the 22 SiLUs behind the time embedding are one by now)
            if (has_type("Conv")) { index_graph(); fuse_image_bias(); }
            if (P.fuse_shortcut && has_type("Conv")) { index_graph(); fuse_conv_shortcut(); }   // (behind fuse_residual, and behind the passes that may still mark either Conv)
        } else if (m.m_fuse_ops_in_attention && has_type("Softmax")) {
            index_graph(); fuse_attention(false);
        }
        std::vector<Operation> live;
        for (size_t i = 0; i < ops().size(); i++)
            if (!dead[i]) live.push_back(std::move(ops()[i]));
        ops() = std::move(live);
    }

    // Sigmoid(x) -> Mul(x, .)   ==> osg.SiLU
    void fuse_silu() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Sigmoid")) continue;
            Operation& sg = ops()[i];
            if (sg.m_input.size() != 1 || sg.m_output.size() != 1 || !act(sg.m_input[0])) continue;
            int j = sole_consumer(sg.m_output[0]);
            if (!is(j, "Mul")) continue;
            Operation& mul = ops()[j];
            if (mul.m_input.size() != 2) continue;
            const std::string& s = sg.m_output[0].m_name;
            int o = other(mul, s);
            if (mul.m_input[o].m_name != sg.m_input[0].m_name || mul.m_input[1 - o].m_name != s) continue;
            mul.m_type = "osg.SiLU";
            Tensor x = mul.m_input[o];
            mul.m_input.clear();
            mul.m_input.push_back(x);
            dead[i] = 1;
        }
    }

    // Reshape[1,G,-1] -> InstanceNormalization(1,0) -> Reshape[n,C,H,W] -> Mul(gamma[C,1,1]) -> Add(beta[C,1,1]) [-> SiLU]
    void fuse_group_norm() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "InstanceNormalization")) continue;
            Operation& in = ops()[i];
            if (in.m_input.size() != 3 || in.m_output.size() != 1) continue;
            const Val* sc = cval(in.m_input[1]);
            const Val* bi = cval(in.m_input[2]);
            if (!sc || !bi || !sc->host_valid || !bi->host_valid) continue;
            bool unit = true;
            for (float f : sc->host_f) unit &= f == 1.0f;
            for (float f : bi->host_f) unit &= f == 0.0f;
            if (!unit) continue;
            int r0 = prod_of(in.m_input[0]);
            if (!is(r0, "Reshape") || use_count(in.m_input[0].m_name) != 1) continue;
            const Tensor& x = ops()[r0].m_input[0];
            if (!act(x) || x.m_shape.size() != 4) continue;
            if (in.m_input[0].m_shape.size() != 3 || in.m_input[0].m_shape[0] != 1) continue;
            long G = (long)in.m_input[0].m_shape[1];
            int r1 = sole_consumer(in.m_output[0]);
            if (!is(r1, "Reshape") || ops()[r1].m_output[0].m_shape != x.m_shape) continue;
            int mu = sole_consumer(ops()[r1].m_output[0]);
            if (!is(mu, "Mul")) continue;
            int gi = other(ops()[mu], ops()[r1].m_output[0].m_name);
            const Val* gam = cval(ops()[mu].m_input[gi]);
            long C = (long)x.m_shape[1];
            auto chan_shape = [&](const Val* v) {
                if (!v || v->numel() != C) return false;
                const Shape& s = v->shape;
                return (s.size() == 3 && s[0] == C) || (s.size() == 4 && s[1] == C);
            };
            if (!chan_shape(gam)) continue;
            int ad = sole_consumer(ops()[mu].m_output[0]);
            if (!is(ad, "Add")) continue;
            int bidx = other(ops()[ad], ops()[mu].m_output[0].m_name);
            if (!chan_shape(cval(ops()[ad].m_input[bidx]))) continue;
            if (C % G || x.m_shape[0] != 1) continue;
            float eps = 1e-5f;
            if (auto* e = attr(in, "epsilon")) eps = std::stof(*e);
            int last = ad;
            bool silu = false;
            int sl = sole_consumer(ops()[ad].m_output[0]);
            if (is(sl, "osg.SiLU")) { silu = true; last = sl; }
            Operation f;
            f.m_name = in.m_name + "_GroupNorm";
            f.m_type = "osg.GroupNorm";
            f.m_input = {x, ops()[mu].m_input[gi], ops()[ad].m_input[bidx]};
            f.m_output = {ops()[last].m_output[0]};
            f.m_attributes = {{"groups", std::to_string(G)}, {"epsilon", std::to_string(eps)}, {"silu", silu ? "1" : "0"}};
            char buf[64];
            snprintf(buf, sizeof buf, "%.9g", eps);
            f.m_attributes[1].second = buf;
            for (int k : {r0, (int)i, r1, mu, ad}) dead[k] = 1;
            if (silu) dead[sl] = 1;
            dead[last] = 0;
            ops()[last] = std::move(f);
        }
    }

    // ReduceMean -> Sub -> Pow(2) -> ReduceMean -> Add(eps) -> Sqrt -> Div -> Mul(gamma) -> Add(beta)
    void fuse_layer_norm() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "ReduceMean")) continue;
            Operation& rm = ops()[i];
            if (rm.m_input.size() != 1 || !act(rm.m_input[0])) continue;
            const Tensor x = rm.m_input[0];
            // both reductions must run over the LAST axis with keepdims = 1 (anything else is not a LayerNorm over the channels)
            auto last_axis_keepdims = [&](const Operation& r) {
                bool ax_ok = false, kd_ok = true;
                for (auto& a : r.m_attributes) {
                    if (a.first == "axes") {
                        auto ax = int_list(a.second);
                        ax_ok = ax.size() == 1 && !r.m_input.empty() && (ax[0] == -1 || ax[0] == (int)r.m_input[0].m_shape.size() - 1);
                    } else if (a.first == "keepdims") kd_ok = std::stoi(a.second) == 1;
                    else return false;
                }
                return ax_ok && kd_ok;
            };
            if (!last_axis_keepdims(rm)) continue;
            int sub = sole_consumer(rm.m_output[0]);
            if (!is(sub, "Sub") || ops()[sub].m_input[0].m_name != x.m_name || ops()[sub].m_input[1].m_name != rm.m_output[0].m_name) continue;
            const std::string d = ops()[sub].m_output[0].m_name;
            if (use_count(d) != 2) continue;
            auto& dc = consumers[d];
            int pw = -1, dv = -1;
            for (int c : dc) { if (is(c, "Pow")) pw = c; if (is(c, "Div")) dv = c; }
            if (pw < 0 || dv < 0 || ops()[pw].m_input[0].m_name != d || ops()[dv].m_input[0].m_name != d) continue;
            float p = 0;
            if (!const_scalar(ops()[pw].m_input[1], &p) || p != 2.0f) continue;
            int rm2 = sole_consumer(ops()[pw].m_output[0]);
            if (!is(rm2, "ReduceMean") || !last_axis_keepdims(ops()[rm2])) continue;
            int ae = sole_consumer(ops()[rm2].m_output[0]);
            if (!is(ae, "Add")) continue;
            float eps = 0;
            if (!const_scalar(ops()[ae].m_input[other(ops()[ae], ops()[rm2].m_output[0].m_name)], &eps)) continue;
            int sq = sole_consumer(ops()[ae].m_output[0]);
            if (!is(sq, "Sqrt")) continue;
            if (sole_consumer(ops()[sq].m_output[0]) != dv || ops()[dv].m_input[1].m_name != ops()[sq].m_output[0].m_name) continue;
            int mu = sole_consumer(ops()[dv].m_output[0]);
            if (!is(mu, "Mul")) continue;
            int gi = other(ops()[mu], ops()[dv].m_output[0].m_name);
            const Val* gam = cval(ops()[mu].m_input[gi]);
            long C = (long)x.m_shape.back();
            if (!gam || gam->numel() != C || gam->shape.back() != C) continue;
            int ad = sole_consumer(ops()[mu].m_output[0]);
            if (!is(ad, "Add")) continue;
            int bidx = other(ops()[ad], ops()[mu].m_output[0].m_name);
            const Val* bet = cval(ops()[ad].m_input[bidx]);
            if (!bet || bet->numel() != C || bet->shape.back() != C) continue;
            Operation f;
            f.m_name = rm.m_name + "_LayerNorm";
            f.m_type = "osg.LayerNorm";
            f.m_input = {x, ops()[mu].m_input[gi], ops()[ad].m_input[bidx]};
            f.m_output = {ops()[ad].m_output[0]};
            char buf[64];
            snprintf(buf, sizeof buf, "%.9g", eps);
            f.m_attributes = {{"epsilon", buf}};
            for (int k : {(int)i, sub, pw, rm2, ae, sq, dv, mu}) dead[k] = 1;
            ops()[ad] = std::move(f);
        }
    }

    bool slice_last_range(const Operation& sl, long* b, long* e) const {
        if (sl.m_input.size() < 3) return false;
        const Val* s = cval(sl.m_input[1]);
        const Val* en = cval(sl.m_input[2]);
        if (!s || !en || s->host_i.size() != 1 || en->host_i.size() != 1) return false;
        long rank = (long)sl.m_input[0].m_shape.size(), dim = (long)sl.m_input[0].m_shape.back();
        if (sl.m_input.size() > 3) {
            const Val* ax = cval(sl.m_input[3]);
            if (!ax || ax->host_i.size() != 1) return false;
            long a = ax->host_i[0];
            if (a < 0) a += rank;
            if (a != rank - 1) return false;
        } else if (rank != 1) return false;
        if (sl.m_input.size() > 4) {
            const Val* st = cval(sl.m_input[4]);
            if (!st || st->host_i.size() != 1 || st->host_i[0] != 1) return false;
        }
        long bb = s->host_i[0], ee = en->host_i[0];
        if (bb < 0) bb += dim;
        if (ee < 0) ee += dim;
        if (ee > dim) ee = dim;
        *b = bb; *e = ee;
        return true;
    }

    // p -> Slice(0:C)=val, Slice(C:2C)=gate ; gate -> Div(sqrt2) -> Erf -> Add(1) -> Mul(gate,.) -> Mul(.,0.5) -> Mul(val,.)
    void fuse_geglu() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Erf")) continue;
            int dv = prod_of(ops()[i].m_input[0]);
            if (!is(dv, "Div") || use_count(ops()[i].m_input[0].m_name) != 1) continue;
            float c = 0;
            // fp16 arithmetic: the divisor is an f16 by the time the Div sees it.  The two exporter forms (the f32 sqrt(2) and its f16 rounding 1.4140625) are
            // the constants that round to the f16 of sqrt(2); anything else (1.413, 1.416) is another function and stays op by op
            if (!const_scalar(ops()[dv].m_input[1], &c) || float_to_half(c) != float_to_half(1.41421356f)) continue;
            const Tensor gate = ops()[dv].m_input[0];
            int gs = prod_of(gate);
            if (!is(gs, "Slice") || use_count(gate.m_name) != 2) continue;
            int a1 = sole_consumer(ops()[i].m_output[0]);
            if (!is(a1, "Add")) continue;
            float one = 0;
            if (!const_scalar(ops()[a1].m_input[other(ops()[a1], ops()[i].m_output[0].m_name)], &one) || one != 1.0f) continue;
            int m1 = sole_consumer(ops()[a1].m_output[0]);
            if (!is(m1, "Mul") || ops()[m1].m_input[other(ops()[m1], ops()[a1].m_output[0].m_name)].m_name != gate.m_name) continue;
            int m2 = sole_consumer(ops()[m1].m_output[0]);
            if (!is(m2, "Mul")) continue;
            float half = 0;
            if (!const_scalar(ops()[m2].m_input[other(ops()[m2], ops()[m1].m_output[0].m_name)], &half) || half != 0.5f) continue;
            int m3 = sole_consumer(ops()[m2].m_output[0]);
            if (!is(m3, "Mul")) continue;
            const Tensor& val = ops()[m3].m_input[other(ops()[m3], ops()[m2].m_output[0].m_name)];
            int vs = prod_of(val);
            if (!is(vs, "Slice") || use_count(val.m_name) != 1) continue;
            const Tensor p = ops()[gs].m_input[0];
            if (!act(p) || ops()[vs].m_input[0].m_name != p.m_name || use_count(p.m_name) != 2) continue;
            long C2 = (long)p.m_shape.back(), b0, e0, b1, e1;
            if (C2 % 2 || !slice_last_range(ops()[vs], &b0, &e0) || !slice_last_range(ops()[gs], &b1, &e1)) continue;
            if (b0 != 0 || e0 != C2 / 2 || b1 != C2 / 2 || e1 != C2) continue;
            Operation f;
            f.m_name = ops()[i].m_name + "_GEGLU";
            f.m_type = "osg.GEGLU";
            f.m_input = {p};
            f.m_output = {ops()[m3].m_output[0]};
            for (int k : {(int)i, dv, gs, vs, a1, m1, m2}) dead[k] = 1;
            ops()[m3] = std::move(f);
        }
    }

    // follows Reshape[1,T,h,d] -> Transpose(0,2,1,3) -> Reshape[h,T,d] backwards from `t`; returns the projection tensor
    bool head_split_source(const Tensor& t, Tensor* src, long* h, long* d, std::vector<int>* chain) {
        int r1 = prod_of(t);
        if (!is(r1, "Reshape") || use_count(t.m_name) != 1 || t.m_shape.size() != 3) return false;
        const Tensor& a = ops()[r1].m_input[0];
        int tp = prod_of(a);
        if (!is(tp, "Transpose") || use_count(a.m_name) != 1) return false;
        auto* pm = attr(ops()[tp], "perm");
        if (!pm || int_list(*pm) != std::vector<int>{0, 2, 1, 3}) return false;
        const Tensor& b = ops()[tp].m_input[0];
        int r0 = prod_of(b);
        if (!is(r0, "Reshape") || use_count(b.m_name) != 1 || b.m_shape.size() != 4 || b.m_shape[0] != 1) return false;
        const Tensor& s = ops()[r0].m_input[0];
        if (!act(s) || s.m_shape.size() != 3 || s.m_shape[0] != 1) return false;
        long T = (long)b.m_shape[1];
        *h = (long)b.m_shape[2];
        *d = (long)b.m_shape[3];
        if ((long)s.m_shape[1] != T || (long)s.m_shape[2] != *h * *d) return false;
        if ((long)t.m_shape[0] != *h || (long)t.m_shape[1] != T || (long)t.m_shape[2] != *d) return false;
        *src = s;
        chain->insert(chain->end(), {r1, tp, r0});
        return true;
    }

    // Pow(x, 2) -> ReduceMean(-1, keepdims) -> Add(eps) -> Sqrt -> Div(1, .) -> Mul(x, .) -> Mul(w, .)  ==> osg.RMSNorm, when m_requires_upcast flags
    // all seven ops (the LLM app's layer norms, src/llm.cpp:379-383): every intermediate then stays fp32 in the reference (each is the sole operand
    // of the next op), so the chain is fp32 arithmetic from the f16 input to one rounding -- which is what the fused kernel does.  Unflagged
    // chains keep their op-by-op f16 roundings.
    bool upcast_flag(const Operation& op) const { return P.fp16 && !P.u8 && m.m_requires_upcast && m.m_requires_upcast(op.m_type, op.m_name); }
    void fuse_rms_norm() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Pow")) continue;
            Operation& pw = ops()[i];
            float two = 0.f, eps = 0.f, one = 0.f;
            if (pw.m_input.size() != 2 || !act(pw.m_input[0]) || !const_scalar(pw.m_input[1], &two) || two != 2.0f) continue;
            const Tensor x = pw.m_input[0];
            const int rm = sole_consumer(pw.m_output[0]);
            if (!is(rm, "ReduceMean")) continue;
            {
                auto* ax = attr(ops()[rm], "axes");
                auto* kd = attr(ops()[rm], "keepdims");
                if (!ax || int_list(*ax) != std::vector<int>{-1} || !kd || *kd != "1") continue;
            }
            const int ad = sole_consumer(ops()[rm].m_output[0]);
            if (!is(ad, "Add") || ops()[ad].m_input.size() != 2) continue;
            if (!const_scalar(ops()[ad].m_input[other(ops()[ad], ops()[rm].m_output[0].m_name)], &eps)) continue;
            const int sq = sole_consumer(ops()[ad].m_output[0]);
            if (!is(sq, "Sqrt")) continue;
            const int dv = sole_consumer(ops()[sq].m_output[0]);
            if (!is(dv, "Div") || ops()[dv].m_input.size() != 2 || ops()[dv].m_input[1].m_name != ops()[sq].m_output[0].m_name ||
                !const_scalar(ops()[dv].m_input[0], &one) || one != 1.0f)
                continue;
            const int m0 = sole_consumer(ops()[dv].m_output[0]);
            if (!is(m0, "Mul") || ops()[m0].m_input.size() != 2) continue;
            if (ops()[m0].m_input[other(ops()[m0], ops()[dv].m_output[0].m_name)].m_name != x.m_name) continue;
            const int m1 = sole_consumer(ops()[m0].m_output[0]);
            if (!is(m1, "Mul") || ops()[m1].m_input.size() != 2) continue;
            const Tensor w = ops()[m1].m_input[other(ops()[m1], ops()[m0].m_output[0].m_name)];
            const Val* wv = cval(w);
            if (!wv || wv->dtype != OSG_F16 || wv->shape.size() != 1) continue;
            bool all_up = true;
            for (int k : {(int)i, rm, ad, sq, dv, m0, m1}) all_up &= upcast_flag(ops()[k]);
            if (!all_up) continue;
            Operation f;
            f.m_name = ops()[m1].m_name + "_RMSNorm";
            f.m_type = "osg.RMSNorm";
            f.m_input = {x, w};
            f.m_output = {ops()[m1].m_output[0]};
            char buf[64];
            snprintf(buf, sizeof buf, "%.9g", eps);
            f.m_attributes = {{"epsilon", buf}};
            for (int k : {(int)i, rm, ad, sq, dv, m0}) dead[k] = 1;
            ops()[m1] = std::move(f);
        }
    }

    // x * cos + Concat(Neg(Slice(x, d/2:d)), Slice(x, 0:d/2)) * sin  ==> osg.RoPE (HF rotate_half; same f16 roundings as the seven ops: bit-identical)
    void fuse_rope() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Add")) continue;
            Operation& add = ops()[i];
            if (add.m_input.size() != 2) continue;
            const int ma = prod_of(add.m_input[0]), mb = prod_of(add.m_input[1]);
            if (!is(ma, "Mul") || !is(mb, "Mul") || use_count(add.m_input[0].m_name) != 1 || use_count(add.m_input[1].m_name) != 1) continue;
            bool done = false;
            for (int swap = 0; swap < 2 && !done; swap++) {
                const Operation& mx = ops()[swap ? mb : ma];      // x * cos
                const Operation& mr = ops()[swap ? ma : mb];      // rotate_half(x) * sin
                if (mx.m_input.size() != 2 || mr.m_input.size() != 2) continue;
                for (int rs = 0; rs < 2 && !done; rs++) {
                    const Tensor rot = mr.m_input[rs], sin_t = mr.m_input[1 - rs];
                    const int cc = prod_of(rot);
                    if (!is(cc, "Concat") || use_count(rot.m_name) != 1 || ops()[cc].m_input.size() != 2) continue;
                    auto* cax = attr(ops()[cc], "axis");
                    if (!cax) continue;
                    const int ng = prod_of(ops()[cc].m_input[0]), s1 = prod_of(ops()[cc].m_input[1]);
                    if (!is(ng, "Neg") || !is(s1, "Slice") || use_count(ops()[cc].m_input[0].m_name) != 1 || use_count(ops()[cc].m_input[1].m_name) != 1) continue;
                    const int s2 = prod_of(ops()[ng].m_input[0]);
                    if (!is(s2, "Slice") || use_count(ops()[ng].m_input[0].m_name) != 1) continue;
                    const Tensor x = ops()[s1].m_input[0];
                    if (!act(x) || ops()[s2].m_input[0].m_name != x.m_name || x.m_shape.empty()) continue;
                    const long d = (long)x.m_shape.back(), rank = (long)x.m_shape.size();
                    if (d <= 0 || d % 2) continue;
                    const int caxis = std::stoi(*cax);
                    if (caxis != -1 && caxis != rank - 1) continue;
                    auto slice_is = [&](int si, long b0, long e0) {
                        const Operation& so = ops()[si];
                        if (so.m_input.size() < 4) return false;
                        const Val *st = cval(so.m_input[1]), *en = cval(so.m_input[2]), *ax = cval(so.m_input[3]);
                        if (!st || !en || !ax || st->host_i.size() != 1 || en->host_i.size() != 1 || ax->host_i.size() != 1) return false;
                        if (so.m_input.size() > 4 && !so.m_input[4].m_name.empty()) {
                            const Val* sp = cval(so.m_input[4]);
                            if (!sp || sp->host_i.size() != 1 || sp->host_i[0] != 1) return false;
                        }
                        const long a = ax->host_i[0];
                        return (a == -1 || a == rank - 1) && st->host_i[0] == b0 && (en->host_i[0] == e0 || (e0 == d && en->host_i[0] >= d));
                    };
                    if (!slice_is(s1, 0, d / 2) || !slice_is(s2, d / 2, d)) continue;
                    const int xi = mx.m_input[0].m_name == x.m_name ? 0 : mx.m_input[1].m_name == x.m_name ? 1 : -1;
                    if (xi < 0) continue;
                    const Tensor cos_t = mx.m_input[1 - xi];
                    Operation f;
                    f.m_name = add.m_name + "_RoPE";
                    f.m_type = "osg.RoPE";
                    f.m_input = {x, cos_t, sin_t};
                    f.m_output = {add.m_output[0]};
                    for (int k : {ma, mb, cc, ng, s1, s2}) dead[k] = 1;
                    ops()[i] = std::move(f);
                    done = true;
                }
            }
        }
    }

    // m_use_scaled_dp_attn_op: the reference's ScaledDotProductAttention rewrite (src/onnxstream.cpp:3635-3755), both forms:
    //   Transpose(k) -> MatMul(q, .) -> Div(., s) -> Add(., mask) -> Softmax(-1) -> MatMul(., v)              scale = f16(1 / s)
    //   Transpose(k) -> Mul(., s2); Mul(q, s) -> MatMul -> Add(., mask) -> Softmax(-1) -> MatMul(., v)         scale = f16(s2 * s)
    // every intermediate with exactly one consumer (the reference's m_intermediate_refs == 1 checks).  The reference matches the ops
    // as CONSECUTIVE queue entries; here they are matched through the graph (the same chains, whatever else the exporter interleaved).
    void fuse_sdpa() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Softmax")) continue;
            Operation& sm = ops()[i];
            auto* ax = attr(sm, "axis");
            if (!ax || *ax != "-1" || sm.m_attributes.size() != 1 || sm.m_input.size() != 1 || sm.m_output.size() != 1) continue;
            const int add = prod_of(sm.m_input[0]);
            if (!is(add, "Add") || use_count(sm.m_input[0].m_name) != 1 || ops()[add].m_input.size() != 2) continue;
            const Tensor mask = ops()[add].m_input[1];
            const Tensor scores = ops()[add].m_input[0];
            const int pre = prod_of(scores);
            if (pre < 0 || use_count(scores.m_name) != 1) continue;
            int mm0 = -1, tp = -1;
            std::vector<int> chain = {(int)i, add};
            Tensor q, s_t, s2_t;
            if (is(pre, "Div") && ops()[pre].m_input.size() == 2) {
                s_t = ops()[pre].m_input[1];
                mm0 = prod_of(ops()[pre].m_input[0]);
                if (!is(mm0, "MatMul") || use_count(ops()[pre].m_input[0].m_name) != 1 || ops()[mm0].m_input.size() != 2) continue;
                q = ops()[mm0].m_input[0];
                tp = prod_of(ops()[mm0].m_input[1]);
                if (tp < 0 || use_count(ops()[mm0].m_input[1].m_name) != 1) continue;
                chain.insert(chain.end(), {pre, mm0});
            } else if (is(pre, "MatMul") && ops()[pre].m_input.size() == 2) {
                mm0 = pre;
                const int mul0 = prod_of(ops()[mm0].m_input[0]), mul1 = prod_of(ops()[mm0].m_input[1]);
                if (!is(mul0, "Mul") || !is(mul1, "Mul") || ops()[mul0].m_input.size() != 2 || ops()[mul1].m_input.size() != 2) continue;
                if (use_count(ops()[mm0].m_input[0].m_name) != 1 || use_count(ops()[mm0].m_input[1].m_name) != 1) continue;
                q = ops()[mul0].m_input[0];
                s_t = ops()[mul0].m_input[1];
                s2_t = ops()[mul1].m_input[1];
                tp = prod_of(ops()[mul1].m_input[0]);
                if (tp < 0 || use_count(ops()[mul1].m_input[0].m_name) != 1) continue;
                chain.insert(chain.end(), {mm0, mul0, mul1});
            } else continue;
            auto* pm = is(tp, "Transpose") ? attr(ops()[tp], "perm") : nullptr;
            if (!pm || int_list(*pm) != std::vector<int>{0, 1, 3, 2} || ops()[tp].m_input.size() != 1) continue;
            const Tensor k = ops()[tp].m_input[0];
            const int mm1 = sole_consumer(sm.m_output[0]);
            if (!is(mm1, "MatMul") || ops()[mm1].m_input.size() != 2 || ops()[mm1].m_input[0].m_name != sm.m_output[0].m_name) continue;
            const Tensor v = ops()[mm1].m_input[1];
            if (!act(q) || !act(k) || !act(v)) continue;
            float s = 0.f, s2 = 0.f;
            auto scalar = [&](const Tensor& t, float* out) {   // "invalid shape of scale" (:7785): a scalar or a 1-element vector
                const Val* sv = cval(t);
                return sv && sv->numel() == 1 && sv->shape.size() <= 1 && const_scalar(t, out);
            };
            if (!scalar(s_t, &s) || (!s2_t.m_name.empty() && !scalar(s2_t, &s2))) continue;
            // fp16 arithmetic: the constants are f16 by the time the op sees them, the product / reciprocal is formed in fp32 and rounded to f16 (:7840-7862)
            const float s16 = half_to_float(float_to_half(s));
            const float val = s2_t.m_name.empty() ? 1.0f / s16 : half_to_float(float_to_half(s2)) * s16;
            const float scale = half_to_float(float_to_half(val));
            Operation f;
            f.m_name = ops()[tp].m_name + "_ScaledDotProductAttention";
            f.m_type = "ScaledDotProductAttention";
            f.m_input = {q, k, mask, v};
            f.m_output = {ops()[mm1].m_output[0]};
            char buf[64];
            snprintf(buf, sizeof buf, "%.9g", scale);
            f.m_attributes = {{"scale", buf}};
            chain.push_back(tp);
            for (int c : chain) dead[c] = 1;
            ops()[mm1] = std::move(f);
        }
    }

    // MatMul(q,kT) -> [Mul(scale)] -> Softmax(-1) -> MatMul(.,v)
    //   full=false: the reference's own AttentionFusedOps rewrite (:3576-3633) -- operands stay [h,T,d]/[h,d,Tk]
    //   full=true : additionally folds the head split / merge Reshape+Transpose chains: reads Q,K,V straight from the
    //               [1,T,h*d] projection outputs and writes [1,T,h*d]
    void fuse_attention(bool full) {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Softmax")) continue;
            Operation& sm = ops()[i];
            auto* ax = attr(sm, "axis");
            if (!ax || *ax != "-1" || sm.m_attributes.size() != 1 || sm.m_input.size() != 1) continue;
            int pre = prod_of(sm.m_input[0]);
            if (pre < 0 || use_count(sm.m_input[0].m_name) != 1) continue;
            int mul = -1, mm0 = pre;
            Tensor scale_t;
            if (is(pre, "Mul")) {
                mul = pre;
                if (ops()[mul].m_input.size() != 2) continue;
                mm0 = prod_of(ops()[mul].m_input[0]);
                if (mm0 < 0 || use_count(ops()[mul].m_input[0].m_name) != 1) continue;
                scale_t = ops()[mul].m_input[1];
            }
            if (!is(mm0, "MatMul")) continue;
            int mm1 = sole_consumer(sm.m_output[0]);
            if (!is(mm1, "MatMul") || ops()[mm1].m_input[0].m_name != sm.m_output[0].m_name) continue;
            const Tensor q = ops()[mm0].m_input[0], kt = ops()[mm0].m_input[1], v = ops()[mm1].m_input[1];
            if (!act(q) || !act(kt) || !act(v)) continue;
            float scale = 1.0f;
            if (mul >= 0) {
                const Val* sv = cval(scale_t);
                if (!sv || !sv->shape.empty() || !const_scalar(scale_t, &scale)) continue;  // "s must be a scalar" (:6723)
            }
            std::vector<int> chain = {mm0, (int)i};
            if (mul >= 0) chain.push_back(mul);
            if (full) {
                Tensor qs, ks, vs;
                long h, d, h2, d2, h3, d3;
                int ktp = prod_of(kt);
                auto* pm = ktp >= 0 ? attr(ops()[ktp], "perm") : nullptr;
                if (!is(ktp, "Transpose") || !pm || int_list(*pm) != std::vector<int>{0, 2, 1} || use_count(kt.m_name) != 1) goto plain;
                {
                    std::vector<int> c2 = chain;
                    c2.push_back(ktp);
                    if (!head_split_source(q, &qs, &h, &d, &c2) || !head_split_source(ops()[ktp].m_input[0], &ks, &h2, &d2, &c2) ||
                        !head_split_source(v, &vs, &h3, &d3, &c2) || h != h2 || h != h3 || d != d2 || d != d3)
                        goto plain;
                    // merge: Reshape[1,h,T,d] -> Transpose(0,2,1,3) -> Reshape[1,T,h*d]
                    int o0 = sole_consumer(ops()[mm1].m_output[0]);
                    if (!is(o0, "Reshape")) goto plain;
                    {
                        // the first merge Reshape must give [1,h,T,d]: [h,1,T,d] -> Transpose(0,2,1,3) -> [1,T,h*d] keeps the heads one after the other
                        // ([h,T,d] order), which is not the per-token interleave that osg.Attention writes
                        const auto& ms = ops()[o0].m_output[0].m_shape;
                        if (ms.size() != 4 || ms[0] != 1 || (long)ms[1] != h || (long)ms[2] != (long)q.m_shape[1] || (long)ms[3] != d) goto plain;
                    }
                    int o1 = sole_consumer(ops()[o0].m_output[0]);
                    auto* pm2 = o1 >= 0 ? attr(ops()[o1], "perm") : nullptr;
                    if (!is(o1, "Transpose") || !pm2 || int_list(*pm2) != std::vector<int>{0, 2, 1, 3}) goto plain;
                    int o2 = sole_consumer(ops()[o1].m_output[0]);
                    if (!is(o2, "Reshape")) goto plain;
                    const auto& os = ops()[o2].m_output[0].m_shape;
                    if (os.size() != 3 || os[0] != 1 || (long)os[1] != (long)q.m_shape[1] || (long)os[2] != h * d) goto plain;
                    Operation f;
                    f.m_name = ops()[mm0].m_name + "_Attention";
                    f.m_type = "osg.Attention";
                    f.m_input = {qs, ks, vs};
                    f.m_output = {ops()[o2].m_output[0]};
                    char buf[64];
                    snprintf(buf, sizeof buf, "%.9g", scale);
                    f.m_attributes = {{"heads", std::to_string(h)}, {"scale", buf}};
                    for (int k : c2) dead[k] = 1;
                    for (int k : {mm1, o0, o1}) dead[k] = 1;
                    ops()[o2] = std::move(f);
                    continue;
                }
            }
        plain:
            {
                Operation f;
                f.m_name = ops()[mm0].m_name + "_AttentionFusedOps";
                f.m_type = "AttentionFusedOps";
                f.m_input = {q, kt, mul >= 0 ? scale_t : Tensor(), v};
                f.m_output = {ops()[mm1].m_output[0]};
                for (int k : chain) dead[k] = 1;
                ops()[mm1] = std::move(f);
            }
        }
    }

    // osg.Linear(x, W[K,2C], b) -> osg.GEGLU  ==> the GEGLU rides in the GEMM epilogue (value/gate columns pair-interleaved at plan time)
    void fuse_linear_geglu() {
        if (P.stream_weights) return;   // needs a re-ordered resident copy of the weight
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "osg.Linear")) continue;
            Operation& op = ops()[i];
            if (attr(op, "osg_residual") || op.m_output.size() != 1) continue;
            const Val* w = cval(op.m_input[1]);
            if (!w || w->shape.size() != 2 || (w->dtype != OSG_F16 && w->dtype != OSG_U8) || w->shape[1] % 32 || w->shape[0] % 64) continue;   // (uint8: resident codes, interleaved as bytes)
            if (op.m_input.size() > 2 && !op.m_input[2].m_name.empty()) {
                const Val* b = cval(op.m_input[2]);
                if (!b || b->dtype != OSG_F16) continue;
            }
            int ge = sole_consumer(op.m_output[0]);
            if (!is(ge, "osg.GEGLU")) continue;
            Operation f = op;
            f.m_attributes.emplace_back("osg_geglu", "1");
            f.m_output = {ops()[ge].m_output[0]};
            dead[i] = 1;
            ops()[ge] = std::move(f);
        }
    }

    // The row-local tail of a BasicTransformerBlock ==> osg.TBlockTail (one launch, osg_tblock_tail / osg_tchain.hip):
    //   osg.Linear(a1, Wo1, bo1, +x0) = x1 -> osg.LayerNorm -> osg.Linear(Wq2) = q -> osg.Attention(q, k, v) -> osg.Linear(Wo2, bo2, +x1) = x2
    //   -> osg.LayerNorm -> osg.Linear(W1, b1, geglu) -> osg.Linear(W2, b2, +x2) = x3 [-> Reshape -> Transpose(0,3,1,2) -> Conv 1x1 (+ residual) = y]
    // anchored at the cross-attention (k / v do not depend on the rows: they are projections of the text context).  Everything between a1 and x3 / y
    // must have exactly the readers the chain itself accounts for.
    void fuse_tblock_tail() {
        if (P.stream_weights || !m.m_hip_fuse_tblock || P.w8_resident) return;
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "osg.Attention")) continue;
            const Operation& at = ops()[i];
            if (at.m_input.size() != 3 || at.m_output.size() != 1) continue;
            const Tensor q = at.m_input[0], kt = at.m_input[1], vt = at.m_input[2];
            if (q.m_name == kt.m_name || q.m_name == vt.m_name) continue;                    // self-attention: q, k, v are views of one projection
            // q = Linear(LayerNorm(x1)), no residual
            const int lq = prod_of(q);
            if (!is(lq, "osg.Linear") || use_count(q.m_name) != 1 || attr(ops()[lq], "osg_residual") || attr(ops()[lq], "osg_geglu")) continue;
            const int ln2 = prod_of(ops()[lq].m_input[0]);
            if (!is(ln2, "osg.LayerNorm") || use_count(ops()[lq].m_input[0].m_name) != 1) continue;
            const Tensor x1 = ops()[ln2].m_input[0];
            const int lo1 = prod_of(x1);
            if (!is(lo1, "osg.Linear") || !attr(ops()[lo1], "osg_residual") || attr(ops()[lo1], "osg_geglu") || ops()[lo1].m_input.size() != 4 || use_count(x1.m_name) != 2) continue;
            // a2 -> Linear(+x1) = x2
            const int lo2 = sole_consumer(at.m_output[0]);
            if (!is(lo2, "osg.Linear") || !attr(ops()[lo2], "osg_residual") || attr(ops()[lo2], "osg_geglu") || ops()[lo2].m_input.size() != 4) continue;
            if (ops()[lo2].m_input[0].m_name != at.m_output[0].m_name || ops()[lo2].m_input[3].m_name != x1.m_name) continue;
            const Tensor x2 = ops()[lo2].m_output[0];
            if (use_count(x2.m_name) != 2) continue;
            int ln3 = -1, l2 = -1;
            for (int c : consumers[x2.m_name]) { if (is(c, "osg.LayerNorm")) ln3 = c; else if (is(c, "osg.Linear")) l2 = c; }
            if (ln3 < 0 || l2 < 0 || ops()[ln3].m_input[0].m_name != x2.m_name) continue;
            const int l1 = sole_consumer(ops()[ln3].m_output[0]);
            if (!is(l1, "osg.Linear") || !attr(ops()[l1], "osg_geglu") || ops()[l1].m_input[0].m_name != ops()[ln3].m_output[0].m_name) continue;
            if (sole_consumer(ops()[l1].m_output[0]) != l2 || !attr(ops()[l2], "osg_residual") || ops()[l2].m_input.size() != 4) continue;
            if (ops()[l2].m_input[0].m_name != ops()[l1].m_output[0].m_name || ops()[l2].m_input[3].m_name != x2.m_name) continue;
            // operands: f16 resident 2-D weights, f16 vectors
            auto wok = [&](const Operation& lin, long K, long Nn) {
                const Val* w = cval(lin.m_input[1]);
                return w && w->dtype == OSG_F16 && w->shape.size() == 2 && w->shape[0] == K && w->shape[1] == Nn;
            };
            auto vok = [&](const Tensor& t, long n, bool may_be_empty) {
                if (t.m_name.empty()) return may_be_empty;
                const Val* b = cval(t);
                return b && b->dtype == OSG_F16 && b->numel() == n;
            };
            const auto& xs = x1.m_shape;
            if (xs.size() != 3 || xs[0] != 1) continue;
            const long T = (long)xs[1], C = (long)xs[2], F = 4 * C;
            const Operation &O1 = ops()[lo1], &LQ = ops()[lq], &O2 = ops()[lo2], &L1 = ops()[l1], &L2 = ops()[l2];
            if (!wok(O1, C, C) || !wok(LQ, C, C) || !wok(O2, C, C) || !wok(L1, C, 2 * F) || !wok(L2, F, C)) continue;
            if (!vok(O1.m_input[2], C, true) || !vok(O2.m_input[2], C, true) || !vok(L1.m_input.size() > 2 ? L1.m_input[2] : Tensor(), 2 * F, true) || !vok(L2.m_input[2], C, true)) continue;
            if (LQ.m_input.size() > 2 && !vok(LQ.m_input[2], C, true)) continue;
            if (!vok(ops()[ln2].m_input[1], C, false) || !vok(ops()[ln2].m_input[2], C, false) || !vok(ops()[ln3].m_input[1], C, false) || !vok(ops()[ln3].m_input[2], C, false)) continue;
            if (!act(O1.m_input[0]) || !act(O1.m_input[3]) || O1.m_input[0].m_shape != xs || O1.m_input[3].m_shape != xs) continue;
            if (kt.m_shape.size() != 3 || kt.m_shape[0] != 1 || (long)kt.m_shape[2] != C || vt.m_shape != kt.m_shape) continue;
            const long heads = std::stol(*attr(at, "heads")), Tk = (long)kt.m_shape[1];
            if (!be.api.osg_tblock_tail_supported((int)(T * N), (int)T, (int)C, (int)heads, (int)Tk)) continue;
            // optional: x3 -> Reshape -> Transpose(0,3,1,2) -> Conv 1x1 (bias, + residual)
            int cv = -1, rsh = -1, trp = -1;
            {
                const int r0 = sole_consumer(L2.m_output[0]);
                const int t0 = is(r0, "Reshape") ? sole_consumer(ops()[r0].m_output[0]) : -1;
                auto* pm = t0 >= 0 ? attr(ops()[t0], "perm") : nullptr;
                const int c0 = is(t0, "Transpose") && pm && int_list(*pm) == std::vector<int>{0, 3, 1, 2} ? sole_consumer(ops()[t0].m_output[0]) : -1;
                if (is(c0, "Conv")) {
                    const Operation& co = ops()[c0];
                    const Val* w = cval(co.m_input[1]);
                    const auto& rs = ops()[r0].m_output[0].m_shape;
                    bool ok = co.m_input.size() == 4 && attr(co, "osg_residual") && !attr(co, "osg_image_bias") && !attr(co, "osg_act") &&
                              co.m_input[0].m_name == ops()[t0].m_output[0].m_name && w && w->dtype == OSG_F16 && w->shape == Shape{C, C, 1, 1} && vok(co.m_input[2], C, true) &&
                              rs.size() == 4 && rs[0] == 1 && (long)(rs[1] * rs[2]) == T && (long)rs[3] == C && act(co.m_input[3]) && co.m_input[3].m_name != co.m_input[0].m_name;
                    for (auto& a : co.m_attributes) {
                        if (a.first == "pads") { for (int v2 : int_list(a.second)) ok = ok && v2 == 0; }
                        else if (a.first == "strides" || a.first == "dilations" || a.first == "kernel_shape") { for (int v2 : int_list(a.second)) ok = ok && v2 == 1; }
                        else if (a.first == "group") ok = ok && std::stoi(a.second) == 1;
                    }
                    if (ok) { cv = c0; rsh = r0; trp = t0; }
                }
            }
            Operation f;
            f.m_name = at.m_name + "_TBlockTail";
            f.m_type = "osg.TBlockTail";
            const Tensor none;
            f.m_input = {O1.m_input[0], O1.m_input[3], O1.m_input[1], O1.m_input[2], ops()[ln2].m_input[1], ops()[ln2].m_input[2], LQ.m_input[1],
                         LQ.m_input.size() > 2 ? LQ.m_input[2] : none, kt, vt, O2.m_input[1], O2.m_input[2], ops()[ln3].m_input[1], ops()[ln3].m_input[2],
                         L1.m_input[1], L1.m_input.size() > 2 ? L1.m_input[2] : none, L2.m_input[1], L2.m_input[2]};
            f.m_attributes = {{"heads", *attr(at, "heads")}, {"scale", *attr(at, "scale")}, {"eps2", *attr(ops()[ln2], "epsilon")}, {"eps3", *attr(ops()[ln3], "epsilon")},
                              {"proj", cv >= 0 ? "1" : "0"}};
            const int last = cv >= 0 ? cv : l2;
            if (cv >= 0) {
                f.m_input.push_back(ops()[cv].m_input[1]);
                f.m_input.push_back(ops()[cv].m_input[2]);
                f.m_input.push_back(ops()[cv].m_input[3]);
            }
            f.m_output = {ops()[last].m_output[0]};
            for (int k2 : {lo1, ln2, lq, (int)i, lo2, ln3, l1, l2, rsh, trp})
                if (k2 >= 0 && k2 != last) dead[k2] = 1;
            ops()[last] = std::move(f);
        }
    }

    // identical osg.SiLU(x) ops (the 22 resnet blocks each re-activate the SAME time embedding) ==> one
    void cse_silu() {
        std::map<std::string, std::string> first;   // input name -> surviving output name
        std::map<std::string, std::string> rename;
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "osg.SiLU")) continue;
            Operation& op = ops()[i];
            if (op.m_input.size() != 1 || op.m_output.size() != 1 || !act(op.m_input[0])) continue;
            if (use_count(op.m_output[0].m_name) >= 1000) continue;  // an extra output the caller reads
            if (use_count(op.m_output[0].m_name) == 0) continue;     // nobody consumes it: a graph output, read by name through get_tensor
            auto it = first.find(op.m_input[0].m_name);
            if (it == first.end()) first[op.m_input[0].m_name] = op.m_output[0].m_name;
            else {
                rename[op.m_output[0].m_name] = it->second;
                dead[i] = 1;
            }
        }
        if (rename.empty()) return;
        for (size_t i = 0; i < ops().size(); i++) {
            if (dead[i]) continue;
            for (auto& in : ops()[i].m_input) {
                auto it = rename.find(in.m_name);
                if (it != rename.end() && in.m_type == TensorDataType::none) in.m_name = it->second;
            }
        }
    }

    // Conv(x) -> Add(., Unsqueeze(Unsqueeze(g[1,C])))  ==> the per-image channel bias g rides in the conv epilogue
    void fuse_image_bias() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Conv")) continue;
            Operation& op = ops()[i];
            if (op.m_output.size() != 1 || attr(op, "osg_residual")) continue;
            if (attr(op, "osg_act")) continue;   // the epilogue applies the activation LAST: silu(conv) + g is not silu(conv + g)
            int ad = sole_consumer(op.m_output[0]);
            if (!is(ad, "Add")) continue;
            int ti = other(ops()[ad], op.m_output[0].m_name);
            const Tensor& t = ops()[ad].m_input[ti];
            const auto& os = op.m_output[0].m_shape;
            if (!act(t) || os.size() != 4 || t.m_shape != std::vector<size_t>{1, os[1], 1, 1}) continue;
            int u1 = prod_of(t);
            if (!is(u1, "Unsqueeze") || use_count(t.m_name) != 1) continue;
            int u0 = prod_of(ops()[u1].m_input[0]);
            if (!is(u0, "Unsqueeze") || use_count(ops()[u1].m_input[0].m_name) != 1) continue;
            const Tensor g = ops()[u0].m_input[0];
            if (!act(g) || g.m_shape != std::vector<size_t>{1, os[1]} || use_count(g.m_name) != 1) continue;
            Operation f = op;
            while (f.m_input.size() < 4) f.m_input.push_back(Tensor());
            f.m_input.push_back(g);
            f.m_attributes.emplace_back("osg_image_bias", "1");
            f.m_output = {ops()[ad].m_output[0]};
            dead[i] = dead[u0] = dead[u1] = 1;
            ops()[ad] = std::move(f);
        }
    }

    // MatMul(x, W) -> Add(., b[N])  ==> osg.Linear(x, W, b)
    void fuse_linear() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "MatMul")) continue;
            Operation& mm = ops()[i];
            const Val* w = cval(mm.m_input[1]);
            if (!act(mm.m_input[0]) || !w || w->shape.size() != 2) continue;
            mm.m_type = "osg.Linear";
            int ad = sole_consumer(mm.m_output[0]);
            if (!is(ad, "Add")) continue;
            int bi = other(ops()[ad], mm.m_output[0].m_name);
            const Val* b = cval(ops()[ad].m_input[bi]);
            if (!b || b->shape.size() != 1 || b->shape[0] != w->shape[1]) continue;
            Operation f = mm;
            f.m_input.push_back(ops()[ad].m_input[bi]);
            f.m_output = {ops()[ad].m_output[0]};
            dead[i] = 1;
            ops()[ad] = std::move(f);
        }
    }

    // {Conv | osg.Linear}(..) -> Add(., r)  with r an activation of the same shape  ==> residual fused in the epilogue
    void fuse_residual() {
        for (size_t i = 0; i < ops().size(); i++) {
            const bool conv = is((int)i, "Conv"), lin = is((int)i, "osg.Linear");
            if (!conv && !lin) continue;
            Operation& op = ops()[i];
            if (op.m_output.size() != 1) continue;
            if (attr(op, "osg_residual")) continue;   // the op this pass has just written in place of an Add: the epilogue takes ONE residual, a second Add stays an Add
            int ad = sole_consumer(op.m_output[0]);
            if (!is(ad, "Add")) continue;
            int ri = other(ops()[ad], op.m_output[0].m_name);
            const Tensor& r = ops()[ad].m_input[ri];
            if (!act(r) || r.m_shape != op.m_output[0].m_shape || r.m_name == op.m_output[0].m_name) continue;
            if (conv && op.m_output[0].m_shape.size() != 4) continue;   // (a Conv1D is lifted to 2-D inside lower_conv: its residual stays an Add)
            // the residual must already exist when the fused op runs: its producer has to precede `ad` (always true in a
            // topologically sorted file) -- the fused op takes the place of the Add.
            Operation f = op;
            if (conv && f.m_input.size() == 2) f.m_input.push_back(Tensor());  // no bias
            if (lin && f.m_input.size() == 2) f.m_input.push_back(Tensor());
            f.m_input.push_back(r);
            f.m_attributes.emplace_back("osg_residual", "1");
            f.m_output = {ops()[ad].m_output[0]};
            dead[i] = 1;
            ops()[ad] = std::move(f);
        }
    }

    // (fuse_conv_shortcut, the pass behind hip_fuse_shortcut, is defined next to lower_conv in lowering_ops.inc: the two share the fused op's input layout)

    // Conv(..) -> osg.SiLU  ==> the activation rides in the convolution's epilogue (the Conv -> Sigmoid -> Mul triple of every block of
    // the exported YOLOv8 graphs; in the SD UNet SiLU follows the GroupNorms instead)
    void fuse_conv_act() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Conv")) continue;
            Operation& op = ops()[i];
            if (op.m_output.size() != 1 || attr(op, "osg_act")) continue;
            int sl = sole_consumer(op.m_output[0]);
            if (!is(sl, "osg.SiLU") || ops()[sl].m_input.size() != 1) continue;
            Operation f = op;
            f.m_attributes.emplace_back("osg_act", "silu");
            f.m_output = {ops()[sl].m_output[0]};
            dead[i] = 1;
            ops()[sl] = std::move(f);
        }
    }

    // Gemm(..) -> osg.SiLU  ==> the activation rides in the GEMM's epilogue (time_embedding.linear_1 -> act, linear_2 -> the resnets' nonlinearity:
    // two launches of the UNet's time-embedding chain)
    void fuse_gemm_act() {
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Gemm")) continue;
            Operation& op = ops()[i];
            if (op.m_output.size() != 1 || op.m_input.size() != 3 || attr(op, "osg_act")) continue;
            const Val* w = cval(op.m_input[1]);
            if (!w || (w->dtype != OSG_F16 && w->dtype != OSG_U8)) continue;
            int sl = sole_consumer(op.m_output[0]);
            if (!is(sl, "osg.SiLU") || ops()[sl].m_input.size() != 1) continue;
            Operation f = op;
            f.m_attributes.emplace_back("osg_act", "silu");
            f.m_output = {ops()[sl].m_output[0]};
            dead[i] = 1;
            ops()[sl] = std::move(f);
        }
    }

    // ------------------------------------------------------------------------------------------------------------------
    // lowering
    // ------------------------------------------------------------------------------------------------------------------
    int in_val_raw(const Tensor& t) {   // may return a strided column view (Val::ld != 0)
        if (is_const_tensor(t)) return const_val(t);
        auto it = P.by_name.find(t.m_name);
        if (it == P.by_name.end()) throw std::invalid_argument("Model::get_tensor_data: input tensor not found: " + t.m_name);
        const int r = P.root_of(it->second);
        if (V(r).host_only && !V(r).dptr) {   // a plan-time value that a launch wants to read after all: give it device storage now
            const size_t bytes = std::max<size_t>(P.val_bytes(r), 8);
            V(r).dptr = P.small_alloc(bytes);
            if (V(r).dtype == OSG_I64) be.check(be.api.osg_upload_sync(be.ctx, V(r).dptr, V(r).host_i.data(), V(r).host_i.size() * 8), "osg_upload_sync");
            else if (V(r).dtype == OSG_F32 && P.fp16) {
                // the reference's fp32 results are rounded to fp16 when they are pushed with fp16 arithmetic on (push_tensor :3029-3034)
                std::vector<uint16_t> h(V(r).host_f.size());
                for (size_t k = 0; k < h.size(); k++) h[k] = float_to_half(V(r).host_f[k]);
                be.check(be.api.osg_upload_sync(be.ctx, V(r).dptr, h.data(), h.size() * 2), "osg_upload_sync");
                V(r).dtype = OSG_F16;
            } else if (V(r).dtype == OSG_F32) be.check(be.api.osg_upload_sync(be.ctx, V(r).dptr, V(r).host_f.data(), V(r).host_f.size() * 4), "osg_upload_sync");
            else throw std::invalid_argument("Model::get_tensor_data: unsupported tensor data format.");
        }
        return it->second;
    }
    // a constant, or an activation whose VALUE is known at plan time (the Shape -> Gather -> Concat -> Reshape chains exporters leave behind)
    const Val* hval(const Tensor& t) const {
        if (is_const_tensor(t)) return &P.vals[const_val(t)];
        auto it = P.by_name.find(t.m_name);
        if (it == P.by_name.end()) return nullptr;
        const Val& v = P.vals[it->second];
        return v.host_valid && v.host_only ? &v : nullptr;
    }
    int host_val(const Operation& op, const Shape& shape, std::vector<int64_t> ints, std::vector<float> floats = {}) {
        const bool is_int = floats.empty();
        check_out(op, shape);
        int v = P.new_val(op.m_output[0].m_name, shape, is_int ? OSG_I64 : OSG_F32, Lay::plain, false);
        V(v).is_const = true;
        V(v).host_valid = V(v).host_only = true;
        V(v).host_i = std::move(ints);
        V(v).host_f = std::move(floats);
        return v;
    }

    // Ops evaluated on the host while the plan is built: Shape (reference :7003), Range (:7589) and ConstantOfShape (:7543) always; Gather (:6316),
    // Cast (:7352), Concat (:4140), Unsqueeze / Squeeze / Reshape, Slice, Add / Sub / Mul / Div, Neg, Less / Greater / Equal / And (:7637), Where (:7034),
    // Expand (:7154) and Trilu when every operand is known at plan time and at least one of them is a plan-time VALUE (a shape chain, an int64
    // graph input, something computed from those) rather than a weight.  Tensor shapes and int64 inputs are fixed per plan (another shape or
    // another token re-plans), so the shape chains exporters leave behind and the mask / position subgraphs of the LLM graphs fold to
    // constants: int64 or fp32 host tensors that get device storage (fp32 -> f16 under fp16 arithmetic) only if a launch reads them.
    // Returns false when the op has to run on the device.
    struct HT {
        Shape shape;
        bool is_int = true;
        std::vector<double> v;
        long numel() const { return (long)v.size(); }
    };
    static HT to_ht(const Val* v) {
        HT h;
        h.shape = v->shape;
        h.is_int = v->dtype == OSG_I64;
        if (h.is_int) h.v.assign(v->host_i.begin(), v->host_i.end());
        else h.v.assign(v->host_f.begin(), v->host_f.end());
        return h;
    }
    int host_out(const Operation& op, HT h) {
        if (h.is_int) {
            std::vector<int64_t> o(h.v.size());
            for (size_t k = 0; k < o.size(); k++) o[k] = (int64_t)h.v[k];
            return host_val(op, h.shape, std::move(o));
        }
        std::vector<float> f(h.v.size());
        for (size_t k = 0; k < f.size(); k++) f[k] = (float)h.v[k];
        check_out(op, h.shape);
        int v = P.new_val(op.m_output[0].m_name, h.shape, OSG_F32, Lay::plain, false);
        V(v).is_const = true;
        V(v).host_valid = V(v).host_only = true;
        V(v).host_f = std::move(f);
        return v;
    }
    // numpy broadcasting of two host tensors through `fn`
    template <class F>
    HT broadcast2(const Operation& op, const HT& a, const HT& b, bool out_int, F&& fn) {
        const size_t r = std::max(a.shape.size(), b.shape.size());
        Shape as(r, 1), bs(r, 1), os(r, 1);
        std::copy(a.shape.begin(), a.shape.end(), as.begin() + (r - a.shape.size()));
        std::copy(b.shape.begin(), b.shape.end(), bs.begin() + (r - b.shape.size()));
        for (size_t k = 0; k < r; k++) {
            need(op, as[k] == bs[k] || as[k] == 1 || bs[k] == 1, "shapes of A and B not compatible.");
            os[k] = std::max(as[k], bs[k]);
        }
        HT o;
        o.shape = os;
        o.is_int = out_int;
        const long n = prod(os);
        need(op, n <= (1L << 24), "plan-time tensor too large.");
        o.v.resize((size_t)n);
        std::vector<long> idx(r, 0);
        for (long e = 0; e < n; e++) {
            long ia = 0, ib = 0;
            for (size_t k = 0; k < r; k++) {
                ia = ia * as[k] + (as[k] == 1 ? 0 : idx[k]);
                ib = ib * bs[k] + (bs[k] == 1 ? 0 : idx[k]);
            }
            o.v[(size_t)e] = fn(a.v[(size_t)ia], b.v[(size_t)ib]);
            for (long k = (long)r - 1; k >= 0; k--) {
                if (++idx[(size_t)k] < os[(size_t)k]) break;
                idx[(size_t)k] = 0;
            }
        }
        return o;
    }
    bool try_host_eval(const Operation& op) {
        const std::string& t = op.m_type;
        if (t == "Shape") {
            need(op, op.m_input.size() == 1, "wrong number of inputs.");
            need(op, op.m_output.size() == 1, "wrong number of outputs.");
            need(op, op.m_attributes.empty(), "unrecognized attribute (not implemented).");
            const int x = in_val_raw(op.m_input[0]);
            const Shape xs = V(x).shape;
            need(op, !xs.empty(), "shape of input not available.");
            host_val(op, {(long)xs.size()}, std::vector<int64_t>(xs.begin(), xs.end()));
            return true;
        }
        static const char* kOps[] = {"Gather", "Cast", "Concat", "Unsqueeze", "Squeeze", "Reshape", "Slice", "Add", "Sub", "Mul", "Div", "Neg", "Range",
                                     "ConstantOfShape", "Less", "Greater", "Equal", "And", "Where", "Expand", "Trilu"};
        bool known = false;
        for (auto* k : kOps) known |= t == k;
        if (P.decode)   // decode plans: the token and its position exist on the device only -- a Gather may index with them, nothing else may read them
            for (size_t k = 0; k < op.m_input.size(); k++) {
                auto it = op.m_input[k].m_name.empty() || is_const_tensor(op.m_input[k]) ? P.by_name.end() : P.by_name.find(op.m_input[k].m_name);
                if (it == P.by_name.end() || !P.vals[P.root_of(it->second)].dev_int || (t == "Gather" && k == 1)) continue;
                throw std::runtime_error(P.dec_fn() + t + " (" + op.m_name + ") needs the value of '" + P.vals[P.root_of(it->second)].name +
                                         "' while the plan is built; in the device token loop it exists on the device only.");
            }
        if (!known || op.m_input.empty() || op.m_output.size() != 1) return false;
        std::vector<const Val*> in;
        bool any_value = false;
        for (auto& ti : op.m_input) {
            if (ti.m_name.empty()) { in.push_back(nullptr); continue; }
            const Val* v = hval(ti);
            if (!v || !v->host_valid || (v->dtype != OSG_I64 && v->dtype != OSG_F32 && v->host_f.empty())) return false;
            if (v->dtype != OSG_I64 && v->host_f.size() != (size_t)v->numel()) return false;   // (a weight without a host copy)
            any_value |= v->host_only;
            in.push_back(v);
        }
        // at least one operand must be a plan-time VALUE (not merely a small weight): all-weight ops stay on the device path
        if (!any_value || !in[0]) return false;
        // Gather / Slice / Concat / Expand / Unsqueeze / ... move DATA: the data operand itself has to be a plan-time value
        if ((t == "Gather" || t == "Slice" || t == "Unsqueeze" || t == "Squeeze" || t == "Reshape" || t == "Expand" || t == "Cast" || t == "Neg" || t == "Trilu") && !in[0]->host_only)
            return false;
        auto ints = [](const Val* v) { return v->dtype == OSG_I64; };
        auto attr_none = [&] { need(op, op.m_attributes.empty(), "unrecognized attribute (not implemented)."); };
        if (t == "Cast") {
            int to = -1;
            for (auto& a : op.m_attributes) {
                if (a.first == "to") to = std::stoi(a.second);
                else throw std::invalid_argument(op.m_type + ": unrecognized attribute (not implemented).");
            }
            need(op, to != -1, "'to' attribute not found.");
            HT x = to_ht(in[0]);
            if (to == 1) {
                need(op, x.is_int, "wrong data type of input (not implemented).");
                if (x.v.empty()) return false;
                x.is_int = false;
            } else if (to == 9 || to == 7 || to == 6) {
                for (auto& e : x.v) e = (double)(int64_t)e;
                x.is_int = true;
            } else
                throw std::invalid_argument(op.m_type + ": requested cast not implemented.");
            host_out(op, std::move(x));
            return true;
        }
        if (t == "Range") {
            need(op, op.m_input.size() == 3, "wrong number of inputs.");
            attr_none();
            for (int k = 0; k < 3; k++) need(op, in[k] && ints(in[k]) && in[k]->host_i.size() == 1 && in[k]->shape.empty(), "start, limit and delta must be int64 scalars (not implemented).");
            const int64_t st = in[0]->host_i[0], lim = in[1]->host_i[0], dl = in[2]->host_i[0];
            need(op, dl == 1, "delta must be 1 (not implemented).");
            need(op, st < lim, "start must be less than limit.");
            std::vector<int64_t> o;
            for (int64_t k = st; k < lim; k++) o.push_back(k);
            const long n = (long)o.size();
            host_val(op, {n}, std::move(o));
            return true;
        }
        if (t == "ConstantOfShape") {
            need(op, op.m_input.size() == 1, "wrong number of inputs.");
            std::string value;
            for (auto& a : op.m_attributes) {
                if (a.first == "value") value = a.second;
                else throw std::invalid_argument(op.m_type + ": unrecognized attribute (not implemented).");
            }
            need(op, !value.empty(), "'value' attribute not specified (not implemented).");
            need(op, in[0]->shape.size() == 1, "input must be 1D.");
            need(op, ints(in[0]), "wrong data type of input.");
            HT o;
            o.is_int = false;
            for (auto d : in[0]->host_i) o.shape.push_back((long)d);
            need(op, prod(o.shape) <= (1L << 24), "plan-time tensor too large.");
            o.v.assign((size_t)prod(o.shape), (double)std::stof(value));
            host_out(op, std::move(o));
            return true;
        }
        if (t == "Neg") {
            need(op, op.m_input.size() == 1, "wrong number of inputs.");
            HT x = to_ht(in[0]);
            for (auto& e : x.v) e = -e;
            host_out(op, std::move(x));
            return true;
        }
        if (t == "Less" || t == "Greater" || t == "Equal" || t == "And") {
            need(op, op.m_input.size() == 2 && in[1], "wrong number of inputs.");
            attr_none();
            const HT a = to_ht(in[0]), b = to_ht(in[1]);
            // two fp32 operands are compared as fixed point with 4 decimals (reference :7682-7683)
            const double fx = !a.is_int && !b.is_int ? 10000.0 : 1.0;
            const int kind = t == "Less" ? 0 : t == "Greater" ? 1 : t == "Equal" ? 2 : 3;
            host_out(op, broadcast2(op, a, b, true, [&](double x, double y) {
                         const int64_t p = a.is_int ? (int64_t)x : (int64_t)((float)x * (float)fx), q = b.is_int ? (int64_t)y : (int64_t)((float)y * (float)fx);
                         return (double)(kind == 0 ? p < q : kind == 1 ? p > q : kind == 2 ? p == q : (p && q));
                     }));
            return true;
        }
        if (t == "Where") {
            need(op, op.m_input.size() == 3 && in[1] && in[2], "wrong number of inputs.");
            attr_none();
            const HT c = to_ht(in[0]), a = to_ht(in[1]), b = to_ht(in[2]);
            need(op, !c.shape.empty(), "condition cannot be a scalar (not implemented).");
            need(op, c.is_int, "wrong data type of condition (not implemented).");
            need(op, (a.shape.empty() || a.shape == c.shape) && (b.shape.empty() || b.shape == c.shape), "shapes of condition, A and/or B not equal (broadcasting not implemented).");
            HT o;
            o.shape = c.shape;
            o.is_int = a.is_int || b.is_int;     // (an int64 operand makes the result int64, the other one is truncated: reference :7067-7110)
            o.v.resize(c.v.size());
            for (size_t k = 0; k < o.v.size(); k++) {
                double x = c.v[k] != 0.0 ? a.v[a.v.size() == 1 ? 0 : k] : b.v[b.v.size() == 1 ? 0 : k];
                o.v[k] = o.is_int ? (double)(int64_t)x : x;
            }
            host_out(op, std::move(o));
            return true;
        }
        if (t == "Expand") {
            need(op, op.m_input.size() == 2 && in[1], "wrong number of inputs.");
            attr_none();
            need(op, in[1]->shape.size() == 1 && ints(in[1]), "shape must be 1D.");
            HT ones;
            ones.is_int = true;
            for (auto d : in[1]->host_i) { need(op, d > 0, "dimension <= 0."); ones.shape.push_back((long)d); }
            need(op, prod(ones.shape) <= (1L << 24), "plan-time tensor too large.");
            ones.v.assign((size_t)prod(ones.shape), 1.0);
            const HT x = to_ht(in[0]);
            host_out(op, broadcast2(op, x, ones, x.is_int, [](double a, double) { return a; }));
            return true;
        }
        if (t == "Trilu") {
            need(op, op.m_input.size() == 2 && in[1], "wrong number of inputs.");
            for (auto& a : op.m_attributes) {
                if (a.first == "upper") need(op, a.second == "1", "'upper' must be 1 (not implemented).");
                else throw std::invalid_argument(op.m_type + ": unrecognized attribute (not implemented).");
            }
            HT x = to_ht(in[0]);
            need(op, !x.is_int, "wrong data type of input.");
            need(op, x.shape.size() == 2, "input must be 2D (not implemented).");
            need(op, ints(in[1]) && in[1]->shape.empty() && in[1]->host_i.size() == 1, "second input (k) must be a scalar (not implemented).");
            const long w = x.shape[1], h = x.shape[0], k = (long)in[1]->host_i[0];
            for (long y = 0; y < h; y++)
                for (long xx = 0; xx < w; xx++)
                    if (!(xx - k >= y)) x.v[(size_t)(y * w + xx)] = 0.0;
            host_out(op, std::move(x));
            return true;
        }
        if (t == "Gather") {
            need(op, op.m_input.size() == 2 && in[1], "wrong number of inputs.");
            int axis = 0;
            for (auto& a : op.m_attributes) {
                if (a.first == "axis") axis = std::stoi(a.second);
                else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
            }
            need(op, ints(in[1]), "wrong data type of indices.");
            need(op, in[0]->shape.size() == 1 && (axis == 0 || axis == -1), "axis must be 0 (not implemented).");
            const HT x = to_ht(in[0]);
            HT o;
            o.is_int = x.is_int;
            o.shape = in[1]->shape;                       // 0-d indices -> 0-d output, 1-d -> 1-d (reference :6391-6394)
            for (int64_t i : in[1]->host_i) {
                if (i < 0) i += (int64_t)x.v.size();
                need(op, i >= 0 && i < (int64_t)x.v.size(), "invalid index in indices.");
                o.v.push_back(x.v[(size_t)i]);
            }
            host_out(op, std::move(o));
            return true;
        }
        if (t == "Concat") {
            HT o;
            o.is_int = true;
            for (auto* v : in) {
                need(op, v && v->shape.size() <= 1, "invalid shape of inputs.");
                const HT x = to_ht(v);
                o.is_int &= x.is_int;
                o.v.insert(o.v.end(), x.v.begin(), x.v.end());
            }
            o.shape = {(long)o.v.size()};
            host_out(op, std::move(o));
            return true;
        }
        if (t == "Unsqueeze" || t == "Squeeze") {
            HT x = to_ht(in[0]);
            std::vector<long> axes;
            if (op.m_input.size() > 1 && in[1]) {
                need(op, ints(in[1]), "wrong data type of axes.");
                axes.assign(in[1]->host_i.begin(), in[1]->host_i.end());
            } else if (auto* a = attr(op, "axes"))
                for (int k : int_list(*a)) axes.push_back(k);
            need(op, !axes.empty(), "axes cannot be empty (not implemented).");
            const long rank_out = t == "Unsqueeze" ? (long)x.shape.size() + (long)axes.size() : (long)x.shape.size();
            for (auto& a : axes) {
                if (a < 0) a += rank_out;
                need(op, a >= 0 && a < rank_out, "wrong data in axes.");
            }
            std::sort(axes.begin(), axes.end());
            if (t == "Unsqueeze")
                for (long a : axes) x.shape.insert(x.shape.begin() + a, 1);
            else
                for (auto it = axes.rbegin(); it != axes.rend(); ++it) {
                    need(op, x.shape[(size_t)*it] == 1, "wrong data in axes.");
                    x.shape.erase(x.shape.begin() + *it);
                }
            host_out(op, std::move(x));
            return true;
        }
        if (t == "Reshape") {
            need(op, op.m_input.size() == 2 && in[1] && ints(in[1]), "wrong data type of shape.");
            HT x = to_ht(in[0]);
            Shape os;
            long unknown = -1, known_n = 1;
            for (size_t k = 0; k < in[1]->host_i.size(); k++) {
                long dsz = (long)in[1]->host_i[k];
                if (dsz == 0) { need(op, k < x.shape.size(), "invalid shape."); dsz = x.shape[k]; }
                if (dsz == -1) { need(op, unknown < 0, "invalid shape."); unknown = (long)k; os.push_back(1); continue; }
                os.push_back(dsz);
                known_n *= dsz;
            }
            if (unknown >= 0) { need(op, known_n > 0 && x.numel() % known_n == 0, "invalid shape."); os[(size_t)unknown] = x.numel() / known_n; }
            need(op, prod(os) == x.numel(), "invalid shape.");
            x.shape = os;
            host_out(op, std::move(x));
            return true;
        }
        if (t == "Slice") {
            need(op, op.m_input.size() >= 3 && in[1] && in[2] && in[0]->shape.size() == 1 && in[1]->host_i.size() == 1 && in[2]->host_i.size() == 1, "unsupported slice of a plan-time vector (not implemented).");
            if (op.m_input.size() > 4 && in[4]) need(op, in[4]->host_i.size() == 1 && in[4]->host_i[0] == 1, "unsupported steps value(s) (not implemented).");
            HT x = to_ht(in[0]);
            int64_t b = in[1]->host_i[0], e = in[2]->host_i[0];
            const int64_t n = (int64_t)x.v.size();
            if (b < 0) b += n;
            if (e < 0) e += n;
            b = std::min(std::max<int64_t>(b, 0), n);
            e = std::min(std::max<int64_t>(e, 0), n);
            need(op, b < e, "invalid value(s) in starts and/or ends.");
            HT o;
            o.is_int = x.is_int;
            o.shape = {(long)(e - b)};
            o.v.assign(x.v.begin() + b, x.v.begin() + e);
            host_out(op, std::move(o));
            return true;
        }
        // Add / Sub / Mul / Div: int64 when both operands are, else fp32 (numpy broadcasting)
        need(op, op.m_input.size() == 2 && in[1], "wrong number of inputs.");
        const HT a = to_ht(in[0]), b = to_ht(in[1]);
        const bool oi = a.is_int && b.is_int;
        const int kind = t == "Add" ? 0 : t == "Sub" ? 1 : t == "Mul" ? 2 : 3;
        host_out(op, broadcast2(op, a, b, oi, [&](double x, double y) -> double {
                     if (oi) {
                         const int64_t p = (int64_t)x, q = (int64_t)y;
                         if (kind == 3) need(op, q != 0, "division by zero.");
                         return (double)(kind == 0 ? p + q : kind == 1 ? p - q : kind == 2 ? p * q : p / q);
                     }
                     const float p = (float)x, q = (float)y;
                     return (double)(kind == 0 ? p + q : kind == 1 ? p - q : kind == 2 ? p * q : p / q);
                 }));
        return true;
    }

