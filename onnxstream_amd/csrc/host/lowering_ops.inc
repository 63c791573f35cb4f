// part of struct Lowering (plan.cpp): the per-op lowering of the f16 plan -- the dispatcher lower() and every lower_* (Conv / GEMM / attention / normalisation / movement ...),
// output views, merged projections, LayerNorm folding, the fused transformer-block tail.
    void lower(const Operation& op) {
        const std::string& t = op.m_type;
        if (try_host_eval(op)) return;
        if (P.decode && t != "Concat" && t != "ScaledDotProductAttention" && t != "Unsqueeze" && t != "Reshape" && t != "Expand")
            for (auto& ti : op.m_input) if (reads_kv_cap(ti)) refuse_kv_cap(op);   // (only the length-aware launches may read a capacity buffer)
        if (P.u8) return lower_u8(op);
        if (t == "Gather") return lower_gather(op);
        if (t == "Cast") return lower_cast(op);
        if (t == "Conv") {
            conv1d_out = Conv1dOut{};
            lower_conv(op);
            if (conv1d_out.y >= 0) {   // Conv1D: NHWC [1, Lo, 1, O] -> plain [1, O, Lo, 1] = the graph's [1, O, Lo]
                check_out(op, {1, conv1d_out.Cout, conv1d_out.Lo});
                P.alias(P.ensure_plain(conv1d_out.y), {1, conv1d_out.Cout, conv1d_out.Lo}, Lay::plain, op.m_output[0].m_name);
            }
            return;
        }
        if (t == "MatMul") return lower_matmul(op);
        if (t == "osg.Linear") return lower_linear(op);
        if (t == "Gemm") return lower_gemm(op);
        if (t == "Add" || t == "Sub" || t == "Mul" || t == "Div") return lower_binary(op);
        if (t == "Sigmoid" || t == "Erf" || t == "Sqrt" || t == "Sin" || t == "Cos" || t == "Neg" || t == "osg.SiLU") return lower_unary(op);
        if (t == "Pow") return lower_pow(op);
        if (t == "InstanceNormalization") return lower_instance_norm(op);
        if (t == "osg.GroupNorm") return lower_group_norm(op);
        if (t == "osg.LayerNorm") return lower_layer_norm(op);
        if (t == "osg.GEGLU") return lower_geglu(op);
        if (t == "osg.Attention") return lower_attention(op);
        if (t == "osg.TBlockTail") return lower_tblock_tail(op);
        if (t == "AttentionFusedOps") return lower_attention_fused_ops(op);
        if (t == "ScaledDotProductAttention") return lower_sdpa(op);
        if (t == "Expand") return lower_expand(op);
        if (t == "osg.RMSNorm") return lower_rms_norm(op);
        if (t == "osg.RoPE") return lower_rope(op);
        if (t == "ReduceMean") return lower_reduce_mean(op);
        if (t == "Softmax") return lower_softmax(op);
        if (t == "Reshape") return lower_reshape(op);
        if (t == "Flatten") return lower_flatten(op);
        if (t == "Unsqueeze" || t == "Squeeze") return lower_squeeze(op, t == "Unsqueeze");
        if (t == "Transpose") return lower_transpose(op);
        if (t == "Concat") return lower_concat(op);
        if (t == "Split") return lower_split(op);
        if (t == "Slice") return lower_slice(op);
        if (t == "Resize") return lower_resize(op);
        if (t == "MaxPool") return lower_maxpool(op);
        throw std::invalid_argument("Model::run: operation not implemented on the HIP backend: " + t);
    }

    static void need(const Operation& op, bool cond, const char* msg) {
        if (!cond) throw std::invalid_argument(op.m_type + ": " + msg);
    }

    // decode plans: does this operand live in a key/value capacity buffer (rows past the device-side length hold nothing)?
    bool reads_kv_cap(const Tensor& t) const {
        if (!P.decode || t.m_name.empty() || is_const_tensor(t)) return false;
        auto it = P.by_name.find(t.m_name);
        if (it == P.by_name.end()) return false;
        const Val& v = P.vals[P.root_of(it->second)];
        return v.kv_cap || (v.rep_src >= 0 && P.vals[P.root_of(v.rep_src)].kv_cap);
    }
    [[noreturn]] void refuse_kv_cap(const Operation& op) const {
        throw std::runtime_error(P.dec_fn() + op.m_type + " (" + op.m_name + ") reads a key/value cache in a form the device token loop does not implement.");
    }
    // chunk plans: the plan-time mask [C][CAP] of an attention over capacity buffers must be exactly the causal form osg_sdpa_chunk works out of the
    // device-side row -- 0 where j <= CAP - C + i (the stand-in caches hold CAP - C rows), ONE other value elsewhere, which is returned (what the
    // graph's mask holds for a barred key, rounded to f16 as an upload of the mask would round it).  Anything else is refused by name.
    float causal_mask_value(const Operation& op, const Val* hm, long C, long cap) const {
        auto refuse = [&](const std::string& why) {
            throw std::runtime_error(P.dec_fn() + op.m_type + " (" + op.m_name + "): the attention mask is not the causal mask of a chunk of " + std::to_string(C) +
                                     " rows behind " + std::to_string(cap - C) + " cached rows (" + why + "); a sliding window or a padding term is not implemented in the device prefill.");
        };
        if (!hm || hm->dtype == OSG_I64 || (long)hm->host_f.size() != C * cap) refuse("its values are not known while the plan is built");
        bool have = false;
        float masked = -65504.0f;      // (C == 1 bars nothing: the value is never applied)
        for (long i = 0; i < C; i++)
            for (long j = 0; j < cap; j++) {
                const float v = half_to_float(float_to_half(hm->host_f[(size_t)(i * cap + j)]));
                if (j <= cap - C + i) {
                    if (v != 0.0f) refuse("a key at or before its query row is barred");
                    continue;
                }
                if (!(v < 0.0f)) refuse("a key behind its query row is not barred");
                if (have && v != masked) refuse("barred keys hold more than one value");
                masked = v;
                have = true;
            }
        return masked;
    }

    // Conv (reference :4494-4707 -> XnnPack::convolution :1292): group 1, dilation 1, pads re-centred (:1315-1329)
    // GEMM-shaped steps ([M,K] x [N,K]^T, plain epilogue) that can ALSO emit the partial row statistics of their output when a folded
    // LayerNorm turns out to consume it (osg_gemm_rowstats): keyed by the root val they write
    struct RsProducer { size_t step; int a, w, bias, res, y; long M, N, K; };
    std::map<int, RsProducer> rs_producers;
    void note_rs_producer(int a, int w, int bias, int res, int y, long M, long Nn, long K) {
        if (P.fusion < 2 || !P.fuse_ln_gemm || Nn % 32 || K % 64 || Nn > 1280) return;
        rs_producers[P.root_of(y)] = RsProducer{P.steps.size() - 1, a, w, bias, res, y, M, Nn, K};
    }
    // switch the producer of x to the row-statistics variant; returns the [M, N/32, 2] fp32 val or -1
    int upgrade_rs_producer(int x, long rows, long C) {
        auto it = rs_producers.find(P.root_of(x));
        if (it == rs_producers.end()) return -1;
        const RsProducer r = it->second;
        if (r.M != rows || r.N != C || V(x).view_off != 0 || r.step >= P.steps.size()) return -1;
        if (viewed_steps.count(r.step)) return -1;   // (its output also goes into a Concat slot: the row-statistics launch has no output views)
        {
            auto cpit = conv_producers.find(P.root_of(r.y));
            if (cpit != conv_producers.end() && (cpit->second.out->sink[0].off >= 0 || cpit->second.out->sink[1].off >= 0)) return -1;   // (a GroupNorm reads its statistics from this launch's epilogue)
        }
        if (V(r.y).batched != V(x).batched) return -1;
        int rs = P.new_val("", {r.M / (V(x).batched ? N : 1), C / 32, 2}, OSG_F32, Lay::plain, V(x).batched);
        Step& st = P.steps[r.step];
        st.writes.push_back(rs);
        st.what += " +rowstats";
        const int a = r.a, w = r.w, bias = r.bias, res = r.res, y = r.y;
        const long M = r.M, Nn = r.N, K = r.K;
        const std::string what = st.what;
        st.run = [=, this] {
            be.check(be.api.osg_gemm_rowstats(be.ctx, P.ptr(a), P.ptr(w), bias >= 0 ? P.ptr(bias) : nullptr, bias >= 0 ? P.vals[bias].dtype : OSG_F16,
                                              res >= 0 ? P.ptr(res) : nullptr, P.ptr(y), (int)M, (int)Nn, (int)K, OSG_ACT_NONE, (float*)P.ptr(rs)),
                     what.c_str());
        };
        rs_producers.erase(it);
        conv_producers.erase(P.root_of(y));   // (the launch is the row-statistics GEMM now: no output views)
        return rs;
    }

    // ---- output views of the plain f16 convolutions (round 3): a Concat of NHWC tensors along the channels whose operands come straight out of
    // convolutions is not launched at all -- each producer stores its result into ITS column slice of the concatenated buffer (osg_conv2d_nhwc_v):
    // as its only destination when the Concat is its only reader, next to the dense tensor when other layers read it too (the skip connections
    // of the UNet: 12 copy launches and 2 x the tensors' bytes per pass).  The launch closure reads its destinations from `ConvOut` at run time.
    // sink[k]: GroupNorm statistics of what the launch stores to dst (k = 0) / dst2 (k = 1), added up by its epilogue into the plan's statistics block at
    // `off` (osg_set_stat_sinks; lower_group_norm arms the producers of the tensor it normalises)
    struct StatSinkRef { long off = -1; int groups = 0, cpg = 0, ch_off = 0; };
    struct ConvOut { int dst; long dst_ld = 0; size_t dst_off = 0; int dst2 = -1; long dst2_ld = 0; size_t dst2_off = 0; StatSinkRef sink[2]; int sink_hw = 0; bool no_sinks = false; };   // (no_sinks: a producer whose epilogue cannot add statistics up, osg.TBlockTail)
    struct ConcatPart { std::shared_ptr<ConvOut> out; int slot; long ch_off; size_t step; };
    std::map<int, std::vector<ConcatPart>> concat_parts;   // root val of a Concat output whose operands ALL go there by output views -> the convolutions that fill it
    struct ConvProducer { size_t step; std::shared_ptr<ConvOut> out; int y; };
    std::map<int, ConvProducer> conv_producers;   // root val of a convolution's output -> its step
    std::set<size_t> viewed_steps;                // steps whose destinations were redirected (their launch must stay the view-aware one)

    // Conv 3x3 (h) with osg_residual = the sole use of Conv 1x1 (x)  ==> ONE contraction over K = 9 C + Cin2 (osg_conv2d_nhwc_cat): a ResNet's conv2 and its
    // conv_shortcut.  The 1x1 convolution dies; the 3x3 one gains (x, Ws, bs) behind its own three inputs and the mark osg_shortcut; lower_conv adds the two
    // biases up in f32 on the host.  Only where the halo kernel's entry takes the shape (conv_cat_takes) and both weights are resident f16 constants.
    static bool conv_cat_takes(long H, long W, long Cin, long Cin2, long Cout) {
        if (!(W == 8 || W == 16 || W == 32 || W == 64)) return false;
        const long TI = W == 8 ? 2 : 1, TH = 128 / (W * TI);
        if (H % TH || (W == 8 && H != 8)) return false;
        return Cin > 0 && Cin2 > 0 && Cin % 64 == 0 && Cin2 % 64 == 0 && Cout % 4 == 0;
    }
    // kernel / stride / pad / dilation / group of a Conv: all strides == st, all pads == pd, no dilation, no groups
    bool conv_plain_geometry(const Operation& op, int st, int pd) const {
        bool ok = true;
        for (auto& a : op.m_attributes) {
            if (a.first == "pads") { for (int v : int_list(a.second)) ok = ok && v == pd; }
            else if (a.first == "strides") { for (int v : int_list(a.second)) ok = ok && v == st; }
            else if (a.first == "dilations") { for (int v : int_list(a.second)) ok = ok && v == 1; }
            else if (a.first == "group") ok = ok && std::stoi(a.second) == 1;
        }
        if (pd != 0 && !attr(op, "pads")) ok = false;
        return ok;
    }
    void fuse_conv_shortcut() {
        if (!P.fuse_shortcut || P.stream_weights || P.w8_resident) return;
        for (size_t i = 0; i < ops().size(); i++) {
            if (!is((int)i, "Conv")) continue;
            Operation& op = ops()[i];
            if (!attr(op, "osg_residual") || attr(op, "osg_image_bias") || attr(op, "osg_shortcut") || op.m_input.size() != 4 || op.m_output.size() != 1) continue;
            const Val* w = cval(op.m_input[1]);
            if (!w || w->dtype != OSG_F16 || w->shape.size() != 4 || w->shape[2] != 3 || w->shape[3] != 3 || !conv_plain_geometry(op, 1, 1)) continue;
            const int sc = prod_of(op.m_input[3]);
            if (!is(sc, "Conv") || sc == (int)i || use_count(op.m_input[3].m_name) != 1) continue;
            const Operation& so = ops()[sc];
            if (attr(so, "osg_residual") || attr(so, "osg_image_bias") || attr(so, "osg_act") || attr(so, "osg_shortcut") || so.m_output.size() != 1) continue;
            if (so.m_input.size() < 2 || so.m_input.size() > 3 || !act(so.m_input[0]) || !act(op.m_input[0])) continue;
            const Val* ws = cval(so.m_input[1]);
            if (!ws || ws->dtype != OSG_F16 || ws->shape.size() != 4 || ws->shape[2] != 1 || ws->shape[3] != 1 || !conv_plain_geometry(so, 1, 0)) continue;
            const auto& hs = op.m_input[0].m_shape;
            const auto& xs = so.m_input[0].m_shape;
            if (hs.size() != 4 || xs.size() != 4 || hs[0] != 1 || xs[0] != 1 || hs[2] != xs[2] || hs[3] != xs[3]) continue;
            const long C = (long)hs[1], Cin2 = (long)xs[1], Cout = w->shape[0];
            if (w->shape[1] != C || ws->shape[1] != Cin2 || ws->shape[0] != Cout || !conv_cat_takes((long)hs[2], (long)hs[3], C, Cin2, Cout)) continue;
            // both biases (where present) must be readable at plan time: [Cout] constants
            auto bias_ok = [&](const Operation& o) {
                if (o.m_input.size() < 3 || o.m_input[2].m_name.empty()) return true;
                const Val* b = cval(o.m_input[2]);
                return b && b->host_valid && (long)b->host_f.size() == Cout;
            };
            if (!bias_ok(op) || !bias_ok(so)) continue;
            const Tensor none;
            op.m_input[3] = so.m_input[0];
            op.m_input.push_back(so.m_input[1]);
            op.m_input.push_back(so.m_input.size() > 2 ? so.m_input[2] : none);
            for (auto it = op.m_attributes.begin(); it != op.m_attributes.end(); ++it)
                if (it->first == "osg_residual") { op.m_attributes.erase(it); break; }
            op.m_attributes.emplace_back("osg_shortcut", "1");
            dead[sc] = 1;
        }
    }

    struct Conv1dOut { int y = -1; long Cout = 0, Lo = 0; } conv1d_out;
    void lower_conv(const Operation& op) {
        const bool has_res = attr(op, "osg_residual") != nullptr;
        const bool has_ib = attr(op, "osg_image_bias") != nullptr;
        const osg_act cact = attr(op, "osg_act") ? OSG_ACT_SILU : OSG_ACT_NONE;
        const size_t nin = op.m_input.size();
        const bool has_sc = attr(op, "osg_shortcut") != nullptr;   // fuse_conv_shortcut: inputs (h, W, b | -, x, Ws, bs | -)
        need(op, has_sc ? (nin == 6 && !has_res && !has_ib) : (nin == 2 || nin == 3 || (has_res && nin == 4) || (has_ib && nin == 5)), "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        std::vector<int> dil = {1, 1}, ks, pads = {0, 0, 0, 0}, strides = {1, 1};
        int group = 1;
        for (auto& a : op.m_attributes) {
            if (a.first == "dilations") dil = int_list(a.second);
            else if (a.first == "group") group = std::stoi(a.second);
            else if (a.first == "kernel_shape") ks = int_list(a.second);
            else if (a.first == "pads") pads = int_list(a.second);
            else if (a.first == "strides") strides = int_list(a.second);
            else if (a.first == "osg_residual" || a.first == "osg_image_bias" || a.first == "osg_act" || a.first == "osg_shortcut") {}
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        int x = in_val(op.m_input[0]);
        // Conv1D (reference :4521-4544): run as the 2-D convolution over [N, C, L, 1] -- dilations / kernel_shape gain a 1, pads [b, e] become [b, 0, e, 0], the
        // stride is repeated -- and the [N, O, Lo, 1] result is handed on as [N, O, Lo]
        const bool is1d = V(x).shape.size() == 3;
        // (the reference keys the lift on dilations.size() == 1, :4521; here the input's rank decides and a dilations attribute that disagrees with it is refused)
        for (auto& a : op.m_attributes)
            if (a.first == "dilations") need(op, (dil.size() == 1) == is1d, "invalid dilations attribute value.");
        if (is1d) {
            need(op, !has_res && !has_ib, "Conv1D with fused epilogue inputs not implemented on the HIP backend.");
            bool have_pads = false, have_strides = false, have_dil = false;
            for (auto& a : op.m_attributes) { have_pads |= a.first == "pads"; have_strides |= a.first == "strides"; have_dil |= a.first == "dilations"; }
            if (have_dil) { need(op, dil.size() == 1, "invalid dilations attribute value."); dil.push_back(1); }
            if (!ks.empty()) { need(op, ks.size() == 1, "invalid kernel_shape attribute value."); ks.push_back(1); }
            if (have_pads) { need(op, pads.size() == 2, "invalid pads attribute value."); pads = {pads[0], 0, pads[1], 0}; }
            if (have_strides) { need(op, strides.size() == 1, "invalid strides attribute value."); strides.push_back(strides[0]); }
            Shape s4 = V(x).shape;
            s4.push_back(1);
            x = P.alias(P.ensure_plain(x), s4, Lay::plain);
        }
        need(op, V(x).shape.size() == 4, "invalid shape of input.");
        for (int d : dil) need(op, d == 1, "dilations != 1 not supported (not implemented).");
        need(op, group == 1, "group != 1 not supported (not implemented).");
        need(op, pads.size() == 4 && strides.size() == 2, "invalid pads/strides.");
        x = P.ensure_nhwc(x);
        int w = in_val(op.m_input[1]);
        const Shape ws = V(w).shape;  // [O, I, kh, kw] as named in model.txt; data is OHWI
        need(op, V(w).is_const && V(w).lay == Lay::nhwc && ws.size() == 4, "weights must be a static *_nchw.bin tensor.");
        const Shape xs = V(x).shape;
        need(op, xs[0] == 1, "batch size must be 1 (push several samples instead).");
        const long Cin = xs[1], H = xs[2], W = xs[3], Cout = ws[0], KH = ws[2], KW = ws[3];
        need(op, ws[1] == Cin, "invalid shape of weights.");
        if (!ks.empty()) need(op, ks.size() == 2 && ks[0] == KH && ks[1] == KW, "kernel_shape does not match the weights.");
        const int ph = pads[0] + pads[2], pw = pads[1] + pads[3];
        const int pt = ph / 2, pb = ph - pt, pl = pw / 2, pr = pw - pl;
        need(op, strides[0] >= 1 && strides[1] >= 1, "invalid pads/strides.");
        need(op, H + ph >= KH && W + pw >= KW, "kernel larger than the padded input.");   // ((H + ph - KH) / stride would truncate the negative extent to 0: one output row)
        const long Ho = (H + ph - KH) / strides[0] + 1, Wo = (W + pw - KW) / strides[1] + 1;
        int bias = -1;
        if (nin >= 3 && !op.m_input[2].m_name.empty()) {
            bias = in_val(op.m_input[2]);
            need(op, V(bias).numel() == Cout, "invalid shape of bias.");
        }
        int res = -1;
        if (has_res) res = P.ensure_nhwc(in_val(op.m_input[3]));
        int ib = -1;      // per-image channel bias [1,Cout] (may be a column view of the merged time-embedding projection)
        long ib_ld = 0;
        if (has_ib) {
            ib = in_val_raw(op.m_input[4]);
            need(op, V(ib).numel() == Cout && V(ib).dtype == OSG_F16 && V(ib).batched == V(x).batched, "invalid image bias.");
            ib_ld = V(ib).ld ? V(ib).ld : Cout;
        }
        int y = is1d ? P.new_val("", {1, Cout, Ho, Wo}, OSG_F16, Lay::nhwc, V(x).batched) : out_val(op, {1, Cout, Ho, Wo}, Lay::nhwc, V(x).batched);
        if (is1d) conv1d_out = Conv1dOut{y, Cout, Ho};   // (lower() hands the [1, O, Lo, 1] result on as the graph's [1, O, Lo] once the launch is planned)
        const long nb = B(x);
        const int sh = strides[0], sw = strides[1];
        // fuse_conv_shortcut: the 1x1 convolution of x2 rides as a second K segment of this launch (osg_conv2d_nhwc_cat); the two biases, both constants of the
        // model, meet in f32 on the host, once, and reach the epilogue as one f32 vector
        int x2 = -1, w2 = -1;
        long Cin2 = 0;
        if (has_sc) {
            x2 = P.ensure_nhwc(in_val(op.m_input[3]));
            w2 = in_val(op.m_input[4]);
            const Shape x2s = V(x2).shape, w2s = V(w2).shape;
            need(op, KH == 3 && KW == 3 && sh == 1 && sw == 1 && pt == 1 && pl == 1 && pb == 1 && pr == 1 && V(w).dtype == OSG_F16, "a fused shortcut needs a 3x3 / stride 1 / pad 1 convolution with f16 weights.");
            need(op, x2s.size() == 4 && x2s[0] == 1 && x2s[2] == H && x2s[3] == W && V(x2).batched == V(x).batched, "invalid shape of the shortcut's input.");
            Cin2 = x2s[1];
            need(op, V(w2).is_const && V(w2).dtype == OSG_F16 && V(w2).lay == Lay::nhwc && w2s == Shape{Cout, Cin2, 1, 1}, "invalid shape of the shortcut's weights.");
            std::vector<float> sum((size_t)Cout, 0.f);
            // the derived constant's tag names both source tensors and the length: Plan::const_alloc hands the SAME buffer to equal tags (and replaces a buffer
            // whose size differs), so two fused pairs may share one only where they add up the same two vectors
            std::string tag = "shortcut_bias|" + std::to_string(Cout);
            int present = 0;
            for (int bi : {2, 5}) {
                if (op.m_input[bi].m_name.empty()) { tag += "|-"; continue; }
                const Val& b = V(in_val(op.m_input[bi]));
                need(op, b.host_valid && (long)b.host_f.size() == Cout, "invalid shape of bias.");
                for (long c = 0; c < Cout; c++) sum[c] += b.host_f[c];
                tag += "|" + b.name;
                present++;
            }
            bias = -1;                                      // neither convolution has a bias: the launch takes none (no derived constant)
            if (present) {
                bias = P.new_val("", {Cout}, OSG_F32, Lay::plain, false);
                V(bias).is_const = true;
                V(bias).name = tag;
                bool fresh;
                V(bias).dptr = P.const_alloc(tag, (size_t)Cout * 4, &fresh);
                if (fresh) be.check(be.api.osg_upload_sync(be.ctx, V(bias).dptr, sum.data(), sum.size() * 4), "osg_upload_sync");
            }
        }
        std::vector<int> reads = {x, w};
        if (has_sc) { reads.push_back(x2); reads.push_back(w2); }
        if (bias >= 0) reads.push_back(bias);
        if (res >= 0) reads.push_back(res);
        if (ib >= 0) reads.push_back(ib);
        // W8A16 with the codes resident (hip_w8_resident): the same launch -- output views, statistics sinks, per-image bias -- through the entry point that takes
        // uint8 codes + (scale, zero point); the kernels are the tuned ones (osg_gemm_w8.hip, osg_conv3x3_w8.hip)
        const bool w8 = V(w).dtype == OSG_U8;
        const float qs = w8 ? V(w).qscale : 0.f;
        const int qz = w8 ? V(w).qzp : 0;
        auto co = std::make_shared<ConvOut>();
        co->dst = y;
        P.add_step((w8 ? "Conv w8 " : "Conv ") + op.m_name + (has_sc ? " +shortcut" : ""), reads, {y}, [=, this] {
            const ConvOut& o = *co;
            if (o.sink[0].off >= 0 || o.sink[1].off >= 0)
                be.check(be.api.osg_set_stat_sinks(be.ctx, o.sink[0].off >= 0 ? P.gn_stats + o.sink[0].off : nullptr, o.sink[0].groups, o.sink[0].cpg, o.sink[0].ch_off,
                                                   o.sink[1].off >= 0 ? P.gn_stats + o.sink[1].off : nullptr, o.sink[1].groups, o.sink[1].cpg, o.sink[1].ch_off, o.sink_hw),
                         "osg_set_stat_sinks");
            if (w8)
                be.check(be.api.osg_conv2d_nhwc_w8_v(be.ctx, P.ptr(x), P.ptr(w), qs, qz, nullptr, nullptr, bias >= 0 ? P.ptr(bias) : nullptr,
                                                     bias >= 0 ? P.vals[bias].dtype : OSG_F16, ib >= 0 ? P.ptr(ib) : nullptr, ib_ld,
                                                     res >= 0 ? P.ptr(res) : nullptr, (char*)P.ptr(o.dst) + o.dst_off, o.dst_ld,
                                                     o.dst2 >= 0 ? (char*)P.ptr(o.dst2) + o.dst2_off : nullptr, o.dst2_ld, (int)nb, (int)H, (int)W, (int)Cin,
                                                     (int)Cout, (int)KH, (int)KW, sh, sw, pt, pl, pb, pr, cact),
                         "Conv");
            else if (has_sc)
                be.check(be.api.osg_conv2d_nhwc_cat(be.ctx, P.ptr(x), P.ptr(w), P.ptr(x2), P.ptr(w2), (int)Cin2, bias >= 0 ? (const float*)P.ptr(bias) : nullptr, (char*)P.ptr(o.dst) + o.dst_off, o.dst_ld,
                                                    o.dst2 >= 0 ? (char*)P.ptr(o.dst2) + o.dst2_off : nullptr, o.dst2_ld, (int)nb, (int)H, (int)W, (int)Cin, (int)Cout, cact),
                         "Conv +shortcut");
            else
            be.check(be.api.osg_conv2d_nhwc_v(be.ctx, OSG_F16, P.ptr(x), P.ptr(w), bias >= 0 ? P.ptr(bias) : nullptr,
                                              bias >= 0 ? P.vals[bias].dtype : OSG_F16, ib >= 0 ? P.ptr(ib) : nullptr, ib_ld,
                                              res >= 0 ? P.ptr(res) : nullptr, (char*)P.ptr(o.dst) + o.dst_off, o.dst_ld,
                                              o.dst2 >= 0 ? (char*)P.ptr(o.dst2) + o.dst2_off : nullptr, o.dst2_ld, (int)nb, (int)H, (int)W, (int)Cin, (int)Cout,
                                              (int)KH, (int)KW, sh, sw, pt, pl, pb, pr, cact),
                     "Conv");
        });
        P.steps.back().flops = 2.0 * nb * Ho * Wo * Cout * (KH * KW * Cin + Cin2);
        if (V(w).dtype == OSG_F16 || w8) conv_producers[P.root_of(y)] = ConvProducer{P.steps.size() - 1, co, y};
        if (KH == 1 && KW == 1 && sh == 1 && sw == 1 && ph == 0 && pw == 0 && ib < 0 && cact == OSG_ACT_NONE)   // a 1x1 convolution IS a GEMM over the pixels (OHWI == [N,K])
            if (!w8) note_rs_producer(x, w, bias, res, y, nb * Ho * Wo, Cout, Cin);
    }

    // resident [K,N] weight -> [N,K] (done once, at plan time)
    int weight_nk(int w) {
        Val& wv = V(w);
        if (wv.as_nhwc >= 0) return wv.as_nhwc;  // reuse the slot: "K-contiguous twin"
        const long K = wv.shape[0], Nn = wv.shape[1];
        int t = P.new_val("", {Nn, K}, OSG_F16, Lay::plain, false);
        Val& tv = V(t);
        tv.is_const = true;
        tv.name = V(w).name + "|nk";
        size_t bytes = (size_t)K * Nn * 2;
        bool fresh;
        tv.dptr = P.const_alloc(tv.name, bytes, &fresh);
        if (fresh) be.check(be.api.osg_transpose_kn_to_nk(be.ctx, OSG_F16, P.ptr(w), tv.dptr, (int)K, (int)Nn), "osg_transpose_kn_to_nk");
        V(w).as_nhwc = t;
        return t;
    }

    // [K,N] uint8 codes -> [N,K] (done once, at plan time)
    int weight_nk_u8(int w) {
        if (V(w).as_nk_u8 >= 0) return V(w).as_nk_u8;
        const long K = V(w).shape[0], Nn = V(w).shape[1];
        int t = P.new_val("", {Nn, K}, OSG_U8, Lay::plain, false);
        V(t).is_const = true;
        V(t).name = V(w).name + "|nk_u8";
        V(t).qscale = V(w).qscale;
        V(t).qzp = V(w).qzp;
        bool fresh;
        V(t).dptr = P.const_alloc(V(t).name, (size_t)K * Nn, &fresh);
        if (fresh) {
            long shape[2] = {K, Nn};
            int perm[2] = {1, 0};
            be.check(be.api.osg_transpose(be.ctx, 1, P.ptr(w), V(t).dptr, 2, shape, perm), "osg_transpose");
            be.check(be.api.osg_sync(be.ctx), "osg_sync");
        }
        V(w).as_nk_u8 = t;
        return t;
    }

    // W8A16 with the codes resident: wq = [N,K] uint8 codes (a resident weight's K-contiguous twin, the concatenation of a merged group, a GEGLU interleave);
    // qv >= 0: per-column (scale, zero point) vectors -- one val of 2 N floats, scales first -- else the scalars the val carries
    void emit_gemm_w8q(const std::string& what, int a, int wq, int qv, int bias, int res, int y, long M, long Nn, long K, osg_act act_ = OSG_ACT_NONE) {
        const float qs = V(wq).qscale;
        const int qz = V(wq).qzp;
        std::vector<int> reads = {a, wq};
        if (qv >= 0) reads.push_back(qv);
        if (bias >= 0) reads.push_back(bias);
        if (res >= 0) reads.push_back(res);
        P.add_step(what, reads, {y}, [=, this] {
            const float* sc = qv >= 0 ? (const float*)P.ptr(qv) : nullptr;
            be.check(be.api.osg_gemm_w8_v(be.ctx, P.ptr(a), P.ptr(wq), qs, qz, sc, sc ? sc + Nn : nullptr, bias >= 0 ? P.ptr(bias) : nullptr,
                                          bias >= 0 ? P.vals[bias].dtype : OSG_F16, res >= 0 ? P.ptr(res) : nullptr, P.ptr(y), (int)M, (int)Nn, (int)K, act_),
                     what.c_str());
        });
        P.steps.back().flops = 2.0 * M * Nn * K;
    }
    void emit_gemm_w8(const std::string& what, int a, int w, int bias, int res, int y, long M, long Nn, long K, osg_act act_ = OSG_ACT_NONE) {
        emit_gemm_w8q(what, a, weight_nk_u8(w), -1, bias, res, y, M, Nn, K, act_);
    }

    struct LnFold { int x, g, b; float eps; long C; int rs; };   // rs: partial row statistics handed over by the producer of x (-1: none)

    void emit_gemm(const std::string& what, int a, int wnk, int bias, int res, int y, long M, long Nn, long K, long batch, long sa, long sb,
                   long sc, int b_is_nk, osg_act act_ = OSG_ACT_NONE) {
        std::vector<int> reads = {a, wnk};
        if (bias >= 0) reads.push_back(bias);
        if (res >= 0) reads.push_back(res);
        P.add_step(what, reads, {y}, [=, this] {
            be.check(be.api.osg_gemm(be.ctx, OSG_F16, P.ptr(a), P.ptr(wnk), b_is_nk, bias >= 0 ? P.ptr(bias) : nullptr,
                                     bias >= 0 ? P.vals[bias].dtype : OSG_F16, res >= 0 ? P.ptr(res) : nullptr, P.ptr(y), (int)M, (int)Nn,
                                     (int)K, (int)batch, sa, sb, sc, act_),
                     what.c_str());
        });
        P.steps.back().flops = 2.0 * M * Nn * K * batch;
        if (b_is_nk && batch == 1 && V(y).ld == 0 && act_ == OSG_ACT_NONE) note_rs_producer(a, wnk, bias, res, y, M, Nn, K);
    }

    // ---- merged projections: osg.Linear / Gemm ops that read the SAME activation and whose results are only consumed through
    // strided views (attention Q/K/V operands, conv image bias) run as ONE GEMM over the concatenated [sum N_i, K] weight:
    // self-attention Q|K|V (3 launches -> 1), every cross-attention K|V of the net (they all read the text context: 32 -> 1),
    // the 22 time-embedding projections of the resnet blocks (22 -> 1).
    struct LinGroup {
        std::vector<int> members;   // op indices, file order
        std::vector<long> off;      // column offset of each member inside the merged output
        long ntot = 0;
        int y = -1;                 // merged output val [rows, ntot]
    };
    bool indexed = false;   // index_graph() describes the op list being lowered
    std::vector<LinGroup> groups;
    std::map<int, std::pair<int, int>> group_of;   // op index -> (group, slot)

    void plan_linear_groups() {
        if (P.fusion < 2 || P.stream_weights) return;   // streamed weights are consumed as the provider hands them over: no merged copies
        dead.assign(ops().size(), 0);
        index_graph();
        indexed = true;
        std::map<std::string, std::vector<int>> by_key;
        for (size_t i = 0; i < ops().size(); i++) {
            const Operation& op = ops()[i];
            const bool lin = op.m_type == "osg.Linear", gemm = op.m_type == "Gemm";
            if (!lin && !gemm) continue;
            if (attr(op, "osg_residual") || op.m_output.size() != 1 || !act(op.m_input[0])) continue;
            const Val* w = cval(op.m_input[1]);
            if (!w || w->shape.size() != 2 || (w->dtype != OSG_F16 && w->dtype != OSG_U8)) continue;
            if (w->dtype == OSG_U8 && (w->shape[0] % 64 || w->shape[1] % 4)) continue;   // (resident codes: the merged launch takes per-column quantisation vectors)
            const bool has_bias = op.m_input.size() > 2 && !op.m_input[2].m_name.empty();
            if (gemm && (!has_bias || !op.m_attributes.empty())) continue;
            if (has_bias && cval(op.m_input[2]) && cval(op.m_input[2])->dtype != OSG_F16) continue;
            // every consumer must understand a leading dimension
            bool ok = use_count(op.m_output[0].m_name) < 1000;
            auto cit = consumers.find(op.m_output[0].m_name);
            if (cit == consumers.end() || cit->second.empty()) ok = false;
            else
                for (int c : cit->second) {
                    const Operation& co = ops()[c];
                    if (co.m_type == "osg.Attention" || co.m_type == "osg.TBlockTail" || co.m_type == "osg.QAttention") continue;   // (all read k / v through (pointer, row pitch))
                    if (co.m_type == "Conv" && attr(co, "osg_image_bias") && co.m_input.size() >= 5 && co.m_input[4].m_name == op.m_output[0].m_name) continue;
                    ok = false;
                }
            if (!ok) continue;
            by_key[op.m_type + "|" + op.m_input[0].m_name + "|" + std::to_string(w->shape[0]) + (has_bias ? "|b" : "|-") + (w->dtype == OSG_U8 ? "|u8" : "")].push_back((int)i);
        }
        for (auto& kv : by_key) {
            if (kv.second.size() < 2) continue;
            LinGroup g;
            for (int i : kv.second) {
                g.members.push_back(i);
                g.off.push_back(g.ntot);
                g.ntot += cval(ops()[i].m_input[1])->shape[1];
            }
            for (size_t s2 = 0; s2 < g.members.size(); s2++) group_of[g.members[s2]] = {(int)groups.size(), (int)s2};
            groups.push_back(std::move(g));
        }
    }

    // emits the merged GEMM the first time one of its members is lowered; returns the member's column view
    int lower_group_member(const Operation& op, int op_index) {
        auto [gi, slot] = group_of.at(op_index);
        LinGroup& g = groups[gi];
        const Val* w0 = cval(op.m_input[1]);
        const long K = w0->shape[0];
        if (g.y < 0) {
            auto lnit = ln_deferred.find(op.m_input[0].m_name);
            const LnFold* lnf = lnit == ln_deferred.end() ? nullptr : &lnit->second;
            int a = lnf ? lnf->x : P.ensure_plain(in_val(op.m_input[0]));
            const Shape as = V(a).shape;
            need(op, !as.empty() && as.back() == K, "invalid shape of inputs.");
            // concatenated [ntot, K] weight and [ntot] bias, built once from the resident per-op tensors
            const bool w8 = w0->dtype == OSG_U8;     // resident codes: concatenated as codes, each member's (scale, zero point) spread over its columns
            const size_t wes = w8 ? 1 : 2;
            need(op, !(w8 && lnf), "a LayerNorm cannot be folded into uint8 weight codes.");
            int wcat = P.new_val("", {g.ntot, K}, w8 ? OSG_U8 : OSG_F16, Lay::plain, false);
            V(wcat).is_const = true;
            V(wcat).name = "merged|" + op.m_input[0].m_name + "|" + ops()[g.members[0]].m_name + "|" + std::to_string(g.members.size()) + (lnf ? "|ln" : "") + (w8 ? "|u8" : "");   // (a folded copy has a tag of its own)
            bool fresh_w, fresh_b = false;
            V(wcat).dptr = P.const_alloc(V(wcat).name, (size_t)g.ntot * K * wes, &fresh_w);
            int qv = -1;
            std::vector<float> qhost;
            if (w8) {
                qv = P.new_val("", {2, g.ntot}, OSG_F32, Lay::plain, false);
                V(qv).is_const = true;
                bool fresh_q;
                V(qv).dptr = P.const_alloc(V(wcat).name + "|q", (size_t)g.ntot * 8, &fresh_q);
                if (fresh_q) qhost.resize((size_t)g.ntot * 2);
                fresh_w = fresh_w || fresh_q;
            }
            const bool has_bias = op.m_input.size() > 2 && !op.m_input[2].m_name.empty();
            int bcat = -1;
            if (has_bias) {
                bcat = P.new_val("", {g.ntot}, OSG_F16, Lay::plain, false);
                V(bcat).is_const = true;
                V(bcat).dptr = P.const_alloc(V(wcat).name + "|bias", (size_t)g.ntot * 2, &fresh_b);
            }
            for (size_t s2 = 0; (fresh_w || fresh_b) && s2 < g.members.size(); s2++) {
                const Operation& mo = ops()[g.members[s2]];
                int wnk = w8 ? weight_nk_u8(in_val(mo.m_input[1])) : weight_nk(in_val(mo.m_input[1]));
                const long Ni = V(wnk).shape[0];
                be.check(be.api.osg_copy(be.ctx, (char*)V(wcat).dptr + (size_t)g.off[s2] * K * wes, P.ptr(wnk), (size_t)Ni * K * wes), "osg_copy");
                for (long c = 0; !qhost.empty() && c < Ni; c++) {
                    qhost[g.off[s2] + c] = V(wnk).qscale;
                    qhost[g.ntot + g.off[s2] + c] = (float)V(wnk).qzp;
                }
                if (has_bias) {
                    int b = in_val(mo.m_input[2]);
                    need(mo, V(b).numel() == Ni, "invalid shape of bias.");
                    be.check(be.api.osg_copy(be.ctx, (char*)V(bcat).dptr + (size_t)g.off[s2] * 2, P.ptr(b), (size_t)Ni * 2), "osg_copy");
                }
            }
            if (!qhost.empty()) be.check(be.api.osg_upload_sync(be.ctx, V(qv).dptr, qhost.data(), qhost.size() * 4), "osg_upload_sync");
            be.check(be.api.osg_sync(be.ctx), "osg_sync");
            Shape ys = as;
            ys.back() = g.ntot;
            g.y = P.new_val("", ys, OSG_F16, Lay::plain, V(a).batched);
            const long M = prod(as) / K * B(a);
            if (lnf) {
                auto [c1, c2] = ln_fold_weight(*lnf, wcat, bcat, P.ptr(wcat), V(wcat).name);   // the concatenated copy is private: fold in place
                emit_gemm_ln("Linear ln+ merged(" + std::to_string(g.members.size()) + ") " + op.m_name, *lnf, wcat, c1, c2, -1, g.y, M, g.ntot, K, OSG_ACT_NONE);
            } else if (w8)
                emit_gemm_w8q("Linear w8 merged(" + std::to_string(g.members.size()) + ") " + op.m_name, a, wcat, qv, bcat, -1, g.y, M, g.ntot, K);
            else
            emit_gemm("Linear merged(" + std::to_string(g.members.size()) + ") " + op.m_name, a, wcat, bcat, -1, g.y, M, g.ntot, K, 1, 0, 0, 0, 1);
        }
        Shape os = V(g.y).shape;
        os.back() = w0->shape[1];
        check_out(op, os);
        int v = P.alias(g.y, os, Lay::plain, op.m_output[0].m_name);
        V(v).ld = g.ntot;
        V(v).view_off = (size_t)g.off[slot] * 2;
        V(v).is_const = false;
        return v;
    }

    // MatMul with a static 2-D weight, optional fused bias / residual
    // [N,K] weight (and bias) re-ordered so that rows 32k..32k+15 are value columns 16k.. and rows 32k+16..32k+31 the matching gate
    // columns (N = 2C): what the GEGLU GEMM epilogue expects
    std::pair<int, int> geglu_interleave(int wnk, int bias, const std::string& suffix) {
        const long Nn = V(wnk).shape[0], K = V(wnk).shape[1], C = Nn / 2;
        const bool w8 = V(wnk).dtype == OSG_U8;   // (resident codes: the same row interleave on bytes; one (scale, zero point) for the whole tensor)
        const int wes = w8 ? 1 : 2;
        int wi = P.new_val("", {Nn, K}, w8 ? OSG_U8 : OSG_F16, Lay::plain, false);
        V(wi).is_const = true;
        V(wi).name = V(wnk).name + "|geglu" + suffix;
        V(wi).qscale = V(wnk).qscale;
        V(wi).qzp = V(wnk).qzp;
        bool fresh;
        V(wi).dptr = P.const_alloc(V(wi).name, (size_t)Nn * K * wes, &fresh);
        if (fresh) {
            be.check(be.api.osg_copy_2d(be.ctx, wes, P.ptr(wnk), 16 * K, 0, V(wi).dptr, 32 * K, 0, C / 16, 16 * K), "osg_copy_2d");
            be.check(be.api.osg_copy_2d(be.ctx, wes, P.ptr(wnk), 16 * K, C * K, V(wi).dptr, 32 * K, 16 * K, C / 16, 16 * K), "osg_copy_2d");
        }
        int bi = -1;
        if (bias >= 0) {
            bi = P.new_val("", {Nn}, OSG_F16, Lay::plain, false);
            V(bi).is_const = true;
            V(bi).dptr = P.const_alloc(V(wi).name + "|bias", (size_t)Nn * 2, &fresh);
            if (fresh) {
                be.check(be.api.osg_copy_2d(be.ctx, 2, P.ptr(bias), 16, 0, V(bi).dptr, 32, 0, C / 16, 16), "osg_copy_2d");
                be.check(be.api.osg_copy_2d(be.ctx, 2, P.ptr(bias), 16, C, V(bi).dptr, 32, 16, C / 16, 16), "osg_copy_2d");
            }
        }
        be.check(be.api.osg_sync(be.ctx), "osg_sync");
        return {wi, bi};
    }

    void lower_linear(const Operation& op) {
        auto lnit = ln_deferred.find(op.m_input[0].m_name);
        const LnFold* lnf = lnit == ln_deferred.end() ? nullptr : &lnit->second;
        if (attr(op, "osg_geglu")) {
            int a = lnf ? lnf->x : P.ensure_plain(in_val(op.m_input[0]));
            int w = in_val(op.m_input[1]);
            const Shape as = V(a).shape;
            const long K = V(w).shape[0], Nn = V(w).shape[1];
            need(op, !as.empty() && as.back() == K, "invalid shape of inputs.");
            int bias = op.m_input.size() > 2 && !op.m_input[2].m_name.empty() ? in_val(op.m_input[2]) : -1;
            const bool w8 = V(w).dtype == OSG_U8;
            need(op, !(w8 && lnf), "a LayerNorm cannot be folded into uint8 weight codes.");
            auto [wi, bi] = geglu_interleave(w8 ? weight_nk_u8(w) : weight_nk(w), bias, lnf ? ln_tag(*lnf, bias) : std::string());
            Shape os = as;
            os.back() = Nn / 2;
            int y = out_val(op, os, Lay::plain, V(a).batched);
            const long M = prod(as) / K * B(a);
            if (w8) {
                emit_gemm_w8q("Linear+GEGLU w8 " + op.m_name, a, wi, -1, bi, -1, y, M, Nn, K, OSG_ACT_GEGLU);
                return;
            }
            if (lnf) {
                auto [c1, c2] = ln_fold_weight(*lnf, wi, bi, P.ptr(wi), V(wi).name);   // the interleaved copy is private: fold in place
                emit_gemm_ln("Linear+GEGLU ln+ " + op.m_name, *lnf, wi, c1, c2, -1, y, M, Nn, K, OSG_ACT_GEGLU);
                return;
            }
            std::vector<int> reads = {a, wi};
            if (bi >= 0) reads.push_back(bi);
            const std::string what = "Linear+GEGLU " + op.m_name;
            P.add_step(what, reads, {y}, [=, this] {
                be.check(be.api.osg_gemm(be.ctx, OSG_F16, P.ptr(a), P.ptr(wi), 1, bi >= 0 ? P.ptr(bi) : nullptr, OSG_F16, nullptr, P.ptr(y), (int)M,
                                         (int)Nn, (int)K, 1, 0, 0, 0, OSG_ACT_GEGLU),
                         what.c_str());
            });
            P.steps.back().flops = 2.0 * M * Nn * K;
            return;
        }
        const bool has_res = attr(op, "osg_residual") != nullptr;
        int a = lnf ? lnf->x : P.ensure_plain(in_val(op.m_input[0]));
        int w = in_val(op.m_input[1]);
        const Shape as = V(a).shape;
        const long K = V(w).shape[0], Nn = V(w).shape[1];
        need(op, !as.empty() && as.back() == K, "invalid shape of inputs.");
        int bias = op.m_input.size() > 2 && !op.m_input[2].m_name.empty() ? in_val(op.m_input[2]) : -1;
        int res = has_res ? P.ensure_plain(in_val(op.m_input[3])) : -1;
        Shape os = as;
        os.back() = Nn;
        int y = out_val(op, os, Lay::plain, V(a).batched);
        const long M = prod(as) / K * B(a);
        if (lnf) {
            const int wnk = weight_nk(w);
            const int wf = private_copy(wnk, ln_tag(*lnf, bias));
            auto [c1, c2] = ln_fold_weight(*lnf, wnk, bias, P.ptr(wf), V(wf).name);
            emit_gemm_ln("Linear ln+ " + op.m_name, *lnf, wf, c1, c2, res, y, M, Nn, K, OSG_ACT_NONE);
            return;
        }
        if (V(w).dtype == OSG_U8) emit_gemm_w8("Linear w8 " + op.m_name, a, w, bias, res, y, M, Nn, K);
        else if (P.stream_weights) emit_gemm("Linear " + op.m_name, a, w, bias, res, y, M, Nn, K, 1, 0, 0, 0, 0);   // [K,N] as streamed; the kernel re-lays it out
        else emit_gemm("Linear " + op.m_name, a, weight_nk(w), bias, res, y, M, Nn, K, 1, 0, 0, 0, 1);
    }

    // MatMul (reference :5669-5861): [.., M,K] x [K,N] (static weight, broadcast) or batched [n,M,K] x [n,K,N]
    void lower_matmul(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        int b = in_val(op.m_input[1]);
        if (V(b).is_const && V(b).shape.size() == 2) return lower_linear(op);
        int a = P.ensure_plain(in_val(op.m_input[0]));
        b = P.ensure_plain(b);
        Shape as = V(a).shape, bs = V(b).shape;
        bool lead1 = false;
        if (as.size() == 4 && as[0] == 1) { as.erase(as.begin()); lead1 = true; }
        if (bs.size() == 4 && bs[0] == 1) bs.erase(bs.begin());
        need(op, as.size() == 3 && bs.size() == 3 && as[0] == bs[0] && as[2] == bs[1], "invalid shape of inputs.");
        const long n = as[0], M = as[1], K = as[2], Nn = bs[2];
        Shape os = {n, M, Nn};
        if (lead1) os.insert(os.begin(), 1);
        const bool batched = V(a).batched || V(b).batched;
        int y = out_val(op, os, Lay::plain, batched);
        const long batch = n * (batched ? N : 1);
        // an operand that is not batched is re-read for every sample: stride 0 across samples is not expressible with one
        // stride, so require both or neither when N > 1
        need(op, N == 1 || (V(a).batched == V(b).batched), "mixing per-sample and shared dynamic operands is not implemented.");
        emit_gemm("MatMul " + op.m_name, a, b, -1, -1, y, M, Nn, K, batch, M * K, K * Nn, M * Nn, 0);
    }

    // Gemm (reference :4300-4375): A[1,K] x B[K,N] + bias, no alpha/beta/trans
    void lower_gemm(const Operation& op) {
        need(op, op.m_input.size() == 3, "wrong number of inputs. 2 inputs case not implemented.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        for (auto& a : op.m_attributes) {
            if (a.first == "alpha" || a.first == "beta") need(op, std::stof(a.second) == 1.0f, (a.first + " != 1 case not implemented.").c_str());
            else if (a.first == "transA" || a.first == "transB") need(op, std::stoi(a.second) == 0, (a.first + " != 0 case not implemented.").c_str());
            else if (a.first == "osg_act") {}
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        int a = P.ensure_plain(in_val(op.m_input[0]));
        int w = in_val(op.m_input[1]);
        int bias = in_val(op.m_input[2]);
        need(op, V(w).is_const && V(w).shape.size() == 2 && V(a).shape.size() == 2, "not implemented (shape of inputs).");
        const long M = V(a).shape[0], K = V(a).shape[1], Nn = V(w).shape[1];
        need(op, V(w).shape[0] == K, "invalid shape of inputs.");
        need(op, M == 1 && V(bias).numel() == Nn, "invalid shape of bias.");
        int y = out_val(op, {M, Nn}, Lay::plain, V(a).batched);
        const osg_act gact = attr(op, "osg_act") ? OSG_ACT_SILU : OSG_ACT_NONE;   // (fuse_gemm_act only marks f16-weight Gemms)
        if (V(w).dtype == OSG_U8) emit_gemm_w8("Gemm w8 " + op.m_name, a, w, bias, -1, y, M * B(a), Nn, K, gact);
        else if (P.stream_weights) emit_gemm("Gemm " + op.m_name, a, w, bias, -1, y, M * B(a), Nn, K, 1, 0, 0, 0, 0, gact);
        else emit_gemm("Gemm " + op.m_name, a, weight_nk(w), bias, -1, y, M * B(a), Nn, K, 1, 0, 0, 0, 1, gact);
    }

    // Add/Sub/Mul/Div with NumPy broadcasting (reference :3906-4000, :5056-5175, :5394-5477, :5605-5668)
    void lower_binary(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        int a = in_val(op.m_input[0]), b = in_val(op.m_input[1]);
        const osg_dtype adt = cur_up ? OSG_F32 : OSG_F16;   // (a flagged op runs in fp32 on upcast operands, m_requires_upcast)
        need(op, V(a).dtype == adt && V(b).dtype == adt, "wrong data type of inputs (only the arithmetic type is supported on the device).");
        const osg_binary_kind kind = op.m_type == "Add" ? OSG_BIN_ADD : op.m_type == "Sub" ? OSG_BIN_SUB : op.m_type == "Mul" ? OSG_BIN_MUL : OSG_BIN_DIV;
        // logical output shape (right-aligned broadcast, :855-876)
        const Shape as = V(a).shape, bs = V(b).shape;
        const size_t rank = std::max(as.size(), bs.size());
        Shape os(rank);
        for (size_t i = 0; i < rank; i++) {
            long da = i + as.size() >= rank ? as[i + as.size() - rank] : 1;
            long db = i + bs.size() >= rank ? bs[i + bs.size() - rank] : 1;
            need(op, da == db || da == 1 || db == 1, "shapes are not broadcastable.");
            os[i] = da == 0 || db == 0 ? 0 : std::max(da, db);   // (NumPy: an extent of 0 against 1 is 0 -- an operand without elements has nothing to stretch)
        }
        const bool batched = V(a).batched || V(b).batched;
        if (prod(os) == 0) {   // an empty operand (the zero-length caches of the LLM flow's first call; its declared 0 is a wildcard for check_out): an empty result, no launch
            const osg_dtype edt = cur_up ? OSG_F32 : OSG_F16;
            V(out_val(op, os, Lay::plain, batched, edt)).up32 = edt == OSG_F32;
            return;
        }
        // ---- NHWC-aware fast paths: keep the conv layout when the other operand is per-channel / same-layout ----
        auto per_channel = [&](int v, long C) {  // logical [C,1,1] / [1,C,1,1] / scalar
            const Shape& s = V(v).shape;
            if (V(v).lay == Lay::nhwc) return false;
            if (V(v).numel() == 1) return true;
            if (V(v).numel() != C) return false;
            return (s.size() == 3 && s[0] == C) || (s.size() == 4 && s[1] == C);
        };
        Lay olay = Lay::plain;
        Shape pa, pb;  // physical shapes handed to the kernel (without the batch dim)
        if (V(a).lay == Lay::nhwc || V(b).lay == Lay::nhwc) {
            int x = V(a).lay == Lay::nhwc ? a : b, o = x == a ? b : a;
            const Shape xs = V(x).shape;
            const long C = xs[1], HW = xs[2] * xs[3];
            if (V(o).lay == Lay::nhwc && V(o).shape == xs) {
                olay = Lay::nhwc;
                pa = pb = {HW, C};
            } else if (per_channel(o, C) && os == xs) {
                olay = Lay::nhwc;
                Shape px = {HW, C}, po = {1, V(o).numel() == 1 ? 1 : C};
                pa = x == a ? px : po;
                pb = x == a ? po : px;
            } else {
                a = P.ensure_plain(a);
                b = P.ensure_plain(b);
            }
        }
        if (olay == Lay::plain) { pa = V(a).shape; pb = V(b).shape; }
        int y = out_val(op, os, olay, batched, adt);
        V(y).up32 = adt == OSG_F32;
        // prepend the sample dim
        const size_t prank = std::max(pa.size(), pb.size()) + 1;
        need(op, prank <= 6, "rank too large for the device broadcast kernel.");
        std::vector<long> sa(prank, 1), sb(prank, 1);
        for (size_t i = 0; i < pa.size(); i++) sa[prank - pa.size() + i] = pa[i];
        for (size_t i = 0; i < pb.size(); i++) sb[prank - pb.size() + i] = pb[i];
        sa[0] = B(a);
        sb[0] = B(b);
        P.add_step(op.m_type + " " + op.m_name, {a, b}, {y}, [=, this] {
            be.check(be.api.osg_binary(be.ctx, adt, kind, P.ptr(a), sa.data(), P.ptr(b), sb.data(), P.ptr(y), (int)prank), op.m_type.c_str());
        });
    }

    void lower_rms_norm(const Operation& op) {
        const int x = P.ensure_plain(in_val(op.m_input[0])), w = in_val(op.m_input[1]);
        need(op, V(x).dtype == OSG_F16 && V(w).dtype == OSG_F16, "wrong data type of input.");
        const Shape s = V(x).shape;
        need(op, !s.empty() && V(w).numel() == s.back(), "invalid shape of the weight.");
        const float eps = std::stof(*attr(op, "epsilon"));
        const int y = out_val(op, s, Lay::plain, V(x).batched);
        const long C = s.back(), rows = P.total_elems(x) / C;
        P.add_step("RMSNorm " + op.m_name, {x, w}, {y}, [=, this] { be.check(be.api.osg_rms_norm(be.ctx, OSG_F16, P.ptr(x), P.ptr(w), P.ptr(y), rows, (int)C, eps), "RMSNorm"); });
    }

    void lower_rope(const Operation& op) {
        const int x = P.ensure_plain(in_val(op.m_input[0])), cs = P.ensure_plain(in_val(op.m_input[1])), sn = P.ensure_plain(in_val(op.m_input[2]));
        need(op, V(x).dtype == OSG_F16 && V(cs).dtype == OSG_F16 && V(sn).dtype == OSG_F16, "wrong data type of input.");
        const Shape s = V(x).shape;
        need(op, s.size() >= 2, "invalid shape of input.");
        const long d = s.back(), T = s[s.size() - 2];
        // (tables of their own per sample: the positions of a decode plan of N sequences -- osg_rope_batch)
        const bool per_sample = V(cs).batched && V(sn).batched && V(x).batched && N > 1;
        need(op, d % 2 == 0 && V(cs).numel() == T * d && V(sn).numel() == T * d && (per_sample || (!V(cs).batched && !V(sn).batched)),
             "cos / sin must be [.., T, d] tables shared by every head.");
        {   // (leading dims of the tables must be 1: one table row per token)
            const Shape cshape = V(cs).shape;
            need(op, cshape.size() >= 2 && cshape.back() == d && cshape[cshape.size() - 2] == T, "invalid shape of the cos / sin tables.");
        }
        const int y = out_val(op, s, Lay::plain, V(x).batched);
        const long bh = P.total_elems(x) / (T * d);
        if (per_sample) {
            const long nb = N, heads = bh / nb;
            P.add_step("RoPE(batch) " + op.m_name, {x, cs, sn}, {y}, [=, this] {
                be.check(be.api.osg_rope_batch(be.ctx, OSG_F16, P.ptr(x), P.ptr(cs), P.ptr(sn), P.ptr(y), nb, heads, T, (int)d), "RoPE");
            });
            return;
        }
        P.add_step("RoPE " + op.m_name, {x, cs, sn}, {y}, [=, this] { be.check(be.api.osg_rope(be.ctx, OSG_F16, P.ptr(x), P.ptr(cs), P.ptr(sn), P.ptr(y), bh, T, (int)d), "RoPE"); });
    }

    // Expand (reference :7154-7230): numpy-style broadcast of the input to `shape` (a plan-time int64 vector).  On the device: x * ones, where
    // `ones` has the target extent in every dimension the input stretches (x * 1 is exact for every f16 value, the sign of zero included)
    // Expand [1,Hkv,1,S,d] -> [1,Hkv,rep,S,d] whose result reaches nothing but the key / value input of ScaledDotProductAttention ops, through Reshapes
    // (to [1,Hkv*rep,S,d]): the transformers `repeat_kv` of a grouped-query model.  Such an Expand is not launched (lower_sdpa reads its source).
    bool repeat_kv_only(const Operation& op, const Shape& xs, const Shape& os) {
        if (!P.sdp_attn || os.size() != 5 || xs.size() != 5 || os[0] != 1 || xs[2] != 1 || os[2] < 2) return false;
        for (int k : {0, 1, 3, 4})
            if (xs[k] != os[k]) return false;
        auto consumers_of = [&](const std::string& name) {
            std::vector<std::pair<int, int>> c;   // (op, input slot)
            auto slots = [&](int i) {
                for (size_t k = 0; k < ops()[i].m_input.size(); k++)
                    if (ops()[i].m_input[k].m_name == name) c.push_back({i, (int)k});
            };
            if (indexed) {
                auto it = consumers.find(name);
                if (it != consumers.end())
                    for (int i : it->second) slots(i);
            } else
                for (size_t i = 0; i < ops().size(); i++)
                    if (dead.empty() || !dead[i]) slots((int)i);
            return c;
        };
        for (auto& e : P.extra_outputs)
            if (e == op.m_output[0].m_name) return false;
        const auto c1 = consumers_of(op.m_output[0].m_name);
        if (c1.empty()) return false;
        for (auto [ri, rk] : c1) {
            const Operation& r = ops()[ri];
            if (r.m_type != "Reshape" || rk != 0 || r.m_output.size() != 1) return false;
            for (auto& e : P.extra_outputs)
                if (e == r.m_output[0].m_name) return false;
            const auto c2 = consumers_of(r.m_output[0].m_name);
            if (c2.empty()) return false;
            for (auto [si, sk] : c2)
                if (ops()[si].m_type != "ScaledDotProductAttention" || (sk != 1 && sk != 3)) return false;
        }
        return true;
    }

    void lower_expand(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        need(op, op.m_attributes.empty(), "unrecognized attribute (not implemented).");
        const Val* sv = hval(op.m_input[1]);
        need(op, sv && sv->dtype == OSG_I64 && sv->host_valid, "wrong data type of shape.");
        need(op, sv->shape.size() == 1, "shape must be 1D.");
        const int x = P.ensure_plain(in_val(op.m_input[0]));
        need(op, V(x).dtype == OSG_F16, "wrong data type of input (only the arithmetic type is supported on the device).");
        Shape xs = V(x).shape;
        Shape ts(sv->host_i.begin(), sv->host_i.end());
        need(op, xs.size() <= ts.size(), "invalid shape of input.");
        while (xs.size() < ts.size()) xs.insert(xs.begin(), 1);
        Shape os(ts.size()), on(ts.size(), 1);
        for (size_t k = 0; k < ts.size(); k++) {
            need(op, ts[k] > 0, "dimension <= 0.");
            need(op, xs[k] == ts[k] || xs[k] == 1 || ts[k] == 1, "shape of input not matching 'shape'.");
            os[k] = std::max(xs[k], ts[k]);
            if (xs[k] == 1 && ts[k] > 1) on[k] = ts[k];
        }
        const int y = out_val(op, os, Lay::plain, V(x).batched);
        if (repeat_kv_only(op, xs, os)) {   // grouped-query attention's repeat_kv: the attention kernel maps query head h to kv head h / rep itself
            V(y).rep_src = x;
            V(y).rep = os[2];
            return;
        }
        if (reads_kv_cap(op.m_input[0])) refuse_kv_cap(op);
        const size_t prank = os.size() + 1;
        need(op, prank <= 6, "rank too large for the device broadcast kernel.");
        const long n_ones = prod(on);
        const int ones = P.new_val("", on, OSG_F16, Lay::plain, false);
        V(ones).is_const = true;
        bool fresh;
        V(ones).dptr = P.const_alloc("", std::max<size_t>((size_t)n_ones * 2, 8), &fresh);
        std::vector<uint16_t> h((size_t)n_ones, float_to_half(1.0f));
        be.check(be.api.osg_upload_sync(be.ctx, V(ones).dptr, h.data(), h.size() * 2), "osg_upload_sync");
        std::vector<long> sa(prank, 1), sb(prank, 1);
        for (size_t k = 0; k < xs.size(); k++) { sa[k + 1] = xs[k]; sb[k + 1] = on[k]; }
        sa[0] = B(x);
        P.add_step("Expand " + op.m_name, {x, ones}, {y}, [=, this] {
            be.check(be.api.osg_binary(be.ctx, OSG_F16, OSG_BIN_MUL, P.ptr(x), sa.data(), P.ptr(ones), sb.data(), P.ptr(y), (int)prank), "Expand");
        });
    }

    void lower_unary(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        int x = in_val(op.m_input[0]);
        const osg_dtype adt = cur_up ? OSG_F32 : OSG_F16;
        need(op, V(x).dtype == adt, "wrong data type of input.");
        const std::string& t = op.m_type;
        const osg_unary_kind k = t == "Sigmoid" ? OSG_UN_SIGMOID : t == "Erf" ? OSG_UN_ERF : t == "Sqrt" ? OSG_UN_SQRT : t == "Sin" ? OSG_UN_SIN
                                 : t == "Cos" ? OSG_UN_COS : t == "Neg" ? OSG_UN_NEG : OSG_UN_SILU;
        int y = out_val(op, V(x).shape, V(x).lay, V(x).batched, adt);
        V(y).up32 = adt == OSG_F32;
        const long n = P.total_elems(x);
        P.add_step(t + " " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_unary(be.ctx, adt, k, P.ptr(x), P.ptr(y), n, 0.f), t.c_str()); });
    }

    // Pow (reference :5478-5604): scalar exponent only
    void lower_pow(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        int x = in_val(op.m_input[0]);
        float p = 0;
        need(op, const_scalar(op.m_input[1], &p) && cval(op.m_input[1])->shape.empty(), "power must be a scalar (not implemented).");
        const osg_dtype adt = cur_up ? OSG_F32 : OSG_F16;
        need(op, V(x).dtype == adt, "wrong data type of input.");
        int y = out_val(op, V(x).shape, V(x).lay, V(x).batched, adt);
        V(y).up32 = adt == OSG_F32;
        const long n = P.total_elems(x);
        P.add_step("Pow " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_unary(be.ctx, adt, OSG_UN_POW, P.ptr(x), P.ptr(y), n, p), "Pow"); });
    }

    // InstanceNormalization (reference :4788-5055): input [1,G,L]
    void lower_instance_norm(const Operation& op) {
        need(op, op.m_input.size() == 3, "wrong number of inputs.");
        int x = P.ensure_plain(in_val(op.m_input[0]));
        int sc = in_val(op.m_input[1]), bi = in_val(op.m_input[2]);
        const Shape s = V(x).shape;
        need(op, s.size() == 3 && s[0] == 1, "input shape must be [1,G,L] (not implemented).");
        need(op, V(sc).numel() == s[1] && V(bi).numel() == s[1] && V(sc).dtype == OSG_F32 && V(bi).dtype == OSG_F32, "invalid scale/bias.");
        float eps = 1e-5f;
        for (auto& a : op.m_attributes) {
            if (a.first == "epsilon") eps = std::stof(a.second);
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        int y = out_val(op, s, Lay::plain, V(x).batched);
        const long rows = s[1] * B(x), L = s[2], G = s[1];
        P.add_step("InstanceNorm " + op.m_name, {x, sc, bi}, {y}, [=, this] {
            be.check(be.api.osg_instance_norm(be.ctx, OSG_F16, P.ptr(x), (const float*)P.ptr(sc), (const float*)P.ptr(bi), P.ptr(y), (int)rows, L,
                                              (int)G, eps),
                     "InstanceNormalization");
        });
    }

    void lower_group_norm(const Operation& op) {
        int x = P.ensure_nhwc(in_val(op.m_input[0]));
        int g = in_val(op.m_input[1]), b = in_val(op.m_input[2]);
        const Shape s = V(x).shape;
        const long G = std::stol(*attr(op, "groups"));
        const float eps = std::stof(*attr(op, "epsilon"));
        const int act = *attr(op, "silu") == "1" ? OSG_ACT_SILU : OSG_ACT_NONE;
        int y = out_val(op, s, Lay::nhwc, V(x).batched);
        const long nb = B(x), HW = s[2] * s[3], C = s[1];
        // ---- statistics from the producer (round 3, m_hip_gn_stats): when x is what convolutions store -- one convolution's output, or a Concat buffer that
        // convolutions fill through output views -- their epilogues add the per-(image, group) sums up on the way out (osg_set_stat_sinks) and the
        // normalisation is ONE streaming launch that reads 2 numbers per group.  Levels with >= 2048 rows (the 64 x 64 and 32 x 32 images of the SD 1.5 UNet):
        // below that the convolutions run split-K, whose slabs have no finished values to add up, and the statistics would cost a launch of their own.
        if (P.gn_stats_on && V(x).dtype == OSG_F16 && HW % 128 == 0 && nb * HW >= 2048 && nb * HW * C >= P.gn_stats_min_elems && C % 8 == 0 && C % G == 0 && V(x).ld == 0 && V(x).view_off == 0) {
            std::vector<ConcatPart> parts;
            const int rx = P.root_of(x);
            auto cp = concat_parts.find(rx);
            if (cp != concat_parts.end()) parts = cp->second;      // (every operand of the Concat is stored there by a convolution: together they cover all channels)
            else {
                auto it = conv_producers.find(rx);
                if (it != conv_producers.end() && it->second.y == x && it->second.out->dst == x && it->second.out->dst_ld == 0) parts.push_back(ConcatPart{it->second.out, 0, 0, it->second.step});
            }
            bool ok = !parts.empty();
            for (auto& pt : parts) ok = ok && !pt.out->no_sinks && pt.out->sink[pt.slot].off < 0 && (pt.out->sink_hw == 0 || pt.out->sink_hw == (int)HW);
            if (ok) {
                const long off = P.gn_stats_bytes;
                P.gn_stats_bytes += (size_t)8 * nb * G * 2 * sizeof(long long);     // (eight copies, one per XCD: include/osgpu.h osg_set_stat_sinks)
                for (auto& pt : parts) {
                    pt.out->sink[pt.slot] = StatSinkRef{off, (int)G, (int)(C / G), (int)pt.ch_off};
                    pt.out->sink_hw = (int)HW;
                    P.steps[pt.step].what += " +gnstats";
                    P.steps[pt.step].side = true;
                }
                P.add_step("GroupNorm stats< " + op.m_name, {x, g, b}, {y}, [=, this] {
                    be.check(be.api.osg_group_norm_stats_nhwc(be.ctx, P.ptr(x), P.ptr(g), P.ptr(b), P.ptr(y), (int)nb, HW, (int)C, (int)G, eps, (osg_act)act, P.gn_stats + off),
                             "GroupNorm");
                });
                P.steps.back().side = true;
                return;
            }
        }
        P.add_step("GroupNorm " + op.m_name, {x, g, b}, {y}, [=, this] {
            be.check(be.api.osg_group_norm_nhwc(be.ctx, OSG_F16, P.ptr(x), P.ptr(g), P.ptr(b), P.ptr(y), (int)nb, HW, (int)C, (int)G, eps, (osg_act)act),
                     "GroupNorm");
        });
    }

    // ---- LayerNorm folded into the GEMM(s) that consume it (osg_gemm_ln): when every consumer of a LayerNorm is an osg.Linear that ends
    // up in ONE GEMM launch (a single Linear / Linear+GEGLU, or the members of one merged group: self-attention Q|K|V), the LayerNorm is
    // not launched at all -- gamma moves into the weight, beta and the mean correction into two fp32 epilogue vectors, the row
    // statistics are accumulated by the GEMM's math waves beside the MFMAs, from the A fragments they read anyway.  48 launches less in the SD 1.5 UNet.
    std::map<std::string, LnFold> ln_deferred;   // LayerNorm output name -> what its consumers fold
    // ConstPool tag of a folded copy: it must name everything that went into the fold -- the LayerNorm's gamma and beta and the Linear's bias -- or a
    // weight tensor shared by two Linears behind different LayerNorms / with different biases would silently reuse the first fold (advisor, round 2)
    std::string ln_tag(const LnFold& f, int bias) {
        return "|ln:" + V(f.g).name + ":" + V(f.b).name + ":" + (bias >= 0 ? V(bias).name : std::string("-"));
    }

    bool ln_can_fold(const Operation& op, int x, int g, int b, long C) {
        if (P.fusion < 2 || !P.fuse_ln_gemm || P.stream_weights) return false;
        if (C % 64) return false;
        if (!V(g).host_valid || !V(b).host_valid || (long)V(g).host_f.size() != C || (long)V(b).host_f.size() != C) return false;
        if (V(x).ld != 0) return false;
        const std::string& out = op.m_output[0].m_name;
        if (use_count(out) >= 1000) return false;
        auto cit = consumers.find(out);
        if (cit == consumers.end() || cit->second.empty()) return false;
        int group = -2;
        for (int c : cit->second) {
            const Operation& co = ops()[c];
            if (dead[c] || co.m_type != "osg.Linear" || co.m_input.empty() || co.m_input[0].m_name != out) return false;
            for (size_t k = 1; k < co.m_input.size(); k++)
                if (co.m_input[k].m_name == out) return false;
            const Val* w = cval(co.m_input[1]);
            if (!w || w->shape.size() != 2 || w->dtype != OSG_F16 || w->shape[0] != C || w->shape[1] % 4) return false;
            if (co.m_input.size() > 2 && !co.m_input[2].m_name.empty() && (!cval(co.m_input[2]) || cval(co.m_input[2])->dtype != OSG_F16)) return false;
            auto git = group_of.find(c);
            const int gi = git == group_of.end() ? -1 : git->second.first;
            if (group == -2) group = gi;
            else if (group != gi || gi < 0) return false;         // several consumers must be members of ONE merged group
        }
        if (group >= 0 && groups[group].members.size() != cit->second.size()) return false;   // ... and be all of its members
        return true;
    }

    // W[N,K] (device, f16) -> W' = f16(gamma[k] * W[n][k]) in place; returns the fp32 device vectors (c1, c2):
    // c1[n] = sum_k W'[n][k], c2[n] = sum_k beta[k] * W[n][k] + bias[n]
    std::pair<int, int> ln_fold_weight(const LnFold& f, int wnk, int bias, void* w_dst, const std::string& tag) {
        const long Nn = V(wnk).shape[0], K = V(wnk).shape[1];
        bool fresh1, fresh2;
        int v1 = P.new_val("", {Nn}, OSG_F32, Lay::plain, false), v2 = P.new_val("", {Nn}, OSG_F32, Lay::plain, false);
        V(v1).is_const = V(v2).is_const = true;
        V(v1).dptr = P.const_alloc(tag + "|c1", (size_t)Nn * 4, &fresh1);
        V(v2).dptr = P.const_alloc(tag + "|c2", (size_t)Nn * 4, &fresh2);
        if (!fresh1 && !fresh2) return {v1, v2};   // folded by an earlier plan of this Model (w_dst is the same pooled buffer)
        std::vector<uint16_t> w((size_t)Nn * K);
        be.check(be.api.osg_sync(be.ctx), "osg_sync");
        be.check(be.api.osg_download(be.ctx, w.data(), P.ptr(wnk), w.size() * 2), "osg_download");
        std::vector<uint16_t> bh;
        if (bias >= 0) {
            bh.resize((size_t)Nn);
            be.check(be.api.osg_download(be.ctx, bh.data(), P.ptr(bias), bh.size() * 2), "osg_download");
        }
        const std::vector<float>& gam = V(f.g).host_f;
        const std::vector<float>& bet = V(f.b).host_f;
        std::vector<float> c1((size_t)Nn), c2((size_t)Nn);
        for (long n = 0; n < Nn; n++) {
            double s1 = 0, s2 = 0;
            uint16_t* row = w.data() + (size_t)n * K;
            for (long k = 0; k < K; k++) {
                const float wv = half_to_float(row[k]);
                s2 += (double)bet[k] * (double)wv;
                const uint16_t folded = float_to_half(gam[k] * wv);
                row[k] = folded;
                s1 += (double)half_to_float(folded);
            }
            c1[n] = (float)s1;
            c2[n] = (float)(s2 + (bias >= 0 ? (double)half_to_float(bh[n]) : 0.0));
        }
        be.check(be.api.osg_upload_sync(be.ctx, w_dst, w.data(), w.size() * 2), "osg_upload_sync");
        be.check(be.api.osg_upload_sync(be.ctx, V(v1).dptr, c1.data(), c1.size() * 4), "osg_upload_sync");
        be.check(be.api.osg_upload_sync(be.ctx, V(v2).dptr, c2.data(), c2.size() * 4), "osg_upload_sync");
        return {v1, v2};
    }

    // a private [N,K] copy of a resident weight (the K-contiguous twin is shared by every user of the tensor: never folded in place)
    int private_copy(int wnk, const std::string& tag) {
        const long Nn = V(wnk).shape[0], K = V(wnk).shape[1];
        int t = P.new_val("", {Nn, K}, OSG_F16, Lay::plain, false);
        V(t).is_const = true;
        V(t).name = V(wnk).name + tag;
        bool fresh;
        V(t).dptr = P.const_alloc(V(t).name, (size_t)Nn * K * 2, &fresh);
        return t;
    }

    void emit_gemm_ln(const std::string& what, const LnFold& f, int wfold, int c1, int c2, int res, int y, long M, long Nn, long K, osg_act act_) {
        const int x = f.x, rs = f.rs;
        const float eps = f.eps;
        std::vector<int> reads = {x, wfold, c1, c2};
        if (res >= 0) reads.push_back(res);
        if (rs >= 0) reads.push_back(rs);
        P.add_step(what, reads, {y}, [=, this] {
            be.check(be.api.osg_gemm_ln(be.ctx, P.ptr(x), P.ptr(wfold), (const float*)P.ptr(c1), (const float*)P.ptr(c2), eps,
                                        rs >= 0 ? (const float*)P.ptr(rs) : nullptr, res >= 0 ? P.ptr(res) : nullptr, P.ptr(y), (int)M, (int)Nn, (int)K, act_),
                     what.c_str());
        });
        P.steps.back().flops = 2.0 * M * Nn * K;
    }

    void lower_layer_norm(const Operation& op) {
        int x = P.ensure_plain(in_val(op.m_input[0]));
        int g = in_val(op.m_input[1]), b = in_val(op.m_input[2]);
        const Shape s = V(x).shape;
        const float eps = std::stof(*attr(op, "epsilon"));
        if (ln_can_fold(op, x, g, b, s.back())) {
            check_out(op, s);
            const int rs = upgrade_rs_producer(x, P.total_elems(x) / s.back(), s.back());
            ln_deferred[op.m_output[0].m_name] = LnFold{x, g, b, eps, s.back(), rs};
            return;
        }
        int y = out_val(op, s, Lay::plain, V(x).batched);
        const long C = s.back(), rows = P.total_elems(x) / C;
        P.add_step("LayerNorm " + op.m_name, {x, g, b}, {y}, [=, this] {
            be.check(be.api.osg_layer_norm(be.ctx, OSG_F16, P.ptr(x), P.ptr(g), P.ptr(b), P.ptr(y), rows, (int)C, eps), "LayerNorm");
        });
    }

    void lower_geglu(const Operation& op) {
        int x = P.ensure_plain(in_val(op.m_input[0]));
        Shape s = V(x).shape;
        const long C = s.back() / 2, rows = P.total_elems(x) / s.back();
        s.back() = C;
        int y = out_val(op, s, Lay::plain, V(x).batched);
        P.add_step("GEGLU " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_geglu(be.ctx, OSG_F16, P.ptr(x), P.ptr(y), rows, C), "GEGLU"); });
    }

    void lower_attention(const Operation& op) {
        int q = P.ensure_plain(in_val_raw(op.m_input[0])), k = P.ensure_plain(in_val_raw(op.m_input[1])), v = P.ensure_plain(in_val_raw(op.m_input[2]));
        const long h = std::stol(*attr(op, "heads"));
        const float scale = std::stof(*attr(op, "scale"));
        const Shape qs = V(q).shape;
        const long Tq = qs[1], C = qs[2], Tk = V(k).shape[1], d = C / h;
        int y = out_val(op, qs, Lay::plain, V(q).batched);
        need(op, V(q).batched == V(k).batched && V(k).batched == V(v).batched, "q/k/v batching mismatch.");
        const long nb = B(q);
        P.add_step("Attention " + op.m_name, {q, k, v}, {y}, [=, this] {
            const long lq = P.vals[q].ld ? P.vals[q].ld : C, lk = P.vals[k].ld ? P.vals[k].ld : C, lv = P.vals[v].ld ? P.vals[v].ld : C;
            be.check(be.api.osg_attention_strided(be.ctx, OSG_F16, P.ptr(q), lq, d, Tq * lq, P.ptr(k), lk, d, Tk * lk, P.ptr(v), lv, d, Tk * lv,
                                                  P.ptr(y), C, d, Tq * C, (int)nb, (int)h, (int)Tq, (int)Tk, (int)d, scale),
                     "Attention");
        });
        P.steps.back().flops = 4.0 * nb * h * Tq * Tk * d;
    }

    // ---- osg.TBlockTail (fuse_tblock_tail): one launch of osg_tblock_tail per transformer block, K / V packs of ALL such blocks from one launch --------
    std::map<std::string, std::pair<int, size_t>> kv_packs;   // fused op name -> (pack buffer val, element offset of its kp; vtp right behind)

    // K / V of cross-attentions that are column views of ONE merged projection of the text context (plan_linear_groups: 32 -> 1) are re-packed by ONE
    // launch for every osg.TBlockTail of the graph that shares the merged output and the head count with `op`
    // (input positions of k / v in the fused ops that read packs)
    static int kv_input(const Operation& o) { return o.m_type == "osg.TBlockTail" ? 8 : -1; }
    void prepack_kv(const Operation& op, int k, int v, long heads, long Tk) {
        struct Job { std::string name; long kcol, vcol, D; };
        const int ki0 = kv_input(op);
        std::vector<Job> jobs;
        const int base = P.root_of(k);
        const long ld = V(k).ld;
        const bool shared = ld > 0 && P.root_of(v) == base && V(v).ld == ld && V(k).view_off % 2 == 0 && V(v).view_off % 2 == 0;
        const long imgs = B(k);
        int src = base;
        long src_ld = ld;
        if (shared) {
            jobs.push_back(Job{op.m_name, (long)V(k).view_off / 2, (long)V(v).view_off / 2, V(k).shape.back() / heads});
            const int gk = indexed && producer.count(op.m_input[ki0].m_name) && group_of.count(producer[op.m_input[ki0].m_name]) ? group_of[producer[op.m_input[ki0].m_name]].first : -1;
            if (gk >= 0)
                for (size_t i = 0; i < ops().size(); i++) {
                    const Operation& o = ops()[i];
                    const int ki = kv_input(o);
                    if (ki < 0 || o.m_name == op.m_name || kv_packs.count(o.m_name) || std::stol(*attr(o, "heads")) != heads) continue;
                    auto pk = producer.find(o.m_input[ki].m_name), pv = producer.find(o.m_input[ki + 1].m_name);
                    if (pk == producer.end() || pv == producer.end()) continue;
                    auto gik = group_of.find(pk->second), giv = group_of.find(pv->second);
                    if (gik == group_of.end() || giv == group_of.end() || gik->second.first != gk || giv->second.first != gk) continue;
                    if ((long)o.m_input[ki].m_shape[1] != Tk) continue;
                    const LinGroup& g = groups[gk];
                    jobs.push_back(Job{o.m_name, g.off[gik->second.second], g.off[giv->second.second], (long)o.m_input[ki].m_shape[2] / heads});
                }
        } else {
            // dense K and V of one block: side by side in a scratch matrix first (never the case in the SD graphs: their K / V projections are merged)
            const long C = V(k).shape.back();
            const int kd = P.ensure_plain(k), vd = P.ensure_plain(v);
            src = P.new_val("", {imgs * Tk, 2 * C}, OSG_F16, Lay::plain, false);
            src_ld = 2 * C;
            const long rows = imgs * Tk;
            P.add_step("KVPack gather " + op.m_name, {kd, vd}, {src}, [=, this] { be.check(be.api.osg_concat2(be.ctx, 2, P.ptr(kd), C, P.ptr(vd), C, P.ptr(src), rows), "KVPack"); });
            jobs.push_back(Job{op.m_name, 0, C, C / heads});
        }
        std::vector<int> table;
        size_t total = 0;
        for (auto& j : jobs) {
            const size_t each = be.api.osg_tblock_kv_pack_elems((int)imgs, (int)heads, (int)j.D);
            table.insert(table.end(), {(int)j.kcol, (int)j.vcol, (int)j.D, (int)total});
            total += 2 * each;
        }
        const int pack = P.new_val("", {(long)total}, OSG_F16, Lay::plain, false);
        void* tdev = P.small_alloc(table.size() * sizeof(int));
        be.check(be.api.osg_upload_sync(be.ctx, tdev, table.data(), table.size() * sizeof(int)), "osg_upload_sync");
        for (size_t j = 0; j < jobs.size(); j++) kv_packs[jobs[j].name] = {pack, (size_t)table[4 * j + 3]};
        const int nj = (int)jobs.size();
        P.add_step("KVPack x" + std::to_string(nj) + " " + op.m_name, {src}, {pack}, [=, this] {
            be.check(be.api.osg_tblock_kv_pack_jobs(be.ctx, P.ptr(src), src_ld, (int)imgs, (int)Tk, (int)heads, nj, (const int*)tdev, P.ptr(pack)), "KVPack");
        });
    }

    // a resident [N,K] weight in the layout osg_tblock_tail streams ([K/8][N][8], osg_tblock_pack_weight): a derived constant of the Model's pool, made once
    int weight_kn8(int wnk) {
        const long Nn = V(wnk).shape[0], K = V(wnk).shape.size() == 2 ? V(wnk).shape[1] : prod(V(wnk).shape) / Nn;
        int t = P.new_val("", {K / 8, Nn, 8}, OSG_F16, Lay::plain, false);
        V(t).is_const = true;
        V(t).name = V(wnk).name + "|kn8";
        bool fresh;
        V(t).dptr = P.const_alloc(V(t).name, (size_t)Nn * K * 2, &fresh);
        if (fresh) {
            be.check(be.api.osg_tblock_pack_weight(be.ctx, P.ptr(wnk), (int)Nn, (int)K, V(t).dptr), "osg_tblock_pack_weight");
            be.check(be.api.osg_sync(be.ctx), "osg_sync");
        }
        return t;
    }

    void lower_tblock_tail(const Operation& op) {
        const bool proj = *attr(op, "proj") == "1";
        need(op, op.m_input.size() == (proj ? 21u : 18u) && op.m_output.size() == 1, "wrong number of inputs.");
        const long heads = std::stol(*attr(op, "heads"));
        const float scale = std::stof(*attr(op, "scale")), eps2 = std::stof(*attr(op, "eps2")), eps3 = std::stof(*attr(op, "eps3"));
        const int a1 = P.ensure_plain(in_val(op.m_input[0])), x0 = P.ensure_plain(in_val(op.m_input[1]));
        auto opt = [&](const Tensor& t) { return t.m_name.empty() ? -1 : in_val(t); };
        const int wo1 = weight_kn8(weight_nk(in_val(op.m_input[2]))), bo1 = opt(op.m_input[3]), g2 = in_val(op.m_input[4]), be2 = in_val(op.m_input[5]);
        const int wq2 = weight_kn8(weight_nk(in_val(op.m_input[6]))), bq2 = opt(op.m_input[7]);
        const int k = in_val_raw(op.m_input[8]), v = in_val_raw(op.m_input[9]);
        const int wo2 = weight_kn8(weight_nk(in_val(op.m_input[10]))), bo2 = opt(op.m_input[11]), g3 = in_val(op.m_input[12]), be3 = in_val(op.m_input[13]);
        const int w1 = weight_kn8(weight_nk(in_val(op.m_input[14]))), b1 = opt(op.m_input[15]), w2 = weight_kn8(weight_nk(in_val(op.m_input[16]))), b2 = opt(op.m_input[17]);
        const Shape as = V(a1).shape;
        need(op, as.size() == 3 && as[0] == 1 && V(x0).shape == as && V(a1).ld == 0 && V(x0).ld == 0, "invalid shape of inputs.");
        const long T = as[1], C = as[2], F = 4 * C, Tk = V(k).shape[1], nb = B(a1), M = T * nb;
        need(op, V(a1).batched == V(x0).batched && V(k).batched == V(a1).batched && V(v).batched == V(a1).batched, "q/k/v batching mismatch.");
        need(op, be.api.osg_tblock_tail_supported((int)M, (int)T, (int)C, (int)heads, (int)Tk) == 1, "shape not taken by osg_tblock_tail.");
        for (int g : {g2, be2, g3, be3}) need(op, V(g).dtype == OSG_F16 && V(g).numel() == C, "invalid LayerNorm operands.");
        int wpo = -1, bpo = -1, xin = -1;
        if (proj) {
            wpo = in_val(op.m_input[18]);
            bpo = opt(op.m_input[19]);
            xin = P.ensure_nhwc(in_val(op.m_input[20]));
            need(op, V(wpo).is_const && V(wpo).lay == Lay::nhwc && V(wpo).dtype == OSG_F16 && V(xin).ld == 0 && P.total_elems(xin) == M * C, "invalid proj_out operands.");
            wpo = weight_kn8(wpo);      // (OHWI of a 1x1 convolution IS [N][K])
        }
        if (!kv_packs.count(op.m_name)) prepack_kv(op, k, v, heads, Tk);
        const auto [pack, koff] = kv_packs.at(op.m_name);
        const size_t each = be.api.osg_tblock_kv_pack_elems((int)nb, (int)heads, (int)(C / heads));
        int y;
        if (proj) {
            const Shape xs = V(xin).shape;   // [1, C, H, W]
            y = out_val(op, xs, Lay::nhwc, V(a1).batched);
        } else
            y = out_val(op, as, Lay::plain, V(a1).batched);
        auto co = std::make_shared<ConvOut>();
        co->dst = y;
        co->no_sinks = true;
        std::vector<int> reads = {a1, x0, wo1, g2, be2, wq2, pack, wo2, g3, be3, w1, w2};
        for (int r : {bo1, bq2, bo2, b1, b2, wpo, bpo, xin})
            if (r >= 0) reads.push_back(r);
        const std::string what = std::string("TBlockTail") + (proj ? "+proj_out " : " ") + op.m_name;
        P.add_step(what, reads, {y}, [=, this] {
            const ConvOut& o = *co;
            auto p = [&](int val) -> const void* { return val >= 0 ? P.ptr(val) : nullptr; };
            osg_tblock_tail_args a{};
            a.a1 = p(a1); a.x0 = p(x0);
            a.wo1 = p(wo1); a.bo1 = p(bo1);
            a.g2 = p(g2); a.be2 = p(be2); a.eps2 = eps2;
            a.wq2 = p(wq2); a.bq2 = p(bq2);
            a.kp = (const char*)P.ptr(pack) + koff * 2;
            a.vtp = (const char*)a.kp + each * 2;
            a.scale = scale; a.Tk = (int)Tk;
            a.wo2 = p(wo2); a.bo2 = p(bo2);
            a.g3 = p(g3); a.be3 = p(be3); a.eps3 = eps3;
            a.w1 = p(w1); a.b1 = p(b1); a.w2 = p(w2); a.b2 = p(b2);
            a.wpo = p(wpo); a.bpo = p(bpo); a.xin = p(xin);
            a.out = (char*)P.ptr(o.dst) + o.dst_off; a.ldo = o.dst_ld;
            a.out2 = o.dst2 >= 0 ? (char*)P.ptr(o.dst2) + o.dst2_off : nullptr; a.ldo2 = o.dst2_ld;
            a.M = (int)M; a.rows_per_img = (int)T; a.C = (int)C; a.heads = (int)heads;
            be.check(be.api.osg_tblock_tail(be.ctx, &a), what.c_str());
        });
        P.steps.back().flops = 2.0 * M * C * C * (proj ? 4 : 3) + 2.0 * M * C * 2 * F + 2.0 * M * F * C + 4.0 * nb * heads * T * Tk * (C / heads);
        if (proj) conv_producers[P.root_of(y)] = ConvProducer{P.steps.size() - 1, co, y};
    }

    // ScaledDotProductAttention (reference :7767-7882): q [B,Hq,T,D], k [B,Hkv,S,D], mask [T,S] | [1,1,T,S], v [B,Hkv,S,Dv] -> [B,Hq,T,Dv]
    void lower_sdpa(const Operation& op) {
        need(op, op.m_input.size() == 4, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        // key / value: a virtual repeat_kv Expand (lower_expand) is read at its source, with the un-repeated head count
        auto kv_operand = [&](const Tensor& t) {
            const int v0 = in_val(t), r = P.root_of(v0);
            if (V(r).rep_src < 0) return P.ensure_plain(v0);
            const int src = P.ensure_plain(V(r).rep_src);
            const Shape ss = V(src).shape, es = V(v0).shape;   // [1,Hkv,1,S,d] and [1,Hkv*rep,S,d]
            need(op, es.size() == 4 && ss.size() == 5 && es[0] == 1 && es[1] == ss[1] * V(r).rep && es[2] == ss[3] && es[3] == ss[4], "invalid shape of key or value.");
            return P.alias(src, Shape{1, ss[1], ss[3], ss[4]}, Lay::plain);
        };
        // (chunk plans: a mask known at plan time is checked and dropped below -- it gets no device storage)
        const Val* hm = P.decode && P.dspec.chunk > 0 ? hval(op.m_input[2]) : nullptr;
        const int q = P.ensure_plain(in_val(op.m_input[0])), k = kv_operand(op.m_input[1]), mk = hm ? -1 : P.ensure_plain(in_val(op.m_input[2])), v = kv_operand(op.m_input[3]);
        const Shape qs = V(q).shape, ks = V(k).shape, vs = V(v).shape, ms = hm ? hm->shape : V(mk).shape;
        need(op, qs.size() == 4, "invalid shape of query.");
        need(op, ks.size() == 4, "invalid shape of key.");
        need(op, vs.size() == 4, "invalid shape of value.");
        need(op, ms.size() == 2 || (ms.size() == 4 && ms[0] == 1 && ms[1] == 1), "invalid shape of mask.");
        const long Bq = qs[0], Hq = qs[1], T = qs[2], D = qs[3], Hkv = ks[1], S = ks[2], Dv = vs[3];
        need(op, ks[0] == Bq && vs[0] == Bq && ks[3] == D && vs[1] == Hkv && vs[2] == S && Hkv > 0 && Hq % Hkv == 0, "invalid shape of query, key or value.");
        need(op, ms[ms.size() - 2] == T && ms[ms.size() - 1] == S, "invalid shape of mask.");
        need(op, V(q).dtype == OSG_F16 && V(k).dtype == OSG_F16 && V(v).dtype == OSG_F16 && (hm || V(mk).dtype == OSG_F16), "wrong data type of query.");
        need(op, Dv == D && D % 8 == 0 && D <= 160, "head dims other than a multiple of 8 up to 160 with Dv == D are not implemented on the HIP backend.");
        need(op, N == 1 || (!hm && !V(mk).batched && V(q).batched == V(k).batched && V(k).batched == V(v).batched), "q/k/v batching mismatch.");
        const float scale = std::stof(*attr(op, "scale"));
        need(op, scale > 0.f, "a scale <= 0 is not implemented on the HIP backend.");
        const int y = out_val(op, Shape{Bq, Hq, T, Dv}, Lay::plain, V(q).batched);
        const long nb = Bq * B(q);
        const bool k_cap = V(P.root_of(k)).kv_cap, v_cap = V(P.root_of(v)).kv_cap;
        if (P.decode && P.dspec.chunk > 0) {
            // chunk plans: C query rows over the capacity buffers [Hkv][CAP][D]; the chunk's first row is the device-side dec_state[0], the causal bound
            // is worked out from it in the kernel, so the mask operand is dropped once it is known to say the same
            const long C = P.dspec.chunk, cap = P.dspec.cap;
            if (!(k_cap && v_cap && T == C && Bq == 1 && nb == 1 && N == 1 && S == cap && V(k).view_off == 0 && V(v).view_off == 0)) refuse_kv_cap(op);
            const float masked = causal_mask_value(op, hm, C, cap);
            P.add_step("ScaledDotProductAttention(chunk) " + op.m_name, {q, k, v}, {y}, [=, this] {
                be.check(be.api.osg_sdpa_chunk(be.ctx, OSG_F16, P.ptr(q), P.ptr(k), P.ptr(v), P.ptr(y), P.dec_state, masked, cap * D, cap * D * Hkv, cap, 1, (int)Hq,
                                               (int)Hkv, (int)C, (int)D, scale),
                         "ScaledDotProductAttention");
            });
            P.steps.back().flops = 4.0 * Hq * C * cap * D;
            return;
        }
        if (k_cap || v_cap) {
            // decode plans: key and value are capacity buffers [Hkv][CAP][D] (S == CAP here), the number of keys is the device-side cache length
            if (!(k_cap && v_cap && T == 1 && Bq == 1 && nb == N && !V(mk).batched && S == P.dspec.cap && V(k).view_off == 0 && V(v).view_off == 0)) refuse_kv_cap(op);
            const long cap = S;
            if (N > 1) {   // N sequences: the capacity buffers of sequence b follow those of b - 1, its length is state[4 * b + 1]; the mask is shared
                P.add_step("ScaledDotProductAttention(len, batch) " + op.m_name, {q, k, mk, v}, {y}, [=, this] {
                    be.check(be.api.osg_sdpa_len_batch(be.ctx, OSG_F16, P.ptr(q), P.ptr(k), P.ptr(v), P.ptr(mk), P.ptr(y), P.dec_state + 1, 4, cap * D, cap * D * Hkv, cap,
                                                       (int)nb, (int)Hq, (int)Hkv, (int)D, scale),
                             "ScaledDotProductAttention");
                });
                return;
            }
            P.add_step("ScaledDotProductAttention(len) " + op.m_name, {q, k, mk, v}, {y}, [=, this] {
                be.check(be.api.osg_sdpa_len(be.ctx, OSG_F16, P.ptr(q), P.ptr(k), P.ptr(v), P.ptr(mk), P.ptr(y), P.dec_state + 1, cap * D, cap * D * Hkv, cap, 1, (int)Hq,
                                             (int)Hkv, (int)D, scale),
                         "ScaledDotProductAttention");
            });
            return;
        }
        P.add_step("ScaledDotProductAttention " + op.m_name, {q, k, mk, v}, {y}, [=, this] {
            be.check(be.api.osg_sdpa(be.ctx, OSG_F16, P.ptr(q), P.ptr(k), P.ptr(v), P.ptr(mk), P.ptr(y), (int)nb, (int)Hq, (int)Hkv, (int)T, (int)S, (int)D, scale),
                     "ScaledDotProductAttention");
        });
        P.steps.back().flops = 4.0 * nb * Hq * T * S * D;
    }

    // AttentionFusedOps (reference :6696-6929): q [n,Tq,d], k [n,d,Tk] (already transposed), optional scalar s, v [n,Tk,d]
    void lower_attention_fused_ops(const Operation& op) {
        need(op, op.m_input.size() == 4, "wrong number of inputs.");
        int q = P.ensure_plain(in_val(op.m_input[0])), k = P.ensure_plain(in_val(op.m_input[1])), v = P.ensure_plain(in_val(op.m_input[3]));
        Shape qs = V(q).shape, ks = V(k).shape, vs = V(v).shape;
        bool lead1 = false;
        if (qs.size() == 4 && qs[0] == 1 && ks.size() == 4 && ks[0] == 1 && vs.size() == 4 && vs[0] == 1) {
            qs.erase(qs.begin()); ks.erase(ks.begin()); vs.erase(vs.begin());
            lead1 = true;
        }
        need(op, qs.size() == 3 && ks.size() == 3 && vs.size() == 3, "shapes of q, k and v must have 3 dimensions.");
        need(op, qs[0] == ks[0] && qs[0] == vs[0] && ks[1] == qs[2] && vs[1] == ks[2] && vs[2] == qs[2], "invalid shape(s) of q, k and/or v.");
        float scale = 1.0f;
        if (!op.m_input[2].m_name.empty()) {
            need(op, cval(op.m_input[2]) && cval(op.m_input[2])->shape.empty() && const_scalar(op.m_input[2], &scale), "s must be a scalar.");
        }
        need(op, (size_t)qs[1] >= m.m_attention_fused_ops_parts, "m_attention_fused_ops_parts is not valid.");
        Shape os = qs;
        if (lead1) os.insert(os.begin(), 1);
        int y = out_val(op, os, Lay::plain, V(q).batched);
        need(op, V(q).batched == V(k).batched && V(k).batched == V(v).batched, "q/k/v batching mismatch.");
        const long heads = qs[0] * B(q), Tq = qs[1], d = qs[2], Tk = ks[2];
        if (d > 160 || d % 8) {
            // head dims the flash kernel does not take (the VAE's single 512-wide head): the reference's own sequence, unsliced --
            // S = f16(Q K^T); S = f16(S * s); P = softmax_rows(S); O = f16(P V)  (reference :6796-6929)
            int sv = P.new_val("", {qs[0], Tq, Tk}, OSG_F16, Lay::plain, V(q).batched);
            int pv = P.new_val("", {qs[0], Tq, Tk}, OSG_F16, Lay::plain, V(q).batched);
            emit_gemm("MatMul " + op.m_name + "/QK", q, k, -1, -1, sv, Tq, Tk, d, heads, Tq * d, d * Tk, Tq * Tk, 0);
            int cur = sv;
            if (scale != 1.0f) {
                int sc = P.new_val("", {1}, OSG_F16, Lay::plain, false);
                V(sc).is_const = true;
                bool fresh;
                V(sc).dptr = P.const_alloc("scale|" + op.m_name, 256, &fresh);
                const uint16_t hbits = float_to_half(scale);
                if (fresh) be.check(be.api.osg_upload_sync(be.ctx, V(sc).dptr, &hbits, 2), "osg_upload_sync");
                const long tot = heads * Tq * Tk;
                P.add_step("Mul " + op.m_name + "/scale", {sv, sc}, {sv}, [=, this] {
                    long as[1] = {tot}, bs[1] = {1};
                    be.check(be.api.osg_binary(be.ctx, OSG_F16, OSG_BIN_MUL, P.ptr(sv), as, P.ptr(sc), bs, P.ptr(sv), 1), "osg_binary");
                });
            }
            P.add_step("Softmax " + op.m_name, {cur}, {pv}, [=, this] {
                be.check(be.api.osg_softmax_last(be.ctx, OSG_F16, P.ptr(cur), P.ptr(pv), heads * Tq, Tk), "osg_softmax_last");
            });
            emit_gemm("MatMul " + op.m_name + "/PV", pv, v, -1, -1, y, Tq, d, Tk, heads, Tq * Tk, Tk * d, Tq * d, 0);
            return;
        }
        P.add_step("AttentionFusedOps " + op.m_name, {q, k, v}, {y}, [=, this] {
            be.check(be.api.osg_attention(be.ctx, OSG_F16, P.ptr(q), P.ptr(k), P.ptr(v), P.ptr(y), (int)heads, (int)Tq, (int)Tk, (int)d, scale, 1),
                     "AttentionFusedOps");
        });
        P.steps.back().flops = 4.0 * heads * Tq * Tk * d;
    }

    // ReduceMean (reference :5237-5393): last axis, keepdims
    void lower_reduce_mean(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        int x = P.ensure_plain(in_val(op.m_input[0]));
        const Shape s = V(x).shape;
        for (auto& a : op.m_attributes) {
            if (a.first == "axes") {
                auto ax = int_list(a.second);
                need(op, ax.size() == 1 && (ax[0] == -1 || ax[0] == (int)s.size() - 1), "reduction supported on the last axis only (not implemented).");
            } else if (a.first == "keepdims") need(op, std::stoi(a.second) == 1, "keepdims must be 1 (not implemented).");
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        Shape os = s;
        os.back() = 1;
        const osg_dtype adt = cur_up ? OSG_F32 : OSG_F16;
        need(op, V(x).dtype == adt, "wrong data type of input.");
        int y = out_val(op, os, Lay::plain, V(x).batched, adt);
        V(y).up32 = adt == OSG_F32;
        const long C = s.back(), rows = P.total_elems(x) / C;
        P.add_step("ReduceMean " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_reduce_mean_last(be.ctx, adt, P.ptr(x), P.ptr(y), rows, C), "ReduceMean"); });
    }

    // Softmax (reference :5862-5998): any axis via transpose-in / softmax / transpose-out (:5883-5923)
    void lower_softmax(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        int x = P.ensure_plain(in_val(op.m_input[0]));
        const Shape s = V(x).shape;
        int axis = -1;
        for (auto& a : op.m_attributes) {
            if (a.first == "axis") axis = std::stoi(a.second);
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        const int rank = (int)s.size();
        if (axis < 0) axis += rank;
        need(op, axis >= 0 && axis < rank, "invalid axis.");
        int y = out_val(op, s, Lay::plain, V(x).batched);
        const long nb = B(x);
        if (axis == rank - 1) {
            const long C = s.back(), rows = P.total_elems(x) / C;
            P.add_step("Softmax " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_softmax_last(be.ctx, OSG_F16, P.ptr(x), P.ptr(y), rows, C), "Softmax"); });
            return;
        }
        // [outer, A, inner] -> [outer, inner, A] -> softmax -> back
        const long outer = prod(s, 0, axis) * nb, A = s[axis], inner = prod(s, axis + 1);
        int t0 = P.new_val("", s, OSG_F16, Lay::plain, V(x).batched), t1 = P.new_val("", s, OSG_F16, Lay::plain, V(x).batched);
        P.add_step("Softmax/T0 " + op.m_name, {x}, {t0}, [=, this] {
            long sh[3] = {outer, A, inner}; int pm[3] = {0, 2, 1};
            be.check(be.api.osg_transpose(be.ctx, 2, P.ptr(x), P.ptr(t0), 3, sh, pm), "Softmax");
        });
        P.add_step("Softmax " + op.m_name, {t0}, {t1}, [=, this] { be.check(be.api.osg_softmax_last(be.ctx, OSG_F16, P.ptr(t0), P.ptr(t1), outer * inner, A), "Softmax"); });
        P.add_step("Softmax/T1 " + op.m_name, {t1}, {y}, [=, this] {
            long sh[3] = {outer, inner, A}; int pm[3] = {0, 2, 1};
            be.check(be.api.osg_transpose(be.ctx, 2, P.ptr(t1), P.ptr(y), 3, sh, pm), "Softmax");
        });
    }

    // Reshape (reference :4708-4787): zero-copy; an NHWC producer is brought back to the logical layout first (:4724)
    void lower_reshape(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        for (auto& a : op.m_attributes) {
            if (a.first == "allowzero") need(op, std::stoi(a.second) == 0, "allowzero != 0 not supported (not implemented).");
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        int x = in_val(op.m_input[0]);
        const Val* sv = hval(op.m_input[1]);
        need(op, sv && sv->dtype == OSG_I64 && sv->host_valid, "wrong data type of shape.");
        const long total = V(x).numel();
        Shape os;
        long known = 1;
        int infer = -1;
        for (size_t i = 0; i < sv->host_i.size(); i++) {
            long d = sv->host_i[i];
            if (d == 0) { need(op, i < V(x).shape.size(), "invalid 0 in shape."); d = V(x).shape[i]; }
            if (d == -1) { need(op, infer < 0, "more than one -1 in shape."); infer = (int)i; os.push_back(1); continue; }
            os.push_back(d);
            known *= d;
        }
        if (infer >= 0) { need(op, known && total % known == 0, "invalid shape."); os[infer] = total / known; }
        need(op, prod(os) == total, "invalid shape.");
        // layout-preserving special case: an NHWC [1,C,H,W] tensor reshaped to [1,C,H*W]... is NOT a no-op; go plain.
        x = P.ensure_plain(x);
        check_out(op, os);
        P.alias(x, os, Lay::plain, op.m_output[0].m_name);
    }

    void lower_flatten(const Operation& op) {
        int x = P.ensure_plain(in_val(op.m_input[0]));
        int axis = 1;
        if (auto* a = attr(op, "axis")) axis = std::stoi(*a);
        const Shape s = V(x).shape;
        if (axis < 0) axis += (int)s.size();
        Shape os = {prod(s, 0, axis), prod(s, axis)};
        check_out(op, os);
        P.alias(x, os, Lay::plain, op.m_output[0].m_name);
    }

    // Unsqueeze (reference :3859-3905) / Squeeze (:7425): axes from a static int64 tensor
    void lower_squeeze(const Operation& op, bool unsq) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        int x = P.ensure_plain(in_val(op.m_input[0]));
        const Val* ax = hval(op.m_input[1]);
        need(op, ax && ax->dtype == OSG_I64 && ax->host_valid, "wrong data type of axes.");
        Shape os = V(x).shape;
        std::vector<long> axes(ax->host_i.begin(), ax->host_i.end());
        if (unsq) {
            const long orank = (long)os.size() + (long)axes.size();
            for (auto& a : axes) if (a < 0) a += orank;
            std::sort(axes.begin(), axes.end());
            for (long a : axes) { need(op, a >= 0 && a <= (long)os.size(), "invalid axis."); os.insert(os.begin() + a, 1); }
        } else {
            for (auto& a : axes) if (a < 0) a += (long)os.size();
            std::sort(axes.rbegin(), axes.rend());
            for (long a : axes) { need(op, a >= 0 && a < (long)os.size() && os[a] == 1, "invalid axis."); os.erase(os.begin() + a); }
        }
        check_out(op, os);
        P.alias(x, os, Lay::plain, op.m_output[0].m_name);
    }

    // Transpose (reference :5176-5236).  (0,2,3,1) of an NHWC tensor and (0,3,1,2) into an NHWC tensor are relabelings.
    void lower_transpose(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        auto* pm = attr(op, "perm");
        need(op, pm != nullptr, "perm attribute not found.");
        std::vector<int> perm = int_list(*pm);
        int x = in_val(op.m_input[0]);
        const Shape s = V(x).shape;
        need(op, perm.size() == s.size(), "invalid perm.");
        Shape os(s.size());
        for (size_t i = 0; i < s.size(); i++) { need(op, perm[i] >= 0 && perm[i] < (int)s.size(), "invalid index in perm."); os[i] = s[perm[i]]; }
        check_out(op, os);
        if (V(x).lay == Lay::nhwc && perm == std::vector<int>{0, 2, 3, 1}) {
            P.alias(x, os, Lay::plain, op.m_output[0].m_name);
            return;
        }
        if (V(x).lay == Lay::plain && s.size() == 4 && perm == std::vector<int>{0, 3, 1, 2}) {
            P.alias(x, os, Lay::nhwc, op.m_output[0].m_name);
            return;
        }
        x = P.ensure_plain(x);
        {   // a permutation that only moves dimensions of extent 1 leaves the memory image as it is (the head split / merge of a ONE-token decode step:
            // [1,1,H,d] <-> [1,H,1,d]): zero-copy, like a Reshape
            int prev = -1;
            bool same_image = V(x).ld == 0 && V(x).dtype != OSG_U8;
            for (size_t i = 0; same_image && i < perm.size(); i++) {
                if (s[perm[i]] == 1) continue;
                if (perm[i] < prev) same_image = false;
                prev = perm[i];
            }
            if (same_image) {
                P.alias(x, os, Lay::plain, op.m_output[0].m_name);
                return;
            }
        }
        int y = P.new_val(op.m_output[0].m_name, os, V(x).dtype, Lay::plain, V(x).batched);
        const int rank = (int)s.size() + 1;
        need(op, rank <= 6, "rank too large.");
        std::vector<long> sh(rank);
        std::vector<int> pp(rank);
        sh[0] = B(x); pp[0] = 0;
        for (int i = 1; i < rank; i++) { sh[i] = s[i - 1]; pp[i] = perm[i - 1] + 1; }
        const int es = (int)esize(V(x).dtype);
        P.add_step("Transpose " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_transpose(be.ctx, es, P.ptr(x), P.ptr(y), rank, sh.data(), pp.data()), "Transpose"); });
    }

    // Concat (reference :4140-4299)
    void lower_concat(const Operation& op) {
        need(op, !op.m_input.empty(), "wrong number of inputs.");
        auto* ax = attr(op, "axis");
        need(op, ax != nullptr, "axis attribute not found.");
        int axis = std::stoi(*ax);
        std::vector<int> xs;
        for (auto& t : op.m_input) xs.push_back(in_val(t));
        const int rank = (int)V(xs[0]).shape.size();
        if (axis < 0) axis += rank;
        need(op, axis >= 0 && axis < rank, "invalid axis.");
        if (P.decode) {
            // decode plans: the cache Concat (axis 2; operands the graph input <cache_in><i> and the one new row; result <cache_out><i>) appends in place --
            // the result aliases the capacity buffer, the row comes from the device-side state
            const int ci = is_const_tensor(op.m_input[0]) ? -1 : P.cache_index(op.m_input[0].m_name, P.dspec.cache_in);
            bool touches = false;
            for (int x : xs) touches |= V(P.root_of(x)).kv_cap;
            if (ci >= 0 && V(P.root_of(xs[0])).kv_cap) {
                const int c = xs[0], r = xs.size() == 2 ? P.ensure_plain(xs[1]) : -1;
                const Shape cs = V(c).shape;
                need(op, r >= 0 && axis == 2 && rank == 4 && op.m_output.size() == 1 && P.cache_index(op.m_output[0].m_name, P.dspec.cache_out) == ci,
                     "in the device token loop a cache is concatenated with one new row along axis 2 into its output.");
                const long C = P.dspec.chunk > 0 ? P.dspec.chunk : 1;      // (a chunk plan appends its C rows from the device-side row on)
                need(op, V(r).shape == Shape{1, cs[1], C, cs[3]} && V(r).dtype == OSG_F16 && V(c).dtype == OSG_F16 && V(r).ld == 0, "invalid shape of the new cache row.");
                const Shape os{1, cs[1], P.dspec.cap, cs[3]};
                check_out(op, os);
                const int y = P.alias(c, os, Lay::plain, op.m_output[0].m_name);
                const long Hkv = cs[1], d = cs[3], cap = P.dspec.cap;
                if (P.dspec.chunk > 0) {
                    need(op, N == 1, "the device prefill runs one sequence.");
                    P.add_step("KVAppend(rows) " + op.m_name, {r, c}, {y}, [=, this] {
                        be.check(be.api.osg_kv_append_rows_at(be.ctx, P.ptr(r), P.ptr(y), P.dec_state, (int)Hkv, (int)C, cap, (int)d), "osg_kv_append_rows_at");
                    });
                    return;
                }
                if (N > 1) {   // N sequences: each appends at the row of its own state
                    need(op, V(r).batched && V(c).batched, "in the device token loop of several sequences every sequence has a cache and a new row of its own.");
                    const long nb = N;
                    P.add_step("KVAppend(batch) " + op.m_name, {r, c}, {y}, [=, this] {
                        be.check(be.api.osg_kv_append_at_batch(be.ctx, P.ptr(r), P.ptr(y), P.dec_state, (int)nb, (int)Hkv, cap, (int)d), "osg_kv_append_at_batch");
                    });
                    return;
                }
                P.add_step("KVAppend " + op.m_name, {r, c}, {y}, [=, this] {
                    be.check(be.api.osg_kv_append_at(be.ctx, P.ptr(r), P.ptr(y), P.dec_state, (int)Hkv, cap, (int)d), "osg_kv_append_at");
                });
                return;
            }
            if (touches) throw std::runtime_error(std::string(P.dec_fn()) + "Concat (" + op.m_name + ") reads a key/value cache in a form the device token loop does not implement.");
        }
        bool all_nhwc = rank == 4 && axis == 1;
        for (int x : xs) all_nhwc &= V(x).lay == Lay::nhwc;
        bool batched = false;
        for (int& x : xs) { if (!all_nhwc) x = P.ensure_plain(x); batched |= V(x).batched; }
        for (int x : xs) need(op, V(x).batched == batched || N == 1, "mixing per-sample and shared operands is not implemented.");
        Shape os = V(xs[0]).shape;
        os[axis] = 0;
        for (int x : xs) {
            const Shape s = V(x).shape;
            need(op, (int)s.size() == rank, "invalid shape of inputs.");
            for (int d = 0; d < rank; d++) need(op, d == axis || s[d] == V(xs[0]).shape[d], "invalid shape of inputs.");
            os[axis] += s[axis];
        }
        int y = out_val(op, os, all_nhwc ? Lay::nhwc : Lay::plain, batched, V(xs[0]).dtype);
        const int es = (int)esize(V(y).dtype);
        // ---- operands that come straight out of convolutions are written into their slice by the convolution itself (see ConvOut) ----
        std::vector<char> placed(xs.size(), 0);
        bool any_empty = false;
        for (int x : xs) any_empty |= V(x).numel() == 0;
        if (all_nhwc && P.fusion >= 2 && indexed && !P.u8 && V(y).dtype == OSG_F16 && os[1] % 4 == 0 && P.concat_views && !any_empty) {
            long coff = 0;
            for (size_t k = 0; k < xs.size(); k++) {
                const int x = xs[k];
                const long Cx = V(x).shape[1];
                auto it = conv_producers.find(P.root_of(x));
                const bool whole = it != conv_producers.end() && it->second.y == x /* the convolution's OWN output, not a same-shape alias of it (advisor, round 3) */ && V(x).ld == 0 && V(x).view_off == 0 && V(x).numel() > 0 && V(x).batched == batched &&
                                   V(it->second.y).shape == V(x).shape && V(x).lay == Lay::nhwc && Cx % 4 == 0 && (coff * es) % 8 == 0;
                if (whole && it->second.out->dst2 < 0 && it->second.out->dst == it->second.y && it->second.out->dst_ld == 0) {
                    ConvOut& o = *it->second.out;
                    Step& st = P.steps[it->second.step];
                    const std::string& xname = op.m_input[k].m_name;
                    int others = use_count(xname) - 1;                 // readers besides this Concat
                    for (size_t k2 = 0; k2 < op.m_input.size(); k2++)
                        if (k2 != k && op.m_input[k2].m_name == xname) others = 1 << 20;   // (the same tensor twice: keep the copy path)
                    if (others == 0) {            // the Concat is its only reader: the slice is the one destination
                        o.dst = y; o.dst_ld = os[1]; o.dst_off = (size_t)coff * es;
                        for (int& wv : st.writes) if (wv == it->second.y) wv = y;
                        placed[k] = 1;
                    } else if (others < (1 << 20)) {   // other layers read the dense tensor: both destinations in one launch
                        o.dst2 = y; o.dst2_ld = os[1]; o.dst2_off = (size_t)coff * es;
                        st.writes.push_back(y);
                        placed[k] = 1;
                    }
                    if (placed[k]) {
                        st.what += " >concat";
                        viewed_steps.insert(it->second.step);
                        rs_producers.erase(P.root_of(x));
                        concat_parts[P.root_of(y)].push_back(ConcatPart{it->second.out, others == 0 ? 0 : 1, coff, it->second.step});
                    }
                }
                coff += Cx;
            }
        }
        // empty operands (the zero-length key/value caches of the LLM flow's first call, src/llm.cpp:388-402) contribute nothing
        {
            std::vector<int> live;
            for (int x : xs)
                if (V(x).numel() > 0) live.push_back(x);
            xs.swap(live);
            if (xs.empty()) return;
        }
        long outer, dst_pitch, off = 0;
        if (all_nhwc) { outer = os[2] * os[3] * (batched ? N : 1); dst_pitch = os[1]; }
        else { outer = prod(os, 0, axis) * (batched ? N : 1); dst_pitch = prod(os, axis); }
        if (std::find(placed.begin(), placed.end(), 0) != placed.end()) concat_parts.erase(P.root_of(y));   // (an operand arrives by a copy launch: no producer-side statistics)
        if (std::find(placed.begin(), placed.end(), 1) != placed.end()) {
            // (the live-operand filter above may have dropped empty operands: `placed` is indexed like the original list only when none was dropped)
            long off2 = 0;
            for (size_t k = 0; k < xs.size(); k++) {
                const int x = xs[k];
                const long inner = V(x).shape[1];
                if (!placed[k]) {
                    const long o = off2;
                    P.add_step("Concat " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_copy_2d(be.ctx, es, P.ptr(x), inner, 0, P.ptr(y), dst_pitch, o, outer, inner), "Concat"); });
                }
                off2 += inner;
            }
            return;
        }
        if (xs.size() == 2 && V(xs[0]).ld == 0 && V(xs[1]).ld == 0) {   // the skip-connection shape: both sources in one launch
            const int xa = xs[0], xb = xs[1];
            const long ia = all_nhwc ? V(xa).shape[1] : prod(V(xa).shape, axis), ib = all_nhwc ? V(xb).shape[1] : prod(V(xb).shape, axis);
            P.add_step("Concat " + op.m_name, {xa, xb}, {y}, [=, this] { be.check(be.api.osg_concat2(be.ctx, es, P.ptr(xa), ia, P.ptr(xb), ib, P.ptr(y), outer), "Concat"); });
            return;
        }
        for (int x : xs) {
            const long inner = all_nhwc ? V(x).shape[1] : prod(V(x).shape, axis);
            const long o = off;
            P.add_step("Concat " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_copy_2d(be.ctx, es, P.ptr(x), inner, 0, P.ptr(y), dst_pitch, o, outer, inner), "Concat"); });
            off += inner;
        }
    }

    // Split (reference :5999-6119): sizes from a static int64 tensor
    void lower_split(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        int x = in_val(op.m_input[0]);
        const Val* sz = hval(op.m_input[1]);
        need(op, sz && sz->dtype == OSG_I64 && sz->host_valid && sz->host_i.size() == op.m_output.size(), "invalid split tensor.");
        int axis = 0;
        if (auto* a = attr(op, "axis")) axis = std::stoi(*a);
        const int rank = (int)V(x).shape.size();
        if (axis < 0) axis += rank;
        const bool nhwc = V(x).lay == Lay::nhwc && axis == 1;
        if (!nhwc) x = P.ensure_plain(x);
        const Shape s = V(x).shape;
        long sum = 0;
        for (auto v : sz->host_i) sum += v;
        need(op, sum == s[axis], "invalid split sizes.");
        const int es = (int)esize(V(x).dtype);
        const long outer = (nhwc ? s[2] * s[3] : prod(s, 0, axis)) * B(x), src_pitch = nhwc ? s[1] : prod(s, axis);
        const long unit = nhwc ? 1 : prod(s, axis + 1);
        long off = 0;
        for (size_t i = 0; i < op.m_output.size(); i++) {
            Shape os = s;
            os[axis] = sz->host_i[i];
            int y = out_val(op, os, nhwc ? Lay::nhwc : Lay::plain, V(x).batched, V(x).dtype, i);
            const long inner = sz->host_i[i] * unit, o = off;
            P.add_step("Split " + op.m_name, {x}, {y}, [=, this] { be.check(be.api.osg_copy_2d(be.ctx, es, P.ptr(x), src_pitch, o, P.ptr(y), inner, 0, outer, inner), "Split"); });
            off += inner;
        }
    }

    // Slice (reference :6499-6695): last or last-but-one axis, step 1, one or two axes.  Without an `axes` input EVERY (start, end) pair applies to the last axis,
    // the second pair to the result of the first (the reference's last_but_one is only ever set from `axes`, :6529-6554)
    void lower_slice(const Operation& op) {
        need(op, op.m_input.size() >= 3 && op.m_input.size() <= 5, "wrong number of inputs.");
        need(op, op.m_attributes.empty(), "unrecognized attribute (not implemented).");
        int x = P.ensure_plain(in_val(op.m_input[0]));
        const Val* st = hval(op.m_input[1]);
        const Val* en = hval(op.m_input[2]);
        const Val* ax = op.m_input.size() > 3 ? hval(op.m_input[3]) : nullptr;
        const Val* sp = op.m_input.size() > 4 ? hval(op.m_input[4]) : nullptr;
        need(op, st && en && st->dtype == OSG_I64 && en->dtype == OSG_I64, "wrong data type of starts.");
        const size_t na = st->host_i.size();
        need(op, (na == 1 || na == 2) && en->host_i.size() == na, "unsupported shape of starts (not implemented).");
        int cur = x;
        for (size_t k = 0; k < na; k++) {
            const Shape s = V(cur).shape;
            const int rank = (int)s.size();
            int axis = rank - 1;
            if (ax) { need(op, ax->host_i.size() == na, "unsupported shape of axes (not implemented)."); axis = (int)ax->host_i[k]; if (axis < 0) axis += rank; }
            need(op, axis == rank - 1 || axis == rank - 2, "unsupported axes value(s): slice supported on last or last but one axis only (not implemented).");
            if (sp) need(op, sp->host_i.size() == na && sp->host_i[k] == 1, "unsupported steps value(s) (not implemented).");
            long dim = s[axis], b = st->host_i[k], e = en->host_i[k];
            if (b < 0) b += dim;
            if (b > dim - 1) b = dim - 1;
            if (e < 0) e += dim;
            if (e > dim) e = dim;
            need(op, b >= 0 && e >= 0 && b < e, "invalid value(s) in starts and/or ends.");
            Shape os = s;
            os[axis] = e - b;
            const bool last = k + 1 == na;
            int y = last ? out_val(op, os, Lay::plain, V(cur).batched, V(cur).dtype) : P.new_val("", os, V(cur).dtype, Lay::plain, V(cur).batched);
            const int es = (int)esize(V(cur).dtype);
            const long unit = prod(s, axis + 1), outer = prod(s, 0, axis) * B(cur), src_pitch = dim * unit, inner = (e - b) * unit, off = b * unit;
            const int src = cur;
            P.add_step("Slice " + op.m_name, {src}, {y}, [=, this] { be.check(be.api.osg_copy_2d(be.ctx, es, P.ptr(src), src_pitch, off, P.ptr(y), inner, 0, outer, inner), "Slice"); });
            cur = y;
        }
    }

    // Resize (reference :6120-6315): nearest / asymmetric / floor, scales or sizes
    void lower_resize(const Operation& op) {
        need(op, op.m_input.size() == 3 || op.m_input.size() == 4, "wrong number of inputs.");
        for (auto& a : op.m_attributes) {
            if (a.first == "coordinate_transformation_mode") need(op, a.second == "asymmetric", "coordinate_transformation_mode must be asymmetric (not implemented).");
            else if (a.first == "mode") need(op, a.second == "nearest", "mode must be nearest (not implemented).");
            else if (a.first == "nearest_mode") need(op, a.second == "floor", "nearest_mode must be floor (not implemented).");
            else if (a.first == "cubic_coeff_a") {}
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        int x = in_val(op.m_input[0]);
        const Shape s = V(x).shape;
        need(op, s.size() == 4 && s[0] == 1, "input must be [1,C,H,W] (not implemented).");
        Shape os = s;
        if (op.m_input.size() == 4 && !op.m_input[3].m_name.empty()) {
            const Val* sz = hval(op.m_input[3]);
            need(op, sz && sz->host_i.size() == 4, "invalid sizes.");
            for (int i = 0; i < 4; i++) os[i] = sz->host_i[i];
        } else {
            const Val* sc = hval(op.m_input[2]);
            need(op, sc && sc->host_valid && sc->host_f.size() == 4, "invalid scales.");
            need(op, sc->host_f[0] == 1.f && sc->host_f[1] == 1.f, "scales for N and C must be 1 (not implemented).");
            for (int i = 2; i < 4; i++) os[i] = (long)std::floor((float)s[i] * sc->host_f[i]);
        }
        need(op, os[0] == s[0] && os[1] == s[1], "resize of N/C not supported.");
        const bool nhwc = V(x).lay == Lay::nhwc;
        int y = out_val(op, os, V(x).lay, V(x).batched, V(x).dtype);
        const int es = (int)esize(V(x).dtype);
        const long nb = B(x);
        P.add_step("Resize " + op.m_name, {x}, {y}, [=, this] {
            be.check(be.api.osg_resize_nearest(be.ctx, es, P.ptr(x), P.ptr(y), (int)nb, (int)s[1], (int)s[2], (int)s[3], (int)os[2], (int)os[3], nhwc ? 1 : 0), "Resize");
        });
    }

    // MaxPool (reference :8075-8148 -> XnnPack::maxpool_nhwc :1536)
    void lower_maxpool(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        std::vector<int> ks, pads = {0, 0, 0, 0}, strides = {1, 1};
        for (auto& a : op.m_attributes) {
            if (a.first == "kernel_shape") ks = int_list(a.second);
            else if (a.first == "pads") pads = int_list(a.second);
            else if (a.first == "strides") strides = int_list(a.second);
            else if (a.first == "ceil_mode") need(op, std::stoi(a.second) == 0, "ceil_mode != 0 not supported.");
            else if (a.first == "dilations") { for (int d : int_list(a.second)) need(op, d == 1, "dilations != 1 not supported."); }
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        need(op, ks.size() == 2 && pads.size() == 4 && strides.size() == 2, "invalid attributes.");
        int x = P.ensure_nhwc(in_val(op.m_input[0]));
        const Shape s = V(x).shape;
        const long Ho = (s[2] + pads[0] + pads[2] - ks[0]) / strides[0] + 1, Wo = (s[3] + pads[1] + pads[3] - ks[1]) / strides[1] + 1;
        int y = out_val(op, {s[0], s[1], Ho, Wo}, Lay::nhwc, V(x).batched);
        const long nb = B(x);
        // pads re-centred as the reference does (:1553-1558, like Conv): the total per direction, the odd cell at the bottom / on the right
        const int ph = pads[0] + pads[2], pw = pads[1] + pads[3];
        const int pt = ph / 2, pb = ph - pt, pl = pw / 2, pr = pw - pl;
        P.add_step("MaxPool " + op.m_name, {x}, {y}, [=, this] {
            be.check(be.api.osg_maxpool_nhwc(be.ctx, OSG_F16, P.ptr(x), P.ptr(y), (int)nb, (int)s[2], (int)s[3], (int)s[1], ks[0], ks[1], strides[0], strides[1],
                                             pt, pl, pb, pr),
                     "MaxPool");
        });
    }
