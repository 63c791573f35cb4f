// part of struct Lowering (plan.cpp): lowering of the uint8-arithmetic plan (m_use_uint8_arithmetic, the W8A8 VAE decoder): one launch per graph op, bit-exact codes.
    // ==================================================================================================================
    // uint8 arithmetic (m_use_uint8_arithmetic; the reference's W8A8 path -- in practice the VAE decoder of `sd --rpi-lowmem`,
    // src/sd.cpp:1212-1222).  One launch per graph op: every op re-quantises to its OWN (scale, zero point) -- derived from
    // range_data.txt by Model::range_to_scale exactly where the reference derives them -- so nothing may be fused without changing
    // codes.  Quantisation parameters are read from the vals at RUN time (a pushed input is quantised per run, reference :3024-3028).
    // ==================================================================================================================
    qu8::QParams out_q(const Operation& op) {
        auto it = m.m_range_data.find(op.m_name);
        if (it == m.m_range_data.end()) throw std::invalid_argument(op.m_type + ": range data not found.");
        return qu8::range_to_scale(it->second.first, it->second.second);
    }
    int out_val_u8(const Operation& op, const Shape& shape, Lay lay, bool batched, qu8::QParams q) {
        int y = out_val(op, shape, lay, batched, OSG_U8);
        V(y).qscale = q.scale;
        V(y).qzp = (int)q.zero_point;
        return y;
    }
    void need_u8(const Operation& op, int v, const char* what) {
        if (V(v).dtype != OSG_U8) throw std::invalid_argument(op.m_type + ": wrong data type of " + what + ".");
    }
    // a 256-byte device table that lives as long as the plan
    void* lut_alloc(size_t bytes) {
        return P.small_alloc(bytes);
    }

    void lower_u8(const Operation& op) {
        const std::string& t = op.m_type;
        if (t == "Conv") return lower_conv_u8(op);
        if (t == "MatMul") return lower_matmul_u8(op);
        if (t == "Add" || t == "Mul") return lower_binary_u8(op);
        if (t == "Sigmoid") return lower_sigmoid_u8(op);
        if (t == "InstanceNormalization") return lower_instance_norm_u8(op);
        if (t == "osg.qu8.InstanceNormNHWC") return lower_instance_norm_u8_nhwc(op);
        if (t == "osg.qu8.AffineAct" || t == "osg.qu8.NormAffineAct") return lower_affine_act_u8(op);
        if (t == "Softmax") return lower_softmax_u8(op);
        if (t == "Reshape" || t == "Flatten" || t == "Unsqueeze" || t == "Squeeze" || t == "Transpose" || t == "Resize") {
            // the codes are re-arranged, scale and zero point carried over (reference :4783, :5231, :6251, :8185) -- except by Squeeze and Unsqueeze, which
            // hand the codes on WITHOUT them (reference :3901, :7470 copy type and data only): their output has scale 0 and zero point 0, whatever the input's
            const int x = in_val_raw(op.m_input[0]);
            if (t == "Reshape") lower_reshape(op);
            else if (t == "Flatten") lower_flatten(op);
            else if (t == "Unsqueeze" || t == "Squeeze") lower_squeeze(op, t == "Unsqueeze");
            else if (t == "Transpose") lower_transpose(op);
            else lower_resize(op);
            const int y = P.by_name.at(op.m_output[0].m_name);
            if (t == "Unsqueeze" || t == "Squeeze") {
                if (V(y).dtype == OSG_U8) P.own_q(y, 0.f, 0);
            } else
                P.share_q(y, x);
            return;
        }
        throw std::invalid_argument("Model::run: operation not implemented with uint8 arithmetic on the HIP backend: " + t);
    }

    // Conv, uint8 branch (reference :4629-4690 -> XnnPack::convolution<uint8_t,int32_t> :1292)
    void lower_conv_u8(const Operation& op) {
        need(op, op.m_input.size() == 2 || op.m_input.size() == 3, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        std::vector<int> dil = {1, 1}, ks, pads = {0, 0, 0, 0}, strides = {1, 1};
        int group = 1;
        for (auto& a : op.m_attributes) {
            if (a.first == "dilations") dil = int_list(a.second);
            else if (a.first == "group") group = std::stoi(a.second);
            else if (a.first == "kernel_shape") ks = int_list(a.second);
            else if (a.first == "pads") pads = int_list(a.second);
            else if (a.first == "strides") strides = int_list(a.second);
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        int x = in_val(op.m_input[0]);
        need(op, V(x).shape.size() == 4, "Conv1D / non 4-D input not implemented on the HIP backend.");
        for (int d : dil) need(op, d == 1, "dilations != 1 not supported (not implemented).");
        need(op, group == 1, "group != 1 not supported (not implemented).");
        need(op, pads.size() == 4 && strides.size() == 2, "invalid pads/strides.");
        need_u8(op, x, "X");
        x = P.ensure_nhwc(x);
        const int w = in_val(op.m_input[1]);
        need_u8(op, w, "W");
        const Shape ws = V(w).shape, xs = V(x).shape;
        need(op, V(w).is_const && V(w).lay == Lay::nhwc && ws.size() == 4, "weights must be a static *_nchw.bin tensor.");
        need(op, xs[0] == 1 && N == 1, "uint8 arithmetic runs one sample per pass (every pushed sample has its own scale).");
        const long Cin = xs[1], H = xs[2], W = xs[3], Cout = ws[0], KH = ws[2], KW = ws[3];
        need(op, ws[1] == Cin, "invalid shape of weights.");
        if (!ks.empty()) need(op, ks.size() == 2 && ks[0] == KH && ks[1] == KW, "kernel_shape does not match the weights.");
        const int ph = pads[0] + pads[2], pw = pads[1] + pads[3];
        const int pt = ph / 2, pb = ph - pt, pl = pw / 2, pr = pw - pl;
        const long Ho = (H + ph - KH) / strides[0] + 1, Wo = (W + pw - KW) / strides[1] + 1;
        int bias = -1;
        if (op.m_input.size() == 3 && !op.m_input[2].m_name.empty()) {
            bias = in_val(op.m_input[2]);
            need(op, V(bias).numel() == Cout && V(bias).dtype == OSG_F32, "wrong data type of B.");
        }
        const qu8::QParams oq = out_q(op);
        const int y = out_val_u8(op, {1, Cout, Ho, Wo}, Lay::nhwc, V(x).batched, oq);
        const int sh = strides[0], sw = strides[1];
        std::vector<int> reads = {x, w};
        if (bias >= 0) reads.push_back(bias);
        // the pipelined kernel's table of code sums per filter tap (include/osgpu.h osg_qu8_conv2d_nhwc_t): a function of the weight alone, so a weight
        // that stays at its address gets it once, here (kept with the Model's constants under the weight's name); a weight that travels through the
        // streaming ring (VRAM budget) has none -- the library then rebuilds it in its workspace before every launch
        int* taps = nullptr;
        if (V(w).dptr && (pt || pl || pb || pr) && KH * KW <= 32) {
            bool fresh;
            taps = (int*)P.const_alloc(V(w).name + "|q8taps", (size_t)Cout * KH * KW * sizeof(int), &fresh);
            if (fresh) be.check(be.api.osg_qu8_conv_tap_sums(be.ctx, V(w).dptr, (int)Cout, (int)KH, (int)KW, (int)Cin, taps), "osg_qu8_conv_tap_sums");
        }
        P.add_step("Conv qu8 " + op.m_name, reads, {y}, [=, this] {
            const Val& qx = P.qv(x);
            be.check(be.api.osg_qu8_conv2d_nhwc_t(be.ctx, P.ptr(x), qx.qscale, qx.qzp, P.ptr(w), P.vals[w].qscale, P.vals[w].qzp,
                                                  bias >= 0 ? (const float*)P.ptr(bias) : nullptr, oq.scale, (int)oq.zero_point, P.ptr(y), 1, (int)H, (int)W, (int)Cin,
                                                  (int)Cout, (int)KH, (int)KW, sh, sw, pt, pl, pb, pr, taps),
                     "Conv");
        });
        P.steps.back().flops = 2.0 * Ho * Wo * Cout * KH * KW * Cin;
    }

    // MatMul, uint8 branch (reference :5779-5837 -> XnnPack::matrix_multiply<uint8_t> :1035): [.., M,K] x [K,N] weight or batched [n,M,K] x [n,K,N]
    void lower_matmul_u8(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        need(op, N == 1, "uint8 arithmetic runs one sample per pass (every pushed sample has its own scale).");
        int a = P.ensure_plain(in_val(op.m_input[0])), b = in_val(op.m_input[1]);
        need_u8(op, a, "input");
        need_u8(op, b, "input");
        const qu8::QParams oq = out_q(op);
        if (V(b).is_const && V(b).shape.size() == 2) {
            const Shape as = V(a).shape;
            const long K = V(b).shape[0], Nn = V(b).shape[1];
            need(op, !as.empty() && as.back() == K, "invalid shape of inputs.");
            const int wq = weight_nk_u8(b);
            Shape os = as;
            os.back() = Nn;
            const int y = out_val_u8(op, os, Lay::plain, V(a).batched, oq);
            const long M = prod(as) / K;
            P.add_step("MatMul qu8 " + op.m_name, {a, wq}, {y}, [=, this] {
                const Val& qa = P.qv(a);
                be.check(be.api.osg_qu8_gemm(be.ctx, P.ptr(a), K, qa.qscale, qa.qzp, P.ptr(wq), P.vals[wq].qscale, P.vals[wq].qzp, nullptr, oq.scale,
                                             (int)oq.zero_point, P.ptr(y), (int)M, (int)Nn, (int)K, 1, 0, 0, 0),
                         "MatMul");
            });
            P.steps.back().flops = 2.0 * M * Nn * K;
            return;
        }
        b = P.ensure_plain(b);
        Shape as = V(a).shape, bs = V(b).shape;
        bool lead1 = false;
        if (as.size() == 4 && as[0] == 1) { as.erase(as.begin()); lead1 = true; }
        if (bs.size() == 4 && bs[0] == 1) bs.erase(bs.begin());
        need(op, as.size() == 3 && bs.size() == 3 && as[0] == bs[0] && as[2] == bs[1], "invalid shape of inputs.");
        const long n = as[0], M = as[1], K = as[2], Nn = bs[2];
        Shape os = {n, M, Nn};
        if (lead1) os.insert(os.begin(), 1);
        const int y = out_val_u8(op, os, Lay::plain, false, oq);
        // the [K,N] operand is an activation: re-laid out to K-contiguous [N,K] by a transpose launch of its own
        const int bt = P.new_val("", {n, Nn, K}, OSG_U8, Lay::plain, false);
        P.add_step("MatMul qu8/T " + op.m_name, {b}, {bt}, [=, this] {
            long sh[3] = {n, K, Nn};
            int pm[3] = {0, 2, 1};
            be.check(be.api.osg_transpose(be.ctx, 1, P.ptr(b), P.ptr(bt), 3, sh, pm), "MatMul");
        });
        // (b is listed as read although the launch takes its codes from bt: the launch reads b's PARAMETERS, and a step that reads a value quantised per run has to
        // lie in the eager prefix of the pass -- Plan::dyn_end goes by the reads)
        P.add_step("MatMul qu8 " + op.m_name, {a, bt, b}, {y}, [=, this] {
            const Val &qa = P.qv(a), &qb = P.qv(b);
            be.check(be.api.osg_qu8_gemm(be.ctx, P.ptr(a), K, qa.qscale, qa.qzp, P.ptr(bt), qb.qscale, qb.qzp, nullptr, oq.scale, (int)oq.zero_point, P.ptr(y),
                                         (int)M, (int)Nn, (int)K, (int)n, M * K, Nn * K, M * Nn),
                     "MatMul");
        });
        P.steps.back().flops = 2.0 * n * M * Nn * K;
    }

    // Add / Mul, uint8 branches (reference :5105-5124, :3977-3996 -> XnnPack::add / multiply with quint8 parameters)
    void lower_binary_u8(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        int a = in_val(op.m_input[0]), b = in_val(op.m_input[1]);
        need_u8(op, a, "inputs");
        need_u8(op, b, "inputs");
        const osg_binary_kind kind = op.m_type == "Add" ? OSG_BIN_ADD : OSG_BIN_MUL;
        const Shape as = V(a).shape, bs = V(b).shape;
        const size_t rank = std::max(as.size(), bs.size());
        Shape os(rank);
        for (size_t i = 0; i < rank; i++) {
            long da = i + as.size() >= rank ? as[i + as.size() - rank] : 1;
            long db = i + bs.size() >= rank ? bs[i + bs.size() - rank] : 1;
            need(op, da == db || da == 1 || db == 1, "shapes are not broadcastable.");
            os[i] = std::max(da, db);
        }
        auto per_channel = [&](int v, long C) {
            const Shape& s = V(v).shape;
            if (V(v).lay == Lay::nhwc) return false;
            if (V(v).numel() == 1) return true;
            if (V(v).numel() != C) return false;
            return (s.size() == 3 && s[0] == C) || (s.size() == 4 && s[1] == C);
        };
        Lay olay = Lay::plain;
        Shape pa, pb;
        if (V(a).lay == Lay::nhwc || V(b).lay == Lay::nhwc) {
            int x = V(a).lay == Lay::nhwc ? a : b, o = x == a ? b : a;
            const Shape xs = V(x).shape;
            const long C = xs[1], HW = xs[2] * xs[3];
            if (V(o).shape == xs && xs.size() == 4) {
                // same-shape operands: stay channels-last (the convolutions either side want it); a plain operand is transposed ONCE here instead of
                // the NHWC one being transposed now and the result transposed back in front of the next convolution
                if (V(o).lay != Lay::nhwc) {
                    const int on = P.ensure_nhwc(o);
                    (o == a ? a : b) = on;
                }
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
        const qu8::QParams oq = out_q(op);
        const int y = out_val_u8(op, os, olay, V(a).batched || V(b).batched, oq);
        const size_t prank = std::max(pa.size(), pb.size());
        const size_t pr = std::max<size_t>(prank, 1);
        need(op, pr <= 6, "rank too large for the device broadcast kernel.");
        std::vector<long> sa(pr, 1), sb(pr, 1);
        for (size_t i = 0; i < pa.size(); i++) sa[pr - pa.size() + i] = pa[i];
        for (size_t i = 0; i < pb.size(); i++) sb[pr - pb.size() + i] = pb[i];
        P.add_step(op.m_type + " qu8 " + op.m_name, {a, b}, {y}, [=, this] {
            const Val &qa = P.qv(a), &qb = P.qv(b);
            be.check(be.api.osg_qu8_binary(be.ctx, kind, P.ptr(a), sa.data(), qa.qscale, qa.qzp, P.ptr(b), sb.data(), qb.qscale, qb.qzp, P.ptr(y), oq.scale,
                                           (int)oq.zero_point, (int)pr),
                     op.m_type.c_str());
        });
    }

    // Sigmoid, uint8 branch (reference :4412-4481): a function of the input code -> 256-entry table built on the host with the host's expf
    void lower_sigmoid_u8(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        const int x = in_val(op.m_input[0]);
        need_u8(op, x, "input");
        const qu8::QParams oq = out_q(op);
        const int y = out_val_u8(op, V(x).shape, V(x).lay, V(x).batched, oq);
        const long n = P.total_elems(x);
        void* lut = lut_alloc(256);
        const bool dyn = P.qv(x).qdyn;
        auto build = [=, this] {
            const Val& qx = P.qv(x);
            uint8_t t[256];
            qu8::sigmoid_lut(qu8::QParams{qx.qscale, (uint8_t)qx.qzp}, oq, t);
            be.check(be.api.osg_upload_sync(be.ctx, lut, t, 256), "osg_upload_sync");
        };
        if (!dyn) build();
        P.add_step("Sigmoid qu8 " + op.m_name, {x}, {y}, [=, this] {
            if (dyn) build();      // the input scale changes from run to run: rebuild (256 expf) before the lookup
            be.check(be.api.osg_qu8_lut(be.ctx, P.ptr(x), P.ptr(y), n, lut), "Sigmoid");
        });
    }

    // InstanceNormalization, uint8 branch (reference :4987-5043): input [1,G,L]
    void lower_instance_norm_u8(const Operation& op) {
        need(op, op.m_input.size() == 3, "wrong number of inputs.");
        const int x = P.ensure_plain(in_val(op.m_input[0]));
        need_u8(op, x, "input");
        const int sc = in_val(op.m_input[1]), bi = in_val(op.m_input[2]);
        const Shape s = V(x).shape;
        need(op, s.size() == 3 && s[0] == 1, "input shape must be [1,G,L] (not implemented).");
        need(op, V(sc).numel() == s[1] && V(bi).numel() == s[1] && V(sc).dtype == OSG_F32 && V(bi).dtype == OSG_F32, "invalid scale/bias.");
        float eps = 1e-5f;
        for (auto& a : op.m_attributes) {
            if (a.first == "epsilon") eps = std::stof(a.second);
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        const qu8::QParams oq = out_q(op);
        const int y = out_val_u8(op, s, Lay::plain, V(x).batched, oq);
        const long rows = s[1], L = s[2];
        P.add_step("InstanceNorm qu8 " + op.m_name, {x, sc, bi}, {y}, [=, this] {
            const Val& qx = P.qv(x);
            be.check(be.api.osg_qu8_instance_norm(be.ctx, P.ptr(x), P.ptr(y), (int)rows, L, (int)rows, (const float*)P.ptr(sc), (const float*)P.ptr(bi), eps, qx.qscale,
                                                  qx.qzp, oq.scale, (int)oq.zero_point),
                     "InstanceNormalization");
        });
    }

    qu8::QParams range_q(const Operation& op, const std::string& name) {
        auto it = m.m_range_data.find(name);
        if (it == m.m_range_data.end()) throw std::invalid_argument(op.m_type + ": range data not found.");
        return qu8::range_to_scale(it->second.first, it->second.second);
    }
    void lower_affine_act_u8(const Operation& op) {
        const bool normed = op.m_type == "osg.qu8.NormAffineAct";
        int x = in_val(op.m_input[0]);
        const int g = in_val(op.m_input[1]), b = in_val(op.m_input[2]);
        need_u8(op, x, "inputs");
        need_u8(op, g, "inputs");
        need_u8(op, b, "inputs");
        const Shape s = V(x).shape;
        need(op, s.size() == 4 && s[0] == 1, "input shape must be [1,C,H,W] (not implemented).");
        const long C = s[1], HW = s[2] * s[3], n = P.total_elems(x);
        need(op, V(g).numel() == C && V(b).numel() == C, "invalid shape of the per-channel operands.");
        const qu8::QParams qm = range_q(op, *attr(op, "mul")), qa = range_q(op, *attr(op, "add"));
        const bool silu = attr(op, "sigmoid") != nullptr;
        qu8::QParams qs{}, qo = qa;
        void* lut = nullptr;
        if (silu) {
            qs = range_q(op, *attr(op, "sigmoid"));
            qo = range_q(op, *attr(op, "mul2"));
            lut = lut_alloc(256);
            uint8_t t[256];
            qu8::sigmoid_lut(qa, qs, t);          // (the Sigmoid's input is the Add's output: parameters from range data, never dynamic)
            be.check(be.api.osg_upload_sync(be.ctx, lut, t, 256), "osg_upload_sync");
        }
        int sc = -1, bi = -1;
        float eps = 1e-5f;
        long G = 0;
        qu8::QParams qn{};
        if (normed) {
            sc = in_val(op.m_input[3]), bi = in_val(op.m_input[4]);
            if (auto* e = attr(op, "norm_epsilon")) eps = std::stof(*e);
            if (auto* gr = attr(op, "norm_groups")) G = std::stol(*gr);
            need(op, G > 0 && C % G == 0 && V(sc).numel() == G && V(bi).numel() == G && V(sc).dtype == OSG_F32 && V(bi).dtype == OSG_F32, "invalid scale/bias.");
            qn = range_q(op, *attr(op, "norm"));
            if (V(x).lay != Lay::nhwc) {
                // the producer left it in the logical layout: the [G][L] row kernels as they are, then the affine pass below on their output
                const int xi = P.ensure_plain(x), nv = P.new_val("", s, OSG_U8, Lay::plain, V(x).batched);
                V(nv).qscale = qn.scale;
                V(nv).qzp = (int)qn.zero_point;
                const long L = (C / G) * HW;
                P.add_step("InstanceNorm qu8 " + *attr(op, "norm"), {xi, sc, bi}, {nv}, [=, this] {
                    const Val& qx = P.qv(xi);
                    be.check(be.api.osg_qu8_instance_norm(be.ctx, P.ptr(xi), P.ptr(nv), (int)G, L, (int)G, (const float*)P.ptr(sc), (const float*)P.ptr(bi), eps, qx.qscale, qx.qzp,
                                                          qn.scale, (int)qn.zero_point),
                             "InstanceNormalization");
                });
                x = nv;
            }
        }
        if (normed && V(x).lay == Lay::nhwc) {
            const int y = out_val_u8(op, s, Lay::nhwc, V(x).batched, qo);
            P.add_step("NormAffineAct qu8 " + op.m_name, {x, g, b, sc, bi}, {y}, [=, this] {
                const Val &qx = P.qv(x), &qg = P.qv(g), &qb = P.qv(b);
                be.check(be.api.osg_qu8_norm_affine_act_nhwc(be.ctx, P.ptr(x), HW, (int)C, (int)G, (int)G, (const float*)P.ptr(sc), (const float*)P.ptr(bi), eps, qx.qscale, qx.qzp,
                                                             qn.scale, (int)qn.zero_point, P.ptr(g), qg.qscale, qg.qzp, qm.scale, (int)qm.zero_point, P.ptr(b), qb.qscale, qb.qzp,
                                                             qa.scale, (int)qa.zero_point, lut, qs.scale, (int)qs.zero_point, qo.scale, (int)qo.zero_point, P.ptr(y)),
                         "NormAffineAct");
            });
            return;
        }
        const int y = out_val_u8(op, s, V(x).lay, V(x).batched, qo);
        const long inner = V(x).lay == Lay::nhwc ? 1 : HW;
        P.add_step("AffineAct qu8 " + op.m_name, {x, g, b}, {y}, [=, this] {
            const Val &qx = P.qv(x), &qg = P.qv(g), &qb = P.qv(b);
            be.check(be.api.osg_qu8_affine_act(be.ctx, P.ptr(x), qx.qscale, qx.qzp, P.ptr(g), qg.qscale, qg.qzp, qm.scale, (int)qm.zero_point, P.ptr(b), qb.qscale, qb.qzp,
                                               qa.scale, (int)qa.zero_point, lut, qs.scale, (int)qs.zero_point, qo.scale, (int)qo.zero_point, P.ptr(y), n, (int)C, inner),
                     "AffineAct");
        });
    }

    void lower_instance_norm_u8_nhwc(const Operation& op) {
        const int x0 = in_val(op.m_input[0]);
        need_u8(op, x0, "input");
        const int sc = in_val(op.m_input[1]), bi = in_val(op.m_input[2]);
        const Shape s = V(x0).shape;
        need(op, s.size() == 4 && s[0] == 1, "input shape must be [1,C,H,W] (not implemented).");
        float eps = 1e-5f;
        long G = 0;
        for (auto& a : op.m_attributes) {
            if (a.first == "epsilon") eps = std::stof(a.second);
            else if (a.first == "groups") G = std::stol(a.second);
            else throw std::invalid_argument("InstanceNormalization: unrecognized attribute: " + a.first + ".");
        }
        const long C = s[1], HW = s[2] * s[3];
        need(op, G > 0 && C % G == 0, "invalid number of groups.");
        need(op, V(sc).numel() == G && V(bi).numel() == G && V(sc).dtype == OSG_F32 && V(bi).dtype == OSG_F32, "invalid scale/bias.");
        const qu8::QParams oq = out_q(op);
        if (V(x0).lay != Lay::nhwc) {
            // the producer left it in the logical layout: the plain [G][L] kernels apply as they are (rows are contiguous there)
            const int x = P.ensure_plain(x0);
            const int y = out_val_u8(op, s, Lay::plain, V(x).batched, oq);
            const long L = (C / G) * HW;
            P.add_step("InstanceNorm qu8 " + op.m_name, {x, sc, bi}, {y}, [=, this] {
                const Val& qx = P.qv(x);
                be.check(be.api.osg_qu8_instance_norm(be.ctx, P.ptr(x), P.ptr(y), (int)G, L, (int)G, (const float*)P.ptr(sc), (const float*)P.ptr(bi), eps, qx.qscale, qx.qzp,
                                                      oq.scale, (int)oq.zero_point),
                         "InstanceNormalization");
            });
            return;
        }
        const int x = x0;
        const int y = out_val_u8(op, s, Lay::nhwc, V(x).batched, oq);
        P.add_step("InstanceNorm qu8 nhwc " + op.m_name, {x, sc, bi}, {y}, [=, this] {
            const Val& qx = P.qv(x);
            be.check(be.api.osg_qu8_instance_norm_nhwc(be.ctx, P.ptr(x), P.ptr(y), HW, (int)C, (int)G, (int)G, (const float*)P.ptr(sc), (const float*)P.ptr(bi), eps, qx.qscale,
                                                       qx.qzp, oq.scale, (int)oq.zero_point),
                     "InstanceNormalization");
        });
    }

    // Softmax, uint8 branch (reference :5960-5975 -> XnnPack::softmax<uint8_t>): last axis; output scale 1/256, zero point 0
    void lower_softmax_u8(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        const int x = P.ensure_plain(in_val(op.m_input[0]));
        need_u8(op, x, "input");
        const Shape s = V(x).shape;
        int axis = -1;
        for (auto& a : op.m_attributes) {
            if (a.first == "axis") axis = std::stoi(a.second);
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        if (axis < 0) axis += (int)s.size();
        need(op, axis == (int)s.size() - 1, "uint8 softmax over a non-last axis is not implemented on the HIP backend.");
        const int y = out_val_u8(op, s, Lay::plain, V(x).batched, qu8::QParams{0x1.0p-8f, 0});
        const long C = s.back(), rows = P.total_elems(x) / C;
        void* lut = lut_alloc(256 * 4);
        const bool dyn = P.qv(x).qdyn;
        auto build = [=, this] {
            uint32_t t[256];
            qu8::softmax_lut(P.qv(x).qscale, (size_t)C, t);
            be.check(be.api.osg_upload_sync(be.ctx, lut, t, sizeof t), "osg_upload_sync");
        };
        if (!dyn) build();
        P.add_step("Softmax qu8 " + op.m_name, {x}, {y}, [=, this] {
            if (dyn) build();
            be.check(be.api.osg_qu8_softmax_last(be.ctx, P.ptr(x), P.ptr(y), rows, C, lut), "Softmax");
        });
    }

    // Gather on the device (reference :6316-6498): rows of a [rows, els] view along axis 0 (leading 1-dims stripped), static int64 indices
    void lower_gather(const Operation& op) {
        need(op, op.m_input.size() == 2, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        int axis = 0;
        for (auto& a : op.m_attributes) {
            if (a.first == "axis") axis = std::stoi(a.second);
            else throw std::invalid_argument(op.m_type + ": unrecognized attribute: " + a.first + ".");
        }
        // decode plans: the indices are a device value (the token / its position, Val::dev_int) -- the launch reads the staging buffer itself, and
        // Plan::generate checks the table's rows against what the loop can produce (dec_tok_limit / dec_pos_limit)
        int dev_idx = -1;
        if (P.decode && !is_const_tensor(op.m_input[1])) {
            auto it = P.by_name.find(op.m_input[1].m_name);
            if (it != P.by_name.end() && V(P.root_of(it->second)).dev_int) dev_idx = it->second;
        }
        const Val* iv = dev_idx >= 0 ? &P.vals[dev_idx] : hval(op.m_input[1]);
        need(op, iv && iv->dtype == OSG_I64 && (iv->host_valid || dev_idx >= 0), "wrong data type of indices.");
        int x = P.ensure_plain(in_val(op.m_input[0]));
        Shape xs = V(x).shape;
        if (axis < 0) axis += (int)xs.size();
        const int prev_axis = axis;
        while (axis > 0 && !xs.empty() && xs[0] == 1) { xs.erase(xs.begin()); axis--; }
        need(op, axis == 0, "axis must be 0 (not implemented).");
        const bool in1d = xs.size() == 1;
        if (in1d) xs.insert(xs.begin(), 1);
        Shape is = iv->shape;
        const bool idx0d = is.empty();
        if (idx0d) is.push_back(1);
        const bool idx1d = is.size() == 1;
        if (idx1d) is.insert(is.begin(), 1);
        need(op, is.size() == 2 && is[0] == 1, "shape of indices must be (1,D) (not implemented).");
        Shape over;
        if (xs.size() > 2) {
            over.assign(xs.begin() + 1, xs.end());
            xs = {xs[0], prod(over)};
        }
        need(op, xs.size() == 2, "input must be 2D or more.");
        Shape os = {1, is[1], xs[1]};
        if (in1d && idx0d) os.clear();
        else if (idx1d) os.erase(os.begin());
        for (int i = 0; i < prev_axis; i++) os.insert(os.begin(), 1);
        if (!over.empty()) os = over;
        const long dim = in1d ? xs[1] : xs[0], els = in1d ? 1 : xs[1];
        std::vector<int64_t> idx = iv->host_i;
        for (auto& i : idx) {
            if (i < 0) i += dim;
            need(op, i >= 0 && i < dim, "invalid index in indices.");
        }
        int idev = dev_idx;
        if (dev_idx >= 0) {
            long& limit = V(P.root_of(dev_idx)).name == P.dspec.pos ? P.dec_pos_limit : P.dec_tok_limit;
            limit = std::min(limit, dim);
        } else {
            idev = P.new_val("", {(long)idx.size()}, OSG_I64, Lay::plain, false);
            V(idev).is_const = true;
            bool fresh;
            std::string tag = "gather|" + op.m_name;
            V(idev).dptr = P.const_alloc(tag, std::max<size_t>(idx.size() * 8, 8), &fresh);
            be.check(be.api.osg_upload_sync(be.ctx, V(idev).dptr, idx.data(), idx.size() * 8), "osg_upload_sync");
        }
        // a decode plan of N sequences: the device indices are one set per sequence, stacked -- one launch gathers all of them from the shared table
        const bool idx_batched = dev_idx >= 0 && V(dev_idx).batched;
        need(op, !(idx_batched && V(x).batched), "per-sample indices into per-sample data are not implemented.");
        int y = out_val(op, os, Lay::plain, V(x).batched || idx_batched, V(x).dtype);
        const int es = (int)esize(V(x).dtype);
        const long nb = B(x), n_idx = dev_idx >= 0 ? P.total_elems(dev_idx) : (long)idx.size(), per_in = V(x).numel(), per_out = n_idx * els;
        P.add_step("Gather " + op.m_name, {x, idev}, {y}, [=, this] {
            for (long b = 0; b < nb; b++)
                be.check(be.api.osg_gather_rows(be.ctx, es, (const char*)P.ptr(x) + b * per_in * es, (const int64_t*)P.ptr(idev), (char*)P.ptr(y) + b * per_out * es, n_idx,
                                                els, dim),
                         "Gather");
        });
    }

    // Cast on the device (reference :7352-7423): the device keeps f16 activations only, so FLOAT -> FLOAT16 / FLOAT are relabelings there
    void lower_cast(const Operation& op) {
        need(op, op.m_input.size() == 1, "wrong number of inputs.");
        need(op, op.m_output.size() == 1, "wrong number of outputs.");
        throw std::invalid_argument(op.m_type + ": requested cast not implemented (only casts of plan-time integer values are supported on the HIP backend).");
    }

    // m_requires_upcast (reference get_tensor_data :2847-2848: the operands of a flagged op are handed over as fp32, the op runs in fp32; its fp32
    // result stays fp32 only while the NEXT op is its sole consumer, push_tensor :3008-3034): cur_up is set while a flagged op is lowered
    bool cur_up = false;
    std::map<int, int> cast_cache32, cast_cache16;
    int cast_val(int v, osg_dtype to) {
        auto& cache = to == OSG_F32 ? cast_cache32 : cast_cache16;
        auto it = cache.find(v);
        if (it != cache.end()) return it->second;
        const int src = P.ensure_plain(v);
        const int y = P.new_val("", V(src).shape, to, Lay::plain, V(src).batched);
        V(y).up32 = to == OSG_F32;
        const osg_dtype from = V(src).dtype;
        const long n = P.total_elems(src);
        P.add_step(std::string(to == OSG_F32 ? "upcast " : "downcast ") + V(src).name, {src}, {y}, [=, this] {
            be.check(be.api.osg_convert(be.ctx, from, to, P.ptr(src), P.ptr(y), n, 1.f, 0), "osg_convert");
        });
        cache[v] = y;
        return y;
    }
    int in_val(const Tensor& t) {
        const int v = P.ensure_dense(in_val_raw(t));
        if (cur_up && V(v).dtype == OSG_F16) return cast_val(v, OSG_F32);
        if (!cur_up && V(v).up32) return cast_val(v, OSG_F16);
        return v;
    }

    void check_out(const Operation& op, const Shape& got, size_t idx = 0) {
        // the reference's per-op self check (check_output_shape, :3070)
        const auto& want = op.m_output[idx].m_shape;
        bool ok = want.size() == got.size();
        for (size_t i = 0; ok && i < got.size(); i++) ok = (long)want[i] == got[i] || (m.m_support_dynamic_shapes && want[i] == 0);
        if (!ok && !(m.m_support_dynamic_shapes && want.empty()))
            throw std::invalid_argument(op.m_type + ": unexpected shape of output. (" + op.m_name + ": computed " + shape_str(got) + ")");
    }

    int out_val(const Operation& op, const Shape& shape, Lay lay, bool batched, osg_dtype dt = OSG_F16, size_t idx = 0) {
        check_out(op, shape, idx);
        return P.new_val(op.m_output[idx].m_name, shape, dt, lay, batched);
    }

    long B(int v) { return V(v).batched ? N : 1; }

    bool upcast_op(const Operation& op) const { return P.fp16 && !P.u8 && m.m_requires_upcast && m.m_requires_upcast(op.m_type, op.m_name); }
    void lower_all() {
        plan_linear_groups();
        if ((m.m_requires_upcast || P.sdp_attn) && !indexed) {   // (the op list no longer changes: one index serves the whole lowering)
            dead.assign(ops().size(), 0);                         // (run_fusions compacted the list: the flags of the old positions mean nothing now)
            index_graph();
            indexed = true;
        }
        static const bool per_type = std::getenv("OSG_PLAN_TIMING") && std::atoi(std::getenv("OSG_PLAN_TIMING")) >= 2;   // host microseconds of the lowering per op type
        std::map<std::string, std::pair<double, int>> type_us;
        for (size_t i = 0; i < ops().size(); i++) {
            const auto t_op = std::chrono::steady_clock::now();
            struct Acc {
                std::map<std::string, std::pair<double, int>>& m; const std::string& t; std::chrono::steady_clock::time_point t0; bool on;
                ~Acc() { if (on) { auto& e = m[t]; e.first += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); e.second++; } }
            } acc{type_us, ops()[i].m_type, t_op, per_type};
            if (i + 1 == ops().size() && per_type) {
                fprintf(stderr, "[plan] lowering by op type (us, ops):");
                for (auto& e : type_us) fprintf(stderr, " %s %.0f/%d", e.first.c_str(), e.second.first, e.second.second);
                fprintf(stderr, "\n");
            }
            if (group_of.count((int)i)) lower_group_member(ops()[i], (int)i);
            else if (ops()[i].m_type == "osg.RMSNorm") lower(ops()[i]);   // (fp32 inside by construction: fuse_rms_norm only fuses fully flagged chains)
            else if (upcast_op(ops()[i])) {
                const Operation& op = ops()[i];
                const std::string& t = op.m_type;
                if (!try_host_eval(op)) {
                    if (!(t == "Pow" || t == "ReduceMean" || t == "Add" || t == "Sub" || t == "Mul" || t == "Div" || t == "Sqrt" || t == "Neg" || t == "Sigmoid" || t == "Erf" ||
                          t == "Sin" || t == "Cos"))
                        throw std::invalid_argument("Model::run: m_requires_upcast is not implemented on the HIP backend for operation " + t + " (" + op.m_name + ").");
                    cur_up = true;
                    try { lower(op); } catch (...) { cur_up = false; throw; }
                    cur_up = false;
                    // push_tensor: the fp32 result is rounded to fp16 unless the next op of the queue is its only consumer
                    auto it = P.by_name.find(op.m_output[0].m_name);
                    if (it != P.by_name.end() && V(it->second).up32) {
                        bool keep = i + 1 < ops().size() && use_count(op.m_output[0].m_name) == 1;
                        if (keep) {
                            keep = false;
                            for (auto& ti : ops()[i + 1].m_input) keep |= ti.m_name == op.m_output[0].m_name;
                        }
                        if (!keep) {
                            const int h = cast_val(it->second, OSG_F16);
                            V(h).name = op.m_output[0].m_name;
                            P.by_name[op.m_output[0].m_name] = h;
                        }
                    }
                }
            } else lower(ops()[i]);
            if (P.calibrate)      // m_range_data_calibrate: every op output is measured right after the launch(es) that produce it
                for (auto& o : ops()[i].m_output) {
                    auto it = P.by_name.find(o.m_name);
                    if (it != P.by_name.end() && V(it->second).dtype == OSG_F16 && !V(it->second).host_only)
                        P.calib.push_back(Plan::Calib{(int)std::max<size_t>(P.steps.size(), 1) - 1, ops()[i].m_name, it->second});
                }
        }
    }

