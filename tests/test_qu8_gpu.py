"""GPU: the uint8-arithmetic kernels (osg_qu8_*, onnxstream_amd/csrc/osg_qu8.hip) against the specification oracle/np_qu8.py -- the numpy
restatement of the reference's uint8 ops that tests/test_qu8_oracle.py pins code for code against the reference's own intermediates.
Everything here is BIT-EXACT (north_star: "bit-exact for int8 indexing"): array_equal on the codes, through the C ABI."""
import numpy as np
import pytest

from oracle import np_qu8 as Q

pytestmark = pytest.mark.gpu
f32 = np.float32


def _codes(rng, shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,pad", [(1, 12, 10, 32, 48, 3, 1, 1), (2, 9, 7, 16, 20, 3, 2, 1), (1, 16, 16, 4, 32, 3, 1, 1),
                                                         (1, 8, 8, 64, 64, 1, 1, 0), (1, 20, 20, 128, 3, 3, 1, 1), (1, 5, 6, 20, 30, 3, 1, 1),
                                                         (1, 64, 64, 128, 128, 3, 1, 1), (1, 33, 31, 48, 70, 3, 1, 1)])
@pytest.mark.parametrize("tile", [64, 128])
def test_qu8_conv(gpu, N, H, W, Cin, Cout, k, stride, pad, tile, monkeypatch):
    monkeypatch.setenv("OSG_QU8_V2", "0")             # the register-staged kernel this test names (the pipelined one would take the 64 x 64 x 128 shape first)
    monkeypatch.setenv("OSG_QU8_TILE", str(tile))     # both tile instantiations on every shape (128 x 128 only takes the 16-byte-chunk shapes)
    rng = np.random.default_rng(Cin * 100 + Cout + k)
    x, w = _codes(rng, (N, H, W, Cin)), _codes(rng, (Cout, k, k, Cin))
    sx, zx, sw, zw = f32(0.0173), 117, f32(0.0042), 131
    bias = (rng.standard_normal(Cout) * 0.5).astype(f32)
    so, zo = f32(float(sx) * float(sw) * np.sqrt(k * k * Cin) * 75.0 / 2.0), 120
    for b in (bias, None):
        want = Q.conv2d_nhwc_u8(x, sx, zx, w, sw, zw, b, (pad,) * 4, (stride, stride), so, zo)
        got = gpu.qu8_conv2d_nhwc(gpu.to_dev(x), (sx, zx), gpu.to_dev(w), (sw, zw), gpu.to_dev(b) if b is not None else None, (so, zo), stride, (pad,) * 4).numpy()
        assert want.min() < 30 and want.max() > 220          # the output range is exercised, saturation included
        assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("batch,M,N,K", [(1, 77, 64, 128), (1, 200, 96, 40), (3, 64, 64, 64), (2, 50, 33, 48), (1, 256, 256, 512), (1, 5, 3, 7)])
@pytest.mark.parametrize("tile", [64, 128])
def test_qu8_gemm(gpu, batch, M, N, K, tile, monkeypatch):
    monkeypatch.setenv("OSG_QU8_V2", "0")
    monkeypatch.setenv("OSG_QU8_TILE", str(tile))
    rng = np.random.default_rng(M + N + K)
    a = _codes(rng, (batch, M, K) if batch > 1 else (M, K))
    b = _codes(rng, (batch, K, N) if batch > 1 else (K, N))
    sa, za, sb, zb = f32(0.021), 140, f32(0.0105), 99
    so, zo = f32(float(sa) * float(sb) * np.sqrt(K) * 75.0 / 2.0), 128
    want = Q.matmul_u8(a, sa, za, b, sb, zb, so, zo)
    b_nk = np.ascontiguousarray(np.swapaxes(b, -1, -2))
    got = gpu.qu8_gemm(gpu.to_dev(a), (sa, za), gpu.to_dev(b_nk), (sb, zb), None, (so, zo)).numpy()
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,pad", [(1, 64, 64, 128, 128, 3, 1, 1), (1, 20, 24, 256, 192, 3, 1, 1), (1, 17, 19, 128, 64, 3, 2, 1), (2, 16, 16, 128, 132, 1, 1, 0),
                                                         (1, 9, 40, 384, 256, 3, 1, 1), (1, 12, 12, 128, 128, 5, 1, 2)])
@pytest.mark.parametrize("nst", [2, 3, 4])
@pytest.mark.parametrize("tile", [64, 128, 256])
def test_qu8_conv_pipelined_kernel(gpu, N, H, W, Cin, Cout, k, stride, pad, nst, tile, monkeypatch):
    """q8_gemm2_kernel (LDS-DMA ring, codes re-biased after the fragment read, zero-filled halo settled from the per-weight tap sums in the epilogue) against the
    specification: border rows and corners, M / N tails, strides, every ring depth.  OSG_QU8_V2=2 takes it for every legal shape, however small."""
    if tile == 256 and nst == 4:
        pytest.skip("the 256 x 128 eight-wave tile has rings of depth 2 and 3")
    monkeypatch.setenv("OSG_QU8_V2", "2")
    monkeypatch.setenv("OSG_QU8_NST", str(nst))
    monkeypatch.setenv("OSG_QU8_V2_TILE", str(min(tile, 128)))     # 64 x 64 (four waves of 32 x 32), 128 x 128 (four of 64 x 64), 256 x 128 (eight of 64 x 64)
    if tile == 256:
        monkeypatch.setenv("OSG_QU8_WGM", "4")
    rng = np.random.default_rng(Cin * 100 + Cout + k + H)
    x, w = _codes(rng, (N, H, W, Cin)), _codes(rng, (Cout, k, k, Cin))
    sx, zx, sw, zw = f32(0.0173), 117, f32(0.0042), 131
    bias = (rng.standard_normal(Cout) * 0.5).astype(f32)
    so, zo = f32(float(sx) * float(sw) * np.sqrt(k * k * Cin) * 75.0 / 2.0), 120
    dw = gpu.to_dev(w)          # (one device weight for both launches: the second one finds its tap-sum table)
    for b in (bias, None):
        want = Q.conv2d_nhwc_u8(x, sx, zx, w, sw, zw, b, (pad,) * 4, (stride, stride), so, zo)
        got = gpu.qu8_conv2d_nhwc(gpu.to_dev(x), (sx, zx), dw, (sw, zw), gpu.to_dev(b) if b is not None else None, (so, zo), stride, (pad,) * 4).numpy()
        assert want.min() < 30 and want.max() > 220
        assert np.array_equal(got, want), int((got != want).sum())
    monkeypatch.setenv("OSG_QU8_V2", "0")
    old = gpu.qu8_conv2d_nhwc(gpu.to_dev(x), (sx, zx), dw, (sw, zw), None, (so, zo), stride, (pad,) * 4).numpy()
    assert np.array_equal(old, got)


@pytest.mark.parametrize("batch,M,N,K", [(1, 256, 256, 512), (2, 200, 132, 256), (1, 77, 64, 128), (3, 130, 128, 384)])
@pytest.mark.parametrize("nst", [2, 3, 4])
@pytest.mark.parametrize("tile", [64, 128])
def test_qu8_gemm_pipelined_kernel(gpu, batch, M, N, K, nst, tile, monkeypatch):
    monkeypatch.setenv("OSG_QU8_V2", "2")
    monkeypatch.setenv("OSG_QU8_NST", str(nst))
    monkeypatch.setenv("OSG_QU8_V2_TILE", str(tile))
    rng = np.random.default_rng(M + N + K)
    a = _codes(rng, (batch, M, K) if batch > 1 else (M, K))
    b = _codes(rng, (batch, K, N) if batch > 1 else (K, N))
    sa, za, sb, zb = f32(0.021), 140, f32(0.0105), 99
    so, zo = f32(float(sa) * float(sb) * np.sqrt(K) * 75.0 / 2.0), 128
    want = Q.matmul_u8(a, sa, za, b, sb, zb, so, zo)
    b_nk = np.ascontiguousarray(np.swapaxes(b, -1, -2))
    got = gpu.qu8_gemm(gpu.to_dev(a), (sa, za), gpu.to_dev(b_nk), (sb, zb), None, (so, zo)).numpy()
    assert np.array_equal(got, want), int((got != want).sum())


def test_qu8_sigmoid_lut(gpu):
    rng = np.random.default_rng(3)
    x = _codes(rng, (1, 32, 16, 16))
    si, zi, so, zo = f32(0.0713), 130, f32(1.0 / 255), 0
    lut = Q.sigmoid_u8(np.arange(256, dtype=np.uint8), si, zi, so, zo)
    got = gpu.qu8_lut(gpu.to_dev(x), lut).numpy()
    assert np.array_equal(got, Q.sigmoid_u8(x, si, zi, so, zo))


@pytest.mark.parametrize("kind", ["add", "mul"])
@pytest.mark.parametrize("ash,bsh", [((1, 16, 16, 32), (1, 16, 16, 32)), ((1, 16, 16, 32), (32,)), ((1, 32, 8, 8), (32, 1, 1)), ((1, 7, 5), (1, 7, 5)),
                                     ((4, 64, 64), (1,)), ((32, 1, 1), (1, 32, 9, 7)), ((1, 1, 1, 48), (2, 5, 7, 48)), ((3, 1, 5), (3, 4, 5)), ((1, 130, 130, 16), ())])
def test_qu8_binary(gpu, kind, ash, bsh):
    rng = np.random.default_rng(len(ash) * 7 + len(bsh))
    a, b = _codes(rng, ash), _codes(rng, bsh)
    for (sa, za, sb, zb, so, zo) in ((f32(0.031), 120, f32(0.017), 131, f32(0.045 if kind == "add" else 0.0125), 125),
                                    (f32(0.0042826), 0, f32(0.00154), 123, f32(0.0061 if kind == "add" else 0.00007), 40)):
        fn = Q.add_u8 if kind == "add" else Q.mul_u8
        want = fn(a, sa, za, b, sb, zb, so, zo)
        got = gpu.qu8_binary(kind, gpu.to_dev(a), (sa, za), gpu.to_dev(b), (sb, zb), (so, zo)).numpy()
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), int((got != want).sum())


@pytest.mark.parametrize("rows,L", [(8, 1024), (32, 4096), (3, 77), (16, 65536)])
def test_qu8_instance_norm(gpu, rows, L):
    rng = np.random.default_rng(rows + L)
    # codes with structure (a bell around a per-row centre), like real activations
    x = np.clip(np.rint(rng.standard_normal((1, rows, L)) * 35 + rng.integers(60, 190, (1, rows, 1))), 0, 255).astype(np.uint8)
    si, zi, so, zo = f32(0.0193), 113, f32(0.0291), 128
    scale = (1.0 + 0.1 * rng.standard_normal(rows)).astype(f32)
    bias = (0.1 * rng.standard_normal(rows)).astype(f32)
    want = Q.instance_norm_u8(x, si, zi, scale, bias, 1e-6, so, zo)
    got = gpu.qu8_instance_norm(gpu.to_dev(x), (si, zi), gpu.to_dev(scale), gpu.to_dev(bias), 1e-6, (so, zo)).numpy()
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("HW,C,silu,nchw", [(256, 128, True, False), (77, 48, True, False), (1024, 512, False, False), (64, 40, True, True), (5, 7, False, True)])
def test_qu8_affine_act_equals_the_separate_launches(gpu, HW, C, silu, nchw):
    """one pass == Mul, Add, Sigmoid lookup, Mul as separate launches, code for code"""
    rng = np.random.default_rng(HW + C)
    shape = (1, C, HW, 1) if nchw else (1, HW, 1, C)          # the per-channel operand broadcasts against dim 1 (NCHW) or the last dim (NHWC)
    x = _codes(rng, shape)
    g, b = _codes(rng, (C,)), _codes(rng, (C,))
    xq, gq, mq, bq, aq, sq, oq = (f32(0.021), 118), (f32(0.011), 90), (f32(0.024), 121), (f32(0.013), 140), (f32(0.027), 117), (f32(1 / 256), 0), (f32(0.019), 15)
    cshape = (1, C, 1, 1) if nchw else (1, 1, 1, C)
    dx, dg, db = gpu.to_dev(x), gpu.to_dev(g.reshape(cshape)), gpu.to_dev(b.reshape(cshape))
    m = gpu.qu8_binary("mul", dx, xq, dg, gq, mq)
    a = gpu.qu8_binary("add", m, mq, db, bq, aq)
    want = a
    lut = None
    if silu:
        table = Q.sigmoid_u8(np.arange(256, dtype=np.uint8), aq[0], aq[1], sq[0], sq[1])
        lut = gpu.to_dev(table)
        sg = gpu.qu8_lut(a, table)
        want = gpu.qu8_binary("mul", a, aq, sg, sq, oq)
    got = gpu.qu8_affine_act(dx, xq, gpu.to_dev(g), gq, mq, gpu.to_dev(b), bq, aq, lut, sq, oq, C, HW if nchw else 1).numpy()
    assert np.array_equal(got, want.numpy()), int((got != want.numpy()).sum())


@pytest.mark.parametrize("H,W,C,G", [(16, 16, 128, 32), (8, 8, 512, 32), (33, 7, 96, 8), (4, 4, 40, 5), (64, 64, 256, 32)])
def test_qu8_instance_norm_nhwc_equals_the_row_kernels(gpu, H, W, C, G):
    """the NHWC addressing of the [1,G,L] InstanceNormalization gives the codes of the row-major kernels on the transposed tensor (and those are
    pinned against the reference restatement above)"""
    rng = np.random.default_rng(H + W + C)
    x_nhwc = _codes(rng, (H * W, C))
    scale, bias = (1 + rng.standard_normal(G) * 0.1).astype(f32), (rng.standard_normal(G) * 0.1).astype(f32)
    xq, oq = (f32(0.031), 121), (f32(0.024), 118)
    rows = np.ascontiguousarray(x_nhwc.reshape(H * W, G, C // G).transpose(1, 0, 2)).reshape(G, H * W * (C // G))     # [G][HW*cpg] in (pixel, channel) order
    want = gpu.qu8_instance_norm(gpu.to_dev(rows), xq, gpu.to_dev(scale), gpu.to_dev(bias), 1e-5, oq).numpy()
    want_nhwc = want.reshape(G, H * W, C // G).transpose(1, 0, 2).reshape(H * W, C)
    got = gpu.qu8_instance_norm_nhwc(gpu.to_dev(x_nhwc), G, xq, gpu.to_dev(scale), gpu.to_dev(bias), 1e-5, oq).numpy()
    assert np.array_equal(got, want_nhwc), int((got != want_nhwc).sum())


@pytest.mark.parametrize("H,W,C,G,silu", [(16, 16, 128, 32, True), (8, 8, 512, 32, True), (33, 7, 96, 8, False), (64, 64, 256, 32, True)])
def test_qu8_norm_affine_act_equals_the_two_ops(gpu, H, W, C, G, silu):
    """InstanceNormalization's per-group table applied inside the affine pass == the NHWC normalisation followed by the affine op, code for code"""
    rng = np.random.default_rng(H * W + C)
    x = _codes(rng, (H * W, C))
    scale, bias = (1 + rng.standard_normal(G) * 0.1).astype(f32), (rng.standard_normal(G) * 0.1).astype(f32)
    g, b = _codes(rng, (C,)), _codes(rng, (C,))
    xq, nq = (f32(0.031), 121), (f32(0.024), 118)
    gq, mq, bq, aq, sq, oq = (f32(0.011), 90), (f32(0.024), 121), (f32(0.013), 140), (f32(0.027), 117), (f32(1 / 256), 0), (f32(0.019), 15)
    lut = gpu.to_dev(Q.sigmoid_u8(np.arange(256, dtype=np.uint8), aq[0], aq[1], sq[0], sq[1])) if silu else None
    dx, ds, dbi, dg, db = gpu.to_dev(x), gpu.to_dev(scale), gpu.to_dev(bias), gpu.to_dev(g), gpu.to_dev(b)
    n = gpu.qu8_instance_norm_nhwc(dx, G, xq, ds, dbi, 1e-5, nq)
    want = gpu.qu8_affine_act(n, nq, dg, gq, mq, db, bq, aq, lut, sq, oq, C, 1).numpy()
    got = gpu.qu8_norm_affine_act_nhwc(dx, G, xq, ds, dbi, 1e-5, nq, dg, gq, mq, db, bq, aq, lut, sq, oq).numpy()
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("rows,C", [(64, 64), (256, 4096), (5, 1000), (3, 7)])
def test_qu8_softmax(gpu, rows, C):
    rng = np.random.default_rng(rows * C)
    x = np.clip(np.rint(rng.standard_normal((1, rows, C)) * 30 + 120), 0, 255).astype(np.uint8)
    si = f32(0.0625)
    want, so, zo = Q.softmax_u8(x, si, -1)
    qscale = min(float(np.iinfo(np.uint32).max) / C, 8388607.0)
    lut = np.rint(qscale * np.exp((np.arange(256, dtype=np.float64) - 255.0) * float(si))).astype(np.uint32)
    got = gpu.qu8_softmax_last(gpu.to_dev(x), lut).numpy()
    assert np.array_equal(got, want), int((got != want).sum())


# ---- the whole W8A8 graph through the product: model_* C API -> planner (uint8 lowering) -> osg_qu8_* -----------------------------------
def _run_vae_qu8(extra=()):
    import os
    import tempfile
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    from onnxstream_amd.synth import sd_vae
    from onnxstream_amd.synth.graph import DirSink
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_tiny_qu8.npz"))
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_vae.build_vae_decoder(DirSink(d), sd_vae.TINY_VAE, quant_all=True)
        open(d + "range_data.txt", "w", newline="").write(str(z["ranges"]))
        m = Model(b.LIB_HOST, 1, "ram+nocache")          # threads = 1: the chunking of the input's percentiles follows the thread count (reference :3104)
        m.hip_read_range_data(d + "range_data.txt")
        m.set_use_uint8_arithmetic(True)
        m.read_file(d + "model.txt")
        m.mangle_tensor_names = False                     # names as they stand in model.txt
        for e in extra:
            m.add_extra_output(e)
        outs = []
        # pass 2 re-quantises the input and must reproduce pass 1; from pass 2 on everything behind the dynamically quantised input is a captured
        # hipGraph, so pass 3 (another input => other input scale / zero point) and pass 4 (the first input again) check that the eager
        # prefix really feeds the replayed graph the parameters of THIS pass
        for zin in (z["z"], z["z"], (z["z"] * np.float32(0.37) + np.float32(0.2)).astype(np.float32), z["z"]):
            m.add_tensor("input_2E_1", zin)
            m.run()
            got = {n: m.get_tensor(n) for n in ("out_5F_image",) + tuple(extra)}
            outs.append({n: v[0] for n, v in got.items() if v is not None})
            m.clear_tensors()
        launches = m.hip_last_kernel_count()
        m.close()
        return z, d, outs, launches


def test_hip_vae_qu8_reproduces_the_reference_bit_for_bit():
    """BASELINE config 3's W8A8 half: the fully uint8 VAE decoder (exporter layout `quant_all`, calibrated range_data.txt) with
    m_use_uint8_arithmetic, as `sd --rpi-lowmem` runs it (src/sd.cpp:1212-1222).  tests/golden/vae_tiny_qu8.npz is the reference's own
    output (reproduced bit for bit by the oracle in tests/test_golden.py); the device must produce the same fp32 image, i.e. the same
    final codes -- which requires every one of the 174 ops upstream to produce the reference's codes."""
    z, _, outs, launches = _run_vae_qu8()
    assert np.array_equal(outs[0]["out_5F_image"], z["ref_u8"]), int((outs[0]["out_5F_image"] != z["ref_u8"]).sum())
    assert np.array_equal(outs[1]["out_5F_image"], z["ref_u8"])
    assert not np.array_equal(outs[2]["out_5F_image"], z["ref_u8"])
    assert np.array_equal(outs[3]["out_5F_image"], z["ref_u8"])
    assert 60 < launches < 200          # (174 graph ops: the layout-only and per-channel affine chains run as single launches)


def test_hip_vae_qu8_every_op_matches_the_reference_intermediates():
    """where oracle/_ref travelled: every op output of the uint8 VAE against the reference's own raw intermediates (oracle/qu8_check.py
    keeps them: codes + scale + zero point), dequantised with the same formula on both sides -> identical floats = identical codes"""
    import os
    from oracle import qu8_check as qc
    from oracle import ref as oref
    if not oref.available():
        pytest.skip("oracle/_ref not present")
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_tiny_qu8.npz"))
    import tempfile
    from onnxstream_amd.synth import sd_vae
    from onnxstream_amd.synth.graph import DirSink
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_vae.build_vae_decoder(DirSink(d), sd_vae.TINY_VAE, quant_all=True)
        ops, vals = qc.run_u8_all(d, {"input.1": z["z"]}, str(z["ranges"]))
    prod = {qc.tname(o): op["type"] for op in ops for o in op["outputs"]}
    names = [qc.tname(op["outputs"][0]) for op in ops if qc.tname(op["outputs"][0]) in vals]
    _, _, outs, _ = _run_vae_qu8(extra=names)
    checked = 0
    for n, pn in zip(names, names):
        v = vals[n]
        if v["dtype"] != 1:
            continue
        ref = ((v["data"].astype(np.int32) - v["zp"]).astype(np.float32) * v["scale"]).astype(np.float32)
        if prod.get(n) == "Conv":
            ref = ref.transpose(0, 3, 1, 2)
        if pn not in outs[0]:
            continue
        got = outs[0][pn]
        assert got.shape == ref.shape, (n, got.shape, ref.shape)
        assert np.array_equal(got, ref), (n, prod.get(n), int((got != ref).sum()), got.size)
        checked += 1
    assert checked >= 150


def test_hip_calibration_run_writes_usable_range_data():
    """m_range_data_calibrate on the device (`sd --rpi-lowmem --decoder-calibrate`, src/sd.cpp:1216-1241): a floating-point pass records the
    0.1 % percentiles of every op output under the op's name (push_tensor hook, src/onnxstream.cpp:2983-3003) and write_range_data saves
    them.  The reference calibrates in fp32 arithmetic, the device in f16, so the ranges agree to f16 accuracy, not bit for bit; the
    uint8 pass driven by the device's own range_data must be as close to the fp32 image as the reference's uint8 pass is."""
    import os
    import tempfile
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    from onnxstream_amd.synth import sd_vae
    from onnxstream_amd.synth.graph import DirSink
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_tiny_qu8.npz"))
    ref = {}
    for line in str(z["ranges"]).split("\r\n"):
        if line:
            n, lo, hi = line.rsplit(",", 2)
            ref[n] = (float(lo), float(hi))
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_vae.build_vae_decoder(DirSink(d), sd_vae.TINY_VAE, quant_all=True)
        m = Model(b.LIB_HOST, 1, "ram+nocache")
        m._set_option("range_data_calibrate", 1)
        m.set_use_fp16_arithmetic(True)
        m.read_file(d + "model.txt")
        m.add_tensor("input.1", z["z"])
        m.run()
        m.hip_write_range_data(d + "range_data.txt")
        m.close()
        ours = {}
        for line in open(d + "range_data.txt", newline="").read().split("\r\n"):
            if line:
                n, lo, hi = line.rsplit(",", 2)
                ours[n] = (float(lo), float(hi))
        assert set(ours) == set(ref), (sorted(set(ref) - set(ours))[:5], sorted(set(ours) - set(ref))[:5])
        worst = max(max(abs(ours[n][0] - ref[n][0]), abs(ours[n][1] - ref[n][1])) / (ref[n][1] - ref[n][0]) for n in ref)
        devs = sorted(((max(abs(ours[n][0] - ref[n][0]), abs(ours[n][1] - ref[n][1])) / (ref[n][1] - ref[n][0]), n) for n in ref), reverse=True)
        print(f"calibration: {len(ours)} ranges, worst deviation from the reference's fp32 calibration {worst:.2e} of the range; top:",
              [(round(v, 4), n[-40:], ours[n], ref[n]) for v, n in devs[:4]], "median", devs[len(devs) // 2][0])
        assert worst <= 5e-2
        m = Model(b.LIB_HOST, 1, "ram+nocache")
        m.hip_read_range_data(d + "range_data.txt")
        m.set_use_uint8_arithmetic(True)
        m.read_file(d + "model.txt")
        m.add_tensor("input.1", z["z"])
        m.run()
        got = m.get_tensor("out_image")[0]
        m.close()
    mx = float(np.abs(z["ref32"]).max())
    e_ref = float(np.abs(z["ref_u8"] - z["ref32"]).max()) / mx
    e_own = float(np.abs(got - z["ref32"]).max()) / mx
    print(f"uint8 pass on own calibration: {e_own:.3f} of max from the fp32 image (reference's uint8 pass: {e_ref:.3f})")
    assert e_own <= 1.5 * e_ref + 0.02
