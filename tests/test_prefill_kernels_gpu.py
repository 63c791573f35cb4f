"""The kernels behind the device prefill of a chat turn (model_hip_turn), against what include/osgpu.h says of them.

* osg_sdpa_chunk bit for bit against osg_sdpa on compacted copies of the first base + C rows with the explicit causal mask built in numpy
  (m[i][j] = 0 for j <= base + i, else `masked`), for fp16 min and -inf as the barred value, over one and two query blocks (C = 80: the second
  partial) and bases on either side of a key tile's edge; then again with NaN bit patterns in k and v at and past base + C.
* its refusals;
* osg_kv_append_rows_at against numpy: every row of the chunk inside the buffer is written, rows outside it are not, nothing else changes;
* osg_prefill_stage: tokens, positions and the first row of a full and of a padded chunk."""
import numpy as np
import pytest

f16, f32 = np.float16, np.float32
pytestmark = pytest.mark.gpu
CAP = 192
FMIN = float(np.finfo(f16).min)


def causal_mask(C, base, masked):
    j = np.arange(base + C)[None, :]
    i = np.arange(C)[:, None]
    return np.where(j <= base + i, f32(0.0), f32(masked)).astype(f16)


@pytest.mark.parametrize("masked", [FMIN, -np.inf], ids=["fp16min", "neginf"])
@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (4, 2), (2, 2)])
def test_sdpa_chunk_has_the_bits_of_sdpa_with_the_explicit_causal_mask(gpu, D, Hq, Hkv, masked):
    rng = np.random.default_rng(D * 10 + Hq)
    k = rng.standard_normal((1, Hkv, CAP, D)).astype(f16)
    v = rng.standard_normal((1, Hkv, CAP, D)).astype(f16)
    dk, dv = gpu.to_dev(k), gpu.to_dev(v)
    scale = float(f16(1.0 / np.sqrt(D)))
    ran = 0
    for C in (1, 16, 64, 80):
        q = rng.standard_normal((1, Hq, C, D)).astype(f16)
        dq = gpu.to_dev(q)
        for base in (0, 1, 63, 64, 100):
            if base + C > CAP:
                continue
            L = base + C
            mask = causal_mask(C, base, masked)
            assert mask.shape == (C, L) and (mask[:, :base + 1] == 0).all()
            ref = gpu.sdpa(dq, gpu.to_dev(k[:, :, :L]), gpu.to_dev(v[:, :, :L]), gpu.to_dev(mask), scale).numpy()
            assert np.isfinite(ref.astype(f32)).all()
            dbase = gpu.to_dev(np.array([base, -7, -7, -7], np.int32))
            got = gpu.sdpa_chunk(dq, dk, dv, dbase, masked, scale).numpy()
            assert got.shape == (1, Hq, C, D) and got.tobytes() == ref.tobytes(), (C, base)
            # rows at and past base + C are never read: NaN bit patterns in them change nothing
            kn, vn = k.copy(), v.copy()
            kn.view(np.uint16)[:, :, L:] = 0x7E01
            vn.view(np.uint16)[:, :, L:] = 0xFFFF
            got = gpu.sdpa_chunk(dq, gpu.to_dev(kn), gpu.to_dev(vn), dbase, masked, scale).numpy()
            assert got.tobytes() == ref.tobytes(), ("nan tail", C, base)
            ran += 1
    assert ran == 20          # (every (C, base) of the table fits: 100 + 80 <= 192)


def test_sdpa_chunk_refuses_what_it_does_not_implement(gpu):
    from onnxstream_amd.osgpu import OsgError
    q, kv = gpu.to_dev(np.zeros((1, 2, 4, 16), f16)), gpu.to_dev(np.zeros((1, 1, 8, 16), f16))
    base = gpu.to_dev(np.array([0], np.int32))
    with pytest.raises(OsgError, match="osg_sdpa_chunk: a chunk holds at most 512 query rows"):
        gpu.sdpa_chunk(gpu.to_dev(np.zeros((1, 2, 513, 16), f16)), gpu.to_dev(np.zeros((1, 1, 520, 16), f16)), gpu.to_dev(np.zeros((1, 1, 520, 16), f16)), base, FMIN, 0.25)
    with pytest.raises(OsgError, match="osg_sdpa_chunk: .*scale > 0"):
        gpu.sdpa_chunk(q, kv, kv, base, FMIN, 0.0)
    with pytest.raises(OsgError, match="osg_sdpa_chunk: query heads"):
        gpu.sdpa_chunk(gpu.to_dev(np.zeros((1, 3, 4, 16), f16)), gpu.to_dev(np.zeros((1, 2, 8, 16), f16)), gpu.to_dev(np.zeros((1, 2, 8, 16), f16)), base, FMIN, 0.25)
    with pytest.raises(OsgError, match="osg_sdpa_chunk: null operand"):
        gpu.sdpa_chunk(q, kv, kv, None, FMIN, 0.25)


@pytest.mark.parametrize("Hkv,cap,d", [(2, 192, 16), (3, 5, 128), (1, 1, 8)])
def test_kv_append_rows_at_writes_the_rows_inside_the_buffer(gpu, Hkv, cap, d):
    rng = np.random.default_rng(cap)
    cache = rng.integers(0, 65536, (Hkv, cap, d)).astype(np.uint16)
    for C in (1, 3, 5):
        src = rng.integers(0, 65536, (Hkv, C, d)).astype(np.uint16)
        bases = {-1, cap - 1, cap}
        if C <= cap:
            bases |= {0, (cap - C) // 2, cap - C}
        for base in sorted(bases):
            dev = gpu.to_dev(cache)
            gpu.kv_append_rows_at(gpu.to_dev(src), dev, gpu.to_dev(np.array([base], np.int32)))
            want = cache.copy()
            for i in range(C):
                if 0 <= base + i < cap:          # a row outside [0, cap) is not written; the others still are
                    want[:, base + i, :] = src[:, i, :]
            if base == cap:
                assert np.array_equal(want, cache)
            assert np.array_equal(dev.numpy(), want), (C, base)


def test_prefill_stage_writes_tokens_positions_and_the_first_row(gpu):
    prompt = np.array([5, 9, 2, 7, 11, 3, 8], np.int64)
    dp = gpu.to_dev(prompt)
    C = 4
    for first, pos0 in ((0, 0), (4, 14)):
        ids, pos = gpu.to_dev(np.full(C, -3, np.int64)), gpu.to_dev(np.full(C, -4, np.int64))
        base = gpu.to_dev(np.array([-5, -6], np.int32))
        gpu.prefill_stage(dp, first, pos0, ids, pos, base)
        n = min(C, len(prompt) - first)
        assert list(ids.numpy()) == list(prompt[first:first + n]) + [0] * (C - n)
        assert list(pos.numpy()) == list(range(pos0, pos0 + n)) + [0] * (C - n)          # padding rows: token 0, position 0
        assert list(base.numpy()) == [pos0, -6]
