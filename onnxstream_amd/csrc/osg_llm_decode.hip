// libosgpu: what surrounds the T = 1 pass of the reference LLM app's token loop (src/llm.cpp:472-496), so that a whole generate call is enqueued
// without one host round trip:
//   osg_decode_pick  <- the app's argmax over the last row of the logits (src/llm.cpp:355-370) and the loop's state advance: the token goes into the
//                       pass's input_ids staging, the cache length into position_ids, tokens[n_tokens++] = tok; end-of-sequence and the invalid
//                       argmax set the stop code, after which every further launch is a predicated no-op
//   osg_kv_append_at <- the cache Concat (pkv ++ new row, axis 2) in place: the new row of every head into a capacity buffer at the device-side row
// (osg_sdpa_len, the attention over such buffers, lives next to osg_sdpa in osg_attention.hip.)
#include "osg_common.h"

namespace {

// (value, index) of the scan "prev = -1.0f; take v when v >= prev" over a set of elements: the largest value >= -1, and among equals the LARGEST index.
// The start state (-1.0f, -1) is an element like any other: a real -1.0f at index i >= 0 beats it on the index.
struct Pick { float v; long i; };
__device__ __forceinline__ Pick pick_better(Pick a, Pick b) { return (b.v > a.v || (b.v == a.v && b.i > a.i)) ? b : a; }

constexpr int kPickThreads = 1024;

__global__ __launch_bounds__(kPickThreads) void decode_pick_kernel(const float* __restrict__ row, long V, long long eos_id, int* __restrict__ state,
                                                                   int64_t* __restrict__ input_ids, int64_t* __restrict__ position_ids,
                                                                   int64_t* __restrict__ tokens, long max_tokens) {
    // stopped, or the token budget of this call is spent: nothing is read or written any more (uniform: every lane sees the same state)
    if (state[3] != 0 || (long)state[2] >= max_tokens) return;
    __shared__ float sv[kPickThreads / 64];
    __shared__ long si[kPickThreads / 64];
    const int tid = threadIdx.x;
    Pick best{-1.0f, -1};
    for (long i = tid; i < V; i += kPickThreads) {   // ascending indices: `>=` keeps the later of two equal values, a NaN compares false
        const float v = row[i];
        if (v >= best.v) best = Pick{v, i};
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Pick o;
        o.v = __shfl_xor(best.v, off);
        o.i = __shfl_xor(best.i, off);
        best = pick_better(best, o);
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best.v; si[tid >> 6] = best.i; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kPickThreads / 64; w++) best = pick_better(best, Pick{sv[w], si[w]});
    const long tok = best.i;
    if (tok < 0) { state[3] = 2; return; }                       // "Invalid result of the Argmax."
    if (eos_id >= 0 && tok == (long)eos_id) { state[3] = 1; return; }
    const int n = state[2], len = state[1];
    tokens[n] = tok;
    input_ids[0] = tok;
    position_ids[0] = len;
    state[0] = len;
    state[1] = len + 1;
    state[2] = n + 1;
}

__global__ __launch_bounds__(256) void kv_append_at_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ cache, const int* __restrict__ row_p,
                                                           int kv_heads, long cap, int d) {
    const long row = *row_p;
    if (row < 0 || row >= cap) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)kv_heads * d) return;
    const long h = i / d, e = i - h * d;
    cache[(h * cap + row) * d + e] = src[i];
}

}  // namespace

extern "C" {

int osg_decode_pick(osg_ctx* ctx, const float* logits, long T, long V, long long eos_id, int* state, int64_t* input_ids, int64_t* position_ids,
                    int64_t* tokens, long max_tokens) {
    if (T <= 0 || V <= 0) OSG_FAIL(ctx, "osg_decode_pick: invalid shape of the logits");
    if (!logits || !state || !input_ids || !position_ids || !tokens) OSG_FAIL(ctx, "osg_decode_pick: null operand");
    if (max_tokens < 0 || max_tokens > 0x7fffffffL) OSG_FAIL(ctx, "osg_decode_pick: invalid token budget");
    hipLaunchKernelGGL(decode_pick_kernel, dim3(1), dim3(kPickThreads), 0, ctx->compute, logits + (T - 1) * V, V, eos_id, state, input_ids, position_ids,
                       tokens, max_tokens);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_kv_append_at(osg_ctx* ctx, const void* src, void* cache, const int* row, int kv_heads, long cap, int d) {
    if (kv_heads <= 0 || cap <= 0 || d <= 0) OSG_FAIL(ctx, "osg_kv_append_at: invalid shape of the cache");
    if (!src || !cache || !row) OSG_FAIL(ctx, "osg_kv_append_at: null operand");
    const long n = (long)kv_heads * d;
    hipLaunchKernelGGL(kv_append_at_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->compute, (const uint16_t*)src, (uint16_t*)cache, row,
                       kv_heads, cap, d);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

}  // extern "C"
