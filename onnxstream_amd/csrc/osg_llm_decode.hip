// libosgpu: what surrounds the T = 1 pass of the reference LLM app's token loop (src/llm.cpp:472-496), so that a whole generate call is enqueued
// without one host round trip:
//   osg_decode_pick  <- the app's argmax over the last row of the logits (src/llm.cpp:355-370) and the loop's state advance: the token goes into the
//                       pass's input_ids staging, the cache length into position_ids, tokens[n_tokens++] = tok; end-of-sequence and the invalid
//                       argmax set the stop code, after which every further launch is a predicated no-op
//   osg_decode_sample <- in the pick's place when the caller samples: temperature, top-k, top-p and a seeded draw over the same row by the integer rule
//                       of include/osgpu.h, then the same state advance
//   osg_decode_count, osg_decode_penalize, osg_decode_*_ext <- repetition, presence and frequency penalties and min-p: a count per vocabulary entry on the
//                       device, step 0 of the rule as a launch of its own into a scratch row (the radix passes read adjusted logits as they read raw
//                       ones), the min-p compare inside the weights, and the count of the appended token raised by the thread that appends it
//   osg_kv_append_at <- the cache Concat (pkv ++ new row, axis 2) in place: the new row of every head into a capacity buffer at the device-side row
//   osg_decode_sample_batch, osg_kv_append_at_batch <- the same two for n_seq sequences side by side, each with its own state (model_hip_generate_batch)
//   osg_kv_append_rows_at, osg_prefill_stage <- the prompt's half of a chat turn (model_hip_turn): the C new rows of a prefill chunk into the capacity
//                       buffer from the device-side row on, and the chunk's tokens, positions and first row into the staging of the chunk plan
// (osg_sdpa_len and osg_sdpa_chunk, the attention over such buffers, live next to osg_sdpa in osg_attention.hip.)
#include <cmath>
#include <cstring>
#include "osg_common.h"

namespace {

// (value, index) of the scan "prev = -1.0f; take v when v >= prev" over a set of elements: the largest value >= -1, and among equals the LARGEST index.
// The start state (-1.0f, -1) is an element like any other: a real -1.0f at index i >= 0 beats it on the index.
struct Pick { float v; long i; };
__device__ __forceinline__ Pick pick_better(Pick a, Pick b) { return (b.v > a.v || (b.v == a.v && b.i > a.i)) ? b : a; }

constexpr int kPickThreads = 1024;

__global__ __launch_bounds__(kPickThreads) void decode_pick_kernel(const float* __restrict__ row, long V, long long eos_id, int* __restrict__ state,
                                                                   int64_t* __restrict__ input_ids, int64_t* __restrict__ position_ids,
                                                                   int64_t* __restrict__ tokens, long max_tokens, int* __restrict__ counts) {
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
    if (counts) counts[tok] += 1;   // (one thread, one launch at a time on the stream: no atomic needed)
}

// ---- osg_decode_sample: the rule of include/osgpu.h.  One workgroup; every pass re-reads the row (coalesced, out of L1 / L2), nothing is sorted. ----
// Every token is one 52-bit composite c = (key << 20) | index, key an order-preserving image of its logit: descending c IS the order of step 1
// (value descending, index descending), and all composites differ.  top-k and top-p are both prefixes of that order, so each is one composite `cut`
// (kept: c >= cut), found by a radix descent over c from the top -- on counts for top-k, on the integer masses q for top-p.  The histograms are
// integer LDS atomics: their sums do not depend on the order the waves arrive in.
typedef unsigned long long u64;
constexpr int kSampleThreads = 1024, kSampleWaves = kSampleThreads / 64;
constexpr int kHistCopies = 8;   // the top byte of a float key takes few values: eight copies of each bin (lane & 7) spread the adds of one wave

struct SampleShared {
    u64 hist[256 * kHistCopies];   // [bin][copy]: the copies of one bin lie in neighbouring banks
    u64 bins[256];
    u64 wsum[kSampleWaves];
    u64 bc[4];
    u64 headq[4];
    uint32_t wkey[kSampleWaves];
    int wcnt[kSampleWaves];
};

__device__ __forceinline__ uint32_t sample_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
// q of step 3: floor(min(exp((v - m) * inv_t), 1) * 2^32); the product by 2^32 is exact, the conversion truncates.  Step 3b (min-p) is the compare
// on x: a token under x_min has no mass, as one whose q is 0 (x_min = -inf: off, the compare is never true -- x is no NaN here)
__device__ __forceinline__ u64 sample_q(float v, float m, float inv_t, float x_min) {
    const float x = (v - m) * inv_t;
    if (x < x_min) return 0;
    const float w = fminf(expf(x), 1.0f);
    return (u64)(w * 4294967296.0f);
}
// the composite of element i with value v; false for a NaN.  -0.0 and +0.0 are one value: both take the key of +0.0
__device__ __forceinline__ bool sample_comp(long i, float& v, u64& c) {
    if (v != v) return false;
    if (v == 0.0f) v = 0.0f;
    c = ((u64)sample_key(v) << 20) | (u64)i;
    return true;
}
// How a pass reads the row: 16-byte loads from the first aligned element on (`head` = the 0-3 elements before it), up to four per thread in flight.
// f(i, v) is called once for every element by exactly one thread, in no particular order.
__device__ __forceinline__ int sample_head(const float* row, long V) {
    const long a = (long)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);
    return (int)(a < V ? a : V);
}
template <class F>
__device__ __forceinline__ void sample_for_each(const float* __restrict__ row, long V, int head, F f) {
    const int tid = threadIdx.x;
    if (tid < head) f((long)tid, row[tid]);
    const long nvec = (V - head) / 4;
    const float4* __restrict__ p = (const float4*)(row + head);
    long j = tid;
    for (; j + 3 * kSampleThreads < nvec; j += 4 * kSampleThreads) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = p[j + u * kSampleThreads];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long i = head + 4 * (j + u * kSampleThreads);
            f(i, x[u].x); f(i + 1, x[u].y); f(i + 2, x[u].z); f(i + 3, x[u].w);
        }
    }
    for (; j + kSampleThreads < nvec; j += 2 * kSampleThreads) {
        const float4 x = p[j], y = p[j + kSampleThreads];
        const long i = head + 4 * j, k = i + 4 * kSampleThreads;
        f(i, x.x); f(i + 1, x.y); f(i + 2, x.z); f(i + 3, x.w);
        f(k, y.x); f(k + 1, y.y); f(k + 2, y.z); f(k + 3, y.w);
    }
    if (j < nvec) {
        const float4 x = p[j];
        const long i = head + 4 * j;
        f(i, x.x); f(i + 1, x.y); f(i + 2, x.z); f(i + 3, x.w);
    }
    const long t = head + 4 * nvec + tid;
    if (t < V) f(t, row[t]);
}
// four consecutive elements from i on, row + i 16-byte aligned; past the end of the row a NaN stands (no token)
__device__ __forceinline__ void sample_load4(const float* __restrict__ row, long V, long i, float (&v)[4]) {
    if (i + 3 < V) {
        const float4 x = *(const float4*)(row + i);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = i + k < V ? row[i + k] : __uint_as_float(0x7fc00000u);
    }
}
// max(1, floor(pm * qtot / 2^ps)) in 128-bit integer arithmetic; pm < 2^24, ps >= 23, so the result fits 64 bits
__device__ __forceinline__ u64 sample_threshold(u64 qtot, uint32_t pm, int ps) {
    const u64 lo = (u64)pm * qtot, hi = __umul64hi((u64)pm, qtot);
    const u64 t = ps >= 128 ? 0 : ps >= 64 ? hi >> (ps - 64) : (hi << (64 - ps)) | (lo >> ps);
    return t ? t : 1;
}
__device__ __forceinline__ u64 wave_sum(u64 s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
__device__ __forceinline__ u64 wave_scan(u64 s, int lane) {   // inclusive, lane order
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up(s, off);
        if (lane >= off) s += o;
    }
    return s;
}

// The largest composite `cut` for which the weights of {c >= cut} sum to at least the target; weight = 1 per token and target given (MASS false:
// 1 <= target <= number of tokens), or weight = q over the tokens with c >= floor_c and target = the top-p threshold of their total (MASS true).
// Seven digits from the top: the four bytes of the key, then the index as 8 + 8 + 4 bits.  It ends early once a whole bin is kept, which is the
// usual case after the key's four bytes (one token holds that key, or all its equals are kept): the lower bits of the cut are 0 then.
template <bool MASS>
__device__ u64 sample_select(const float* __restrict__ row, long V, int head, float m, float inv_t, float x_min, u64 floor_c, u64 target, uint32_t pm,
                             int ps, SampleShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63;
    u64 prefix = 0, above = 0;
    for (int d = 0; d < 7; d++) {
        const int shift = d < 4 ? 44 - 8 * d : d == 4 ? 12 : d == 5 ? 4 : 0;
        const int bits = d == 6 ? 4 : 8;
        for (int j = tid; j < 256 * kHistCopies; j += kSampleThreads) sh.hist[j] = 0;
        __syncthreads();
        sample_for_each(row, V, head, [&](long i, float v) {
            u64 c;
            if (!sample_comp(i, v, c)) return;
            if (((c ^ prefix) >> (shift + bits)) != 0) return;
            u64 w = 1;
            if (MASS) {
                if (c < floor_c) return;
                w = sample_q(v, m, inv_t, x_min);
                if (w == 0) return;
            }
            atomicAdd(&sh.hist[((c >> shift) & (u64)((1 << bits) - 1)) * kHistCopies + (lane & (kHistCopies - 1))], w);
        });
        __syncthreads();
        if (tid < 256) {
            u64 s = 0;
#pragma unroll
            for (int k = 0; k < kHistCopies; k++) s += sh.hist[tid * kHistCopies + k];
            sh.bins[tid] = s;
        }
        __syncthreads();
        if (tid < 64) {   // wave 0 walks the bins from the top: lane L owns bins 255 - 4L ... 252 - 4L
            u64 b[4], s = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                b[k] = sh.bins[255 - 4 * lane - k];
                s += b[k];
            }
            const u64 incl = wave_scan(s, lane);
            if (MASS && d == 0) target = sample_threshold(__shfl(incl, 63), pm, ps);
            const u64 hit = __ballot(above + incl >= target);   // (never 0: the target is at most the total)
            if (hit != 0 && lane == __ffsll((long long)hit) - 1) {
                u64 acc = above + incl - s;
                int k = 0;
                for (; k < 3; k++) {
                    if (acc + b[k] >= target) break;
                    acc += b[k];
                }
                sh.bc[0] = (u64)(255 - 4 * lane - k);
                sh.bc[1] = acc;
                sh.bc[2] = b[k];
                sh.bc[3] = target;
            }
        }
        __syncthreads();
        const u64 binw = sh.bc[2];
        prefix |= sh.bc[0] << shift;
        above = sh.bc[1];
        target = sh.bc[3];
        if (above + binw == target) return prefix;
        if (MASS && d == 3) {   // one key, one q: the bin holds binw / q equal tokens, of which the ceil((target - above) / q) largest indices are kept
            const u64 q = sample_q(sample_key_value((uint32_t)(prefix >> 20)), m, inv_t, x_min);
            if ((target - above + q - 1) / q * q == binw) return prefix;
        }
    }
    return prefix;
}

// Philox4x32-10, word 0 | word 1 << 32 of the output for key = (seed lo, seed hi), counter = (n lo, n hi, 0, 0)
__device__ __forceinline__ u64 sample_philox(u64 seed, u64 n) {
    uint32_t c0 = (uint32_t)n, c1 = (uint32_t)(n >> 32), c2 = 0, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (u64)c0 | ((u64)c1 << 32);
}

// the rule, for the workgroup that runs it: osg_decode_sample launches one over the one sequence, osg_decode_sample_batch one per sequence over its own
// row, state, staging slots, token list and seed -- ONE body, so the two cannot drift apart
__device__ __forceinline__ void decode_sample_body(const float* __restrict__ row, long V, long long eos_id, int* __restrict__ state,
                                                   int64_t* __restrict__ input_ids, int64_t* __restrict__ position_ids, int64_t* __restrict__ tokens,
                                                   long max_tokens, float inv_t, long top_k, uint32_t pm, int ps, u64 seed, u64 draw_base, float x_min,
                                                   int* __restrict__ counts) {
    const int n_tok = state[2];
    if (state[3] != 0 || (long)n_tok >= max_tokens) return;   // as osg_decode_pick: uniform, nothing is read or written any more
    __shared__ SampleShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- step 1: the largest value and the number of tokens that are no NaN (key 0 belongs to a NaN: no token has it) ----
    const int head = sample_head(row, V);
    uint32_t kmax = 0;
    int cnt = 0;
    sample_for_each(row, V, head, [&](long i, float v) {
        u64 c;
        if (!sample_comp(i, v, c)) return;
        kmax = max(kmax, (uint32_t)(c >> 20));
        cnt++;
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, off));
        cnt += __shfl_xor(cnt, off);
    }
    if (lane == 0) { sh.wkey[wave] = kmax; sh.wcnt[wave] = cnt; }
    __syncthreads();
    kmax = 0;
    cnt = 0;
    for (int w = 0; w < kSampleWaves; w++) { kmax = max(kmax, sh.wkey[w]); cnt += sh.wcnt[w]; }
    const float m = sample_key_value(kmax);
    if (cnt == 0 || (__float_as_uint(m) & 0x7fffffffu) == 0x7f800000u) {   // nothing to order, or +-inf on top: the invalid argmax
        if (tid == 0) state[3] = 2;
        return;
    }
    // ---- steps 2 and 4: the cut ----
    u64 cut = 0;
    if (top_k > 0 && top_k < (long)cnt) cut = sample_select<false>(row, V, head, m, inv_t, x_min, 0, (u64)top_k, 0, 0, sh);
    if (pm != 0) {
        const u64 p_cut = sample_select<true>(row, V, head, m, inv_t, x_min, cut, 0, pm, ps, sh);
        cut = p_cut > cut ? p_cut : cut;
    }
    // ---- step 5: the draw, in ascending index order, in two levels: wave w sums the indices [head + w * cw, head + (w + 1) * cw), every thread finds the
    // range in which the running sum passes t, the sixteen waves split THAT range again, and one wave walks a sixteenth of a sixteenth.  A lane holds four
    // consecutive tokens of a block of 256.  The 0-3 tokens of the head come first of all; they go through LDS. ----
    auto kept_q = [&](long i, float v) -> u64 {
        u64 c;
        if (!sample_comp(i, v, c) || c < cut) return 0;
        return sample_q(v, m, inv_t, x_min);
    };
    auto block_q = [&](long i, long hi, const float (&v)[4], u64 (&q)[4]) -> u64 {   // (tokens at and past `hi` belong to the next range, or to nobody)
        u64 sum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            q[k] = i + k < hi ? kept_q(i + k, v[k]) : 0;
            sum += q[k];
        }
        return sum;
    };
    auto range_sum = [&](long lo, long hi) -> u64 {
        u64 s = 0;
        for (long i = lo + 4 * lane; i < hi; i += 512) {
            float v0[4], v1[4];
            u64 q[4];
            sample_load4(row, V, i, v0);
            sample_load4(row, V, i + 256, v1);
            s += block_q(i, hi, v0, q);
            s += block_q(i + 256, hi, v1, q);
        }
        return wave_sum(s);
    };
    // which of the sixteen ranges holds t, given their sums in sh.wsum; base = the running sum before it (t lies in one of them)
    auto find_range = [&](u64 t, u64& base) -> int {
        int w = 0;
        for (; w < kSampleWaves - 1; w++) {
            const u64 s = sh.wsum[w];
            if (t < base + s) break;
            base += s;
        }
        return w;
    };
    const long cw = ((V - head + kSampleWaves - 1) / kSampleWaves + 255) / 256 * 256;
    {
        const long lo = head + (long)wave * cw;
        const u64 s = range_sum(lo, lo + cw < V ? lo + cw : V);
        if (lane == 0) sh.wsum[wave] = s;
        if (tid < 4) sh.headq[tid] = tid < head ? kept_q(tid, row[tid]) : 0;
    }
    __syncthreads();
    u64 Q = sh.headq[0] + sh.headq[1] + sh.headq[2];
    for (int w = 0; w < kSampleWaves; w++) Q += sh.wsum[w];
    const u64 t = __umul64hi(sample_philox(seed, draw_base + (u64)n_tok), Q);   // t < Q; Q >= 2^32: the first token of the order is always kept
    long tok = -1;
    u64 base = 0;
    for (int k = 0; k < 3 && tok < 0; k++) {
        base += sh.headq[k];
        if (t < base) tok = k;
    }
    if (tok >= 0) {
        if (tid != 0) return;
    } else {
        const int w1 = find_range(t, base);
        const long lo1 = head + (long)w1 * cw, hi1 = lo1 + cw < V ? lo1 + cw : V;
        const long cs = cw / kSampleWaves;   // (a multiple of 16: 16-byte loads stay aligned)
        __syncthreads();
        {
            const long lo = lo1 + (long)wave * cs;
            const u64 s = range_sum(lo, lo + cs < hi1 ? lo + cs : hi1);
            if (lane == 0) sh.wsum[wave] = s;
        }
        __syncthreads();
        const int w2 = find_range(t, base);
        if (wave != w2) return;
        const long lo = lo1 + (long)w2 * cs, hi = lo + cs < hi1 ? lo + cs : hi1;
        for (long i0 = lo; i0 < hi; i0 += 256) {
            float v[4];
            u64 q[4];
            const long i = i0 + 4 * lane;
            sample_load4(row, V, i, v);
            const u64 mine = block_q(i, hi, v, q);
            const u64 incl = wave_scan(mine, lane);
            const u64 hit = __ballot(base + incl > t);
            const u64 total = __shfl(incl, 63);   // (while every lane of the wave is still here)
            if (hit != 0) {
                if (lane != __ffsll((long long)hit) - 1) return;
                u64 acc = base + incl - mine;
                int k = 0;
                for (; k < 3; k++) {
                    acc += q[k];
                    if (acc > t) break;
                }
                tok = i + k;
                break;
            }
            base += total;
        }
    }
    if (tok < 0) return;   // (not reached: this wave's range holds t)
    if (eos_id >= 0 && tok == (long)eos_id) { state[3] = 1; return; }
    const int len = state[1];
    tokens[n_tok] = tok;
    input_ids[0] = tok;
    position_ids[0] = len;
    state[0] = len;
    state[1] = len + 1;
    state[2] = n_tok + 1;
    if (counts) counts[tok] += 1;   // (the one thread that appends)
}

__global__ __launch_bounds__(kSampleThreads) void decode_sample_kernel(const float* __restrict__ row, long V, long long eos_id, int* __restrict__ state,
                                                                       int64_t* __restrict__ input_ids, int64_t* __restrict__ position_ids,
                                                                       int64_t* __restrict__ tokens, long max_tokens, float inv_t, long top_k, uint32_t pm,
                                                                       int ps, u64 seed, u64 draw_base, float x_min, int* __restrict__ counts) {
    decode_sample_body(row, V, eos_id, state, input_ids, position_ids, tokens, max_tokens, inv_t, top_k, pm, ps, seed, draw_base, x_min, counts);
}

// workgroup s = sequence s: everything it touches is indexed by blockIdx.x alone (uniform: the seed is one scalar load)
__global__ __launch_bounds__(kSampleThreads) void decode_sample_batch_kernel(const float* __restrict__ logits, long V, long long eos_id, int* __restrict__ state,
                                                                             int64_t* __restrict__ input_ids, int64_t* __restrict__ position_ids,
                                                                             int64_t* __restrict__ tokens, long max_tokens, float inv_t, long top_k,
                                                                             uint32_t pm, int ps, const u64* __restrict__ seeds, u64 draw_base, float x_min,
                                                                             int* __restrict__ counts) {
    const long s = blockIdx.x;
    decode_sample_body(logits + s * V, V, eos_id, state + 4 * s, input_ids + s, position_ids + s, tokens + s * max_tokens, max_tokens, inv_t, top_k, pm, ps,
                       seeds[s], draw_base, x_min, counts ? counts + s * V : nullptr);
}

__global__ __launch_bounds__(256) void kv_append_at_batch_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ cache, const int* __restrict__ state,
                                                                 int kv_heads, long cap, int d) {
    const long b = blockIdx.y;
    const long row = state[4 * b];
    if (row < 0 || row >= cap) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)kv_heads * d) return;
    const long h = i / d, e = i - h * d;
    cache[((b * kv_heads + h) * cap + row) * d + e] = src[b * kv_heads * d + i];
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

// osg_kv_append_rows_at: one thread per 16-bit element of src [kv_heads][C][d]; a row outside [0, cap) is skipped, the others are written
__global__ __launch_bounds__(256) void kv_append_rows_at_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ cache, const int* __restrict__ base_p,
                                                                int kv_heads, int C, long cap, int d) {
    const long base = *base_p;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)kv_heads * C * d) return;
    const long e = i % d, r = (i / d) % C, h = i / ((long)d * C);
    const long row = base + r;
    if (row < 0 || row >= cap) return;
    cache[(h * cap + row) * d + e] = src[i];
}

// osg_prefill_stage: one workgroup; every number but the tokens is a kernel argument (the host knows where a chunk stands)
__global__ __launch_bounds__(256) void prefill_stage_kernel(const int64_t* __restrict__ prompt, long first, long n_valid, long pos0, int C,
                                                            int64_t* __restrict__ input_ids, int64_t* __restrict__ position_ids, int* __restrict__ base) {
    for (int i = threadIdx.x; i < C; i += 256) {
        const bool real = i < n_valid;
        input_ids[i] = real ? prompt[first + i] : 0;
        position_ids[i] = real ? pos0 + i : 0;
    }
    if (threadIdx.x == 0) *base = (int)pos0;
}

// osg_decode_count: one thread per token; integer atomics, so the table does not depend on the order the threads arrive in
__global__ __launch_bounds__(256) void decode_count_kernel(const int64_t* __restrict__ tokens, long n, int* __restrict__ counts, long V) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long t = (long)tokens[i];
    if (t < 0 || t >= V) return;
    atomicAdd(&counts[t], 1);
}

// step 0 of the rule for one element: every product and sum is rounded on its own.  __fmul_rn and its kin are plain operators to this compiler, which
// contracts a product and a sum into an fma by default: the pragma and the empty asm below are what keep the roundings apart.
__device__ __forceinline__ float penalized(float l, int c, float r, float inv_r, float presence, float frequency) {
#pragma clang fp contract(off)
    if (c <= 0) return l;
    float b = l > 0.0f ? __fmul_rn(l, inv_r) : __fmul_rn(l, r);
    float f = __fmul_rn(frequency, (float)c);
    asm volatile("" : "+v"(b), "+v"(f));   // (the products are opaque from here on: the code generator fuses across the pragma once it vectorises)
    const float u = __fadd_rn(presence, f);
    return __fsub_rn(b, u);
}

// osg_decode_penalize: blockIdx.y = the sequence.  A thread takes one 16-byte group of the row from its first aligned element on, as sample_for_each
// lays a row out; the 0-3 elements before it and the 0-3 behind the last whole group go to the threads after the groups', one element each.  The counts
// and the output are read and written 16 bytes at a time where their own rows stand as the logits row does, else element by element.
__global__ __launch_bounds__(256) void decode_penalize_kernel(const float* __restrict__ rows, long row_stride, long V, const int* __restrict__ counts,
                                                              float* __restrict__ out, float r, float inv_r, float presence, float frequency) {
    const long s = blockIdx.y;
    const float* __restrict__ row = rows + s * row_stride;
    const int* __restrict__ cnt = counts + s * V;
    float* __restrict__ o = out + s * V;
    const int head = sample_head(row, V);
    const long nvec = (V - head) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g < nvec) {
        const long i = head + 4 * g;
        const float4 x = *(const float4*)(row + i);
        int c[4];
        if ((((uintptr_t)(cnt + i)) & 15) == 0) {
            const int4 cc = *(const int4*)(cnt + i);
            c[0] = cc.x; c[1] = cc.y; c[2] = cc.z; c[3] = cc.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = cnt[i + k];
        }
        float4 y;
        y.x = penalized(x.x, c[0], r, inv_r, presence, frequency);
        y.y = penalized(x.y, c[1], r, inv_r, presence, frequency);
        y.z = penalized(x.z, c[2], r, inv_r, presence, frequency);
        y.w = penalized(x.w, c[3], r, inv_r, presence, frequency);
        if ((((uintptr_t)(o + i)) & 15) == 0) *(float4*)(o + i) = y;
        else { o[i] = y.x; o[i + 1] = y.y; o[i + 2] = y.z; o[i + 3] = y.w; }
        return;
    }
    // the head [0, head), then the tail [head + 4 nvec, V): at most six elements in all
    long e = g - nvec;
    if (e >= head) e = head + 4 * nvec + (e - head);
    if (e < V) o[e] = penalized(row[e], cnt[e], r, inv_r, presence, frequency);
}

// min_p's x_min: the fp32 nearest to the double-precision log of min_p's fp32 value; 0 turns the step off
float min_p_x(float min_p) { return min_p > 0.0f ? (float)std::log((double)min_p) : -INFINITY; }

// top_p = pm * 2^-ps exactly, pm < 2^24 (the fp32 significand as an integer); pm = 0 says top-p is off
void split_top_p(float top_p, uint32_t& pm, int& ps) {
    pm = 0;
    ps = 0;
    if (top_p < 1.0f) {
        uint32_t u;
        std::memcpy(&u, &top_p, 4);
        const int e = (int)(u >> 23);
        pm = e ? ((u & 0x7fffffu) | 0x800000u) : (u & 0x7fffffu);
        ps = e ? 150 - e : 149;
    }
}

}  // namespace

extern "C" {

// the old entry points are the _ext ones with min_p = 0 and no count table: ONE launch path, ONE device body behind both
int osg_decode_pick(osg_ctx* ctx, const float* logits, long T, long V, long long eos_id, int* state, int64_t* input_ids, int64_t* position_ids,
                    int64_t* tokens, long max_tokens) {
    return osg_decode_pick_ext(ctx, logits, T, V, eos_id, state, input_ids, position_ids, tokens, max_tokens, nullptr);
}

int osg_decode_pick_ext(osg_ctx* ctx, const float* logits, long T, long V, long long eos_id, int* state, int64_t* input_ids, int64_t* position_ids,
                        int64_t* tokens, long max_tokens, int* counts) {
    if (T <= 0 || V <= 0) OSG_FAIL(ctx, "osg_decode_pick: invalid shape of the logits");
    if (!logits || !state || !input_ids || !position_ids || !tokens) OSG_FAIL(ctx, "osg_decode_pick: null operand");
    if (max_tokens < 0 || max_tokens > 0x7fffffffL) OSG_FAIL(ctx, "osg_decode_pick: invalid token budget");
    hipLaunchKernelGGL(decode_pick_kernel, dim3(1), dim3(kPickThreads), 0, ctx->compute, logits + (T - 1) * V, V, eos_id, state, input_ids, position_ids,
                       tokens, max_tokens, counts);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_decode_sample(osg_ctx* ctx, const float* logits, long T, long V, long long eos_id, int* state, int64_t* input_ids, int64_t* position_ids,
                      int64_t* tokens, long max_tokens, float temperature, long top_k, float top_p, unsigned long long seed, unsigned long long draw_base) {
    return osg_decode_sample_ext(ctx, logits, T, V, eos_id, state, input_ids, position_ids, tokens, max_tokens, temperature, top_k, top_p, seed, draw_base, 0.0f,
                                 nullptr);
}

int osg_decode_sample_ext(osg_ctx* ctx, const float* logits, long T, long V, long long eos_id, int* state, int64_t* input_ids, int64_t* position_ids,
                          int64_t* tokens, long max_tokens, float temperature, long top_k, float top_p, unsigned long long seed, unsigned long long draw_base,
                          float min_p, int* counts) {
    if (T <= 0 || V <= 0) OSG_FAIL(ctx, "osg_decode_sample: invalid shape of the logits");
    if (V > (1L << 20)) OSG_FAIL(ctx, "osg_decode_sample: more than 2^20 logits per row");
    if (!logits || !state || !input_ids || !position_ids || !tokens) OSG_FAIL(ctx, "osg_decode_sample: null operand");
    if (max_tokens < 0 || max_tokens > 0x7fffffffL) OSG_FAIL(ctx, "osg_decode_sample: invalid token budget");
    const float inv_t = 1.0f / temperature;
    if (!(temperature > 0.0f) || !(inv_t > 0.0f) || std::isinf(temperature) || std::isinf(inv_t))
        OSG_FAIL(ctx, "osg_decode_sample: temperature and 1 / temperature must be positive and finite");
    if (top_k < 0) OSG_FAIL(ctx, "osg_decode_sample: top_k must be >= 0");
    if (!(top_p > 0.0f) || !(top_p <= 1.0f)) OSG_FAIL(ctx, "osg_decode_sample: top_p must be in (0, 1]");
    if (!(min_p >= 0.0f) || !(min_p <= 1.0f)) OSG_FAIL(ctx, "osg_decode_sample: min_p must be in [0, 1]");
    uint32_t pm;
    int ps;
    split_top_p(top_p, pm, ps);
    hipLaunchKernelGGL(decode_sample_kernel, dim3(1), dim3(kSampleThreads), 0, ctx->compute, logits + (T - 1) * V, V, eos_id, state, input_ids, position_ids,
                       tokens, max_tokens, inv_t, top_k, pm, ps, seed, draw_base, min_p_x(min_p), counts);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_decode_sample_batch(osg_ctx* ctx, const float* logits, long V, int n_seq, long long eos_id, int* state, int64_t* input_ids, int64_t* position_ids,
                            int64_t* tokens, long max_tokens, float temperature, long top_k, float top_p, const unsigned long long* seeds,
                            unsigned long long draw_base) {
    return osg_decode_sample_batch_ext(ctx, logits, V, n_seq, eos_id, state, input_ids, position_ids, tokens, max_tokens, temperature, top_k, top_p, seeds,
                                       draw_base, 0.0f, nullptr);
}

int osg_decode_sample_batch_ext(osg_ctx* ctx, const float* logits, long V, int n_seq, long long eos_id, int* state, int64_t* input_ids,
                                int64_t* position_ids, int64_t* tokens, long max_tokens, float temperature, long top_k, float top_p,
                                const unsigned long long* seeds, unsigned long long draw_base, float min_p, int* counts) {
    if (V <= 0 || n_seq <= 0 || n_seq > 65535) OSG_FAIL(ctx, "osg_decode_sample_batch: invalid shape of the logits");
    if (V > (1L << 20)) OSG_FAIL(ctx, "osg_decode_sample_batch: more than 2^20 logits per row");
    if (!logits || !state || !input_ids || !position_ids || !tokens || !seeds) OSG_FAIL(ctx, "osg_decode_sample_batch: null operand");
    if (max_tokens < 0 || max_tokens > 0x7fffffffL) OSG_FAIL(ctx, "osg_decode_sample_batch: invalid token budget");
    const float inv_t = 1.0f / temperature;
    if (!(temperature > 0.0f) || !(inv_t > 0.0f) || std::isinf(temperature) || std::isinf(inv_t))
        OSG_FAIL(ctx, "osg_decode_sample_batch: temperature and 1 / temperature must be positive and finite");
    if (top_k < 0) OSG_FAIL(ctx, "osg_decode_sample_batch: top_k must be >= 0");
    if (!(top_p > 0.0f) || !(top_p <= 1.0f)) OSG_FAIL(ctx, "osg_decode_sample_batch: top_p must be in (0, 1]");
    if (!(min_p >= 0.0f) || !(min_p <= 1.0f)) OSG_FAIL(ctx, "osg_decode_sample_batch: min_p must be in [0, 1]");
    uint32_t pm;
    int ps;
    split_top_p(top_p, pm, ps);
    hipLaunchKernelGGL(decode_sample_batch_kernel, dim3((unsigned)n_seq), dim3(kSampleThreads), 0, ctx->compute, logits, V, eos_id, state, input_ids, position_ids,
                       tokens, max_tokens, inv_t, top_k, pm, ps, (const u64*)seeds, draw_base, min_p_x(min_p), counts);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_decode_count(osg_ctx* ctx, const int64_t* tokens, long n, int* counts, long V) {
    if (n < 0 || V <= 0) OSG_FAIL(ctx, "osg_decode_count: invalid number of tokens or of vocabulary entries");
    if (n == 0) return 0;
    if (!tokens || !counts) OSG_FAIL(ctx, "osg_decode_count: null operand");
    if ((n + 255) / 256 > 0x7fffffffL) OSG_FAIL(ctx, "osg_decode_count: too many tokens for one launch");
    hipLaunchKernelGGL(decode_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->compute, tokens, n, counts, V);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_decode_penalize(osg_ctx* ctx, const float* rows, long row_stride, long V, int n_seq, const int* counts, float* out, float r, float inv_r,
                        float presence, float frequency) {
    if (V <= 0 || n_seq <= 0 || n_seq > 65535 || row_stride < 0) OSG_FAIL(ctx, "osg_decode_penalize: invalid shape of the logits");
    if (!rows || !counts || !out) OSG_FAIL(ctx, "osg_decode_penalize: null operand");
    if ((((uintptr_t)rows) & 3) || (((uintptr_t)counts) & 3) || (((uintptr_t)out) & 3)) OSG_FAIL(ctx, "osg_decode_penalize: operands must be 4-byte aligned");
    const long threads = V / 4 + 6;      // at most V / 4 whole groups, three elements before them and three behind
    if ((threads + 255) / 256 > 0x7fffffffL) OSG_FAIL(ctx, "osg_decode_penalize: too many elements for one launch");
    hipLaunchKernelGGL(decode_penalize_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)n_seq), dim3(256), 0, ctx->compute, rows, row_stride, V, counts,
                       out, r, inv_r, presence, frequency);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_kv_append_at_batch(osg_ctx* ctx, const void* src, void* cache, const int* state, int batch, int kv_heads, long cap, int d) {
    if (batch <= 0 || batch > 65535 || kv_heads <= 0 || cap <= 0 || d <= 0) OSG_FAIL(ctx, "osg_kv_append_at_batch: invalid shape of the cache");
    if (!src || !cache || !state) OSG_FAIL(ctx, "osg_kv_append_at_batch: null operand");
    const long n = (long)kv_heads * d;
    hipLaunchKernelGGL(kv_append_at_batch_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, ctx->compute, (const uint16_t*)src,
                       (uint16_t*)cache, state, kv_heads, cap, d);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_kv_append_rows_at(osg_ctx* ctx, const void* src, void* cache, const int* base, int kv_heads, int C, long cap, int d) {
    if (kv_heads <= 0 || C <= 0 || cap <= 0 || d <= 0) OSG_FAIL(ctx, "osg_kv_append_rows_at: invalid shape of the cache");
    if (!src || !cache || !base) OSG_FAIL(ctx, "osg_kv_append_rows_at: null operand");
    const long n = (long)kv_heads * C * d;
    if ((n + 255) / 256 > 0x7fffffffL) OSG_FAIL(ctx, "osg_kv_append_rows_at: too many elements for one launch");
    hipLaunchKernelGGL(kv_append_rows_at_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->compute, (const uint16_t*)src, (uint16_t*)cache, base,
                       kv_heads, C, cap, d);
    OSG_LAUNCH_CHECK(ctx);
    return 0;
}

int osg_prefill_stage(osg_ctx* ctx, const int64_t* prompt, long n_prompt, long first, long pos0, int C, int64_t* input_ids, int64_t* position_ids, int* base) {
    if (n_prompt <= 0 || first < 0 || first >= n_prompt || C <= 0 || pos0 < 0 || pos0 + C > 0x7fffffffL) OSG_FAIL(ctx, "osg_prefill_stage: invalid chunk");
    if (!prompt || !input_ids || !position_ids || !base) OSG_FAIL(ctx, "osg_prefill_stage: null operand");
    const long left = n_prompt - first;
    hipLaunchKernelGGL(prefill_stage_kernel, dim3(1), dim3(256), 0, ctx->compute, prompt, first, left < C ? left : (long)C, pos0, C, input_ids, position_ids, base);
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
