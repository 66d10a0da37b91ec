// Sampled (t > 0) token draw on the device: one workgroup per row draws a token id from the
// row's float32 probs, as the logits kernels write them for want_probs rows ([row][2][V]: probs, logprobs), by
// inverting the row's CDF at a counter-based uniform word, and rewrites the row's TokOut record as
// process_step's host rules do.
//
// Uniform word: Philox4x32-10 (Random123), key = the state's 64-bit sample seed (lo, hi), counter =
// (0, seek, 16 * temp_idx + cand, token index); output word 0 = x0. u = (x0 + 0.5) * 2^-32 and target = u * S
// in double, S = the row's total; id = the smallest i with C_i > target (C_i the inclusive prefix in double, in
// ascending id), or the largest i with p_i > 0 if rounding leaves none. A row with S == 0 keeps its record.
//
// The row (207 KB) does not fit the LDS and is read twice from L2, coalesced. Pass 1: every wavefront sums
// 64-id chunks (chunk c = ids [64 c, 64 c + 64)) in double, one partial per chunk in LDS. Wavefront 0 then scans
// the partials (lane l owns kSamplePerLane consecutive chunks; the lanes' totals are chained in lane order),
// finds the first chunk whose inclusive prefix exceeds the target, loads that chunk again and walks it in
// ascending id from the chunk's exclusive prefix. No atomics: every value has one writer.
#include "../common.h"
#include "../kernels.h"

namespace wm {

static constexpr int ST = 1024;               // threads per row
static constexpr int SW = ST / 64;            // wavefronts
static constexpr int kSampleMaxChunks = 1024; // n_vocab <= 65536

__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                     uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0;
        const uint32_t h1 = __umulhi(M1, c2), l1 = M1 * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += W0; k1 += W1;
    }
    return c0;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double lane_bcast(double v, int lane) {  // `lane` wavefront-uniform
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// ctr[r] = {seek, 16 * temp_idx + cand, token index, source row}: row r draws from probs row `source` and
// starts from in[source]; out[r] receives the record (in == out is allowed when every source is its own row)
__global__ void __launch_bounds__(ST) sample_kernel(const float* __restrict__ probs, int V, const TokOut* in, TokOut* out,
                                                    const int4* __restrict__ ctr, const uint32_t* __restrict__ words,
                                                    uint32_t key_lo, uint32_t key_hi, int token_beg) {
    __shared__ double part[kSampleMaxChunks];
    __shared__ int wlast[SW];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int4 c = ctr[r];
    const float* row = probs + (long)c.w * 2 * V;
    const int nch = (V + 63) >> 6;

    // pass 1: chunk sums, and the largest id with p > 0
    int last = -1;
    for (int ch = wave; ch < nch; ch += SW) {
        const int i = ch * 64 + lane;
        const float p = i < V ? row[i] : 0.0f;
        if (p > 0.0f) last = i;
        const double sum = wave_sum((double)p);
        if (lane == 0) part[ch] = sum;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (lane == 0) wlast[wave] = last;
    __syncthreads();
    if (wave != 0) return;

    last = lane < SW ? wlast[lane] : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));

    // scan of the chunk sums: lane l owns chunks [l * per, l * per + per)
    const int per = (nch + 63) >> 6;
    const int c0 = lane * per;
    double mine = 0.0;
    for (int k = 0; k < per; k++)
        if (c0 + k < nch) mine += part[c0 + k];
    double run = 0.0, base = 0.0;
    for (int l = 0; l < 64; l++) {
        if (lane == l) base = run;
        run += lane_bcast(mine, l);
    }
    const double S = run;
    TokOut rec = in[c.w];
    if (!(S > 0.0) || last < 0) {  // nothing to draw from: the record as the logits kernel wrote it
        if (lane == 0) out[r] = rec;
        return;
    }
    const uint32_t x0 = words ? words[r] : philox4x32_10_x0(0u, (uint32_t)c.x, (uint32_t)c.y, (uint32_t)c.z, key_lo, key_hi);
    const double u = ((double)x0 + 0.5) * 0x1p-32;
    const double target = u * S;

    // the first chunk whose inclusive prefix exceeds the target, and its exclusive prefix
    int my_ch = nch;
    double my_start = 0.0, acc = base;
    for (int k = 0; k < per; k++) {
        if (c0 + k >= nch) break;
        const double nx = acc + part[c0 + k];
        if (my_ch == nch && nx > target) { my_ch = c0 + k; my_start = acc; }
        acc = nx;
    }
    const unsigned long long hit = __ballot(my_ch < nch);
    int id = -1;
    if (hit) {
        const int l = __ffsll((long long)hit) - 1;
        int ch = __builtin_amdgcn_readlane(my_ch, l);
        double cum = lane_bcast(my_start, l);
        // walk the chunk in ascending id (and, if its rounding differs from the chunk sum's, the chunks after it)
        for (; id < 0 && ch < nch; ch++) {
            const int i = ch * 64 + lane;
            const float p = i < V ? row[i] : 0.0f;
            const int pb = __float_as_int(p);
#pragma unroll
            for (int q = 0; q < 64; q++) {
                const float pq = __int_as_float(__builtin_amdgcn_readlane(pb, q));
                cum += (double)pq;
                if (id < 0 && pq > 0.0f && cum > target) id = ch * 64 + q;
            }
        }
    }
    if (id < 0) id = last;
    if (lane == 0) {
        rec.id = id;
        rec.p = row[id];
        rec.plog = row[V + id];
        if (id >= token_beg) { rec.tid = id; rec.pt = rec.p; }
        out[r] = rec;
    }
}

void launch_sample(const float* probs, int n_vocab, const TokOut* in, TokOut* out, const int* ctr, const uint32_t* words,
                   uint64_t seed, int token_beg, int n, hipStream_t st) {
    if (n <= 0) return;
    if (n > kSampleMaxRows) WM_FAIL("sample: %d rows in a launch (at most %d)", n, kSampleMaxRows);
    if (n_vocab < 1 || n_vocab > 64 * kSampleMaxChunks) WM_FAIL("sample: n_vocab %d outside [1, %d]", n_vocab, 64 * kSampleMaxChunks);
    sample_kernel<<<n, ST, 0, st>>>(probs, n_vocab, in, out, (const int4*)ctr, words, (uint32_t)seed, (uint32_t)(seed >> 32),
                                    token_beg);
    WM_CHECK(hipGetLastError());
}

}  // namespace wm
