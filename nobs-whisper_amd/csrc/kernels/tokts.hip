// Token times (whisper_full_params.token_timestamps): the two device passes.
//
// signal_energy_kernel: e[i] = (sum_{j = -32..32, 0 <= i + j < n} |x[i + j]|) / 65.0f for every sample of every clip,
// bit for bit the sequential host loop: the f32 sum starts at 0.0f and adds in ascending j, the divide is the
// correctly rounded one (this file is built with -ffp-contract=off). A workgroup owns a tile of kEnergyTile samples
// of one clip; |x| of the tile and a 32-sample halo on each side goes to LDS (samples outside the clip as +0.0f:
// the sum is never negative, so adding +0.0f leaves its bits), then every thread adds the 65 values of each of its
// outputs in that order.
//
// token_vad_kernel: the voice-activity adjust of the token times of one segment per workgroup, tokens in order
// (token j reads token j - 1's adjusted t1 and token j + 1's unadjusted t0). Per text token: the threshold is half
// the mean energy of the window around it, summed in f64 (per-thread partials, then a fixed reduction tree), and each
// of the two walks along the signal is a chunked search: kVadChunk samples per round, one per thread, the first
// lane at which the walk would stop found by ballot, and the rounds end there. Every value that steers the control
// flow comes from LDS or from values all threads hold alike, so the workgroup stays convergent; a walk of a clip of N
// samples takes at most N / kVadChunk + 2 rounds. No atomics, no waits on other workgroups.
#include <climits>

#include "../common.h"
#include "../kernels.h"

namespace wm {

static constexpr int ET = 256;                    // threads of an energy workgroup
static constexpr int EPT = kEnergyTile / ET;      // outputs per thread
static constexpr int EH = 32;                     // halo on each side

__global__ void __launch_bounds__(ET) signal_energy_kernel(const TtClip* __restrict__ clips, float* __restrict__ energy) {
    __shared__ float tile[kEnergyTile + 2 * EH];
    const TtClip cl = clips[blockIdx.y];
    const long base = (long)blockIdx.x * kEnergyTile;
    const int n = cl.n;
    if (base >= n) return;  // (uniform: the grid is sized by the longest clip)
    const int tid = threadIdx.x;
    for (int i = tid; i < kEnergyTile + 2 * EH; i += ET) {
        const long g = base - EH + i;
        tile[i] = (g >= 0 && g < n) ? fabsf(cl.pcm[g]) : 0.0f;
    }
    __syncthreads();
    float* e = energy + cl.e_off;
#pragma unroll
    for (int q = 0; q < EPT; q++) {
        const int i = tid + ET * q;
        const long g = base + i;
        if (g >= n) continue;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 2 * EH + 1; j++) s = __fadd_rn(s, tile[i + j]);
        e[g] = __fdiv_rn(s, 65.0f);
    }
}

void launch_signal_energy(const TtClip* clips, int n_clips, int max_n, float* energy, hipStream_t st) {
    if (n_clips <= 0 || max_n <= 0) return;
    if (n_clips > 65535) WM_FAIL("signal energy: %d clips in one launch", n_clips);
    dim3 grid(cdiv(max_n, kEnergyTile), n_clips);
    hipLaunchKernelGGL(signal_energy_kernel, grid, dim3(ET), 0, st, clips, energy);
    WM_CHECK(hipGetLastError());
}

// ---- voice-activity adjust --------------------------------------------------------------------------------------
static constexpr int VT = kVadChunk;  // threads = samples per round of a walk
static constexpr int VW = VT / 64;
static constexpr int kVadHw = 2000;   // half window of the threshold, samples
static_assert(VT == 256, "the reductions below take 4 wavefronts");

__device__ __forceinline__ int tt_to_sample(long long t, int N) {
    long long k = (t * 16000) / 100;
    k = k < N - 1 ? k : N - 1;
    return (int)(k > 0 ? k : 0);
}
__device__ __forceinline__ long long tt_to_ts(int k) { return (100 * (long long)k) / 16000; }

__device__ __forceinline__ double tt_block_sum(double v, double* shd) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (shd[0] + shd[1]) + (shd[2] + shd[3]);
    __syncthreads();
    return r;
}

// Where the walk  `while (k is before bound && cmp(e[k], thold)) k += dir`  from k0 stops. dir = +1: k is before
// bound while k < bound; dir = -1: while k > bound. GT: cmp is e > thold, else e < thold. k0 and bound lie in
// [0, N - 1], so every sample read does. All arguments are the same in every thread; so is the result.
template <bool GT>
__device__ int tt_walk(const float* __restrict__ e, int k0, int dir, int bound, float thold, int max_rounds, int* shi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int r = 0; r < max_rounds; r++) {
        const long long step = (long long)r * VT + tid;
        const long long k = k0 + dir * step;
        bool stop = dir > 0 ? k >= bound : k <= bound;
        if (!stop) {
            const float v = e[k];
            stop = GT ? !(v > thold) : !(v < thold);
        }
        const unsigned long long b = __ballot(stop);
        if (lane == 0) shi[wave] = b ? wave * 64 + (__ffsll((long long)b) - 1) : INT_MAX;
        __syncthreads();
        const int m = min(min(shi[0], shi[1]), min(shi[2], shi[3]));
        __syncthreads();
        if (m != INT_MAX) return (int)(k0 + dir * ((long long)r * VT + m));
    }
    return bound;  // not reached: the walk is at its bound after at most N steps
}

__global__ void __launch_bounds__(VT) token_vad_kernel(const float* __restrict__ energy, const TtClip* __restrict__ clips,
                                                       const TtSeg* __restrict__ segs, TtSpan* spans) {
    __shared__ double shd[VW];
    __shared__ int shi[VW];
    const TtSeg sg = segs[blockIdx.x];
    const TtClip cl = clips[sg.clip];
    const int N = cl.n, n = sg.n_tok;
    if (N < 1 || n < 2) return;
    const float* e = energy + cl.e_off;
    TtSpan* tok = spans + sg.tok0;
    const int tid = threadIdx.x;
    const int max_rounds = N / VT + 2;
    long long prev_t1 = 0;
    for (int j = 0; j < n; j++) {
        const TtSpan cur = tok[j];
        if (!cur.is_text) {
            prev_t1 = cur.t1;
            continue;
        }
        const long long next_t0 = j < n - 1 ? tok[j + 1].t0 : 0;
        long long t0 = cur.t0, t1 = cur.t1;
        int s0 = tt_to_sample(t0, N), s1 = tt_to_sample(t1, N);
        const int ss0 = max(s0 - kVadHw, 0), ss1 = min(s1 + kVadHw, N), ns = ss1 - ss0;
        double part = 0.0;
        for (int k = ss0 + tid; k < ss1; k += VT) part += (double)e[k];
        const double S = tt_block_sum(part, shd);
        const float thold = (float)(0.5 * S / (double)ns);
        // start
        if (e[s0] > thold && j > 0) {
            const int k = tt_walk<true>(e, s0, -1, 0, thold, max_rounds, shi);
            t0 = tt_to_ts(k);
            if (t0 < prev_t1) t0 = prev_t1;
            else s0 = k;
        } else {
            const int k = tt_walk<false>(e, s0, +1, s1, thold, max_rounds, shi);
            s0 = k;
            t0 = tt_to_ts(k);
        }
        // end
        if (e[s1] > thold) {
            const int k = tt_walk<true>(e, s1, +1, N - 1, thold, max_rounds, shi);
            t1 = tt_to_ts(k);
            if (j < n - 1 && t1 > next_t0) t1 = next_t0;
            else s1 = k;
        } else {
            const int k = tt_walk<false>(e, s1, -1, s0, thold, max_rounds, shi);
            s1 = k;
            t1 = tt_to_ts(k);
        }
        if (tid == 0) {
            tok[j].t0 = t0;
            tok[j].t1 = t1;
        }
        prev_t1 = t1;
    }
}

void launch_token_vad(const float* energy, const TtClip* clips, const TtSeg* segs, int n_segs, TtSpan* spans, hipStream_t st) {
    if (n_segs <= 0) return;
    hipLaunchKernelGGL(token_vad_kernel, dim3(n_segs), dim3(VT), 0, st, energy, clips, segs, spans);
    WM_CHECK(hipGetLastError());
}

}  // namespace wm
