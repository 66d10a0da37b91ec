// Token-level timestamps from cross-attention DTW (DESIGN.md "Token timestamps (DTW)"): the kernels of
// the alignment pass that runs after a window's segments are final.
//   1. align_scores_kernel: softmaxed q.k rows of the alignment heads of one decoder layer (MFMA; the
//      attention kernels are flash-style and never hold these weights);
//   2. align_stats_kernel + align_cost_kernel: per-(head, frame) z-score over the token rows, width-7
//      median along the frames, head mean, negation, row slice -> cost[N][F];
//   3. align_dtw_kernel: OpenAI's dtw_cpu as an anti-diagonal wavefront (one workgroup per clip, one
//      thread per row), byte trace in global memory, backtrace on one lane -> first frame of every row.
// Every clip of a launch is described by an AlignClip (kernels.h); all sums are f32.
#include <cmath>

#include "../kernels.h"

namespace wm {

// ---- 1. scores --------------------------------------------------------------------------------------
// One workgroup per (alignment head of this layer, clip): Q [n <= 256][64] stays in registers as MFMA A
// fragments (wave w owns the 16-row tiles w, w + 4, w + 8, w + 12), the head's K plane [ctx][64] is
// streamed ONCE through LDS in tiles of 64 keys. Sweep 1 writes the raw f32 scores of the frames t < F
// and keeps every row's running max and sum over the n_keys keys (f32, rescaled when the max moves; ctx is the
// plane's allocated rows, n_keys <= ctx those of the call's audio context); sweep 2
// normalises the stored scores in place: P = exp(s - m) / l. Each lane re-reads only what it wrote.
// Q and K both carry d_head^-0.25, so the product is q.k / 8.
constexpr int kAlKeys = 64;   // keys per LDS tile
constexpr int kAlKPad = 72;   // LDS row stride in elements (64 + 16 bytes: the 16 keys of a B fragment on distinct banks)

template <typename T>
__global__ __launch_bounds__(256) void align_scores_kernel(const T* __restrict__ q, int q_stride, const T* __restrict__ cross,
                                                           const AlignClip* __restrict__ clips, int L, int layer, int H, int ctx,
                                                           int n_keys, const int2* __restrict__ heads, float* __restrict__ P) {
    typedef typename Frag<T>::type F8;
    __shared__ __attribute__((aligned(16))) T Ks[kAlKeys * kAlKPad];
    const AlignClip cl = clips[blockIdx.y];
    const int h = heads[blockIdx.x].x, a = heads[blockIdx.x].y;
    const int n = cl.n_rows, F = cl.frames;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const T* K = cross + ((((size_t)cl.slot * L + layer) * 2) * H + h) * (size_t)ctx * 64;
    float* Pa = P + cl.p_off + (size_t)a * n * F;

    // this wave's row tiles and their Q fragments (rows >= n: zero)
    int nt = 0;
    F8 qf[4][2];
    float m[4][4], l[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r0 = (wave + 4 * i) * 16;
        if (r0 < n) nt = i + 1;
        const int row = r0 + lr;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            F8 v = {};
            if (row < n) v = *(const F8*)(q + (size_t)(cl.row0 + row) * q_stride + h * 64 + 32 * ks + 8 * lq);
            qf[i][ks] = v;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) { m[i][r] = -INFINITY; l[i][r] = 0.0f; }
    }

    const int n_kt = (n_keys + kAlKeys - 1) / kAlKeys;
    for (int kt = 0; kt < n_kt; kt++) {
        const int k0 = kt * kAlKeys;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int c = tid + 256 * u, key = c >> 3, part = c & 7;
            F8 v = {};
            if (k0 + key < n_keys) v = *(const F8*)(K + (size_t)(k0 + key) * 64 + part * 8);
            *(F8*)(Ks + key * kAlKPad + part * 8) = v;
        }
        __syncthreads();
        F8 bf[4][2];
#pragma unroll
        for (int ct = 0; ct < 4; ct++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++) bf[ct][ks] = *(const F8*)(Ks + (ct * 16 + lr) * kAlKPad + 32 * ks + 8 * lq);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i >= nt) continue;
            f32x4 acc[4];
#pragma unroll
            for (int ct = 0; ct < 4; ct++) {
                acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                acc[ct] = mfma16x16x32(qf[i][0], bf[ct][0], acc[ct]);
                acc[ct] = mfma16x16x32(qf[i][1], bf[ct][1], acc[ct]);
            }
            // accumulator element r of column tile ct: row r0 + 4 lq + r, key k0 + 16 ct + lr
            const int r0 = (wave + 4 * i) * 16 + 4 * lq;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float s[4], mx = -INFINITY;
#pragma unroll
                for (int ct = 0; ct < 4; ct++) {
                    const int key = k0 + 16 * ct + lr;
                    s[ct] = key < n_keys ? acc[ct][r] : -INFINITY;
                    mx = fmaxf(mx, s[ct]);
                    if (r0 + r < n && key < F) Pa[(size_t)(r0 + r) * F + key] = s[ct];
                }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
                const float mn = fmaxf(m[i][r], mx);  // finite: every tile holds a key < n_keys
                float sum = 0.0f;
#pragma unroll
                for (int ct = 0; ct < 4; ct++) sum += expf(s[ct] - mn);
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o);
                l[i][r] = l[i][r] * expf(m[i][r] - mn) + sum;
                m[i][r] = mn;
            }
        }
    }
    // sweep 2: normalise the stored scores (each lane the elements it stored)
    const int f_kt = (F + kAlKeys - 1) / kAlKeys;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i >= nt) continue;
        const int r0 = (wave + 4 * i) * 16 + 4 * lq;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (r0 + r >= n) continue;
            const float mr = m[i][r], inv = 1.0f / l[i][r];
            float* row = Pa + (size_t)(r0 + r) * F;
            for (int kt = 0; kt < f_kt; kt++)
#pragma unroll
                for (int ct = 0; ct < 4; ct++) {
                    const int key = kt * kAlKeys + 16 * ct + lr;
                    if (key < F) row[key] = expf(row[key] - mr) * inv;
                }
        }
    }
}

void launch_align_scores(DType dt, const void* q, int q_stride, const void* cross, const AlignClip* clips, int n_clips,
                         int max_rows, int L, int layer, int H, int ctx, int n_keys, const int2* heads, int n_heads,
                         float* P, hipStream_t st) {
    if (n_clips <= 0 || n_heads <= 0) return;
    if (n_keys < 1 || n_keys > ctx) WM_FAIL("align scores: %d keys of a %d-row cache plane", n_keys, ctx);
    if (max_rows > 256) WM_FAIL("align scores: %d token rows per clip (at most 256)", max_rows);
    const dim3 grid(n_heads, n_clips);
    if (dt == DType::F16)
        align_scores_kernel<half_t><<<grid, 256, 0, st>>>((const half_t*)q, q_stride, (const half_t*)cross, clips, L, layer, H,
                                                         ctx, n_keys, heads, P);
    else
        align_scores_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)q, q_stride, (const bf16_t*)cross, clips, L, layer, H,
                                                         ctx, n_keys, heads, P);
    WM_CHECK(hipGetLastError());
}

// ---- 2. cost ----------------------------------------------------------------------------------------
// stats[a][t] = {mean, 1 / sqrt(population variance + 1e-9)} of P[a][.][t] over the clip's n token rows:
// 64 frames x 4 row groups per workgroup, two sweeps (mean, then squared deviations from it)
__global__ __launch_bounds__(256) void align_stats_kernel(const float* __restrict__ P, const AlignClip* __restrict__ clips,
                                                          float* __restrict__ stats) {
    __shared__ float red[4][64];
    const AlignClip cl = clips[blockIdx.z];
    const int n = cl.n_rows, F = cl.frames, a = blockIdx.y;
    if ((int)blockIdx.x * 64 >= F) return;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, t = blockIdx.x * 64 + tx;
    const float* Pa = P + cl.p_off + (size_t)a * n * F;
    float s = 0.0f;
    if (t < F)
        for (int i = ty; i < n; i += 4) s += Pa[(size_t)i * F + t];
    red[ty][tx] = s;
    __syncthreads();
    const float mean = ((red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx])) / (float)n;
    __syncthreads();
    float v = 0.0f;
    if (t < F)
        for (int i = ty; i < n; i += 4) {
            const float dv = Pa[(size_t)i * F + t] - mean;
            v += dv * dv;
        }
    red[ty][tx] = v;
    __syncthreads();
    if (ty == 0 && t < F) {
        const float var = ((red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx])) / (float)n;
        float* o = stats + cl.st_off + ((size_t)a * F + t) * 2;
        o[0] = mean;
        o[1] = 1.0f / sqrtf(var + 1e-9f);
    }
}

__device__ __forceinline__ void al_cswap(float& x, float& y) {
    const float lo = fminf(x, y), hi = fmaxf(x, y);
    x = lo;
    y = hi;
}

// cost[r][t] = -mean_a median7_k Z[a][n_sot + r][refl(t + k)], Z = (P - mean) * rstd; refl reflects without
// repeating the edge and is then clamped to [0, F - 1] (F < 4)
__global__ __launch_bounds__(256) void align_cost_kernel(const float* __restrict__ P, const AlignClip* __restrict__ clips, int A,
                                                         const float* __restrict__ stats, float* __restrict__ cost) {
    const AlignClip cl = clips[blockIdx.z];
    const int n = cl.n_rows, F = cl.frames, N = n - cl.n_sot - 1;
    const int r = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (r >= N || t >= F) return;
    const int i = cl.n_sot + r;
    int tt[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        int x = t + k - 3;
        if (x < 0) x = -x;
        if (x >= F) x = 2 * (F - 1) - x;
        tt[k] = min(max(x, 0), F - 1);
    }
    float acc = 0.0f;
    for (int a = 0; a < A; a++) {
        const float* Pr = P + cl.p_off + ((size_t)a * n + i) * F;
        const float* sa = stats + cl.st_off + (size_t)a * F * 2;
        float z[7];
#pragma unroll
        for (int k = 0; k < 7; k++) z[k] = (Pr[tt[k]] - sa[2 * tt[k]]) * sa[2 * tt[k] + 1];
        // odd-even transposition sort, 7 rounds
#pragma unroll
        for (int round = 0; round < 7; round++)
#pragma unroll
            for (int k = round & 1; k + 1 < 7; k += 2) al_cswap(z[k], z[k + 1]);
        acc += z[3];
    }
    cost[cl.cost_off + (size_t)r * F + t] = -(acc / (float)A);
}

void launch_align_cost(const float* P, const AlignClip* clips, int n_clips, int A, int max_rows, int max_frames, float* stats,
                       float* cost, hipStream_t st) {
    if (n_clips <= 0 || A <= 0 || max_rows <= 0 || max_frames <= 0) return;
    align_stats_kernel<<<dim3(cdiv(max_frames, 64), A, n_clips), 256, 0, st>>>(P, clips, stats);
    WM_CHECK(hipGetLastError());
    align_cost_kernel<<<dim3(cdiv(max_frames, 256), max_rows, n_clips), 256, 0, st>>>(P, clips, A, stats, cost);
    WM_CHECK(hipGetLastError());
}

// ---- 3. DTW -----------------------------------------------------------------------------------------
// C[i][j] = cost[i-1][j-1] + min(C[i-1][j-1], C[i-1][j], C[i][j-1]), C[0][0] = 0, the rest of row 0 and
// column 0 +inf. Thread i - 1 owns row i and walks it one cell per step: at step s it computes the cell of
// anti-diagonal s (j = s - i + 1). Its left neighbour is its own last value, the upper one row i - 1's value
// of step s - 1 (through LDS, double buffered, one barrier per step), the diagonal one the upper value it
// read a step earlier. Every cell is one f32 add of the same operands as in the sequential loop, so the
// result is that loop's, bit for bit. N <= 256.
__global__ __launch_bounds__(256) void align_dtw_kernel(const float* __restrict__ cost, const AlignClip* __restrict__ clips,
                                                        unsigned char* __restrict__ trace, int* __restrict__ fr,
                                                        int* __restrict__ path, int* __restrict__ path_len) {
    __shared__ float rowv[2][260];
    const AlignClip cl = clips[blockIdx.x];
    const int N = cl.n_rows - cl.n_sot - 1, F = cl.frames;
    const float* C = cost + cl.cost_off;
    unsigned char* tr = trace + cl.tr_off;
    const int i = threadIdx.x + 1;
    const bool active = i <= N;
    float left = INFINITY, diag = i == 1 ? 0.0f : INFINITY;
    float cnext = active ? C[(size_t)(i - 1) * F] : 0.0f;
    const int n_steps = N + F - 1;
    for (int s = 1; s <= n_steps; s++) {
        const int j = s - i + 1;
        if (active && j >= 1 && j <= F) {
            const float cc = cnext;
            if (j < F) cnext = C[(size_t)(i - 1) * F + j];  // the next step's cost, a step early
            const float up = i == 1 ? INFINITY : rowv[(s - 1) & 1][i - 1];
            const float c0 = diag, c1 = up, c2 = left;
            const unsigned char t = (c0 < c1 && c0 < c2) ? 0 : (c1 < c0 && c1 < c2) ? 1 : 2;
            const float v = cc + fminf(c0, fminf(c1, c2));
            tr[(size_t)(i - 1) * F + (j - 1)] = t;
            diag = up;
            left = v;
            rowv[s & 1][i] = v;
        }
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    // backtrace from (N, F); the trace of row 0 is 2 and of column 0 is 1. The last point seen in a row
    // (the walk goes backwards) is the row's first frame.
    int* f = fr + cl.fr_off;
    int* pp = path ? path + 2 * cl.path_off : nullptr;
    int bi = N, bj = F, k = 0;
    while ((bi > 0 || bj > 0) && k < N + F) {  // (a path has at most N + F - 1 points: the pairs reserved)
        if (bi > 0 && bj > 0) f[bi - 1] = bj - 1;
        if (pp) { pp[2 * k] = bi - 1; pp[2 * k + 1] = bj - 1; }
        k++;
        const int t = bi == 0 ? 2 : bj == 0 ? 1 : tr[(size_t)(bi - 1) * F + (bj - 1)];
        if (t == 0) { bi--; bj--; }
        else if (t == 1) bi--;
        else bj--;
    }
    if (path_len) path_len[blockIdx.x] = k;
}

void launch_align_dtw(const float* cost, const AlignClip* clips, int n_clips, int max_n, unsigned char* trace, int* fr,
                      int* path, int* path_len, hipStream_t st) {
    if (n_clips <= 0) return;
    if (max_n > 256) WM_FAIL("align dtw: %d rows per clip (at most 256)", max_n);
    align_dtw_kernel<<<n_clips, 256, 0, st>>>(cost, clips, trace, fr, path, path_len);
    WM_CHECK(hipGetLastError());
}

}  // namespace wm
