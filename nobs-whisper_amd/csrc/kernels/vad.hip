// Silero-VAD v5 (16 kHz) on gfx950: vad_frontend, vad_lstm, vad_gather (vad.h). f32 throughout, accurate
// expf / tanhf / sqrtf. tests/vad_ref.py is the reference; nothing here is pinned bit-exact.
#include <algorithm>

#include "../common.h"
#include "../vad.h"

namespace wm {

// ---- vad_frontend -------------------------------------------------------------------------------------------------
// Every layer up to the LSTM input is a product of a k-major weight matrix [K][OUT] with input vectors that lie
// contiguous in LDS: an STFT frame is 256 consecutive samples of the padded window, and a k = 3 conv's input at output
// position p is the three consecutive frames p * stride .. + 2 of a [frame][channel] image with a zero frame at both
// ends (k = tap * C + channel). A task is (group of NP positions, output o): consecutive threads take consecutive o, so
// a wave's weight loads are coalesced (from L2: the 1.2 MB of weights stay resident, and a weight is loaded by the
// tile's position groups only, so a copy through LDS would add traffic, not save it) and its LDS reads are broadcasts.
template <int NP, typename Store>
__device__ __forceinline__ void vad_dense(const float* __restrict__ wt, int OUT, int K, int n_pos, int P, const float* in, int in_ws,
                                          int in_ps, Store store) {
    const int G = n_pos / NP;
    for (int task = threadIdx.x; task < OUT * G; task += blockDim.x) {
        const int g = task / OUT, o = task - g * OUT;
        const float* x[NP];
        float acc[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int q = g * NP + i;
            x[i] = in + (q / P) * in_ws + (q % P) * in_ps;
            acc[i] = 0.0f;
        }
        const float* wp = wt + o;
        for (int k = 0; k < K; k += 4) {
            const float w0 = wp[(size_t)k * OUT], w1 = wp[(size_t)(k + 1) * OUT], w2 = wp[(size_t)(k + 2) * OUT], w3 = wp[(size_t)(k + 3) * OUT];
#pragma unroll
            for (int i = 0; i < NP; i++) {
                const float4 v = *(const float4*)(x[i] + k);
                acc[i] = fmaf(v.x, w0, acc[i]);
                acc[i] = fmaf(v.y, w1, acc[i]);
                acc[i] = fmaf(v.z, w2, acc[i]);
                acc[i] = fmaf(v.w, w3, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < NP; i++) store(g * NP + i, o, acc[i]);
    }
}

constexpr int TW = kVadTile;
constexpr int kSpecPad = 260;  // 258 rows of the basis, padded
constexpr int kPadded = kVadWindow + 2 * kVadPad;  // samples of a reflect-padded window (640)
constexpr int kF0 = kVadFrames + 2;                // frames of the STFT / layer-0 images with their zero frames (6)

__global__ __launch_bounds__(512) void vad_frontend_kernel(VadWeights W, const VadClip* __restrict__ clips, float* __restrict__ xg) {
    const VadClip cl = clips[blockIdx.y];
    const int w0 = blockIdx.x * TW;
    if (w0 >= cl.n_win) return;  // (uniform for the workgroup)
    const int nw = min(TW, cl.n_win - w0);
    const int tid = threadIdx.x;
    __shared__ __align__(16) float s_audio[TW][kPadded];
    __shared__ __align__(16) float s_spec[TW * kVadFrames][kSpecPad];
    __shared__ __align__(16) float s_a0[TW][kF0][kVadC0Pad];  // magnitudes
    __shared__ __align__(16) float s_a1[TW][kF0][128];
    __shared__ __align__(16) float s_a2[TW][2 + 2][64];
    __shared__ __align__(16) float s_a3[TW][1 + 2][64];
    __shared__ __align__(16) float s_a4[TW][128];

    // the windows of the tile, each reflect-padded by 64 within its own 512 samples (zeros beyond the clip)
    for (int idx = tid; idx < TW * kPadded; idx += blockDim.x) {
        const int w = idx / kPadded, i = idx - w * kPadded;
        int j = i - kVadPad;
        if (j < 0) j = -j;
        if (j >= kVadWindow) j = 2 * (kVadWindow - 1) - j;
        const long long g = (long long)(w0 + w) * kVadWindow + j;
        s_audio[w][i] = (w < nw && g < cl.n_samples) ? cl.pcm[g] : 0.0f;
    }
    // the zero frames and channels of the conv inputs
    for (int idx = tid; idx < TW * kF0 * kVadC0Pad; idx += blockDim.x) (&s_a0[0][0][0])[idx] = 0.0f;
    for (int idx = tid; idx < TW * kF0 * 128; idx += blockDim.x) (&s_a1[0][0][0])[idx] = 0.0f;
    for (int idx = tid; idx < TW * 4 * 64; idx += blockDim.x) (&s_a2[0][0][0])[idx] = 0.0f;
    for (int idx = tid; idx < TW * 3 * 64; idx += blockDim.x) (&s_a3[0][0][0])[idx] = 0.0f;
    __syncthreads();

    // STFT: 258 basis rows x (4 frames of 256 samples at hop 128) per window
    vad_dense<4>(W.basis_t, 2 * kVadBins, kVadFft, TW * kVadFrames, kVadFrames, &s_audio[0][0], kPadded, kVadHop,
                 [&](int q, int o, float v) { s_spec[q][o] = v; });
    __syncthreads();
    for (int idx = tid; idx < TW * kVadFrames * kVadBins; idx += blockDim.x) {
        const int q = idx / kVadBins, b = idx - q * kVadBins;
        const float re = s_spec[q][b], im = s_spec[q][kVadBins + b];
        s_a0[q / kVadFrames][q % kVadFrames + 1][b] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    // four conv1d (k = 3, pad 1, strides 1, 2, 2, 1) + ReLU: 4 -> 4 -> 2 -> 1 -> 1 frames
    vad_dense<4>(W.conv_t[0], 128, 3 * kVadC0Pad, TW * kVadFrames, kVadFrames, &s_a0[0][0][0], kF0 * kVadC0Pad, kVadC0Pad,
                 [&](int q, int o, float v) { s_a1[q / kVadFrames][q % kVadFrames + 1][o] = fmaxf(v + W.conv_b[0][o], 0.0f); });
    __syncthreads();
    vad_dense<1>(W.conv_t[1], 64, 3 * 128, TW * 2, 2, &s_a1[0][0][0], kF0 * 128, 2 * 128,
                 [&](int q, int o, float v) { s_a2[q / 2][q % 2 + 1][o] = fmaxf(v + W.conv_b[1][o], 0.0f); });
    __syncthreads();
    vad_dense<1>(W.conv_t[2], 64, 3 * 64, TW, 1, &s_a2[0][0][0], 4 * 64, 2 * 64,
                 [&](int q, int o, float v) { s_a3[q][1][o] = fmaxf(v + W.conv_b[2][o], 0.0f); });
    __syncthreads();
    vad_dense<1>(W.conv_t[3], 128, 3 * 64, TW, 1, &s_a3[0][0][0], 3 * 64, 64,
                 [&](int q, int o, float v) { s_a4[q][o] = fmaxf(v + W.conv_b[3][o], 0.0f); });
    __syncthreads();
    // the input half of the LSTM gates
    float* out = xg + (cl.win0 + w0) * (long long)(4 * kVadHidden);
    vad_dense<TW>(W.wih_t, 4 * kVadHidden, kVadHidden, TW, TW, &s_a4[0][0], TW * 128, 128, [&](int q, int o, float v) {
        if (q < nw) out[(size_t)q * (4 * kVadHidden) + o] = v + W.b_ih[o] + W.b_hh[o];
    });
}

void launch_vad_frontend(const VadWeights& w, const VadClip* clips, int n_clips, int max_win, float* xg, hipStream_t st) {
    if (n_clips <= 0 || max_win <= 0) return;
    hipLaunchKernelGGL(vad_frontend_kernel, dim3(cdiv(max_win, TW), n_clips), dim3(512), 0, st, w, clips, xg);
    WM_CHECK(hipGetLastError());
}

// ---- vad_lstm -----------------------------------------------------------------------------------------------------
// One workgroup of 512 threads per clip; a clip's chain never leaves it. Thread g keeps row g of W_hh in 128 registers
// for the whole clip (8 waves = 2 per SIMD: 256 VGPRs each); h lives in LDS and is read as broadcast 16-byte reads;
// xg[t + 1] is loaded while step t computes. Per step: 128 FMAs per thread (four partial sums), the gate
// pre-activations to LDS, a barrier, 128 threads update c and h and store h_t, a barrier. The head (ReLU, dot, sigmoid)
// then runs over the stored h_t, a window per thread.
__device__ __forceinline__ float vad_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(512) void vad_lstm_kernel(VadWeights W, const VadClip* __restrict__ clips, const float* __restrict__ xg,
                                                       float* __restrict__ hbuf, float* __restrict__ probs) {
    const VadClip cl = clips[blockIdx.x];
    if (cl.n_win <= 0) return;
    const int g = threadIdx.x;
    __shared__ __align__(16) float s_h[kVadHidden];
    __shared__ float s_gate[4 * kVadHidden];
    float w[kVadHidden];
    {
        const float4* wr = (const float4*)(W.whh + (size_t)g * kVadHidden);
#pragma unroll
        for (int k = 0; k < kVadHidden / 4; k++) {
            const float4 v = wr[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    }
    const float* x = xg + cl.win0 * (long long)(4 * kVadHidden);
    float* ho = hbuf + cl.win0 * (long long)kVadHidden;
    float c = 0.0f;
    if (g < kVadHidden) s_h[g] = 0.0f;
    float xn = x[g];
    __syncthreads();
    for (int t = 0; t < cl.n_win; t++) {
        const float xt = xn;
        if (t + 1 < cl.n_win) xn = x[(size_t)(t + 1) * (4 * kVadHidden) + g];
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
        for (int k = 0; k < kVadHidden / 4; k++) {
            const float4 hv = *(const float4*)&s_h[4 * k];
            a0 = fmaf(w[4 * k], hv.x, a0);
            a1 = fmaf(w[4 * k + 1], hv.y, a1);
            a2 = fmaf(w[4 * k + 2], hv.z, a2);
            a3 = fmaf(w[4 * k + 3], hv.w, a3);
        }
        s_gate[g] = xt + ((a0 + a1) + (a2 + a3));
        __syncthreads();
        if (g < kVadHidden) {
            const float gi = vad_sigmoid(s_gate[g]), gf = vad_sigmoid(s_gate[kVadHidden + g]);
            const float gg = tanhf(s_gate[2 * kVadHidden + g]), go = vad_sigmoid(s_gate[3 * kVadHidden + g]);
            c = gf * c + gi * gg;
            const float h = go * tanhf(c);
            s_h[g] = h;
            ho[(size_t)t * kVadHidden + g] = h;
        }
        __syncthreads();
    }
    // the head: p_t = sigmoid(w . ReLU(h_t) + b) (the stores of h above are visible to the workgroup after the barrier)
    if (g < kVadHidden) s_gate[g] = W.head_w[g];
    __syncthreads();
    for (int t = g; t < cl.n_win; t += blockDim.x) {
        const float4* hr = (const float4*)(ho + (size_t)t * kVadHidden);
        float acc = 0.0f;
        for (int k = 0; k < kVadHidden / 4; k++) {
            const float4 v = hr[k];
            acc = fmaf(s_gate[4 * k], fmaxf(v.x, 0.0f), acc);
            acc = fmaf(s_gate[4 * k + 1], fmaxf(v.y, 0.0f), acc);
            acc = fmaf(s_gate[4 * k + 2], fmaxf(v.z, 0.0f), acc);
            acc = fmaf(s_gate[4 * k + 3], fmaxf(v.w, 0.0f), acc);
        }
        probs[cl.win0 + t] = vad_sigmoid(acc + W.head_b);
    }
}

void launch_vad_lstm(const VadWeights& w, const VadClip* clips, int n_clips, const float* xg, float* h, float* probs, hipStream_t st) {
    if (n_clips <= 0) return;
    hipLaunchKernelGGL(vad_lstm_kernel, dim3(n_clips), dim3(512), 0, st, w, clips, xg, h, probs);
    WM_CHECK(hipGetLastError());
}

// ---- vad_gather ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vad_gather_kernel(const VadGatherClip* __restrict__ clips, const VadPiece* __restrict__ pieces) {
    const VadGatherClip cl = clips[blockIdx.y];
    const VadPiece* pc = pieces + cl.piece0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cl.out_len; i += gridDim.x * 256) {
        int lo = 0, hi = cl.n_pieces - 1;  // the last piece that starts at or before i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pc[mid].vad_start <= i) lo = mid;
            else hi = mid - 1;
        }
        const VadPiece q = pc[lo];
        cl.dst[i] = (i >= q.vad_start && i < q.vad_end) ? cl.src[q.orig_start + (i - q.vad_start)] : 0.0f;
    }
}

void launch_vad_gather(const VadGatherClip* clips, const VadPiece* pieces, int n_clips, int max_out, hipStream_t st) {
    if (n_clips <= 0 || max_out <= 0) return;
    hipLaunchKernelGGL(vad_gather_kernel, dim3(std::min(cdiv(max_out, 256), 4096), n_clips), dim3(256), 0, st, clips, pieces);
    WM_CHECK(hipGetLastError());
}

}  // namespace wm
