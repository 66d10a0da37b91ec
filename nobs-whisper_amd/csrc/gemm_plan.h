// Which kernel, which tile, which split and which reduce a GEMM call gets (kernels/gemm.hip launch_gemm and
// launch_gemm_partials): one pure function of the shape and the tuning knobs, free of HIP, so
// tools/gemm_plan_check.cpp builds with a plain C++ compiler and the engine can ask what a shape will run
// (engine.cpp step_variant). The launchers only follow the plan. The table shape -> kernel: kernels/gemm.hip's header.
#pragma once

namespace wm {

enum Epi : int {
    EPI_STORE = 0,     // T out[orow][n] = (v) * colscale(n)
    EPI_GELU = 1,      // T out = gelu_ggml(v)   (ggml's f16 GELU table)
    EPI_RESID = 2,     // f32 out[orow][n] = v + out[orow][n]            (residual stream, in place)
    EPI_GELU_POS = 3,  // f32 out = gelu_ggml(v) + pos[m % pos_rows][n]   (conv2 + positional emb)
    EPI_F32 = 4,       // f32 out = v                                       (logits)
    EPI_CROSSKV = 5,   // T scatter into cross cache [slot][L][2][H][ctx][64]; K columns scaled; row m = (window m / rpw, t = m % rpw)
    EPI_QKV_DEC = 6,   // n<d: T q[m][n]*scale ; d<=n<2d: K cache (scaled) ; 2d<=n<3d: V cache
    EPI_GELU_F = 7,    // T out = tanh-GELU by formula in f32 (fp8 mode, and bf16 encoders: not ggml's f16 table)
};

// The process-wide debug / tuning inputs of the plan (gemm.hip current_knobs()):
//   variant     -1 auto, 0 register-staged, 1 LDS-DMA 128^2 in place of 256^2, >= 2 the 256^2 phase-interleaved
//               kernel (the auto choice for big GEMMs) wherever the shape is big
//   dec_splits  override of the decode-step split count (0 = heuristic)
//   dec_bm_min  gemm_dec_kernel's row tile is capped from below by this (32: the smallest tile that holds the step)
//   group_m_env gemm8p_kernel's tile grouping when >= 0 (-1: by the shape)
struct GemmKnobs { int variant = -1, dec_splits = 0, dec_bm_min = 32, group_m_env = -1; };

// has_ws / ws_elems: the split-K workspace (GemmArgs::splitk_ws non-null, splitk_ws_elems); fused_ln: EPI_RESID with
// ln_out; w8: e4m3 weights (w8_scale); partials: launch_gemm_partials (slabs only, no reduce, epi = EPI_STORE)
struct GemmShape { int epi, M, N, K; bool has_ws; long ws_elems; bool fused_ln, w8, partials; };

enum GemmKernel { GK_8P, GK_GLDS, GK_DEC, GK_REG };       // gemm8p_ / gemm_glds_ / gemm_dec_ / gemm_kernel
enum GemmReduce { GR_NONE, GR_PLAIN, GR_LN, GR_LN4 };     // splitk_reduce_ / _resid_ln_ / _resid_ln4_kernel

struct GemmPlan {
    GemmKernel kernel; int bm, bn;       // tile: GK_8P 256x256, GK_GLDS 128x128, GK_DEC 32|64|128 x 64, GK_REG 64x64 | 128x64 | 128x128
    int grid_x, grid_y, grid_z, threads;
    int tiles_n;                         // GK_8P / GK_GLDS: column tiles (grid_x = tiles_n * row tiles)
    bool split; int splits, kc;          // split: partial sums go to the slabs; kc = K of one chunk (the whole K when unsplit)
    int gm;                              // GK_8P tile grouping
    GemmReduce reduce; int red_grid, red_threads, red_npt;
    char error[96];                      // non-empty: the call fails with this text, nothing is launched
};
// partials: splits = 0 when the shape / workspace does not allow the slabs (nothing to launch, no error)
GemmPlan gemm_plan(const GemmShape& s, const GemmKnobs& k);

}  // namespace wm
