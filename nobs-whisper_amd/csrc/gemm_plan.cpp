// gemm_plan (gemm_plan.h): every decision of a GEMM launch, no HIP.
#include "gemm_plan.h"

#include <algorithm>
#include <cstdio>

namespace wm {
namespace {

int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// decode-step split count: the largest keeping the grid <= 256 workgroups (one per CU), with chunks
// of >= 2 K-tiles and at most 12 splits. Independent of M, so a row's sums never depend on the batch.
// Large-v3: FC1 3 splits, QKV 4, N = d GEMMs 10, FC2 12; against the round-2 rule (the smallest count
// reaching >= 160 workgroups, <= 8 splits) decode 844 -> 838 ms per step at 128 clips, 659 -> 654 at 64,
// 433 -> 413 at 16 (profiles/r02_dec_fill_ab.txt). Decode-step weights are read once per step by one
// workgroup each: non-temporal LDS-DMA (aux = 2).
int dec_splits_for(int tiles, int nk) {
    int splits = 1;
    while (tiles * (splits + 1) <= 256 && splits < 12 && (splits + 1) * 2 <= nk) splits++;
    return splits;
}
// The split plan of a gemm_dec_kernel launch (K % 64 == 0): dec_splits_for's count (or the override) as
// chunks of whole K-tiles, kc elements each, and the number of chunks that makes. splits = 0: the slabs do
// not fit the workspace.
struct DecPlan { int splits, kc; };
DecPlan dec_plan(const GemmShape& s, int splits_override) {
    const int nk = s.K / 64;
    int splits = dec_splits_for(cdiv(s.N, 64), nk);
    if (splits_override > 0) splits = std::min(splits_override, nk);
    const int kc = cdiv(nk, splits) * 64;
    splits = cdiv(s.K, kc);
    if ((long)splits * s.M * s.N > s.ws_elems) return {0, 0};
    return {splits, kc};
}

// The encoder GEMMs' tile order (gemm8p_kernel gm). Row-major (n fastest) lets the 32 workgroups an XCD
// runs at once cover ~1.6 m-tiles x 20 n-tiles of FC1, so every B tile is fetched by every XCD for every
// m-tile; groups of 4 m-tiles make them a 4 x 8 block. Measured (large-v3, 128 x 30 s, rocprofv3
// FETCH_SIZE x2, profiles/r05_gemm_gm_pmc.txt): FC1 2068 -> 1111 MB per launch, QKV 1243 -> 848 MB; the
// d-wide GEMMs (5 n-tiles) fetched more (857 -> 987 MB), and stay row-major. The encode phase time does not
// move (321.3 / 320.1 / 324.0 / 331.8 ms at gm 0 / 4 / 8 / 16): the kernel is bound by its MFMA / LDS
// schedule, not by L2 misses.
int gemm_group_m(int tiles_n, int env) {
    if (env >= 0) return env;
    return tiles_n >= 8 ? 4 : 0;
}

GemmPlan fail(GemmPlan p, const char* fmt, int arg) {
    snprintf(p.error, sizeof p.error, fmt, arg);
    return p;
}

void grid(GemmPlan& p, int x, int y, int z, int threads) {
    p.grid_x = x; p.grid_y = y; p.grid_z = z; p.threads = threads;
}

// gemm_dec_kernel over the DecPlan's chunks. Row tile: the smallest of 32 / 64 / 128 rows that holds the step
// (the grid's row chunks stay cdiv(M, 128): a smaller tile is only taken when one tile holds every row);
// dec_bm_min caps the tile from below for the A/B (128: always 128 rows, the round-5 kernel). Every value
// gives the same bits.
// 65..128 rows stay one 128-row tile: two 64-row chunks (on gridDim.y, or 8 ids apart so both land on one
// XCD's L2) read each weight tile twice and measured slower in the 128-clip step (decode 809 -> 832-840 ms,
// profiles/r06_bm_m64_ab_*.json) though some isolated shapes gained (xq 11.9 -> 10.7 us)
void dec_kernel(GemmPlan& p, const GemmShape& s, const DecPlan& d, int bm_min, bool split) {
    p.kernel = GK_DEC;
    p.bm = s.M <= 32 && bm_min <= 32 ? 32 : s.M <= 64 && bm_min <= 64 ? 64 : 128;
    p.bn = 64;
    p.split = split; p.splits = d.splits; p.kc = d.kc;
    grid(p, cdiv(s.N, 64), p.bm == 128 ? cdiv(s.M, 128) : 1, d.splits, 256);
}

// gemm_kernel (register-staged): unsplit over the whole K, or `splits` chunks of kc
void reg_kernel(GemmPlan& p, const GemmShape& s, int bm, int bn, int rows_y, int splits) {
    p.kernel = GK_REG;
    p.bm = bm; p.bn = bn;
    p.split = splits > 0;
    if (p.split) {
        p.kc = cdiv(cdiv(s.K, splits), 64) * 64;
        p.splits = cdiv(s.K, p.kc);
    }
    grid(p, cdiv(s.N, bn), rows_y, p.splits, 256);
}

// the plain split-K reduce of a decode step: one thread per 4 columns (N % 4 == 0), 64-thread
// workgroups when that is under 64K threads so the work spreads over every CU (at 128 clips a d-wide
// reduce is 41K threads: 160 busy 256-thread workgroups before, 640 of 64 now); the same bits
void reduce_plain(GemmPlan& p, const GemmShape& s) {
    const long total = (long)s.M * s.N, work = (s.N & 3) == 0 ? total / 4 : total;
    p.reduce = GR_PLAIN;
    p.red_threads = work < 65536 ? 64 : 256;
    p.red_grid = (int)std::min<long>(4096, cdiv(work, p.red_threads));
}

// the reduce fused with the next LayerNorm, one workgroup per row. ln4: take the 4-columns-per-thread kernel
// where it applies (the register-staged path never did, and the two kernels' LayerNorm sums associate
// differently, so it keeps its choice)
GemmPlan reduce_ln(GemmPlan p, const GemmShape& s, bool ln4) {
    p.red_grid = s.M;
    if (ln4 && s.N % 4 == 0 && s.N <= 4096 && p.splits <= 16) {
        p.reduce = GR_LN4;
        p.red_threads = cdiv(s.N / 4, 64) * 64;
        return p;
    }
    const int npt = cdiv(s.N, 256);
    if (npt > 8) return fail(p, "fused LN width %d > 2048", s.N);
    p.reduce = GR_LN;
    p.red_threads = 256;
    p.red_npt = npt <= 4 ? 4 : 8;
    return p;
}

}  // namespace

GemmPlan gemm_plan(const GemmShape& s, const GemmKnobs& k) {
    GemmPlan p{};
    p.kernel = GK_REG;
    p.splits = 1; p.kc = s.K;
    p.grid_y = p.grid_z = 1;
    const bool k64 = s.K % 64 == 0;
    if (s.partials) {  // the slabs of a decode-step projection for a consumer that reduces them itself
        DecPlan d{0, 0};
        if (s.has_ws && s.M <= 128 && k64) d = dec_plan(s, k.dec_splits);
        dec_kernel(p, s, d, k.dec_bm_min, true);
        return p;
    }
    // e4m3 weights: the decode-step split-K kernel only
    if (s.w8 && !(s.has_ws && s.M <= 128 && k64 && k.variant != 0 && (s.epi != EPI_RESID || s.fused_ln)))
        return fail(p, "e4m3 weights need the decode-step GEMM path (M %d <= 128, K %% 64 == 0)", s.M);
    if ((long)s.M * s.N >= 256L * 128 * 128) {  // the big shapes: encoder, cross K/V, prefill
        const bool big256 = k.variant >= 2 || (k.variant < 0 && (s.N % 256 == 0 || s.N >= 1024) && s.M >= 1024);
        if (k64 && big256) {
            p.kernel = GK_8P; p.bm = p.bn = 256;
            p.tiles_n = cdiv(s.N, 256);
            p.gm = gemm_group_m(p.tiles_n, k.group_m_env);
            grid(p, p.tiles_n * cdiv(s.M, 256), 1, 1, 512);
        } else if (k64 && k.variant != 0) {
            p.kernel = GK_GLDS; p.bm = p.bn = 128;
            p.tiles_n = cdiv(s.N, 128);
            grid(p, p.tiles_n * cdiv(s.M, 128), 1, 1, 256);
        } else {
            reg_kernel(p, s, 128, 128, cdiv(s.M, 128), 0);
        }
        return p;
    }
    const int nk = cdiv(s.K, 64);
    if (s.has_ws && (s.M <= 128 || !s.fused_ln) && k64 && k.variant != 0) {
        // decode step and small prefill (gemm_dec_kernel; M > 128 as 128-row chunks, gridDim.y): the
        // split count depends on N and K only (dec_splits_for), so a row's sums, and the bits of every
        // result, do not depend on how many clips share the launch (batch == single). (Chunks of >= 5
        // K-tiles measured faster in isolation, 9.6 vs 10.4 us at N = K = 1280, but not in the decode
        // step: 82.0 vs 81.6 us of GEMM + reduce per layer.)
        const DecPlan d = dec_plan(s, k.dec_splits);
        // unsplit at M <= 64 (the logits GEMM of a small batch): the 64-row register-staged kernel
        // below wastes less of its tile (measured 23 vs 51 us at M = 16, N = 51866)
        const bool small_unsplit = d.splits == 1 && !s.fused_ln && s.M <= 64 && !s.w8;
        if (s.w8 && !d.splits) return fail(p, "e4m3 decode GEMM: split-K workspace too small", 0);
        if (d.splits && !small_unsplit) {
            const bool split = d.splits > 1 || s.fused_ln;
            dec_kernel(p, s, d, k.dec_bm_min, split);
            if (!split) return p;
            if (s.fused_ln) return reduce_ln(p, s, true);
            reduce_plain(p, s);
            return p;
        }
    }
    if (s.has_ws && s.M <= 128) {
        // decode step (M = active clips <= 128): one M tile, the weight stream read exactly once;
        // K split to ~128 workgroups with >= 4 K-tiles each (partial slabs: M*N*splits*8 bytes)
        const int tiles = cdiv(s.N, 64);
        int splits = std::min(std::max(1, 128 / tiles), std::max(1, nk / 4));
        while (splits > 1 && (long)splits * s.M * s.N > s.ws_elems) splits--;
        const bool split = splits > 1 || s.fused_ln;
        reg_kernel(p, s, s.M <= 64 ? 64 : 128, 64, 1, split ? splits : 0);
        if (!split) return p;
        if (s.fused_ln) return reduce_ln(p, s, false);
        reduce_plain(p, s);
        return p;
    }
    if (s.fused_ln) return fail(p, "fused LN requires the decode split-K path", 0);
    const int tiles = cdiv(s.N, 64) * cdiv(s.M, 64);
    int splits = std::min(16, std::max(1, 512 / tiles));
    splits = std::min(splits, std::max(1, nk / 2));
    while (splits > 1 && (long)splits * s.M * s.N > s.ws_elems) splits--;
    const bool split = s.has_ws && splits > 1;
    reg_kernel(p, s, 64, 64, cdiv(s.M, 64), split ? splits : 0);
    if (split) {
        p.reduce = GR_PLAIN;
        p.red_threads = 256;
        p.red_grid = (int)std::min<long>(1024, cdiv((long)s.M * s.N, 256));
    }
    return p;
}

}  // namespace wm
