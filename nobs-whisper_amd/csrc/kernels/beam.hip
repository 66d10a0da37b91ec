// Self-cache gather for beam search: when hypotheses are re-parented, rows [row0, row1) of K
// and V of every layer and head move from the parent's self slot to the beam's, for all clips in one launch.
//
// Cache [slots][L][2][H][n_ctx][64] in a 2-byte type: a row is 128 bytes = 8 x 16 bytes, and the rows
// [row0, row1) of one (layer, K|V, head) are contiguous, so a copy is L * 2 * H segments of (row1 - row0) * 8
// 16-byte units. Thread u of a copy moves unit u % (rows * 8) of segment u / (rows * 8): 8 consecutive lanes
// move one whole row, a wavefront 8 rows, every access 16 bytes. Pure bandwidth: each byte is read and written
// once (twice for a staged copy).
//
// Parallel assignment (every copy reads the cache as it was before the launch) by the host's schedule
// (beam.h beam_schedule): a copy whose destination no copy reads goes straight from src to dst in phase 0;
// the others are read into the staging buffer in phase 0 and written to dst in phase 1, a second launch that
// runs only when some copy is staged. Phase 0 writes only slots that nothing reads, phase 1 reads only the
// staging buffer, so neither phase has a hazard within itself.
#include <algorithm>

#include "../beam.h"
#include "../common.h"
#include "../kernels.h"

namespace wm {

static constexpr int GT = 256;

__global__ void __launch_bounds__(GT) kv_gather_kernel(uint4* __restrict__ cache, uint4* __restrict__ stage,
                                                       const KvCopy* __restrict__ copies, int segs, int n_ctx, int phase) {
    const KvCopy c = copies[blockIdx.y];
    if (phase == 1 && c.mode == 0) return;
    const int seg_units = (c.row1 - c.row0) * 8;
    const long units = (long)segs * seg_units;
    const long slot_units = (long)segs * n_ctx * 8;
    const uint4* src = cache + (long)c.src_slot * slot_units + (long)c.row0 * 8;
    uint4* dst = cache + (long)c.dst_slot * slot_units + (long)c.row0 * 8;
    uint4* stg = stage + c.stage_off;
    for (long u = (long)blockIdx.x * GT + threadIdx.x; u < units; u += (long)gridDim.x * GT) {
        const long seg = u / seg_units;
        const long at = seg * n_ctx * 8 + (u - seg * seg_units);
        if (phase == 0) {
            const uint4 x = src[at];
            if (c.mode == 0) dst[at] = x;
            else stg[u] = x;
        } else {
            dst[at] = stg[u];
        }
    }
}

void launch_kv_gather(void* cache, int n_slots, int L, int H, int n_ctx, const KvCopy* copies_host, const KvCopy* copies_dev,
                      int n_copies, void* stage, long stage_units, hipStream_t st) {
    if (n_copies <= 0) return;
    const int segs = L * 2 * H;
    long max_units = 0, need = 0;
    bool staged = false;
    for (int i = 0; i < n_copies; i++) {
        const KvCopy& c = copies_host[i];
        if (c.dst_slot < 0 || c.dst_slot >= n_slots || c.src_slot < 0 || c.src_slot >= n_slots || c.row0 < 0 ||
            c.row1 > n_ctx || c.row0 >= c.row1)
            WM_FAIL("kv gather: copy %d {%d <- %d, rows [%d, %d)} outside %d slots x %d rows", i, c.dst_slot, c.src_slot, c.row0,
                    c.row1, n_slots, n_ctx);
        const long units = (long)segs * (c.row1 - c.row0) * 8;
        max_units = std::max(max_units, units);
        if (c.mode) {
            staged = true;
            if (c.stage_off < 0) WM_FAIL("kv gather: copy %d has a negative staging offset", i);
            need = std::max(need, c.stage_off + units);
        }
    }
    if (staged && (!stage || need > stage_units)) WM_FAIL("kv gather: staging buffer of %ld units, %ld needed", stage_units, need);
    const dim3 grid((unsigned)std::min<long>(cdiv(max_units, (long)GT), 2048), n_copies);
    kv_gather_kernel<<<grid, GT, 0, st>>>((uint4*)cache, (uint4*)stage, copies_dev, segs, n_ctx, 0);
    if (staged) kv_gather_kernel<<<grid, GT, 0, st>>>((uint4*)cache, (uint4*)stage, copies_dev, segs, n_ctx, 1);
    WM_CHECK(hipGetLastError());
}

}  // namespace wm
