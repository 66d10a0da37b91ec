// whisper_full_parallel's split and snap rules (parallel.h). Host only.
#include "parallel.h"

#include <cstdlib>

namespace wm {

std::vector<int> parallel_cuts(int n_samples, int offset_ms, int n_processors) {
    const int off = parallel_offset_samples(offset_ms), n_per = parallel_n_per(n_samples, offset_ms, n_processors);
    std::vector<int> cuts(n_processors, 0);
    for (int k = 1; k < n_processors; k++) cuts[k] = off + k * n_per;
    return cuts;
}

SnapRange parallel_snap_range(int n_samples, int cut, int snap) {
    if (snap <= 0) return {0, 0};
    const int64_t lo = (int64_t)cut - 16 * (int64_t)snap, hi = (int64_t)cut + 16 * (int64_t)snap;
    int64_t w_lo = lo <= 0 ? 0 : (lo + kParWindow - 1) / kParWindow;
    int64_t w_hi = hi < 0 ? -1 : hi / kParWindow;
    w_hi = std::min<int64_t>(w_hi, n_samples / kParWindow - 1);  // wholly inside the clip
    if (w_hi < w_lo) return {0, 0};
    return {(int)w_lo, (int)(w_hi - w_lo + 1)};
}

int parallel_snap_pick(const float* rms, SnapRange r, int cut) {
    if (r.n_w <= 0) return cut;
    const auto dist = [&](int i) { return std::abs((int64_t)kParWindow * (r.w_lo + i) - cut); };
    int best = 0;
    for (int i = 1; i < r.n_w; i++)
        if (rms[i] < rms[best] || (rms[i] == rms[best] && dist(i) < dist(best))) best = i;  // (equal distance: the smaller w stays)
    return kParWindow * (r.w_lo + best) + kParWindow / 2;
}

}  // namespace wm
