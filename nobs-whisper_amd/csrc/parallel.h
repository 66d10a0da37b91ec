// whisper_full_parallel, the host half that needs no HIP: where a recording is cut into pieces, how a
// cut moves to the quietest 20 ms near it, and how a piece's times go back to the recording's axis when the pieces are
// merged. Builds with a plain C++ compiler (tools/parallel_check.cpp); tests/parallel_ref.py is its reference.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace wm {

constexpr int kParRate = 16000;
constexpr int kParWindow = 320;   // samples of an RMS window (20 ms)
constexpr int kParallelMax = 128; // pieces of one call: the clips of one scheduler

// upstream's offset_samples = WHISPER_SAMPLE_RATE * offset_ms / 1000 and n_samples_per_processor, in its int arithmetic
inline int parallel_offset_samples(int offset_ms) { return (int)((int64_t)kParRate * offset_ms / 1000); }
inline int parallel_n_per(int n_samples, int offset_ms, int n_processors) {
    return (n_samples - parallel_offset_samples(offset_ms)) / n_processors;
}
// The piece starts: cuts[0] = 0 (piece 0 keeps the caller's offset_ms), cuts[k] = offset_samples + k * n_per. Piece k is
// [cuts[k], cuts[k + 1]), the last one runs to n_samples (it takes the remainder). n_per > 0.
std::vector<int> parallel_cuts(int n_samples, int offset_ms, int n_processors);

// snap_ms bounded so that moved cuts stay strictly increasing: min(snap_ms, 1000 * (n_per / 2 - 320) / 16000); <= 0: off
inline int parallel_snap(int snap_ms, int n_per) {
    return (int)std::min<int64_t>(snap_ms, (int64_t)1000 * (n_per / 2 - kParWindow) / kParRate);
}
// the RMS windows w that lie wholly inside the clip with |320 w - cut| <= 16 * snap: [w_lo, w_lo + n_w)
struct SnapRange { int w_lo, n_w; };
SnapRange parallel_snap_range(int n_samples, int cut, int snap);
// rms[i] = the RMS of window r.w_lo + i. The lowest wins, then the smaller |320 w - cut|, then the smaller w; the new cut
// is 320 w + 160. An empty range leaves the cut.
int parallel_snap_pick(const float* rms, SnapRange r, int cut);

// what a time (10 ms units) of the piece that starts at `cut` gains when it is merged
inline int64_t parallel_shift(int cut, int offset_ms) {
    return (int64_t)100 * (cut - parallel_offset_samples(offset_ms)) / kParRate + offset_ms / 10;
}
// a merged segment of a piece k >= 1: shifted, then t0 = max(t0, the t1 of the segment merged before it)
inline void parallel_place(int64_t shift, int64_t last_t1, bool have_last, int64_t& t0, int64_t& t1) {
    t0 += shift;
    t1 += shift;
    if (have_last && t0 < last_t1) t0 = last_t1;
}
// a token's t0, t1 or t_dtw: shifted unless it is -1 (not set); never clamped
inline int64_t parallel_token_time(int64_t t, int64_t shift) { return t == -1 ? t : t + shift; }
// The segments of a piece k >= 1 appended to the merged list (Seg: t0, t1, tokens with t0, t1, t_dtw; engine.h's
// Segment is one); appended() runs after each one, when it is the list's last.
template <typename Seg, typename F>
void parallel_merge_piece(std::vector<Seg>& out, std::vector<Seg>& piece, int64_t shift, F&& appended) {
    for (Seg& g : piece) {
        parallel_place(shift, out.empty() ? 0 : out.back().t1, !out.empty(), g.t0, g.t1);
        for (auto& t : g.tokens) {  // (a deviation from upstream, which leaves them relative to the piece)
            t.t0 = parallel_token_time(t.t0, shift);
            t.t1 = parallel_token_time(t.t1, shift);
            t.t_dtw = parallel_token_time(t.t_dtw, shift);
        }
        out.push_back(std::move(g));
        appended();
    }
}

}  // namespace wm
