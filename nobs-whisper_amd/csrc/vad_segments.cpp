// get_speech_timestamps, the piece table and the time map of the VAD filter (vad_segments.h; no HIP header).
#include "vad_segments.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace wm {

namespace {
constexpr int kBig = INT_MAX / 2 + 1;  // 2^30 samples: "unbounded"
// a caller's duration in ms as samples, computed in 64 bits and clamped to [-2^30, 2^30]
int ms_to_samples(int ms) { return (int)std::clamp<int64_t>((int64_t)kVadRate * ms / 1000, -(int64_t)kBig, kBig); }
}  // namespace

std::vector<VadSpan> vad_segments_from_probs(const float* probs, int n_probs, const VadParams& p) {
    const float thr = p.threshold;
    const float neg = std::max(thr - 0.15f, 0.01f);
    const int min_speech = ms_to_samples(p.min_speech_duration_ms);
    const int min_silence = ms_to_samples(p.min_silence_duration_ms);
    const int pad = ms_to_samples(p.speech_pad_ms);
    int max_speech = kBig;  // also for a value that is not finite, above 100000 s, or that leaves nothing after the pad
    if (std::isfinite(p.max_speech_duration_s) && p.max_speech_duration_s <= 100000.0f && p.max_speech_duration_s >= -100000.0f) {
        const int64_t v = (int64_t)((double)kVadRate * (double)p.max_speech_duration_s) - kVadWindow - 2 * (int64_t)pad;
        if (v >= 0 && v <= kBig) max_speech = (int)v;
    }
    const int min_silence_max = kVadRate * 98 / 1000;
    const int audio_len = n_probs * kVadWindow;

    std::vector<VadSpan> sp;
    bool triggered = false;
    int temp_end = 0, prev_end = 0, next_start = 0, start = 0;
    for (int i = 0; i < n_probs; i++) {
        const float prob = probs[i];
        const int cur = kVadWindow * i;
        if (prob >= thr && temp_end) {
            temp_end = 0;
            if (next_start < prev_end) next_start = cur;
        }
        if (prob >= thr && !triggered) {
            triggered = true;
            start = cur;
            continue;
        }
        if (triggered && cur - start > max_speech) {
            if (prev_end) {
                sp.push_back({start, prev_end});
                if (next_start < prev_end) triggered = false;
                else start = next_start;
                prev_end = next_start = temp_end = 0;
            } else {
                sp.push_back({start, cur});
                prev_end = next_start = temp_end = 0;
                triggered = false;
                continue;
            }
        }
        if (prob < neg && triggered) {
            if (!temp_end) temp_end = cur;
            if (cur - temp_end > min_silence_max) prev_end = temp_end;
            if (cur - temp_end < min_silence) continue;
            if (temp_end - start > min_speech) sp.push_back({start, temp_end});
            prev_end = next_start = temp_end = 0;
            triggered = false;
            continue;
        }
    }
    if (triggered && audio_len - start > min_speech) sp.push_back({start, audio_len});

    for (size_t k = 0; k < sp.size(); k++) {
        // (64 bits: the pad may be as large as 2^30)
        if (k == 0) sp[k].start = (int)std::max<int64_t>(0, (int64_t)sp[k].start - pad);
        if (k + 1 < sp.size()) {
            const int silence = sp[k + 1].start - sp[k].end;
            if (silence < 2 * (int64_t)pad) {
                sp[k].end += silence / 2;
                sp[k + 1].start = std::max(0, sp[k + 1].start - silence / 2);
            } else {
                sp[k].end = (int)std::min<int64_t>(audio_len, (int64_t)sp[k].end + pad);
                sp[k + 1].start = (int)std::max<int64_t>(0, (int64_t)sp[k + 1].start - pad);
            }
        } else sp[k].end = (int)std::min<int64_t>(audio_len, (int64_t)sp[k].end + pad);
    }
    return sp;
}

std::vector<VadPiece> vad_piece_table(const std::vector<VadSpan>& segs, int n_samples, float samples_overlap) {
    // a negative or non-finite overlap counts as none, a huge one as 2^30 samples
    const float ov = samples_overlap * (float)kVadRate;
    const int overlap = !std::isfinite(ov) || ov <= 0.0f ? 0 : ov >= (float)kBig ? kBig : (int)ov;
    std::vector<VadPiece> out;
    int pos = 0;
    for (size_t k = 0; k < segs.size(); k++) {
        const int s = std::min(segs[k].start, n_samples);
        int e = std::min(segs[k].end, n_samples);
        if (k + 1 < segs.size()) e = (int)std::min<int64_t>((int64_t)e + overlap, std::min(segs[k + 1].start, n_samples));
        if (e <= s) continue;
        if (!out.empty()) pos += kVadGap;
        out.push_back({s, e, pos, pos + (e - s)});
        pos += e - s;
    }
    return out;
}

int64_t vad_map_time(const std::vector<VadPiece>& t, int64_t t10ms) {
    if (t.empty()) return t10ms;
    const int64_t x = t10ms * 160;
    int64_t orig = t[0].orig_start;
    for (const VadPiece& q : t) {
        if (x < q.vad_start) break;
        orig = x < q.vad_end ? q.orig_start + (x - q.vad_start) : q.orig_end;
    }
    // floor division (x may be negative only for a negative time, which no caller passes)
    return orig >= 0 ? orig / 160 : -((-orig + 159) / 160);
}

}  // namespace wm
