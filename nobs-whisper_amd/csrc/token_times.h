// Per-token t0 / t1 / vlen and max_len wrapping (whisper_full_params.token_timestamps, thold_pt, thold_ptsum,
// max_len, split_on_word): the host parts, free of HIP, so tools/token_times_check.cpp builds with a
// plain C++ compiler. Times are 10 ms units, absolute within the clip.
//
// phase 1 (tt_phase1) places a segment's tokens from its timestamp tokens and spreads the intervals in between
// by voice length; the voice-activity adjust between phase 1 and the wrap runs on the device (kernels/tokts.hip);
// tt_wrap cuts a segment into pieces of at most max_len bytes of text.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace wm {

struct TtTok {
    int id = 0, tid = 0;
    float pt = 0.0f, ptsum = 0.0f;
    int64_t t0 = -1, t1 = -1;
    float vlen = 0.0f;
};
// per clip, for one whisper_full / full_batch call
struct TtState {
    int64_t t_beg = 0, t_last = 0;
    int tid_last = 0;
};
struct TtPiece {
    int i0 = 0, i1 = 0;  // tokens [i0, i1) of the segment that was wrapped
    int64_t t0 = 0, t1 = 0;
    std::string text;
};

// f32 sum over the bytes: ' ' 0.01, ',' 2, '.' '!' '?' 3, a digit 3, any other byte 1
float tt_voice_length(const std::string& s);
// double -> int64, truncating; NaN -> 0, out of range -> the nearest end (no undefined conversion)
int64_t tt_trunc(double x);
// `vocab`: the string of every token id (whisper_token_to_str), specials included
void tt_phase1(std::vector<TtTok>& tok, int64_t t0, int64_t t1, TtState& st, int token_beg, float thold_pt, float thold_ptsum,
               const std::vector<std::string>& vocab);
// the pieces of a segment [t0, t1] with tokens `tok` (their t0 as adjusted), in order; always at least one
std::vector<TtPiece> tt_wrap(const std::vector<TtTok>& tok, int64_t t0, int64_t t1, int max_len, bool split_on_word,
                             int token_eot, const std::vector<std::string>& vocab);

}  // namespace wm
