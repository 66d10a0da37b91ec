// Silero-VAD (whisper_vad_*, whisper_full_params.vad), the host half that needs no HIP: the model file's
// parser (vad_file.cpp), and get_speech_timestamps, the piece table of the filtered audio and the time map
// (vad_segments.cpp). Both build with a plain C++ compiler (tools/vad_check.cpp); tests/vad_ref.py is their reference.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace wm {

constexpr int kVadRate = 16000;
constexpr int kVadWindow = 512;   // samples per probability
constexpr int kVadPad = 64;       // reflect padding on both sides of a window
constexpr int kVadFft = 256, kVadHop = 128, kVadBins = 129, kVadFrames = 4;
constexpr int kVadHidden = 128;
constexpr int kVadGap = 1600;     // zero samples between two pieces of the filtered audio

// The tensors of a model file as f32, in torch layout (f16 tensors are widened at load).
struct VadFile {
    std::vector<float> basis;            // [258][256]
    std::vector<float> conv_w[4];        // [out][in][3]
    std::vector<float> conv_b[4];        // [out]
    std::vector<float> w_ih, w_hh;       // [512][128], gates i, f, g, o
    std::vector<float> b_ih, b_hh;       // [512]
    std::vector<float> head_w;           // [128]
    std::vector<float> head_b;           // [1]
};
constexpr int kVadConvIn[4] = {129, 128, 64, 64}, kVadConvOut[4] = {128, 64, 64, 128}, kVadConvStride[4] = {1, 2, 2, 1};

// Parses the file image [data, data + size): the 16 kHz v5 geometry only. false and a reason in *err for anything else:
// another magic, type or geometry, an unknown, missing or duplicate tensor, another shape or element type, a
// truncated record. Never reads past the buffer.
bool vad_parse(const uint8_t* data, size_t size, VadFile& out, std::string* err);

struct VadParams {  // whisper_vad_params
    float threshold;
    int min_speech_duration_ms, min_silence_duration_ms;
    float max_speech_duration_s;
    int speech_pad_ms;
    float samples_overlap;
};
struct VadSpan { int start, end; };  // samples of the original audio
// Silero's get_speech_timestamps over the window probabilities; the audio counts as n_probs * 512 samples long.
std::vector<VadSpan> vad_segments_from_probs(const float* probs, int n_probs, const VadParams& p);

struct VadPiece { int orig_start, orig_end, vad_start, vad_end; };  // samples
// Segment k copied as [s_k, min(e_k + overlap, s_{k+1})), the last as [s_k, e_k), ends clamped to n_samples; pieces lie
// end to end with kVadGap zeros between them. The overlap is clamped to the next start so that the map stays monotone.
std::vector<VadPiece> vad_piece_table(const std::vector<VadSpan>& segs, int n_samples, float samples_overlap);
inline int vad_filtered_len(const std::vector<VadPiece>& t) { return t.empty() ? 0 : t.back().vad_end; }
// a time on the filtered axis (10 ms units) back to the original axis: inside a piece by its offset, in the gap after a
// piece or beyond the last one the piece's end
int64_t vad_map_time(const std::vector<VadPiece>& t, int64_t t10ms);

}  // namespace wm
