// Silero-VAD on the device (whisper_vad_*, whisper_full_params.vad): the model's weights, the buffers of
// a run, and the three launches of kernels/vad.hip. The host half that needs no HIP is vad_segments.h.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "vad_segments.h"

namespace wm {

// The weights on the device, f32, in the layouts the kernels read: every matrix k-major ([k][out]) so that the threads
// of a wave, one output each, load a row of it coalesced. A conv's k is tap * Cp + channel, where Cp is the input
// channel count (132 for layer 0: 129 padded with zero rows to a multiple of four).
struct VadWeights {
    const float* basis_t;    // [256][258]
    const float* conv_t[4];  // [3 * Cp][out]
    const float* conv_b[4];  // [out]
    const float* wih_t;      // [128][512]
    const float *b_ih, *b_hh;  // [512]
    const float* whh;        // [512][128], as in the file: thread g of vad_lstm keeps row g in registers
    const float* head_w;     // [128]
    float head_b;
};
constexpr int kVadC0Pad = 132;
constexpr int kVadTile = 4;  // windows per workgroup of vad_frontend

struct VadClip {
    const float* pcm;  // device
    int n_samples, n_win;
    long long win0;    // the clip's first row in xg [.][512], h [.][128] and probs [.]
};
struct VadGatherClip {
    const float* src;  // device: the original PCM
    float* dst;        // device: out_len filtered samples
    int piece0, n_pieces, out_len;
};

// xg[t] = W_ih x_t + b_ih + b_hh of every window of every clip: one workgroup per (clip, tile of kVadTile windows)
void launch_vad_frontend(const VadWeights& w, const VadClip* clips, int n_clips, int max_win, float* xg, hipStream_t st);
// the LSTM chain of every clip, one workgroup of 512 threads per clip, then the head over its stored h: probs
void launch_vad_lstm(const VadWeights& w, const VadClip* clips, int n_clips, const float* xg, float* h, float* probs, hipStream_t st);
// the filtered PCM of every clip from its pieces (zeros in the gaps), one thread per output sample
void launch_vad_gather(const VadGatherClip* clips, const VadPiece* pieces, int n_clips, int max_out, hipStream_t st);

struct VadModel {
    VadWeights w{};
    float* blob = nullptr;  // one allocation behind every pointer of w
    int device = 0;
};
// Parses the file image and uploads it (synchronous). nullptr and a reason in *err when the parser refuses it.
VadModel* vad_model_load(const uint8_t* data, size_t size, int device, std::string* err);
VadModel* vad_model_load_file(const char* path, int device, std::string* err);
void vad_model_free(VadModel* m);

// called around every launch (the engine times them as kernel class K_VAD); null: nothing
struct VadHooks {
    void (*begin)(void* u, int kernel, double bytes);  // kernel: 0 frontend, 1 lstm, 2 gather
    void (*end)(void* u);
    void* u;
};

// the device buffers of a run, grown on demand and kept
struct VadScratch {
    float *pcm = nullptr, *xg = nullptr, *h = nullptr, *probs = nullptr, *out = nullptr;
    VadClip* clips = nullptr;
    VadGatherClip* gclips = nullptr;
    VadPiece* pieces = nullptr;
    size_t cap_pcm = 0, cap_xg = 0, cap_h = 0, cap_probs = 0, cap_out = 0, cap_pieces = 0;  // elements of each buffer
    int cap_clips = 0, cap_gclips = 0;
    std::vector<const float*> dev_pcm;  // after vad_probs_run: where each clip's PCM is on the device
};
void vad_scratch_free(VadScratch& sc);

// Probabilities of every 512-sample window of every clip (host PCM is uploaded to sc.pcm, each clip on a 64-float
// boundary): frontend, lstm + head, one copy back; synchronises st. xg_out (host, or null): the LSTM inputs of clip 0.
void vad_probs_run(const VadModel& m, VadScratch& sc, const float* const* pcm, const int* n, int n_clips, bool on_device,
                   hipStream_t st, const VadHooks* hooks, std::vector<std::vector<float>>& probs, float* xg_out);
// The filtered PCM of every clip into sc.out (each clip on a 64-float boundary) from its device PCM and piece table;
// synchronises st. out_ptr / out_len: per clip.
void vad_gather_run(VadScratch& sc, const float* const* dev_pcm, const std::vector<std::vector<VadPiece>>& tables, hipStream_t st,
                    const VadHooks* hooks, std::vector<const float*>& out_ptr, std::vector<int>& out_len);

}  // namespace wm
