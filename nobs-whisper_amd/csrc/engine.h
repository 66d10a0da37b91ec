// Engine internals: model (weights in one HBM arena), vocabulary/tokenizer, per-state workspace,
// and the batched window scheduler that implements whisper_full semantics for many clips at once.
#pragma once
#include <map>
#include <memory>
#include <atomic>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/whisper_mi355x.h"
#include "beam.h"
#include "common.h"
#include "grammar.h"
#include "kernels.h"
#include "parallel.h"
#include "vad.h"

namespace wm {

struct Hparams {
    int32_t n_vocab, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels, ftype;
};

// whisper.cpp's whisper_vocab semantics (special ids shift for multilingual files, extra
// tokens synthesised up to n_vocab) — SURVEY.md §8a rows a4, a12.
struct Vocab {
    int n_vocab = 51864;
    int token_eot = 50256, token_sot = 50257, token_translate = 50357, token_transcribe = 50358;
    int token_solm = 50359, token_prev = 50360, token_nosp = 50361, token_not = 50362, token_beg = 50363;
    std::map<std::string, int> token_to_id;
    std::vector<std::string> id_to_token;
    bool is_multilingual() const { return n_vocab >= 51865; }
    int num_languages() const { return n_vocab - 51765 - (is_multilingual() ? 1 : 0); }
};

extern const char* const k_lang_codes[100];
extern const char* const k_lang_names[100];
int lang_index(const char* code);
std::vector<int> tokenize(const Vocab& v, const std::string& text);

struct LayerW {
    float *ln1_w, *ln1_b;
    void* wqkv; float* bqkv;
    void* wo; float* bo;
    float *lnx_w, *lnx_b;     // decoder cross-attn LN
    void* wxq; float* bxq;    // decoder cross-attn query
    void* wxo; float* bxo;    // decoder cross-attn out
    float *ln2_w, *ln2_b;
    void* w1; float* b1;
    void* w2; float* b2;
    // block-quantized GGML files: the projection weights as the file's blocks (the compute-type
    // pointers above are null then, except where a layer's matrix was stored unquantized)
    QMat qqkv, qo, qxq, qxo, q1, q2;
};

struct Weights {
    void* conv1_w; float* conv1_b;
    void* conv2_w; float* conv2_b;
    float* pos_e;
    float *lnpost_w, *lnpost_b;
    void* tok_emb; float* pos_d;
    float* tok_emb_f32 = nullptr;       // quantized GGML embedding: exact f32 rows for the lookups
    float *lnd_w, *lnd_b;
    void* wkv_cross; float* bkv_cross;  // [L_d][2][d][d], bias [L_d][2][d] (K part zero)
    void* wkT = nullptr;                // [L_d][H][d][64]: cross K per head, transposed (direct cross attention)
    std::vector<LayerW> enc, dec;
    void* mel_tab;    // MelTablesDev (sin, cos, hann)
    float* filt_t;    // [201][n_mels]
};

struct Context {
    Hparams hp;
    Vocab vocab;
    VocabIds vid;
    DType dt = DType::F16;
    int device = 0;
    std::string path;
    int filt_n_mel = 0, filt_n_fft = 0;
    std::vector<float> filters;
    Weights w;
    char* arena = nullptr;
    size_t arena_bytes = 0;
    whisper_timings timings{};
    std::mutex timings_mu;  // states on different threads add their phase times here
    whisper_state* default_state = nullptr;  // whisper_init_from_file_with_params (with state)
    float k_scale = 0.0f;                    // d_head^-0.25
    // Cross attention straight from the encoder output (kernels/xattn.hip) is available for this
    // model (its per-head transposed Wk is in the arena); each call picks direct or cached form.
    bool cross_direct = false;
    // block-quantized file (ggml type of its projection matrices, 0 = f16/f32 file) kept quantized in
    // the arena: decode steps of few clips read the blocks (gemm_small_kernel, the persistent step);
    // the big-M GEMMs (encoder, prefill, decode steps of many clips) read a compute-type copy of every
    // projection, expanded once per context on first use (ensure_expanded, engine.cpp)
    int quant = 0;
    struct LayerMats { const void *wqkv, *wo, *wxq, *wxo, *w1, *w2; };
    std::mutex exp_mu;
    std::atomic<bool> expanded{false};
    char* arena_exp = nullptr;
    std::vector<LayerMats> exp_enc, exp_dec;
    std::string model_type;
    whisper_context* owner = nullptr;  // the whisper.h handle wrapping this context
    // fp8 encoder (large-v3-turbo fp8 config): QKV, FC1 and FC2 as e4m3 GEMMs with per-row scales.
    // The e4m3 weights are quantized from the loaded (or broadcast) bf16 weights on first use.
    struct Fp8Layer { void* wqkv = nullptr; float* sqkv = nullptr; void* w1 = nullptr; float* s1 = nullptr;
                      void* w2 = nullptr; float* s2 = nullptr; };
    bool fp8_enc = false;
    bool fp8_ready = false;
    std::mutex fp8_mu;
    std::vector<Fp8Layer> enc8;
    char* arena8 = nullptr;
    // fp8 mode, decoder: the decode-step projections (self QKV, self out, cross Q, cross out, FC1, FC2)
    // read e4m3 weights with per-output-row scales (same quantizer, same arena); the token embedding
    // (logits), the cross-attention K/V weights and prefill keep the compute type
    struct Fp8Dec { void *wqkv, *wo, *wxq, *wxo, *w1, *w2; float *sqkv, *so, *sxq, *sxo, *s1, *s2; };
    std::vector<Fp8Dec> dec8;
    // persistent decode step (kernels/pdec.hip): the decoder layers' pointers as a device array
    std::mutex pdec_mu;
    void* pdec_layers = nullptr;
    void* pdec_layers_exp = nullptr;  // (a quantized file's expanded copy)
    // States released by whisper_free_state, kept with their workspace and captured decode graphs
    // for the next whisper_init_state: whisper.rs:83-85 creates (and drops) a state on every
    // transcribe call, which would otherwise pay ~30 hipMallocs and a graph capture per call.
    std::mutex pool_mu;
    std::vector<whisper_state*> pool;
    // every state of this context that is alive (pooled or held by a caller), under pool_mu:
    // whisper_free orphans the ones a caller still holds, so a later whisper_free_state does not touch
    // the freed context (a garbage collector may finalise a context before its states)
    std::vector<whisper_state*> live;
    // token timestamps from cross-attention DTW (whisper_context_params.dtw_token_timestamps): the alignment
    // heads {layer, head} in list order, resolved once when the context is created (engine.cpp resolve_dtw)
    bool dtw = false;
    std::vector<std::pair<int, int>> dtw_heads;
    std::mutex dtw_mu;
    void* dtw_heads_dev = nullptr;  // int2 {head, index in dtw_heads} grouped by layer (dtw_layer_first)
    std::vector<int> dtw_layer_first;  // [n_text_layer + 1]: layer l's entries of dtw_heads_dev
    int dtw_last_layer = -1;
    // The deny mask of the last (suppress_nst, suppress_regex) asked for (suppress.h): matching the
    // whole vocabulary with std::regex costs milliseconds, so a call whose key equals the cached one rebuilds nothing.
    // States on different threads share it under the mutex and copy the words out.
    struct DenyKey {
        bool nst = false, has_regex = false;
        std::string regex;
        bool on() const { return nst || has_regex; }
        bool operator==(const DenyKey& o) const { return nst == o.nst && has_regex == o.has_regex && regex == o.regex; }
    };
    std::mutex deny_mu;
    bool deny_cached = false;
    DenyKey deny_key;
    std::vector<uint32_t> deny_words;
    long deny_builds = 0;  // masks built since the context was created (whisper_mi355x_suppress_builds)
    // The vocabulary decoded for grammar calls (grammar.h): built by the first one, under the mutex
    std::mutex gram_mu;
    bool gram_vocab_built = false;
    GramVocab gram_vocab;
    // ... and its copy on the device for the reject kernel (kernels.h GramTable; ~1 MB for large-v3's vocabulary), built
    // with it and freed with the context
    GramTable gram_tab{};
    void* gram_tab_mem[4] = {nullptr, nullptr, nullptr, nullptr};
    // The VAD model of the last whisper_full_params.vad_model_path asked for (vad.h), keyed by the path
    // (upstream keeps it per state). A call holds its own reference, so a call with another path on another thread
    // replaces the entry without pulling the weights from under it.
    std::mutex vad_mu;
    std::string vad_path;
    std::shared_ptr<VadModel> vad;
};

// The device side of a grammar call's masks (engine.cpp gram_masks): the call's flat rules, the rows' stack lists of a
// step and the rows' overflow words, with their pinned staging. A state's workspace has one; the debug hook its own.
struct GramDev {
    GramElem* elems = nullptr;
    int* rule_off = nullptr;
    size_t cap_elems = 0, cap_rules = 0;
    GramRow *rows = nullptr, *h_rows = nullptr;
    unsigned *over = nullptr, *h_over = nullptr;
    int cap_rows = 0;
    // masks built on the host (rows the kernel does not take, rows it flagged), by serialized state; at most 256, then
    // the table starts over
    std::unordered_map<std::string, std::vector<uint32_t>> host_masks;
    long rows_device = 0, rows_patched = 0, rows_host = 0;
};
void gram_dev_free(GramDev& d);
// the call's rules to the device (synchronises the stream); the host-mask table starts empty
void gram_dev_rules(GramDev& d, const GrammarRules& g, hipStream_t st);
// The reject words of n grammar states into gram [n][grammar_words] on the device, in stream order: the kernel for the
// rows it takes, grammar_reject on the host for rows whose stack list does not fit or whose pending partial has
// n_remain != 0, and for rows the kernel flagged (one synchronisation to read the flags). flags (if given): 0 decided
// by the kernel, 1 patched after overflow, 2 host only. h_stage: pinned [n][grammar_words]. s: the state whose
// K_GRAMMAR timing the launch goes to, or null.
void gram_masks(Context* c, GramDev& d, const GrammarRules& g, const Grammar* const* states, int n, uint32_t* gram,
                uint32_t* h_stage, int* flags, hipStream_t st, whisper_state* s);

struct TokenData {
    int id, tid;
    float p, plog, pt, ptsum;
    int64_t t_dtw = -1;  // 10 ms units; -1 = not aligned (DTW off, a timestamp token, an unaligned window)
    // whisper_full_params.token_timestamps (token_time_windows): 10 ms units, -1 / 0 when off
    int64_t t0 = -1, t1 = -1;
    float vlen = 0.0f;
};
// a token as whisper.h reports it (the getters; the history a logits_filter_callback gets)
inline whisper_token_data token_data(const TokenData& x) {
    whisper_token_data r;
    memset(&r, 0, sizeof(r));
    r.id = x.id; r.tid = x.tid; r.p = x.p; r.plog = x.plog; r.pt = x.pt; r.ptsum = x.ptsum;
    r.t0 = x.t0; r.t1 = x.t1; r.t_dtw = x.t_dtw; r.vlen = x.vlen;  // (-1, -1, 0 without token_timestamps)
    return r;
}

struct Segment {
    int64_t t0, t1;
    std::string text;
    float no_speech_prob;
    std::vector<TokenData> tokens;
    // whisper_full_params.tdrz_enable: a <|solm|> token lies in the segment's token range (false when the field is off)
    bool speaker_turn_next = false;
};

// Workspace sized for a batch of up to `cap_jobs` clips; grows on demand, never shrinks.
struct Workspace {
    int cap_jobs = 0, cap_enc = 0, cap_tok = 0;
    int cap_cross = 0;  // slots of the cross K/V cache (sized by the calls that use it, not cap_jobs)
    size_t cap_mel = 0, cap_pcm = 0;
    // encoder (cap_enc windows)
    void *mel_img = nullptr, *h1 = nullptr, *hn = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr;
    float* x = nullptr;
    float* hs = nullptr;  // fp8 encoder: per-row scales of the quantized GEMM inputs
    // caches (cap_jobs slots). In direct mode `cross` is allocated on first use (prompts too long
    // for the direct prefill) and cross_fresh[slot] says whether a slot's cross K/V match enc.
    void *cross = nullptr, *self = nullptr;
    std::vector<char> cross_fresh;
    int* kvslot = nullptr;  // identity [cap_jobs]: row_slot of a one-clip cross-KV GEMM
    void* wdq = nullptr;    // quantized files: one layer's projection weights dequantized (16 d^2)
    // direct cross attention: encoder output per slot [cap_jobs][T][d], Q' [cap_xq][2H][d],
    // split partials [xo_rows][H][d] f32 + [xo_rows][H][2]
    void *enc = nullptr, *qx = nullptr;
    float *xo = nullptr, *xml = nullptr;
    int cap_xq = 0;
    // decoder (cap_tok tokens)
    float* dx = nullptr;
    void *dh = nullptr, *dq = nullptr, *datt = nullptr, *dff = nullptr, *lrow = nullptr;
    float *logits = nullptr, *probs = nullptr;
    float* splitk = nullptr;  // split-K partial slabs for decode-step GEMMs
    long splitk_elems = 0;
    int *tok = nullptr, *pos = nullptr, *slot = nullptr, *nkv_self = nullptr, *nkv_cross = nullptr, *lrows = nullptr;
    SeqCtl* ctl = nullptr;
    TokOut* tout = nullptr;
    void* lrec = nullptr;  // split logits kernel: per-chunk records
    // the deny mask of suppress_nst / suppress_regex (suppress_words(n_vocab) words; allocated with the first
    // workspace and kept until the state goes, so its address can be a kernel argument of captured steps) and the
    // key of the mask it holds
    uint32_t* deny = nullptr;
    bool deny_held = false;
    Context::DenyKey deny_key;
    // the grammar's reject words of a step's rows, [cap_jobs][grammar_words(n_vocab)] (grammar.h), and
    // their pinned staging: sized with cap_jobs, so a captured step's pointer lives as long as its graph
    uint32_t* gram = nullptr;
    uint32_t* h_gram = nullptr;
    GramDev gd;
    // whisper_full_params.logits_filter_callback (allocated by the first call that has one, for cap_jobs
    // rows, so a captured step's pointer lives as long as its graph): the rows after the pre-callback rules
    // [cap_jobs][n_vocab] f32, and the pinned rows the callback edits
    float *frows = nullptr, *h_frows = nullptr;
    int *win_job = nullptr, *win_seek = nullptr, *win_slot = nullptr;
    // persistent decode step: the hand-off block (granules + error word) and the error word's host copy
    unsigned* pd_sync = nullptr;
    unsigned* h_pd_err = nullptr;
    // pipelined greedy decoding (engine.cpp decode_pipelined): two ring slots of [cap_jobs TokOut][16-byte error
    // word] on the device and in pinned host memory, and the event after each slot's copy
    char* ring = nullptr;
    char* h_ring = nullptr;
    hipEvent_t ring_ev[2] = {nullptr, nullptr};
    // beam search and best_of candidates (engine.cpp beam_step, sample_step): the self slot of every row of a step (rows of one clip share its cross
    // slot in `slot`), the top-k candidates [cap_jobs][kTopkMax] of the logits rows, the self-cache copies of a
    // re-parenting and the gather's staging buffer (grown on demand, 16-byte units)
    int *sslot = nullptr, *h_sslot = nullptr;
    int *sctr = nullptr, *h_sctr = nullptr;  // sampled draws: [cap_jobs][4] {seek, 16 * temp_idx + cand, token index, source row}
    TokOut *cand = nullptr, *h_cand = nullptr;
    KvCopy *kvcp = nullptr, *h_kvcp = nullptr;
    void* kvstage = nullptr;
    long kvstage_units = 0;
    // mel / pcm
    float* pcm = nullptr;
    float* mel = nullptr;
    float** mel_ptrs = nullptr;
    const float** pcm_ptrs = nullptr;
    int *n_samp = nullptr, *n_len = nullptr, *mel_max = nullptr;
    // host pinned staging
    int* h_ints = nullptr;
    int2* qtiles = nullptr;   // prefill attention tiles {first token, count} (cap_tok), device
    int2* h_qtiles = nullptr; // the same, pinned host staging
    int n_qtiles = 0;
    TokOut* h_tout = nullptr;
    SeqCtl* h_ctl = nullptr;
    // token-timestamp alignment (contexts with dtw_token_timestamps only; allocated by the first aligned
    // window): clip descriptors, score rows P of one group of clips (grown on demand), per-(head, frame)
    // statistics, the cost matrix and DTW trace of every slot's last aligned window, first frames per row
    AlignClip* al_clips = nullptr;
    float *al_P = nullptr, *al_stats = nullptr, *al_cost = nullptr;
    size_t al_P_elems = 0;
    unsigned char* al_trace = nullptr;
    int* al_fr = nullptr;
    char* h_al = nullptr;  // pinned: [cap_jobs AlignClip][cap_jobs * al_rows int]
    int al_cap = 0, al_rows = 0;
    // token times (whisper_full_params.token_timestamps; allocated by the first call that sets it): the clips'
    // energy signals, laid out as `pcm` (each clip on a 64-float boundary) and grown like it, the clip descriptors,
    // and the segment / token lists of one adjust launch (grown on demand)
    float* energy = nullptr;
    size_t cap_energy = 0;
    TtClip* tt_clips = nullptr;
    TtSeg* tt_segs = nullptr;
    TtSpan* tt_spans = nullptr;
    int tt_cap_clips = 0, tt_cap_segs = 0, tt_cap_spans = 0;
    // whisper_full_params.vad (allocated by the first call that sets it): the PCM, the LSTM inputs, h and the
    // probabilities of a call's clips, and the filtered PCM that compute_mel then reads
    VadScratch vad;
};

// Live per-kernel-class timing with HIP events on the state's stream (bench.py's roofline leg).
// `work` is the algorithmic FLOPs (MFMA-bound classes) or HBM bytes (HBM-bound classes).
enum KClass { K_GEMM_ENC = 0, K_ATTN_ENC, K_ATTN_CROSS, K_ATTN_SELF, K_GEMM_DEC, K_LOGITS, K_MEL, K_PDEC, K_OTHER,
              K_ALIGN_SCORES, K_ALIGN_COST, K_ALIGN_DTW, K_TOPK, K_KV_GATHER, K_SAMPLE, K_TOKTS, K_GRAMMAR, K_VAD, K_LOGITS_STAGE, K_NCLASS };
struct KStat { double ms = 0, work = 0; long count = 0; };

// What a decode step does besides greedy's plain step (whisper_state::mode; all off between steps). topk > 0: the
// logits launch is the top-k form with that many candidates per row (results in ws.h_cand; beam search).
// split_slots: the rows' self slots (ws.sslot) differ from their cross slots, so the step runs the launch chain in the
// cache form (the persistent step has one slot array). sample: the step's graph ends with launch_sample over ws.sctr
// (best_of candidates). key(): the mode as DecGraph::beam.
struct StepMode {
    int topk = 0;
    bool split_slots = false, sample = false;
    int key() const { return topk | (split_slots ? 1 << 8 : 0) | (sample ? 1 << 9 : 0); }
};

}  // namespace wm

struct whisper_state {
    wm::Context* ctx = nullptr;  // nullptr once the context was freed before the state (orphan)
    int device = 0;
    hipStream_t stream = nullptr;
    // second stream + fork/join events: decode steps run their rows as two groups concurrently
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    wm::Workspace ws;
    // cross attention form of the current call: straight from the encoder output (large batches) or
    // through a per-clip cross K/V cache (small batches, and whisper.cpp's own form)
    bool direct = false;
    // whisper.h single-clip results (job 0 of the last call) + batch results
    std::vector<std::vector<wm::Segment>> results;
    std::vector<int> lang_ids;
    std::vector<std::vector<whisper_mi355x_window_decision>> decisions;  // per job, per window
    std::vector<int> prompt_past;  // persists across whisper_full calls on this state
    std::mt19937 rng{0};           // decoder 0's rng: created with the state, never reset
    int lang_id = 0;
    int n_len = 0, n_len_org = 0;  // last mel
    // whisper_full_params.audio_ctx as the last whisper_full call stored it (or whisper_mi355x_set_audio_ctx): the
    // encoder positions that encode / decode / language detection on this state work on (wm::enc_ctx); <= 0 = the
    // model's n_audio_ctx. The caches keep n_audio_ctx as their row stride whatever this says.
    int audio_ctx = 0;
    std::vector<float> logits_host;
    double phase_ms[5] = {0, 0, 0, 0, 0};
    double align_ms = 0;  // token-timestamp alignment passes of the last call
    double tokts_ms = 0;  // token_timestamps passes (energy, phase 1, adjust, wrap) of the last call
    // whisper_full_params.vad: the wall time of the filter step of the last call (0 when off), and per
    // job the piece table that took its times back to the original axis (empty when off, or no speech)
    double vad_ms = 0;
    std::vector<std::vector<wm::VadPiece>> vad_maps;
    // the piece starts (samples) of the last whisper_full_parallel call on this state (whisper_mi355x_parallel_cuts)
    std::vector<int> par_cuts;
    // per job of the last call: the cost matrix of its last aligned window (rows x frames f32 on the device,
    // in this state's or its twin's workspace); rows = 0: no window of the job was aligned
    struct AlignInfo { int rows = 0, frames = 0; const float* cost = nullptr; };
    std::vector<AlignInfo> align_info;
    long decoded_tokens = 0;
    // standalone encode/decode API support
    int last_enc_windows = 0;
    bool mel_ready = false;  // whisper_pcm_to_mel (or a full call) has run on this state
    bool pooled = false;     // this state was recycled from the context's pool (workspace + graphs kept)
    // kernel timing (off unless whisper_mi355x_kernel_timing enabled it)
    int ktime_mask = 0;  // bit k: time kernel class k
    wm::KStat kstat[wm::K_NCLASS];
    wm::KStat vad_kstat[3];  // class K_VAD by kernel: frontend, lstm, gather (WHISPER_MI355X_KSTAT_VAD_*)
    struct KPending { int cls; hipEvent_t a, b; double work; int sub = 0; };  // sub: which kernel of class K_VAD
    std::vector<KPending> kpending;
    std::vector<hipEvent_t> kpool;
    // decode steps replayed as hipGraphs, one per (active-clip count, timing mask, cross form, path
    // signature): `sig` encodes the per-call switches that pick the step's kernels (dec_path_sig), so a
    // changed setting never replays a graph captured for another path
    // (gen: g_pdec_gen when a persistent step was captured; its graph holds the stamps pointer and spin limit of
    // that time, so a setter call retires it)
    // pdec: 0 = launch chain, 1 = the persistent step (kernels/pdec.hip)
    // (par: 0 for the per-step path; the pipelined path alternates two instances, 0 and 1, so that one step's
    // graph events are read while the other instance runs)
    // (beam: the step's mode, StepMode::key(): 0 for greedy steps; a sampled step's graph also depends on `seed`, the
    // draw's key)
    // (actx: the encoder positions of the call, wm::enc_ctx: the cross-attention split counts, grid sizes and the
    // direct form's slot stride of a captured step depend on it)
    // (deny: the step's logits launch reads the deny mask, whisper_state::deny_on: the pointer, or null, is a kernel
    // argument)
    // (gram, gram_pen: the logits launch reads the grammar's reject words, whisper_state::gram_on, and the penalty is a
    // kernel argument)
    // (filt: the call has a logits_filter_callback, whisper_state::filter_on: the graph ends with the stage kernel, and the
    // rest of the step follows the callbacks as plain launches; tdrz: tdrz_enable, the VocabIds argument keeps solm)
    struct DecGraph { int n_tok, n_rows, mask; bool direct; int sig; int pdec; int gen; int par; int beam; hipGraphExec_t exec; std::vector<KPending> ev; uint64_t seed = 0; int actx = 0; bool deny = false; bool gram = false; float gram_pen = 0.0f; bool filt = false; bool tdrz = false; };
    std::vector<DecGraph> dec_graphs;
    std::vector<KPending>* capture_ev = nullptr;  // non-null while a decode step is being captured
    double cur_self_work = 0;                     // self-attention bytes of the current step
    whisper_state* twin = nullptr;                // second half of a paired batch (full_batch)
    // persistent launches of this state that gave up (a wait timed out: not all 256 workgroups resident, e.g.
    // beside another process's kernels) and were re-run on the per-kernel path; after one, the state's steps
    // take the per-kernel path for kPdecBackoffMs (pdec_off) instead of paying the timeout on every step
    long pdec_give_ups = 0;
    double pdec_lost_ms = 0;    // wall time of the given-up launches (wait until give-up + the re-run)
    double pdec_off_until = 0;  // now_ms() clock
    bool pdec_off = false;      // the backoff as frozen once per step (dec_path_prepare), so its plan, graph and step_variant agree
    // the mode of the step that is running (a beam step, a sampled step, the prefill's top-k pass); set by
    // engine.cpp's ModeScope for that step only
    wm::StepMode mode;
    // the current call has a deny mask (suppress_nst or suppress_regex is set): its logits launches read ws.deny
    bool deny_on = false;
    // the current call has a grammar (whisper_full_params.grammar_rules): its flat rules, its penalty; its
    // logits launches read ws.gram (the rows' counters are in ws.gd: whisper_mi355x_grammar_stats)
    bool gram_on = false;
    wm::GrammarRules gram_rules;
    float gram_penalty = 0.0f;
    // the current call has a logits_filter_callback: a logits launch is the stage kernel, and the
    // prefiltered form follows the callbacks (engine.cpp logits_finish); tdrz_on: tdrz_enable, solm is not suppressed
    bool filter_on = false, tdrz_on = false;
    // beam_info[job] = the beams of the job's last beam-searched window (whisper_mi355x_beam_info)
    struct BeamRec { std::vector<int> tokens; double sum_logprobs_all = 0; int flags = 0; };
    std::vector<std::vector<BeamRec>> beam_info;
    // sampled attempts with best_of > 1 candidates. sample_seed: the draws' Philox key; cand_info[job]
    // = the candidates of the job's last such attempt (whisper_mi355x_cand_info).
    uint64_t sample_seed = 0;
    std::vector<std::vector<BeamRec>> cand_info;
    // cache rows the gather moved since the state was created, and what whole-sequence copies would have moved
    double gather_rows = 0, gather_rows_full = 0;
};

struct whisper_context {
    wm::Context c;
};

namespace wm {
// encoder positions per window of the state's current value (whisper.cpp: exp_n_audio_ctx > 0 ? it : n_audio_ctx)
inline int enc_ctx(const Context* c, const whisper_state* s) { return s->audio_ctx > 0 ? s->audio_ctx : c->hp.n_audio_ctx; }
bool load_context(Context* c, const char* path, int device, DType dt, bool load_weights);
void free_context(Context* c);
whisper_state* new_state(Context* c);
void free_state(whisper_state* s);
// after an engine error (wm::Error) mid-call: end a half-done graph capture, drain both streams and
// return pending timing events, so that the state and its context stay usable
void recover_state(whisper_state* s);
// frees the states kept in the context's pool (whisper_free)
void drain_state_pool(Context* c);
void orphan_states(Context* c);
// alignment heads of a context from its whisper_context_params; false (one stderr line) when the
// configuration is invalid for the model
bool resolve_dtw(Context* c, const whisper_context_params& cp);

struct FullOpts {
    int fixed_tokens = 0;
    // teacher forcing (fixed-work mode only; a parity-test hook): the token chosen at step i of job j is
    // replaced by forced[j * fixed_tokens + i] after the logits rules ran, so every later step decodes
    // the given sequence through the same kernels; the raw logits of jobs spot[0..n_spot) are copied
    // to spot_logits[(i * n_spot + k) * n_vocab] at every step i (prefill = step 0)
    const int* forced = nullptr;
    const int* spot = nullptr;
    int n_spot = 0;
    float* spot_logits = nullptr;
    // whisper_full_parallel (full_parallel below): the jobs are the pieces of one recording. Every job but
    // the single API's (job 0 of a call with single_api) decodes from its own time 0 (offset_ms = 0), and
    // encoder_begin_callback is asked for every job. stopped (if given): set when a callback ended the call early.
    bool pieces = false;
    bool* stopped = nullptr;
};
// whisper_full over n_jobs clips. With single_api, job 0 is the single API's job: it runs on the state's own
// prompt_past / rng and has the new-segment and progress callbacks (one clip: whisper_full_with_state); every other clip
// is decoded as on a fresh state.
// tokens decoded by every whisper_full / full_batch call of the process (whisper_mi355x_decoded_tokens_total)
extern std::atomic<long> g_decoded_tokens_total;
int full_batch(Context* c, whisper_state* s, const whisper_full_params& p, const float* const* pcm, const int* n,
               int n_jobs, bool on_device, const FullOpts& o, bool single_api);
// whisper_full_parallel / whisper_mi355x_full_parallel: the recording cut into n_processors pieces
// (parallel.h; snap_ms > 0 moves each cut to the quietest 20 ms near it), the pieces decoded as the jobs of one scheduler
// (beam search: in groups of 32 / beam_size), their results merged into results[0] of the state on the recording's axis.
int full_parallel(Context* c, whisper_state* s, const whisper_full_params& p, const float* pcm, int n_samples,
                  int n_processors, int snap_ms, bool on_device);
// The deny mask of (suppress_nst, regex) from the context's one-entry cache, built when the key differs: 0 and the
// words in `words` (if given), or -8 and one stderr line when the pattern does not compile. Host only.
int deny_lookup(Context* c, bool suppress_nst, const char* regex, std::vector<uint32_t>* words);
// The call's grammar fields validated and flattened (grammar.h): 0 (rules off when the call has no grammar), or -9 and
// one stderr line. Host only.
int grammar_check(const whisper_full_params& p, GrammarRules& rules);
// The context's VAD model for `path` (loaded on first use, or when the path changes): null and one stderr line when the
// path is null or the file is unreadable or refused (whisper_full* then returns -11).
std::shared_ptr<VadModel> vad_lookup(Context* c, const char* path);
// the context's decoded vocabulary, built on first use
const GramVocab& gram_vocab(Context* c);

// pieces exposed for whisper.h's low-level API
int compute_mel(Context* c, whisper_state* s, const float* const* pcm, const int* n, int n_jobs, bool on_device);
int encode_windows(Context* c, whisper_state* s, const int* jobs, const int* seeks, const int* slots, int n_win);
int decode_tokens(Context* c, whisper_state* s, const int* tokens, const int* pos, const int* slots, int n_tok,
                  const int* logit_rows, int n_logit_rows);
// whisper_lang_auto_detect_with_state's ranking of a row's 100 language logits: {logit, language id}, best first
// (std::sort over the languages in code order, as whisper.cpp: equal logits resolve as there)
std::vector<std::pair<float, int>> rank_languages(const float* logits);
}  // namespace wm
