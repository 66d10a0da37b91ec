// extern "C" whisper.h entry points (include/whisper.h) and the MI355X extensions
// (include/whisper_mi355x.h). See include/whisper.h for the whisper.rs call site of each.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/whisper_mi355x.h"
#include "engine.h"
#include "suppress.h"

namespace wm { extern int g_gemm_variant; extern int g_dec_splits; extern int g_dec_bm; extern unsigned long long* g_gemm_stamps; }
using namespace wm;

static Context* C(whisper_context* ctx) { return ctx ? &ctx->c : nullptr; }

// Engine errors (wm::Error: a HIP error such as out of memory, an unsupported shape) end the call
// with WHISPER_MI355X_ERR_RUNTIME and leave the context and the state usable; whisper-rs turns the
// non-zero return into WhisperError (whisper.rs:127-129) and the app logs and skips the chunk
// (state.rs:157-159).
template <typename F> static int guarded(whisper_state* s, F&& f) {
    try {
        return f();
    } catch (const wm::Error&) {
    } catch (const std::bad_alloc&) {
        fprintf(stderr, "whisper_mi355x: host out of memory\n");
    }
    if (s) recover_state(s);
    return WHISPER_MI355X_ERR_RUNTIME;
}

// ---- what the kernel-level hooks below own: released also when a launcher refuses the shape (WM_FAIL throws) ----
struct HookStream {
    hipStream_t st = nullptr;
    HookStream() { WM_CHECK(hipStreamCreate(&st)); }
    ~HookStream() { hipStreamDestroy(st); }
};
struct HookBufs {  // device buffers
    std::vector<void*> p;
    void* get(size_t bytes) {
        void* q = nullptr;
        WM_CHECK(hipMalloc(&q, bytes));
        p.push_back(q);
        return q;
    }
    ~HookBufs() { for (void* q : p) hipFree(q); }
};
struct HookEvent {
    hipEvent_t e = nullptr;
    HookEvent() { WM_CHECK(hipEventCreate(&e)); }
    ~HookEvent() { hipEventDestroy(e); }
};
// `run` reps times on the stream between two events: the average ms per run, 0 at reps == 0; warm: one run
// before the first event
template <typename F> static float timed_ms(hipStream_t st, int reps, bool warm, F run) {
    HookEvent e0, e1;
    if (warm) run();
    WM_CHECK(hipEventRecord(e0.e, st));
    for (int r = 0; r < reps; r++) run();
    WM_CHECK(hipEventRecord(e1.e, st));
    WM_CHECK(hipStreamSynchronize(st));
    float t = 0;
    WM_CHECK(hipEventElapsedTime(&t, e0.e, e1.e));
    return reps > 0 ? t / reps : 0.0f;
}

static DType env_dtype(DType def) {
    const char* e = getenv("WHISPER_MI355X_DTYPE");
    if (!e) return def;
    return (strcmp(e, "bf16") == 0 || strcmp(e, "BF16") == 0) ? DType::BF16 : DType::F16;
}

static whisper_context* make_ctx(const char* path, whisper_context_params cp, int dtype, bool load) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
        fprintf(stderr, "whisper_mi355x: no HIP device available (this engine has no CPU path)\n");
        return nullptr;
    }
    const int dev = cp.gpu_device >= 0 && cp.gpu_device < n_dev ? cp.gpu_device : 0;
    whisper_context* w = new whisper_context();
    // dtype 2 = bf16 with the fp8 encoder GEMMs (large-v3-turbo fp8 config)
    w->c.fp8_enc = dtype == 2;
    if (dtype == 2) dtype = (int)DType::BF16;
    bool ok = false;
    try {
        ok = load_context(&w->c, path, dev, (DType)dtype, load);
    } catch (const wm::Error&) {
    } catch (const std::bad_alloc&) {
    }
    if (!ok) {
        free_context(&w->c);
        delete w;
        return nullptr;
    }
    if (w->c.quant && w->c.fp8_enc) {  // the e4m3 weights are quantized from compute-type matrices
        fprintf(stderr, "whisper_mi355x: fp8 mode needs an f16 model file; %s is block-quantized, fp8 off\n", path);
        w->c.fp8_enc = false;
    }
    if (!resolve_dtw(&w->c, cp)) {  // (one stderr line said why)
        free_context(&w->c);
        delete w;
        return nullptr;
    }
    w->c.owner = w;
    return w;
}

extern "C" {

const char* whisper_version(void) { return "1.7.6-mi355x"; }

struct whisper_context_params whisper_context_default_params(void) {
    whisper_context_params r;
    memset(&r, 0, sizeof(r));
    r.use_gpu = true;
    r.flash_attn = false;
    r.gpu_device = 0;
    r.dtw_token_timestamps = false;
    r.dtw_aheads_preset = WHISPER_AHEADS_NONE;
    r.dtw_n_top = -1;
    r.dtw_aheads.n_heads = 0;
    r.dtw_aheads.heads = nullptr;
    r.dtw_mem_size = 1024 * 1024 * 128;
    return r;
}
struct whisper_context_params* whisper_context_default_params_by_ref(void) {
    return new whisper_context_params(whisper_context_default_params());
}
void whisper_free_context_params(struct whisper_context_params* p) { delete p; }

struct whisper_full_params whisper_full_default_params(enum whisper_sampling_strategy strategy) {
    whisper_full_params r;
    memset(&r, 0, sizeof(r));
    r.strategy = strategy;
    r.n_threads = std::min(4, (int)std::thread::hardware_concurrency());
    r.n_max_text_ctx = 16384;
    r.offset_ms = 0;
    r.duration_ms = 0;
    r.translate = false;
    r.no_context = true;
    r.no_timestamps = false;
    r.single_segment = false;
    r.print_special = false;
    r.print_progress = true;
    r.print_realtime = false;
    r.print_timestamps = true;
    r.token_timestamps = false;
    r.thold_pt = 0.01f;
    r.thold_ptsum = 0.01f;
    r.max_len = 0;
    r.split_on_word = false;
    r.max_tokens = 0;
    r.debug_mode = false;
    r.audio_ctx = 0;
    r.tdrz_enable = false;
    r.suppress_regex = nullptr;
    r.initial_prompt = nullptr;
    r.prompt_tokens = nullptr;
    r.prompt_n_tokens = 0;
    r.language = "en";
    r.detect_language = false;
    r.suppress_blank = true;
    r.suppress_nst = false;
    r.temperature = 0.0f;
    r.max_initial_ts = 1.0f;
    r.length_penalty = -1.0f;
    r.temperature_inc = 0.2f;
    r.entropy_thold = 2.4f;
    r.logprob_thold = -1.0f;
    r.no_speech_thold = 0.6f;
    r.greedy.best_of = -1;
    r.beam_search.beam_size = -1;
    r.beam_search.patience = -1.0f;
    r.grammar_penalty = 100.0f;
    r.vad = false;
    r.vad_model_path = nullptr;
    r.vad_params.threshold = 0.5f;
    r.vad_params.min_speech_duration_ms = 250;
    r.vad_params.min_silence_duration_ms = 100;
    r.vad_params.max_speech_duration_s = INFINITY;
    r.vad_params.speech_pad_ms = 30;
    r.vad_params.samples_overlap = 0.1f;
    if (strategy == WHISPER_SAMPLING_GREEDY) r.greedy.best_of = 5;
    else { r.beam_search.beam_size = 5; r.beam_search.patience = -1.0f; }
    return r;
}
struct whisper_full_params* whisper_full_default_params_by_ref(enum whisper_sampling_strategy s) {
    return new whisper_full_params(whisper_full_default_params(s));
}
void whisper_free_params(struct whisper_full_params* p) { delete p; }

// ---- init / free ----------------------------------------------------------------------------------
struct whisper_context* whisper_init_from_file_with_params_no_state(const char* path, struct whisper_context_params p) {
    return make_ctx(path, p, (int)env_dtype(DType::F16), true);
}
struct whisper_context* whisper_init_from_file_with_params(const char* path, struct whisper_context_params p) {
    whisper_context* w = whisper_init_from_file_with_params_no_state(path, p);
    if (w) w->c.default_state = whisper_init_state(w);
    if (w && !w->c.default_state) { whisper_free(w); return nullptr; }
    return w;
}
struct whisper_context* whisper_init_from_buffer_with_params_no_state(void*, size_t, struct whisper_context_params) {
    fprintf(stderr, "whisper_mi355x: init from buffer is not supported; use a model file\n");
    return nullptr;
}
struct whisper_context* whisper_init_from_buffer_with_params(void* b, size_t n, struct whisper_context_params p) {
    return whisper_init_from_buffer_with_params_no_state(b, n, p);
}
struct whisper_context* whisper_init_with_params_no_state(struct whisper_model_loader*, struct whisper_context_params) {
    fprintf(stderr, "whisper_mi355x: custom model loaders are not supported; use a model file\n");
    return nullptr;
}
struct whisper_context* whisper_init_with_params(struct whisper_model_loader* l, struct whisper_context_params p) {
    return whisper_init_with_params_no_state(l, p);
}
struct whisper_state* whisper_init_state(struct whisper_context* ctx) {
    if (!ctx) return nullptr;
    whisper_state* s = nullptr;
    guarded(nullptr, [&] { s = new_state(&ctx->c); return 0; });
    return s;
}
int whisper_ctx_init_openvino_encoder_with_state(struct whisper_context*, struct whisper_state*, const char*, const char*, const char*) { return 1; }
int whisper_ctx_init_openvino_encoder(struct whisper_context*, const char*, const char*, const char*) { return 1; }
void whisper_free_state(struct whisper_state* s) { free_state(s); }
void whisper_free(struct whisper_context* ctx) {
    if (!ctx) return;
    if (ctx->c.default_state) free_state(ctx->c.default_state);
    ctx->c.default_state = nullptr;
    drain_state_pool(&ctx->c);
    orphan_states(&ctx->c);  // states the caller still holds stay valid to whisper_free_state
    free_context(&ctx->c);  // weight arena + the fp8 arena
    delete ctx;
}

// ---- mel / encode / decode ------------------------------------------------------------------------
int whisper_pcm_to_mel_with_state(struct whisper_context* ctx, struct whisper_state* s, const float* samples, int n, int) {
    if (!ctx || !s) return -1;
    hipSetDevice(ctx->c.device);
    const float* pp[1] = {samples};
    int nn[1] = {n};
    return guarded(s, [&] { return compute_mel(&ctx->c, s, pp, nn, 1, false); });
}
int whisper_pcm_to_mel(struct whisper_context* ctx, const float* samples, int n, int t) {
    return whisper_pcm_to_mel_with_state(ctx, ctx ? ctx->c.default_state : nullptr, samples, n, t);
}
int whisper_set_mel_with_state(struct whisper_context*, struct whisper_state*, const float*, int, int) {
    fprintf(stderr, "whisper_mi355x: whisper_set_mel is not supported (mel is computed on device)\n");
    return -1;
}
int whisper_set_mel(struct whisper_context* ctx, const float* d, int n, int m) { return whisper_set_mel_with_state(ctx, nullptr, d, n, m); }
int whisper_encode_with_state(struct whisper_context* ctx, struct whisper_state* s, int offset, int) {
    if (!ctx || !s || !s->mel_ready) return -1;
    hipSetDevice(ctx->c.device);
    int job = 0, slot = 0;
    return guarded(s, [&] { return encode_windows(&ctx->c, s, &job, &offset, &slot, 1); });
}
int whisper_encode(struct whisper_context* ctx, int offset, int t) {
    return whisper_encode_with_state(ctx, ctx ? ctx->c.default_state : nullptr, offset, t);
}
int whisper_decode_with_state(struct whisper_context* ctx, struct whisper_state* s, const whisper_token* tokens, int n_tokens,
                              int n_past, int) {
    if (!ctx || !s || !s->mel_ready || n_tokens <= 0) return -1;
    if (n_past + n_tokens > ctx->c.hp.n_text_ctx) return -1;
    hipSetDevice(ctx->c.device);
    std::vector<int> pos(n_tokens), slot(n_tokens, 0);
    for (int i = 0; i < n_tokens; i++) pos[i] = n_past + i;
    int row = n_tokens - 1;
    return guarded(s, [&] {
        if (decode_tokens(&ctx->c, s, tokens, pos.data(), slot.data(), n_tokens, &row, 1) != 0) return -1;
        const int V = ctx->c.hp.n_vocab;
        s->logits_host.assign((size_t)n_tokens * V, 0.0f);
        WM_CHECK(hipMemcpyAsync(s->logits_host.data() + (size_t)(n_tokens - 1) * V, s->ws.logits, (size_t)V * 4,
                                hipMemcpyDeviceToHost, s->stream));
        WM_CHECK(hipStreamSynchronize(s->stream));
        return 0;
    });
}
int whisper_decode(struct whisper_context* ctx, const whisper_token* t, int n, int n_past, int th) {
    return whisper_decode_with_state(ctx, ctx ? ctx->c.default_state : nullptr, t, n, n_past, th);
}
float* whisper_get_logits_from_state(struct whisper_state* s) { return s ? s->logits_host.data() : nullptr; }
float* whisper_get_logits(struct whisper_context* ctx) {
    return ctx && ctx->c.default_state ? ctx->c.default_state->logits_host.data() : nullptr;
}

// ---- tokens / languages ---------------------------------------------------------------------------
int whisper_tokenize(struct whisper_context* ctx, const char* text, whisper_token* tokens, int n_max) {
    if (!ctx || !text) return -1;
    std::vector<int> t = tokenize(ctx->c.vocab, text);
    if (n_max < (int)t.size()) return -(int)t.size();
    for (size_t i = 0; i < t.size(); i++) tokens[i] = t[i];
    return (int)t.size();
}
int whisper_token_count(struct whisper_context* ctx, const char* text) { return -whisper_tokenize(ctx, text, nullptr, 0); }
int whisper_lang_max_id(void) { return 99; }
int whisper_lang_id(const char* lang) { return lang_index(lang); }
const char* whisper_lang_str(int id) { return id >= 0 && id < 100 ? k_lang_codes[id] : nullptr; }
const char* whisper_lang_str_full(int id) { return id >= 0 && id < 100 ? k_lang_names[id] : nullptr; }
int whisper_lang_auto_detect_with_state(struct whisper_context* ctx, struct whisper_state* s, int offset_ms, int, float* probs) {
    if (!ctx || !s || !s->mel_ready) return -1;
    const int seek = offset_ms / 10;
    if (seek < 0 || seek >= s->n_len_org) return -2;
    hipSetDevice(ctx->c.device);
    int job = 0, slot = 0;
    const Vocab& v = ctx->c.vocab;
    std::vector<float> lg(100);
    const int rc = guarded(s, [&] {
        if (encode_windows(&ctx->c, s, &job, &seek, &slot, 1) != 0) return -6;
        int tok = v.token_sot, pos = 0, row = 0;
        if (decode_tokens(&ctx->c, s, &tok, &pos, &slot, 1, &row, 1) != 0) return -7;
        // on the state's stream (it does not synchronise with the null stream: a plain hipMemcpy could read the row
        // before the pass has written it)
        WM_CHECK(hipMemcpyAsync(lg.data(), s->ws.logits + v.token_sot + 1, 100 * 4, hipMemcpyDeviceToHost, s->stream));
        WM_CHECK(hipStreamSynchronize(s->stream));
        return 0;
    });
    if (rc != 0) return rc;
    std::vector<std::pair<float, int>> ids = rank_languages(lg.data());
    const float mx = ids[0].first;
    double sum = 0.0;
    for (auto& kv : ids) { kv.first = exp(kv.first - mx); sum += kv.first; }
    for (auto& kv : ids) kv.first /= sum;
    if (probs) for (auto& kv : ids) probs[kv.second] = kv.first;
    return ids[0].second;
}
int whisper_lang_auto_detect(struct whisper_context* ctx, int offset_ms, int t, float* probs) {
    return whisper_lang_auto_detect_with_state(ctx, ctx ? ctx->c.default_state : nullptr, offset_ms, t, probs);
}

int whisper_n_len_from_state(struct whisper_state* s) { return s ? s->n_len_org : 0; }
int whisper_n_len(struct whisper_context* ctx) { return ctx && ctx->c.default_state ? ctx->c.default_state->n_len_org : 0; }
int whisper_n_vocab(struct whisper_context* ctx) { return ctx->c.vocab.n_vocab; }
int whisper_n_text_ctx(struct whisper_context* ctx) { return ctx->c.hp.n_text_ctx; }
int whisper_n_audio_ctx(struct whisper_context* ctx) { return ctx->c.hp.n_audio_ctx; }
int whisper_is_multilingual(struct whisper_context* ctx) { return ctx->c.vocab.is_multilingual() ? 1 : 0; }
int whisper_model_n_vocab(struct whisper_context* ctx) { return ctx->c.hp.n_vocab; }
int whisper_model_n_audio_ctx(struct whisper_context* ctx) { return ctx->c.hp.n_audio_ctx; }
int whisper_model_n_audio_state(struct whisper_context* ctx) { return ctx->c.hp.n_audio_state; }
int whisper_model_n_audio_head(struct whisper_context* ctx) { return ctx->c.hp.n_audio_head; }
int whisper_model_n_audio_layer(struct whisper_context* ctx) { return ctx->c.hp.n_audio_layer; }
int whisper_model_n_text_ctx(struct whisper_context* ctx) { return ctx->c.hp.n_text_ctx; }
int whisper_model_n_text_state(struct whisper_context* ctx) { return ctx->c.hp.n_text_state; }
int whisper_model_n_text_head(struct whisper_context* ctx) { return ctx->c.hp.n_text_head; }
int whisper_model_n_text_layer(struct whisper_context* ctx) { return ctx->c.hp.n_text_layer; }
int whisper_model_n_mels(struct whisper_context* ctx) { return ctx->c.hp.n_mels; }
int whisper_model_ftype(struct whisper_context* ctx) { return ctx->c.hp.ftype; }
int whisper_model_type(struct whisper_context* ctx) {
    const int L = ctx->c.hp.n_audio_layer;
    return L == 4 ? 1 : L == 6 ? 2 : L == 12 ? 3 : L == 24 ? 4 : 5;
}
const char* whisper_model_type_readable(struct whisper_context* ctx) { return ctx->c.model_type.c_str(); }

const char* whisper_token_to_str(struct whisper_context* ctx, whisper_token t) {
    if (!ctx || t < 0 || t >= (int)ctx->c.vocab.id_to_token.size()) return nullptr;
    return ctx->c.vocab.id_to_token[t].c_str();
}
whisper_token whisper_token_eot(struct whisper_context* ctx) { return ctx->c.vocab.token_eot; }
whisper_token whisper_token_sot(struct whisper_context* ctx) { return ctx->c.vocab.token_sot; }
whisper_token whisper_token_solm(struct whisper_context* ctx) { return ctx->c.vocab.token_solm; }
whisper_token whisper_token_prev(struct whisper_context* ctx) { return ctx->c.vocab.token_prev; }
whisper_token whisper_token_nosp(struct whisper_context* ctx) { return ctx->c.vocab.token_nosp; }
whisper_token whisper_token_not(struct whisper_context* ctx) { return ctx->c.vocab.token_not; }
whisper_token whisper_token_beg(struct whisper_context* ctx) { return ctx->c.vocab.token_beg; }
whisper_token whisper_token_lang(struct whisper_context* ctx, int id) { return ctx->c.vocab.token_sot + 1 + id; }
whisper_token whisper_token_translate(struct whisper_context* ctx) { return ctx->c.vocab.token_translate; }
whisper_token whisper_token_transcribe(struct whisper_context* ctx) { return ctx->c.vocab.token_transcribe; }

struct whisper_timings* whisper_get_timings(struct whisper_context* ctx) { return ctx ? &ctx->c.timings : nullptr; }
void whisper_print_timings(struct whisper_context* ctx) {
    if (!ctx) return;
    const whisper_timings& t = ctx->c.timings;
    fprintf(stderr, "whisper_mi355x: encode %.2f ms, prompt %.2f ms, decode %.2f ms\n", t.encode_ms, t.prompt_ms, t.decode_ms);
}
void whisper_reset_timings(struct whisper_context* ctx) { if (ctx) ctx->c.timings = whisper_timings{}; }
const char* whisper_print_system_info(void) { return "HIP = 1 | gfx950 | MFMA = 1 | RCCL = 1 | "; }

// ---- full ----------------------------------------------------------------------------------------
int whisper_full_with_state(struct whisper_context* ctx, struct whisper_state* s, struct whisper_full_params p,
                            const float* samples, int n_samples) {
    if (!ctx || !s) return -1;
    const float* pp[1] = {samples};
    int nn[1] = {n_samples};
    FullOpts o;
    return guarded(s, [&] { return full_batch(&ctx->c, s, p, pp, nn, 1, false, o, true); });
}
int whisper_full(struct whisper_context* ctx, struct whisper_full_params p, const float* samples, int n) {
    return whisper_full_with_state(ctx, ctx ? ctx->c.default_state : nullptr, p, samples, n);
}
// the pieces of the recording as the jobs of one device batch, merged on the recording's axis
int whisper_mi355x_full_parallel(struct whisper_context* ctx, struct whisper_state* s, struct whisper_full_params p,
                                 const float* pcm, int n_samples, int n_processors, int snap_ms, bool pcm_on_device) {
    if (n_processors > kParallelMax) {  // the clips of one scheduler (asked before anything else: no device is needed)
        fprintf(stderr, "whisper_mi355x: whisper_full_parallel: n_processors %d > %d\n", n_processors, kParallelMax);
        return -1;
    }
    if (!ctx || !s || n_samples < 0 || (!pcm && n_samples > 0)) return -1;
    return guarded(s, [&] { return full_parallel(&ctx->c, s, p, pcm, n_samples, n_processors, snap_ms, pcm_on_device); });
}
int whisper_mi355x_parallel_cuts(struct whisper_state* s, int* cuts, int cap) {
    if (!s) return 0;
    for (int k = 0; cuts && k < cap && k < (int)s->par_cuts.size(); k++) cuts[k] = s->par_cuts[k];
    return (int)s->par_cuts.size();
}
int whisper_full_parallel(struct whisper_context* ctx, struct whisper_full_params p, const float* samples, int n, int n_processors) {
    return whisper_mi355x_full_parallel(ctx, ctx ? ctx->c.default_state : nullptr, p, samples, n, n_processors, 0, false);
}

static const Segment* seg(whisper_state* s, int job, int i) {
    if (!s || job < 0 || job >= (int)s->results.size() || i < 0 || i >= (int)s->results[job].size()) return nullptr;
    return &s->results[job][i];
}
int whisper_full_n_segments_from_state(struct whisper_state* s) { return s && !s->results.empty() ? (int)s->results[0].size() : 0; }
int whisper_full_n_segments(struct whisper_context* ctx) { return whisper_full_n_segments_from_state(ctx ? ctx->c.default_state : nullptr); }
int whisper_full_lang_id_from_state(struct whisper_state* s) { return s ? s->lang_id : -1; }
int whisper_full_lang_id(struct whisper_context* ctx) { return whisper_full_lang_id_from_state(ctx ? ctx->c.default_state : nullptr); }
int64_t whisper_full_get_segment_t0_from_state(struct whisper_state* s, int i) { auto g = seg(s, 0, i); return g ? g->t0 : 0; }
int64_t whisper_full_get_segment_t0(struct whisper_context* ctx, int i) { return whisper_full_get_segment_t0_from_state(ctx->c.default_state, i); }
int64_t whisper_full_get_segment_t1_from_state(struct whisper_state* s, int i) { auto g = seg(s, 0, i); return g ? g->t1 : 0; }
int64_t whisper_full_get_segment_t1(struct whisper_context* ctx, int i) { return whisper_full_get_segment_t1_from_state(ctx->c.default_state, i); }
bool whisper_full_get_segment_speaker_turn_next_from_state(struct whisper_state* s, int i) { auto g = seg(s, 0, i); return g && g->speaker_turn_next; }
bool whisper_full_get_segment_speaker_turn_next(struct whisper_context* ctx, int i) { return whisper_full_get_segment_speaker_turn_next_from_state(ctx->c.default_state, i); }
const char* whisper_full_get_segment_text_from_state(struct whisper_state* s, int i) { auto g = seg(s, 0, i); return g ? g->text.c_str() : nullptr; }
const char* whisper_full_get_segment_text(struct whisper_context* ctx, int i) { return whisper_full_get_segment_text_from_state(ctx->c.default_state, i); }
int whisper_full_n_tokens_from_state(struct whisper_state* s, int i) { auto g = seg(s, 0, i); return g ? (int)g->tokens.size() : 0; }
int whisper_full_n_tokens(struct whisper_context* ctx, int i) { return whisper_full_n_tokens_from_state(ctx->c.default_state, i); }
const char* whisper_full_get_token_text_from_state(struct whisper_context* ctx, struct whisper_state* s, int i, int t) {
    auto g = seg(s, 0, i);
    if (!g || t < 0 || t >= (int)g->tokens.size()) return nullptr;
    return whisper_token_to_str(ctx, g->tokens[t].id);
}
const char* whisper_full_get_token_text(struct whisper_context* ctx, int i, int t) {
    return whisper_full_get_token_text_from_state(ctx, ctx->c.default_state, i, t);
}
whisper_token whisper_full_get_token_id_from_state(struct whisper_state* s, int i, int t) {
    auto g = seg(s, 0, i);
    return g && t >= 0 && t < (int)g->tokens.size() ? g->tokens[t].id : -1;
}
whisper_token whisper_full_get_token_id(struct whisper_context* ctx, int i, int t) { return whisper_full_get_token_id_from_state(ctx->c.default_state, i, t); }
static whisper_token_data tdata(const Segment* g, int t) {
    whisper_token_data r;
    memset(&r, 0, sizeof(r));
    if (!g || t < 0 || t >= (int)g->tokens.size()) { r.id = -1; return r; }
    return token_data(g->tokens[t]);
}
whisper_token_data whisper_full_get_token_data_from_state(struct whisper_state* s, int i, int t) { return tdata(seg(s, 0, i), t); }
whisper_token_data whisper_full_get_token_data(struct whisper_context* ctx, int i, int t) { return tdata(seg(ctx->c.default_state, 0, i), t); }
float whisper_full_get_token_p_from_state(struct whisper_state* s, int i, int t) { return tdata(seg(s, 0, i), t).p; }
float whisper_full_get_token_p(struct whisper_context* ctx, int i, int t) { return tdata(seg(ctx->c.default_state, 0, i), t).p; }
float whisper_full_get_segment_no_speech_prob_from_state(struct whisper_state* s, int i) { auto g = seg(s, 0, i); return g ? g->no_speech_prob : 0.0f; }
float whisper_full_get_segment_no_speech_prob(struct whisper_context* ctx, int i) { return whisper_full_get_segment_no_speech_prob_from_state(ctx->c.default_state, i); }

int whisper_bench_memcpy(int) { return 0; }
const char* whisper_bench_memcpy_str(int) { return "whisper_mi355x: memcpy benchmark not implemented\n"; }
int whisper_bench_ggml_mul_mat(int) { return 0; }
const char* whisper_bench_ggml_mul_mat_str(int) { return "whisper_mi355x: ggml mul_mat benchmark not applicable (no ggml)\n"; }
void whisper_log_set(ggml_log_callback, void*) {}

// ---- MI355X extensions -----------------------------------------------------------------------------
struct whisper_context* whisper_mi355x_init(const char* path, struct whisper_context_params p, int dtype, bool load) {
    return make_ctx(path, p, dtype, load);
}
int whisper_mi355x_weight_arena(struct whisper_context* ctx, void** ptr, size_t* bytes) {
    if (!ctx) return -1;
    *ptr = ctx->c.arena;
    *bytes = ctx->c.arena_bytes;
    return 0;
}
int whisper_mi355x_rccl_unique_id(char out[128]) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return -1;
    static_assert(sizeof(id) == 128, "ncclUniqueId size");
    memcpy(out, &id, 128);
    return 0;
}
// One ncclBroadcast of the packed weight arena from rank 0 over xGMI.
int whisper_mi355x_broadcast_weights(struct whisper_context* ctx, const char uid[128], int rank, int world) {
    if (!ctx) return -1;
    if (world <= 1) return 0;
    hipSetDevice(ctx->c.device);
    ncclUniqueId id;
    memcpy(&id, uid, 128);
    ncclComm_t comm;
    if (ncclCommInitRank(&comm, world, id, rank) != ncclSuccess) return -2;
    hipStream_t st = nullptr;
    ncclResult_t r = ncclInternalError;
    const int rc = guarded(nullptr, [&] {
        WM_CHECK(hipStreamCreate(&st));
        r = ncclBroadcast(ctx->c.arena, ctx->c.arena, ctx->c.arena_bytes, ncclChar, 0, comm, st);
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
    if (st) hipStreamDestroy(st);
    ncclCommDestroy(comm);
    if (rc != 0) return rc;
    return r == ncclSuccess ? 0 : -3;
}

int whisper_mi355x_full_batch(struct whisper_context* ctx, struct whisper_state* s, struct whisper_full_params p,
                              const float* const* pcm, const int* n, int n_jobs, bool on_device, int fixed_tokens) {
    // fixed work decodes at most a window's n_max = n_text_ctx / 2 - 4 tokens (whisper.cpp's limit: a 229-token
    // prompt + 220 tokens ends at the last self-cache row)
    if (!ctx || !s || n_jobs <= 0 || fixed_tokens > ctx->c.hp.n_text_ctx / 2 - 4) return -1;
    FullOpts o;
    o.fixed_tokens = fixed_tokens;
    return guarded(s, [&] { return full_batch(&ctx->c, s, p, pcm, n, n_jobs, on_device, o, false); });
}
int whisper_mi355x_full_batch_forced(struct whisper_context* ctx, struct whisper_state* s, struct whisper_full_params p,
                                     const float* const* pcm, const int* n, int n_jobs, bool on_device, int fixed_tokens,
                                     const int* forced, const int* spot, int n_spot, float* spot_logits) {
    if (!ctx || !s || n_jobs <= 0 || fixed_tokens <= 0 || fixed_tokens > ctx->c.hp.n_text_ctx / 2 - 4 || !forced || n_spot < 0 ||
        (n_spot && (!spot || !spot_logits)))
        return -1;
    for (int k = 0; k < n_spot; k++)
        if (spot[k] < 0 || spot[k] >= n_jobs) return -1;
    FullOpts o;
    o.fixed_tokens = fixed_tokens;
    o.forced = forced;
    o.spot = spot;
    o.n_spot = n_spot;
    o.spot_logits = spot_logits;
    return guarded(s, [&] { return full_batch(&ctx->c, s, p, pcm, n, n_jobs, on_device, o, false); });
}
int whisper_mi355x_beam_info(struct whisper_state* s, int job, int beam, int* tokens, int cap, double* sum_logprobs_all,
                             int* flags) {
    if (!s || job < 0 || job >= (int)s->beam_info.size() || beam < 0 || beam >= (int)s->beam_info[job].size()) return -1;
    const whisper_state::BeamRec& r = s->beam_info[job][beam];
    for (int i = 0; tokens && i < cap && i < (int)r.tokens.size(); i++) tokens[i] = r.tokens[i];
    if (sum_logprobs_all) *sum_logprobs_all = r.sum_logprobs_all;
    if (flags) *flags = r.flags;
    return (int)r.tokens.size();
}
int whisper_mi355x_cand_info(struct whisper_state* s, int job, int cand, int* tokens, int cap, double* sum_logprobs_all,
                             int* flags) {
    if (!s || job < 0 || job >= (int)s->cand_info.size() || cand < 0 || cand >= (int)s->cand_info[job].size()) return -1;
    const whisper_state::BeamRec& r = s->cand_info[job][cand];
    for (int i = 0; tokens && i < cap && i < (int)r.tokens.size(); i++) tokens[i] = r.tokens[i];
    if (sum_logprobs_all) *sum_logprobs_all = r.sum_logprobs_all;
    if (flags) *flags = r.flags;
    return (int)r.tokens.size();
}
void whisper_mi355x_set_sample_seed(struct whisper_state* s, uint64_t seed) {
    if (s) s->sample_seed = seed;
}
int whisper_mi355x_batch_n_segments(struct whisper_state* s, int job) {
    return s && job >= 0 && job < (int)s->results.size() ? (int)s->results[job].size() : 0;
}
const char* whisper_mi355x_batch_segment_text(struct whisper_state* s, int job, int i) { auto g = seg(s, job, i); return g ? g->text.c_str() : nullptr; }
int64_t whisper_mi355x_batch_segment_t0(struct whisper_state* s, int job, int i) { auto g = seg(s, job, i); return g ? g->t0 : 0; }
int64_t whisper_mi355x_batch_segment_t1(struct whisper_state* s, int job, int i) { auto g = seg(s, job, i); return g ? g->t1 : 0; }
int whisper_mi355x_batch_segment_n_tokens(struct whisper_state* s, int job, int i) { auto g = seg(s, job, i); return g ? (int)g->tokens.size() : 0; }
whisper_token_data whisper_mi355x_batch_token_data(struct whisper_state* s, int job, int i, int t) { return tdata(seg(s, job, i), t); }
bool whisper_mi355x_batch_segment_speaker_turn_next(struct whisper_state* s, int job, int i) { auto g = seg(s, job, i); return g && g->speaker_turn_next; }
int whisper_mi355x_batch_lang_id(struct whisper_state* s, int job) {
    return s && job >= 0 && job < (int)s->lang_ids.size() ? s->lang_ids[job] : -1;
}
long whisper_mi355x_batch_decoded_tokens(struct whisper_state* s) { return s ? s->decoded_tokens : 0; }
int whisper_mi355x_window_decisions(struct whisper_state* s, int job, struct whisper_mi355x_window_decision* out, int cap) {
    if (!s || job < 0 || job >= (int)s->decisions.size()) return 0;
    const auto& d = s->decisions[job];
    if ((int)d.size() > cap) return -(int)d.size();
    for (size_t i = 0; i < d.size(); i++) out[i] = d[i];
    return (int)d.size();
}
int whisper_mi355x_phase_ms(struct whisper_state* s, double out[5]) {
    if (!s) return -1;
    for (int i = 0; i < 5; i++) out[i] = s->phase_ms[i];
    return 0;
}
double whisper_mi355x_align_ms(struct whisper_state* s) { return s ? s->align_ms : 0.0; }
int whisper_mi355x_align_cost(struct whisper_state* s, int job, float* out, long cap, int* rows, int* frames) {
    return guarded(nullptr, [&]() -> int {
        if (!s || job < 0 || job >= (int)s->align_info.size()) return -1;
        const whisper_state::AlignInfo& a = s->align_info[job];
        if (rows) *rows = a.rows;
        if (frames) *frames = a.frames;
        if (a.rows <= 0 || !a.cost) return 0;
        const long n = (long)a.rows * a.frames;
        if (!out || cap < n) return -2;
        hipSetDevice(s->device);
        WM_CHECK(hipMemcpy(out, a.cost, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    });
}
int whisper_mi355x_get_mel(struct whisper_state* s, float* out, int cap) {
    return guarded(nullptr, [&]() -> int {
        if (!s || !s->ctx || !s->ws.mel) return -1;  // orphan state: its context was freed
        Context* c = s->ctx;
        const int nm = c->hp.n_mels, nl = s->n_len;
        if ((long)nm * nl > cap) return -nm * nl;
        hipSetDevice(c->device);
        // recompute n_samples from n_len: n_len = (n + 480000) / 160 is not invertible; keep it via n_len_org
        int n_samp = 0;
        WM_CHECK(hipMemcpy(&n_samp, s->ws.n_samp, sizeof(int), hipMemcpyDeviceToHost));
        float* tmp;
        WM_CHECK(hipMalloc((void**)&tmp, (size_t)nm * nl * 4));
        launch_mel_normalize(s->ws.mel, nl, n_samp, s->ws.mel_max, nm, tmp, s->stream);
        WM_CHECK(hipMemcpyAsync(out, tmp, (size_t)nm * nl * 4, hipMemcpyDeviceToHost, s->stream));
        WM_CHECK(hipStreamSynchronize(s->stream));
        WM_CHECK(hipFree(tmp));
        return nl;
    });
}
int whisper_mi355x_get_encoder_out(struct whisper_state* s, float* out, int cap) {
    return guarded(nullptr, [&]() -> int {
        if (!s || !s->ctx || !s->ws.hn || s->last_enc_windows < 1) return -1;  // orphan state: -1
        Context* c = s->ctx;
        const long n = (long)enc_ctx(c, s) * c->hp.n_audio_state;
        if (n > cap) return -1;
        hipSetDevice(c->device);
        std::vector<uint16_t> h(n);
        WM_CHECK(hipMemcpy(h.data(), s->ws.hn, n * 2, hipMemcpyDeviceToHost));
        for (long i = 0; i < n; i++) {
            if (c->dt == DType::F16) out[i] = h2f(h[i]);
            else { uint32_t u = (uint32_t)h[i] << 16; memcpy(&out[i], &u, 4); }
        }
        return 0;
    });
}
int whisper_mi355x_set_audio_ctx(struct whisper_state* s, int audio_ctx) {
    if (!s || !s->ctx) return -1;  // orphan state: its context was freed
    if (audio_ctx > s->ctx->hp.n_audio_ctx) return -5;
    s->audio_ctx = audio_ctx;
    return 0;
}
int whisper_mi355x_state_info(struct whisper_state* s, int out[5]) {
    if (!s || !out) return -1;
    out[0] = s->direct ? 1 : 0;
    out[1] = s->ws.cap_jobs;
    out[2] = s->ws.cap_cross;
    out[3] = (int)s->dec_graphs.size();
    out[4] = s->pooled ? 1 : 0;
    return 5;
}
void* whisper_mi355x_state_stream(struct whisper_state* s) { return s ? (void*)s->stream : nullptr; }
int whisper_mi355x_kernel_timing(struct whisper_state* s, int class_mask) {
    if (!s) return -1;
    s->ktime_mask = class_mask;
    for (auto& k : s->kstat) k = KStat();
    for (auto& k : s->vad_kstat) k = KStat();
    return 0;
}
int whisper_mi355x_kernel_stats(struct whisper_state* s, int cls, double out[3]) {
    if (s && cls == WHISPER_MI355X_KSTAT_PDEC_GIVE_UPS) {
        out[0] = s->pdec_lost_ms;
        out[1] = (double)s->pdec_give_ups;
        out[2] = 0.0;
        return 0;
    }
    if (s && cls == WHISPER_MI355X_KSTAT_BEAM_GATHER && s->ctx) {
        const Hparams& hp = s->ctx->hp;
        const double row_bytes = (double)hp.n_text_layer * 2 * hp.n_text_head * 128;
        out[0] = s->gather_rows * row_bytes;
        out[1] = s->gather_rows_full * row_bytes;
        out[2] = 0.0;
        return 0;
    }
    if (s && cls >= WHISPER_MI355X_KSTAT_VAD_FRONTEND && cls <= WHISPER_MI355X_KSTAT_VAD_GATHER) {
        const KStat& k = s->vad_kstat[cls - WHISPER_MI355X_KSTAT_VAD_FRONTEND];
        out[0] = k.ms; out[1] = (double)k.count; out[2] = k.work;
        return 0;
    }
    if (cls == WHISPER_MI355X_KSTAT_LOGITS_STAGE) cls = K_LOGITS_STAGE;
    if (!s || cls < 0 || cls >= K_NCLASS) return -1;
    out[0] = s->kstat[cls].ms;
    out[1] = (double)s->kstat[cls].count;
    out[2] = s->kstat[cls].work;
    return 0;
}
// ---- kernel-level test/tuning hooks ---------------------------------------------------------------

void whisper_mi355x_set_gemm_variant(int v) { wm::g_gemm_variant = v; }
void whisper_mi355x_set_gemm_stamps(void* dev) { wm::g_gemm_stamps = (unsigned long long*)dev; }
void whisper_mi355x_set_dec_splits(int splits) { wm::g_dec_splits = splits; }
void whisper_mi355x_set_dec_bm(int rows) { wm::g_dec_bm = rows; }
void whisper_mi355x_set_pdec_spin(long ticks) {
    wm::g_pdec_spin_ticks = ticks;
    wm::g_pdec_gen.fetch_add(1, std::memory_order_release);
}
void whisper_mi355x_set_pdec_stamps(void* dev) {
    wm::g_pdec_stamps = (unsigned long long*)dev;
    wm::g_pdec_gen.fetch_add(1, std::memory_order_release);
}
// debug: device pointers of the state's decode workspace: 0 x (f32 [rows][d]), 1 final LN rows, 2 (unused), 3
// attention outputs, 4 GELU rows, 5 cross q, 6 Q', 7 cross partials, 8 their {m, l}
void* whisper_mi355x_debug_ws(struct whisper_state* s, int which) {
    if (!s) return nullptr;
    const wm::Workspace& w = s->ws;
    void* p[9] = {w.dx, w.dh, nullptr, w.datt, w.dff, w.dq, w.qx, w.xo, w.xml};
    return which >= 0 && which < 9 ? p[which] : nullptr;
}
long whisper_mi355x_decoded_tokens_total(void) { return wm::g_decoded_tokens_total.load(); }
long whisper_mi355x_pdec_give_ups(struct whisper_state* s) { return s ? s->pdec_give_ups : wm::g_pdec_give_ups_total.load(); }
void whisper_mi355x_set_pdec_blocks(int on) { wm::g_pdec_blocks = on != 0; }
// out[M][N] (f32 for epi EPI_F32 / EPI_RESID, else the context dtype) = A[M][K] . B[N][K]^T + bias,
// all device pointers; runs `reps` times and returns the average ms per launch in *ms.
int whisper_mi355x_debug_gemm(struct whisper_context* ctx, int epi, const void* A, int M, int K, const void* B, int N,
                              const float* bias, void* out, int reps, float* ms) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx) return -1;
        // out of EPI_CROSSKV = a cross cache [M / n_audio_ctx][N / 2K][2][K / 64][n_audio_ctx][64], slots in order
        const int T = ctx->c.hp.n_audio_ctx;
        if (epi == EPI_CROSSKV && (M % T != 0 || K % 64 != 0 || N % (2 * K) != 0)) return -1;
        hipSetDevice(ctx->c.device);
        HookBufs b;
        HookStream hs;
        GemmArgs g = gemm_plain(A, M, K, B, N, bias, out, N);
        if (M <= 128) {  // decode-step shapes take the split-K path, as in the engine
            g.splitk_ws_elems = 64L * M * N;
            g.splitk_ws = (float*)b.get(g.splitk_ws_elems * sizeof(float));
        }
        if (epi == EPI_CROSSKV) {
            std::vector<int> slots(M / T);
            for (int i = 0; i < M / T; i++) slots[i] = i;
            int* dslot = (int*)b.get(slots.size() * sizeof(int));
            WM_CHECK(hipMemcpy(dslot, slots.data(), slots.size() * sizeof(int), hipMemcpyHostToDevice));
            g.cache = out; g.row_slot = dslot; g.d = K; g.H = K / 64; g.ctx = T; g.L = N / (2 * K); g.layer = 0;
        }
        const float t = timed_ms(hs.st, reps, true, [&] { launch_gemm(ctx->c.dt, epi, g, hs.st); });
        if (ms) *ms = t;
        return 0;
    });
}
int whisper_mi355x_debug_gemm_small(struct whisper_context* ctx, int epi, const void* A, int M, int K, const void* B,
                                    int N, const float* bias, void* out, const float* ln_w, const float* ln_b, int reps,
                                    float* ms) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !gemm_small_ok(M, K, ln_w != nullptr)) return -1;
        hipSetDevice(ctx->c.device);
        HookStream hs;
        GemmArgs g = gemm_plain(A, M, K, B, N, bias, out, N);
        g.a_ln_w = ln_w; g.a_ln_b = ln_b;
        const float t = timed_ms(hs.st, reps, true, [&] { launch_gemm_small(ctx->c.dt, epi, g, ln_w != nullptr, hs.st); });
        if (ms) *ms = t;
        return 0;
    });
}
// GGML block-quantized weights given by field (QMat: qs, qh, dm; qh only for the q5 types)
static bool debug_qmat(QMat* q, int type, const void* qs, const void* qh, const void* dm) {
    const bool known = type == 2 || type == 3 || type == 6 || type == 7 || type == 8;
    if (!known || !qs || !dm || ((type == 6 || type == 7) && !qh)) return false;
    q->type = type;
    q->qs = (const uint8_t*)qs;
    q->qh = (const uint32_t*)qh;
    q->dm = (const uint16_t*)dm;
    return true;
}
int whisper_mi355x_debug_dequant(struct whisper_context* ctx, int type, const void* qs, const void* qh, const void* dm,
                                 long rows, int K, void* out) {
    return guarded(nullptr, [&]() -> int {
        QMat q;
        if (!ctx || !out || rows < 1 || K < 1 || !debug_qmat(&q, type, qs, qh, dm)) return -1;
        hipSetDevice(ctx->c.device);
        launch_dequant(ctx->c.dt, q, rows, K, out, nullptr);
        WM_CHECK(hipDeviceSynchronize());
        return 0;
    });
}
int whisper_mi355x_debug_dequant_multi(struct whisper_context* ctx, const int* type, int n, const void* const* qs,
                                       const void* const* qh, const void* const* dm, const long* rows, const int* K,
                                       void* const* out) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !type || !qs || !qh || !dm || !rows || !K || !out || n < 1 || n > 6) return -1;
        DequantJobs J;
        J.n = n;
        for (int j = 0; j < n; j++) {
            if (!out[j] || rows[j] < 1 || K[j] < 1 || !debug_qmat(&J.q[j], type[j], qs[j], qh[j], dm[j])) return -1;
            J.rows[j] = rows[j];
            J.K[j] = K[j];
            J.out[j] = out[j];
        }
        hipSetDevice(ctx->c.device);
        launch_dequant_multi(ctx->c.dt, J, nullptr);
        WM_CHECK(hipDeviceSynchronize());
        return 0;
    });
}
int whisper_mi355x_debug_gemm_small_q(struct whisper_context* ctx, int epi, const void* A, int M, int K, int type,
                                      const void* qs, const void* qh, const void* dm, int N, const float* bias,
                                      float scale, void* out, const float* ln_w, const float* ln_b) {
    return guarded(nullptr, [&]() -> int {
        QMat q;
        if (!ctx || !A || !out || N < 1 || !gemm_small_ok(M, K, ln_w != nullptr) || (ln_w && !ln_b) ||
            !debug_qmat(&q, type, qs, qh, dm))
            return -1;
        hipSetDevice(ctx->c.device);
        HookStream hs;
        GemmArgs g = gemm_plain(A, M, K, nullptr, N, bias, out, N);
        g.q = q;
        g.sc_div = N; g.sc_mod = 1; g.sc_lim = 1; g.scale = scale;  // every column scaled (EPI_STORE), as the cross-Q call
        g.a_ln_w = ln_w; g.a_ln_b = ln_b;
        launch_gemm_small(ctx->c.dt, epi, g, ln_w != nullptr, hs.st);
        WM_CHECK(hipStreamSynchronize(hs.st));
        return 0;
    });
}
int whisper_mi355x_debug_gemm_fp8(struct whisper_context* ctx, int epi, const void* A8, const float* a_scale, int M,
                                  int K, const void* B8, const float* b_scale, int N, const float* bias, void* out,
                                  int reps, float* ms) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx) return -1;
        hipSetDevice(ctx->c.device);
        HookStream hs;
        const GemmArgs g = gemm_plain(A8, M, K, B8, N, bias, out, N);
        const float t = timed_ms(hs.st, reps, true, [&] { launch_gemm_fp8(ctx->c.dt, epi, g, a_scale, b_scale, hs.st); });
        if (ms) *ms = t;
        return 0;
    });
}
int whisper_mi355x_debug_gemm_w8(struct whisper_context* ctx, int epi, const void* A, int M, int K, const void* B8,
                                 const float* b_scale, int N, const float* bias, void* out, const float* ln_w,
                                 const float* ln_b, void* y) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !b_scale || M < 1 || M > 128 || K % 64 || (epi == EPI_RESID && (!ln_w || !y))) return -1;
        hipSetDevice(ctx->c.device);
        HookBufs b;
        HookStream hs;
        GemmArgs g = gemm_plain(A, M, K, B8, N, bias, out, N);
        g.w8_scale = b_scale;
        if (epi == EPI_RESID) { g.ln_w = ln_w; g.ln_b = ln_b; g.ln_out = y; }
        g.splitk_ws_elems = 16L * M * N;
        g.splitk_ws = (float*)b.get(g.splitk_ws_elems * sizeof(float));
        launch_gemm(ctx->c.dt, epi, g, hs.st);
        WM_CHECK(hipStreamSynchronize(hs.st));
        return 0;
    });
}
int whisper_mi355x_debug_quant_fp8(struct whisper_context* ctx, const void* x, long rows, int K, void* q, float* s) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx) return -1;
        hipSetDevice(ctx->c.device);
        launch_quant_rows_fp8(ctx->c.dt, x, rows, K, q, s, nullptr);
        WM_CHECK(hipDeviceSynchronize());
        return 0;
    });
}
int whisper_mi355x_debug_attn_encoder(struct whisper_context* ctx, const void* qkv, int B, int T, int d, int H,
                                      int variant, void* out, int reps, float* ms) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || B < 1 || T < 1 || d != 64 * H || (variant != 2 && variant != 6)) return -1;
        hipSetDevice(ctx->c.device);
        HookStream hs;
        const float t = timed_ms(hs.st, reps, true, [&] { launch_attn_encoder(ctx->c.dt, qkv, out, B, T, d, H, hs.st, variant); });
        if (ms) *ms = t;
        return 0;
    });
}

int whisper_mi355x_debug_gemm_ln(struct whisper_context* ctx, const void* A, int M, int K, const void* B, int N,
                                 const float* bias, float* x, const float* ln_w, const float* ln_b, void* y, int reps,
                                 float* ms) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || M > 128) return -1;
        hipSetDevice(ctx->c.device);
        HookBufs b;
        HookStream hs;
        GemmArgs g = gemm_plain(A, M, K, B, N, bias, x, N);
        g.ln_w = ln_w; g.ln_b = ln_b; g.ln_out = y;
        g.splitk_ws_elems = 64L * M * N;
        g.splitk_ws = (float*)b.get(g.splitk_ws_elems * sizeof(float));
        // (x is updated in place by every launch: no warm launch, and at least one)
        const float t = timed_ms(hs.st, std::max(1, reps), false, [&] { launch_gemm(ctx->c.dt, EPI_RESID, g, hs.st); });
        if (ms) *ms = t;
        return 0;
    });
}
// Direct cross attention (kernels/xattn.hip: Q' projection, one pass over E, split merge + Wv) on
// caller data, all device pointers in the context dtype: enc [slots][n_ctx][d], slot [n] int,
// q [n][d] (already scaled), wkt [H][d][64], wv [d][d], bv [d] f32 -> out [n][d].
int whisper_mi355x_debug_xattn(struct whisper_context* ctx, const void* enc, const int* slot, const void* q,
                               const void* wkt, const void* wv, const float* bv, int n, int n_ctx, int d, float scale,
                               int splits, float rescale_thr, void* out, int reps, float* ms) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || n <= 0 || !xattn_supported(d)) return -1;
        hipSetDevice(ctx->c.device);
        const DType dt = ctx->c.dt;
        const int H = d / 64;
        if (splits <= 0) splits = xattn_splits(n, n_ctx);
        HookBufs b;
        HookStream hs;
        void* qx = b.get((size_t)n * 2 * H * d * 2);
        float* op = (float*)b.get((size_t)n * splits * H * d * 4);
        float* ml = (float*)b.get((size_t)n * splits * H * 2 * 4);
        const float t = timed_ms(hs.st, reps, true, [&] {
            launch_xattn_qproj(dt, q, wkt, n, d, H, scale, qx, hs.st);
            launch_xattn_step(dt, enc, slot, qx, n, n_ctx, d, splits, rescale_thr, op, ml, hs.st);
            launch_xattn_combine(dt, op, ml, splits, wv, bv, n, d, H, out, hs.st);
        });
        if (ms) *ms = t;
        return 0;
    });
}

// ---- decoder attention (kernels/attn.hip) on caller data: one launch each, all device pointers ----------
// slabs [splits][n][3d] f32 (q | k | v partial sums), bias [3d] f32 or null, cache
// [slots][L][2][H][n_ctx][64] in the context dtype (K[pos], V[pos] are written), slot / pos [n] int -> out [n][d]
int whisper_mi355x_debug_attn_self_step(struct whisper_context* ctx, const float* slabs, int splits, const float* bias,
                                        float scale, void* cache, const int* slot, const int* pos, int n, int L,
                                        int layer, int H, int n_ctx, void* out) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || n <= 0 || splits < 1 || splits > 16) return -1;
        hipSetDevice(ctx->c.device);
        const int d = 64 * H;
        const DecSlabs sl{slabs, splits, (long)n * 3 * d, 3 * d, bias, scale};
        HookStream hs;
        hipStream_t st = hs.st;
        launch_attn_self_step(ctx->c.dt, sl, cache, slot, pos, n, L, layer, H, n_ctx, d, out, st);
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
// slabs [splits][n][d] f32 (cross-Q partial sums), bias [d] f32 or null, n_kv [n] int (keys per token); the
// launcher picks the 1024- or the 256-thread kernel by n
int whisper_mi355x_debug_attn_cross_step(struct whisper_context* ctx, const float* slabs, int splits, const float* bias,
                                         float scale, const void* cache, const int* slot, const int* n_kv, int n, int L,
                                         int layer, int H, int n_ctx, void* out) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || n <= 0 || splits < 1 || splits > 16) return -1;
        hipSetDevice(ctx->c.device);
        const int d = 64 * H;
        const DecSlabs sl{slabs, splits, (long)n * d, d, bias, scale};
        HookStream hs;
        hipStream_t st = hs.st;
        launch_attn_cross_step(ctx->c.dt, sl, cache, slot, n_kv, n, L, layer, H, n_ctx, d, out, st);
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
// ---- beam search's kernels on caller data (kernels/logits.hip top-k forms, kernels/beam.hip) ---------------------
static_assert(sizeof(whisper_mi355x_cand) == sizeof(TokOut), "whisper_mi355x_cand mirrors TokOut");
// the deny mask of a hook on the device (null stays null: the launch without a mask)
static const uint32_t* hook_deny(HookBufs& b, const uint32_t* deny, int n_vocab, hipStream_t st) {
    if (!deny) return nullptr;
    const size_t bytes = (size_t)suppress_words(n_vocab) * sizeof(uint32_t);
    uint32_t* d = (uint32_t*)b.get(bytes);
    WM_CHECK(hipMemcpyAsync(d, deny, bytes, hipMemcpyHostToDevice, st));
    return d;
}
// the grammar words of a hook's n rows on the device (null stays null: the launch without a grammar)
static const uint32_t* hook_gram(HookBufs& b, const uint32_t* gram, int n, int n_vocab, hipStream_t st) {
    if (!gram) return nullptr;
    const size_t bytes = (size_t)n * grammar_words(n_vocab) * sizeof(uint32_t);
    uint32_t* d = (uint32_t*)b.get(bytes);
    WM_CHECK(hipMemcpyAsync(d, gram, bytes, hipMemcpyHostToDevice, st));
    return d;
}
int whisper_mi355x_debug_logits_topk(struct whisper_context* ctx, const float* logits, int n, const int* rules,
                                     const float* temperature, int k, int split, struct whisper_mi355x_cand* cand,
                                     struct whisper_mi355x_cand* greedy) {
    return whisper_mi355x_debug_logits_topk_deny(ctx, logits, n, rules, temperature, k, split, cand, greedy, nullptr);
}
int whisper_mi355x_debug_logits_topk_deny(struct whisper_context* ctx, const float* logits, int n, const int* rules,
                                          const float* temperature, int k, int split, struct whisper_mi355x_cand* cand,
                                          struct whisper_mi355x_cand* greedy, const uint32_t* deny) {
    return whisper_mi355x_debug_logits_topk_gram(ctx, logits, n, rules, temperature, k, split, cand, greedy, deny, nullptr, 0.0f);
}
int whisper_mi355x_debug_logits_topk_gram(struct whisper_context* ctx, const float* logits, int n, const int* rules,
                                          const float* temperature, int k, int split, struct whisper_mi355x_cand* cand,
                                          struct whisper_mi355x_cand* greedy, const uint32_t* deny, const uint32_t* gram,
                                          float penalty) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !logits || !rules || !cand || !greedy || n <= 0 || k < 1 || k > kTopkMax) return -1;
        hipSetDevice(ctx->c.device);
        const int V = ctx->c.hp.n_vocab;
        std::vector<SeqCtl> ctl(n);
        for (int r = 0; r < n; r++) {
            const int* q = rules + (size_t)r * 10;
            ctl[r] = SeqCtl{q[0], q[1], q[2], q[3], q[4], temperature ? temperature[r] : 0.0f, q[5], q[6], q[7], q[8], 0, q[9]};
        }
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        SeqCtl* d_ctl = (SeqCtl*)b.get(n * sizeof(SeqCtl));
        TokOut* d_out = (TokOut*)b.get((size_t)n * (kTopkMax + 1) * sizeof(TokOut));
        void* rec = split ? b.get(logits_rec_bytes(n)) : nullptr;
        WM_CHECK(hipMemcpyAsync(d_ctl, ctl.data(), n * sizeof(SeqCtl), hipMemcpyHostToDevice, st));
        const uint32_t* d_deny = hook_deny(b, deny, V, st);
        const uint32_t* d_gram = hook_gram(b, gram, n, V, st);
        launch_logits(logits, V, d_ctl, n, ctx->c.vid, d_out + (size_t)n * kTopkMax, nullptr, rec, d_deny, d_gram, penalty, st);
        launch_logits_topk(logits, V, d_ctl, n, ctx->c.vid, d_out, k, rec, d_deny, d_gram, penalty, st);
        std::vector<TokOut> out((size_t)n * (kTopkMax + 1));
        WM_CHECK(hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(TokOut), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        for (int r = 0; r < n; r++) {
            memcpy(&greedy[r], &out[(size_t)n * kTopkMax + r], sizeof(TokOut));
            for (int q = 0; q < k; q++) memcpy(&cand[(size_t)r * k + q], &out[(size_t)r * kTopkMax + q], sizeof(TokOut));
        }
        return 0;
    });
}
// ---- the sampled draw on caller data (kernels/sample.hip) ---------------------------------------------------------
int whisper_mi355x_debug_sample(struct whisper_context* ctx, const float* probs, const struct whisper_mi355x_cand* rec_in, int n,
                                int n_vocab, uint64_t seed, const int* counters, const uint32_t* words,
                                struct whisper_mi355x_cand* rec_out) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !probs || !rec_in || !counters || !rec_out || n <= 0 || n > kSampleMaxRows || n_vocab < 1 || n_vocab > 65536)
            return -1;
        hipSetDevice(ctx->c.device);
        const size_t pbytes = (size_t)n * 2 * n_vocab * sizeof(float);
        std::vector<int> ctr((size_t)n * 4);
        for (int r = 0; r < n; r++) {
            for (int k = 0; k < 3; k++) ctr[(size_t)r * 4 + k] = counters[(size_t)r * 3 + k];
            ctr[(size_t)r * 4 + 3] = r;
        }
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        float* d_probs = (float*)b.get(pbytes);
        TokOut* d_rec = (TokOut*)b.get(n * sizeof(TokOut));
        int* d_ctr = (int*)b.get(ctr.size() * sizeof(int));
        uint32_t* d_words = words ? (uint32_t*)b.get(n * sizeof(uint32_t)) : nullptr;
        WM_CHECK(hipMemcpyAsync(d_probs, probs, pbytes, hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_rec, rec_in, n * sizeof(TokOut), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_ctr, ctr.data(), ctr.size() * sizeof(int), hipMemcpyHostToDevice, st));
        if (d_words) WM_CHECK(hipMemcpyAsync(d_words, words, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        launch_sample(d_probs, n_vocab, d_rec, d_rec, d_ctr, d_words, seed, ctx->c.vid.beg, n, st);  // in place, as a step does
        WM_CHECK(hipMemcpyAsync(rec_out, d_rec, n * sizeof(TokOut), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
// ---- the token-time kernels on caller data (kernels/tokts.hip) -----------------------------------------------------
double whisper_mi355x_token_times_ms(struct whisper_state* s) { return s ? s->tokts_ms : 0.0; }
// clip c starts at the running offset rounded up to 64 floats; false when a clip has fewer than 1 sample
static bool tt_hook_clips(const int* n_samples, int n_clips, std::vector<TtClip>& cl, size_t& total, int& max_n) {
    cl.resize(n_clips);
    total = 0;
    max_n = 0;
    for (int c = 0; c < n_clips; c++) {
        if (n_samples[c] < 1) return false;
        cl[c] = TtClip{nullptr, (long long)total, n_samples[c], 0};
        total += ((size_t)n_samples[c] + 63) & ~(size_t)63;
        max_n = std::max(max_n, n_samples[c]);
    }
    return true;
}
int whisper_mi355x_debug_signal_energy(struct whisper_context* ctx, const float* pcm, const int* n_samples, int n_clips,
                                       float* energy_out) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !pcm || !n_samples || !energy_out || n_clips < 1 || n_clips > 65535) return -1;
        std::vector<TtClip> cl;
        size_t total;
        int max_n;
        if (!tt_hook_clips(n_samples, n_clips, cl, total, max_n)) return -1;
        hipSetDevice(ctx->c.device);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        float* d_pcm = (float*)b.get(total * sizeof(float));
        float* d_e = (float*)b.get(total * sizeof(float));
        TtClip* d_cl = (TtClip*)b.get(cl.size() * sizeof(TtClip));
        for (TtClip& c : cl) c.pcm = d_pcm + c.e_off;
        WM_CHECK(hipMemcpyAsync(d_pcm, pcm, total * sizeof(float), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemsetAsync(d_e, 0, total * sizeof(float), st));  // (the padding between clips)
        WM_CHECK(hipMemcpyAsync(d_cl, cl.data(), cl.size() * sizeof(TtClip), hipMemcpyHostToDevice, st));
        launch_signal_energy(d_cl, n_clips, max_n, d_e, st);
        WM_CHECK(hipMemcpyAsync(energy_out, d_e, total * sizeof(float), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
static_assert(sizeof(whisper_mi355x_token_span) == sizeof(TtSpan), "whisper_mi355x_token_span mirrors TtSpan");
int whisper_mi355x_debug_token_vad(struct whisper_context* ctx, const float* energy, const int* n_samples, int n_clips,
                                   const int* seg_clip, const int* seg_n_tokens, int n_segs,
                                   struct whisper_mi355x_token_span* spans) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !energy || !n_samples || !seg_clip || !seg_n_tokens || !spans || n_clips < 1 || n_segs < 1) return -1;
        std::vector<TtClip> cl;
        size_t total;
        int max_n;
        if (!tt_hook_clips(n_samples, n_clips, cl, total, max_n)) return -1;
        std::vector<TtSeg> sg(n_segs);
        long n_tok = 0;
        for (int q = 0; q < n_segs; q++) {
            if (seg_clip[q] < 0 || seg_clip[q] >= n_clips || seg_n_tokens[q] < 2 || n_tok + seg_n_tokens[q] > INT32_MAX) return -1;
            sg[q] = TtSeg{seg_clip[q], (int)n_tok, seg_n_tokens[q], 0};
            n_tok += seg_n_tokens[q];
        }
        hipSetDevice(ctx->c.device);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        float* d_e = (float*)b.get(total * sizeof(float));
        TtClip* d_cl = (TtClip*)b.get(cl.size() * sizeof(TtClip));
        TtSeg* d_sg = (TtSeg*)b.get(sg.size() * sizeof(TtSeg));
        TtSpan* d_sp = (TtSpan*)b.get((size_t)n_tok * sizeof(TtSpan));
        WM_CHECK(hipMemcpyAsync(d_e, energy, total * sizeof(float), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_cl, cl.data(), cl.size() * sizeof(TtClip), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_sg, sg.data(), sg.size() * sizeof(TtSeg), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_sp, spans, (size_t)n_tok * sizeof(TtSpan), hipMemcpyHostToDevice, st));
        launch_token_vad(d_e, d_cl, d_sg, n_segs, d_sp, st);
        WM_CHECK(hipMemcpyAsync(spans, d_sp, (size_t)n_tok * sizeof(TtSpan), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
// ---- the deny mask of suppress_nst / suppress_regex (suppress.h; host only) ------------------------------------------
int whisper_mi355x_suppress_mask(struct whisper_context* ctx, bool suppress_nst, const char* regex, uint32_t* words,
                                 int cap_words) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !words || cap_words < suppress_words(ctx->c.hp.n_vocab)) return -1;
        std::vector<uint32_t> w;
        if (const int r = deny_lookup(&ctx->c, suppress_nst, regex, &w)) return r;
        memcpy(words, w.data(), w.size() * sizeof(uint32_t));
        return (int)w.size();
    });
}
long whisper_mi355x_suppress_builds(struct whisper_context* ctx) {
    if (!ctx) return 0;
    std::lock_guard<std::mutex> lk(ctx->c.deny_mu);
    return ctx->c.deny_builds;
}
// ---- whisper_full_params.grammar_rules (grammar.h; host only) ----------------------------------------------------------
int whisper_mi355x_grammar_mask(struct whisper_context* ctx, const whisper_grammar_element** rules, size_t n_rules,
                                size_t i_start, const whisper_token* accepted_tokens, int n_accepted, uint32_t* words,
                                int cap_words) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !words || n_accepted < 0 || (n_accepted > 0 && !accepted_tokens) ||
            cap_words < grammar_words(ctx->c.hp.n_vocab))
            return -1;
        whisper_full_params p{};
        p.grammar_rules = rules;
        p.n_grammar_rules = n_rules;
        p.i_start_rule = i_start;
        GrammarRules g;
        if (const int r = grammar_check(p, g)) return r;
        Grammar st;
        st.init(g);
        const Vocab& v = ctx->c.vocab;
        for (int k = 0; k < n_accepted; k++) {
            if (accepted_tokens[k] < 0 || accepted_tokens[k] >= (int)v.id_to_token.size()) return -1;
            st.accept_token(g, v.id_to_token[accepted_tokens[k]]);
        }
        grammar_reject(g, gram_vocab(&ctx->c), st, words);
        return grammar_words(ctx->c.hp.n_vocab);
    });
}
int whisper_mi355x_grammar_stats(struct whisper_state* state, struct whisper_mi355x_grammar_stats* out) {
    if (!state || !out) return -1;
    memset(out, 0, sizeof(*out));
    for (const whisper_state* s : {(const whisper_state*)state, (const whisper_state*)state->twin}) {  // (a paired batch's second half)
        if (!s) continue;
        out->rows_device += s->ws.gd.rows_device;
        out->rows_patched += s->ws.gd.rows_patched;
        out->rows_host += s->ws.gd.rows_host;
        out->kernel_ms += s->kstat[K_GRAMMAR].ms;
        out->kernel_launches += s->kstat[K_GRAMMAR].count;
    }
    return 0;
}
int whisper_mi355x_debug_grammar_reject(struct whisper_context* ctx, const whisper_grammar_element** rules, size_t n_rules,
                                        size_t i_start, const whisper_token* accepted_tokens, const int* n_accepted, int n_rows,
                                        uint32_t* words, int* flags) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !n_accepted || !words || !flags || n_rows <= 0) return -1;
        whisper_full_params p{};
        p.grammar_rules = rules;
        p.n_grammar_rules = n_rules;
        p.i_start_rule = i_start;
        GrammarRules g;
        if (const int r = grammar_check(p, g)) return r;
        if (!g.on()) return -1;
        const Vocab& v = ctx->c.vocab;
        std::vector<Grammar> states(n_rows);
        std::vector<const Grammar*> ptrs(n_rows);
        size_t k = 0;
        for (int r = 0; r < n_rows; r++) {
            if (n_accepted[r] < 0 || (n_accepted[r] > 0 && !accepted_tokens)) return -1;
            states[r].init(g);
            for (int i = 0; i < n_accepted[r]; i++, k++) {
                if (accepted_tokens[k] < 0 || accepted_tokens[k] >= (int)v.id_to_token.size()) return -1;
                states[r].accept_token(g, v.id_to_token[accepted_tokens[k]]);
            }
            ptrs[r] = &states[r];
        }
        hipSetDevice(ctx->c.device);
        const size_t W = grammar_words(ctx->c.hp.n_vocab), bytes = (size_t)n_rows * W * sizeof(uint32_t);
        HookBufs b;
        HookStream hs;
        struct Dev { GramDev d; ~Dev() { gram_dev_free(d); } } dev;
        uint32_t* d_gram = (uint32_t*)b.get(bytes);
        WM_CHECK(hipMemsetAsync(d_gram, 0xff, bytes, hs.st));  // (words nothing writes would show)
        gram_dev_rules(dev.d, g, hs.st);
        gram_masks(&ctx->c, dev.d, g, ptrs.data(), n_rows, d_gram, words, flags, hs.st, nullptr);  // (words: the staging too)
        WM_CHECK(hipMemcpyAsync(words, d_gram, bytes, hipMemcpyDeviceToHost, hs.st));
        WM_CHECK(hipStreamSynchronize(hs.st));
        return (int)W;
    });
}
// ---- the greedy logits kernels and the step advance on caller data (kernels/logits.hip) --------------------------
static_assert(sizeof(whisper_mi355x_seq_ctl) == sizeof(SeqCtl), "whisper_mi355x_seq_ctl mirrors SeqCtl");
int whisper_mi355x_debug_logits(struct whisper_context* ctx, const float* logits, int n,
                                const struct whisper_mi355x_seq_ctl* ctl, int form, struct whisper_mi355x_cand* out,
                                float* probs) {
    return whisper_mi355x_debug_logits_deny(ctx, logits, n, ctl, form, out, probs, nullptr);
}
int whisper_mi355x_debug_logits_deny(struct whisper_context* ctx, const float* logits, int n,
                                     const struct whisper_mi355x_seq_ctl* ctl, int form, struct whisper_mi355x_cand* out,
                                     float* probs, const uint32_t* deny) {
    return whisper_mi355x_debug_logits_gram(ctx, logits, n, ctl, form, out, probs, deny, nullptr, 0.0f);
}
int whisper_mi355x_debug_logits_gram(struct whisper_context* ctx, const float* logits, int n,
                                     const struct whisper_mi355x_seq_ctl* ctl, int form, struct whisper_mi355x_cand* out,
                                     float* probs, const uint32_t* deny, const uint32_t* gram, float penalty) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !logits || !ctl || !out || n <= 0 || form < 0 || form > 1) return -1;
        for (int r = 0; r < n; r++)
            if (ctl[r].want_probs && !probs) return -1;
        hipSetDevice(ctx->c.device);
        const int V = ctx->c.hp.n_vocab;
        const size_t pbytes = (size_t)n * 2 * V * sizeof(float);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        SeqCtl* d_ctl = (SeqCtl*)b.get(n * sizeof(SeqCtl));
        TokOut* d_out = (TokOut*)b.get(n * sizeof(TokOut));
        float* d_probs = probs ? (float*)b.get(pbytes) : nullptr;
        void* rec = form ? b.get(logits_rec_bytes(n)) : nullptr;
        WM_CHECK(hipMemcpyAsync(d_ctl, ctl, n * sizeof(SeqCtl), hipMemcpyHostToDevice, st));
        if (d_probs) WM_CHECK(hipMemsetAsync(d_probs, 0xff, pbytes, st));  // rows the kernel leaves alone read as NaN
        const uint32_t* d_deny = hook_deny(b, deny, V, st);
        launch_logits(logits, V, d_ctl, n, ctx->c.vid, d_out, d_probs, rec, d_deny, hook_gram(b, gram, n, V, st), penalty, st);
        WM_CHECK(hipGetLastError());
        WM_CHECK(hipMemcpyAsync(out, d_out, n * sizeof(TokOut), hipMemcpyDeviceToHost, st));
        if (d_probs) WM_CHECK(hipMemcpyAsync(probs, d_probs, pbytes, hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
// ---- the halves of a logits launch around a logits_filter_callback --------------------------------
static VocabIds hook_vid(struct whisper_context* ctx, int flags) {
    VocabIds v = ctx->c.vid;
    if (flags & 1) v.solm = -1;  // tdrz_enable: matches no id
    return v;
}
int whisper_mi355x_debug_logits_stage(struct whisper_context* ctx, const float* logits, int n,
                                      const struct whisper_mi355x_seq_ctl* ctl, int flags, float* out_rows) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !logits || !ctl || !out_rows || n <= 0) return -1;
        hipSetDevice(ctx->c.device);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        SeqCtl* d_ctl = (SeqCtl*)b.get(n * sizeof(SeqCtl));
        WM_CHECK(hipMemcpyAsync(d_ctl, ctl, n * sizeof(SeqCtl), hipMemcpyHostToDevice, st));
        launch_logits_stage(logits, ctx->c.hp.n_vocab, d_ctl, n, hook_vid(ctx, flags), out_rows, st);
        WM_CHECK(hipGetLastError());
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
int whisper_mi355x_debug_logits_ex(struct whisper_context* ctx, const float* raw, const float* filtered, int n,
                                   const struct whisper_mi355x_seq_ctl* ctl, int form, int flags,
                                   struct whisper_mi355x_cand* out, float* probs) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !raw || !ctl || !out || n <= 0 || form < 0 || form > 1) return -1;
        for (int r = 0; r < n; r++)
            if (ctl[r].want_probs && !probs) return -1;
        hipSetDevice(ctx->c.device);
        const int V = ctx->c.hp.n_vocab;
        const size_t pbytes = (size_t)n * 2 * V * sizeof(float);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        SeqCtl* d_ctl = (SeqCtl*)b.get(n * sizeof(SeqCtl));
        TokOut* d_out = (TokOut*)b.get(n * sizeof(TokOut));
        float* d_probs = probs ? (float*)b.get(pbytes) : nullptr;
        void* rec = form ? b.get(logits_rec_bytes(n)) : nullptr;
        WM_CHECK(hipMemcpyAsync(d_ctl, ctl, n * sizeof(SeqCtl), hipMemcpyHostToDevice, st));
        if (d_probs) WM_CHECK(hipMemsetAsync(d_probs, 0xff, pbytes, st));  // rows the kernel leaves alone read as NaN
        launch_logits(raw, V, d_ctl, n, hook_vid(ctx, flags), d_out, d_probs, rec, nullptr, nullptr, 0.0f, st, filtered);
        WM_CHECK(hipGetLastError());
        WM_CHECK(hipMemcpyAsync(out, d_out, n * sizeof(TokOut), hipMemcpyDeviceToHost, st));
        if (d_probs) WM_CHECK(hipMemcpyAsync(probs, d_probs, pbytes, hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
int whisper_mi355x_debug_logits_topk_ex(struct whisper_context* ctx, const float* raw, const float* filtered, int n,
                                        const struct whisper_mi355x_seq_ctl* ctl, int k, int split, int flags,
                                        struct whisper_mi355x_cand* cand, struct whisper_mi355x_cand* greedy) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !raw || !ctl || !cand || !greedy || n <= 0 || k < 1 || k > kTopkMax) return -1;
        hipSetDevice(ctx->c.device);
        const int V = ctx->c.hp.n_vocab;
        const VocabIds vid = hook_vid(ctx, flags);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        SeqCtl* d_ctl = (SeqCtl*)b.get(n * sizeof(SeqCtl));
        TokOut* d_out = (TokOut*)b.get((size_t)n * (kTopkMax + 1) * sizeof(TokOut));
        void* rec = split ? b.get(logits_rec_bytes(n)) : nullptr;
        WM_CHECK(hipMemcpyAsync(d_ctl, ctl, n * sizeof(SeqCtl), hipMemcpyHostToDevice, st));
        launch_logits(raw, V, d_ctl, n, vid, d_out + (size_t)n * kTopkMax, nullptr, rec, nullptr, nullptr, 0.0f, st, filtered);
        launch_logits_topk(raw, V, d_ctl, n, vid, d_out, k, rec, nullptr, nullptr, 0.0f, st, filtered);
        WM_CHECK(hipGetLastError());
        std::vector<TokOut> out((size_t)n * (kTopkMax + 1));
        WM_CHECK(hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(TokOut), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        for (int r = 0; r < n; r++) {
            memcpy(&greedy[r], &out[(size_t)n * kTopkMax + r], sizeof(TokOut));
            for (int q = 0; q < k; q++) memcpy(&cand[(size_t)r * k + q], &out[(size_t)r * kTopkMax + q], sizeof(TokOut));
        }
        return 0;
    });
}
int whisper_mi355x_debug_decode_advance(struct whisper_context* ctx, int n, int ct, int beg,
                                        const struct whisper_mi355x_cand* tout, int* ints,
                                        struct whisper_mi355x_seq_ctl* ctl, const unsigned* err,
                                        struct whisper_mi355x_cand* ring, unsigned* ring_err) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !tout || !ints || !ctl || !ring || !ring_err || n <= 0 || ct < n) return -1;
        hipSetDevice(ctx->c.device);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        TokOut* d_tout = (TokOut*)b.get(n * sizeof(TokOut));
        int* d_ints = (int*)b.get((size_t)5 * ct * sizeof(int));
        SeqCtl* d_ctl = (SeqCtl*)b.get(ct * sizeof(SeqCtl));
        TokOut* d_ring = (TokOut*)b.get(ct * sizeof(TokOut));
        unsigned* d_err = (unsigned*)b.get(2 * sizeof(unsigned));  // [0]: the error word, [1]: the ring's copy
        const unsigned h_err[2] = {err ? *err : 0u, *ring_err};
        WM_CHECK(hipMemcpyAsync(d_tout, tout, n * sizeof(TokOut), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_ints, ints, (size_t)5 * ct * sizeof(int), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_ctl, ctl, ct * sizeof(SeqCtl), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_ring, ring, ct * sizeof(TokOut), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(d_err, h_err, sizeof(h_err), hipMemcpyHostToDevice, st));
        launch_decode_advance(n, ct, beg, d_tout, d_ints, d_ctl, d_ring, err ? d_err : nullptr, d_err + 1, st);
        WM_CHECK(hipMemcpyAsync(ints, d_ints, (size_t)5 * ct * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipMemcpyAsync(ctl, d_ctl, ct * sizeof(SeqCtl), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipMemcpyAsync(ring, d_ring, ct * sizeof(TokOut), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipMemcpyAsync(ring_err, d_err + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}
int whisper_mi355x_debug_kv_gather(struct whisper_context* ctx, void* cache, int n_slots, int L, int H, int n_ctx,
                                   const int* copies, int n_copies, int* n_staged) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || !cache || !copies || n_copies < 0 || n_slots <= 0 || L <= 0 || H <= 0 || n_ctx <= 0) return -1;
        if (n_staged) *n_staged = 0;
        if (n_copies == 0) return 0;
        hipSetDevice(ctx->c.device);
        std::vector<KvCopy> cp(n_copies);
        for (int i = 0; i < n_copies; i++) {
            cp[i] = KvCopy{copies[4 * i], copies[4 * i + 1], copies[4 * i + 2], copies[4 * i + 3], 0, 0, 0};
            for (int q = 0; q < i; q++)
                if (cp[q].dst_slot == cp[i].dst_slot) return -1;
        }
        const long need = beam_schedule(cp, (long)L * 2 * H * 8);
        HookBufs b;
        HookStream hs;
        hipStream_t st = hs.st;
        KvCopy* d_cp = (KvCopy*)b.get(n_copies * sizeof(KvCopy));
        void* stage = need > 0 ? b.get((size_t)need * 16) : nullptr;
        WM_CHECK(hipMemcpyAsync(d_cp, cp.data(), n_copies * sizeof(KvCopy), hipMemcpyHostToDevice, st));
        launch_kv_gather(cache, n_slots, L, H, n_ctx, cp.data(), d_cp, n_copies, stage, need, st);
        WM_CHECK(hipStreamSynchronize(st));
        if (n_staged)
            for (const KvCopy& c : cp) *n_staged += c.mode;
        return 0;
    });
}
// q [tokens][q_stride] (already scaled), tiles [n_tiles] int pairs {first token, count <= 64}, slot / n_kv per token
int whisper_mi355x_debug_attn_prefill(struct whisper_context* ctx, const void* q, int q_stride, const void* cache,
                                      const int* slot, const int* n_kv, const void* tiles, int n_tiles, int L,
                                      int layer, int H, int n_ctx, void* out) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || n_tiles <= 0) return -1;
        hipSetDevice(ctx->c.device);
        HookStream hs;
        hipStream_t st = hs.st;
        launch_attn_prefill(ctx->c.dt, q, q_stride, cache, slot, n_kv, tiles, n_tiles, L, layer, H, n_ctx, 64 * H, out, st);
        WM_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

// ---- token-timestamp alignment kernels (kernels/align.hip) on caller data ------------------------------
// clip descriptors with the packed offsets the three hooks share: P [A][n_rows][F], cost [N][F], fr [N],
// path [N + F] pairs, clip after clip
static std::vector<AlignClip> align_hook_clips(int n_clips, const int* slot, const int* n_rows, const int* n_sot,
                                               const int* frames, int A, int* max_rows, int* max_n, int* max_f) {
    std::vector<AlignClip> cl(n_clips);
    long row0 = 0, p = 0, stt = 0, cost = 0, fr = 0, path = 0;
    *max_rows = *max_n = *max_f = 0;
    for (int k = 0; k < n_clips; k++) {
        AlignClip& a = cl[k];
        a = AlignClip{};
        a.slot = slot ? slot[k] : 0; a.row0 = (int)row0; a.n_rows = n_rows[k]; a.n_sot = n_sot ? n_sot[k] : 0; a.frames = frames[k];
        const long N = a.n_rows - a.n_sot - 1;
        a.p_off = p; a.st_off = stt; a.cost_off = cost; a.tr_off = cost; a.fr_off = fr; a.path_off = path;
        row0 += a.n_rows;
        p += (long)A * a.n_rows * a.frames;
        stt += (long)A * a.frames * 2;
        cost += std::max(N, 0L) * a.frames;
        fr += std::max(N, 0L);
        path += std::max(N, 0L) + a.frames;
        *max_rows = std::max(*max_rows, a.n_rows);
        *max_n = std::max(*max_n, (int)N);
        *max_f = std::max(*max_f, a.frames);
    }
    return cl;
}
static AlignClip* align_hook_upload(const std::vector<AlignClip>& cl) {
    AlignClip* d = nullptr;
    WM_CHECK(hipMalloc((void**)&d, cl.size() * sizeof(AlignClip)));
    WM_CHECK(hipMemcpy(d, cl.data(), cl.size() * sizeof(AlignClip), hipMemcpyHostToDevice));
    return d;
}
int whisper_mi355x_debug_align_scores(struct whisper_context* ctx, const void* q, const void* cross, int n_slots,
                                      int n_clips, const int* slot, const int* n_rows, const int* frames, int n_heads,
                                      const int* head_layer, const int* head_idx, float* P) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || n_clips <= 0 || n_heads <= 0) return -1;
        const Hparams& hp = ctx->c.hp;
        const int L = hp.n_text_layer, H = hp.n_text_head, d = hp.n_text_state;
        long tot = 0;
        for (int k = 0; k < n_clips; k++) {
            if (n_rows[k] < 1 || n_rows[k] > 256 || frames[k] < 1 || frames[k] > hp.n_audio_ctx || slot[k] < 0 ||
                slot[k] >= n_slots)
                return -1;
            tot += n_rows[k];
        }
        for (int a = 0; a < n_heads; a++)
            if (head_layer[a] < 0 || head_layer[a] >= L || head_idx[a] < 0 || head_idx[a] >= H) return -1;
        hipSetDevice(ctx->c.device);
        int mr, mn, mf;
        const std::vector<AlignClip> cl = align_hook_clips(n_clips, slot, n_rows, nullptr, frames, n_heads, &mr, &mn, &mf);
        AlignClip* dcl = align_hook_upload(cl);
        int2* dh = nullptr;
        WM_CHECK(hipMalloc((void**)&dh, n_heads * sizeof(int2)));
        for (int l = 0; l < L; l++) {  // one launch per layer that has heads, as the engine's pass
            std::vector<int2> hl;
            for (int a = 0; a < n_heads; a++)
                if (head_layer[a] == l) hl.push_back(make_int2(head_idx[a], a));
            if (hl.empty()) continue;
            WM_CHECK(hipMemcpy(dh, hl.data(), hl.size() * sizeof(int2), hipMemcpyHostToDevice));
            launch_align_scores(ctx->c.dt, (const char*)q + (size_t)l * tot * d * 2, d, cross, dcl, n_clips, mr, L, l, H,
                                hp.n_audio_ctx, hp.n_audio_ctx, dh, (int)hl.size(), P, nullptr);
            WM_CHECK(hipDeviceSynchronize());
        }
        hipFree(dh);
        hipFree(dcl);
        return 0;
    });
}
int whisper_mi355x_debug_align_cost(struct whisper_context* ctx, const float* P, int n_clips, const int* n_rows,
                                    const int* n_sot, const int* frames, int n_heads, float* cost) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || n_clips <= 0 || n_heads <= 0) return -1;
        for (int k = 0; k < n_clips; k++)
            if (frames[k] < 1 || n_sot[k] < 0 || n_rows[k] - n_sot[k] - 1 < 1) return -1;
        hipSetDevice(ctx->c.device);
        int mr, mn, mf;
        const std::vector<AlignClip> cl = align_hook_clips(n_clips, nullptr, n_rows, n_sot, frames, n_heads, &mr, &mn, &mf);
        AlignClip* dcl = align_hook_upload(cl);
        float* stats = nullptr;
        const long st_el = cl.back().st_off + (long)n_heads * cl.back().frames * 2;
        WM_CHECK(hipMalloc((void**)&stats, (size_t)st_el * sizeof(float)));
        launch_align_cost(P, dcl, n_clips, n_heads, mn, mf, stats, cost, nullptr);
        WM_CHECK(hipDeviceSynchronize());
        hipFree(stats);
        hipFree(dcl);
        return 0;
    });
}
int whisper_mi355x_debug_align_dtw(struct whisper_context* ctx, const float* cost, int n_clips, const int* rows,
                                   const int* frames, int* fr, int* path, int* path_len) {
    return guarded(nullptr, [&]() -> int {
        if (!ctx || n_clips <= 0 || !fr) return -1;
        std::vector<int> n_rows(n_clips);
        for (int k = 0; k < n_clips; k++) {
            if (rows[k] < 1 || rows[k] > 256 || frames[k] < 1) return -1;
            n_rows[k] = rows[k] + 1;  // (n_sot = 0, the last row dropped: N = rows)
        }
        hipSetDevice(ctx->c.device);
        int mr, mn, mf;
        const std::vector<AlignClip> cl = align_hook_clips(n_clips, nullptr, n_rows.data(), nullptr, frames, 1, &mr, &mn, &mf);
        AlignClip* dcl = align_hook_upload(cl);
        const long n_cost = cl.back().cost_off + (long)rows[n_clips - 1] * frames[n_clips - 1];
        const long n_fr = cl.back().fr_off + rows[n_clips - 1];
        const long n_path = cl.back().path_off + rows[n_clips - 1] + frames[n_clips - 1];
        unsigned char* trace = nullptr;
        int *dfr = nullptr, *dpath = nullptr, *dlen = nullptr;
        WM_CHECK(hipMalloc((void**)&trace, (size_t)n_cost));
        WM_CHECK(hipMalloc((void**)&dfr, (size_t)n_fr * sizeof(int)));
        WM_CHECK(hipMalloc((void**)&dpath, (size_t)n_path * 2 * sizeof(int)));
        WM_CHECK(hipMalloc((void**)&dlen, (size_t)n_clips * sizeof(int)));
        launch_align_dtw(cost, dcl, n_clips, mn, trace, dfr, dpath, dlen, nullptr);
        WM_CHECK(hipDeviceSynchronize());
        WM_CHECK(hipMemcpy(fr, dfr, (size_t)n_fr * sizeof(int), hipMemcpyDeviceToHost));
        if (path) WM_CHECK(hipMemcpy(path, dpath, (size_t)n_path * 2 * sizeof(int), hipMemcpyDeviceToHost));
        if (path_len) WM_CHECK(hipMemcpy(path_len, dlen, (size_t)n_clips * sizeof(int), hipMemcpyDeviceToHost));
        hipFree(trace);
        hipFree(dfr);
        hipFree(dpath);
        hipFree(dlen);
        hipFree(dcl);
        return 0;
    });
}
// ---- whisper.h's VAD block (Silero v5 on the device: vad.h) ------------------------------------------
struct whisper_vad_context {
    VadModel* m = nullptr;
    VadScratch sc;
    hipStream_t st = nullptr;
    std::vector<float> probs;  // of the last whisper_vad_detect_speech
    ~whisper_vad_context() {
        if (m) hipSetDevice(m->device);
        vad_scratch_free(sc);
        if (st) hipStreamDestroy(st);
        vad_model_free(m);
    }
};
struct whisper_vad_segments {
    std::vector<std::pair<float, float>> seg;  // 10 ms units
};

struct whisper_vad_params whisper_vad_default_params(void) {
    whisper_vad_params p;
    p.threshold = 0.5f;
    p.min_speech_duration_ms = 250;
    p.min_silence_duration_ms = 100;
    p.max_speech_duration_s = FLT_MAX;
    p.speech_pad_ms = 30;
    p.samples_overlap = 0.1f;
    return p;
}
struct whisper_vad_context_params whisper_vad_default_context_params(void) {
    whisper_vad_context_params p;
    p.n_threads = 4;
    p.use_gpu = true;  // (the only path there is: false is accepted and ignored)
    p.gpu_device = 0;
    return p;
}
static whisper_vad_context* vad_ctx_from_image(const uint8_t* data, size_t size, int device, const char* what) {
    whisper_vad_context* v = nullptr;
    guarded(nullptr, [&]() -> int {
        std::string err;
        VadModel* m = vad_model_load(data, size, device, &err);
        if (!m) {
            fprintf(stderr, "whisper_mi355x: vad model '%s' refused: %s\n", what, err.c_str());
            return -1;
        }
        v = new whisper_vad_context();
        v->m = m;
        try {
            WM_CHECK(hipStreamCreateWithFlags(&v->st, hipStreamNonBlocking));
        } catch (...) {
            delete v;
            v = nullptr;
            throw;
        }
        return 0;
    });
    return v;
}
struct whisper_vad_context* whisper_vad_init_from_file_with_params(const char* path_model, struct whisper_vad_context_params params) {
    FILE* fp = path_model ? fopen(path_model, "rb") : nullptr;
    if (!fp) {
        fprintf(stderr, "whisper_mi355x: vad model '%s' refused: cannot open the file\n", path_model ? path_model : "(null)");
        return nullptr;
    }
    std::vector<uint8_t> buf;
    uint8_t chunk[1 << 16];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, fp)) > 0 && buf.size() <= ((size_t)64 << 20)) buf.insert(buf.end(), chunk, chunk + n);
    fclose(fp);
    return vad_ctx_from_image(buf.data(), buf.size(), params.gpu_device, path_model);
}
struct whisper_vad_context* whisper_vad_init_with_params(struct whisper_model_loader* loader, struct whisper_vad_context_params params) {
    if (!loader || !loader->read) return nullptr;
    std::vector<uint8_t> buf;
    uint8_t chunk[1 << 16];
    while (buf.size() <= ((size_t)64 << 20)) {  // (a VAD model is about 1 MB)
        if (loader->eof && loader->eof(loader->context)) break;
        const size_t n = loader->read(loader->context, chunk, sizeof chunk);
        if (n == 0 || n > sizeof chunk) break;
        buf.insert(buf.end(), chunk, chunk + n);
    }
    if (loader->close) loader->close(loader->context);
    return vad_ctx_from_image(buf.data(), buf.size(), params.gpu_device, "(loader)");
}
bool whisper_vad_detect_speech(struct whisper_vad_context* vctx, const float* samples, int n_samples) {
    if (!vctx || n_samples < 0 || (!samples && n_samples > 0)) return false;
    return guarded(nullptr, [&]() -> int {
        WM_CHECK(hipSetDevice(vctx->m->device));
        std::vector<std::vector<float>> probs;
        vad_probs_run(*vctx->m, vctx->sc, &samples, &n_samples, 1, false, vctx->st, nullptr, probs, nullptr);
        vctx->probs.swap(probs[0]);
        return 0;
    }) == 0;
}
int whisper_vad_n_probs(struct whisper_vad_context* vctx) { return vctx ? (int)vctx->probs.size() : 0; }
float* whisper_vad_probs(struct whisper_vad_context* vctx) { return vctx ? vctx->probs.data() : nullptr; }
struct whisper_vad_segments* whisper_vad_segments_from_probs(struct whisper_vad_context* vctx, struct whisper_vad_params q) {
    if (!vctx) return nullptr;
    const VadParams vp{q.threshold, q.min_speech_duration_ms, q.min_silence_duration_ms, q.max_speech_duration_s, q.speech_pad_ms, q.samples_overlap};
    whisper_vad_segments* out = new whisper_vad_segments();
    for (const VadSpan& s : vad_segments_from_probs(vctx->probs.data(), (int)vctx->probs.size(), vp))
        out->seg.push_back({(float)s.start / 160.0f, (float)s.end / 160.0f});
    return out;
}
struct whisper_vad_segments* whisper_vad_segments_from_samples(struct whisper_vad_context* vctx, struct whisper_vad_params params,
                                                               const float* samples, int n_samples) {
    if (!whisper_vad_detect_speech(vctx, samples, n_samples)) return nullptr;
    return whisper_vad_segments_from_probs(vctx, params);
}
int whisper_vad_segments_n_segments(struct whisper_vad_segments* segments) { return segments ? (int)segments->seg.size() : 0; }
float whisper_vad_segments_get_segment_t0(struct whisper_vad_segments* segments, int i_segment) {
    return segments && i_segment >= 0 && i_segment < (int)segments->seg.size() ? segments->seg[i_segment].first : 0.0f;
}
float whisper_vad_segments_get_segment_t1(struct whisper_vad_segments* segments, int i_segment) {
    return segments && i_segment >= 0 && i_segment < (int)segments->seg.size() ? segments->seg[i_segment].second : 0.0f;
}
void whisper_vad_free_segments(struct whisper_vad_segments* segments) { delete segments; }
void whisper_vad_free(struct whisper_vad_context* ctx) { delete ctx; }

// ---- the VAD hooks of whisper_mi355x.h ------------------------------------------------------------------------------
double whisper_mi355x_vad_ms(struct whisper_state* s) { return s ? s->vad_ms : 0.0; }
int whisper_mi355x_vad_map(struct whisper_state* s, int job, int* out, int cap) {
    if (!s || job < 0 || cap < 0 || (cap > 0 && !out)) return -1;
    if (job >= (int)s->vad_maps.size()) return s->vad_maps.empty() && job < (int)s->results.size() ? 0 : -1;
    const std::vector<VadPiece>& t = s->vad_maps[job];
    for (int k = 0; k < (int)t.size() && k < cap; k++) {
        out[4 * k] = t[k].orig_start; out[4 * k + 1] = t[k].orig_end; out[4 * k + 2] = t[k].vad_start; out[4 * k + 3] = t[k].vad_end;
    }
    return (int)t.size();
}
int whisper_mi355x_vad_probs_batch(struct whisper_vad_context* vctx, const float* const* pcm, const int* n_samples, int n_clips,
                                   bool pcm_on_device, float* probs_out, int* n_probs) {
    if (!vctx || !pcm || !n_samples || !probs_out || !n_probs || n_clips < 1 || n_clips > 65535) return -1;
    for (int c = 0; c < n_clips; c++)
        if (n_samples[c] < 0 || (n_samples[c] > 0 && !pcm[c])) return -1;
    return guarded(nullptr, [&]() -> int {
        WM_CHECK(hipSetDevice(vctx->m->device));
        std::vector<std::vector<float>> probs;
        vad_probs_run(*vctx->m, vctx->sc, pcm, n_samples, n_clips, pcm_on_device, vctx->st, nullptr, probs, nullptr);
        size_t at = 0;
        for (int c = 0; c < n_clips; c++) {
            n_probs[c] = (int)probs[c].size();
            std::copy(probs[c].begin(), probs[c].end(), probs_out + at);
            at += probs[c].size();
        }
        return 0;
    });
}
int whisper_mi355x_debug_vad_frontend(struct whisper_vad_context* vctx, const float* pcm, int n_samples, float* xg_out) {
    if (!vctx || n_samples < 0 || (n_samples > 0 && (!pcm || !xg_out))) return -1;
    return guarded(nullptr, [&]() -> int {
        WM_CHECK(hipSetDevice(vctx->m->device));
        std::vector<std::vector<float>> probs;
        vad_probs_run(*vctx->m, vctx->sc, &pcm, &n_samples, 1, false, vctx->st, nullptr, probs, xg_out);
        return (int)probs[0].size();
    });
}
int whisper_mi355x_debug_vad_gather(struct whisper_context* ctx, const float* const* pcm, const int* n_samples, int n_clips,
                                    const int* pieces, const int* n_pieces, float* out) {
    if (!ctx || !pcm || !n_samples || !pieces || !n_pieces || !out || n_clips < 1 || n_clips > 65535) return -1;
    std::vector<std::vector<VadPiece>> tables(n_clips);
    const int* q = pieces;
    for (int c = 0; c < n_clips; c++) {
        if (n_samples[c] < 0 || n_pieces[c] < 0 || (n_samples[c] > 0 && !pcm[c])) return -1;
        int at = 0;  // every piece inside the clip, as long on both axes, and in order on the filtered one
        for (int k = 0; k < n_pieces[c]; k++, q += 4) {
            const VadPiece p{q[0], q[1], q[2], q[3]};
            if (p.orig_start < 0 || p.orig_end <= p.orig_start || p.orig_end > n_samples[c] || p.vad_start < at ||
                (long long)p.vad_end - p.vad_start != (long long)p.orig_end - p.orig_start)
                return -1;
            at = p.vad_end;
            tables[c].push_back(p);
        }
    }
    return guarded(nullptr, [&]() -> int {
        WM_CHECK(hipSetDevice(ctx->c.device));
        HookStream hs;
        struct Sc { VadScratch sc; ~Sc() { vad_scratch_free(sc); } } h;
        HookBufs b;
        std::vector<const float*> dev(n_clips, nullptr);
        for (int c = 0; c < n_clips; c++) {
            float* d = (float*)b.get(std::max<size_t>((size_t)n_samples[c], 1) * sizeof(float));
            if (n_samples[c] > 0) WM_CHECK(hipMemcpyAsync(d, pcm[c], (size_t)n_samples[c] * sizeof(float), hipMemcpyHostToDevice, hs.st));
            dev[c] = d;
        }
        std::vector<const float*> optr;
        std::vector<int> olen;
        vad_gather_run(h.sc, dev.data(), tables, hs.st, nullptr, optr, olen);
        size_t at = 0;
        for (int c = 0; c < n_clips; c++) {
            if (olen[c] > 0) WM_CHECK(hipMemcpy(out + at, optr[c], (size_t)olen[c] * sizeof(float), hipMemcpyDeviceToHost));
            at += (size_t)olen[c];
        }
        return (int)at;
    });
}

// ABI self-description (no device needed): sizes/offsets that a binding generator must agree on.
int whisper_mi355x_abi_layout(size_t out[8]) {
    out[0] = sizeof(whisper_full_params);
    out[1] = sizeof(whisper_context_params);
    out[2] = sizeof(whisper_token_data);
    out[3] = offsetof(whisper_full_params, initial_prompt);
    out[4] = offsetof(whisper_full_params, language);
    out[5] = offsetof(whisper_full_params, greedy);
    out[6] = offsetof(whisper_full_params, new_segment_callback);
    out[7] = offsetof(whisper_full_params, vad_params);
    return 8;
}
void* whisper_mi355x_dev_alloc(struct whisper_context* ctx, size_t bytes) {
    void* p = nullptr;
    hipSetDevice(ctx->c.device);
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
void whisper_mi355x_dev_free(struct whisper_context* ctx, void* p) { hipSetDevice(ctx->c.device); hipFree(p); }
int whisper_mi355x_memcpy(struct whisper_context* ctx, void* dst, const void* src, size_t bytes, int kind) {
    hipSetDevice(ctx->c.device);
    return hipMemcpy(dst, src, bytes, (hipMemcpyKind)kind) == hipSuccess ? 0 : -1;
}

}  // extern "C"
