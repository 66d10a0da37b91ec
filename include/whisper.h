/*
 * whisper.h — the C ABI that nobs-whisper_amd's libwhisper_mi355x.so exports.
 *
 * Drop-in boundary: the reference app never calls this header directly; it calls
 * whisper-rs 0.15.1 (src-tauri/src/whisper.rs:3), whose -sys crate 0.14.1 is a bindgen binding of
 * whisper.cpp's whisper.h (src-tauri/Cargo.lock:5641-5659). The declarations below restate that
 * header's types and functions (whisper.cpp ≈ v1.7.x, [ext]: not present offline) so a
 * whisper-rs-sys build can link this library instead of the CMake-built whisper.cpp. Each entry
 * point the reference reaches is annotated with the whisper.rs line that reaches it:
 *
 *   whisper.rs:39-40   WhisperContextParameters::default(), use_gpu(true)
 *                          -> whisper_context_default_params()
 *   whisper.rs:41-45   WhisperContext::new_with_params(path, params)
 *                          -> whisper_init_from_file_with_params_no_state()
 *   whisper.rs:55-59   drop of WhisperContext            -> whisper_free()
 *   whisper.rs:83-85   ctx.create_state()                -> whisper_init_state()
 *   whisper.rs:88      FullParams::new(Greedy{best_of:1}) -> whisper_full_default_params(GREEDY)
 *   whisper.rs:91-124  FullParams setters                -> plain field writes of whisper_full_params
 *   whisper.rs:127-129 state.full(params, &audio)        -> whisper_full_with_state()
 *   whisper.rs:132     state.full_n_segments()           -> whisper_full_n_segments_from_state()
 *   whisper.rs:136-137 state.get_segment(i).to_str_lossy()
 *                          -> whisper_full_get_segment_text_from_state()
 *   end of transcribe  drop of WhisperState              -> whisper_free_state()
 *
 * Struct layouts follow the upstream header field by field; they cannot be byte-checked against
 * whisper-rs-sys's generated bindings offline (SURVEY.md §7 hard part (i)). Functions of the
 * upstream header that this engine does not implement are exported as stubs that return an
 * error value, so a static link of whisper-rs resolves.
 *
 * Both sampling strategies are implemented. WHISPER_SAMPLING_BEAM_SEARCH (whisper-rs SamplingStrategy::BeamSearch)
 * keeps beam_size <= 8 hypotheses per window at t = 0 and extends each by its beam_size most probable tokens after
 * the logits rules, where upstream draws them from the softmax; patience is accepted and ignored; attempts at t > 0
 * are single sampled decoders, as with the greedy strategy (whisper_mi355x.h).
 *
 * whisper_full_params.token_timestamps, thold_pt, thold_ptsum, max_len and split_on_word are implemented (DESIGN.md §13,
 * whisper_mi355x.h). whisper_full_params.audio_ctx is implemented: the encoder, the cross K/V and every cross
 * attention of the call work on the first audio_ctx positions of each window; <= 0 = the model's n_audio_ctx, a value
 * above it makes whisper_full* return -5 (whisper_mi355x.h).
 *
 * whisper_full_params.suppress_nst and suppress_regex are implemented (whisper_mi355x.h): the tokens of
 * upstream's non-speech list, and every token whose whole string the pattern matches (std::regex, ECMAScript; NULL =
 * off), get a logit of -inf in every decoding mode. A pattern that does not compile makes whisper_full* return -8
 * before anything is encoded, with one line on stderr (upstream throws std::regex_error).
 *
 * whisper_full_params.grammar_rules, n_grammar_rules, i_start_rule and grammar_penalty are implemented (DESIGN.md §16,
 * whisper_mi355x.h) with upstream's semantics in every decoding mode: each decoder, beam and best_of candidate follows the
 * grammar from its start state, and every token the grammar rejects loses grammar_penalty before the token is chosen
 * (EOT too, unless the grammar may end there). n_grammar_rules == 0 or grammar_rules == NULL: no grammar. A malformed
 * grammar (a null rule, i_start_rule >= n_grammar_rules, a RULE_REF out of range, a CHAR_RNG_UPPER or CHAR_ALT that does
 * not follow a char class) or a left-recursive one (upstream recurses without end) makes whisper_full* return -9 before
 * anything is encoded, with one line on stderr.
 *
 * whisper_full_params.vad, vad_model_path and vad_params are implemented, and so is the whisper_vad_* block below
 * (whisper_mi355x.h): Silero VAD v5 (16 kHz) runs on the device ahead of the mel, whisper_full*,
 * whisper_full_parallel and whisper_mi355x_full_batch* transcribe the speech pieces only (laid end to end with 0.1 s of
 * silence between them; offset_ms / duration_ms apply to that filtered audio), and every segment and token time is mapped
 * back to the original audio. A clip in which no speech is found yields zero segments and 0. A null, unreadable or refused
 * vad_model_path makes whisper_full* return -11 before anything is encoded, with one line on stderr. The loaded VAD model
 * is cached per whisper_context, keyed by the path (upstream keeps it per state). vad == false (the default): the call
 * runs as before and launches no VAD kernel. The model file is ggml's legacy container as upstream's
 * convert-silero-vad-to-ggml.py writes it, restated in tools/make_vad_model.py; like the struct layouts, that layout
 * could not be checked against a real file offline.
 *
 * whisper_full_parallel is implemented (whisper_mi355x.h): the recording is cut into n_processors pieces
 * where upstream cuts it, the pieces are decoded side by side as one device batch on the default state (no threads, no
 * extra states), and their segments are merged with upstream's time shift. Unlike upstream, token times are shifted with
 * their segments. n_processors <= 1 is whisper_full; n_processors > 128 returns -1.
 *
 * whisper_full_params.logits_filter_callback is implemented (whisper_mi355x.h; whisper-rs
 * FullParams::set_filter_logits_callback). It is called as cb(ctx, state, tokens, n_tokens, logits, user_data) once per
 * decoder row per logits evaluation of whisper_full*, whisper_full_parallel and whisper_mi355x_full_batch* (greedy
 * decoders, every beam, every best_of candidate, fixed-work and forced runs; not from whisper_decode* or
 * whisper_lang_auto_detect*), on the calling thread, between two launches, with the state's stream drained; within a step
 * the rows are called in the order they were staged. ctx and state are those of the call. This engine's contract:
 *   - logits: n_vocab floats in host memory, valid during the call, any entry may be written (finite or -inf; not
 *     checked). Already applied: the temperature divide (in float, when t > 0), suppress_blank on the initial step (EOT and
 *     " "), <|notimestamps|>, no_timestamps, sot / nosp / solm (see tdrz_enable) / translate / transcribe / prev and the
 *     language tokens; every entry those rules did not touch is the raw logit bit for bit (divided when t > 0). They are
 *     not applied a second time: a callback that sets logits[sot] = 0 re-enables it, as upstream would.
 *   - applied after it, to the row as the callback left it: the deny mask of suppress_nst / suppress_regex, suppress_eot
 *     (fixed-work mode), timestamp pairing, max_initial_ts, monotonic timestamps, the log-softmax, the timestamp-mass
 *     rule, the grammar penalty and the choice. no_speech_prob stays that of the raw, undivided row.
 *   - tokens / n_tokens: the row's own sequence of this attempt (id, tid, p, plog, pt, ptsum; the rest as the getters
 *     report them mid-attempt), without the prompt; n_tokens == 0 on the prefill row; a beam gets its own re-parented
 *     history, a best_of candidate its own.
 * The order of the rules is the one of oracle/oracle_whisper.cpp's restatement of whisper_process_logits; the upstream
 * source could not be consulted offline. A call with a callback pays a host round trip of the rows per step and never
 * decodes pipelined; its decoder launches are chosen as without one. NULL (the default): nothing new is allocated or
 * launched. A batch above 128 clips runs as two halves on two threads: the second half's callbacks then come from its
 * thread, serialised with the first half's.
 *
 * whisper_full_params.tdrz_enable is implemented: with it <|solm|> is not suppressed, and a segment whose
 * token range holds one reports whisper_full_get_segment_speaker_turn_next* (and
 * whisper_mi355x_batch_segment_speaker_turn_next) = true; the token's text appears only with print_special. false (the
 * default): <|solm|> is suppressed and every segment reports false. No real tinydiarize model could be run offline: the
 * field is tested with a callback that raises the token's logit.
 *
 * No field of whisper_full_params is ignored any more, but beam_search.patience, which upstream ignores as well.
 */
#ifndef WHISPER_H
#define WHISPER_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WHISPER_API __attribute__((visibility("default")))

#define WHISPER_SAMPLE_RATE 16000
#define WHISPER_N_FFT       400
#define WHISPER_HOP_LENGTH  160
#define WHISPER_CHUNK_SIZE  30

struct whisper_context;
struct whisper_state;
struct whisper_full_params;

typedef int32_t whisper_pos;
typedef int32_t whisper_token;
typedef int32_t whisper_seq_id;

enum whisper_alignment_heads_preset {
    WHISPER_AHEADS_NONE,
    WHISPER_AHEADS_N_TOP_MOST,
    WHISPER_AHEADS_CUSTOM,
    WHISPER_AHEADS_TINY_EN,
    WHISPER_AHEADS_TINY,
    WHISPER_AHEADS_BASE_EN,
    WHISPER_AHEADS_BASE,
    WHISPER_AHEADS_SMALL_EN,
    WHISPER_AHEADS_SMALL,
    WHISPER_AHEADS_MEDIUM_EN,
    WHISPER_AHEADS_MEDIUM,
    WHISPER_AHEADS_LARGE_V1,
    WHISPER_AHEADS_LARGE_V2,
    WHISPER_AHEADS_LARGE_V3,
    WHISPER_AHEADS_LARGE_V3_TURBO,
};

typedef struct whisper_ahead {
    int n_text_layer;
    int n_head;
} whisper_ahead;

typedef struct whisper_aheads {
    size_t n_heads;
    const whisper_ahead * heads;
} whisper_aheads;

struct whisper_context_params {
    bool  use_gpu;
    bool  flash_attn;
    int   gpu_device;

    bool dtw_token_timestamps;
    enum whisper_alignment_heads_preset dtw_aheads_preset;

    int dtw_n_top;
    struct whisper_aheads dtw_aheads;

    size_t dtw_mem_size;
};

typedef struct whisper_token_data {
    whisper_token id;
    whisper_token tid;

    float p;
    float plog;
    float pt;
    float ptsum;

    int64_t t0;
    int64_t t1;
    int64_t t_dtw;

    float vlen;
} whisper_token_data;

typedef struct whisper_model_loader {
    void * context;
    size_t (*read)(void * ctx, void * output, size_t read_size);
    bool   (*eof)(void * ctx);
    void   (*close)(void * ctx);
} whisper_model_loader;

typedef struct whisper_timings {
    float sample_ms;
    float encode_ms;
    float decode_ms;
    float batchd_ms;
    float prompt_ms;
} whisper_timings;

enum whisper_gretype {
    WHISPER_GRETYPE_END            = 0,
    WHISPER_GRETYPE_ALT            = 1,
    WHISPER_GRETYPE_RULE_REF       = 2,
    WHISPER_GRETYPE_CHAR           = 3,
    WHISPER_GRETYPE_CHAR_NOT       = 4,
    WHISPER_GRETYPE_CHAR_RNG_UPPER = 5,
    WHISPER_GRETYPE_CHAR_ALT       = 6,
};

typedef struct whisper_grammar_element {
    enum whisper_gretype type;
    uint32_t             value;
} whisper_grammar_element;

typedef struct whisper_vad_params {
    float threshold;
    int   min_speech_duration_ms;
    int   min_silence_duration_ms;
    float max_speech_duration_s;
    int   speech_pad_ms;
    float samples_overlap;
} whisper_vad_params;

struct whisper_vad_context;
struct whisper_vad_segments;

typedef struct whisper_vad_context_params {
    int  n_threads;
    bool use_gpu;     /* accepted and ignored: the device path is the only one */
    int  gpu_device;
} whisper_vad_context_params;

enum whisper_sampling_strategy {
    WHISPER_SAMPLING_GREEDY,
    WHISPER_SAMPLING_BEAM_SEARCH,
};

typedef void (*whisper_new_segment_callback)(struct whisper_context * ctx, struct whisper_state * state, int n_new, void * user_data);
typedef void (*whisper_progress_callback)(struct whisper_context * ctx, struct whisper_state * state, int progress, void * user_data);
typedef bool (*whisper_encoder_begin_callback)(struct whisper_context * ctx, struct whisper_state * state, void * user_data);
typedef bool (*ggml_abort_callback)(void * data);
typedef void (*whisper_logits_filter_callback)(struct whisper_context * ctx, struct whisper_state * state,
                                               const whisper_token_data * tokens, int n_tokens, float * logits, void * user_data);

struct whisper_full_params {
    enum whisper_sampling_strategy strategy;

    int n_threads;
    int n_max_text_ctx;
    int offset_ms;
    int duration_ms;

    bool translate;
    bool no_context;
    bool no_timestamps;
    bool single_segment;
    bool print_special;
    bool print_progress;
    bool print_realtime;
    bool print_timestamps;

    bool  token_timestamps;
    float thold_pt;
    float thold_ptsum;
    int   max_len;
    bool  split_on_word;
    int   max_tokens;

    bool debug_mode;
    int  audio_ctx;

    bool tdrz_enable;

    const char * suppress_regex;

    const char * initial_prompt;
    const whisper_token * prompt_tokens;
    int prompt_n_tokens;

    const char * language;
    bool detect_language;

    bool suppress_blank;
    bool suppress_nst;

    float temperature;
    float max_initial_ts;
    float length_penalty;

    float temperature_inc;
    float entropy_thold;
    float logprob_thold;
    float no_speech_thold;

    struct {
        int best_of;
    } greedy;

    struct {
        int beam_size;
        float patience;
    } beam_search;

    whisper_new_segment_callback new_segment_callback;
    void * new_segment_callback_user_data;

    whisper_progress_callback progress_callback;
    void * progress_callback_user_data;

    whisper_encoder_begin_callback encoder_begin_callback;
    void * encoder_begin_callback_user_data;

    ggml_abort_callback abort_callback;
    void * abort_callback_user_data;

    whisper_logits_filter_callback logits_filter_callback;
    void * logits_filter_callback_user_data;

    const whisper_grammar_element ** grammar_rules;
    size_t                           n_grammar_rules;
    size_t                           i_start_rule;
    float                            grammar_penalty;

    bool         vad;
    const char * vad_model_path;
    whisper_vad_params vad_params;
};

/* ---- context / state lifetime ---------------------------------------------------------------- */
WHISPER_API const char * whisper_version(void);
WHISPER_API struct whisper_context * whisper_init_from_file_with_params(const char * path_model, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_from_buffer_with_params(void * buffer, size_t buffer_size, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_with_params(struct whisper_model_loader * loader, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_from_file_with_params_no_state(const char * path_model, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_from_buffer_with_params_no_state(void * buffer, size_t buffer_size, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_with_params_no_state(struct whisper_model_loader * loader, struct whisper_context_params params);
WHISPER_API struct whisper_state * whisper_init_state(struct whisper_context * ctx);
WHISPER_API int  whisper_ctx_init_openvino_encoder_with_state(struct whisper_context * ctx, struct whisper_state * state, const char * model_path, const char * device, const char * cache_dir);
WHISPER_API int  whisper_ctx_init_openvino_encoder(struct whisper_context * ctx, const char * model_path, const char * device, const char * cache_dir);
WHISPER_API void whisper_free(struct whisper_context * ctx);
WHISPER_API void whisper_free_state(struct whisper_state * state);
WHISPER_API void whisper_free_params(struct whisper_full_params * params);
WHISPER_API void whisper_free_context_params(struct whisper_context_params * params);

/* ---- mel / encode / decode ------------------------------------------------------------------- */
WHISPER_API int whisper_pcm_to_mel(struct whisper_context * ctx, const float * samples, int n_samples, int n_threads);
WHISPER_API int whisper_pcm_to_mel_with_state(struct whisper_context * ctx, struct whisper_state * state, const float * samples, int n_samples, int n_threads);
WHISPER_API int whisper_set_mel(struct whisper_context * ctx, const float * data, int n_len, int n_mel);
WHISPER_API int whisper_set_mel_with_state(struct whisper_context * ctx, struct whisper_state * state, const float * data, int n_len, int n_mel);
WHISPER_API int whisper_encode(struct whisper_context * ctx, int offset, int n_threads);
WHISPER_API int whisper_encode_with_state(struct whisper_context * ctx, struct whisper_state * state, int offset, int n_threads);
WHISPER_API int whisper_decode(struct whisper_context * ctx, const whisper_token * tokens, int n_tokens, int n_past, int n_threads);
WHISPER_API int whisper_decode_with_state(struct whisper_context * ctx, struct whisper_state * state, const whisper_token * tokens, int n_tokens, int n_past, int n_threads);

/* ---- tokens / languages ---------------------------------------------------------------------- */
WHISPER_API int whisper_tokenize(struct whisper_context * ctx, const char * text, whisper_token * tokens, int n_max_tokens);
WHISPER_API int whisper_token_count(struct whisper_context * ctx, const char * text);
WHISPER_API int whisper_lang_max_id(void);
WHISPER_API int whisper_lang_id(const char * lang);
WHISPER_API const char * whisper_lang_str(int id);
WHISPER_API const char * whisper_lang_str_full(int id);
WHISPER_API int whisper_lang_auto_detect(struct whisper_context * ctx, int offset_ms, int n_threads, float * lang_probs);
WHISPER_API int whisper_lang_auto_detect_with_state(struct whisper_context * ctx, struct whisper_state * state, int offset_ms, int n_threads, float * lang_probs);

WHISPER_API int whisper_n_len(struct whisper_context * ctx);
WHISPER_API int whisper_n_len_from_state(struct whisper_state * state);
WHISPER_API int whisper_n_vocab(struct whisper_context * ctx);
WHISPER_API int whisper_n_text_ctx(struct whisper_context * ctx);
WHISPER_API int whisper_n_audio_ctx(struct whisper_context * ctx);
WHISPER_API int whisper_is_multilingual(struct whisper_context * ctx);

WHISPER_API int whisper_model_n_vocab(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_ctx(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_state(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_head(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_layer(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_ctx(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_state(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_head(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_layer(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_mels(struct whisper_context * ctx);
WHISPER_API int whisper_model_ftype(struct whisper_context * ctx);
WHISPER_API int whisper_model_type(struct whisper_context * ctx);
WHISPER_API const char * whisper_model_type_readable(struct whisper_context * ctx);

WHISPER_API float * whisper_get_logits(struct whisper_context * ctx);
WHISPER_API float * whisper_get_logits_from_state(struct whisper_state * state);

WHISPER_API const char * whisper_token_to_str(struct whisper_context * ctx, whisper_token token);
WHISPER_API whisper_token whisper_token_eot(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_sot(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_solm(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_prev(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_nosp(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_not(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_beg(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_lang(struct whisper_context * ctx, int lang_id);
WHISPER_API whisper_token whisper_token_translate(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_transcribe(struct whisper_context * ctx);

/* ---- timings / system ------------------------------------------------------------------------ */
WHISPER_API struct whisper_timings * whisper_get_timings(struct whisper_context * ctx);
WHISPER_API void whisper_print_timings(struct whisper_context * ctx);
WHISPER_API void whisper_reset_timings(struct whisper_context * ctx);
WHISPER_API const char * whisper_print_system_info(void);

/* ---- full transcription ---------------------------------------------------------------------- */
WHISPER_API struct whisper_context_params * whisper_context_default_params_by_ref(void);
WHISPER_API struct whisper_context_params   whisper_context_default_params(void);
WHISPER_API struct whisper_full_params * whisper_full_default_params_by_ref(enum whisper_sampling_strategy strategy);
WHISPER_API struct whisper_full_params   whisper_full_default_params(enum whisper_sampling_strategy strategy);

WHISPER_API int whisper_full(struct whisper_context * ctx, struct whisper_full_params params, const float * samples, int n_samples);
WHISPER_API int whisper_full_with_state(struct whisper_context * ctx, struct whisper_state * state, struct whisper_full_params params, const float * samples, int n_samples);
WHISPER_API int whisper_full_parallel(struct whisper_context * ctx, struct whisper_full_params params, const float * samples, int n_samples, int n_processors);

WHISPER_API int whisper_full_n_segments(struct whisper_context * ctx);
WHISPER_API int whisper_full_n_segments_from_state(struct whisper_state * state);
WHISPER_API int whisper_full_lang_id(struct whisper_context * ctx);
WHISPER_API int whisper_full_lang_id_from_state(struct whisper_state * state);
WHISPER_API int64_t whisper_full_get_segment_t0(struct whisper_context * ctx, int i_segment);
WHISPER_API int64_t whisper_full_get_segment_t0_from_state(struct whisper_state * state, int i_segment);
WHISPER_API int64_t whisper_full_get_segment_t1(struct whisper_context * ctx, int i_segment);
WHISPER_API int64_t whisper_full_get_segment_t1_from_state(struct whisper_state * state, int i_segment);
WHISPER_API bool whisper_full_get_segment_speaker_turn_next(struct whisper_context * ctx, int i_segment);
WHISPER_API bool whisper_full_get_segment_speaker_turn_next_from_state(struct whisper_state * state, int i_segment);
WHISPER_API const char * whisper_full_get_segment_text(struct whisper_context * ctx, int i_segment);
WHISPER_API const char * whisper_full_get_segment_text_from_state(struct whisper_state * state, int i_segment);
WHISPER_API int whisper_full_n_tokens(struct whisper_context * ctx, int i_segment);
WHISPER_API int whisper_full_n_tokens_from_state(struct whisper_state * state, int i_segment);
WHISPER_API const char * whisper_full_get_token_text(struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API const char * whisper_full_get_token_text_from_state(struct whisper_context * ctx, struct whisper_state * state, int i_segment, int i_token);
WHISPER_API whisper_token whisper_full_get_token_id(struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API whisper_token whisper_full_get_token_id_from_state(struct whisper_state * state, int i_segment, int i_token);
WHISPER_API whisper_token_data whisper_full_get_token_data(struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API whisper_token_data whisper_full_get_token_data_from_state(struct whisper_state * state, int i_segment, int i_token);
WHISPER_API float whisper_full_get_token_p(struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API float whisper_full_get_token_p_from_state(struct whisper_state * state, int i_segment, int i_token);
WHISPER_API float whisper_full_get_segment_no_speech_prob(struct whisper_context * ctx, int i_segment);
WHISPER_API float whisper_full_get_segment_no_speech_prob_from_state(struct whisper_state * state, int i_segment);

/* ---- voice activity detection (Silero VAD v5, 16 kHz) ------------------------------- */
/* Defaults: threshold 0.5, min_speech_duration_ms 250, min_silence_duration_ms 100, max_speech_duration_s FLT_MAX,
 * speech_pad_ms 30, samples_overlap 0.1; context: n_threads 4, use_gpu true, gpu_device 0. A probability covers 512
 * samples (32 ms); the LSTM state starts at zero with every whisper_vad_detect_speech call. Segment times t0 / t1 are in
 * 10 ms units, like every other time of this header, and so whisper-rs documents them (centiseconds); upstream releases
 * have differed here (seconds in some), which cannot be checked offline. An init function returns NULL, with one line
 * on stderr, for a file that is unreadable, truncated, of another geometry than v5 at 16 kHz, or that lacks, repeats or
 * misshapes a tensor. */
WHISPER_API struct whisper_vad_params         whisper_vad_default_params(void);
WHISPER_API struct whisper_vad_context_params whisper_vad_default_context_params(void);
WHISPER_API struct whisper_vad_context * whisper_vad_init_from_file_with_params(const char * path_model, struct whisper_vad_context_params params);
WHISPER_API struct whisper_vad_context * whisper_vad_init_with_params(struct whisper_model_loader * loader, struct whisper_vad_context_params params);
WHISPER_API bool    whisper_vad_detect_speech(struct whisper_vad_context * vctx, const float * samples, int n_samples);
WHISPER_API int     whisper_vad_n_probs(struct whisper_vad_context * vctx);
WHISPER_API float * whisper_vad_probs(struct whisper_vad_context * vctx);
WHISPER_API struct whisper_vad_segments * whisper_vad_segments_from_probs(struct whisper_vad_context * vctx, struct whisper_vad_params params);
WHISPER_API struct whisper_vad_segments * whisper_vad_segments_from_samples(struct whisper_vad_context * vctx, struct whisper_vad_params params, const float * samples, int n_samples);
WHISPER_API int   whisper_vad_segments_n_segments(struct whisper_vad_segments * segments);
WHISPER_API float whisper_vad_segments_get_segment_t0(struct whisper_vad_segments * segments, int i_segment);
WHISPER_API float whisper_vad_segments_get_segment_t1(struct whisper_vad_segments * segments, int i_segment);
WHISPER_API void  whisper_vad_free_segments(struct whisper_vad_segments * segments);
WHISPER_API void  whisper_vad_free(struct whisper_vad_context * ctx);

/* ---- benchmarks / logging -------------------------------------------------------------------- */
WHISPER_API int whisper_bench_memcpy(int n_threads);
WHISPER_API const char * whisper_bench_memcpy_str(int n_threads);
WHISPER_API int whisper_bench_ggml_mul_mat(int n_threads);
WHISPER_API const char * whisper_bench_ggml_mul_mat_str(int n_threads);
typedef void (*ggml_log_callback)(int level, const char * text, void * user_data);
WHISPER_API void whisper_log_set(ggml_log_callback log_callback, void * user_data);

#ifdef __cplusplus
}
#endif

#endif /* WHISPER_H */
