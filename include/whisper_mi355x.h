/*
 * whisper_mi355x.h — additive extensions of the whisper.h ABI for MI355X (SURVEY.md §8b
 * "Additive batch extension"). The reference calls one clip at a time
 * (src-tauri/src/whisper.rs:150-151: "GPU can only process one at a time"); these entry points
 * let a caller hand over many independent 30 s chunks at once, keep PCM resident in HBM, pick
 * the compute type, and broadcast weights to the other GPUs of a node over RCCL/xGMI.
 * Nothing here replaces a reference interface; whisper.h's functions are unchanged.
 */
#ifndef WHISPER_MI355X_H
#define WHISPER_MI355X_H

#include "whisper.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Return code of every entry point below (and of whisper_full_with_state / whisper_pcm_to_mel /
 * whisper_encode / whisper_decode) when the engine hit a device error (a HIP error such as out of
 * memory) or an unsupported shape: the call is abandoned, nothing is aborted, and the context and
 * the state stay usable (whisper.rs:127-129 maps any non-zero return to TranscriptionError). */
#define WHISPER_MI355X_ERR_RUNTIME (-10)

/* compute type of weights and GEMM activations. FP8_ENC: bf16, with the encoder's QKV, FC1 and FC2
 * GEMMs on OCP e4m3 weights and activations (per-row f32 scales; the large-v3-turbo fp8 config).
 * FP8_ENC is a throughput mode, not a whisper.cpp-parity mode. */
enum whisper_mi355x_dtype { WHISPER_MI355X_F16 = 0, WHISPER_MI355X_BF16 = 1, WHISPER_MI355X_FP8_ENC = 2 };

/* Context on HIP device `gpu_device` (from params) with an explicit compute type.
 * load_weights = false: parse the file and allocate the device weight arena without filling it
 * (a rank that receives the weights by whisper_mi355x_broadcast_weights). */
WHISPER_API struct whisper_context * whisper_mi355x_init(const char * path_model, struct whisper_context_params params,
                                                         int dtype, bool load_weights);

/* Device weight arena (one contiguous allocation holding every converted tensor). */
WHISPER_API int whisper_mi355x_weight_arena(struct whisper_context * ctx, void ** dev_ptr, size_t * bytes);

/* RCCL (rccl.h) unique id for a weight broadcast: filled by rank 0, shipped to the other ranks by
 * the caller (any side channel), then every rank calls whisper_mi355x_broadcast_weights. */
WHISPER_API int whisper_mi355x_rccl_unique_id(char out[128]);
WHISPER_API int whisper_mi355x_broadcast_weights(struct whisper_context * ctx, const char unique_id[128], int rank, int world);

/* Batched whisper_full: n_jobs independent clips, each processed exactly as one
 * whisper_full_with_state call on a fresh state would process it. pcm[j] points at n_samples[j]
 * f32 samples, on the host (pcm_on_device = false) or already in this context's HBM (true).
 * Fixed-work benchmark mode: fixed_tokens > 0 decodes exactly that many tokens per window with EOT
 * suppressed and no temperature fallback; at most n_text_ctx / 2 - 4 (a window's limit,
 * 220), else -1. Returns 0 on success.
 * Beam search (params.strategy = WHISPER_SAMPLING_BEAM_SEARCH, here and in whisper_full*): the t = 0 attempt of
 * every window decodes beam_size hypotheses per clip, each beam's candidates being its beam_size most probable
 * tokens after the logits rules (upstream samples them); patience is ignored. beam_size < 1 counts
 * as 1 (the greedy result, bit for bit), beam_size > 8 returns -4. With beam_size > 1 every live beam of every clip
 * is one row of a cache-form decode step: n_jobs * beam_size <= 32, else -1 (one stderr line). fixed_tokens > 0
 * with the beam strategy returns -1.
 * Sampled attempts (t > 0, the temperature fallback) under both strategies decode N = max(1, greedy.best_of)
 * candidates per clip and keep the best-scoring one, as upstream does. N = 1: one decoder sampled on
 * the host with std::discrete_distribution. N > 1: the candidates are rows of one cache-form decode step, their
 * tokens drawn on the device from a counter-based generator (whisper_mi355x_set_sample_seed); this needs
 * n_jobs * N <= 32, a larger batch samples one host candidate per clip as with N = 1 (one stderr line). N > 8
 * returns -4. Attempts at t = 0 do not depend on best_of. */
WHISPER_API int whisper_mi355x_full_batch(struct whisper_context * ctx, struct whisper_state * state,
                                          struct whisper_full_params params, const float * const * pcm,
                                          const int * n_samples, int n_jobs, bool pcm_on_device, int fixed_tokens);
/* Parity-test hook: the fixed-work batch with teacher forcing. The token decoded after step i of job j
 * is forced[j * fixed_tokens + i] (whatever the logits rules chose), and the raw logits of the jobs
 * spot[0..n_spot) at every step i (step 0 = the prefill) go to spot_logits[(i * n_spot + k) * n_vocab]
 * (host memory, fixed_tokens * n_spot * n_vocab floats). The kernels are the ones whisper_mi355x_full_batch
 * runs on the same batch (above 128 jobs: two concurrent halves, each forced and spot-copied by its own
 * jobs). */
WHISPER_API int whisper_mi355x_full_batch_forced(struct whisper_context * ctx, struct whisper_state * state,
                                                 struct whisper_full_params params, const float * const * pcm,
                                                 const int * n_samples, int n_jobs, bool pcm_on_device, int fixed_tokens,
                                                 const int * forced, const int * spot, int n_spot, float * spot_logits);
/* Beam `beam` of the last beam-searched window (the t = 0 attempt) of job `job` of the last full / full_batch call
 * (job 0 for whisper_full_with_state): its tokens as decoded (before the cut at result_len; at most cap are
 * copied), its sum of token log-probabilities, and flags: bit 0 completed, bit 1 failed, bit 2 the window's
 * winner. Returns the token count, or -1 when there is no such beam (greedy strategy, no window decoded). */
#define WHISPER_MI355X_BEAM_COMPLETED 1
#define WHISPER_MI355X_BEAM_FAILED 2
#define WHISPER_MI355X_BEAM_WINNER 4
WHISPER_API int whisper_mi355x_beam_info(struct whisper_state * state, int job, int beam, int * tokens, int cap,
                                         double * sum_logprobs_all, int * flags);
/* Candidate `cand` of the last sampled attempt with best_of > 1 candidates (device-drawn, see above) of job `job`
 * of the last full / full_batch call: tokens, sum and flags as whisper_mi355x_beam_info reports a beam. Returns the
 * token count, or -1 when there is no such candidate (no sampled attempt, best_of <= 1, or the host path). */
WHISPER_API int whisper_mi355x_cand_info(struct whisper_state * state, int job, int cand, int * tokens, int cap,
                                         double * sum_logprobs_all, int * flags);
/* Seed of the device-side draws of this state's sampled candidates (default 0; a recycled state starts at 0 again).
 * The draw of token i of candidate c in the attempt at temperature index k of the window at `seek` (10 ms frames)
 * is Philox4x32-10 word 0 of counter (0, seek, 16 k + c, i) under key (seed lo, seed hi): it does not depend on
 * other clips, attempts or calls. */
WHISPER_API void whisper_mi355x_set_sample_seed(struct whisper_state * state, uint64_t seed);
WHISPER_API int whisper_mi355x_batch_n_segments(struct whisper_state * state, int job);
WHISPER_API const char * whisper_mi355x_batch_segment_text(struct whisper_state * state, int job, int i_segment);
WHISPER_API int64_t whisper_mi355x_batch_segment_t0(struct whisper_state * state, int job, int i_segment);
WHISPER_API int64_t whisper_mi355x_batch_segment_t1(struct whisper_state * state, int job, int i_segment);
WHISPER_API int whisper_mi355x_batch_segment_n_tokens(struct whisper_state * state, int job, int i_segment);
WHISPER_API whisper_token_data whisper_mi355x_batch_token_data(struct whisper_state * state, int job, int i_segment, int i_token);
/* whisper_full_get_segment_speaker_turn_next for a clip of the batch (whisper_full_params.tdrz_enable; false when off) */
WHISPER_API bool whisper_mi355x_batch_segment_speaker_turn_next(struct whisper_state * state, int job, int i_segment);
WHISPER_API int whisper_mi355x_batch_lang_id(struct whisper_state * state, int job);
/* tokens generated (all decode steps, all attempts) by the last whisper_mi355x_full_batch */
WHISPER_API long whisper_mi355x_batch_decoded_tokens(struct whisper_state * state);
/* tokens generated by every whisper_full / whisper_mi355x_full_batch call of the process so far (lets a
 * caller that drives whisper.h through its own states, e.g. the WhisperEngine mirror, count per call) */
WHISPER_API long whisper_mi355x_decoded_tokens_total(void);
/* Debug: device pointers of a state's decode workspace (0 residual x, 1 final LayerNorm rows, 2 unused (NULL),
 * 3 attention outputs, 4 GELU rows, 5 cross q, 6 Q', 7 cross-attention partials, 8 their {m, l}); NULL when
 * not allocated. */
WHISPER_API void * whisper_mi355x_debug_ws(struct whisper_state * state, int which);

/* Per-window decisions of whisper_full's temperature-fallback loop (the integer outcomes that are
 * comparable with whisper.cpp even when a sampled t > 0 attempt is not): one record per decoded
 * 30 s window, in seek order. temp_idx: index of the temperature finally used (0 = greedy t = 0
 * succeeded); n_attempts = temp_idx + 1; failed0: the t = 0 attempt failed (timestamp rule or
 * entropy < entropy_thold); logprob_fail0: its avg_logprob < logprob_thold; result_len0,
 * avg_logprob0, entropy0: that attempt's sequence score inputs; no_speech: the window was
 * dropped as silence. job = 0 for whisper_full_with_state. Returns the record count (or -count
 * when cap is too small). */
struct whisper_mi355x_window_decision {
    int32_t seek;
    int32_t temp_idx;
    int32_t failed0;
    int32_t logprob_fail0;
    int32_t result_len0;
    int32_t no_speech;
    float   avg_logprob0;
    float   entropy0;
    float   no_speech_prob;
    float   pad;
};
WHISPER_API int whisper_mi355x_window_decisions(struct whisper_state * state, int job,
                                                struct whisper_mi355x_window_decision * out, int cap);

/* whisper_full_parallel as one device batch. The recording is cut as upstream cuts it: with
 * offset_samples = 16000 * offset_ms / 1000 and n_per = (n_samples - offset_samples) / n_processors (int arithmetic),
 * piece 0 is [0, offset_samples + n_per) with the caller's params, piece k >= 1 starts at cut_k = offset_samples +
 * k * n_per with offset_ms = 0 and no new-segment or progress callback, and the last piece runs to n_samples;
 * duration_ms, encoder_begin_callback and abort_callback hold for every piece. The pieces are the jobs of one batch on
 * `state` (beam search with n_processors * beam_size > 32: consecutive groups of 32 / beam_size jobs): piece 0 is decoded
 * as whisper_full_with_state on `state` decodes it (carried prompt, rng, language, live callbacks), every other piece
 * as on a fresh state. The results are merged in piece order into what the whisper_full_*_from_state getters of `state`
 * see: a segment of piece k >= 1 gains 100 * (cut_k - offset_samples) / 16000 + offset_ms / 10 on t0 and t1, then t0 =
 * max(t0, t1 of the segment before it), and new_segment_callback is called with n_new = 1 after each one. Unlike
 * upstream, which leaves them relative to the piece, every token t0 / t1 / t_dtw that is not -1 gains the same amount
 * (unclamped). whisper_mi355x_window_decisions(state, 0, ..) gives the pieces' records in piece order, seek shifted
 * alike. n_processors <= 1 (or n_per <= 0) is whisper_full_with_state; n_processors > 128 returns -1 (one stderr line).
 * A group's error code is returned at once.
 * snap_ms > 0 moves every interior cut to the quietest 20 ms near it: of the 320-sample windows w that lie wholly
 * inside the recording with |320 w - cut_k| <= 16 * snap, snap = min(snap_ms, 1000 * (n_per / 2 - 320) / 16000) (not
 * positive: nothing moves), the one with the lowest RMS (the device pass of whisper_mi355x_find_silence_boundaries;
 * ties: the smaller |320 w - cut_k|, then the smaller w) gives the new cut 320 w + 160. Piece lengths and time shifts
 * follow the moved cuts. whisper_full_parallel is this call with the default state, snap_ms = 0 and host PCM.
 * whisper_mi355x_parallel_cuts: the piece starts (samples; cuts[0] = 0) of the last such call on the state; returns
 * their count (at most cap are copied). */
WHISPER_API int whisper_mi355x_full_parallel(struct whisper_context * ctx, struct whisper_state * state,
                                             struct whisper_full_params params, const float * pcm, int n_samples,
                                             int n_processors, int snap_ms, bool pcm_on_device);
WHISPER_API int whisper_mi355x_parallel_cuts(struct whisper_state * state, int * cuts, int cap);

/* Phase timings of the last full/full_batch call, milliseconds (host wall clock around
 * stream-synchronised phases): mel, encode (incl. cross-KV), prefill, decode steps, logits. */
WHISPER_API int whisper_mi355x_phase_ms(struct whisper_state * state, double out[5]);

/* Token-level timestamps from cross-attention DTW (whisper_context_params.dtw_token_timestamps with an
 * alignment-heads preset, dtw_n_top or dtw_aheads; DESIGN.md "Token timestamps (DTW)"). Every text token of an
 * aligned window carries whisper_token_data.t_dtw (10 ms units, as t0 / t1) through whisper_full_get_token_data*
 * and whisper_mi355x_batch_token_data; every other token has t_dtw = -1. An invalid configuration (preset NONE,
 * an empty list, dtw_n_top outside [1, n_text_layer], a head outside the model) makes the init return NULL.
 * whisper_mi355x_align_ms: wall time of the alignment passes of the last full / full_batch call (0 with the
 * switch off; not part of whisper_mi355x_phase_ms' five slots).
 * whisper_mi355x_align_cost: the cost matrix [rows][frames] (f32; rows = the `not` row + the text tokens) of the
 * job's last aligned window, copied from the device buffer the DTW kernel read. *rows = 0 when no window of the
 * job was aligned. Returns 0, -1 on bad arguments, -2 when cap_floats is too small (rows / frames are set). */
WHISPER_API double whisper_mi355x_align_ms(struct whisper_state * state);
WHISPER_API int whisper_mi355x_align_cost(struct whisper_state * state, int job, float * out, long cap_floats,
                                          int * rows, int * frames);

/* Per-token t0 / t1 / vlen and line-length-limited segments (whisper_full_params.token_timestamps, thold_pt,
 * thold_ptsum, max_len, split_on_word; whisper-rs set_token_timestamps, set_max_len, set_split_on_word).
 * With token_timestamps set, every token of whisper_full_get_token_data* and whisper_mi355x_batch_token_data carries
 * t0, t1 (10 ms units, absolute within the clip) and vlen: placed from the timestamp tokens, the intervals between them
 * spread by voice length, then adjusted on the clip's smoothed energy signal (a 65-tap mean of |pcm|, computed on the
 * device once per call); with max_len > 0 as well, every segment is cut into pieces of at most max_len bytes of text
 * (split_on_word: only before a token that starts with a space), and the segment getters, whisper_full_n_segments and
 * the new-segment callback's n_new see the pieces. Without token_timestamps the five fields change nothing: t0 = t1 =
 * -1, vlen = 0, no segment is cut.
 * whisper_mi355x_token_times_ms: wall time of these passes in the last full / full_batch call (0 when off; not part
 * of whisper_mi355x_phase_ms' five slots). */
WHISPER_API double whisper_mi355x_token_times_ms(struct whisper_state * state);
/* Debug: the two token-time kernels (kernels/tokts.hip) on caller data, host pointers, one launch each.
 * Clips are concatenated: clip c of n_samples[c] >= 1 samples starts at the running offset rounded up to 64 floats,
 * in pcm, energy and energy_out alike (so each holds sum of n_samples[c] rounded up to 64 floats).
 * signal_energy: energy_out[i] = (sum_{j=-32..32, inside the clip} |pcm[i + j]|) / 65.0f per clip, the f32 sum taken
 * from 0.0f in ascending j (the padding between clips comes back as 0).
 * token_vad: segment q of seg_n_tokens[q] >= 2 tokens belongs to clip seg_clip[q]; spans holds the segments' tokens
 * back to back, in / out: t0, t1 in 10 ms units, is_text = 0 for a token the pass leaves as it is (ids >= eot).
 * Both return 0, or -1 on bad arguments (a clip index out of range, n_samples < 1, a segment of fewer than 2 tokens),
 * and then launch nothing. */
struct whisper_mi355x_token_span {
    int64_t t0, t1;
    int32_t is_text, pad;
};
WHISPER_API int whisper_mi355x_debug_signal_energy(struct whisper_context * ctx, const float * pcm, const int * n_samples,
                                                   int n_clips, float * energy_out);
WHISPER_API int whisper_mi355x_debug_token_vad(struct whisper_context * ctx, const float * energy, const int * n_samples,
                                               int n_clips, const int * seg_clip, const int * seg_n_tokens, int n_segs,
                                               struct whisper_mi355x_token_span * spans);

/* Normalised log-mel of the last whisper_pcm_to_mel_with_state / whisper_full_with_state call,
 * copied to host: [n_mel][n_len] f32. Returns n_len. */
WHISPER_API int whisper_mi355x_get_mel(struct whisper_state * state, float * out, int cap_floats);
/* Encoder output (ln_post) of window 0 of the last encode, [A][n_audio_state] f32; A = the state's audio context
 * (n_audio_ctx unless whisper_full_params.audio_ctx / whisper_mi355x_set_audio_ctx shortened it). */
WHISPER_API int whisper_mi355x_get_encoder_out(struct whisper_state * state, float * out, int cap_floats);
/* The state's audio context (whisper.cpp's exp_n_audio_ctx) for the low-level API: whisper_encode_with_state,
 * whisper_decode_with_state and whisper_lang_auto_detect_with_state work on the first audio_ctx encoder positions of
 * a window (the mel window is 2 * audio_ctx frames, zero past it); <= 0 = the model's n_audio_ctx. whisper_full_with_state
 * stores its params.audio_ctx here after its language detection; a new state, and one from the context's pool, start
 * at 0. Set it before the encode whose output the decode calls read. Returns 0, -5 when audio_ctx > n_audio_ctx (the
 * value is then left as it was), -1 for a null state or one whose context was freed. */
WHISPER_API int whisper_mi355x_set_audio_ctx(struct whisper_state * state, int audio_ctx);

/* Live per-kernel-class timing with HIP events on the state's stream (used by bench.py for the
 * roofline). Classes: 0 encoder-side GEMM (work = FLOPs), 1 encoder attention (FLOPs),
 * 2 decoder cross-attention (HBM bytes), 3 decoder self-attention (bytes), 4 decoder GEMM (bytes),
 * 5 logits processing (bytes), 6 mel (bytes), 7 the persistent decode step (bytes), 8 prefill attention
 * (bytes), 9 / 10 / 11 the token-timestamp alignment's score (FLOPs), cost (bytes) and DTW (bytes) kernels,
 * 12 beam search's top-k logits kernel (bytes), 13 its self-cache gather (bytes read + written),
 * 14 the sampled draw of best_of candidates (bytes: two passes over the rows' probs),
 * 15 the token-time kernels (signal energy and the voice-activity adjust; bytes),
 * 16 the grammar's reject kernel (bytes), 17 the three VAD kernels (whisper_full_params.vad; bytes). The bits of
 * classes 16 and 17 lie in the layer-stride field below: time them with classes 2 and 3 off.
 * class_mask bit k times class k (0 = off); bits 16..23, when > 1, time
 * the decoder's per-layer attention launches (classes 2, 3) of every k-th layer only.
 * Every call resets the counters; stats out = {total ms, launches, total work}. */
WHISPER_API int whisper_mi355x_kernel_timing(struct whisper_state * state, int class_mask);
WHISPER_API int whisper_mi355x_kernel_stats(struct whisper_state * state, int cls, double out[3]);
/* Pseudo class of whisper_mi355x_kernel_stats: out = {ms lost, give-ups, 0} of the persistent decode step
 * (kernels/pdec.hip) on this state since it was created (or recycled): a launch that gave up (not all of its
 * 256 workgroups became resident within the wait limit, e.g. another process held CUs) is re-run on the
 * per-kernel path, and the state's next steps take that path for about a second. Not reset by
 * whisper_mi355x_kernel_timing. whisper_mi355x_pdec_give_ups returns the count alone (NULL: the total of every
 * state of the process). */
#define WHISPER_MI355X_KSTAT_PDEC_GIVE_UPS 100
WHISPER_API long whisper_mi355x_pdec_give_ups(struct whisper_state * state);
/* Pseudo class of whisper_mi355x_kernel_stats: out = {bytes the self-cache gather of beam search copied on this
 * state since it was created (or recycled), the bytes whole-sequence copies would have been (no common-prefix
 * rule), 0}. Not reset by whisper_mi355x_kernel_timing. */
#define WHISPER_MI355X_KSTAT_BEAM_GATHER 101
/* Pseudo classes of whisper_mi355x_kernel_stats: class 17 (the VAD kernels) by kernel, out as for a class: vad_frontend,
 * vad_lstm (with the head), vad_gather. Filled when class 17 is timed, reset with it. */
#define WHISPER_MI355X_KSTAT_VAD_FRONTEND 102
#define WHISPER_MI355X_KSTAT_VAD_LSTM 103
#define WHISPER_MI355X_KSTAT_VAD_GATHER 104
/* The stage kernel of whisper_full_params.logits_filter_callback (kernel-timing class 18, work in bytes: 8 per logit),
 * out as for a class: one launch per logits launch of a call with a callback (but the top-k pass of a beam attempt's
 * prefill, which reads the rows the prefill's greedy pass staged: one callback per row), none in a call without one. */
#define WHISPER_MI355X_KSTAT_LOGITS_STAGE 105

/* Kernel-level test/tuning hooks (device pointers): one fused-epilogue GEMM launch of the engine
 * (epi as in kernels.h: 0 store, 1 gelu, 2 residual f32, 4 f32, 5 cross K/V: out is then a cross cache of
 * M / n_audio_ctx slots for N / 2K layers, K = d), averaged over reps; and the
 * GEMM variant override: -1 auto; 0 register-staged kernels only; 1 LDS-DMA, 128x128 tiles in place of the
 * 256x256 phase-interleaved kernel; >= 2 the 256x256 phase-interleaved kernel wherever the shape is big. */
WHISPER_API int whisper_mi355x_debug_gemm(struct whisper_context * ctx, int epi, const void * A, int M, int K,
                                          const void * B, int N, const float * bias, void * out, int reps, float * ms);
WHISPER_API void whisper_mi355x_set_gemm_variant(int variant);
/* debug: device buffer of [grid][4] u64 the encoder GEMM kernel fills with s_memtime stamps (entry, main loop
 * start / end, epilogue end) per workgroup; null turns it off */
WHISPER_API void whisper_mi355x_set_gemm_stamps(void * dev);
/* Debug/tuning: the small-M decode GEMM (M <= 32, K % 256 == 0): out = A.B^T + bias with epilogue epi
 * (2 residual: out f32 += ..., 4 f32, 0 store, 1 gelu); with ln_w != NULL, A is f32 [M][K] and the
 * product uses LN(A) * ln_w + ln_b (K <= 1280). The first launch's result stays in out; reps more
 * launches are timed (note: epi 2 accumulates into out on every launch). */
WHISPER_API int whisper_mi355x_debug_gemm_small(struct whisper_context * ctx, int epi, const void * A, int M, int K,
                                                const void * B, int N, const float * bias, void * out,
                                                const float * ln_w, const float * ln_b, int reps, float * ms);
/* Test hooks for GGML block-quantized weights (device pointers). A matrix [rows][K] (K % 32 == 0) of ggml type
 * `type` (2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0) is given as the engine keeps it, the file's blocks regrouped by
 * field, row-major: qs = the quant bytes [rows][K/2] ([rows][K] for q8_0), qh = the q5 high bits, one u32 per
 * block [rows][K/32] (NULL for the other types), dm = the f16 scale d per block [rows][K/32], or d then m
 * [rows][K/32][2] for the *_1 types.
 * debug_dequant: out[rows][K] (the context's compute type) = the dequantized weights, one launch.
 * debug_dequant_multi: n <= 6 such matrices by one launch (the per-layer form); all of one type, else nonzero.
 * debug_gemm_small_q: whisper_mi355x_debug_gemm_small with B given as blocks [N][K], one launch; with epi 0
 * every output column is multiplied by scale before it is rounded. */
WHISPER_API int whisper_mi355x_debug_dequant(struct whisper_context * ctx, int type, const void * qs, const void * qh,
                                             const void * dm, long rows, int K, void * out);
WHISPER_API int whisper_mi355x_debug_dequant_multi(struct whisper_context * ctx, const int * type, int n,
                                                   const void * const * qs, const void * const * qh,
                                                   const void * const * dm, const long * rows, const int * K,
                                                   void * const * out);
WHISPER_API int whisper_mi355x_debug_gemm_small_q(struct whisper_context * ctx, int epi, const void * A, int M, int K,
                                                  int type, const void * qs, const void * qh, const void * dm, int N,
                                                  const float * bias, float scale, void * out, const float * ln_w,
                                                  const float * ln_b);
WHISPER_API void whisper_mi355x_set_dec_splits(int splits); /* 0 = heuristic */
/* Test hook: the split-K decode GEMM's smallest row tile (32, 64 or 128; 0 = WHISPER_MI355X_DEC_BM or 32).
 * A step takes the smallest tile holding its rows; every value gives the same bits. */
WHISPER_API void whisper_mi355x_set_dec_bm(int rows);
/* Test hook: a persistent decode step's waits give up after this many 100 MHz ticks (default 5,000,000 =
 * 50 ms); 0 makes every persistent launch give up, so each step takes the re-run path. Decode graphs
 * captured before the call are retired (not replayed) once it changes the value; likewise for the stamps
 * pointer below, so a freed stamps buffer is never written. */
WHISPER_API void whisper_mi355x_set_pdec_spin(long ticks);
/* Profiling hook: device buffer of 256 * n_text_layer * 8 * 2 u64 that persistent decode steps captured
 * from now on fill with the 100 MHz clock (per workgroup, layer and phase: input arrived, phase
 * signalled); NULL turns it off. */
WHISPER_API void whisper_mi355x_set_pdec_stamps(void * dev);
/* Quantized files: 1 = persistent decode steps stream the GGML blocks; 0 (default) = they read the
 * context's expanded compute-type copy once it exists (faster). */
WHISPER_API void whisper_mi355x_set_pdec_blocks(int on);
// fp8 (OCP e4m3) GEMM with per-row f32 scales (A per row m, B per row n), then epilogue `epi`;
// A8 [M][K], B8 [N][K] bytes, K % 128 == 0 (large-v3-turbo fp8 encoder path)
WHISPER_API int whisper_mi355x_debug_gemm_fp8(struct whisper_context * ctx, int epi, const void * A8,
                                              const float * a_scale, int M, int K, const void * B8,
                                              const float * b_scale, int N, const float * bias, void * out,
                                              int reps, float * ms);
// decode-step GEMM with e4m3 weights (fp8 mode decoder): out = A[M][K] (compute dtype) .
// (B8[N][K] e4m3 * b_scale[n])^T + bias, epilogue `epi`, M <= 128, K % 64 == 0; with epi 2 and
// ln_w != null the fused residual + LayerNorm form (x = out in/out, y = LN output)
WHISPER_API int whisper_mi355x_debug_gemm_w8(struct whisper_context * ctx, int epi, const void * A, int M, int K,
                                             const void * B8, const float * b_scale, int N, const float * bias,
                                             void * out, const float * ln_w, const float * ln_b, void * y);
// q[r][:] = e4m3(x[r][:] / s[r]), s[r] = max|x[r][:]| / 448; x in the context's MFMA type
WHISPER_API int whisper_mi355x_debug_quant_fp8(struct whisper_context * ctx, const void * x, long rows, int K,
                                               void * q, float * s);
/* Debug/tuning: one encoder self-attention launch (device pointers): qkv [B*T][3d] (Q | K | V, compute
 * type of ctx), out [B*T][d], d = 64 H; variant 6 = the production launch (attn_enc2_kernel held to 128 VGPRs,
 * two workgroups per CU, scalar softmax FMAs, XCD-grouped grid), 2 = the plain attn_enc2_kernel (the tests'
 * bitwise reference); any other variant returns -1. The first launch's result stays in out; reps more launches
 * are timed (ms per launch). */
WHISPER_API int whisper_mi355x_debug_attn_encoder(struct whisper_context * ctx, const void * qkv, int B, int T, int d,
                                                  int H, int variant, void * out, int reps, float * ms);
/* Debug/tuning: the decode-step residual GEMM with its fused LayerNorm (M <= 128):
 * x[M][N] (f32, in/out) += A.B^T + bias, then y[M][N] (compute dtype) = LN(x) * ln_w + ln_b. */
WHISPER_API int whisper_mi355x_debug_gemm_ln(struct whisper_context * ctx, const void * A, int M, int K,
                                             const void * B, int N, const float * bias, float * x,
                                             const float * ln_w, const float * ln_b, void * y, int reps, float * ms);

/* Debug/tuning: the direct cross attention of decode steps (Q' projection, one pass over the
 * encoder output per token, split merge + value projection) on caller data, device pointers in the
 * context's compute type: enc [slots][n_ctx][d], slot [n] (int), q [n][d] (already scaled by
 * d_head^-0.25), wkt [d/64][d][64] (cross K weights per head, transposed), wv [d][d], bv [d] (f32)
 * -> out [n][d]. splits <= 0 picks the engine's split count; rescale_thr is the online-softmax
 * lazy-rescale threshold in log2 units (the engine uses 8). */
WHISPER_API int whisper_mi355x_debug_xattn(struct whisper_context * ctx, const void * enc, const int * slot,
                                           const void * q, const void * wkt, const void * wv, const float * bv,
                                           int n, int n_ctx, int d, float scale, int splits, float rescale_thr,
                                           void * out, int reps, float * ms);

/* Debug: the decoder attention launchers (kernels/attn.hip) on caller data, one launch each, every pointer a
 * device pointer, the caches and out in the context's compute type; d = 64 H. cache
 * [slots][L][2][H][n_ctx][64] (K | V per layer), slot [n] (int).
 * self_step: slabs [splits][n][3d] (f32 split-K partial sums of q | k | v), bias [3d] (f32, may be null);
 *   q = T((sum + bias) scale), k likewise, v = T(sum + bias); k, v are written to cache rows pos[i] and token i
 *   attends rows [0, pos[i]] -> out [n][d]. n_ctx <= 448.
 * cross_step: slabs [splits][n][d] (q only), bias [d]; token i attends rows [0, n_kv[i]) -> out [n][d]; the
 *   launcher picks the 1024- or the 256-thread kernel from n (WHISPER_MI355X_XWIDE_MAX). n_ctx <= 1536.
 * prefill: q [tokens][q_stride] (already scaled), tiles [n_tiles] int pairs {first token, count <= 64} (runs of
 *   consecutive tokens of one slot, n_kv non-decreasing), slot / n_kv per token -> out [tokens][d].
 * Return 0, -1 on bad arguments (null ctx, n <= 0, splits outside 1..16), or the runtime error code when the
 * launcher refuses the shape (nothing is launched). */
WHISPER_API int whisper_mi355x_debug_attn_self_step(struct whisper_context * ctx, const float * slabs, int splits,
                                                    const float * bias, float scale, void * cache, const int * slot,
                                                    const int * pos, int n, int L, int layer, int H, int n_ctx,
                                                    void * out);
WHISPER_API int whisper_mi355x_debug_attn_cross_step(struct whisper_context * ctx, const float * slabs, int splits,
                                                     const float * bias, float scale, const void * cache,
                                                     const int * slot, const int * n_kv, int n, int L, int layer,
                                                     int H, int n_ctx, void * out);
WHISPER_API int whisper_mi355x_debug_attn_prefill(struct whisper_context * ctx, const void * q, int q_stride,
                                                  const void * cache, const int * slot, const int * n_kv,
                                                  const void * tiles, int n_tiles, int L, int layer, int H, int n_ctx,
                                                  void * out);

/* Debug: beam search's two kernels on caller data.
 * logits_topk: logits = n device rows [n][n_vocab] (f32, the context's vocabulary); rules = host [n][10] ints per row
 * {is_initial, last_ts, penult_ts, has_ts, seek_delta, suppress_blank, no_timestamps, suppress_eot, tid0_initial
 * (< 0: no max_initial_ts rule), want_nosp}, temperature = host [n] (NULL: 0). k <= 8 candidates per row go to
 * cand (host [n][k]; rank order; id = -1: fewer tokens have p > 0), and greedy (host [n]) receives what the greedy
 * logits launch returns for the same rows in the same form. split = 1: the form the engine takes for this row
 * count (the split form up to 16 rows), 0: one workgroup per row.
 * kv_gather: cache = device [n_slots][L][2][H][n_ctx][64] of 2-byte elements; copies = host [n_copies][4] ints
 * {dst_slot, src_slot, row0, row1}: rows [row0, row1) of K and V of every layer and head move from src to dst as a
 * parallel assignment (every copy reads the cache as it was before). Destinations must be distinct.
 * *n_staged (optional) = copies that went through the staging buffer. Return 0, -1 on bad arguments, or the runtime
 * error code when the launcher refuses the list (nothing is launched). */
struct whisper_mi355x_cand {
    int32_t id, tid;
    float   p, plog, pt, ptsum, no_speech_prob, pad;
};
WHISPER_API int whisper_mi355x_debug_logits_topk(struct whisper_context * ctx, const float * logits, int n,
                                                 const int * rules, const float * temperature, int k, int split,
                                                 struct whisper_mi355x_cand * cand, struct whisper_mi355x_cand * greedy);
WHISPER_API int whisper_mi355x_debug_kv_gather(struct whisper_context * ctx, void * cache, int n_slots, int L, int H,
                                               int n_ctx, const int * copies, int n_copies, int * n_staged);

/* Debug: the sampled draw (kernels/sample.hip) on caller data, one launch. probs = host [n][2][n_vocab] (probs,
 * logprobs per row, as the logits kernels write them for want_probs rows), rec_in = host [n] records the rows start
 * from, counters = host [n][3] {seek, 16 * temp_idx + cand, token index}, words = null, or host [n] uniform words
 * used instead of the Philox word. rec_out (host [n]) receives the rows' records. 1 <= n <= 32, n_vocab <= 65536;
 * ids >= the context's first timestamp token also set tid and pt. Return 0, -1 on bad arguments, or the runtime
 * error's negative code. */
WHISPER_API int whisper_mi355x_debug_sample(struct whisper_context * ctx, const float * probs,
                                            const struct whisper_mi355x_cand * rec_in, int n, int n_vocab, uint64_t seed,
                                            const int * counters, const uint32_t * words, struct whisper_mi355x_cand * rec_out);

/* Debug: the greedy logits kernels and the device-side step advance (kernels/logits.hip) on caller data, one
 * launch each through the engine's launcher.
 * logits: logits = n device rows [n][n_vocab] (f32, the context's vocabulary); ctl = host [n], the per-row rule
 * inputs (every field per row, rows may differ); form = 0: one workgroup per row, 1: the form the engine takes for
 * this row count (the split form up to 16 rows, one workgroup per row above). out = host [n] records. probs = host
 * [n][2][n_vocab] (probs | logprobs per row) or NULL; required when a row has want_probs. Rows without want_probs
 * are not written by the kernels: their probs rows come back as NaN (all bits set).
 * decode_advance: n rows of a step with ct >= n entries per region; tout = host [n] (the step's records), ints =
 * host [5 ct] (tok | pos | slot | nkv_self | nkv_cross), ctl = host [ct], ring = host [ct], all three read and
 * written back (entries the kernel does not own return as given); err = host error word or NULL; *ring_err is
 * uploaded as given and receives the ring's copy of the word (0 when err is NULL).
 * Return 0, -1 on bad arguments (nothing touches the device), or the runtime error code. */
struct whisper_mi355x_seq_ctl {
    int32_t is_initial, last_ts, penult_ts, has_ts, seek_delta;
    float   temperature;
    int32_t suppress_blank, no_timestamps, suppress_eot, tid0_initial; /* tid0_initial < 0: no max_initial_ts rule */
    int32_t want_probs, want_nosp;
};
WHISPER_API int whisper_mi355x_debug_logits(struct whisper_context * ctx, const float * logits, int n,
                                            const struct whisper_mi355x_seq_ctl * ctl, int form,
                                            struct whisper_mi355x_cand * out, float * probs);
WHISPER_API int whisper_mi355x_debug_decode_advance(struct whisper_context * ctx, int n, int ct, int beg,
                                                    const struct whisper_mi355x_cand * tout, int * ints,
                                                    struct whisper_mi355x_seq_ctl * ctl, const unsigned * err,
                                                    struct whisper_mi355x_cand * ring, unsigned * ring_err);

/* The deny mask of whisper_full_params.suppress_nst / suppress_regex (whisper.h) for this context's vocabulary, as
 * whisper_full* builds it, from the context's one-entry cache. Host only: nothing touches the device.
 * words (cap_words >= (n_vocab + 31) / 32) receives the mask: token i is bit i & 31 of word i >> 5, set = the
 * token's logit becomes -inf before the softmax; bits at and above n_vocab are 0. regex = NULL: no pattern (an empty
 * string is a pattern like any other). Returns the word count, -1 on bad arguments (null ctx or words, cap_words too
 * small), -8 when the pattern does not compile (one stderr line; words is not written).
 * whisper_mi355x_suppress_builds: masks built (not taken from the cache) since the context was created. */
WHISPER_API int  whisper_mi355x_suppress_mask(struct whisper_context * ctx, bool suppress_nst, const char * regex,
                                              uint32_t * words, int cap_words);
WHISPER_API long whisper_mi355x_suppress_builds(struct whisper_context * ctx);
/* Debug: whisper_mi355x_debug_logits / whisper_mi355x_debug_logits_topk with a deny mask: deny = host
 * [(n_vocab + 31) / 32] words as above, uploaded and given to the launches, or NULL: the launches of the hooks
 * without _deny, bit for bit. */
WHISPER_API int whisper_mi355x_debug_logits_deny(struct whisper_context * ctx, const float * logits, int n,
                                                 const struct whisper_mi355x_seq_ctl * ctl, int form,
                                                 struct whisper_mi355x_cand * out, float * probs, const uint32_t * deny);
WHISPER_API int whisper_mi355x_debug_logits_topk_deny(struct whisper_context * ctx, const float * logits, int n,
                                                      const int * rules, const float * temperature, int k, int split,
                                                      struct whisper_mi355x_cand * cand, struct whisper_mi355x_cand * greedy,
                                                      const uint32_t * deny);

/* whisper_full_params.grammar_rules, n_grammar_rules, i_start_rule and grammar_penalty (whisper.h).
 * A decoder keeps a grammar state (a list of stacks of rule positions and a pending partial UTF-8 character), advanced by
 * every token that is fed next; before each logits step the state's reject mask over the vocabulary is taken, and the
 * logits kernels subtract grammar_penalty from every rejected token (and from EOT unless the grammar may end here), after
 * the timestamp rule and only when that rule did not mask the text tokens, and take the row's log-softmax again.
 * whisper_mi355x_grammar_mask: the reject mask of the state that init and the accepted tokens reach, for this context's
 * vocabulary, as whisper_full* builds it. Host only. words (cap_words >= (n_vocab + 31) / 32): token i is bit i & 31 of
 * word i >> 5; set = a token below EOT with a non-empty string that the state rejects; the EOT bit = the grammar may not
 * end here; bits above EOT are 0; a state whose stack list is empty (the grammar was violated: it is off for the rest of
 * the attempt) gives all zeros. Returns the word count, -1 on bad arguments, -9 when the grammar is refused (a null
 * rule, i_start >= n_rules, a RULE_REF out of range, a CHAR_RNG_UPPER or CHAR_ALT that does not follow a char class,
 * more than 65535 elements, left recursion; one stderr line). */
WHISPER_API int whisper_mi355x_grammar_mask(struct whisper_context * ctx, const whisper_grammar_element ** rules,
                                            size_t n_rules, size_t i_start, const whisper_token * accepted_tokens,
                                            int n_accepted, uint32_t * words, int cap_words);
/* Rows of grammar calls on this state (and on the second state a batch of more than 128 clips runs its other half on)
 * since it was created or recycled: rows whose mask the reject kernel (kernels/grammar.hip) decided, rows it flagged (a
 * token's simulation exceeded the kernel's bounds) and the host patched, rows the host built because the kernel does not
 * take their state (more than 32 stacks, a stack deeper than 16, a pending partial UTF-8 character); and the reject
 * kernel's time and launches from the kernel-timing class 16 (K_GRAMMAR; whisper_mi355x_kernel_timing with bit 16 set,
 * else 0). */
struct whisper_mi355x_grammar_stats { long rows_device, rows_patched, rows_host; double kernel_ms; long kernel_launches; };
WHISPER_API int whisper_mi355x_grammar_stats(struct whisper_state * state, struct whisper_mi355x_grammar_stats * out);
/* Debug: the reject masks of n_rows grammar states through the device path of whisper_full*, fallback included. Row r's
 * state is init plus accept of its n_accepted[r] tokens, which follow one another in accepted_tokens. words
 * [n_rows][(n_vocab + 31) / 32] receives the masks as read back from the device; flags[r]: 0 decided by the kernel,
 * 1 patched by the host after the kernel flagged the row, 2 built by the host alone. Returns the word count per row, -1
 * on bad arguments (no rules included), -9 for a refused grammar. */
WHISPER_API int whisper_mi355x_debug_grammar_reject(struct whisper_context * ctx, const whisper_grammar_element ** rules,
                                                    size_t n_rules, size_t i_start, const whisper_token * accepted_tokens,
                                                    const int * n_accepted, int n_rows, uint32_t * words, int * flags);
/* Debug: the _deny hooks with the grammar's reject words: gram = host [n][(n_vocab + 31) / 32] words, row r's mask as
 * above, uploaded and given to the launches with `penalty` (the launches then take the one-workgroup-per-row form,
 * whatever form / split say), or NULL: the _deny hooks, bit for bit. */
WHISPER_API int whisper_mi355x_debug_logits_gram(struct whisper_context * ctx, const float * logits, int n,
                                                 const struct whisper_mi355x_seq_ctl * ctl, int form,
                                                 struct whisper_mi355x_cand * out, float * probs, const uint32_t * deny,
                                                 const uint32_t * gram, float penalty);
WHISPER_API int whisper_mi355x_debug_logits_topk_gram(struct whisper_context * ctx, const float * logits, int n,
                                                      const int * rules, const float * temperature, int k, int split,
                                                      struct whisper_mi355x_cand * cand, struct whisper_mi355x_cand * greedy,
                                                      const uint32_t * deny, const uint32_t * gram, float penalty);

/* Debug: the two halves of a logits launch of a call with whisper_full_params.logits_filter_callback (whisper.h), one
 * launch each through the engine's launchers. flags bit 0: tdrz_enable (<|solm|> is not suppressed).
 * logits_stage: logits = device [n][n_vocab] f32 (not written), out_rows = device [n][n_vocab] f32: row r after the
 * rules that precede the callback, under ctl[r]. Nothing outside the n rows is written.
 * logits_ex: whisper_mi355x_debug_logits (form as there) over raw = device [n][n_vocab]; filtered = device
 * [n][n_vocab] makes it the prefiltered form (the rules that follow the callback over `filtered`, the no-speech
 * probability from `raw`), NULL the plain form. logits_topk_ex: the same for whisper_mi355x_debug_logits_topk, with the
 * rows' rules as ctl (want_probs is ignored). Return 0, -1 on bad arguments, or the runtime error code. */
WHISPER_API int whisper_mi355x_debug_logits_stage(struct whisper_context * ctx, const float * logits, int n,
                                                  const struct whisper_mi355x_seq_ctl * ctl, int flags, float * out_rows);
WHISPER_API int whisper_mi355x_debug_logits_ex(struct whisper_context * ctx, const float * raw, const float * filtered, int n,
                                               const struct whisper_mi355x_seq_ctl * ctl, int form, int flags,
                                               struct whisper_mi355x_cand * out, float * probs);
WHISPER_API int whisper_mi355x_debug_logits_topk_ex(struct whisper_context * ctx, const float * raw, const float * filtered,
                                                    int n, const struct whisper_mi355x_seq_ctl * ctl, int k, int split,
                                                    int flags, struct whisper_mi355x_cand * cand,
                                                    struct whisper_mi355x_cand * greedy);

/* ---- whisper_full_params.vad and the whisper_vad_* block (kernels/vad.hip) ----
 * With vad set, a call first filters its clips on the device: vad_frontend (one workgroup per clip and tile of four
 * 512-sample windows: reflect pad, STFT, magnitude, four convs, the input half of the LSTM gates), vad_lstm (one workgroup
 * of 512 threads per clip walks the clip's windows with W_hh in registers, then the head), one copy of the probabilities
 * (4 bytes per 32 ms) to the host, get_speech_timestamps there, and vad_gather (the speech pieces end to end with 1600 zero
 * samples between them). The rest of the call sees the filtered clips as device PCM. Segment k = samples [s_k, e_k) is
 * copied as [s_k, min(e_k + samples_overlap * 16000, s_{k+1})) and the last as [s_k, e_k): the overlap is clamped to the
 * next start, which keeps the time map monotone. The map takes a time t (10 ms units) of the filtered axis to the original
 * one: inside piece k, orig_start_k + (160 t - vad_start_k); in the gap after piece k or beyond the last piece, the end of
 * piece k; floor-divided by 160. It is applied once to every segment's t0 / t1 and to every token's t0, t1 and t_dtw that
 * is not -1 (the new-segment callback sees mapped times too). whisper_mi355x_window_decisions' seek stays on the
 * filtered axis. The three kernels are kernel-timing class 17 (K_VAD, work in bytes; WHISPER_MI355X_KSTAT_VAD_* gives it by kernel).
 *
 * whisper_mi355x_vad_ms: wall time of the filter step of the last full / full_batch call (the slower half of a paired
 * batch); 0 with vad off. It is not one of whisper_mi355x_phase_ms' five slots.
 * whisper_mi355x_vad_map: the piece table of a job of the last call, {orig_start, orig_end, vad_start, vad_end} in
 * samples per piece, the first `cap` pieces into out[4 * cap]; returns the job's piece count (0 with vad off or no
 * speech), -1 on bad arguments.
 * whisper_mi355x_vad_probs_batch: the probabilities of n_clips clips in one pass (one launch of each kernel), host or
 * device PCM; clip c's n_probs[c] = ceil(n_samples[c] / 512) values follow one another in probs_out (host). Every
 * clip's values are those of a whisper_vad_detect_speech call on it alone, bit for bit. 0, or -1 on bad arguments.
 * whisper_mi355x_debug_vad_frontend: the LSTM inputs xg[t] = W_ih x_t + b_ih + b_hh of one clip, host [n_windows][512];
 * returns n_windows, -1 on bad arguments.
 * whisper_mi355x_debug_vad_gather: vad_gather on caller data: host clips, clip c's n_pieces[c] pieces (four ints each,
 * as above, one after the other in `pieces`), the filtered clips one after the other in out (host; clip c's length is
 * its last piece's vad_end). Returns the samples written, -1 on bad arguments (a piece outside its clip, of different
 * lengths on the two axes, or out of order included).
 * All return -1 before touching the device. */
struct whisper_vad_context;
WHISPER_API double whisper_mi355x_vad_ms(struct whisper_state * state);
WHISPER_API int whisper_mi355x_vad_map(struct whisper_state * state, int job, int * out, int cap);
WHISPER_API int whisper_mi355x_vad_probs_batch(struct whisper_vad_context * vctx, const float * const * pcm,
                                               const int * n_samples, int n_clips, bool pcm_on_device, float * probs_out,
                                               int * n_probs);
WHISPER_API int whisper_mi355x_debug_vad_frontend(struct whisper_vad_context * vctx, const float * pcm, int n_samples,
                                                  float * xg_out);
WHISPER_API int whisper_mi355x_debug_vad_gather(struct whisper_context * ctx, const float * const * pcm,
                                                const int * n_samples, int n_clips, const int * pieces,
                                                const int * n_pieces, float * out);

/* Debug/tuning: the token-timestamp alignment kernels (kernels/align.hip) on caller data, one kernel each.
 * Clip k has n_rows[k] token rows and frames[k] = F_k frames; buffers hold the clips one after the other.
 * scores: q [n_text_layer][sum n_rows][d] (device, compute type: the cross-Q rows of every layer, already scaled
 * by d_head^-0.25), cross = a cross K/V cache [n_slots][n_text_layer][2][H][n_audio_ctx][64] (device), slot[k] =
 * the clip's slot, heads {head_layer[a], head_idx[a]} -> P (device f32), clip k at sum_{k' < k} A n_rows F,
 * laid out [A][n_rows][F]: softmax over all n_audio_ctx keys, frames t < F kept. One launch per layer.
 * cost: P as above, n_sot[k] leading rows and the last row dropped -> cost (device f32) [N_k][F_k] per clip,
 * N_k = n_rows[k] - n_sot[k] - 1.
 * dtw: cost (device f32) [rows[k]][frames[k]] per clip, all clips in one launch -> fr (host int, rows[k] per
 * clip: first frame of every row), path (host, optional: int pairs {row, frame} from the last cell back to
 * (0, 0), rows[k] + frames[k] pairs reserved per clip) and path_len (host, optional: pairs written per clip).
 * host arrays are plain host pointers. Return 0, or -1 on bad arguments. */
WHISPER_API int whisper_mi355x_debug_align_scores(struct whisper_context * ctx, const void * q, const void * cross,
                                                  int n_slots, int n_clips, const int * slot, const int * n_rows,
                                                  const int * frames, int n_heads, const int * head_layer,
                                                  const int * head_idx, float * P);
WHISPER_API int whisper_mi355x_debug_align_cost(struct whisper_context * ctx, const float * P, int n_clips,
                                                const int * n_rows, const int * n_sot, const int * frames, int n_heads,
                                                float * cost);
WHISPER_API int whisper_mi355x_debug_align_dtw(struct whisper_context * ctx, const float * cost, int n_clips,
                                               const int * rows, const int * frames, int * fr, int * path,
                                               int * path_len);

/* Audio front-end on the GPU (src-tauri/src/audio.rs), for n_clips clips at
 * once on HIP device `device`. pcm / audio / out point at host buffers, or (on_device = true) at
 * buffers already in that device's HBM.
 *
 * whisper_mi355x_find_silence_boundaries replaces audio.rs:400-467 find_silence_boundaries(audio,
 * sample_rate) (with estimate_noise_floor, audio.rs:373-397): counts[c] = number of split points of
 * clip c (only the first `cap` are stored, boundaries[c * cap + i], sample indices); noise_floor[c]
 * (optional) = the adaptive noise floor; rms_out (optional, [n_clips][rms_stride]) = the RMS of
 * every 20 ms window, bit-identical to audio.rs:364-370 calculate_rms. Returns 0, or -1 on bad
 * arguments. split_at_silences (audio.rs:469-507) is pure indexing and stays with the caller. */
WHISPER_API int whisper_mi355x_find_silence_boundaries(int device, const float * const * pcm, const int * n_samples,
                                                       int n_clips, int sample_rate, bool pcm_on_device, int * counts,
                                                       int * boundaries, int cap, float * noise_floor, float * rms_out,
                                                       int rms_stride);
/* audio.rs:331-337 resample_chunk(audio, input_sample_rate) -> 16 kHz (audio.rs:509-563: rubato 0.15.0
 * FftFixedIn, 1024-sample chunks, 2 sub-chunks, last chunk zero-padded, output truncated to
 * len * 16000 / rate). out[c] must hold whisper_mi355x_resample_len(n_in[c], rate_in) floats. */
WHISPER_API int whisper_mi355x_resample_len(int n_in, int rate_in);
WHISPER_API int whisper_mi355x_resample_chunk(int device, const float * const * audio, const int * n_in, int n_clips,
                                              int rate_in, bool on_device, float * const * out);
/* The resampler's FFT pipeline as one linear map (tests): block sizes fsi / fso of rate_in, and
 * W [2*fsi][fso] with output block m = sum_t x[(m-1)*fsi + t] W[t][:]. */
WHISPER_API int whisper_mi355x_resample_operator(int rate_in, int * fsi, int * fso, float * W, long cap);

/* ABI self-description, no device needed: sizeof(whisper_full_params), sizeof(whisper_context_params),
 * sizeof(whisper_token_data), offsetof(full_params, initial_prompt / language / greedy /
 * new_segment_callback / vad_params). Lets a binding (bindgen, ctypes) be checked field-by-field. */
WHISPER_API int whisper_mi355x_abi_layout(size_t out[8]);

/* State introspection (tests): out[0] = cross-attention form of the last call (1 = straight from the
 * encoder output, 0 = cached cross K/V), out[1] = clip slots of the workspace, out[2] = slots of the
 * cross K/V cache, out[3] = decode-step graphs kept, out[4] = 1 if the state was recycled from the
 * context's state pool (whisper_init_state after a whisper_free_state keeps the workspace and the
 * captured decode graphs; WHISPER_MI355X_STATE_POOL=0 disables the pool). Returns 5. */
WHISPER_API int whisper_mi355x_state_info(struct whisper_state * state, int out[5]);

/* HIP stream of a state (hipStream_t), for callers that enqueue their own work around it. */
WHISPER_API void * whisper_mi355x_state_stream(struct whisper_state * state);

/* Model-free micro-API used by the kernel parity tests: allocate/copy device memory on the
 * context's device. */
WHISPER_API void * whisper_mi355x_dev_alloc(struct whisper_context * ctx, size_t bytes);
WHISPER_API void   whisper_mi355x_dev_free(struct whisper_context * ctx, void * p);
WHISPER_API int    whisper_mi355x_memcpy(struct whisper_context * ctx, void * dst, const void * src, size_t bytes, int kind);

#ifdef __cplusplus
}
#endif

#endif /* WHISPER_MI355X_H */
