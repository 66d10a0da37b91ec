// Host-side launchers of the gfx950 kernels. Every launcher takes the stream it runs on and
// never allocates or synchronises (so a decode step can be captured into a hipGraph).
#pragma once
#include <atomic>

#include "common.h"
#include "gemm_plan.h"
#include "grammar.h"

namespace wm {

// ---- mel (kernels/mel.hip) ---------------------------------------------------------------------
void launch_mel(const float* const* d_pcm, const int* d_n, const void* d_tab, const float* d_filt_t, int n_mel,
                float* const* d_mel, const int* d_nlen, int* d_max, int n_jobs, int max_frames, hipStream_t st);
// frames: mel frames of a window (2 * the encoder positions, <= 3000); image rows [0, frames + 2) are written
void launch_mel_window(DType dt, float* const* d_mel, const int* d_nlen, const int* d_n, const int* d_max,
                       const int* d_win_job, const int* d_win_seek, int n_win, int n_mel, int frames, void* out,
                       hipStream_t st);
void launch_mel_normalize(const float* d_mel, int nl, int n_samples, const int* d_max, int n_mel, float* out, hipStream_t st);
// ---- audio front-end (kernels/audio.hip; audio.rs VAD chunking + resampler) ------------------------
// rms[c][w] (row stride rms_stride >= max_n / (rate/50)) of every 20 ms window, then per clip the
// noise floor (floor_out, optional) and the silence boundaries: counts[c], bounds[c][cap]
void launch_silence_boundaries(const float* const* pcm, const int* n_samples, int n_clips, int max_n, int sample_rate,
                               float* rms, int rms_stride, int* counts, int* bounds, int cap, float* floor_out,
                               hipStream_t st);
// out[c][m*fso + j] = sum_t in[c][(m-1)*fsi + t] * W[t][j] for m*fso + j < n_out[c]; W [2*fsi][ldw]
void launch_resample(const float* const* in, const int* n_in, int n_clips, int max_out, const float* W, int ldw, int fsi,
                     int fso, float* const* out, const int* n_out, hipStream_t st);

// ---- layer norm / embedding (kernels/norm.hip) ------------------------------------------------
// y[i] = LN(x[row(i)]) * w + b, x f32 [.][D] (row stride D), y T [M][D]; row(i) = rows ? rows[i] : i
void launch_layernorm(DType dt, const float* x, const int* rows, int M, int D, const float* w, const float* b,
                      void* y, hipStream_t st);
// x[i][:] = tok_emb[tok[i]][:] + pos_emb[pos[i]][:]   (f32 out; tok_emb in the MFMA type, or f32
// when te_f32: a quantized GGML embedding's exact dequantized rows)
void launch_embed(DType dt, const void* tok_emb, bool te_f32, const float* pos_emb, const int* tok, const int* pos,
                  int n, int D, float* x, hipStream_t st);
// embedding fused with the first LayerNorm: x as above, y[i] = LN(x[i]) * w + b (T out)
void launch_embed_ln(DType dt, const void* tok_emb, bool te_f32, const float* pos_emb, const int* tok, const int* pos,
                     int n, int D, float* x, const float* w, const float* b, void* y, hipStream_t st);

// ---- GEMM (kernels/gemm.hip): C[M][N] = A[M][K] . B[N][K]^T + bias, fused epilogues --------------
// (enum Epi, the epilogue ids, and gemm_plan, what a shape will run: gemm_plan.h)

// GGML block-quantized weight matrix [N][K] (the app's catalog ships q5_0 / q5_1
// files, model.rs:153-186) kept in HBM as the file's blocks, regrouped by field (same bits, same bytes):
// qs = the quant bytes of every block [N][K/2] (q4_*, q5_*: two 4-bit values per byte, the block's
// weights j and j + 16 in byte j) or [N][K] (q8_0), qh = the q5 high bits [N][K/32] (bit j = weight j),
// dm = the f16 scale d per block [N][K/32] (q4_0, q5_0, q8_0) or d and min m [N][K/32][2] (q4_1,
// q5_1). type: ggml type id (2 q4_0, 3 q4_1,
// 6 q5_0, 7 q5_1, 8 q8_0), 0 = not quantized. w = d * (q - offset) or d * q + m, exact in f32, then
// rounded once to the compute type.
struct QMat {
    int type = 0;
    const uint8_t* qs = nullptr;
    const uint32_t* qh = nullptr;
    const uint16_t* dm = nullptr;
};

struct GemmArgs {
    const void* A; long a_rpb, a_bstride, a_rstride;  // A row m -> A + (m/a_rpb)*a_bstride + (m%a_rpb)*a_rstride
    const void* B;                                     // [N][K] row-major
    const float* bias;                                 // [N] or null
    int M, N, K;
    void* out; long ldo; long o_rpb, o_bstride, o_off; // out row = (m/o_rpb)*o_bstride + (m%o_rpb) + o_off
    const float* pos; int pos_rows;                    // EPI_GELU_POS
    float scale; int sc_div, sc_mod, sc_lim;           // column n scaled iff ((n/sc_div)%sc_mod) < sc_lim
    // caches (EPI_CROSSKV / EPI_QKV_DEC)
    void* cache; const int* row_slot; const int* row_pos; int L, layer, H, ctx, d;
    // EPI_CROSSKV: rows of A per window (the call's encoder positions, <= ctx; ctx stays the cache's row stride).
    // 0 = ctx (launch_gemm fills it in)
    int rpw;
    // split-K workspace for skinny (decode-step) GEMMs: f32 [splits][M][N]; null disables split-K
    float* splitk_ws; long splitk_ws_elems;
    // EPI_RESID on the split-K path only: fused LayerNorm of the updated residual rows,
    // ln_out[m][:] = LN(out[m][:]) * ln_w + ln_b (the next GEMM's input; null = no LN)
    const float* ln_w; const float* ln_b; void* ln_out;
    // small-M decode GEMM (launch_gemm_small) with lna: A is the f32 residual stream and the
    // workgroup applies LN(A) * a_ln_w + a_ln_b (ggml_norm) to its rows before the product
    const float* a_ln_w; const float* a_ln_b;
    // small-M decode GEMM: B given as GGML blocks (q.type != 0) instead of the compute type
    QMat q;
    // decode-step split-K slabs stored write-through (sc1) instead of write-back (every decode step)
    int slab_wt;
    // decode-step GEMMs in fp8 mode: B is OCP e4m3 [N][K] bytes, column n scaled by w8_scale[n]
    const float* w8_scale;
    // debug (whisper_mi355x_set_gemm_stamps): the encoder GEMM kernel writes s_memtime at 4 points per workgroup
    unsigned long long* stamps;
};
extern unsigned long long* g_gemm_stamps;
// out[M][ldo] = A[M][K] . B[N][K]^T + bias on contiguous rows, nothing scaled: the call every other one starts from
inline GemmArgs gemm_plain(const void* A, int M, int K, const void* B, int N, const float* bias, void* out, long ldo) {
    GemmArgs g{};
    g.A = A; g.a_rpb = M > 0 ? M : 1; g.a_bstride = 0; g.a_rstride = K;
    g.B = B; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.out = out; g.ldo = ldo; g.o_rpb = M > 0 ? M : 1; g.o_bstride = 0; g.o_off = 0;
    g.sc_div = 0; g.sc_mod = 1; g.sc_lim = 0; g.scale = 1.0f;
    return g;
}

// the plan's knobs as the launchers see them now (whisper_mi355x_set_gemm_variant / _dec_splits / _dec_bm and the
// environment), for callers that ask gemm_plan what a shape will run
GemmKnobs current_knobs();
void launch_gemm(DType dt, int epi, const GemmArgs& a, hipStream_t st);
// fp8 (OCP e4m3) operands with per-row f32 scales: C = (A8 . B8^T) * a_scale[m] * b_scale[n], then
// the epilogue (EPI_STORE / EPI_GELU / EPI_GELU_F / EPI_RESID); K % 128 == 0, N % 16 == 0. A/B strides
// in bytes.
void launch_gemm_fp8(DType dt, int epi, const GemmArgs& a, const float* a_scale, const float* b_scale, hipStream_t st);
// q[r][:] = e4m3(x[r][:] / s[r]), s[r] = max|x[r][:]| / 448 (x in the MFMA type, K % 8 == 0)
void launch_quant_rows_fp8(DType dt, const void* x, long rows, int K, void* q, float* s, hipStream_t st);
// LayerNorm (f32 residual rows -> LN * w + b) quantized per row to fp8 e4m3: q [M][D] bytes, s [M]
void launch_layernorm_fp8(const float* x, int M, int D, const float* w, const float* b, void* q, float* s,
                          hipStream_t st);
// uploads the f16 GELU table the GELU epilogues read (once per context/device, before any GEMM)
void init_gelu_table();
// Decode step (M <= 128, K % 64 == 0): only the split-K partial sums, slabs [splits][M][N] f32 in
// a.splitk_ws, no epilogue; the consumer reduces them (attention prologues). Returns the split
// count, or 0 when the shape/workspace does not allow it (the caller then uses launch_gemm).
int launch_gemm_partials(DType dt, const GemmArgs& a, hipStream_t st);
// Decode steps of M <= 32 rows: one launch, no split-K slabs and no reduce launch (one workgroup =
// 16 output columns over the whole K, its 8 waves splitting K and summing in LDS). Epilogues
// EPI_F32 / EPI_STORE / EPI_GELU / EPI_RESID. lna: A = LN(f32 residual rows) computed in the
// prologue (K <= 1280). M > 32 runs as 32-row chunks (block-quantized weights, a.q, take this path at
// every batch size). gemm_small_ok: false when the shape is not supported (K % 32; lna: K <= 1280,
// K % 128).
bool gemm_small_ok(int M, int K, bool lna);
// out[r][k] (compute type) = the dequantized weights of rows [0, rows) of a block-quantized matrix
void launch_dequant(DType dt, const QMat& q, long rows, int K, void* out, hipStream_t st);
// up to 6 matrices of ONE GGML type dequantized by one launch (start[] is filled by the launcher)
struct DequantJobs {
    int n = 0;
    QMat q[6];
    long rows[6];
    int K[6];
    void* out[6];
    long start[7];
};
void launch_dequant_multi(DType dt, DequantJobs J, hipStream_t st);
void launch_gemm_small(DType dt, int epi, const GemmArgs& a, bool lna, hipStream_t st);

// ---- attention (kernels/attn.hip) --------------------------------------------------------------
// encoder self-attention: qkv [B*T][3d] -> out [B*T][d]; softmax scale 1/sqrt(64)
// variant: -1 = the default (6: attn_enc2_kernel held to 128 VGPRs, scalar softmax FMAs), else
// 1 / 2 / 3 / 5 (attn_enc_kernel / _enc2_ / _enc3_ / _enc2_ with packed FMAs; kernel benchmarks only)
void launch_attn_encoder(DType dt, const void* qkv, void* out, int B, int T, int d, int H, hipStream_t st,
                         int variant = -1);
// Decoder attention over a cache [slot][L][2][H][ctx][64]: token i attends keys [0, n_kv[i]) of slot[i];
// q [n][q_stride] at head h offset h*64; out [n][d].
// Prefill: runs of consecutive tokens of one clip, tiles[t] = {first token, count <= 64} (int2), one
// workgroup per (tile, head); K/V staged once per tile.
void launch_attn_prefill(DType dt, const void* q, int q_stride, const void* cache, const int* slot, const int* n_kv,
                         const void* tiles, int n_tiles, int L, int layer, int H, int ctx, int d, void* out,
                         hipStream_t st);

// Decode-step attention with the projection GEMM's split-K reduce fused into its prologue.
// Slab z holds rows [M][ld] of partial sums; the value of (row i, column c) is
// sum_z ws[z*zstride + i*ld + c] + bias[c] (the same order as the standalone reduce).
struct DecSlabs {
    const float* ws; int splits; long zstride; int ld; const float* bias; float scale;
};
// self attention of token i: q/k/v columns [0,d)/[d,2d)/[2d,3d) of the QKV slabs (q and k scaled,
// as the EPI_QKV_DEC epilogue); writes this position's k, v into the self cache at pos[i].
void launch_attn_self_step(DType dt, const DecSlabs& sl, void* cache, const int* slot, const int* pos, int n, int L,
                           int layer, int H, int ctx, int d, void* out, hipStream_t st);
// decode steps of up to this many clips use the 1024-thread cache-form kernel (WHISPER_MI355X_XWIDE_MAX,
// default 8, read per call)
int attn_cross_wide_max();
// cross attention of token i over n_kv[i] keys of the cross cache; q from the cross-Q slabs.
void launch_attn_cross_step(DType dt, const DecSlabs& sl, const void* cache, const int* slot, const int* n_kv, int n,
                            int L, int layer, int H, int ctx, int d, void* out, hipStream_t st);

// ---- cross attention from the encoder output (kernels/xattn.hip) --------------------------------
// enc [slot][Tn][d] (the encoder's ln_post output in the MFMA type). For token i (clip slot[i]):
//   qproj:   qx[i][h][:] / qx[i][H+h][:] = hi / lo parts of scale * Wk_h^T q[i][h*64:(h+1)*64]
//            (wkt = Wk per head, transposed: [H][d][64]);
//   step:    rows split sp: unnormalised partial O^T opart[i][sp][h][d] and ml[i][sp][h] = {m (log2 units), l};
//            the running max moves only when a tile exceeds it by more than thr (log2 units);
//   combine: out[i][h*64+j] = (sum_sp w_sp O_sp / L) . Wv[h*64+j][:] + bv[h*64+j]   (MFMA type)
bool xattn_supported(int d);
int xattn_splits(int n, int Tn);
void launch_xattn_qproj(DType dt, const void* q, const void* wkt, int n, int d, int H, float scale, void* qx,
                        hipStream_t st);
void launch_xattn_step(DType dt, const void* enc, const int* slot, const void* qx, int n, int Tn, int d, int splits,
                       float thr, float* opart, float* ml, hipStream_t st);
void launch_xattn_combine(DType dt, const float* opart, const float* ml, int splits, const void* wv, const float* bv, int n,
                          int d, int H, void* out, hipStream_t st);

// ---- token timestamps from cross-attention DTW (kernels/align.hip) -------------------------------
// One clip of an alignment launch. Its token rows are rows [row0, row0 + n_rows) of the pass's q, over
// cross-cache slot `slot`; n_sot = 1 or 2 leading rows and the last row (eot) are not aligned, so the cost
// matrix has N = n_rows - n_sot - 1 rows; `frames` = F <= n_audio_ctx encoder positions. Offsets in
// elements of their buffers: P [A][n_rows][F] f32, stats [A][F][2] f32, cost [N][F] f32, trace [N][F]
// bytes, fr [N] int, path [N + F] int pairs.
struct AlignClip {
    int slot, row0, n_rows, n_sot, frames, pad;
    long p_off, st_off, cost_off, tr_off, fr_off, path_off;
};
// Softmaxed score rows of the alignment heads of one decoder layer: heads[k] = {head, index a in the
// context's head list} (device, n_heads entries); q [rows][q_stride] in the compute type (cross-Q of that
// layer, already scaled), cross = the cross K/V cache [slot][L][2][H][ctx][64]. P[a][i][t] =
// softmax_t(q_i . k_t) over the first n_keys <= ctx keys in f32, written for t < F only. K is read once per (clip, head).
void launch_align_scores(DType dt, const void* q, int q_stride, const void* cross, const AlignClip* clips, int n_clips,
                         int max_rows, int L, int layer, int H, int ctx, int n_keys, const int2* heads, int n_heads,
                         float* P, hipStream_t st);
// z-score per (head, frame) over the token rows, width-7 median along the frames, head mean, negation,
// row slice: P -> cost (stats is scratch). max_rows / max_frames: the largest N / F of the clips.
void launch_align_cost(const float* P, const AlignClip* clips, int n_clips, int A, int max_rows, int max_frames, float* stats,
                       float* cost, hipStream_t st);
// OpenAI's dtw_cpu in f32, one workgroup per clip: fr[r] = frame of the first path point of cost row r.
// trace is scratch; path / path_len (optional) receive the path from (N - 1, F - 1) back to (0, 0).
void launch_align_dtw(const float* cost, const AlignClip* clips, int n_clips, int max_n, unsigned char* trace, int* fr,
                      int* path, int* path_len, hipStream_t st);

// ---- persistent decode step (kernels/pdec.hip) ---------------------------------------------------
// One launch = every decoder layer of one decode step for M <= kPdecMaxRows clips in the cross K/V cache
// form, phases handed off through data-tagged granules (see pdec.hip). Output: out_dh [M][d] (T) = the final
// LayerNorm of each row, the logits GEMM's input.
constexpr int kPdecMaxRows = 4;
// one projection matrix [N][K]: the compute type (qt = 0, w = T weights) or GGML blocks (qt = ggml type,
// w = QMat::qs, qh, dm as in QMat)
struct PdecMat {
    const void* w;
    const uint32_t* qh;
    const uint16_t* dm;
    int qt;
};
struct PdecLayer {
    PdecMat qkv, o, xq, xo, f1, f2;
    const float *bqkv, *bo, *bxq, *bxo, *b1, *b2;
    const float *ln1_w, *ln1_b, *lnx_w, *lnx_b, *ln2_w, *ln2_b;
};
// The hand-off block (one allocation, zeroed before every launch): data-tagged 8-byte granules (offsets
// in granules): x rows x0, x1, x2 [R][d] (f32), and packed T pairs: qkv [R][3d/2], self-attention output
// so [R][d/2], cross q qx [R][d/2], cross-attention output xo [R][d/2], GELU rows ff [R][2d]; the
// cross-attention split partials part [max(256, R * H * S)][66] (f32: o[64], max, sum; one per task); then the
// error word (byte offset); R = kPdecMaxRows.
struct PdecGranules {
    long x0, x1, x2, qkv, so, qx, xo, ff, part;
    long err_bytes, zero_bytes, bytes;  // the error word; 256 zero bytes that no one writes (a zero page)
};
PdecGranules pdec_granules(int d, int L, int H);
// LDS layout of one workgroup (byte offsets, 16-aligned), shared by the launcher and the kernel: rows are
// provisioned for the launch's clip count when it is 1 or 2 (those launches also hold the |x| < 10 part
// of ggml's f16 GELU table, 2 x 0x4900 entries), else for kPdecMaxRows
struct PdecLds {
    int xs, xf, sc, red, qf, res, ost, lred, lnp, part, lflag, gtab, bytes, rows, cmax;
};
constexpr int kPdecGeluHalf = 0x4900;  // f16 bit patterns below 10.0 (one sign)
__host__ __device__ inline PdecLds pdec_lds(int d, int M, int S) {
    auto up = [](int b) { return (b + 15) & ~15; };
    PdecLds l{};
    l.rows = M <= 2 ? M : kPdecMaxRows;
    const int c1 = 2 * ((3 * d / 2 + 255) / 256), c4 = 2 * ((2 * d + 255) / 256);
    l.cmax = c1 > c4 ? c1 : c4;
    int o = 0;
    l.xs = o; o += up(l.rows * 4 * d * 2);
    l.xf = o; o += up(l.rows * d * 4);
    l.sc = o; o += 1536 * 4;
    l.red = o; o += up((8 + 256) * 4);
    l.qf = o; o += 192 * 4;
    l.res = o; o += up(68 * 4);
    l.ost = o; o += up(l.rows * l.cmax * 4);
    l.lred = o; o += 2 * kPdecMaxRows * 4 * 8;
    l.lnp = o; o += up(6 * d * 4);
    l.part = o; o += up(S * 66 * 4);
    l.lflag = o; o += 16;
    l.gtab = o; o += M <= 2 ? up(2 * kPdecGeluHalf * 2) : 0;
    l.bytes = o;
    return l;
}
struct PdecArgs {
    const PdecLayer* layers;  // device array [L]
    int L, M, d, n_text_ctx, n_audio_ctx;  // n_audio_ctx: the cross cache's row stride
    int n_audio_len;                       // keys per clip of the cross attention (<= n_audio_ctx)
    const void* tok_emb; int te_f32; const float* pos_d;
    const float *lnd_w, *lnd_b;
    const int *tok, *pos, *slot;      // [M]
    void* self_cache; const void* cross_cache;
    float k_scale;
    int s_cross;                        // key splits per (clip, head) of the cross attention
    int quant;                          // the layers' matrices are GGML blocks (PdecMat.qt != 0)
    void* sync;                         // the hand-off block (gr.bytes), zeroed by the launcher
    PdecGranules gr;
    void* out_dh;
    const uint16_t* gelu_tab;           // ggml's f16 GELU table on the device (gelu_table_device)
    long spin_ticks;                    // a wait gives up after this many 100 MHz ticks (g_pdec_spin_ticks)
    unsigned long long* stamps;         // debug (g_pdec_stamps): [256][L][8][2] clock at input / publish, or null
};
extern unsigned long long* g_pdec_stamps;
// bumped by the stamps / spin setters: decode graphs captured with a persistent step under an older value
// are retired, not replayed (they hold the old pointer and limit as kernel arguments)
extern std::atomic<int> g_pdec_gen;  // bumped by the stamps / spin setters (capi.cpp); read once per dec_graph
// persistent launches that gave up, every state of the process (whisper_mi355x_pdec_give_ups(NULL))
extern std::atomic<long> g_pdec_give_ups_total;
// 5,000,000 = 50 ms; a test hook sets 0 to make every launch give up (the re-run path)
extern long g_pdec_spin_ticks;
// 1: quantized files' persistent steps stream the GGML blocks even when the expanded copy exists
extern int g_pdec_blocks;
// a kernel exists for the shape: plain weights at d 384 / 512 / 768 / 1024 / 1280, GGML blocks (f16
// compute) at 768 / 1024 / 1280
bool pdec_supported(int d, int H, bool quant);
int pdec_cross_splits(int H, int rows);  // key splits per (clip, head): a function of the shape only
void launch_pdec(DType dt, const PdecArgs& a, hipStream_t st);
const uint16_t* gelu_table_device();

// ---- logits processing (kernels/logits.hip) ----------------------------------------------------
struct VocabIds {
    int n_vocab, eot, sot, translate, transcribe, solm, prev, nosp, not_, beg, space, n_lang;
};
struct SeqCtl {             // per-sequence inputs of whisper_process_logits
    int is_initial, last_ts, penult_ts, has_ts, seek_delta;
    float temperature;
    int suppress_blank, no_timestamps, suppress_eot, tid0_initial;  // tid0_initial < 0: no max_initial_ts rule
    int want_probs, want_nosp;  // want_probs: 1 = the probs row goes to the host's sampler, 2 = it stays on the device (launch_sample)
};
struct TokOut { int id, tid; float p, plog, pt, ptsum, nosp_prob, pad; };
// rec: scratch of logits_rec_bytes(n_seq) bytes for the split form (rows spread over several workgroups
// each, used for up to 16 rows); null = one workgroup per row
// deny: the deny mask of suppress_nst / suppress_regex on the device (suppress.h: (n_vocab + 31) / 32 words, bit
// i & 31 of word i >> 5 = token i gets -inf like any other rule; nosp_prob stays the raw row's), or null: no mask,
// and the launch is bit for bit the one from before the mask existed
// gram: the grammar's reject words on the device (grammar.h, DESIGN.md §16: [n_seq][(n_vocab + 31) / 32], row r's bit
// i = token i <= eot of row r loses gram_penalty after the timestamp rule, when that rule did not mask the text tokens,
// and the row's log-softmax is taken again), or null: no grammar, and the launch is the one from before the rule
// existed. With gram the launch takes the one-workgroup-per-row form whatever n_seq is (also launch_logits_topk).
void launch_logits(const float* logits, long ld, const SeqCtl* ctl, int n_seq, const VocabIds& v,
                   TokOut* out, float* probs, void* rec, const uint32_t* deny, const uint32_t* gram, float gram_penalty,
                   hipStream_t st, const float* filtered = nullptr);
size_t logits_rec_bytes(int n_seq);
// Top-k after the rules (beam search): the k <= kTopkMax most probable tokens of every row, p > 0, in
// (p descending, id ascending) order, as TokOut records cand[row * kTopkMax + j]; j = 0 repeats the record
// launch_logits returns for the row (same form by n_seq / rec, same bits: id 0, p 0 when no token has p > 0);
// a record j > 0 without a token has id = -1. Rows are t = 0 rows (want_probs is ignored).
constexpr int kTopkMax = 8;
void launch_logits_topk(const float* logits, long ld, const SeqCtl* ctl, int n_seq, const VocabIds& v, TokOut* cand, int k,
                        void* rec, const uint32_t* deny, const uint32_t* gram, float gram_penalty, hipStream_t st,
                        const float* filtered = nullptr);
// whisper_full_params.logits_filter_callback. The rules of a row come in two halves with the caller's
// callback between them: launch_logits_stage writes out[row][n_vocab] (f32, row stride n_vocab) = the row after the
// temperature divide, suppress_blank, <|notimestamps|>, no_timestamps, sot / nosp / solm / translate / transcribe / prev
// and the language tokens (solm is kept when v.solm matches no id: tdrz_enable); logits is not written. `filtered` of
// launch_logits / launch_logits_topk (null: the launch from before the callback existed) is such a buffer after the
// callback: the launch is then the prefiltered form, which skips the divide and those rules, applies every other rule
// to the filtered row and takes the no-speech probability from the raw row `logits`. Being prefiltered is a property of
// the launch, not of a row: SeqCtl does not change.
void launch_logits_stage(const float* logits, long ld, const SeqCtl* ctl, int n_seq, const VocabIds& v, float* out,
                         hipStream_t st);
// ---- the grammar's reject masks (kernels/grammar.hip) -------------------------------------------------
// What the kernel takes of a row's grammar state, and a token's working set (stacks per token, depth): a state or a
// token's simulation beyond them is the host's (grammar_reject).
constexpr int kGramRowStacks = 32, kGramRowDepth = 16;
constexpr int kGramTokStacks = 8, kGramTokDepth = 16;
static_assert(kGramTokDepth >= kGramRowDepth, "a row's stack fits a token's slot");
constexpr int kGramTokEmpty = -2;  // GramTable::tail_rem of an id whose string is empty (never penalised)
// (same_as: the first row of the launch with this row's state, or the row itself: the rows of a step mostly share a few
// states, so a state is simulated once and its words are copied to the rows that share it)
struct GramRow {  // n_stacks < 0: the row is not the kernel's (its words are left alone)
    int n_stacks, allow_eot, same_as;
    uint8_t depth[kGramRowStacks];
    uint16_t stk[kGramRowStacks][kGramRowDepth];  // positions (element indices), the top last
};
// The vocabulary decoded once per context, on the device, for ids < eot: CSR offsets [eot + 1], the code points, and the
// trailing partial of decode(string, {0, 0}) (tail_rem: bytes missing, -1 an invalid token, kGramTokEmpty)
struct GramTable {
    const uint32_t *off, *cps, *tail_val;
    const int* tail_rem;
    int eot, n_vocab;
};
// gram[row][(n_vocab + 31) / 32] of the n_rows rows (grammar.h's layout: the EOT bit = !allow_eot, bits above eot 0, a
// row without stacks all zeros); over[row] (zeroed by the caller) becomes non-zero when a token of the row exceeded a
// bound: that row's words are then not to be used. elems / rule_off: the call's flat rules on the device.
void launch_grammar_reject(const GramTable& t, const GramElem* elems, const int* rule_off, const GramRow* rows, int n_rows,
                           uint32_t* gram, unsigned* over, hipStream_t st);
// ---- sampled draw (kernels/sample.hip; best_of candidates of a t > 0 attempt) -------
// Row r < n (<= kSampleMaxRows, one workgroup each) draws a token from probs row src = ctr[r][3] of the
// [.][2][n_vocab] buffer launch_logits fills for want_probs rows: uniform word x0 = words[r] if words, else
// Philox4x32-10 word 0 of counter (0, ctr[r][0], ctr[r][1], ctr[r][2]) = (0, seek, 16 * temp_idx + cand, token
// index) under key `seed`; id = the first id whose inclusive prefix sum (double, ascending id) exceeds
// (x0 + 0.5) * 2^-32 * total. out[r] = in[src] with id, p, plog of the drawn token (and tid = id, pt = p when
// id >= token_beg); a row whose probs sum to 0 keeps in[src]. in == out is allowed when src == r for every row.
// ctr: device [n][4] ints.
constexpr int kSampleMaxRows = 32;
void launch_sample(const float* probs, int n_vocab, const TokOut* in, TokOut* out, const int* ctr, const uint32_t* words,
                   uint64_t seed, int token_beg, int n, hipStream_t st);
// ---- self-cache gather (kernels/beam.hip; beam search re-parenting) --------------------------------
// Every copy of the list (beam.h KvCopy, scheduled by beam_schedule) moves rows [row0, row1) of K and V of every
// layer and head of the cache [n_slots][L][2][H][n_ctx][64] (2-byte type) from src_slot to dst_slot, as a
// parallel assignment: one launch, and a second one when a copy goes through `stage` (stage_units 16-byte
// units). copies_host is read for the bounds check and the grid, copies_dev by the kernel.
struct KvCopy;
void launch_kv_gather(void* cache, int n_slots, int L, int H, int n_ctx, const KvCopy* copies_host, const KvCopy* copies_dev,
                      int n_copies, void* stage, long stage_units, hipStream_t st);
// ---- token times (kernels/tokts.hip; whisper_full_params.token_timestamps) ---------
// A clip: its n PCM samples on the device and where its energy signal starts in the energy buffer (floats).
struct TtClip { const float* pcm; long long e_off; int n, pad; };
// A segment of n_tok >= 2 tokens of clip `clip`: spans[tok0 .. tok0 + n_tok).
struct TtSeg { int clip, tok0, n_tok, pad; };
// A token: t0, t1 in 10 ms units (in / out), is_text = 0 for ids >= eot (left as they are).
struct TtSpan { long long t0, t1; int is_text, pad; };
constexpr int kEnergyTile = 1024;  // samples of a clip per workgroup of the energy kernel
constexpr int kVadChunk = 256;     // samples per round of the adjust kernel's walks
// energy[clips[c].e_off + i] = (sum_{j=-32..32, inside the clip} |pcm[i + j]|) / 65.0f, the bits of the sequential
// f32 loop; max_n = the longest clip (the grid). clips: device [n_clips].
void launch_signal_energy(const TtClip* clips, int n_clips, int max_n, float* energy, hipStream_t st);
// The voice-activity adjust of every segment's tokens (one workgroup per segment, tokens in order), spans in place.
// The caller checks the lists (clip indices, token ranges, n >= 1 samples): the kernel trusts them.
void launch_token_vad(const float* energy, const TtClip* clips, const TtSeg* segs, int n_segs, TtSpan* spans, hipStream_t st);
// pipelined greedy decoding: advance every row's input token, position and SeqCtl on the device after a step
// and copy its TokOut (+ the persistent launch's error word, if err) to a ring slot (kernels/logits.hip)
void launch_decode_advance(int n, int ct, int beg, const TokOut* tout, int* ints, SeqCtl* ctl, TokOut* ring,
                           const unsigned* err, unsigned* ring_err, hipStream_t st);

}  // namespace wm
