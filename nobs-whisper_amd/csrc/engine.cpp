// The MI355X Whisper engine: workspace, encoder/decoder forward on one HIP stream, and the
// batched window scheduler that reproduces whisper_full_with_state for every clip of a batch
// (reference call site whisper.rs:127-129).
//
// Control flow is whisper.cpp's [ext], restated in oracle/oracle_whisper.cpp `full()` and kept
// per clip here (prompt/temperature/seek/segments live on the host, one small struct per clip);
// the arithmetic is batched across clips: one encoder pass per group of windows, one cross-KV
// GEMM, a ragged prefill, then lockstep decode steps over every clip still decoding. Per step the
// host receives only a 32-byte TokOut per clip (plus the probs row of clips that sample at t>0).
#include <optional>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <thread>

#include "engine.h"
#include "suppress.h"
#include "token_times.h"

namespace wm {

static size_t esize(DType) { return 2; }

// device buffers: freed and nulled together, so that a workspace whose (re)allocation failed half way
// can be released as a whole (ensure_ws) and the state reused
static void dfree(void*& p) {
    if (p) { void* q = p; p = nullptr; WM_CHECK(hipFree(q)); }
}
template <typename T> static void dfree(T*& p) {
    void* q = (void*)p;
    p = nullptr;
    dfree(q);
}
template <typename T> static void dalloc(T*& p, size_t bytes) {
    void* q = nullptr;
    p = nullptr;
    WM_CHECK(hipMalloc(&q, bytes));
    p = (T*)q;
}

// ---- live kernel timing (HIP events on the state's stream) ------------------------------------------
static hipEvent_t kt_event(whisper_state* s) {
    if (!s->kpool.empty()) { hipEvent_t e = s->kpool.back(); s->kpool.pop_back(); return e; }
    hipEvent_t e;
    WM_CHECK(hipEventCreate(&e));
    return e;
}
// Record a timing event on the state's stream. While a decode step is being captured, the record
// is added as an explicit event-record node of the graph: a stream-captured hipEventRecord does
// not yield a timestamp on replay (hipEventElapsedTime -> invalid handle), an explicit node does
// (tools/probe/graph_events.hip).
static void kt_record(whisper_state* s, hipEvent_t e, hipStream_t st) {
    if (!s->capture_ev) { WM_CHECK(hipEventRecord(e, st)); return; }
    hipStreamCaptureStatus cs;
    unsigned long long id = 0;
    hipGraph_t g = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t nd = 0;
    WM_CHECK(hipStreamGetCaptureInfo_v2(st, &cs, &id, &g, &deps, &nd));
    hipGraphNode_t node;
    WM_CHECK(hipGraphAddEventRecordNode(&node, g, deps, nd, e));
    WM_CHECK(hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies));
}
// Times the launches of its scope on stream `st` (default: the state's stream) when the class is
// enabled. For K_ATTN_SELF `work` is the share of the step's rows (the bytes grow every step and
// are filled in when the events are read).
struct KT {
    whisper_state* s;
    int cls;
    double work;
    hipStream_t st;
    hipEvent_t a = nullptr;
    int sub = 0;  // (class K_VAD: the kernel)
    KT(whisper_state* s_, int c, double w, hipStream_t st_ = nullptr, bool on = true)
        : s(s_), cls(c), work(w), st(st_ ? st_ : s_->stream) {
        if (on && ((s->ktime_mask >> c) & 1)) { a = kt_event(s); kt_record(s, a, st); }
    }
    ~KT() {
        if (!a) return;
        hipEvent_t b = kt_event(s);
        kt_record(s, b, st);
        (s->capture_ev ? *s->capture_ev : s->kpending).push_back({cls, a, b, work, sub});
    }
};
static void drop_graphs(whisper_state* s) {
    for (auto& g : s->dec_graphs) {
        hipGraphExecDestroy(g.exec);
        for (auto& e : g.ev) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    }
    s->dec_graphs.clear();
}
// accumulate the timing events of one graph replay (stream already synchronised)
static void kt_flush_graph(whisper_state* s, const whisper_state::DecGraph& g) {
    for (auto& p : g.ev) {
        if (!((s->ktime_mask >> p.cls) & 1)) continue;
        float ms = 0.0f;
        const hipError_t e = hipEventElapsedTime(&ms, p.a, p.b);
        if (e != hipSuccess) {
            static bool warned = false;
            if (!warned) fprintf(stderr, "whisper_mi355x: graph kernel timing unavailable (%s)\n", hipGetErrorString(e));
            warned = true;
            continue;
        }
        s->kstat[p.cls].ms += ms;
        s->kstat[p.cls].work += p.cls == K_ATTN_SELF ? s->cur_self_work * p.work : p.work;
        s->kstat[p.cls].count++;
    }
}
void kt_flush(whisper_state* s) {
    if (s->kpending.empty()) return;
    WM_CHECK(hipStreamSynchronize(s->stream));
    for (auto& p : s->kpending) {
        float ms = 0.0f;
        WM_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
        s->kstat[p.cls].ms += ms;
        s->kstat[p.cls].work += p.cls == K_ATTN_SELF ? s->cur_self_work * p.work : p.work;
        s->kstat[p.cls].count++;
        if (p.cls == K_VAD) {
            s->vad_kstat[p.sub].ms += ms;
            s->vad_kstat[p.sub].work += p.work;
            s->vad_kstat[p.sub].count++;
        }
        s->kpool.push_back(p.a);
        s->kpool.push_back(p.b);
    }
    s->kpending.clear();
}
// GEMM launch with its algorithmic work: FLOPs for encoder-side GEMMs (MFMA-bound), HBM bytes
// (weights + activations) for decode-side GEMMs (weight-streaming)
// Decode-step split-K slabs are stored write-through (sc1): the lines leave the XCD's L2 while the
// GEMM runs instead of being written back at the kernel boundary before the reduce can start
// (MI355X_MICROARCH.md price list, "boundary": + dirty bytes / 6 TB/s). Same-box A/B, large-v3 bf16:
// decode 864 -> 824 ms per step at 128 clips, 423 -> 413 at 16 (profiles/r03_envab_slab_gelu.txt).
static void tgemm_ws(whisper_state* s, int cls, DType dt, int epi, const GemmArgs& g0, hipStream_t st, float* ws,
                     long ws_elems) {
    GemmArgs g = g0;
    if (cls == K_GEMM_DEC) { g.splitk_ws = ws; g.splitk_ws_elems = ws_elems; g.slab_wt = 1; }
    const double work = cls == K_GEMM_ENC ? 2.0 * g.M * g.N * g.K
                                          : 2.0 * g.N * g.K + 2.0 * g.M * g.K + 4.0 * g.M * g.N;
    KT kt(s, cls, work, st);
    launch_gemm(dt, epi, g, st);
}
static void tgemm(whisper_state* s, int cls, DType dt, int epi, const GemmArgs& g0, hipStream_t st) {
    tgemm_ws(s, cls, dt, epi, g0, st, s->ws.splitk, s->ws.splitk_elems);
}

static whisper_state* create_state(Context* c) {
    WM_CHECK(hipSetDevice(c->device));
    whisper_state* s = new whisper_state();
    s->ctx = c;
    s->device = c->device;
    try {
        WM_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        WM_CHECK(hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking));
        WM_CHECK(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
        WM_CHECK(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
    } catch (...) {
        if (s->ev_join) hipEventDestroy(s->ev_join);
        if (s->ev_fork) hipEventDestroy(s->ev_fork);
        if (s->stream2) hipStreamDestroy(s->stream2);
        if (s->stream) hipStreamDestroy(s->stream);
        delete s;
        throw;
    }
    std::lock_guard<std::mutex> lk(c->pool_mu);
    c->live.push_back(s);
    return s;
}

// A recycled state is a fresh whisper_state to its new owner: everything whisper_init_state would
// start from (prompt_past, the rng, results, mel, timing) is reset; only the device workspace and the
// decode graphs captured over it (keyed by active-clip count) are kept.
static void reset_for_reuse(whisper_state* s) {
    s->direct = false;
    s->results.clear();
    s->lang_ids.clear();
    s->decisions.clear();
    s->prompt_past.clear();
    s->rng = std::mt19937(0);
    s->lang_id = 0;
    s->audio_ctx = 0;
    s->n_len = s->n_len_org = 0;
    s->logits_host.clear();
    for (double& t : s->phase_ms) t = 0;
    s->align_ms = 0;
    s->tokts_ms = 0;
    s->vad_ms = 0;
    s->vad_maps.clear();
    s->align_info.clear();
    s->decoded_tokens = 0;
    s->last_enc_windows = 0;
    s->mel_ready = false;
    s->ktime_mask = 0;
    for (auto& k : s->kstat) k = KStat();
    for (auto& k : s->vad_kstat) k = KStat();
    s->cur_self_work = 0;
    s->pdec_give_ups = 0;
    s->pdec_lost_ms = 0;
    s->pdec_off_until = 0;
    s->pdec_off = false;
    s->mode = StepMode{};
    s->deny_on = false;
    s->gram_on = false;
    s->filter_on = s->tdrz_on = false;
    s->ws.gd.host_masks.clear();
    s->ws.gd.rows_device = s->ws.gd.rows_patched = s->ws.gd.rows_host = 0;
    s->beam_info.clear();
    s->sample_seed = 0;
    s->cand_info.clear();
    s->gather_rows = s->gather_rows_full = 0;
    std::fill(s->ws.cross_fresh.begin(), s->ws.cross_fresh.end(), 0);
}

// states kept per context, and the largest workspace kept (clips): the app's pattern is one clip per
// call (whisper.rs:83-85, state.rs:147); a batch-sized workspace is released, not kept
static int pool_states() {
    const char* e = getenv("WHISPER_MI355X_STATE_POOL");
    return e ? std::max(0, atoi(e)) : 2;
}
static const int kPoolMaxJobs = 16;

whisper_state* new_state(Context* c) {
    {
        std::lock_guard<std::mutex> lk(c->pool_mu);
        if (!c->pool.empty()) {
            whisper_state* s = c->pool.back();
            c->pool.pop_back();
            reset_for_reuse(s);
            s->pooled = true;
            return s;
        }
    }
    return create_state(c);
}

static void free_ws(Workspace& w);

static void destroy_state(whisper_state* s) {
    if (s->twin) {
        destroy_state(s->twin);
        s->twin = nullptr;
    }
    if (Context* c = s->ctx) {
        std::lock_guard<std::mutex> lk(c->pool_mu);
        c->live.erase(std::remove(c->live.begin(), c->live.end(), s), c->live.end());
    }
    hipSetDevice(s->device);
    hipStreamSynchronize(s->stream);
    hipStreamSynchronize(s->stream2);
    drop_graphs(s);
    try { free_ws(s->ws); } catch (const Error&) {}
    for (auto& p : s->kpending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (hipEvent_t e : s->kpool) hipEventDestroy(e);
    hipEventDestroy(s->ev_fork);
    hipEventDestroy(s->ev_join);
    hipStreamDestroy(s->stream2);
    hipStreamDestroy(s->stream);
    delete s;
}

void free_state(whisper_state* s) {
    if (!s) return;
    Context* c = s->ctx;
    if (!c) {  // its context is gone: nothing to pool into
        destroy_state(s);
        return;
    }
    hipSetDevice(c->device);
    const bool healthy = hipStreamSynchronize(s->stream) == hipSuccess && hipStreamSynchronize(s->stream2) == hipSuccess &&
                         s->kpending.empty();
    if (healthy && s->ws.cap_jobs <= kPoolMaxJobs) {
        std::lock_guard<std::mutex> lk(c->pool_mu);
        if ((int)c->pool.size() < pool_states()) {
            c->pool.push_back(s);
            return;
        }
    }
    destroy_state(s);
}

void drain_state_pool(Context* c) {
    std::vector<whisper_state*> p;
    {
        std::lock_guard<std::mutex> lk(c->pool_mu);
        p.swap(c->pool);
    }
    for (whisper_state* s : p) destroy_state(s);
}

void orphan_states(Context* c) {
    std::lock_guard<std::mutex> lk(c->pool_mu);
    for (whisper_state* s : c->live) s->ctx = nullptr;
    c->live.clear();
}

void recover_state(whisper_state* s) {
    if (!s) return;
    hipSetDevice(s->device);
    for (hipStream_t st : {s->stream, s->stream2}) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            hipGraph_t g = nullptr;
            hipStreamEndCapture(st, &g);
            if (g) hipGraphDestroy(g);
        }
    }
    s->capture_ev = nullptr;
    s->mode = StepMode{};
    hipStreamSynchronize(s->stream);
    hipStreamSynchronize(s->stream2);
    (void)hipGetLastError();
    for (auto& p : s->kpending) { s->kpool.push_back(p.a); s->kpool.push_back(p.b); }
    s->kpending.clear();
}

// the token-timestamp alignment's buffers (ensure_align)
static void free_align(Workspace& w) {
    dfree(w.al_clips); dfree(w.al_P); dfree(w.al_stats); dfree(w.al_cost); dfree(w.al_trace); dfree(w.al_fr);
    if (w.h_al) { char* q = w.h_al; w.h_al = nullptr; WM_CHECK(hipHostFree(q)); }
    w.al_P_elems = 0;
    w.al_cap = w.al_rows = 0;
}

static void free_ws(Workspace& w) {
    free_align(w);
    // sub-allocations (pos/slot/.. of tok, win_seek/win_slot of win_job, pcm_ptrs/n_* of mel_ptrs)
    // are freed with their parent
    dfree(w.mel_img); dfree(w.h1); dfree(w.hn); dfree(w.qkv); dfree(w.att); dfree(w.ff); dfree(w.x);
    dfree(w.cross); dfree(w.self); dfree(w.dx); dfree(w.dh); dfree(w.dq); dfree(w.datt); dfree(w.dff);
    dfree(w.lrow); dfree(w.logits); dfree(w.probs); dfree(w.tok); dfree(w.ctl); dfree(w.tout); dfree(w.lrec); dfree(w.win_job);
    dfree(w.pcm); dfree(w.mel); dfree(w.mel_ptrs); dfree(w.splitk); dfree(w.enc); dfree(w.qx); dfree(w.xo);
    dfree(w.xml); dfree(w.kvslot); dfree(w.hs); dfree(w.qtiles); dfree(w.wdq); dfree(w.pd_sync);
    dfree(w.sslot); dfree(w.cand); dfree(w.kvcp); dfree(w.kvstage); dfree(w.sctr);
    dfree(w.energy); dfree(w.tt_clips); dfree(w.tt_segs); dfree(w.tt_spans); dfree(w.deny); dfree(w.gram);
    if (w.h_gram) hipHostFree(w.h_gram);
    dfree(w.frows);
    if (w.h_frows) hipHostFree(w.h_frows);
    gram_dev_free(w.gd);
    vad_scratch_free(w.vad);
    if (w.h_sslot) hipHostFree(w.h_sslot);
    if (w.h_sctr) hipHostFree(w.h_sctr);
    if (w.h_cand) hipHostFree(w.h_cand);
    if (w.h_kvcp) hipHostFree(w.h_kvcp);
    if (w.h_pd_err) hipHostFree(w.h_pd_err);
    if (w.h_ring) hipHostFree(w.h_ring);
    for (auto& e : w.ring_ev)
        if (e) hipEventDestroy(e);
    if (w.h_ints) hipHostFree(w.h_ints);
    if (w.h_qtiles) hipHostFree(w.h_qtiles);
    if (w.h_tout) hipHostFree(w.h_tout);
    if (w.h_ctl) hipHostFree(w.h_ctl);
    w = Workspace();
}

// prefills with at most this many tokens per clip take the direct cross attention; longer prompts
// go through a cross K/V cache computed for their clips on demand
static const int kXDirectMaxTok = 8;
// lazy-rescale threshold of the direct cross attention's online softmax (log2 units: P <= 2^8)
static const float kXattnThr = 8.0f;

// Cross attention form per call. The direct form reads E once per clip and layer (half the bytes of
// the cached K + V) but its split partials are [H][d] per (clip, split) whatever the batch, and it
// adds two launches per layer (Q' projection, combine); at a few clips a step is launch- and
// latency-bound and the cached form (one attention kernel, whisper.cpp's own numerics) wins: the
// cross K/V of a window then costs one GEMM at encode time. WHISPER_MI355X_CROSS=direct|cache
// forces a form; otherwise direct above 32 clips.
static bool pick_direct(Context* c, int n_jobs) {
    if (!c->cross_direct) return false;
    // read per call (tests switch the form per case)
    const char* e = getenv("WHISPER_MI355X_CROSS");
    if (e && strcmp(e, "direct") == 0) return true;
    if (e && strcmp(e, "cache") == 0) return false;
    return n_jobs > 32;
}

// encoder windows per launch group. Round 6: 128 (a whole headline batch per launch): the encoder GEMMs'
// 256 x 256 tiles then fill their last round of 256 CUs (32 windows: QKV 2820 tiles = 11.02 rounds, i.e. a 12th
// round of 4 tiles; 128 windows: 11250 = 43.9), and the encoder attention's grid is 30 whole rounds: encode
// 313.6 -> 304.1 ms per step, 3384 -> 3402 audio-s/s (profiles/r06_encb_ab_*.json; round 2 had measured 32 / 64 /
// 128 the same). ~6.5 GB of encoder activations for large-v3. WHISPER_MI355X_ENC_BATCH overrides it.
static int enc_batch() {
    static const int v = getenv("WHISPER_MI355X_ENC_BATCH") ? std::max(1, atoi(getenv("WHISPER_MI355X_ENC_BATCH"))) : 128;
    return v;
}

// Cross K/V cache for at least `slots` slots (cache form: the call's clips; direct form: the clips
// whose prompts are too long for the direct prefill). Sized by the calls that use it, so a state
// that ran a large direct-form batch does not allocate a cache for all of its slots later.
// A reallocation drops the state's decode graphs first: a captured cache-form step holds the old
// w.cross pointer, and the cross cache is sized apart from cap_jobs (a direct-form call of > 32 clips
// followed by cache-form calls of 8 and then 16 clips regrows it under graphs captured at 8).
static void ensure_cross(Context* c, whisper_state* s, int slots) {
    Workspace& w = s->ws;
    if (w.cross && w.cap_cross >= slots) return;
    const Hparams& hp = c->hp;
    WM_CHECK(hipStreamSynchronize(s->stream));
    WM_CHECK(hipStreamSynchronize(s->stream2));
    drop_graphs(s);
    dfree(w.cross);
    w.cap_cross = 0;
    std::fill(w.cross_fresh.begin(), w.cross_fresh.end(), 0);
    dalloc(w.cross, (size_t)slots * hp.n_text_layer * 2 * hp.n_audio_ctx * hp.n_audio_state * esize(c->dt));
    w.cap_cross = slots;
}

// (Re)allocate the workspace for n_jobs clips. Encoder activations are sized for at most
// enc_batch() windows at once; caches for n_jobs slots. If an allocation fails (out of memory),
// the whole workspace is released and the error propagates: the state stays usable (empty).
// Beam search passes its decoder rows (clips x beams) as n_jobs and its clips as n_clips: the self cache and
// the per-row buffers hold every beam, the encoder activations and the cross K/V cache only the clips.
static void ensure_ws_impl(Context* c, whisper_state* s, int n_jobs, int n_clips) {
    Workspace& w = s->ws;
    const Hparams& hp = c->hp;
    const size_t d = hp.n_audio_state, nm = hp.n_mels, T = hp.n_audio_ctx, E = esize(c->dt);
    const int n_enc = std::min(n_clips, enc_batch());
    if (n_enc > w.cap_enc || n_jobs > w.cap_jobs) drop_graphs(s);
    if (!w.deny) dalloc(w.deny, (size_t)suppress_words(hp.n_vocab) * sizeof(uint32_t));  // (kept when the workspace grows)
    if (n_enc > w.cap_enc) {
        dfree(w.mel_img); dfree(w.h1); dfree(w.hn); dfree(w.qkv); dfree(w.att); dfree(w.ff); dfree(w.x);
        dfree(w.win_job); dfree(w.hs);
        w.cap_enc = 0;
        dalloc(w.mel_img, (size_t)n_enc * 3002 * nm * E);
        dalloc(w.h1, (size_t)n_enc * 3002 * d * E);
        WM_CHECK(hipMemset(w.h1, 0, (size_t)n_enc * 3002 * d * E));  // conv padding rows stay zero
        dalloc(w.hn, (size_t)n_enc * T * d * E);
        dalloc(w.qkv, (size_t)n_enc * T * 3 * d * E);
        dalloc(w.att, (size_t)n_enc * T * d * E);
        dalloc(w.ff, (size_t)n_enc * T * 4 * d * E);
        dalloc(w.x, (size_t)n_enc * T * d * 4);
        if (c->fp8_enc) {
            dalloc(w.hs, (size_t)n_enc * T * sizeof(float));
        }
        dalloc(w.win_job, (size_t)n_enc * 3 * sizeof(int));
        w.win_seek = w.win_job + n_enc;
        w.win_slot = w.win_job + 2 * n_enc;
        w.cap_enc = n_enc;
    }
    if (n_jobs > w.cap_jobs) {
        const int L = hp.n_text_layer;
        const int n_tok = n_jobs * (hp.n_text_ctx / 2 + 8);
        dfree(w.cross); dfree(w.self); dfree(w.dx); dfree(w.dh); dfree(w.dq); dfree(w.datt); dfree(w.dff);
        dfree(w.lrow); dfree(w.logits); dfree(w.probs); dfree(w.tok); dfree(w.ctl); dfree(w.tout); dfree(w.lrec); dfree(w.mel_ptrs);
        dfree(w.splitk); dfree(w.enc); dfree(w.qx); dfree(w.xo); dfree(w.xml); dfree(w.kvslot); dfree(w.qtiles);
        free_align(w);  // sized by cap_jobs
        for (auto& a : s->align_info) a = {};  // (pointers into al_cost)
        if (w.h_ring) { WM_CHECK(hipHostFree(w.h_ring)); w.h_ring = nullptr; w.ring = nullptr; }
        dfree(w.sslot); dfree(w.cand); dfree(w.kvcp); dfree(w.sctr); dfree(w.gram);
        dfree(w.frows);  // (sized by cap_jobs: ensure_filter_rows allocates them again for a call that has a callback)
        for (void** h : {(void**)&w.h_qtiles, (void**)&w.h_ints, (void**)&w.h_tout, (void**)&w.h_ctl, (void**)&w.h_sslot,
                         (void**)&w.h_cand, (void**)&w.h_kvcp, (void**)&w.h_sctr, (void**)&w.h_gram, (void**)&w.h_frows})
            if (*h) { void* q = *h; *h = nullptr; WM_CHECK(hipHostFree(q)); }
        w.cap_jobs = w.cap_tok = w.cap_cross = w.cap_xq = 0;
        // split-K slabs: decode steps (<= 128 rows per group, two concurrent groups) and the prefill
        // GEMMs below the big-GEMM size (M*N < 2^22), whose split count depends on N and K only
        // (kernels/gemm.hip dec_splits_for: splits * N <= 16384, <= 12 splits)
        w.splitk_elems = std::max(16L * std::min(n_tok, 256) * 4 * (long)d, std::min(16384L * n_tok, 12L << 22));
        dalloc(w.splitk, w.splitk_elems * 4);
        w.cross_fresh.assign(n_jobs, 0);
        {
            std::vector<int> ident(n_jobs);
            for (int k = 0; k < n_jobs; k++) ident[k] = k;
            dalloc(w.kvslot, (size_t)n_jobs * sizeof(int));
            WM_CHECK(hipMemcpy(w.kvslot, ident.data(), (size_t)n_jobs * sizeof(int), hipMemcpyHostToDevice));
        }
        dalloc(w.self, (size_t)n_jobs * L * 2 * hp.n_text_ctx * d * E);
        dalloc(w.dx, (size_t)n_tok * d * 4);
        dalloc(w.dh, (size_t)n_tok * d * E);
        dalloc(w.dq, (size_t)n_tok * d * E);
        dalloc(w.datt, (size_t)n_tok * d * E);
        dalloc(w.dff, (size_t)n_tok * 4 * d * E);
        dalloc(w.lrow, (size_t)n_jobs * d * E);
        dalloc(w.logits, (size_t)n_jobs * hp.n_vocab * 4);
        dalloc(w.probs, (size_t)n_jobs * 2 * hp.n_vocab * 4);
        dalloc(w.tok, ((size_t)5 * n_tok + n_jobs) * sizeof(int));
        w.pos = w.tok + n_tok;
        w.slot = w.tok + 2 * n_tok;
        w.nkv_self = w.tok + 3 * n_tok;
        w.nkv_cross = w.tok + 4 * n_tok;
        w.lrows = w.tok + 5 * n_tok;
        dalloc(w.ctl, (size_t)n_jobs * sizeof(SeqCtl));
        dalloc(w.tout, (size_t)n_jobs * sizeof(TokOut));
        dalloc(w.lrec, logits_rec_bytes(n_jobs));
        dalloc(w.mel_ptrs, (size_t)n_jobs * (2 * sizeof(void*) + 3 * sizeof(int)));
        w.pcm_ptrs = (const float**)(w.mel_ptrs + n_jobs);
        w.n_samp = (int*)(w.pcm_ptrs + n_jobs);
        w.n_len = w.n_samp + n_jobs;
        w.mel_max = w.n_len + n_jobs;
        WM_CHECK(hipHostMalloc((void**)&w.h_ints, ((size_t)5 * n_tok + n_jobs) * sizeof(int) + 64, 0));
        dalloc(w.qtiles, (size_t)n_tok * sizeof(int2));
        WM_CHECK(hipHostMalloc((void**)&w.h_qtiles, (size_t)n_tok * sizeof(int2), 0));
        WM_CHECK(hipHostMalloc((void**)&w.h_tout, (size_t)n_jobs * sizeof(TokOut), 0));
        WM_CHECK(hipHostMalloc((void**)&w.h_ctl, (size_t)n_jobs * sizeof(SeqCtl), 0));
        dalloc(w.sslot, (size_t)n_jobs * sizeof(int));
        dalloc(w.cand, (size_t)n_jobs * kTopkMax * sizeof(TokOut));
        dalloc(w.kvcp, (size_t)n_jobs * sizeof(KvCopy));
        WM_CHECK(hipHostMalloc((void**)&w.h_sslot, (size_t)n_jobs * sizeof(int), 0));
        WM_CHECK(hipHostMalloc((void**)&w.h_cand, (size_t)n_jobs * kTopkMax * sizeof(TokOut), 0));
        WM_CHECK(hipHostMalloc((void**)&w.h_kvcp, (size_t)n_jobs * sizeof(KvCopy), 0));
        dalloc(w.sctr, (size_t)n_jobs * 4 * sizeof(int));
        WM_CHECK(hipHostMalloc((void**)&w.h_sctr, (size_t)n_jobs * 4 * sizeof(int), 0));
        dalloc(w.gram, (size_t)n_jobs * grammar_words(hp.n_vocab) * sizeof(uint32_t));
        WM_CHECK(hipHostMalloc((void**)&w.h_gram, (size_t)n_jobs * grammar_words(hp.n_vocab) * sizeof(uint32_t), 0));
        w.cap_jobs = n_jobs;
        w.cap_tok = n_tok;
    }
    // the buffers of this call's cross attention form (allocated on first use, kept)
    if (s->direct && !w.enc) {
        // no cross K/V cache up front: decode steps (and short prefills) read E directly
        const int H = hp.n_text_head;
        w.cap_xq = std::max(kXDirectMaxTok * w.cap_jobs, 128);
        // n * xattn_splits(n) <= max(n, 255 + n) per row group; two concurrent groups at most double it
        const size_t xo_rows = (size_t)std::max(w.cap_xq, 512) + w.cap_jobs + 512;
        dalloc(w.enc, (size_t)w.cap_jobs * T * d * E);
        dalloc(w.qx, (size_t)w.cap_xq * 2 * H * d * E);
        dalloc(w.xo, xo_rows * H * d * 4);
        dalloc(w.xml, xo_rows * H * 2 * 4);
    }
    if (!s->direct) ensure_cross(c, s, n_clips);
    if (c->quant && !w.wdq) dalloc(w.wdq, (size_t)16 * d * d * E);
}

static void ensure_ws(Context* c, whisper_state* s, int n_jobs, int n_clips = -1) {
    try {
        ensure_ws_impl(c, s, n_jobs, n_clips < 0 ? n_jobs : n_clips);
    } catch (const Error&) {
        hipStreamSynchronize(s->stream);
        hipStreamSynchronize(s->stream2);
        drop_graphs(s);
        free_ws(s->ws);
        throw;
    }
}

// ---- mel ------------------------------------------------------------------------------------------
static inline int mel_n_len(int n) { return (n + 16000 * 30) / 160; }
static inline int mel_n_len_org(int n) { return 1 + (int)(((int64_t)n + 200 - 400) / 160); }

int compute_mel(Context* c, whisper_state* s, const float* const* pcm, const int* n, int n_jobs, bool on_device) {
    s->direct = pick_direct(c, n_jobs);
    ensure_ws(c, s, n_jobs);
    Workspace& w = s->ws;
    const int nm = c->hp.n_mels;
    size_t pcm_tot = 0, mel_tot = 0;
    int max_frames = 1;
    for (int j = 0; j < n_jobs; j++) {
        pcm_tot += ((size_t)n[j] + 63) & ~(size_t)63;
        mel_tot += (size_t)nm * mel_n_len(n[j]);
        max_frames = std::max(max_frames, std::min((n[j] + 200) / 160 + 1, mel_n_len(n[j])));
    }
    if (!on_device && pcm_tot > w.cap_pcm) {
        dfree(w.pcm);
        w.cap_pcm = 0;
        dalloc(w.pcm, pcm_tot * 4);
        w.cap_pcm = pcm_tot;
    }
    if (mel_tot > w.cap_mel) {
        dfree(w.mel);
        w.cap_mel = 0;
        dalloc(w.mel, mel_tot * 4);
        w.cap_mel = mel_tot;
    }
    std::vector<const float*> pp(n_jobs);
    std::vector<float*> mp(n_jobs);
    std::vector<int> ints(3 * n_jobs);
    size_t po = 0, mo = 0;
    for (int j = 0; j < n_jobs; j++) {
        if (on_device) pp[j] = pcm[j];
        else {
            pp[j] = w.pcm + po;
            if (n[j] > 0) WM_CHECK(hipMemcpyAsync(w.pcm + po, pcm[j], (size_t)n[j] * 4, hipMemcpyHostToDevice, s->stream));
            po += ((size_t)n[j] + 63) & ~(size_t)63;
        }
        mp[j] = w.mel + mo;
        mo += (size_t)nm * mel_n_len(n[j]);
        ints[j] = n[j];
        ints[n_jobs + j] = mel_n_len(n[j]);
    }
    // one host block -> device, laid out as the workspace carves it (ensure_ws: arrays of cap_jobs
    // entries, whatever this call's clip count): [mel ptrs][pcm ptrs][n][n_len] ([max] is the kernel's)
    const size_t cap = w.cap_jobs;
    std::vector<char> blk(cap * (2 * sizeof(void*) + 2 * sizeof(int)));
    memcpy(blk.data(), mp.data(), n_jobs * sizeof(void*));
    memcpy(blk.data() + cap * sizeof(void*), pp.data(), n_jobs * sizeof(void*));
    memcpy(blk.data() + 2 * cap * sizeof(void*), ints.data(), n_jobs * sizeof(int));
    memcpy(blk.data() + 2 * cap * sizeof(void*) + cap * sizeof(int), ints.data() + n_jobs, n_jobs * sizeof(int));
    WM_CHECK(hipMemcpyAsync(w.mel_ptrs, blk.data(), blk.size(), hipMemcpyHostToDevice, s->stream));
    {
        double bytes = 0;
        for (int j = 0; j < n_jobs; j++)
            bytes += 4.0 * n[j] + 4.0 * nm * std::min((n[j] + 200) / 160 + 1, mel_n_len(n[j]));
        KT kt(s, K_MEL, bytes);
        launch_mel(w.pcm_ptrs, w.n_samp, c->w.mel_tab, c->w.filt_t, nm, w.mel_ptrs, w.n_len, w.mel_max, n_jobs, max_frames,
                   s->stream);
    }
    WM_CHECK(hipStreamSynchronize(s->stream));  // blk (pageable) must outlive the copy
    s->n_len = mel_n_len(n[0]);
    s->n_len_org = mel_n_len_org(n[0]);
    s->mel_ready = true;
    return 0;
}

// ---- token times: the clips' energy signals (whisper_full_params.token_timestamps) -------------
template <typename T> static void tt_grow(T*& p, int& cap, size_t need) {
    if ((size_t)cap >= need) return;
    dfree(p);
    cap = 0;
    const size_t n = std::max(need, (size_t)64);
    dalloc(p, n * sizeof(T));
    cap = (int)n;
}

// After compute_mel of the same call, from the same device PCM: the caller's buffers (on_device), else w.pcm,
// where compute_mel put every clip on a 64-float boundary. The energy buffer has that layout.
static void compute_energy(whisper_state* s, const float* const* pcm, const int* n, int n_jobs, bool on_device) {
    Workspace& w = s->ws;
    std::vector<TtClip> cl(n_jobs);
    size_t off = 0;
    int max_n = 0;
    double bytes = 0;
    for (int j = 0; j < n_jobs; j++) {
        cl[j] = TtClip{on_device ? pcm[j] : w.pcm + off, (long long)off, n[j], 0};
        off += ((size_t)n[j] + 63) & ~(size_t)63;
        max_n = std::max(max_n, n[j]);
        bytes += 8.0 * n[j];
    }
    if (off > w.cap_energy) {
        dfree(w.energy);
        w.cap_energy = 0;
        dalloc(w.energy, off * 4);
        w.cap_energy = off;
    }
    tt_grow(w.tt_clips, w.tt_cap_clips, (size_t)n_jobs);
    WM_CHECK(hipMemcpyAsync(w.tt_clips, cl.data(), cl.size() * sizeof(TtClip), hipMemcpyHostToDevice, s->stream));
    {
        KT kt(s, K_TOKTS, bytes);
        launch_signal_energy(w.tt_clips, n_jobs, max_n, w.energy, s->stream);
    }
    WM_CHECK(hipStreamSynchronize(s->stream));  // cl (pageable) must outlive the copy
}

// ---- encoder + cross KV ---------------------------------------------------------------------------
// fp8 mode, decoder half: WHISPER_MI355X_FP8_DEC=1 (read when a context first quantizes its weights).
// Off by default: correct (tests/test_gpu_fp8.py) but slower, because the decode-step GEMMs are
// latency-bound, not bound by their weight bytes (profiles/r02_fp8_decoder_ab.txt: large-v3 fp8 at
// 128 clips decode 849 -> 936 ms per step, turbo fp8 at 256 clips 193 -> 210 ms).
static bool dec_fp8() {
    const char* e = getenv("WHISPER_MI355X_FP8_DEC");
    return e && atoi(e) == 1;
}

// fp8 encoder weights: e4m3 copies of QKV, FC1 and FC2 with per-output-row scales, quantized on the
// device from the bf16 weights once per context (after load or the RCCL weight broadcast); in the
// same arena the decoder's decode-step projections (dec_fp8()).
static void ensure_fp8(Context* c) {
    std::lock_guard<std::mutex> lk(c->fp8_mu);
    if (c->fp8_ready) return;
    const Hparams& hp = c->hp;
    const size_t d = hp.n_audio_state, nl = hp.n_audio_layer;
    const size_t per = 3 * d * d + 4 * d * d + 4 * d * d, per_s = (3 * d + 4 * d + d) * sizeof(float);
    // decoder: wqkv [3t][t], wo / wxq / wxo [t][t], w1 [4t][t], w2 [t][4t] (+ one f32 scale per row)
    const size_t t = hp.n_text_state, nd = dec_fp8() ? hp.n_text_layer : 0;
    const size_t per_d = 14 * t * t, per_ds = (3 * t + 3 * t + 4 * t + t) * sizeof(float);
    WM_CHECK(hipSetDevice(c->device));
    dalloc(c->arena8, nl * (per + per_s) + nd * (per_d + per_ds));
    c->enc8.assign(nl, Context::Fp8Layer{});
    char* p = c->arena8;
    for (size_t l = 0; l < nl; l++) {
        Context::Fp8Layer& f = c->enc8[l];
        const LayerW& L = c->w.enc[l];
        f.wqkv = p; p += 3 * d * d;
        f.w1 = p; p += 4 * d * d;
        f.w2 = p; p += 4 * d * d;
        f.sqkv = (float*)p; p += 3 * d * sizeof(float);
        f.s1 = (float*)p; p += 4 * d * sizeof(float);
        f.s2 = (float*)p; p += d * sizeof(float);
        launch_quant_rows_fp8(c->dt, L.wqkv, 3 * d, (int)d, f.wqkv, f.sqkv, nullptr);
        launch_quant_rows_fp8(c->dt, L.w1, 4 * d, (int)d, f.w1, f.s1, nullptr);
        launch_quant_rows_fp8(c->dt, L.w2, d, (int)(4 * d), f.w2, f.s2, nullptr);
    }
    c->dec8.assign(nd, Context::Fp8Dec{});
    for (size_t l = 0; l < nd; l++) {
        Context::Fp8Dec& f = c->dec8[l];
        const LayerW& L = c->w.dec[l];
        auto q = [&](const void* w, size_t rows, size_t cols, void*& q8, float*& sc) {
            q8 = p; p += rows * cols;
            sc = (float*)p; p += rows * sizeof(float);
            launch_quant_rows_fp8(c->dt, w, (long)rows, (int)cols, q8, sc, nullptr);
        };
        q(L.wqkv, 3 * t, t, f.wqkv, f.sqkv);
        q(L.wo, t, t, f.wo, f.so);
        q(L.wxq, t, t, f.wxq, f.sxq);
        q(L.wxo, t, t, f.wxo, f.sxo);
        q(L.w1, 4 * t, t, f.w1, f.s1);
        q(L.w2, t, 4 * t, f.w2, f.s2);
    }
    WM_CHECK(hipDeviceSynchronize());
    c->fp8_ready = true;
}

// fp8 mode, FC1 -> FC2: the GELU output is re-quantized per row (one pass). An MX hand-off (FC1's
// epilogue quantizing per 32-column block for a block-scaled FC2) measured slower on turbo at 256 clips
// (encode 743-815 vs 578 ms per step: the MX-A FC2 tile spilled past 256 VGPRs) and was removed.
static void tgemm_fp8(whisper_state* s, int epi, const GemmArgs& g, const float* sa, const float* sb, hipStream_t st) {
    KT kt(s, K_GEMM_ENC, 2.0 * g.M * g.N * g.K, st);
    launch_gemm_fp8(s->ctx->dt, epi, g, sa, sb, st);
}

// Encoder FC1 GELU. f16 (whisper.cpp's CPU numerics, the parity mode): ggml's f16 GELU table
// (EPI_GELU), bit-exact with the oracle. bf16: the tanh formula in f32 (EPI_GELU_F; ggml-metal, the
// reference app's back-end (whisper.rs:40 use_gpu), evaluates GELU by formula too, and the epilogue
// stages no 75.8 KB table per tile): encode 340 -> 336 ms per step at 128 clips
// (profiles/r03_envab_slab_gelu.txt).
static int enc_gelu_epi(DType dt) { return dt == DType::BF16 ? EPI_GELU_F : EPI_GELU; }

// Projection weights of one layer in the compute type: the arena's matrices, or, for a block-quantized
// file, the context's expanded copy (ensure_expanded: every projection dequantized once per context,
// 3.2 GB for large-v3, on first use outside a graph capture). The encoder, the prefill and the decode
// steps of many clips are big-M GEMMs that read every weight many times, so they read the copy; the
// decode steps of few clips stream the blocks themselves (gemm_small_kernel, the persistent step).
// Until the copy exists (a first use inside a capture) a layer is dequantized into the state's scratch.
using LayerMats = Context::LayerMats;
// (returns the end of the layer's matrices in p)
static char* dequant_layer(Context* c, const LayerW& L, char* p, LayerMats& m, hipStream_t st) {
    const int d = c->hp.n_audio_state;
    const size_t E = esize(c->dt);
    // one launch for the layer when its blocks share one type (a ggml file quantizes every projection
    // alike), else one per matrix
    DequantJobs J;
    bool one_type = true;
    auto one = [&](const QMat& q, long rows, int K, const void*& dst) {
        if (!q.type) return;
        if (J.n && q.type != J.q[0].type) one_type = false;
        J.q[J.n] = q; J.rows[J.n] = rows; J.K[J.n] = K; J.out[J.n] = p; J.n++;
        dst = p;
        p += (size_t)rows * K * E;
    };
    one(L.qqkv, 3L * d, d, m.wqkv);
    one(L.qo, d, d, m.wo);
    one(L.qxq, d, d, m.wxq);
    one(L.qxo, d, d, m.wxo);
    one(L.q1, 4L * d, d, m.w1);
    one(L.q2, d, 4 * d, m.w2);
    if (one_type) launch_dequant_multi(c->dt, J, st);
    else
        for (int j = 0; j < J.n; j++) launch_dequant(c->dt, J.q[j], J.rows[j], J.K[j], J.out[j], st);
    return p;
}

static void ensure_expanded(Context* c, hipStream_t st) {
    if (!c->quant || c->expanded.load(std::memory_order_acquire)) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    WM_CHECK(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone) return;
    std::lock_guard<std::mutex> lk(c->exp_mu);
    if (c->expanded.load(std::memory_order_relaxed)) return;
    // encoder layers: QKV, out, FC1, FC2 = 12 d^2; decoder layers + cross Q, cross out = 14 d^2
    const size_t d = c->hp.n_audio_state;
    dalloc(c->arena_exp, (12 * c->w.enc.size() + 14 * c->w.dec.size()) * d * d * esize(c->dt));
    char* p = c->arena_exp;
    auto fill = [&](const std::vector<LayerW>& layers, std::vector<LayerMats>& out) {
        out.resize(layers.size());
        for (size_t l = 0; l < layers.size(); l++) {
            const LayerW& L = layers[l];
            out[l] = LayerMats{L.wqkv, L.wo, L.wxq, L.wxo, L.w1, L.w2};
            p = dequant_layer(c, L, p, out[l], st);
        }
    };
    fill(c->w.enc, c->exp_enc);
    fill(c->w.dec, c->exp_dec);
    WM_CHECK(hipStreamSynchronize(st));  // other states' streams read the copy from now on
    c->expanded.store(true, std::memory_order_release);
}

static LayerMats layer_mats(Context* c, whisper_state* s, bool dec, int l, hipStream_t st) {
    const LayerW& L = dec ? c->w.dec[l] : c->w.enc[l];
    LayerMats m{L.wqkv, L.wo, L.wxq, L.wxo, L.w1, L.w2};
    if (!c->quant) return m;
    ensure_expanded(c, st);
    if (c->expanded.load(std::memory_order_acquire)) return dec ? c->exp_dec[l] : c->exp_enc[l];
    dequant_layer(c, L, (char*)s->ws.wdq, m, st);
    return m;
}

int encode_windows(Context* c, whisper_state* s, const int* jobs, const int* seeks, const int* slots, int n_win) {
    const Hparams& hp = c->hp;
    Workspace& w = s->ws;
    // T: the encoder positions of this call (whisper_full_params.audio_ctx). The conv images keep
    // their 3002-row layout and the cross cache its n_audio_ctx-row planes; hn, qkv, att, ff, x and the direct
    // form's E hold T rows per window, packed.
    const int d = hp.n_audio_state, nm = hp.n_mels, T = enc_ctx(c, s), H = hp.n_audio_head;
    const DType dt = c->dt;
    const size_t E = esize(dt);
    const int KCLS = K_GEMM_ENC;
    const Weights& W = c->w;
    hipStream_t st = s->stream;
    const bool fp8 = c->fp8_enc && d % 128 == 0;
    if (fp8) ensure_fp8(c);
    for (int b0 = 0; b0 < n_win; b0 += w.cap_enc) {
        const int nb = std::min(w.cap_enc, n_win - b0);
        int* hi = w.h_ints;
        for (int i = 0; i < nb; i++) { hi[i] = jobs[b0 + i]; hi[nb + i] = seeks[b0 + i]; hi[2 * nb + i] = slots[b0 + i]; }
        WM_CHECK(hipMemcpyAsync(w.win_job, hi, 3 * nb * sizeof(int), hipMemcpyHostToDevice, st));
        const int* d_job = w.win_job;
        const int* d_seek = w.win_job + nb;
        const int* d_slot = w.win_job + 2 * nb;
        launch_mel_window(dt, w.mel_ptrs, w.n_len, w.n_samp, w.mel_max, d_job, d_seek, nb, nm, 2 * T, w.mel_img, st);
        // conv1 (stride 1, pad 1) + GELU -> h1 rows 1..2T of each 3002-row image (conv2's last position reads
        // rows 2T - 2 .. 2T: no row past the ones written here)
        {
            GemmArgs g = gemm_plain(w.mel_img, nb * 2 * T, 3 * nm, W.conv1_w, d, W.conv1_b, w.h1, d);
            g.a_rpb = 2 * T; g.a_bstride = (long)3002 * nm; g.a_rstride = nm;
            g.o_rpb = 2 * T; g.o_bstride = 3002; g.o_off = 1;
            tgemm(s, KCLS, dt, EPI_GELU, g, st);
        }
        // conv2 (stride 2, pad 1) + GELU + positional embedding -> residual stream x (f32)
        {
            GemmArgs g = gemm_plain(w.h1, nb * T, 3 * d, W.conv2_w, d, W.conv2_b, w.x, d);
            g.a_rpb = T; g.a_bstride = (long)3002 * d; g.a_rstride = 2 * d;
            g.pos = W.pos_e; g.pos_rows = T;
            tgemm(s, KCLS, dt, EPI_GELU_POS, g, st);
        }
        const int M = nb * T;
        for (int l = 0; l < hp.n_audio_layer; l++) {
            const LayerW& L = W.enc[l];
            if (fp8) {
                // e4m3 path: LN quantized per row into hn (bytes), QKV/FC1/FC2 on the fp8 MFMA; the
                // GELU output is re-quantized per row into the qkv buffer (free again after attention)
                const Context::Fp8Layer& F = c->enc8[l];
                launch_layernorm_fp8(w.x, M, d, L.ln1_w, L.ln1_b, w.hn, w.hs, st);
                tgemm_fp8(s, EPI_STORE, gemm_plain(w.hn, M, d, F.wqkv, 3 * d, L.bqkv, w.qkv, 3 * d), w.hs, F.sqkv, st);
                {
                    KT kt(s, K_ATTN_ENC, 4.0 * nb * H * (double)T * T * 64);
                    launch_attn_encoder(dt, w.qkv, w.att, nb, T, d, H, st);
                }
                tgemm(s, KCLS, dt, EPI_RESID, gemm_plain(w.att, M, d, L.wo, d, L.bo, w.x, d), st);
                launch_layernorm_fp8(w.x, M, d, L.ln2_w, L.ln2_b, w.hn, w.hs, st);
                tgemm_fp8(s, EPI_GELU_F, gemm_plain(w.hn, M, d, F.w1, 4 * d, L.b1, w.ff, 4 * d), w.hs, F.s1, st);
                launch_quant_rows_fp8(dt, w.ff, M, 4 * d, w.qkv, w.hs, st);
                tgemm_fp8(s, EPI_RESID, gemm_plain(w.qkv, M, 4 * d, F.w2, d, L.b2, w.x, d), w.hs, F.s2, st);
                continue;
            }
            const LayerMats Wm = layer_mats(c, s, false, l, st);
            launch_layernorm(dt, w.x, nullptr, M, d, L.ln1_w, L.ln1_b, w.hn, st);
            tgemm(s, KCLS, dt, EPI_STORE, gemm_plain(w.hn, M, d, Wm.wqkv, 3 * d, L.bqkv, w.qkv, 3 * d), st);
            {
                KT kt(s, K_ATTN_ENC, 4.0 * nb * H * (double)T * T * 64);
                launch_attn_encoder(dt, w.qkv, w.att, nb, T, d, H, st);
            }
            tgemm(s, KCLS, dt, EPI_RESID, gemm_plain(w.att, M, d, Wm.wo, d, L.bo, w.x, d), st);
            launch_layernorm(dt, w.x, nullptr, M, d, L.ln2_w, L.ln2_b, w.hn, st);
            tgemm(s, KCLS, dt, enc_gelu_epi(dt), gemm_plain(w.hn, M, d, Wm.w1, 4 * d, L.b1, w.ff, 4 * d), st);
            tgemm(s, KCLS, dt, EPI_RESID, gemm_plain(w.ff, M, 4 * d, Wm.w2, d, L.b2, w.x, d), st);
        }
        launch_layernorm(dt, w.x, nullptr, M, d, W.lnpost_w, W.lnpost_b, w.hn, st);
        if (s->direct) {
            // keep E per slot for the direct cross attention; the slot's cross K/V (if any) is stale
            for (int k = 0; k < nb; k++) {
                WM_CHECK(hipMemcpyAsync((char*)w.enc + (size_t)slots[b0 + k] * T * d * E, (const char*)w.hn + (size_t)k * T * d * E,
                                        (size_t)T * d * E, hipMemcpyDeviceToDevice, st));
                w.cross_fresh[slots[b0 + k]] = 0;
            }
        } else {
            // cross K/V of every decoder layer in one GEMM, scattered into each window's slot
            GemmArgs g = gemm_plain(w.hn, M, d, W.wkv_cross, 2 * hp.n_text_layer * d, W.bkv_cross, nullptr, 0);
            g.scale = c->k_scale;
            g.cache = w.cross; g.row_slot = d_slot; g.L = hp.n_text_layer; g.H = hp.n_text_head; g.ctx = hp.n_audio_ctx; g.d = d;
            g.rpw = T;
            tgemm(s, KCLS, dt, EPI_CROSSKV, g, st);
            for (int k = 0; k < nb; k++) w.cross_fresh[slots[b0 + k]] = 1;
        }
        WM_CHECK(hipStreamSynchronize(st));  // h_ints reused by the next micro-batch
    }
    s->last_enc_windows = n_win;
    return 0;
}

// ---- decoder --------------------------------------------------------------------------------------
// n_tok tokens (ragged over slots) -> logits of n_rows rows (row r = token lrows[r]) into w.logits.
// token metadata (already in w.h_ints: [tok | pos | slot | - | -] with stride cap_tok, lrows at 5*cap_tok) -> device
static void decoder_upload(Context* c, whisper_state* s, int n_tok, int n_rows, bool tiles) {
    const Hparams& hp = c->hp;
    Workspace& w = s->ws;
    int* hi = w.h_ints;
    const int ct = w.cap_tok;
    double self_kv = 0;
    for (int i = 0; i < n_tok; i++) {
        hi[3 * ct + i] = hi[ct + i] + 1;
        hi[4 * ct + i] = enc_ctx(c, s);  // cross keys of the call; rows past them in a slot's planes are an earlier call's
        self_kv += hi[ct + i] + 1;
    }
    s->cur_self_work = self_kv * hp.n_text_head * 64 * 2 * 2;
    WM_CHECK(hipMemcpyAsync(w.tok, hi, ((size_t)5 * ct + n_rows) * sizeof(int), hipMemcpyHostToDevice, s->stream));
    if (!tiles) return;
    // prefill attention tiles: runs of <= 64 consecutive tokens of one slot with increasing positions
    int nt = 0;
    for (int i = 0; i < n_tok; i++) {
        const bool cont = i > 0 && hi[2 * ct + i] == hi[2 * ct + i - 1] && hi[ct + i] > hi[ct + i - 1] &&
                          w.h_qtiles[nt - 1].y < 64;
        if (cont) w.h_qtiles[nt - 1].y++;
        else w.h_qtiles[nt++] = make_int2(i, 1);
    }
    w.n_qtiles = nt;
    WM_CHECK(hipMemcpyAsync(w.qtiles, w.h_qtiles, (size_t)nt * sizeof(int2), hipMemcpyHostToDevice, s->stream));
}

// One group of decoder rows on one stream: rows [r0, r0+n) of the token arrays and activations,
// with its own split-K slab region and cross-attention partials, so that two groups can run at the
// same time (decode steps).
struct DecView {
    int r0, n;
    hipStream_t st;
    float* splitk;
    long splitk_elems;
    float *xo, *xml;
};

// The small-M decode path (decoder_rows_small): every projection one launch (no split-K slabs, no
// reduce launch), LayerNorm in the GEMM prologue. Default for decode steps of <= 4 clips: at one clip
// base f16 471-481 -> 539-540 audio-s/s, large-v3 f16 78 -> 80 (profiles/r03_smallm_b1_ab.txt); at 16
// clips it measured slower (large-v3 bf16: 101 vs 94 us per decoder layer, r03_prof16_smallm{0,1}.md:
// its 80 workgroups of 16 columns pull the weights more slowly than split-K's 200-240, and the
// LayerNorm recomputed by every workgroup costs ~4.7 us per LN-consuming GEMM at 16 rows).
// WHISPER_MI355X_SMALLM=0 off, =1 up to 32 clips, =k up to k clips (read per call). Block-quantized
// files use it up to quant_small_max() clips whatever this says.
static int small_m_max() {
    const char* e = getenv("WHISPER_MI355X_SMALLM");
    if (!e) return 4;
    const int v = atoi(e);
    return v == 1 ? 32 : std::max(0, std::min(32, v));
}

// Decode steps of block-quantized files: up to this many clips the small-M path reads the blocks
// in its GEMMs; above it (its 32-row chunks each re-read the blocks: large-v3-q5_0 at 128 clips decoded
// in 2534 ms per step against 857 for f16) the layer's blocks are dequantized once per step into the
// scratch (one launch) and the split-K path runs as for f16 / bf16 weights. WHISPER_MI355X_QSMALL_MAX.
static int quant_small_max() {
    const char* e = getenv("WHISPER_MI355X_QSMALL_MAX");  // read per call (tests switch it)
    return e ? atoi(e) : 32;
}

// The persistent decode step (kernels/pdec.hip) for decode steps of up to this many clips in the cache
// form: WHISPER_MI355X_PDEC (default 4 = kPdecMaxRows; 0 = off; read per call).
static int pdec_max() {
    const char* e = getenv("WHISPER_MI355X_PDEC");
    return e ? std::max(0, std::min(kPdecMaxRows, atoi(e))) : kPdecMaxRows;
}

// Rows up to which a decode step's row group takes the small-M path, by the two switches above
static int small_rows_max(Context* c) { return c->quant ? std::max(quant_small_max(), small_m_max()) : small_m_max(); }

// fp8 mode: decode steps read the e4m3 copies of the decoder's projection weights (split-K path only)
static bool dec_fp8(Context* c) { return c->fp8_enc && !c->dec8.empty(); }

// The per-call switches that choose a decode step's kernels, folded into the key of its captured graph.
static int dec_path_sig() {
    return small_m_max() | (std::min(std::max(quant_small_max(), 0), 1023) << 6) |
           (std::min(std::max(attn_cross_wide_max(), 0), 1023) << 16) | (pdec_max() << 26) | ((g_pdec_blocks & 1) << 29);
}

// Quantized files: the persistent step reads the context's expanded compute-type copy when it exists
// (measured faster: the one-wave-per-SIMD kernel pays for the in-register dequantization; large-v3
// q5_0, 1 clip: 2.79 ms per step streaming blocks, 1.52 reading the copy); whisper_mi355x_set_pdec_blocks(1)
// makes it stream the GGML blocks (0.69 bytes per q5_0 weight) instead.
static bool pdec_blocks(Context* c) {
    return c->quant && (g_pdec_blocks || !c->expanded.load(std::memory_order_acquire));
}

// A decode step of n clips runs as one persistent launch when the model shape has a kernel, the
// weights are f16 / bf16 or GGML blocks (not the fp8 decoder copies), the device has the 256 CUs the
// grid is built for, and the step is in the cross K/V cache form.
static bool pdec_use(Context* c, whisper_state* s, int n, bool xdirect) {
    if (xdirect || s->pdec_off || s->mode.split_slots || n < 1 || n > pdec_max()) return false;
    if (dec_fp8(c)) return false;
    // one weight form for every decoder matrix (the kernel is built per form)
    const bool quant = c->w.dec[0].qqkv.type != 0;
    for (const LayerW& L : c->w.dec)
        for (const QMat* q : {&L.qqkv, &L.qo, &L.qxq, &L.qxo, &L.q1, &L.q2})
            if ((q->type != 0) != quant) return false;
    const bool blocks = pdec_blocks(c);
    if (blocks && c->dt != DType::F16) return false;
    if (!pdec_supported(c->hp.n_text_state, c->hp.n_text_head, blocks)) return false;
    static const int cus = [] {
        int dev = 0, v = 0;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
        return v;
    }();
    return cus == 256;
}

// Row groups of a decode step. The split-K pass (every LayerNorm folded into a split-K reduce) takes at
// most 128 rows, so a step over n > 128 clips runs as ceil(n / 128) groups of near-equal size,
// alternating between the state's two streams (forked from and joined back into the state's stream:
// branches of the step's hipGraph); two groups for 129..256 clips measured the same as the unfused
// path in bf16 (turbo at 256 clips: decode 213 vs 217 ms per step) and the fp8 decoder weights exist
// only on the split-K path.
// Splitting steps of 32..128 clips into two concurrent groups measured slower on large-v3 at 128 clips
// (2360-2392 vs 2729-2740 audio-s/s: the cross-attention pass at 64 clips per group reads E at 3.6
// instead of 4.7 TB/s), and so did two separate graphs on two streams (942 vs 843 ms of decode per
// step, profiles/r02_dec_groups_ab.txt); both were removed.
static int dec_groups(int n_tok) { return cdiv(n_tok, 128); }

// How a decode step of n clips (one token per clip, logits of every row) runs, decided here and nowhere
// else: decoder_launch and the row functions take the plan and follow it, dec_graph keys the step's graph
// on its path. A row group runs as the persistent launch (decoder_rows_pdec; <= 4 clips, so one group),
// the small-M GEMMs (decoder_rows_small) or the split-K pass (decoder_rows_step); the small-M condition is
// evaluated on a group's rows, so the last, shorter group of a step may take another path than the others.
enum StepPath { STEP_PDEC, STEP_SMALL, STEP_SPLITK };
struct StepPlan {
    int n;               // clips (rows) of the step
    int groups, gsz;     // row groups and the rows of each but the last (n - (groups - 1) * gsz rows)
    StepPath path, tail_path;  // of a group of gsz rows, of the last group
    bool xdirect;        // cross attention from the encoder output (else from the cross K/V cache)
    bool w8;             // the split-K pass reads the fp8 weights
    bool pdec_ok;        // false: a re-run of a step whose persistent launch gave up
    bool pipe;           // built into a pipelined step graph (its advance kernel copies the error word)
};
static StepPlan step_plan(Context* c, whisper_state* s, int n, bool xdirect, bool pdec_ok = true) {
    StepPlan P{};
    P.n = n; P.groups = dec_groups(n); P.gsz = cdiv(n, P.groups);
    P.xdirect = xdirect; P.w8 = dec_fp8(c); P.pdec_ok = pdec_ok;
    const int d = c->hp.n_text_state;
    const bool pd = pdec_ok && pdec_use(c, s, n, xdirect);
    auto path = [&](int rows) {
        if (pd) return STEP_PDEC;
        // (beam search with several beams per clip, split_slots: the split-K chain at every row count, so that a
        // beam's bits do not change when other beams complete and the step's rows drop to the small-M range)
        const bool small = !P.w8 && !s->mode.split_slots && rows <= small_rows_max(c) && gemm_small_ok(rows, d, true) &&
                           gemm_small_ok(rows, 4 * d, false);
        return small ? STEP_SMALL : STEP_SPLITK;
    };
    P.path = path(P.gsz);
    P.tail_path = P.groups == 1 ? P.path : path(n - (P.groups - 1) * P.gsz);
    return P;
}

// Device array of the decoder layers' pointers (once per context and weight form): the arena's
// matrices, the GGML blocks of a quantized file, or that file's expanded compute-type copy
static const PdecLayer* pdec_layers(Context* c, bool blocks) {
    std::lock_guard<std::mutex> lk(c->pdec_mu);
    void*& slot = blocks || !c->quant ? c->pdec_layers : c->pdec_layers_exp;
    if (!slot) {
        std::vector<PdecLayer> h(c->hp.n_text_layer);
        for (int l = 0; l < c->hp.n_text_layer; l++) {
            const LayerW& L = c->w.dec[l];
            LayerMats m{L.wqkv, L.wo, L.wxq, L.wxo, L.w1, L.w2};
            if (c->quant && !blocks) m = c->exp_dec[l];
            auto mat = [&](const void* w, const QMat& q) {
                return q.type && blocks ? PdecMat{q.qs, q.qh, q.dm, q.type} : PdecMat{w, nullptr, nullptr, 0};
            };
            h[l] = PdecLayer{mat(m.wqkv, L.qqkv), mat(m.wo, L.qo), mat(m.wxq, L.qxq), mat(m.wxo, L.qxo), mat(m.w1, L.q1),
                             mat(m.w2, L.q2), L.bqkv, L.bo, L.bxq, L.bxo, L.b1, L.b2,
                             L.ln1_w, L.ln1_b, L.lnx_w, L.lnx_b, L.ln2_w, L.ln2_b};
        }
        void* p = nullptr;
        WM_CHECK(hipMalloc(&p, h.size() * sizeof(PdecLayer)));
        WM_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(PdecLayer), hipMemcpyHostToDevice));
        slot = p;
    }
    return (const PdecLayer*)slot;
}

// Everything a persistent step allocates, before a decode step is captured (no hipMalloc in a capture)
static void pdec_prepare(Context* c, whisper_state* s) {
    Workspace& w = s->ws;
    pdec_layers(c, pdec_blocks(c));
    if (w.pd_sync) return;
    // the hand-off block
    dalloc(w.pd_sync, pdec_granules(c->hp.n_text_state, c->hp.n_text_layer, c->hp.n_text_head).bytes);
    WM_CHECK(hipHostMalloc((void**)&w.h_pd_err, 16, 0));
    *w.h_pd_err = 0;
}

// One decode step of the view's rows as the persistent launch + the logits GEMM (graph-capturable).
// The launch's error word is copied to the host (a node of the step's graph): decode_step checks it
// after the step's synchronisation and re-runs the step on the per-kernel path if the launch gave up.
static void decoder_rows_pdec(Context* c, whisper_state* s, const DecView& v, bool pipe) {
    const Hparams& hp = c->hp;
    Workspace& w = s->ws;
    const int d = hp.n_text_state, H = hp.n_text_head, L = hp.n_text_layer, V = hp.n_vocab;
    const int n = v.n;
    hipStream_t st = v.st;
    if (!w.pd_sync) WM_FAIL("pdec: buffers not allocated (pdec_prepare)");
    const bool blocks = pdec_blocks(c);
    PdecArgs a{};
    a.layers = pdec_layers(c, blocks);
    a.L = L; a.M = n; a.d = d; a.n_text_ctx = hp.n_text_ctx; a.n_audio_ctx = hp.n_audio_ctx;
    a.n_audio_len = enc_ctx(c, s);
    a.tok_emb = c->w.tok_emb_f32 ? (const void*)c->w.tok_emb_f32 : c->w.tok_emb;
    a.te_f32 = c->w.tok_emb_f32 != nullptr;
    a.pos_d = c->w.pos_d;
    a.lnd_w = c->w.lnd_w; a.lnd_b = c->w.lnd_b;
    a.tok = w.tok + v.r0; a.pos = w.pos + v.r0; a.slot = w.slot + v.r0;
    a.self_cache = w.self; a.cross_cache = w.cross;
    a.k_scale = c->k_scale;
    a.quant = blocks;
    a.s_cross = pdec_cross_splits(H, a.n_audio_len);
    a.sync = w.pd_sync;
    a.gr = pdec_granules(d, L, H);
    a.out_dh = (char*)w.dh + (size_t)v.r0 * d * esize(c->dt);
    a.gelu_tab = gelu_table_device();
    a.spin_ticks = g_pdec_spin_ticks;
    a.stamps = g_pdec_stamps;
    {
        // weights once + cross K/V + self K/V of every row, per launch
        const double bytes = 14.0 * d * d * 2 * L + (double)n * L * 2 * a.n_audio_len * d * 2 + s->cur_self_work;
        KT kt(s, K_PDEC, bytes, st);
        launch_pdec(c->dt, a, st);
    }
    // (a pipelined step graph's advance kernel writes the error word to its ring slot instead)
    if (!pipe)
        WM_CHECK(hipMemcpyAsync(w.h_pd_err, (const char*)w.pd_sync + a.gr.err_bytes, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    GemmArgs g = gemm_plain(a.out_dh, n, d, c->w.tok_emb, V, nullptr, w.logits + (size_t)v.r0 * V, V);
    tgemm_ws(s, K_GEMM_DEC, c->dt, EPI_F32, g, st, v.splitk, v.splitk_elems);
}

// The view's rows of the token arrays and activations (what the three layer-by-layer passes below work on)
struct DecRows {
    int n;
    hipStream_t st;
    int *tok, *pos, *slot, *nkv_self, *nkv_cross;
    int* sslot;  // the rows' self-cache slots: `slot`, or the hypotheses' own slots (StepMode::split_slots)
    float* dx;
    void *dh, *dq, *datt, *dff, *qx;
};
static DecRows dec_rows(Context* c, whisper_state* s, const DecView& v) {
    Workspace& w = s->ws;
    const size_t d = c->hp.n_text_state, H = c->hp.n_text_head, E = esize(c->dt), r0 = v.r0;
    return DecRows{v.n, v.st, w.tok + r0, w.pos + r0, w.slot + r0, w.nkv_self + r0, w.nkv_cross + r0,
                   (s->mode.split_slots ? w.sslot : w.slot) + r0, w.dx + r0 * d,
                   (char*)w.dh + r0 * d * E, (char*)w.dq + r0 * d * E, (char*)w.datt + r0 * d * E, (char*)w.dff + r0 * 4 * d * E,
                   w.qx ? (void*)((char*)w.qx + r0 * 2 * H * d * E) : nullptr};
}

// Token + positional embedding of the rows into dx; `ln`: and layer 0's first LayerNorm of it into dh (one launch)
static void embed_rows(Context* c, const DecRows& r, bool ln) {
    const Weights& W = c->w;
    const int d = c->hp.n_text_state;
    const void* te = W.tok_emb_f32 ? (const void*)W.tok_emb_f32 : W.tok_emb;
    if (ln) launch_embed_ln(c->dt, te, W.tok_emb_f32 != nullptr, W.pos_d, r.tok, r.pos, r.n, d, r.dx, W.dec[0].ln1_w, W.dec[0].ln1_b, r.dh, r.st);
    else launch_embed(c->dt, te, W.tok_emb_f32 != nullptr, W.pos_d, r.tok, r.pos, r.n, d, r.dx, r.st);
}

// Layer l's cross attention from the encoder output (kernels/xattn.hip), after the caller's cross-Q GEMM
// left q in dq: Q' = s Wk^T q (hi/lo) -> one pass over E per clip -> split merge + Wv into datt. (Fusing
// the cross-Q reduce into the Q' projection was bit-identical but slower, 855 vs 848 ms per step at 128
// clips: removed.) step_cls: the timing class of the pass over E; the roofline's K_ATTN_CROSS holds decode
// steps only (E bytes read once per clip and layer), prefill counts it as K_OTHER.
static void xattn_tail(Context* c, whisper_state* s, const DecView& v, const DecRows& r, int l, int step_cls, bool kt_layer) {
    const Weights& W = c->w;
    const DType dt = c->dt;
    const int d = c->hp.n_text_state, H = c->hp.n_text_head, Ta = enc_ctx(c, s), n = r.n;  // (E is packed: Ta rows per slot)
    const int S = xattn_splits(n, Ta);
    hipStream_t st = r.st;
    {
        KT kt(s, K_GEMM_DEC, 2.0 * d * d + 2.0 * n * d + 4.0 * n * H * d, st);
        launch_xattn_qproj(dt, r.dq, (const char*)W.wkT + (size_t)l * H * d * 64 * 2, n, d, H, c->k_scale, r.qx, st);
    }
    {
        KT kt(s, step_cls, (double)n * Ta * d * 2, st, kt_layer);
        launch_xattn_step(dt, s->ws.enc, r.slot, r.qx, n, Ta, d, S, kXattnThr, v.xo, v.xml, st);
    }
    {
        KT kt(s, K_GEMM_DEC, 2.0 * d * d + 4.0 * n * S * d + 2.0 * n * d, st);
        launch_xattn_combine(dt, v.xo, v.xml, S, (const char*)W.wkv_cross + (size_t)(2 * l + 1) * d * d * 2,
                             W.bkv_cross + (size_t)(2 * l + 1) * d, n, d, H, r.datt, st);
    }
}

// kernel timing (bench roofline): bits 16..23 of the mask = time the per-layer attention launches of
// every k-th layer only (fewer event nodes in the timed decode graphs; every layer does the same work)
static int kt_layer_stride(const whisper_state* s) { return std::max(1, (s->ktime_mask >> 16) & 0xFF); }

// Decode step over <= 32 rows (the app's one clip per call, whisper.rs:83-85 / state.rs:147; one
// rank's 16-clip shard of configs[3] at 8 GPUs), kernels only: every projection is ONE launch of
// gemm_small_kernel (no split-K slabs, no reduce launch), and the LayerNorm in front of the QKV,
// cross-Q and FC1 projections runs in that GEMM's prologue from the f32 residual stream. Per layer:
// QKV (raw f32 sums) -> self attention (bias, scale, cache append, attention) -> Wo (+x) -> cross-Q
// -> cross attention -> Wxo (+x) -> FC1 (GELU) -> FC2 (+x): 8 launches in the cache form, against
// 15 on the split-K path. Results per row do not depend on the other rows (batch == single within
// this path); they differ in the last bits from the split-K path's (another summation order).
static void decoder_rows_small(Context* c, whisper_state* s, const DecView& v, bool xdirect, double self_share) {
    const Hparams& hp = c->hp;
    Workspace& w = s->ws;
    const int d = hp.n_text_state, H = hp.n_text_head, V = hp.n_vocab, L = hp.n_text_layer;
    const DType dt = c->dt;
    const Weights& W = c->w;
    hipStream_t st = v.st;
    const int n = v.n;
    const DecRows r = dec_rows(c, s, v);
    const int kt_stride = kt_layer_stride(s);
    float* raw = v.splitk;  // f32 projection sums handed to the attention prologues ([n][3d] / [n][d])
    const double kvrow = (double)H * 64 * 2 * 2;
    // q: the matrix's GGML blocks (quantized files; type 0: none, the dense Wt is read)
    auto small = [&](const QMat& q, int epi, const void* A, int K, const void* Wt, int N, const float* bias, void* out,
                     long ldo, const float* lnw = nullptr, const float* lnb = nullptr) {
        GemmArgs g = gemm_plain(A, n, K, Wt, N, bias, out, ldo);
        g.a_ln_w = lnw;
        g.a_ln_b = lnb;
        g.q = q;
        KT kt(s, K_GEMM_DEC, 2.0 * N * K + 2.0 * n * K + 4.0 * n * N, st);
        launch_gemm_small(dt, epi, g, lnw != nullptr, st);
    };
    embed_rows(c, r, false);
    for (int l = 0; l < L; l++) {
        const LayerW& Lw = W.dec[l];
        const bool kt_layer = l % kt_stride == 0;
        // self attention: LN1 in the QKV GEMM, raw sums to the attention prologue (+ bias, q/k scale)
        small(Lw.qqkv, EPI_F32, r.dx, d, Lw.wqkv, 3 * d, nullptr, raw, 3 * d, Lw.ln1_w, Lw.ln1_b);
        {
            const DecSlabs sl{raw, 1, (long)n * 3 * d, 3 * d, Lw.bqkv, c->k_scale};
            KT kt(s, K_ATTN_SELF, self_share, st, kt_layer);
            launch_attn_self_step(dt, sl, w.self, r.sslot, r.pos, n, L, l, H, hp.n_text_ctx, d, r.datt, st);
        }
        small(Lw.qo, EPI_RESID, r.datt, d, Lw.wo, d, Lw.bo, r.dx, d);
        if (xdirect) {
            GemmArgs g = gemm_plain(r.dx, n, d, Lw.wxq, d, Lw.bxq, r.dq, d);
            g.scale = c->k_scale; g.sc_div = d; g.sc_mod = 1; g.sc_lim = 1;
            g.a_ln_w = Lw.lnx_w; g.a_ln_b = Lw.lnx_b;
            g.q = Lw.qxq;
            {
                KT kt(s, K_GEMM_DEC, 2.0 * d * d + 2.0 * n * d + 4.0 * n * d, st);
                launch_gemm_small(dt, EPI_STORE, g, true, st);
            }
            xattn_tail(c, s, v, r, l, K_ATTN_CROSS, kt_layer);
        } else {
            small(Lw.qxq, EPI_F32, r.dx, d, Lw.wxq, d, nullptr, raw, d, Lw.lnx_w, Lw.lnx_b);
            const DecSlabs sl{raw, 1, (long)n * d, d, Lw.bxq, c->k_scale};
            KT kt(s, K_ATTN_CROSS, (double)n * enc_ctx(c, s) * kvrow, st, kt_layer);
            launch_attn_cross_step(dt, sl, w.cross, r.slot, r.nkv_cross, n, L, l, H, hp.n_audio_ctx, d, r.datt, st);
        }
        small(Lw.qxo, EPI_RESID, r.datt, d, Lw.wxo, d, Lw.bxo, r.dx, d);
        small(Lw.q1, EPI_GELU, r.dx, d, Lw.w1, 4 * d, Lw.b1, r.dff, 4 * d, Lw.ln2_w, Lw.ln2_b);
        small(Lw.q2, EPI_RESID, r.dff, 4 * d, Lw.w2, d, Lw.b2, r.dx, d);
    }
    launch_layernorm(dt, r.dx, nullptr, n, d, W.lnd_w, W.lnd_b, r.dh, st);
    GemmArgs g = gemm_plain(r.dh, n, d, W.tok_emb, V, nullptr, w.logits + (size_t)v.r0 * V, V);
    tgemm_ws(s, K_GEMM_DEC, dt, EPI_F32, g, st, v.splitk, v.splitk_elems);
}

// The dense weights of decoder layer l for the two split-K / unfused passes below; a block-quantized file's
// blocks are dequantized into the scratch first (one launch)
static LayerW layer_dense(Context* c, whisper_state* s, int l, hipStream_t st) {
    LayerW Lw = c->w.dec[l];
    if (c->quant) {
        const LayerMats m = layer_mats(c, s, true, l, st);
        Lw.wqkv = (void*)m.wqkv; Lw.wo = (void*)m.wo; Lw.wxq = (void*)m.wxq; Lw.wxo = (void*)m.wxo;
        Lw.w1 = (void*)m.w1; Lw.w2 = (void*)m.w2;
    }
    return Lw;
}

// One decode step of the view's rows on the split-K path (one token per clip, logits of every row, <= 128
// rows per view); kernels only (graph-capturable). Every LayerNorm is folded into the embedding or into the
// split-K reduce of the preceding residual GEMM, and the QKV (and, cache form, cross-Q) projections leave
// split-K partial sums that the attention kernels reduce in their prologue (no separate reduce launch).
// P.w8 (fp8 mode): the projections read the e4m3 copies of the layer's weights.
static void decoder_rows_step(Context* c, whisper_state* s, const DecView& v, const StepPlan& P, double self_share) {
    const Hparams& hp = c->hp;
    Workspace& w = s->ws;
    const int d = hp.n_text_state, H = hp.n_text_head, V = hp.n_vocab, L = hp.n_text_layer;
    const DType dt = c->dt;
    const Weights& W = c->w;
    hipStream_t st = v.st;
    const int n = v.n;
    const DecRows r = dec_rows(c, s, v);
    const int KCLS = K_GEMM_DEC;
    const double kvrow = (double)H * 64 * 2 * 2;  // K and V row bytes of one position, all heads
    const int kt_stride = kt_layer_stride(s);
    auto gemm = [&](int epi, const GemmArgs& g) { tgemm_ws(s, KCLS, dt, epi, g, st, v.splitk, v.splitk_elems); };
    auto use8 = [&](GemmArgs g, void* q8, float* sc) {
        if (P.w8) { g.B = q8; g.w8_scale = sc; }
        return g;
    };
    // x += A W + bias; its reduce also writes LayerNorm(x; lnw, lnb) into dh
    auto resid = [&](const void* A, int K, const void* Wt, const float* bias, const float* lnw, const float* lnb, void* q8,
                     float* sc) {
        GemmArgs g = use8(gemm_plain(A, n, K, Wt, d, bias, r.dx, d), q8, sc);
        g.ln_w = lnw; g.ln_b = lnb; g.ln_out = r.dh;
        gemm(EPI_RESID, g);
    };
    auto partials = [&](const void* A, const void* Wt, int N, const float* bias, float scale, void* q8,
                        float* sc) -> DecSlabs {
        GemmArgs g = use8(gemm_plain(A, n, d, Wt, N, bias, nullptr, N), q8, sc);
        g.splitk_ws = v.splitk;
        g.splitk_ws_elems = v.splitk_elems;
        g.slab_wt = 1;
        KT kt(s, KCLS, 2.0 * g.N * g.K + 2.0 * g.M * g.K + 4.0 * g.M * g.N, st);
        const int splits = launch_gemm_partials(dt, g, st);
        if (splits <= 0 || splits > 16) WM_FAIL("decode partials GEMM not applicable (splits %d)", splits);
        return DecSlabs{v.splitk, splits, (long)n * N, N, bias, scale};
    };
    embed_rows(c, r, true);
    for (int l = 0; l < L; l++) {
        const LayerW Lw = layer_dense(c, s, l, st);
        static const Context::Fp8Dec no8{};
        const Context::Fp8Dec& F = P.w8 ? c->dec8[l] : no8;
        const bool kt_layer = l % kt_stride == 0;
        {
            const DecSlabs sl = partials(r.dh, Lw.wqkv, 3 * d, Lw.bqkv, c->k_scale, F.wqkv, F.sqkv);
            KT kt(s, K_ATTN_SELF, self_share, st, kt_layer);
            launch_attn_self_step(dt, sl, w.self, r.sslot, r.pos, n, L, l, H, hp.n_text_ctx, d, r.datt, st);
        }
        resid(r.datt, d, Lw.wo, Lw.bo, Lw.lnx_w, Lw.lnx_b, F.wo, F.so);
        if (P.xdirect) {
            GemmArgs g = use8(gemm_plain(r.dh, n, d, Lw.wxq, d, Lw.bxq, r.dq, d), F.wxq, F.sxq);
            g.scale = c->k_scale; g.sc_div = d; g.sc_mod = 1; g.sc_lim = 1;
            gemm(EPI_STORE, g);
            xattn_tail(c, s, v, r, l, K_ATTN_CROSS, kt_layer);
        } else {
            const DecSlabs sl = partials(r.dh, Lw.wxq, d, Lw.bxq, c->k_scale, F.wxq, F.sxq);
            KT kt(s, K_ATTN_CROSS, (double)n * enc_ctx(c, s) * kvrow, st, kt_layer);
            launch_attn_cross_step(dt, sl, w.cross, r.slot, r.nkv_cross, n, L, l, H, hp.n_audio_ctx, d, r.datt, st);
        }
        resid(r.datt, d, Lw.wxo, Lw.bxo, Lw.ln2_w, Lw.ln2_b, F.wxo, F.sxo);
        gemm(EPI_GELU, use8(gemm_plain(r.dh, n, d, Lw.w1, 4 * d, Lw.b1, r.dff, 4 * d), F.w1, F.s1));
        if (l + 1 < L) resid(r.dff, 4 * d, Lw.w2, Lw.b2, W.dec[l + 1].ln1_w, W.dec[l + 1].ln1_b, F.w2, F.s2);
        else resid(r.dff, 4 * d, Lw.w2, Lw.b2, W.lnd_w, W.lnd_b, F.w2, F.s2);  // dh = final LN of every row
    }
    gemm(EPI_F32, gemm_plain(r.dh, n, d, W.tok_emb, V, nullptr, w.logits + (size_t)v.r0 * V, V));
}

// The unfused decoder forward over the view's tokens (prefill, language detection, whisper_decode: one view
// at r0 = 0, over the attention tiles that decoder_upload built) + logits of n_rows rows (row r = token
// lrows[r]); kernels only.
// `al` (the token-timestamp alignment, align_windows; cache form): after the cross-Q GEMM of a layer that has
// alignment heads the score kernel runs on those rows, and the pass ends after the cross-Q of the highest
// such layer (the remaining layers, the final LN and the logits GEMM are not needed).
struct AlignPass {
    const AlignClip* clips;
    int n_clips, max_rows;
    long total_rows;
    float* P;
};
static void decoder_rows_prefill(Context* c, whisper_state* s, const DecView& v, int n_rows, bool xdirect,
                                 const AlignPass* al = nullptr) {
    const Hparams& hp = c->hp;
    Workspace& w = s->ws;
    const int d = hp.n_text_state, H = hp.n_text_head, V = hp.n_vocab, L = hp.n_text_layer;
    const DType dt = c->dt;
    const Weights& W = c->w;
    hipStream_t st = v.st;
    const int n = v.n;
    const DecRows r = dec_rows(c, s, v);
    const int KCLS = K_GEMM_DEC;
    const double kvrow = (double)H * 64 * 2 * 2;  // K and V row bytes of one position, all heads
    const int kt_stride = kt_layer_stride(s);
    auto gemm = [&](int epi, const GemmArgs& g) { tgemm_ws(s, KCLS, dt, epi, g, st, v.splitk, v.splitk_elems); };
    // x += A W + bias; then LayerNorm(x; lnw, lnb) into dh (lnw null: none)
    auto resid = [&](const void* A, int K, const void* Wt, const float* bias, const float* lnw, const float* lnb) {
        gemm(EPI_RESID, gemm_plain(A, n, K, Wt, d, bias, r.dx, d));
        if (lnw) launch_layernorm(dt, r.dx, nullptr, n, d, lnw, lnb, r.dh, st);
    };
    embed_rows(c, r, false);
    launch_layernorm(dt, r.dx, nullptr, n, d, W.dec[0].ln1_w, W.dec[0].ln1_b, r.dh, st);
    for (int l = 0; l < L; l++) {
        const LayerW Lw = layer_dense(c, s, l, st);
        const bool kt_layer = l % kt_stride == 0;
        {
            GemmArgs g = gemm_plain(r.dh, n, d, Lw.wqkv, 3 * d, Lw.bqkv, r.dq, d);
            g.scale = c->k_scale;
            g.cache = w.self; g.row_slot = r.slot; g.row_pos = r.pos; g.L = L; g.layer = l; g.H = H;
            g.ctx = hp.n_text_ctx; g.d = d;
            gemm(EPI_QKV_DEC, g);
            KT kt(s, K_ATTN_SELF, 1.0, st, kt_layer);
            launch_attn_prefill(dt, r.dq, d, w.self, r.slot, r.nkv_self, w.qtiles, w.n_qtiles, L, l, H, hp.n_text_ctx, d, r.datt, st);
        }
        resid(r.datt, d, Lw.wo, Lw.bo, Lw.lnx_w, Lw.lnx_b);
        GemmArgs gq = gemm_plain(r.dh, n, d, Lw.wxq, d, Lw.bxq, r.dq, d);
        gq.scale = c->k_scale; gq.sc_div = d; gq.sc_mod = 1; gq.sc_lim = 1;
        gemm(EPI_STORE, gq);
        if (xdirect) {
            xattn_tail(c, s, v, r, l, K_OTHER, kt_layer);
        } else {
            if (al) {
                const int k0 = c->dtw_layer_first[l], k1 = c->dtw_layer_first[l + 1];
                if (k1 > k0) {
                    KT kt(s, K_ALIGN_SCORES, 2.0 * al->total_rows * enc_ctx(c, s) * 64 * (k1 - k0), st);
                    launch_align_scores(dt, r.dq, d, w.cross, al->clips, al->n_clips, al->max_rows, L, l, H, hp.n_audio_ctx,
                                        enc_ctx(c, s), (const int2*)c->dtw_heads_dev + k0, k1 - k0, al->P, st);
                }
                if (l == c->dtw_last_layer) return;
            }
            KT kt(s, K_OTHER, (double)n * enc_ctx(c, s) * kvrow, st);
            launch_attn_prefill(dt, r.dq, d, w.cross, r.slot, r.nkv_cross, w.qtiles, w.n_qtiles, L, l, H, hp.n_audio_ctx, d, r.datt, st);
        }
        resid(r.datt, d, Lw.wxo, Lw.bxo, Lw.ln2_w, Lw.ln2_b);
        gemm(EPI_GELU, gemm_plain(r.dh, n, d, Lw.w1, 4 * d, Lw.b1, r.dff, 4 * d));
        if (l + 1 < L) resid(r.dff, 4 * d, Lw.w2, Lw.b2, W.dec[l + 1].ln1_w, W.dec[l + 1].ln1_b);
        else resid(r.dff, 4 * d, Lw.w2, Lw.b2, nullptr, nullptr);
    }
    launch_layernorm(dt, w.dx, w.lrows, n_rows, d, W.lnd_w, W.lnd_b, w.lrow, st);
    gemm(EPI_F32, gemm_plain(w.lrow, n_rows, d, W.tok_emb, V, nullptr, w.logits, V));
}

// The two stream halves of a decode step's scratch: group views on the state's stream use the first
// half of the split-K slabs and cross-attention partials, views on stream2 the second. A group of
// <= gmax rows uses at most gmax * xattn_splits(gmax) partial rows; the offset of the second half is the worst
// case over the audio contexts a call may ask for (xattn_splits grows with its key count: the model's n_audio_ctx).
static void dec_halves(Context* c, whisper_state* s, int gmax, bool xdirect, DecView& a, DecView& b) {
    Workspace& w = s->ws;
    const int H = c->hp.n_text_head, d = c->hp.n_text_state;
    const long half = w.splitk_elems / 2;
    long xoff = 0;
    if (xdirect)
        for (int n = 1; n <= gmax; n++) xoff = std::max(xoff, (long)n * xattn_splits(n, c->hp.n_audio_ctx));
    a = DecView{0, 0, s->stream, w.splitk, half, w.xo, w.xml};
    b = DecView{0, 0, s->stream2, w.splitk + half, half, w.xo ? w.xo + xoff * H * d : nullptr,
                w.xml ? w.xml + xoff * H * 2 : nullptr};
}

// One row group of a decode step on the plan's path for it; self_share: its share of the step's self-attention work
static void decoder_group(Context* c, whisper_state* s, const DecView& v, const StepPlan& P, double self_share) {
    switch (v.n == P.gsz ? P.path : P.tail_path) {
    case STEP_PDEC: decoder_rows_pdec(c, s, v, P.pipe); break;
    case STEP_SMALL: decoder_rows_small(c, s, v, P.xdirect, self_share); break;
    case STEP_SPLITK: decoder_rows_step(c, s, v, P, self_share); break;
    }
}

// The decode step the plan describes (token metadata already on the device); kernels only (graph-capturable)
static void decoder_launch(Context* c, whisper_state* s, const StepPlan& P) {
    Workspace& w = s->ws;
    const int n_tok = P.n, gsz = P.gsz;
    if (P.groups == 1) {
        decoder_group(c, s, DecView{0, n_tok, s->stream, w.splitk, w.splitk_elems, w.xo, w.xml}, P, 1.0);
        return;
    }
    DecView half[2];
    dec_halves(c, s, gsz, P.xdirect, half[0], half[1]);
    // block-quantized files before the expanded copy exists: one dequantization scratch per state, so
    // the groups run one after the other on the state's stream
    if (c->quant && !c->expanded.load(std::memory_order_acquire)) half[1] = half[0];
    WM_CHECK(hipEventRecord(s->ev_fork, s->stream));
    WM_CHECK(hipStreamWaitEvent(s->stream2, s->ev_fork, 0));
    for (int g = 0, r0 = 0; r0 < n_tok; g++, r0 += gsz) {
        DecView v = half[g & 1];
        v.r0 = r0;
        v.n = std::min(gsz, n_tok - r0);
        decoder_group(c, s, v, P, (double)v.n / n_tok);
    }
    WM_CHECK(hipEventRecord(s->ev_join, s->stream2));
    WM_CHECK(hipStreamWaitEvent(s->stream, s->ev_join, 0));
}


// Cross K/V of the given slots (all decoder layers, one GEMM per clip) into the cache, for slots
// whose cache is stale: direct mode computes it only for prompts too long for the direct prefill.
static void ensure_cross_cache(Context* c, whisper_state* s, const std::vector<int>& slots) {
    Workspace& w = s->ws;
    const Hparams& hp = c->hp;
    const int d = hp.n_audio_state, T = enc_ctx(c, s), L = hp.n_text_layer;  // (E: T rows per slot, packed)
    const size_t E = esize(c->dt);
    std::vector<int> stale;
    int need = 0;
    for (int sl : slots) need = std::max(need, sl + 1);
    ensure_cross(c, s, need);
    for (int sl : slots)
        if (!w.cross_fresh[sl]) stale.push_back(sl);
    std::sort(stale.begin(), stale.end());
    // one GEMM per run of consecutive slots (E is slot-major, so a run is one [k*T][d] matrix)
    for (size_t a = 0; a < stale.size();) {
        size_t b = a + 1;
        while (b < stale.size() && stale[b] == stale[b - 1] + 1) b++;
        const int sl = stale[a], k = (int)(b - a);
        GemmArgs g = gemm_plain((const char*)w.enc + (size_t)sl * T * d * E, k * T, d, c->w.wkv_cross, 2 * L * d,
                                c->w.bkv_cross, nullptr, 0);
        g.scale = c->k_scale;
        g.cache = w.cross; g.row_slot = w.kvslot + sl; g.L = L; g.H = hp.n_text_head; g.ctx = hp.n_audio_ctx; g.d = d;
        g.rpw = T;
        tgemm(s, K_GEMM_ENC, c->dt, EPI_CROSSKV, g, s->stream);
        for (size_t i = a; i < b; i++) w.cross_fresh[stale[i]] = 1;
        a = b;
    }
}

// Direct cross attention for this forward (tokens/slots already in w.h_ints)? Yes for one-token
// steps and short prompts; otherwise the clips involved get a cross K/V cache first.
static bool choose_xdirect(Context* c, whisper_state* s, int n_tok) {
    if (!s->direct) return false;
    Workspace& w = s->ws;
    const int* slot = w.h_ints + 2 * w.cap_tok;
    std::vector<int> cnt(w.cap_jobs, 0);
    int mx = 0;
    for (int i = 0; i < n_tok; i++) mx = std::max(mx, ++cnt[slot[i]]);
    if (n_tok <= w.cap_xq && mx <= kXDirectMaxTok) return true;
    std::vector<int> used;
    for (int k = 0; k < w.cap_jobs; k++) if (cnt[k]) used.push_back(k);
    ensure_cross_cache(c, s, used);
    return false;
}

// prefill / language detection / whisper_decode: the unfused pass over the tiles that decoder_upload builds
static void decoder_forward(Context* c, whisper_state* s, int n_tok, int n_rows) {
    Workspace& w = s->ws;
    const bool xdirect = choose_xdirect(c, s, n_tok);
    decoder_upload(c, s, n_tok, n_rows, true);
    decoder_rows_prefill(c, s, DecView{0, n_tok, s->stream, w.splitk, w.splitk_elems, w.xo, w.xml}, n_rows, xdirect);
}

int decode_tokens(Context* c, whisper_state* s, const int* tokens, const int* pos, const int* slots, int n_tok,
                  const int* logit_rows, int n_logit_rows) {
    Workspace& w = s->ws;
    if (n_tok > w.cap_tok) return -1;
    int* hi = w.h_ints;
    for (int i = 0; i < n_tok; i++) { hi[i] = tokens[i]; hi[w.cap_tok + i] = pos[i]; hi[2 * w.cap_tok + i] = slots[i]; }
    for (int r = 0; r < n_logit_rows; r++) hi[5 * w.cap_tok + r] = logit_rows[r];
    decoder_forward(c, s, n_tok, n_logit_rows);
    return 0;
}

// ---- scheduler ------------------------------------------------------------------------------------
// (PH_BEAM: the clip's t = 0 attempt decodes as beam_k hypotheses, beam_step; PH_SAMPLE: a t > 0 attempt decodes
// as best_of candidates drawn on the device, sample_step)
enum Phase { PH_ENCODE, PH_LANG, PH_PREFILL, PH_DECODE, PH_BEAM, PH_SAMPLE, PH_DONE };

// The decoder state of one hypothesis of an attempt: the clip's one greedy / host-sampled decoder (Job::seq), a beam, a
// best_of candidate. The per-token code (process_step, fill_ctl, score_seq) takes the clip and the sequence.
struct Seq {
    std::vector<TokenData> tokens;
    int result_len = 0;
    double sum_logprobs_all = 0, sum_logprobs = -INFINITY, avg_logprobs = -INFINITY, entropy = 0, score = -INFINITY;
    int seek_delta = 100 * WHISPER_CHUNK_SIZE;
    bool has_ts = false, failed = false, completed = false;
    int step = 0;  // index of the last token decoded (advanced by process_step)
    // the grammar state after `tokens` (a grammar call): set by process_step, which starts every attempt,
    // beam and candidate from the call's init state with its first token; copied with the sequence when a beam takes
    // its parent's state
    Grammar gram;
};

struct Job {
    int slot = 0;
    // the single API's job (job 0 of a call with Sched::single_api): the state's carried prompt and rng, the progress and
    // new-segment callbacks, -3 without audio. Every other job decodes as on a fresh state.
    bool single = false;
    int n_samples = 0, n_len = 0, n_len_org = 0;
    int seek = 0, seek_start = 0, seek_end = 0;
    bool lang_pending = false;
    int lang_id = 0;
    std::vector<int> prompt_init, prompt_past, prompt;
    int temp_idx = 0;
    Seq seq;  // the attempt's decoder; after a beam or best_of attempt: its winner (hyps_finish)
    float no_speech_prob = 0.0f;
    std::mt19937* rng = nullptr;
    std::mt19937 own_rng{0};
    Phase phase = PH_ENCODE;
    std::vector<Segment> result;
    int n_new_segments = 0;
    whisper_mi355x_window_decision dec{};                // the current window's fallback decisions
    std::vector<whisper_mi355x_window_decision> decisions;
    // token-timestamp alignment of the window that just finished (finish_window -> align_windows): its seek and
    // frame count before seek advanced, and its first new segment
    bool al_pending = false;
    int al_seek = 0, al_frames = 0;
    size_t al_seg0 = 0;
    // token times of the window that just finished (finish_window -> token_time_windows): its first new segment, and
    // the clip's state, which lives for this call
    bool tt_pending = false;
    size_t tt_seg0 = 0;
    TtState tt;
};

// A hypothesis of a beam attempt or a candidate of a sampled attempt (§12): a sequence, a decoder row
// per step while it is live, with its own self-cache slot.
struct Hyp : Seq {
    bool ended = false;  // process_step said stop (completed, failed, or the window's last step)
    int sslot = 0;
    bool live() const { return !ended && !failed && !completed; }
};
// the hypotheses of a clip in PH_BEAM or PH_SAMPLE (a clip is in one of them at a time)
struct Hyps {
    std::vector<Hyp> h;
    std::vector<std::vector<int>> held;  // beams only, per beam: the tokens (prompt included) whose K/V rows its self slot holds
    bool live() const {
        for (const Hyp& q : h)
            if (q.live()) return true;
        return false;
    }
};

struct Sched {
    int beam_k = 0;    // > 0: WHISPER_SAMPLING_BEAM_SEARCH with this many beams (t = 0 attempts)
    int sample_n = 1;  // > 1: sampled (t > 0) attempts decode this many candidates per clip on the device
    std::vector<Hyps> hyps;  // per clip (when either is on)
    Context* c;
    whisper_state* s;
    whisper_full_params p;
    FullOpts o;
    std::vector<float> temps;
    std::vector<Job> jobs;
    bool single_api;  // job 0 is the single API's job (Job::single); no other job is
    int n_max_steps;
    long decoded = 0;
    double t_mel = 0, t_enc = 0, t_prefill = 0, t_decode = 0, t_logits = 0, t_align = 0, t_tokts = 0, t_vad = 0;
    // whisper_full_params.vad (vad_filter): the filtered clips on the device, their lengths, and per job the piece table
    bool vad_on = false;
    std::vector<const float*> vad_pcm;
    std::vector<int> vad_n;
    std::vector<std::vector<VadPiece>> vad_maps;
    // from pass to pass of full_batch_one: the call detects every clip's language (pass_lang); apply_audio_ctx has run;
    // a callback asked to stop; per row of the last prefill / decode step, a host-sampled row's probs
    bool need_lang = false, ctx_applied = false, aborted = false;
    std::vector<std::vector<float>> probs_rows;
    // a grammar call: the init state every sequence starts from, and per staged row of the coming logits launch the
    // grammar state of its sequence (fill_ctl -> ctl_upload)
    Grammar gram0;
    std::vector<const Grammar*> gram_rows;
    // a call with a logits_filter_callback: per staged row of the coming logits launch its sequence, whose
    // tokens are the history the callback gets (fill_ctl -> filter_round_trip), and the scratch they are converted into;
    // filter_reuse: the coming launch reads the rows the last round trip left on the device (the prefill's top-k pass
    // over rows whose callbacks have just run)
    std::vector<const Seq*> filter_rows;
    std::vector<whisper_token_data> filter_tokens;
    bool filter_reuse = false;
    // filter_fetched: the staged rows' copy to the host is already behind a synchronise (run_step enqueues it with the
    // step's graph, so a step pays one synchronise before its callbacks, not two)
    bool filter_fetched = false;
};

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
struct ScopeTimer {  // ScopeTimer timed{S.t_x}: the wall time of the scope, added to one of Sched's t_* sums
    double& sum;
    const double t0 = now_ms();
    ~ScopeTimer() { sum += now_ms() - t0; }
};
// the caller's abort callback, asked where whisper_full asks it (true: stop)
static bool abort_asked(const Sched& S) { return S.p.abort_callback && S.p.abort_callback(S.p.abort_callback_user_data); }

static void score_seq(const whisper_full_params& p, Seq& q) {
    if (q.result_len == 0) return;
    double result = 0.0;
    for (int i = 0; i < q.result_len; ++i) result += q.tokens[i].plog;
    q.sum_logprobs = result;
    q.avg_logprobs = result / q.result_len;
    double penalty = q.result_len;
    if (p.length_penalty > 0.0f) penalty = pow((5.0 + penalty) / 6.0, p.length_penalty);
    q.score = result / penalty;
    std::map<int, int> counts;
    int cnt = 0;
    for (int i = std::max(0, q.result_len - 32); i < q.result_len; ++i) { counts[q.tokens[i].id]++; cnt++; }
    double entropy = 0.0;
    for (auto& kv : counts) { const double f = kv.second / (double)cnt; entropy -= f * log(f); }
    q.entropy = entropy;
}

// The end of an attempt for a sequence that has not failed: cut to result_len and scored; the entropy rule may fail it
static void seq_finish(const whisper_full_params& p, Seq& q) {
    if (q.failed) return;
    q.tokens.resize(q.result_len);
    score_seq(p, q);
    if (q.result_len > 32 && q.entropy < p.entropy_thold) q.failed = true;
}

static void start_attempt(Sched& S, Job& j) {
    const Vocab& v = S.c->vocab;
    const float t = S.temps[j.temp_idx];
    j.seq = Seq();
    j.prompt.clear();
    if (!j.prompt_past.empty() && t < 0.5f && S.p.n_max_text_ctx > 0) {
        const int n_take = std::min(std::min(S.p.n_max_text_ctx, S.c->hp.n_text_ctx / 2), (int)j.prompt_past.size());
        j.prompt = {v.token_prev};
        j.prompt.insert(j.prompt.begin() + 1, j.prompt_past.end() - n_take, j.prompt_past.end());
    }
    j.prompt.insert(j.prompt.end(), j.prompt_init.begin(), j.prompt_init.end());
}

// a sampled attempt whose best_of candidates are drawn on the device (else: one host-sampled decoder)
static bool sample_attempt(const Sched& S, const Job& j) {
    return S.sample_n > 1 && j.temp_idx > 0 && S.temps[j.temp_idx] >= 1e-6f;
}

// (r: the row of the staging that ctl is; a grammar call notes the row's grammar state for ctl_upload, which follows the
// staging at once: the sequences are not touched in between)
static void fill_ctl(Sched& S, const Job& j, const Seq& q, int r, bool want_nosp) {
    SeqCtl& ctl = S.s->ws.h_ctl[r];
    const Vocab& v = S.c->vocab;
    const float t = S.temps[j.temp_idx];
    ctl.is_initial = q.tokens.empty();
    ctl.last_ts = q.tokens.size() > 0 && q.tokens.back().id >= v.token_beg;
    ctl.penult_ts = q.tokens.size() < 2 || q.tokens[q.tokens.size() - 2].id >= v.token_beg;
    ctl.has_ts = q.has_ts;
    ctl.seek_delta = q.seek_delta;
    ctl.temperature = t;
    ctl.suppress_blank = S.p.suppress_blank;
    ctl.no_timestamps = S.p.no_timestamps;
    ctl.suppress_eot = S.o.fixed_tokens > 0;
    if (S.p.max_initial_ts > 0.0f) {
        const float precision = float(WHISPER_CHUNK_SIZE) / S.c->hp.n_audio_ctx;
        ctl.tid0_initial = (int)std::round(S.p.max_initial_ts / precision);
    } else ctl.tid0_initial = -1;
    ctl.want_probs = t >= 1e-6f ? (sample_attempt(S, j) ? 2 : 1) : 0;
    ctl.want_nosp = want_nosp;
    if (S.s->gram_on) {
        if ((int)S.gram_rows.size() <= r) S.gram_rows.resize(r + 1, nullptr);
        S.gram_rows[r] = q.tokens.empty() ? &S.gram0 : &q.gram;
    }
    if (S.s->filter_on) {
        if ((int)S.filter_rows.size() <= r) S.filter_rows.resize(r + 1, nullptr);
        S.filter_rows[r] = &q;
    }
}

// whisper_full_params.tdrz_enable: a segment whose token range holds <|solm|> is followed by a speaker turn
static void mark_speaker_turn(const Sched& S, Segment& g) {
    if (!S.p.tdrz_enable) return;
    for (const TokenData& t : g.tokens)
        if (t.id == S.c->vocab.token_solm) g.speaker_turn_next = true;
}

static void finish_window(Sched& S, Job& j) {
    const Vocab& v = S.c->vocab;
    const whisper_full_params& p = S.p;
    const int seek_delta = j.seq.seek_delta;
    const int result_len = j.seq.result_len;
    const auto& toks = j.seq.tokens;
    const bool is_no_speech = (j.no_speech_prob > p.no_speech_thold && j.seq.avg_logprobs < p.logprob_thold);
    std::vector<int> past;
    if (j.prompt.front() == v.token_prev)
        past.insert(past.end(), j.prompt.begin() + 1, j.prompt.end() - j.prompt_init.size());
    for (int i = 0; i < result_len && !is_no_speech && i < (int)toks.size(); ++i) past.push_back(toks[i].id);
    j.prompt_past.swap(past);
    const size_t n_before = j.result.size();
    if (!toks.empty() && !is_no_speech) {
        int i0 = 0;
        int64_t t0 = j.seek + 2 * (toks.front().tid - v.token_beg);
        std::string text;
        for (int i = 0; i < (int)toks.size(); i++) {
            if (p.print_special || toks[i].id < v.token_eot) text += v.id_to_token[toks[i].id];
            if (toks[i].id > v.token_beg && !p.single_segment) {
                const int64_t t1 = j.seek + 2 * (toks[i].tid - v.token_beg);
                if (!text.empty()) {
                    j.result.push_back({t0, t1, text, j.no_speech_prob, {}});
                    for (int k = i0; k <= i; k++) j.result.back().tokens.push_back(toks[k]);
                    mark_speaker_turn(S, j.result.back());
                }
                text = "";
                while (i < (int)toks.size() && toks[i].id > v.token_beg) i++;
                i--;
                t0 = t1;
                i0 = i + 1;
            }
        }
        if (!text.empty()) {
            const int64_t t1 = j.seek + seek_delta;
            j.result.push_back({t0, t1, text, j.no_speech_prob, {}});
            for (int k = i0; k < (int)toks.size(); k++) j.result.back().tokens.push_back(toks[k]);
            mark_speaker_turn(S, j.result.back());
        }
    }
    j.n_new_segments = (int)(j.result.size() - n_before);
    if (S.c->dtw && j.n_new_segments > 0) {  // aligned by align_windows before the clip's next encode
        j.al_pending = true;
        j.al_seek = j.seek;
        j.al_frames = std::min(std::min(3000, seek_delta), j.seek_end - j.seek);
        j.al_seg0 = n_before;
    }
    if (p.token_timestamps && j.n_new_segments > 0) {  // placed by token_time_windows, after align_windows
        j.tt_pending = true;
        j.tt_seg0 = n_before;
    }
    j.dec.seek = j.seek;
    j.dec.temp_idx = j.temp_idx;
    j.dec.no_speech = is_no_speech;
    j.dec.no_speech_prob = j.no_speech_prob;
    j.decisions.push_back(j.dec);
    j.seek += seek_delta;
    j.phase = (j.seek + 10 >= j.seek_end) ? PH_DONE : PH_ENCODE;
}

// The attempt of j.seq is over (a beam or best_of attempt: its winner, already through seq_finish, which then changes
// nothing: the tokens are cut, and the score and the entropy rule give the same again)
static void attempt_done(Sched& S, Job& j) {
    const Seq& q = j.seq;
    seq_finish(S.p, j.seq);
    if (j.temp_idx == 0) {  // the greedy attempt's outcome (comparable with whisper.cpp bit for bit)
        j.dec = whisper_mi355x_window_decision{};
        j.dec.failed0 = q.failed;
        j.dec.logprob_fail0 = q.avg_logprobs < S.p.logprob_thold;
        j.dec.result_len0 = q.result_len;
        j.dec.avg_logprob0 = (float)q.avg_logprobs;
        j.dec.entropy0 = (float)q.entropy;
    }
    bool success = true;
    if (j.temp_idx != (int)S.temps.size() - 1)
        if (q.failed || q.avg_logprobs < S.p.logprob_thold) success = false;
    if (!success) {
        j.temp_idx++;
        j.phase = PH_PREFILL;
        return;
    }
    finish_window(S, j);
}


// ---- token timestamps from cross-attention DTW ------------------------------------------------------
// (DESIGN.md "Token timestamps (DTW)"; the algorithm is whisper.cpp's
// whisper_exp_compute_token_level_timestamps_dtw / OpenAI's timing.py)
static const whisper_ahead kAhTinyEn[] = {{1, 0}, {2, 0}, {2, 5}, {3, 0}, {3, 1}, {3, 2}, {3, 3}, {3, 4}};
static const whisper_ahead kAhTiny[] = {{2, 2}, {3, 0}, {3, 2}, {3, 3}, {3, 4}, {3, 5}};
static const whisper_ahead kAhBaseEn[] = {{3, 3}, {4, 7}, {5, 1}, {5, 5}, {5, 7}};
static const whisper_ahead kAhBase[] = {{3, 1}, {4, 2}, {4, 3}, {4, 7}, {5, 1}, {5, 2}, {5, 4}, {5, 6}};
static const whisper_ahead kAhSmallEn[] = {{6, 6}, {7, 0}, {7, 3}, {7, 8}, {8, 2}, {8, 5}, {8, 7}, {9, 0}, {9, 4}, {9, 8},
                                           {9, 10}, {10, 0}, {10, 1}, {10, 2}, {10, 3}, {10, 6}, {10, 11}, {11, 2}, {11, 4}};
static const whisper_ahead kAhSmall[] = {{5, 3}, {5, 9}, {8, 0}, {8, 4}, {8, 7}, {8, 8}, {9, 0}, {9, 7}, {9, 9}, {10, 5}};
static const whisper_ahead kAhMediumEn[] = {{11, 4}, {14, 1}, {14, 12}, {14, 14}, {15, 4}, {16, 0}, {16, 4}, {16, 9}, {17, 12},
                                            {17, 14}, {18, 7}, {18, 10}, {18, 15}, {20, 0}, {20, 3}, {20, 9}, {20, 14}, {21, 12}};
static const whisper_ahead kAhMedium[] = {{13, 15}, {15, 4}, {15, 15}, {16, 1}, {20, 0}, {23, 4}};
static const whisper_ahead kAhLargeV1[] = {{9, 19}, {11, 2}, {11, 4}, {11, 17}, {22, 7}, {22, 11}, {22, 17}, {23, 2}, {23, 15}};
static const whisper_ahead kAhLargeV2[] = {{10, 12}, {13, 17}, {16, 11}, {16, 12}, {16, 13}, {17, 15}, {17, 16}, {18, 4},
                                           {18, 11}, {18, 19}, {19, 11}, {21, 2}, {21, 3}, {22, 3}, {22, 9}, {22, 12},
                                           {23, 5}, {23, 7}, {23, 13}, {25, 5}, {26, 1}, {26, 12}, {27, 15}};
static const whisper_ahead kAhLargeV3[] = {{7, 0}, {10, 17}, {12, 18}, {13, 12}, {16, 1}, {17, 14}, {19, 11}, {21, 4}, {24, 1}, {25, 6}};
static const whisper_ahead kAhLargeV3Turbo[] = {{2, 4}, {2, 11}, {3, 3}, {3, 6}, {3, 11}, {3, 14}};

bool resolve_dtw(Context* c, const whisper_context_params& cp) {
    c->dtw = false;
    c->dtw_heads.clear();
    if (!cp.dtw_token_timestamps) return true;
    const int L = c->hp.n_text_layer, H = c->hp.n_text_head;
    auto bad = [](const char* what) {
        fprintf(stderr, "whisper_mi355x: dtw_token_timestamps: %s\n", what);
        return false;
    };
    const whisper_ahead* tab = nullptr;
    size_t n = 0;
#define WM_AH(name) tab = name, n = sizeof(name) / sizeof(name[0])
    switch (cp.dtw_aheads_preset) {
        case WHISPER_AHEADS_NONE: return bad("no alignment heads preset (WHISPER_AHEADS_NONE)");
        case WHISPER_AHEADS_N_TOP_MOST:
            if (cp.dtw_n_top < 1 || cp.dtw_n_top > L) return bad("dtw_n_top outside [1, n_text_layer]");
            for (int l = L - cp.dtw_n_top; l < L; l++)
                for (int h = 0; h < H; h++) c->dtw_heads.emplace_back(l, h);
            break;
        case WHISPER_AHEADS_CUSTOM: tab = cp.dtw_aheads.heads; n = tab ? cp.dtw_aheads.n_heads : 0; break;
        case WHISPER_AHEADS_TINY_EN: WM_AH(kAhTinyEn); break;
        case WHISPER_AHEADS_TINY: WM_AH(kAhTiny); break;
        case WHISPER_AHEADS_BASE_EN: WM_AH(kAhBaseEn); break;
        case WHISPER_AHEADS_BASE: WM_AH(kAhBase); break;
        case WHISPER_AHEADS_SMALL_EN: WM_AH(kAhSmallEn); break;
        case WHISPER_AHEADS_SMALL: WM_AH(kAhSmall); break;
        case WHISPER_AHEADS_MEDIUM_EN: WM_AH(kAhMediumEn); break;
        case WHISPER_AHEADS_MEDIUM: WM_AH(kAhMedium); break;
        case WHISPER_AHEADS_LARGE_V1: WM_AH(kAhLargeV1); break;
        case WHISPER_AHEADS_LARGE_V2: WM_AH(kAhLargeV2); break;
        case WHISPER_AHEADS_LARGE_V3: WM_AH(kAhLargeV3); break;
        case WHISPER_AHEADS_LARGE_V3_TURBO: WM_AH(kAhLargeV3Turbo); break;
        default: return bad("unknown alignment heads preset");
    }
#undef WM_AH
    for (size_t k = 0; k < n; k++) c->dtw_heads.emplace_back(tab[k].n_text_layer, tab[k].n_head);
    if (c->dtw_heads.empty()) return bad("empty alignment head list");
    for (auto& lh : c->dtw_heads)
        if (lh.first < 0 || lh.first >= L || lh.second < 0 || lh.second >= H) {
            c->dtw_heads.clear();
            return bad("an alignment head lies outside the model's n_text_layer x n_text_head");
        }
    // the score kernel runs once per layer: the list grouped by layer, each entry with its list index
    c->dtw_layer_first.assign(L + 1, 0);
    c->dtw_last_layer = -1;
    for (auto& lh : c->dtw_heads) {
        c->dtw_layer_first[lh.first + 1]++;
        c->dtw_last_layer = std::max(c->dtw_last_layer, lh.first);
    }
    for (int l = 0; l < L; l++) c->dtw_layer_first[l + 1] += c->dtw_layer_first[l];
    c->dtw = true;
    return true;
}

// score rows of one group of clips: at most this many bytes of P (a clip of 224 rows x 1500 frames is 1.3 MB
// per head; large-v3's 10 heads at 128 clips of ~130 rows: 1.0 GB)
static const size_t kAlignPBytes = (size_t)1 << 30;

static void ensure_align(Context* c, whisper_state* s) {
    Workspace& w = s->ws;
    {
        std::lock_guard<std::mutex> lk(c->dtw_mu);
        if (!c->dtw_heads_dev) {
            std::vector<int2> h(c->dtw_heads.size());
            std::vector<int> at(c->dtw_layer_first.begin(), c->dtw_layer_first.end() - 1);
            for (size_t a = 0; a < c->dtw_heads.size(); a++) h[at[c->dtw_heads[a].first]++] = make_int2(c->dtw_heads[a].second, (int)a);
            void* p = nullptr;
            WM_CHECK(hipMalloc(&p, h.size() * sizeof(int2)));
            WM_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(int2), hipMemcpyHostToDevice));
            c->dtw_heads_dev = p;
        }
    }
    if (w.al_clips && w.al_cap >= w.cap_jobs) return;
    free_align(w);
    // rows of a cost matrix: the `not` row + at most n_max = n_text_ctx / 2 - 4 text tokens
    const size_t rows = c->hp.n_text_ctx / 2 - 4 + 1, T = c->hp.n_audio_ctx, A = c->dtw_heads.size(), nj = w.cap_jobs;
    dalloc(w.al_clips, nj * sizeof(AlignClip));
    dalloc(w.al_stats, nj * A * T * 2 * sizeof(float));
    dalloc(w.al_cost, nj * rows * T * sizeof(float));
    dalloc(w.al_trace, nj * rows * T);
    dalloc(w.al_fr, nj * rows * sizeof(int));
    WM_CHECK(hipHostMalloc((void**)&w.h_al, nj * sizeof(AlignClip) + nj * rows * sizeof(int), 0));
    w.al_cap = (int)nj;
    w.al_rows = (int)rows;
}

// Align every window that just finished with new segments (Job::al_pending), all clips in one pass: the token
// rows [sot, lang?, not, text.., eot] of each window run teacher-forced from position 0 through the unfused
// prefill pass in the cached-K cross form, the alignment heads' softmaxed score rows are taken after each cross-Q
// GEMM, then cost matrix, DTW and backtrace run on the device and the first frame of every text row comes back.
// The pass overwrites the finished window's self-K/V rows of its slot: the clip's next window prefills from
// position 0, so nothing reads them again. Runs before the clip's next encode replaces its encoder output and
// cross K/V, and before the new-segment callback.
static void align_windows(Sched& S) {
    Context* c = S.c;
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    const Vocab& v = c->vocab;
    const Hparams& hp = c->hp;
    struct Item { int job, n_sot, F; std::vector<int> toks; std::vector<TokenData*> text; };
    std::vector<Item> items;
    for (int k = 0; k < (int)S.jobs.size(); k++) {
        Job& j = S.jobs[k];
        if (!j.al_pending) continue;
        j.al_pending = false;
        Item it;
        it.job = k;
        it.F = std::min(j.al_frames / 2, enc_ctx(c, s));
        it.toks = {v.token_sot};
        if (v.is_multilingual()) it.toks.push_back(v.token_sot + 1 + j.lang_id);
        it.n_sot = (int)it.toks.size();
        it.toks.push_back(v.token_not);
        for (size_t g = j.al_seg0; g < j.result.size(); g++)
            for (TokenData& td : j.result[g].tokens)
                if (td.id < v.token_eot) { it.toks.push_back(td.id); it.text.push_back(&td); }
        if (it.text.empty() || it.F < 1) continue;  // left unaligned
        it.toks.push_back(v.token_eot);
        items.push_back(std::move(it));
    }
    if (items.empty()) return;
    ScopeTimer timed{S.t_align};
    ensure_align(c, s);
    hipStream_t st = s->stream;
    if (s->direct) {  // the clips' cross K/V from their encoder output, as prompts too long for the direct prefill
        ensure_cross(c, s, w.cap_jobs);
        std::vector<int> slots;
        for (const Item& it : items) slots.push_back(S.jobs[it.job].slot);
        ensure_cross_cache(c, s, slots);
    }
    const size_t A = c->dtw_heads.size(), T = hp.n_audio_ctx;
    AlignClip* hc = (AlignClip*)w.h_al;
    int* h_fr = (int*)(w.h_al + (size_t)w.al_cap * sizeof(AlignClip));
    for (size_t i0 = 0; i0 < items.size();) {
        // one group: as many clips as fit the token buffers and the score buffer
        int nt = 0, ng = 0, max_rows = 0, max_n = 0, max_f = 0;
        size_t p_el = 0, st_el = 0, i1 = i0;
        int* hi = w.h_ints;
        const int ct = w.cap_tok;
        for (; i1 < items.size(); i1++) {
            const Item& it = items[i1];
            const int n = (int)it.toks.size();
            const size_t pe = A * n * it.F;
            if (ng > 0 && (nt + n > ct || (p_el + pe) * sizeof(float) > kAlignPBytes)) break;
            if (n > ct) WM_FAIL("alignment: %d token rows do not fit the decoder workspace", n);
            const Job& j = S.jobs[it.job];
            AlignClip& cl = hc[ng++];
            cl = AlignClip{};
            cl.slot = j.slot; cl.row0 = nt; cl.n_rows = n; cl.n_sot = it.n_sot; cl.frames = it.F;
            cl.p_off = (long)p_el; cl.st_off = (long)st_el;
            cl.cost_off = (long)((size_t)j.slot * w.al_rows * T);
            cl.tr_off = cl.cost_off;
            cl.fr_off = (long)j.slot * w.al_rows;
            p_el += pe;
            st_el += A * it.F * 2;
            for (int t = 0; t < n; t++) { hi[nt] = it.toks[t]; hi[ct + nt] = t; hi[2 * ct + nt] = j.slot; nt++; }
            max_rows = std::max(max_rows, n);
            max_n = std::max(max_n, n - it.n_sot - 1);
            max_f = std::max(max_f, it.F);
        }
        if (p_el > w.al_P_elems) {
            WM_CHECK(hipStreamSynchronize(st));
            dfree(w.al_P);
            w.al_P_elems = 0;
            dalloc(w.al_P, p_el * sizeof(float));
            w.al_P_elems = p_el;
        }
        WM_CHECK(hipMemcpyAsync(w.al_clips, hc, (size_t)ng * sizeof(AlignClip), hipMemcpyHostToDevice, st));
        decoder_upload(c, s, nt, 0, true);
        const AlignPass al{w.al_clips, ng, max_rows, nt, w.al_P};
        const DecView dv{0, nt, st, w.splitk, w.splitk_elems, w.xo, w.xml};
        decoder_rows_prefill(c, s, dv, 0, false, &al);
        {
            KT kt(s, K_ALIGN_COST, (double)p_el * 4 * 3);
            launch_align_cost(w.al_P, w.al_clips, ng, (int)A, max_n, max_f, w.al_stats, w.al_cost, st);
        }
        {
            KT kt(s, K_ALIGN_DTW, (double)ng * max_n * max_f * 5);
            launch_align_dtw(w.al_cost, w.al_clips, ng, max_n, w.al_trace, w.al_fr, nullptr, nullptr, st);
        }
        WM_CHECK(hipMemcpyAsync(h_fr, w.al_fr, (size_t)w.al_cap * w.al_rows * sizeof(int), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        for (size_t i = i0; i < i1; i++) {
            Item& it = items[i];
            const Job& j = S.jobs[it.job];
            const int* fr = h_fr + (size_t)j.slot * w.al_rows;
            for (size_t r = 0; r < it.text.size(); r++) it.text[r]->t_dtw = j.al_seek + 2 * (int64_t)fr[r + 1];  // row 0 = `not`
            s->align_info[it.job] = {(int)it.text.size() + 1, it.F, w.al_cost + (size_t)j.slot * w.al_rows * T};
        }
        i0 = i1;
    }
}

// Token times of every window that just finished with new segments (Job::tt_pending), whatever attempt decided it
// (greedy, beam, sampled: the segments hold the kept sequence's tokens). Per new segment, in order: phase 1 on the
// host (token_times.cpp) with the clip's state; then the voice-activity adjust of every segment of two tokens or more,
// all clips in one launch, only the {t0, t1, is_text} records crossing the bus; then, with max_len > 0, the wrap.
// Runs after align_windows, which holds pointers into the token vectors the wrap rebuilds (and so the pieces carry
// their t_dtw), and before the new-segment callback.
static void token_time_windows(Sched& S) {
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    const Vocab& v = S.c->vocab;
    const whisper_full_params& p = S.p;
    std::vector<int> pend;
    for (int k = 0; k < (int)S.jobs.size(); k++)
        if (S.jobs[k].tt_pending) pend.push_back(k);
    if (pend.empty()) return;
    ScopeTimer timed{S.t_tokts};
    std::vector<TtSeg> segs;
    std::vector<TtSpan> spans;
    struct Ref { int job; size_t seg; };
    std::vector<Ref> refs;
    std::vector<TtTok> tok;
    double bytes = 0;
    for (int k : pend) {
        Job& j = S.jobs[k];
        if (j.n_samples < 1) continue;  // no energy: the tokens keep t0 = t1 = -1
        for (size_t g = j.tt_seg0; g < j.result.size(); g++) {
            Segment& sg = j.result[g];
            tok.assign(sg.tokens.size(), TtTok());
            for (size_t i = 0; i < tok.size(); i++) {
                const TokenData& td = sg.tokens[i];
                tok[i].id = td.id; tok[i].tid = td.tid; tok[i].pt = td.pt; tok[i].ptsum = td.ptsum;
            }
            tt_phase1(tok, sg.t0, sg.t1, j.tt, v.token_beg, p.thold_pt, p.thold_ptsum, v.id_to_token);
            for (size_t i = 0; i < tok.size(); i++) {
                TokenData& td = sg.tokens[i];
                td.t0 = tok[i].t0; td.t1 = tok[i].t1; td.vlen = tok[i].vlen;
            }
            if (tok.size() < 2) continue;
            segs.push_back(TtSeg{k, (int)spans.size(), (int)tok.size(), 0});
            refs.push_back({k, g});
            for (const TtTok& t : tok) {
                const bool text = t.id < v.token_eot;
                spans.push_back(TtSpan{t.t0, t.t1, text ? 1 : 0, 0});
                if (text) bytes += 4.0 * std::min<double>(j.n_samples, 160.0 * (double)std::max<int64_t>(0, t.t1 - t.t0) + 4000.0);
            }
        }
    }
    if (!segs.empty()) {
        hipStream_t st = s->stream;
        tt_grow(w.tt_segs, w.tt_cap_segs, segs.size());
        tt_grow(w.tt_spans, w.tt_cap_spans, spans.size());
        WM_CHECK(hipMemcpyAsync(w.tt_segs, segs.data(), segs.size() * sizeof(TtSeg), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemcpyAsync(w.tt_spans, spans.data(), spans.size() * sizeof(TtSpan), hipMemcpyHostToDevice, st));
        {
            KT kt(s, K_TOKTS, bytes + 2.0 * spans.size() * sizeof(TtSpan));
            launch_token_vad(w.energy, w.tt_clips, w.tt_segs, (int)segs.size(), w.tt_spans, st);
        }
        WM_CHECK(hipMemcpyAsync(spans.data(), w.tt_spans, spans.size() * sizeof(TtSpan), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));
        for (size_t q = 0; q < segs.size(); q++) {
            Segment& sg = S.jobs[refs[q].job].result[refs[q].seg];
            for (int i = 0; i < segs[q].n_tok; i++) {
                sg.tokens[i].t0 = spans[segs[q].tok0 + i].t0;
                sg.tokens[i].t1 = spans[segs[q].tok0 + i].t1;
            }
        }
    }
    for (int k : pend) {
        Job& j = S.jobs[k];
        j.tt_pending = false;
        if (p.max_len <= 0) continue;
        std::vector<Segment> out(std::make_move_iterator(j.result.begin() + j.tt_seg0), std::make_move_iterator(j.result.end()));
        j.result.resize(j.tt_seg0);
        for (Segment& sg : out) {
            tok.assign(sg.tokens.size(), TtTok());
            for (size_t i = 0; i < tok.size(); i++) { tok[i].id = sg.tokens[i].id; tok[i].t0 = sg.tokens[i].t0; }
            for (TtPiece& pc : tt_wrap(tok, sg.t0, sg.t1, p.max_len, p.split_on_word, v.token_eot, v.id_to_token)) {
                j.result.push_back({pc.t0, pc.t1, std::move(pc.text), sg.no_speech_prob, {}});
                j.result.back().tokens.assign(sg.tokens.begin() + pc.i0, sg.tokens.begin() + pc.i1);
            }
        }
        j.n_new_segments = (int)(j.result.size() - j.tt_seg0);
    }
}

// teacher-forcing hook (FullOpts::spot): the raw logits rows of the spot jobs among `act` (row r of
// w.logits belongs to act[r]) for step `step` of each: the index of the token that process_step takes from the row
static void copy_spot_logits(Sched& S, const std::vector<int>& act) {
    if (!S.o.spot_logits || S.o.n_spot <= 0) return;
    Workspace& w = S.s->ws;
    const size_t V = S.c->hp.n_vocab;
    for (int r = 0; r < (int)act.size(); r++)
        for (int k = 0; k < S.o.n_spot; k++)
            if (S.o.spot[k] == act[r]) {
                const Seq& q = S.jobs[act[r]].seq;
                const int step = q.tokens.empty() ? 0 : q.step + 1;
                if (step < 0 || step >= S.o.fixed_tokens) continue;
                WM_CHECK(hipMemcpyAsync(S.o.spot_logits + ((size_t)step * S.o.n_spot + k) * V, w.logits + (size_t)r * V,
                                        V * 4, hipMemcpyDeviceToHost, S.s->stream));
            }
    WM_CHECK(hipStreamSynchronize(S.s->stream));
}

// One whisper_full "sample + update" iteration: the record r of a step's row applied to sequence q of clip j; returns
// true if decoding continues. The one place that advances q.step: the first token of an attempt (the prefill row's) has
// index 0, every later one the next index.
// (drawn: r is the record of a token drawn on the device, launch_sample, which applied the sampled branch's rules)
static bool process_step(Sched& S, const Job& j, Seq& q, const TokOut& r, const float* probs_row, bool drawn = false) {
    const Vocab& v = S.c->vocab;
    const whisper_full_params& p = S.p;
    if (!q.tokens.empty()) q.step++;
    const int i = q.step;
    const float t = S.temps[j.temp_idx];
    TokenData td;
    td.tid = r.tid; td.pt = r.pt; td.ptsum = r.ptsum;
    if (t < 1e-6f || drawn) {
        td.id = r.id; td.p = r.p; td.plog = r.plog;
    } else {
        const int n = v.n_vocab;
        std::discrete_distribution<> dist(probs_row, probs_row + n);
        td.id = dist(*j.rng);
        td.p = probs_row[td.id];
        td.plog = probs_row[n + td.id];
        if (td.id >= v.token_beg) { td.tid = td.id; td.pt = td.p; }
        else { td.tid = r.tid; td.pt = r.pt; }
    }
    if (S.o.forced && S.o.fixed_tokens > 0) td.id = S.o.forced[(long)j.slot * S.o.fixed_tokens + i];
    if (S.s->gram_on) {  // the grammar follows the token that is fed next (an attempt's first token: from the init state)
        if (q.tokens.empty()) q.gram = S.gram0;
        if (td.id >= 0 && td.id < (int)v.id_to_token.size()) q.gram.accept_token(S.s->gram_rules, v.id_to_token[td.id]);
    }
    q.tokens.push_back(td);
    q.sum_logprobs_all += td.plog;
    S.decoded++;
    const int delta_min = 10;
    if (td.id > v.token_beg) {
        const int sd_new = 2 * (td.id - v.token_beg);
        if (q.has_ts && q.seek_delta > sd_new && q.result_len < i && S.o.fixed_tokens <= 0) {
            q.failed = true;
            return false;
        }
        q.seek_delta = sd_new;
        q.result_len = i + 1;
        q.has_ts = true;
    }
    if (S.o.fixed_tokens > 0) {
        if (i == S.n_max_steps - 1) {  // fixed-work mode: one full window per chunk
            q.result_len = S.n_max_steps;
            q.seek_delta = 100 * WHISPER_CHUNK_SIZE;
            q.completed = true;
            return false;
        }
    } else if (td.id == v.token_eot || (p.max_tokens > 0 && i >= p.max_tokens) ||
               (q.has_ts && j.seek + q.seek_delta + delta_min >= j.seek_end)) {
        if (q.result_len == 0 && !p.no_timestamps) {
            if (j.seek + q.seek_delta + delta_min >= j.seek_end) q.result_len = i + 1;
            else { q.failed = true; return false; }
        }
        if (p.single_segment || p.no_timestamps) { q.result_len = i + 1; q.seek_delta = 100 * WHISPER_CHUNK_SIZE; }
        q.completed = true;
        return false;
    }
    if (S.o.fixed_tokens <= 0 && i == S.n_max_steps - 1 &&
        (q.result_len == 0 || q.seek_delta < 100 * WHISPER_CHUNK_SIZE / 2)) {
        q.failed = true;
        return false;
    }
    // whisper.cpp's loop runs i < n_max: after the last iteration nothing more is sampled (its
    // trailing decode cannot change the result, so it is skipped here)
    if (i + 1 >= S.n_max_steps) return false;
    return true;
}

// A step mode held for one step, also when an error unwinds. A mode with split slots runs in the cache form, whatever
// the call's cross form is (best_of candidates in a direct-form call): `direct` comes back with the mode's end.
struct ModeScope {
    whisper_state* s;
    const bool direct;
    ModeScope(whisper_state* s_, StepMode m) : s(s_), direct(s_->direct) {
        s->mode = m;
        if (m.split_slots) s->direct = false;
    }
    ~ModeScope() {
        s->mode = StepMode{};
        s->direct = direct;
    }
    ModeScope(const ModeScope&) = delete;
};

// A grammar call: the reject words of the first n staged rows' grammar states (Sched::gram_rows) into ws.gram, before the
// rows' logits launch (gram_masks: the reject kernel, the host for what it does not take)
static void gram_upload(Sched& S, int n) {
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    if ((int)S.gram_rows.size() < n) WM_FAIL("grammar: %d rows to upload, %zu staged", n, S.gram_rows.size());
    for (int r = 0; r < n; r++)
        if (!S.gram_rows[r]) WM_FAIL("grammar: row %d of %d was not staged", r, n);
    gram_masks(S.c, w.gd, s->gram_rules, S.gram_rows.data(), n, w.gram, w.h_gram, nullptr, s->stream, s);
}

// the SeqCtl of the first n staged rows to the device; true if a row wants its probs
static bool ctl_upload(Sched& S, int n) {
    Workspace& w = S.s->ws;
    if (S.s->gram_on) gram_upload(S, n);
    bool any_probs = false;
    for (int r = 0; r < n; r++) any_probs |= w.h_ctl[r].want_probs != 0;
    WM_CHECK(hipMemcpyAsync(w.ctl, w.h_ctl, n * sizeof(SeqCtl), hipMemcpyHostToDevice, S.s->stream));
    return any_probs;
}
// the launches' VocabIds: tdrz_enable keeps <|solm|> (its id matches no token, so no kernel code changes for it)
static VocabIds call_vid(const Context* c, const whisper_state* s) {
    VocabIds v = c->vid;
    if (s->tdrz_on) v.solm = -1;
    return v;
}
// The rules over the n rows' logits and the choice: the launch from before the callback existed (filtered null), or the
// prefiltered form over the rows the callbacks left in ws.frows
static void logits_rules(Context* c, whisper_state* s, int n, const float* filtered) {
    Workspace& w = s->ws;
    const uint32_t* deny = s->deny_on ? w.deny : nullptr;  // suppress_nst / suppress_regex (deny_prepare)
    const uint32_t* gram = s->gram_on ? w.gram : nullptr;  // the rows' grammar words (gram_upload)
    const float pen = s->gram_penalty;
    const VocabIds vid = call_vid(c, s);
    if (s->mode.topk > 0) {  // a beam step: top-k candidates per row (candidate 0 = the greedy record of the row)
        KT kt(s, K_TOPK, (double)n * c->hp.n_vocab * 4);
        launch_logits_topk(w.logits, c->hp.n_vocab, w.ctl, n, vid, w.cand, s->mode.topk, w.lrec, deny, gram, pen, s->stream, filtered);
        return;
    }
    KT kt(s, K_LOGITS, (double)n * c->hp.n_vocab * 4);
    launch_logits(w.logits, c->hp.n_vocab, w.ctl, n, vid, w.tout, w.probs, w.lrec, deny, gram, pen, s->stream, filtered);
}
// the tokens of a sampled step's rows drawn from their probs, the TokOut records rewritten in place
static void sample_launch(Context* c, whisper_state* s, int n) {
    Workspace& w = s->ws;
    KT kt(s, K_SAMPLE, (double)n * c->hp.n_vocab * 4 * 2);
    launch_sample(w.probs, c->hp.n_vocab, w.tout, w.tout, w.sctr, nullptr, s->sample_seed, c->vid.beg, n, s->stream);
}
// The logits launch of n staged rows. A call with a logits_filter_callback gets its first half only: the stage kernel
// writes the rows after the pre-callback rules to ws.frows, and logits_finish goes on from there.
static void logits_launch(Context* c, whisper_state* s, int n) {
    if (!s->filter_on) {
        logits_rules(c, s, n, nullptr);
        return;
    }
    Workspace& w = s->ws;
    KT kt(s, K_LOGITS_STAGE, (double)n * c->hp.n_vocab * 8);
    launch_logits_stage(w.logits, c->hp.n_vocab, w.ctl, n, call_vid(c, s), w.frows, s->stream);
}
// the n staged rows' copy to the pinned host rows, in stream order behind the stage kernel
static void filter_fetch(Sched& S, int n) {
    Workspace& w = S.s->ws;
    WM_CHECK(hipMemcpyAsync(w.h_frows, w.frows, (size_t)n * S.c->hp.n_vocab * sizeof(float), hipMemcpyDeviceToHost, S.s->stream));
}
// The staged rows to the host (the stream is drained by then), the caller's callback once per row in staged order, with
// the row's own sequence of this attempt as its history, and the rows back to the device
static void filter_round_trip(Sched& S, int n) {
    Context* c = S.c;
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    const size_t V = c->hp.n_vocab;
    if ((int)S.filter_rows.size() < n) WM_FAIL("logits filter: %d rows, %zu staged", n, S.filter_rows.size());
    if (!S.filter_fetched) {
        filter_fetch(S, n);
        WM_CHECK(hipStreamSynchronize(s->stream));
    }
    S.filter_fetched = false;
    for (int r = 0; r < n; r++) {
        const Seq* q = S.filter_rows[r];
        if (!q) WM_FAIL("logits filter: row %d of %d was not staged", r, n);
        S.filter_tokens.clear();
        for (const TokenData& t : q->tokens) S.filter_tokens.push_back(token_data(t));
        S.p.logits_filter_callback(c->owner, s, S.filter_tokens.data(), (int)S.filter_tokens.size(), w.h_frows + (size_t)r * V,
                                   S.p.logits_filter_callback_user_data);
    }
    WM_CHECK(hipMemcpyAsync(w.frows, w.h_frows, (size_t)n * V * sizeof(float), hipMemcpyHostToDevice, s->stream));
}
// The second half of a logits launch of a call with a callback: the round trip, the prefiltered form, a sampled step's draw
static void logits_second_half(Sched& S, int n) {
    if (!S.filter_reuse) filter_round_trip(S, n);
    logits_rules(S.c, S.s, n, S.s->ws.frows);
    if (S.s->mode.sample) sample_launch(S.c, S.s, n);
}
static void logits_finish(Sched& S, int n, bool any_probs, std::vector<std::vector<float>>& probs_rows) {
    Context* c = S.c;
    Workspace& w = S.s->ws;
    hipStream_t st = S.s->stream;
    if (S.s->filter_on) logits_second_half(S, n);
    if (S.s->mode.topk > 0) {
        WM_CHECK(hipMemcpyAsync(w.h_cand, w.cand, (size_t)n * kTopkMax * sizeof(TokOut), hipMemcpyDeviceToHost, st));
        probs_rows.assign(n, {});
        WM_CHECK(hipStreamSynchronize(st));
        return;
    }
    WM_CHECK(hipMemcpyAsync(w.h_tout, w.tout, n * sizeof(TokOut), hipMemcpyDeviceToHost, st));
    probs_rows.assign(n, {});
    if (any_probs) {  // sampling clips (t > 0): probs and logprobs rows for std::discrete_distribution
        const size_t V = c->hp.n_vocab;
        for (int r = 0; r < n; r++)
            if (w.h_ctl[r].want_probs == 1) {
                probs_rows[r].resize(2 * V);
                WM_CHECK(hipMemcpyAsync(probs_rows[r].data(), w.probs + (size_t)r * 2 * V, 2 * V * 4, hipMemcpyDeviceToHost, st));
            }
    }
    WM_CHECK(hipStreamSynchronize(st));
}
// logits kernel over the prefill rows of the `act` jobs (row r of w.logits belongs to act[r]) + D2H
static void prefill_logits(Sched& S, const std::vector<int>& act, std::vector<std::vector<float>>& probs_rows) {
    const int n = (int)act.size();
    for (int r = 0; r < n; r++) fill_ctl(S, S.jobs[act[r]], S.jobs[act[r]].seq, r, true);
    const bool any = ctl_upload(S, n);
    logits_launch(S.c, S.s, n);
    logits_finish(S, n, any, probs_rows);
}

// One decode step (decoder over n active clips + logits kernel) as a replayed hipGraph: the host
// cost of ~11 launches per layer is paid once per distinct n at capture time.
// After a persistent launch gave up, the state's steps take the per-kernel path for this long (a co-tenant
// holding CUs would otherwise cost the 50 ms timeout on every step)
static const double kPdecBackoffMs = 1000.0;

// the persistent launch's error word on the device (null for the launch chain)
static const unsigned* pd_err_ptr(Context* c, whisper_state* s, int pd) {
    const Hparams& hp = c->hp;
    Workspace& w = s->ws;
    if (pd == 1) return (const unsigned*)((const char*)w.pd_sync + pdec_granules(hp.n_text_state, hp.n_text_layer, hp.n_text_head).err_bytes);
    return nullptr;
}
static size_t ring_slot_bytes(const Workspace& w) { return (size_t)w.cap_jobs * sizeof(TokOut) + 16; }

// The decode graph of the planned step (keyed by its rows and pd: 0 launch chain, 1 persistent step), instance
// `par` (captured on first use; graphs of a persistent path captured under an older stamps pointer / spin
// limit are retired first). par 0: the per-step path's; par 1, 2: the pipelined path's two instances, which
// end with the device-side advance writing the step's results to ring slot par - 1.
static whisper_state::DecGraph* dec_graph(Context* c, whisper_state* s, StepPlan P, int par) {
    const int n = P.n, pd = P.path == STEP_PDEC;
    P.pipe = par > 0;
    const int sig = dec_path_sig();
    const int beam = s->mode.key();
    // read once: a setter stores its value before it bumps the generation, so a graph captured below under
    // generation `gen` holds that generation's (or a newer) stamps pointer and spin limit, and is retired later
    const int gen = g_pdec_gen.load(std::memory_order_acquire);
    for (size_t i = 0; i < s->dec_graphs.size();) {
        auto& g = s->dec_graphs[i];
        if (g.pdec && g.gen != gen) {
            hipGraphExecDestroy(g.exec);
            for (auto& e : g.ev) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
            s->dec_graphs.erase(s->dec_graphs.begin() + i);
        } else {
            i++;
        }
    }
    for (auto& g : s->dec_graphs)
        if (g.n_tok == n && g.n_rows == n && g.mask == s->ktime_mask && g.direct == s->direct && g.sig == sig && g.pdec == pd &&
            g.par == par && g.beam == beam && g.actx == enc_ctx(c, s) && g.deny == s->deny_on && g.gram == s->gram_on &&
            (!s->gram_on || g.gram_pen == s->gram_penalty) && (!s->mode.sample || g.seed == s->sample_seed) &&
            g.filt == s->filter_on && g.tdrz == s->tdrz_on)
            return &g;
    whisper_state::DecGraph g{n, n, s->ktime_mask, s->direct, sig, pd, gen, par, beam, nullptr, {}};
    g.seed = s->sample_seed;  // (a kernel argument of the draw below)
    g.actx = enc_ctx(c, s);
    g.deny = s->deny_on;
    g.gram = s->gram_on;
    g.gram_pen = s->gram_penalty;
    g.filt = s->filter_on;
    g.tdrz = s->tdrz_on;
    hipGraph_t graph;
    s->capture_ev = &g.ev;
    WM_CHECK(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    decoder_launch(c, s, P);
    logits_launch(c, s, n);
    if (s->mode.sample && !s->filter_on) sample_launch(c, s, n);  // (with a callback: after it, logits_second_half)
    if (par > 0) {
        Workspace& w = s->ws;
        char* slot = w.ring + (par - 1) * ring_slot_bytes(w);
        launch_decode_advance(n, w.cap_tok, c->vid.beg, w.tout, w.tok, w.ctl, (TokOut*)slot, pd_err_ptr(c, s, pd),
                              (unsigned*)(slot + (size_t)w.cap_jobs * sizeof(TokOut)), s->stream);
    }
    WM_CHECK(hipStreamEndCapture(s->stream, &graph));
    s->capture_ev = nullptr;
    WM_CHECK(hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0));
    WM_CHECK(hipGraphDestroy(graph));
    s->dec_graphs.push_back(std::move(g));
    return &s->dec_graphs.back();
}

// persistent launches of different states of this process on one device never overlap: two of them could hold
// half the CUs each. A pipelined run holds its device's lock for the whole run (a step is always in flight), so
// persistent steps of other threads on that device wait for it (documented). A caller's
// abort callback runs under the lock; if it calls back into the library on the same device from the same thread,
// that thread already holds the lock and does not take it again (g_pdec_held): its persistent launch then relies
// on the launch's bounded waits (a launch whose workgroups cannot all become resident gives up and the step
// re-runs on the per-kernel path) instead of deadlocking the thread on itself.
static std::mutex g_pdec_run_mu[16];
static thread_local unsigned g_pdec_held = 0;  // devices whose lock this thread holds (bit per device & 15)
struct PdecRunLock {
    int dev;
    bool owns = false;
    explicit PdecRunLock(int device, bool take = true) : dev(device & 15) {
        if (take) lock();
    }
    void lock() {
        if (owns || (g_pdec_held >> dev & 1)) return;
        g_pdec_run_mu[dev].lock();
        g_pdec_held |= 1u << dev;
        owns = true;
    }
    ~PdecRunLock() {
        if (!owns) return;
        g_pdec_held &= ~(1u << dev);
        g_pdec_run_mu[dev].unlock();
    }
};

// the plan of a step of n rows, with the state's backoff frozen for the step (step_variant and the step's
// graph see the same pdec_off) and the persistent path's buffers prepared
static StepPlan dec_path_prepare(Context* c, whisper_state* s, int n) {
    s->pdec_off = s->pdec_give_ups > 0 && now_ms() < s->pdec_off_until;
    const StepPlan P = step_plan(c, s, n, s->direct);
    if (P.path == STEP_PDEC) pdec_prepare(c, s);
    return P;
}

// The persistent launch of a step of n rows gave up (a wait timed out: not every workgroup became
// resident): the step again on the per-kernel path from the inputs on the device, which rewrites
// everything the launch may have written (the self K/V rows of this position); results in w.h_tout.
// Counted (whisper_mi355x_pdec_give_ups; t0: when the step began) and followed by kPdecBackoffMs of steps
// on the per-kernel path.
static void rerun_given_up(Sched& S, int n, bool any_probs, std::vector<std::vector<float>>& probs_rows, double t0) {
    Context* c = S.c;
    whisper_state* s = S.s;
    static bool warned = false;
    if (!warned) fprintf(stderr, "whisper_mi355x: persistent decode step timed out; step re-run on the per-kernel path\n");
    warned = true;
    *s->ws.h_pd_err = 0;
    decoder_launch(c, s, step_plan(c, s, n, s->direct, false));
    logits_launch(c, s, n);
    logits_finish(S, n, any_probs, probs_rows);
    s->pdec_give_ups++;
    g_pdec_give_ups_total++;
    s->pdec_off_until = now_ms() + kPdecBackoffMs;
    s->pdec_lost_ms += now_ms() - t0;
}

// The staged step of n rows (step_upload) through the par-0 graph of its plan, and its records on the host
// (logits_finish: w.h_tout and the wanted probs rows, or w.h_cand in the top-k mode).
static void run_step(Sched& S, int n, bool any_probs, std::vector<std::vector<float>>& probs_rows) {
    Context* c = S.c;
    whisper_state* s = S.s;
    const double t_step = now_ms();
    whisper_state::DecGraph* G = dec_graph(c, s, dec_path_prepare(c, s, n), 0);
    // A persistent launch needs its 256 workgroups resident together: persistent steps of different states
    // (threads) of this process on one device never overlap, so two of them cannot hold half the CUs each
    // (steps on different devices do not wait for each other)
    // (a call with a logits_filter_callback: the lock goes when the graph has run, before the callbacks; a launch that
    // gave up has staged nothing usable, so its re-run comes first and is the one whose rows the callbacks see)
    bool gave_up;
    {
        PdecRunLock lk(c->device, G->pdec != 0);
        WM_CHECK(hipGraphLaunch(G->exec, s->stream));
        if (s->filter_on) {
            filter_fetch(S, n);
            WM_CHECK(hipStreamSynchronize(s->stream));
        } else logits_finish(S, n, any_probs, probs_rows);
        gave_up = G->pdec && *s->ws.h_pd_err != 0;
    }
    kt_flush_graph(s, *G);
    if (gave_up) rerun_given_up(S, n, any_probs, probs_rows, t_step);  // (stages and fetches its own rows)
    else if (s->filter_on) {
        S.filter_fetched = true;
        logits_finish(S, n, any_probs, probs_rows);
    }
}

// Pipelined greedy decoding. The per-step path waits for a step's 32-byte results before it launches the next
// step, so every step pays the host's round trip (copy, synchronise, process_step, upload, launch: ~40-60 us,
// a fifth of a base-model persistent step). Here a small kernel advances every row's input token, position and
// logits-rule state on the device after the step (launch_decode_advance: the token the logits kernel chose, as
// process_step + fill_ctl would), the next step's graph is launched at once, and the host processes step k
// while step k + 1 runs. The results are the per-step path's bits: the same graphs on the same inputs. A row
// whose attempt ends at step k has had step k + 1 computed for it (its self-K/V row at the next position, never
// read: a new attempt prefills over it); the other rows' step k + 1 results are used, since a row's results
// do not depend on the other rows. Taken only where the host has nothing to decide per step: greedy attempts
// (no sampling), no forced tokens or logits hooks, no other job in another phase, and attempts that already
// decoded pipe_min_step() tokens (24; the speculative step at an attempt's end costs one step, which pays off only
// over a long attempt). WHISPER_MI355X_PIPE=0 turns it off.
static int pipe_min_step() {  // kPipeMinStep, or WHISPER_MI355X_PIPE_MIN (tests: exercise short attempts)
    const char* e = getenv("WHISPER_MI355X_PIPE_MIN");
    return e ? atoi(e) : 24;
}
static bool pipe_on() {  // (read per call: tests compare both paths in one process)
    const char* e = getenv("WHISPER_MI355X_PIPE");
    return !e || atoi(e) != 0;
}

static bool pipe_ok(Sched& S, const std::vector<int>& act) {
    if (!pipe_on() || S.o.forced || (S.o.spot_logits && S.o.n_spot > 0)) return false;
    if (S.s->gram_on) return false;  // the host advances the grammar after every step
    if (S.s->filter_on) return false;  // the host's callback sits in the middle of every step's logits rules
    for (size_t k = 0; k < S.jobs.size(); k++) {
        const Job& j = S.jobs[k];
        if (j.phase == PH_DONE) continue;
        if (j.phase != PH_DECODE) return false;
        if (S.temps[j.temp_idx] >= 1e-6f || j.seq.step < pipe_min_step()) return false;
    }
    return !act.empty();
}

// Everything about a decode step of n rows that can change a row's bits with n: the path (persistent step,
// small-M GEMMs, launch chain), the cache-form cross-attention kernel (the wide one up to
// attn_cross_wide_max() rows), the direct form's key-split count (xattn_splits), the logits GEMM's kernel
// (gemm_plan: gemm_kernel's 64-row tile up to 64 rows; above, rows 65..80 take gemm_dec_kernel unsplit and
// rows 81..128 gemm_glds_kernel, which give a row the same bits, so that boundary is not in the key:
// tests/test_gpu_kernels.py test_logits_gemm_rows_80_81_bitwise) and the number of 128-row groups
// (dec_groups). Equal keys: a row's results at n and at n' rows are the same bits.
static long step_variant(Context* c, whisper_state* s, int n) {
    const int pd = pdec_use(c, s, n, s->direct) ? 1 : 0;
    const bool small = n <= small_rows_max(c);  // deliberately coarser than step_plan's test (no w8, no gemm_small_ok)
    const bool wide = !s->direct && n <= attn_cross_wide_max();
    const int sp = s->direct ? xattn_splits(n, enc_ctx(c, s)) : 0;
    const Workspace& w = s->ws;
    const GemmPlan lg = gemm_plan(GemmShape{EPI_F32, n, c->hp.n_vocab, c->hp.n_text_state, w.splitk != nullptr, w.splitk_elems,
                                            false, false, false}, current_knobs());
    const bool lg64 = lg.kernel == GK_REG && lg.bm == 64;
    return pd | (long)small << 2 | (long)wide << 3 | (long)sp << 4 | (long)lg64 << 9 | (long)dec_groups(n) << 10;
}

// token `tok` at position `pos` of the clip in `slot` as row i of the decoder's host staging
static void stage_token(Workspace& w, int i, int tok, int pos, int slot) {
    w.h_ints[i] = tok; w.h_ints[w.cap_tok + i] = pos; w.h_ints[2 * w.cap_tok + i] = slot;
}

// Row r of a decode step's host staging: sequence q of clip j decodes its last token (the row's own logits row), with
// its self-cache rows in slot `sslot` (the clip's own slot, or a hypothesis's) and its logits-rule inputs
static void stage_row(Sched& S, const Job& j, const Seq& q, int sslot, int r) {
    Workspace& w = S.s->ws;
    stage_token(w, r, q.tokens.back().id, (int)j.prompt.size() + q.step, j.slot);
    w.h_ints[5 * w.cap_tok + r] = r;
    w.h_sslot[r] = sslot;
    fill_ctl(S, j, q, r, false);
}

// the n staged rows to the device (the self slots and the draw counters where the step's mode reads them); true if a
// row wants its probs
static bool step_upload(Sched& S, int n) {
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    decoder_upload(S.c, s, n, n, false);
    if (s->mode.split_slots) WM_CHECK(hipMemcpyAsync(w.sslot, w.h_sslot, n * sizeof(int), hipMemcpyHostToDevice, s->stream));
    const bool any_probs = ctl_upload(S, n);
    if (s->mode.sample) WM_CHECK(hipMemcpyAsync(w.sctr, w.h_sctr, (size_t)n * 4 * sizeof(int), hipMemcpyHostToDevice, s->stream));
    return any_probs;
}

// the inputs of a greedy / host-sampled decode step of the `act` jobs, staged and on the device
static bool step_inputs(Sched& S, const std::vector<int>& act) {
    for (int r = 0; r < (int)act.size(); r++) stage_row(S, S.jobs[act[r]], S.jobs[act[r]].seq, S.jobs[act[r]].slot, r);
    return step_upload(S, (int)act.size());
}

// one decode step of the `act` jobs on the per-step path; row r of w.h_tout and probs_rows belongs to act[r]
static void decode_step(Sched& S, const std::vector<int>& act, std::vector<std::vector<float>>& probs_rows) {
    const bool any_probs = step_inputs(S, act);
    run_step(S, (int)act.size(), any_probs, probs_rows);
}

// A pipelined step of the `act` rows gave up: the device's inputs again from the host's (the graphs' own
// advance has moved them on), then the re-run
static void pipe_give_up(Sched& S, const std::vector<int>& act, double t0) {
    const int n = (int)act.size();
    WM_CHECK(hipStreamSynchronize(S.s->stream));
    step_inputs(S, act);
    std::vector<std::vector<float>> probs_rows;
    rerun_given_up(S, n, false, probs_rows, t0);
}

// Decode the `act` jobs step after step with the next step in flight while the host processes the last one,
// until an attempt ends (or the caller's abort callback fires: returns true); the jobs are left exactly as the
// per-step path leaves them: every step it ran is processed, except the one in flight when the callback asked
// to abort (the per-step path would not have started it). The callback is asked after every step; when an
// attempt ended, the main loop asks it again before its next step (one call more than the per-step path).
static bool decode_pipelined(Sched& S, const std::vector<int>& act) {
    Context* c = S.c;
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    const int n = (int)act.size();
    hipStream_t st = s->stream;
    const size_t slot_b = ring_slot_bytes(w);
    if (!w.h_ring) {  // written by the advance kernel over the bus (coherent pinned memory), read after the event
        WM_CHECK(hipHostMalloc((void**)&w.h_ring, 2 * slot_b, hipHostMallocCoherent | hipHostMallocMapped));
        WM_CHECK(hipHostGetDevicePointer((void**)&w.ring, w.h_ring, 0));
    }
    for (auto& e : w.ring_ev)
        if (!e) WM_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    step_inputs(S, act);
    const StepPlan P = dec_path_prepare(c, s, n);
    const int pd = P.path == STEP_PDEC;
    dec_graph(c, s, P, 1);
    dec_graph(c, s, P, 2);  // (may grow dec_graphs: the pointers are taken after both exist)
    whisper_state::DecGraph* G[2] = {dec_graph(c, s, P, 1), dec_graph(c, s, P, 2)};
    PdecRunLock lk(c->device, pd != 0);
    double t_step = now_ms();
    WM_CHECK(hipGraphLaunch(G[0]->exec, st));
    WM_CHECK(hipEventRecord(w.ring_ev[0], st));
    for (int k = 0;; k++) {
        const int par = k & 1;
        char* hslot = w.h_ring + par * slot_b;
        // step k produces token j.step + 1 of each job; a job continues past it only if j.step + 2 < n_max. Step
        // k + 1 runs for every row, also for a row whose attempt ends at step k, so it is launched only when every
        // row's next position fits the self cache and the positional table (prompt + step + 1 < n_text_ctx: a
        // 229-token prompt at the 220-token limit would write row 448); otherwise the main loop's
        // per-step path decodes the rows that continue
        bool more = false, fits = true;
        for (int r = 0; r < n; r++) {
            const Job& j = S.jobs[act[r]];
            more |= j.seq.step + 2 < S.n_max_steps;
            fits &= (int)j.prompt.size() + j.seq.step + 1 < c->hp.n_text_ctx;
        }
        more = more && fits;
        if (more) {
            WM_CHECK(hipGraphLaunch(G[par ^ 1]->exec, st));
            WM_CHECK(hipEventRecord(w.ring_ev[par ^ 1], st));
        }
        s->cur_self_work += (double)n * c->hp.n_text_head * 64 * 2 * 2;  // (kernel timing: one more key per row)
        WM_CHECK(hipEventSynchronize(w.ring_ev[par]));
        kt_flush_graph(s, *G[par]);
        const TokOut* out = (const TokOut*)hslot;
        if (pd && *(const unsigned*)(hslot + (size_t)w.cap_jobs * sizeof(TokOut))) {
            // step k gave up: re-run it on the per-kernel path from the host's inputs, then leave
            pipe_give_up(S, act, t_step);
            for (int r = 0; r < n; r++) {
                Job& j = S.jobs[act[r]];
                if (!process_step(S, j, j.seq, w.h_tout[r], nullptr)) attempt_done(S, j);
            }
            return false;
        }
        bool ended = false;
        for (int r = 0; r < n; r++) {
            Job& j = S.jobs[act[r]];
            if (!process_step(S, j, j.seq, out[r], nullptr)) {
                attempt_done(S, j);
                ended = true;
            }
        }
        const bool aborted = abort_asked(S);
        if (!ended && !aborted && more) {
            t_step = now_ms();
            continue;
        }
        if (more) {
            // step k + 1 ran for every row: its results stand for the rows still decoding if a step of that
            // many rows computes the same bits (step_variant); otherwise the main loop runs step k + 1 again
            // for them from the host's inputs (the speculative one only wrote their self-K/V rows at the
            // next position, which the re-run writes again)
            WM_CHECK(hipMemcpyAsync(w.h_tout, w.tout, (size_t)n * sizeof(TokOut), hipMemcpyDeviceToHost, st));
            WM_CHECK(hipStreamSynchronize(st));
            kt_flush_graph(s, *G[par ^ 1]);
            if (aborted) {
                if (pd) *w.h_pd_err = 0;
                return true;
            }
            std::vector<int> still;
            for (int r = 0; r < n; r++)
                if (S.jobs[act[r]].phase == PH_DECODE) still.push_back(r);
            if (still.empty() || step_variant(c, s, (int)still.size()) != step_variant(c, s, n)) {
                if (pd) *w.h_pd_err = 0;  // (a discarded step's give-up is not one)
                return false;
            }
            if (pd && *(const unsigned*)(w.h_ring + (par ^ 1) * slot_b + (size_t)w.cap_jobs * sizeof(TokOut))) {
                // its persistent launch gave up: the step again, for all n rows, from the host's inputs (the
                // graph's own advance has moved the device's past step k + 1)
                pipe_give_up(S, act, now_ms());
            }
            for (int r : still) {
                Job& j = S.jobs[act[r]];
                if (!process_step(S, j, j.seq, w.h_tout[r], nullptr)) attempt_done(S, j);
            }
        }
        return aborted;
    }
}

// Batches above kPairMin clips run as two independent halves at
// once: the first on this state, the second on a twin state (its own streams, workspace and decode
// graphs, kept with this state for later calls) from a second host thread, and the twin's per-clip
// results are appended. Each half is exactly a batch of its own clips (the same bits as two separate
// calls), and one half's launch chain runs in the other's latency gaps: two 128-chunk large-v3 batches
// in flight measured 3720 vs 3201 audio-s/s back to back (profiles/r03_overlap_two_batches.txt),
// where one 256-row decode step ran as two lockstep row groups before.
static const int kPairMin = 128;
// decoder rows (clips x beams) of a beam-search call with beam_size > 1: every live beam of every clip is a row of
// one cache-form step (whisper_mi355x.h)
static const int kBeamMaxRows = 32;
std::atomic<long> g_decoded_tokens_total{0};

// ---- beam search (WHISPER_SAMPLING_BEAM_SEARCH) --------------------------------------------------
// The t = 0 attempt of every window decodes beam_k hypotheses per clip: one decoder row per live beam, the rows of
// all clips in one step. A clip's rows share its cross slot and own their self slots (beam b of job k: slot
// b * n_jobs + k, so beam 0 has the clip's own slot, the one the prefill writes). After a step the top-k kernel's
// candidates are pooled per clip (beam.h), every live position takes its parent's state, runs process_step on
// the new token as greedy decoding does, and the self-cache rows that differ are gathered (kernels/beam.hip).
// beam_k = 1 takes greedy's own step plan (so it may run the persistent step and gives greedy's bits); beam_k > 1
// takes the launch chain in the cache form, where a row's results do not depend on the step's other rows.
static bool beam_attempt(const Sched& S, const Job& j) { return S.beam_k > 0 && j.temp_idx == 0 && S.temps[0] < 1e-6f; }

static BeamCand to_cand(const TokOut& t) {
    // (candidate 0 repeats the greedy record: id 0 with p 0 when the row has no token left)
    return BeamCand{t.p > 0.0f ? t.id : -1, t.tid, t.p, t.plog, t.pt, t.ptsum};
}

// Contract points 4 / 5 for job k. rows: the beams whose candidates are cands[r * kTopkMax + rank] (`first`: the
// prefill row, as beam 0); positions: the beam positions to fill. The copies of the re-parenting are appended
// to `copies`.
static void beam_reparent(Sched& S, int k, const std::vector<int>& rows, const TokOut* cands, const std::vector<int>& positions,
                          bool first, std::vector<KvCopy>& copies) {
    const Job& j = S.jobs[k];
    Hyps& B = S.hyps[k];
    const int K = S.beam_k;
    std::vector<BeamCand> bc(rows.size() * K);
    std::vector<double> sums(rows.size());
    for (size_t r = 0; r < rows.size(); r++) {
        sums[r] = first ? 0.0 : B.h[rows[r]].sum_logprobs_all;
        for (int q = 0; q < K; q++) bc[r * K + q] = to_cand(cands[r * kTopkMax + q]);
    }
    const std::vector<BeamPick> picks = beam_select(rows, sums, bc.data(), K, positions);
    std::vector<int> slots;
    for (const Hyp& b : B.h) slots.push_back(b.sslot);
    const std::vector<KvCopy> cp = beam_copies(picks, B.held, slots);
    for (const KvCopy& x : cp) {
        S.s->gather_rows += x.row1 - x.row0;
        S.s->gather_rows_full += x.row1;
    }
    copies.insert(copies.end(), cp.begin(), cp.end());
    const std::vector<Hyp> old = B.h;
    for (const BeamPick& pk : picks) {
        Hyp& b = B.h[pk.beam];
        if (pk.parent < 0) { b.failed = true; continue; }
        const int sl = b.sslot;
        b = old[pk.parent];
        b.sslot = sl;
        const size_t r = std::find(rows.begin(), rows.end(), pk.parent) - rows.begin();
        b.ended = !process_step(S, j, b, cands[r * kTopkMax + pk.rank], nullptr);
    }
}

// the self-cache copies of a step's re-parentings, all clips in one gather
static void beam_gather(Sched& S, std::vector<KvCopy>& copies) {
    if (copies.empty()) return;
    Context* c = S.c;
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    const Hparams& hp = c->hp;
    const long upr = (long)hp.n_text_layer * 2 * hp.n_text_head * 8;  // 16-byte units of one row: layers, K | V, heads
    const long need = beam_schedule(copies, upr);
    if ((int)copies.size() > w.cap_jobs) WM_FAIL("beam search: %zu self-cache copies for %d slots", copies.size(), w.cap_jobs);
    if (need > w.kvstage_units) {
        WM_CHECK(hipStreamSynchronize(s->stream));
        dfree(w.kvstage);
        w.kvstage_units = 0;
        dalloc(w.kvstage, (size_t)need * 16);
        w.kvstage_units = need;
    }
    double rows = 0;
    for (size_t i = 0; i < copies.size(); i++) {
        w.h_kvcp[i] = copies[i];
        rows += copies[i].row1 - copies[i].row0;
    }
    WM_CHECK(hipMemcpyAsync(w.kvcp, w.h_kvcp, copies.size() * sizeof(KvCopy), hipMemcpyHostToDevice, s->stream));
    KT kt(s, K_KV_GATHER, rows * upr * 16 * 2);
    launch_kv_gather(w.self, w.cap_jobs, hp.n_text_layer, hp.n_text_head, hp.n_text_ctx, w.h_kvcp, w.kvcp, (int)copies.size(),
                     w.kvstage, w.kvstage_units, s->stream);
}

// Contract point 4: the beams of job k start from the candidates of its prefill row (rank r to beam r)
static void beam_start(Sched& S, int k, const TokOut* cands, std::vector<KvCopy>& copies) {
    const Job& j = S.jobs[k];
    Hyps& B = S.hyps[k];
    const int K = S.beam_k, n_jobs = (int)S.jobs.size();
    B.h.assign(K, Hyp());
    B.held.assign(K, {});
    B.held[0] = j.prompt;  // the prefill wrote the prompt's rows into the clip's own slot
    std::vector<int> positions;
    for (int b = 0; b < K; b++) {
        B.h[b].sslot = b * n_jobs + j.slot;
        positions.push_back(b);
    }
    beam_reparent(S, k, {0}, cands, positions, true, copies);
}

// The end of a beam attempt (contract point 6) or of a best_of attempt of job k: its hypotheses scored as attempt_done
// scores a single decoder's sequence, the winner (beam_winner) moved into the Job (none: the attempt failed), the
// hypotheses recorded in `info` (beam_info[k] or cand_info[k]), and on to attempt_done
static void hyps_finish(Sched& S, int k, std::vector<Hyp>& hyps, std::vector<whisper_state::BeamRec>& info) {
    Job& j = S.jobs[k];
    const int K = (int)hyps.size();
    std::vector<double> score(K);
    std::vector<char> failed(K);
    std::vector<whisper_state::BeamRec> recs(K);
    for (int b = 0; b < K; b++) {
        Hyp& q = hyps[b];
        for (const TokenData& t : q.tokens) recs[b].tokens.push_back(t.id);
        recs[b].sum_logprobs_all = q.sum_logprobs_all;
        seq_finish(S.p, q);
        score[b] = q.score;
        failed[b] = q.failed;
        recs[b].flags = (q.completed ? 1 : 0) | (q.failed ? 2 : 0);
    }
    const int win = beam_winner(score, failed);
    if (win >= 0) {
        recs[win].flags |= 4;
        j.seq = std::move(static_cast<Seq&>(hyps[win]));
    } else {
        j.seq.failed = true;
    }
    info = std::move(recs);
    hyps.clear();
    attempt_done(S, j);
}

// The rows of a step of the `jobs` clips' live hypotheses, staged in job order: {job, hypothesis} of every row
// (`what`, max_rows: the row-limit message)
static std::vector<std::pair<int, int>> stage_hyps(Sched& S, const std::vector<int>& jobs, const char* what, int max_rows) {
    std::vector<std::pair<int, int>> rows;
    for (int k : jobs) {
        const std::vector<Hyp>& h = S.hyps[k].h;
        for (int b = 0; b < (int)h.size(); b++) {
            if (!h[b].live()) continue;
            if ((int)rows.size() >= max_rows) WM_FAIL("%s: more than %d rows in a step", what, max_rows);
            stage_row(S, S.jobs[k], h[b], h[b].sslot, (int)rows.size());
            rows.push_back({k, b});
        }
    }
    return rows;
}

// One decode step of every live beam of the `bjobs` clips (all in PH_BEAM), then the re-parenting of each clip
static void beam_step(Sched& S, const std::vector<int>& bjobs) {
    Workspace& w = S.s->ws;
    const int K = S.beam_k;
    const std::vector<std::pair<int, int>> rows = stage_hyps(S, bjobs, "beam search", w.cap_jobs);
    for (auto& kb : rows)  // this step writes the token's K/V row into the beam's slot
        S.hyps[kb.first].held[kb.second].push_back(S.hyps[kb.first].h[kb.second].tokens.back().id);
    const int n = (int)rows.size();
    {
        ModeScope mode(S.s, StepMode{K, K > 1, false});
        std::vector<std::vector<float>> probs_rows;
        step_upload(S, n);
        run_step(S, n, false, probs_rows);  // (K = 1 may run the persistent step, as a greedy step does)
    }
    std::vector<KvCopy> copies;
    for (int r0 = 0; r0 < n;) {
        const int k = rows[r0].first;
        std::vector<int> live;
        int r1 = r0;
        while (r1 < n && rows[r1].first == k) live.push_back(rows[r1++].second);
        beam_reparent(S, k, live, w.h_cand + (size_t)r0 * kTopkMax, live, false, copies);
        r0 = r1;
    }
    beam_gather(S, copies);
}

// ---- sampled attempts with best_of candidates ------------------------------------------------------
// A t > 0 attempt of a clip decodes sample_n candidates: one decoder row per live candidate, the rows of all clips
// in one cache-form step on the split-K launch chain, as beam steps run. A clip's rows share its cross slot and own
// their self slots (candidate b of job k: slot b * n_jobs + k; candidate 0 has the clip's own slot, the one the
// prefill writes). Every row's token is drawn on the device (kernels/sample.hip) from a counter that names the
// window, the attempt, the candidate and the token index, so only the 32-byte records come back per step, and a
// candidate's draws do not depend on the step's other rows. Candidates never change parents: the only self-cache
// copy is the prompt's rows at the start.

// The candidates of the sampled attempts that were just prefilled: `rows` = {job, its row of the prefill's logits
// launch}. One draw launch takes every candidate's first token from its clip's prefill row (the rows' probs are
// still in w.probs, their records in w.tout); the prompt's self-cache rows go to the candidates' own slots.
static void sample_start(Sched& S, const std::vector<std::pair<int, int>>& rows) {
    Context* c = S.c;
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    const int N = S.sample_n, n_jobs = (int)S.jobs.size(), m = (int)rows.size() * N;
    if (m > w.cap_jobs || m > kSampleMaxRows) WM_FAIL("best_of: %d candidate rows (at most %d)", m, std::min(w.cap_jobs, kSampleMaxRows));
    if (s->direct) {  // the steps run in the cache form: the clips' cross K/V from their encoder output
        std::vector<int> slots;
        for (auto& jr : rows) slots.push_back(S.jobs[jr.first].slot);
        ensure_cross(c, s, n_jobs);
        ensure_cross_cache(c, s, slots);
    }
    for (int q = 0; q < (int)rows.size(); q++) {
        const Job& j = S.jobs[rows[q].first];
        for (int b = 0; b < N; b++) {
            int* ctr = w.h_sctr + (size_t)(q * N + b) * 4;
            ctr[0] = j.seek; ctr[1] = 16 * j.temp_idx + b; ctr[2] = 0; ctr[3] = rows[q].second;
        }
    }
    WM_CHECK(hipMemcpyAsync(w.sctr, w.h_sctr, (size_t)m * 4 * sizeof(int), hipMemcpyHostToDevice, s->stream));
    {
        KT kt(s, K_SAMPLE, (double)m * c->hp.n_vocab * 4 * 2);
        launch_sample(w.probs, c->hp.n_vocab, w.tout, w.cand, w.sctr, nullptr, s->sample_seed, c->vid.beg, m, s->stream);
    }
    WM_CHECK(hipMemcpyAsync(w.h_cand, w.cand, (size_t)m * sizeof(TokOut), hipMemcpyDeviceToHost, s->stream));
    WM_CHECK(hipStreamSynchronize(s->stream));
    std::vector<KvCopy> copies;
    for (int q = 0; q < (int)rows.size(); q++) {
        Job& j = S.jobs[rows[q].first];
        std::vector<Hyp>& h = S.hyps[rows[q].first].h;
        h.assign(N, Hyp());
        for (int b = 0; b < N; b++) {
            Hyp& bm = h[b];
            bm.sslot = b * n_jobs + j.slot;
            bm.ended = !process_step(S, j, bm, w.h_cand[q * N + b], nullptr, true);
            if (b > 0 && bm.live()) copies.push_back(KvCopy{bm.sslot, j.slot, 0, (int)j.prompt.size(), 0, 0, 0});
        }
        j.phase = PH_SAMPLE;
    }
    beam_gather(S, copies);
}

// One decode step of every live candidate of the `sjobs` clips (all in PH_SAMPLE)
static void sample_step(Sched& S, const std::vector<int>& sjobs) {
    Workspace& w = S.s->ws;
    const std::vector<std::pair<int, int>> rows = stage_hyps(S, sjobs, "best_of", std::min(w.cap_jobs, kSampleMaxRows));
    const int n = (int)rows.size();
    for (int r = 0; r < n; r++) {  // the rows' draw counters
        const Job& j = S.jobs[rows[r].first];
        int* ctr = w.h_sctr + (size_t)r * 4;
        ctr[0] = j.seek; ctr[1] = 16 * j.temp_idx + rows[r].second; ctr[2] = S.hyps[rows[r].first].h[rows[r].second].step + 1; ctr[3] = r;
    }
    {
        ModeScope mode(S.s, StepMode{0, true, true});
        // (rerun_given_up would not draw; split slots never plan the persistent step: pdec_use)
        if (pdec_use(S.c, S.s, n, S.s->direct)) WM_FAIL("best_of: a sampled step planned the persistent path");
        std::vector<std::vector<float>> probs_rows;
        step_upload(S, n);
        run_step(S, n, false, probs_rows);  // the records only: the rows' probs stay on the device (want_probs = 2)
    }
    for (int r = 0; r < n; r++) {
        Hyp& q = S.hyps[rows[r].first].h[rows[r].second];
        q.ended = !process_step(S, S.jobs[rows[r].first], q, w.h_tout[r], nullptr, true);
    }
}

// The scheduler's pass over the clips in phase `ph` (PH_BEAM, PH_SAMPLE): a clip without a live hypothesis ends its
// attempt (also right after the prefill; its hypotheses go to info[clip]), the live hypotheses of all the others take
// one step together. A pass as full_batch_one's others: S.aborted when the abort callback fired before the step.
static int hyps_pass(Sched& S, Phase ph, void (*step)(Sched&, const std::vector<int>&), std::vector<std::vector<whisper_state::BeamRec>>& info) {
    std::vector<int> jobs;
    for (int k = 0; k < (int)S.jobs.size(); k++) {
        if (S.jobs[k].phase != ph) continue;
        if (S.hyps[k].live()) jobs.push_back(k);
        else hyps_finish(S, k, S.hyps[k].h, info[k]);
    }
    if (jobs.empty()) return 0;
    if (abort_asked(S)) { S.aborted = true; return 0; }
    ScopeTimer timed{S.t_decode};
    step(S, jobs);
    return 0;
}
static int pass_beam(Sched& S) { return hyps_pass(S, PH_BEAM, beam_step, S.s->beam_info); }
static int pass_sample(Sched& S) { return hyps_pass(S, PH_SAMPLE, sample_step, S.s->cand_info); }

// whisper_full_params.audio_ctx against the model's context: 0, or -5 and the stderr line
static int check_audio_ctx(const Context* c, int audio_ctx) {
    if (audio_ctx <= c->hp.n_audio_ctx) return 0;
    fprintf(stderr, "whisper_mi355x: audio_ctx is larger than the maximum allowed (%d > %d)\n", audio_ctx, c->hp.n_audio_ctx);
    return -5;
}

// The twin's half of a paired batch (n clips) appended to the caller's state: per-clip results, then the counters.
// The halves ran concurrently: a phase lasted as long as its slower half; kernel time adds up.
static void merge_twin(whisper_state* s, whisper_state* t, int n) {
    for (int j = 0; j < n; j++) {
        s->results.push_back(std::move(t->results[j]));
        s->lang_ids.push_back(t->lang_ids[j]);
        s->decisions.push_back(std::move(t->decisions[j]));
        s->align_info.push_back(t->align_info[j]);  // (its cost matrix stays in the twin's workspace)
        s->beam_info.push_back(std::move(t->beam_info[j]));
        s->cand_info.push_back(std::move(t->cand_info[j]));
        if (j < (int)t->vad_maps.size()) s->vad_maps.push_back(std::move(t->vad_maps[j]));
    }
    s->vad_ms = std::max(s->vad_ms, t->vad_ms);
    s->align_ms = std::max(s->align_ms, t->align_ms);
    s->tokts_ms = std::max(s->tokts_ms, t->tokts_ms);
    s->decoded_tokens += t->decoded_tokens;
    s->pdec_give_ups += t->pdec_give_ups;
    s->pdec_lost_ms += t->pdec_lost_ms;
    t->pdec_give_ups = 0;
    t->pdec_lost_ms = 0;
    for (int k = 0; k < 5; k++) s->phase_ms[k] = std::max(s->phase_ms[k], t->phase_ms[k]);
    for (int k = 0; k < K_NCLASS; k++) {
        s->kstat[k].ms += t->kstat[k].ms;
        s->kstat[k].work += t->kstat[k].work;
        s->kstat[k].count += t->kstat[k].count;
        t->kstat[k] = KStat();
    }
    for (int k = 0; k < 3; k++) {
        s->vad_kstat[k].ms += t->vad_kstat[k].ms;
        s->vad_kstat[k].work += t->vad_kstat[k].work;
        s->vad_kstat[k].count += t->vad_kstat[k].count;
        t->vad_kstat[k] = KStat();
    }
}

// ---- full_batch_one: set-up, then a pass per phase of whisper.cpp's per-clip state machine, then the results ---------
// Checks the call's arguments and fills S.beam_k and S.sample_n; 0, or the call's error code
static int check_args(Sched& S, int n_jobs) {
    const auto fail = [](int rc, const char* fmt, auto... a) { fprintf(stderr, fmt, a...); return rc; };  // one stderr line
    // beam search: beam_size hypotheses per clip at t = 0; patience is accepted and ignored
    if (S.p.strategy == WHISPER_SAMPLING_BEAM_SEARCH) {
        S.beam_k = std::max(1, S.p.beam_search.beam_size);
        if (S.beam_k > kBeamMax) return fail(-4, "whisper_mi355x: beam_size %d > %d\n", S.beam_k, kBeamMax);
        if (S.o.fixed_tokens > 0) {
            fprintf(stderr, "whisper_mi355x: the fixed-work mode decodes greedily (no beam search)\n");
            return -1;
        }
        if (S.beam_k > 1 && (long)n_jobs * S.beam_k > kBeamMaxRows)
            return fail(-1, "whisper_mi355x: beam search of %d clips x %d beams exceeds %d decoder rows per step\n", n_jobs, S.beam_k,
                        kBeamMaxRows);
    } else if (S.p.strategy != WHISPER_SAMPLING_GREEDY) return fail(-100, "whisper_mi355x: unknown sampling strategy %d\n", (int)S.p.strategy);
    // whisper.cpp uses best_of for sampled (t > 0) fallback attempts only, under both strategies: t = 0 is unaffected.
    // (the fixed-work mode has no fallback)
    S.sample_n = S.o.fixed_tokens > 0 ? 1 : std::max(1, S.p.greedy.best_of);
    if (S.sample_n > kBeamMax) return fail(-4, "whisper_mi355x: best_of %d > %d\n", S.sample_n, kBeamMax);
    if (S.sample_n > 1 && (long)n_jobs * S.sample_n > kBeamMaxRows) {
        // every candidate is a decoder row with its own self slot; above the row limit sampled attempts run one
        // host-sampled candidate per clip (the reference's Greedy{best_of: 1})
        static const int warned = fail(0, "whisper_mi355x: best_of=%d x %d clips exceeds %d decoder rows per step: fallback attempts sample 1 candidate\n",
                                       S.sample_n, n_jobs, kBeamMaxRows);  // (once per process)
        S.sample_n = 1;
    }
    return 0;
}

// audio_ctx. whisper_full_with_state detects the language before it checks and stores
// params.audio_ctx in the state, so the detection pass encodes at the state's earlier value (0 on a fresh state,
// and for every clip of the batch API); this is that check-and-store, run once: after the detection pass, or before the
// loop when there is none, or after the loop when nothing was encoded.
static int apply_audio_ctx(Sched& S) {
    if (S.ctx_applied || S.p.detect_language) return 0;
    S.ctx_applied = true;
    if (const int r = check_audio_ctx(S.c, S.p.audio_ctx)) return r;
    S.s->audio_ctx = S.p.audio_ctx;
    return 0;
}

// the tokens every attempt of the clip begins with, once its language is known; false: a language outside the table
static bool build_prompt_init(Sched& S, Job& j) {
    const Vocab& v = S.c->vocab;
    j.prompt_init = {v.token_sot};
    if (v.is_multilingual()) {
        if (j.lang_id < 0) return false;
        j.prompt_init.push_back(v.token_sot + 1 + j.lang_id);
        j.prompt_init.push_back(S.p.translate ? v.token_translate : v.token_transcribe);
    }
    if (S.p.no_timestamps) j.prompt_init.push_back(v.token_not);
    return true;
}

// The clips of the call as jobs (after compute_mel): the carried and the initial prompt, the seek range, the rng, the
// first phase. -3: the single API's auto-detect has no audio (whisper_full_with_state); -7: see build_prompt_init.
static int make_jobs(Sched& S, const int* n, int n_jobs) {
    const whisper_full_params& p = S.p;
    S.need_lang = p.language == nullptr || strlen(p.language) == 0 || strcmp(p.language, "auto") == 0 || p.detect_language;
    std::vector<int> init_prompt_tokens;
    if (!p.prompt_tokens && p.initial_prompt) init_prompt_tokens = tokenize(S.c->vocab, p.initial_prompt);
    else if (p.prompt_tokens && p.prompt_n_tokens > 0) init_prompt_tokens.assign(p.prompt_tokens, p.prompt_tokens + p.prompt_n_tokens);
    const bool is_distil = S.c->hp.n_text_layer == 2 && S.c->hp.n_vocab != 51866;
    S.p.no_timestamps = p.no_timestamps || is_distil;
    S.jobs.resize(n_jobs);
    for (int k = 0; k < n_jobs; k++) {
        Job& j = S.jobs[k];
        j.slot = k;
        j.single = S.single_api && k == 0;
        j.n_samples = n[k];
        j.n_len = mel_n_len(n[k]);
        j.n_len_org = mel_n_len_org(n[k]);
        j.seek_start = S.o.pieces && !j.single ? 0 : p.offset_ms / 10;  // (a later piece of a recording: offset_ms = 0)
        j.seek_end = p.duration_ms == 0 ? j.n_len_org : j.seek_start + p.duration_ms / 10;
        j.seek = j.seek_start;
        j.rng = j.single ? &S.s->rng : &j.own_rng;
        if (j.single) j.prompt_past = S.s->prompt_past;
        if (p.no_context) j.prompt_past.clear();
        if (!init_prompt_tokens.empty()) {
            for (int t : init_prompt_tokens) j.prompt_past.push_back(t);
            std::rotate(j.prompt_past.begin(), j.prompt_past.end() - init_prompt_tokens.size(), j.prompt_past.end());
        }
        const bool no_audio = S.need_lang && 0 >= j.n_len_org;  // whisper_full_with_state: failed auto-detect -> -3
        if (no_audio && j.single && !S.vad_on) return -3;  // (a clip the VAD found no speech in: no segments, 0)
        if (no_audio || j.seek_end < j.seek_start + 10) { j.phase = PH_DONE; continue; }
        j.lang_pending = S.need_lang;
        if (!S.need_lang) j.lang_id = lang_index(p.language);
        j.phase = PH_ENCODE;
    }
    for (auto& j : S.jobs)
        if (j.phase != PH_DONE && !j.lang_pending && !build_prompt_init(S, j)) return -7;
    return 0;
}

// The passes of the scheduler loop. Each takes the Sched, works on every clip that is in its phase and moves it on.
// It returns 0, or the error code that the call returns at once (nothing is published), and sets S.aborted when a
// callback asked to stop: the loop then ends, and the call returns 0 with the windows finished so far.
// pass_encode encodes every window that is due. Per clip, in clip order: the progress callback, the "nothing left" test, the
// encoder-begin callback (false stops the call), the abort callback; a stop ends the pass before anything is encoded.
static int pass_encode(Sched& S) {
    const whisper_full_params& p = S.p;
    std::vector<int> wj, ws_, wsl;
    for (int k = 0; k < (int)S.jobs.size(); k++) {
        Job& j = S.jobs[k];
        if (j.phase != PH_ENCODE) continue;
        if (j.single && p.progress_callback) {
            const int prog = (100 * (j.seek - j.seek_start)) / std::max(1, j.seek_end - j.seek_start);
            p.progress_callback(S.c->owner, S.s, prog, p.progress_callback_user_data);
        }
        if (j.seek + 10 >= j.seek_end && !j.lang_pending) { j.phase = PH_DONE; continue; }
        if (((S.single_api || S.o.pieces) && p.encoder_begin_callback && !p.encoder_begin_callback(S.c->owner, S.s, p.encoder_begin_callback_user_data)) ||
            abort_asked(S)) {
            S.aborted = true;
            return 0;
        }
        wj.push_back(k);
        ws_.push_back(j.lang_pending ? 0 : j.seek);
        wsl.push_back(j.slot);
    }
    if (wj.empty()) return 0;
    { ScopeTimer timed{S.t_enc}; encode_windows(S.c, S.s, wj.data(), ws_.data(), wsl.data(), (int)wj.size()); }
    for (int k : wj) {
        Job& j = S.jobs[k];
        if (j.lang_pending) { j.phase = PH_LANG; continue; }
        if (j.seek > j.seek_start && j.seek + 500 >= j.seek_end) j.prompt_past.clear();
        j.temp_idx = 0;
        j.phase = PH_PREFILL;
    }
    return 0;
}

std::vector<std::pair<float, int>> rank_languages(const float* logits) {
    std::map<std::string, int> g_lang;  // whisper.cpp iterates g_lang, a std::map: the codes in key order
    for (int i = 0; i < 100; i++) g_lang[k_lang_codes[i]] = i;
    std::vector<std::pair<float, int>> ids;
    for (auto& kv : g_lang) ids.emplace_back(logits[kv.second], kv.second);
    std::sort(ids.begin(), ids.end(), [](const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first > b.first; });
    return ids;
}

// Language detection: [sot] at position 0 of every clip that waits for it, the best of the language logits. Every
// clip of the call detects in this one pass (need_lang holds for all of them), so apply_audio_ctx follows it here.
static int pass_lang(Sched& S) {
    Context* c = S.c;
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    const Vocab& v = c->vocab;
    std::vector<int> act;
    for (int k = 0; k < (int)S.jobs.size(); k++) if (S.jobs[k].phase == PH_LANG) act.push_back(k);
    if (act.empty()) return 0;
    const int na = (int)act.size();
    const int det_ctx = enc_ctx(c, s);
    std::vector<float> lg((size_t)na * 100);
    {
        ScopeTimer timed{S.t_prefill};
        for (int r = 0; r < na; r++) {
            stage_token(w, r, v.token_sot, 0, S.jobs[act[r]].slot);
            w.h_ints[5 * w.cap_tok + r] = r;
        }
        decoder_forward(c, s, na, na);
        for (int r = 0; r < na; r++)
            WM_CHECK(hipMemcpyAsync(lg.data() + r * 100, w.logits + (size_t)r * c->hp.n_vocab + v.token_sot + 1, 100 * 4,
                                    hipMemcpyDeviceToHost, s->stream));
        WM_CHECK(hipStreamSynchronize(s->stream));
    }
    if (const int r = apply_audio_ctx(S)) return r;
    // window 0 as the detection encoded it serves the first attempt only at the same audio context
    const bool same_ctx = enc_ctx(c, s) == det_ctx;
    for (int r = 0; r < na; r++) {
        Job& j = S.jobs[act[r]];
        j.lang_id = rank_languages(lg.data() + r * 100)[0].second;
        j.lang_pending = false;
        if (!build_prompt_init(S, j)) return -7;
        if (S.p.detect_language) { j.phase = PH_DONE; continue; }
        if (j.seek == 0 && same_ctx) {
            j.temp_idx = 0;
            j.phase = PH_PREFILL;
        } else j.phase = PH_ENCODE;
    }
    return 0;
}

// Prefills every attempt that is due: the prompt rows, the logits of each last row (again in the top-k form when a
// row is a beam attempt), then per row the attempt's first token, its beams or its best_of candidates.
static int pass_prefill(Sched& S) {
    Context* c = S.c;
    whisper_state* s = S.s;
    Workspace& w = s->ws;
    std::vector<int> act;
    for (int k = 0; k < (int)S.jobs.size(); k++) if (S.jobs[k].phase == PH_PREFILL) act.push_back(k);
    if (act.empty()) return 0;
    if (abort_asked(S)) { S.aborted = true; return 0; }
    const int na = (int)act.size();
    {
        ScopeTimer timed{S.t_prefill};
        int nt = 0;
        for (int r = 0; r < na; r++) {
            Job& j = S.jobs[act[r]];
            start_attempt(S, j);
            for (int t = 0; t < (int)j.prompt.size(); t++) stage_token(w, nt++, j.prompt[t], t, j.slot);
            w.h_ints[5 * w.cap_tok + r] = nt - 1;
        }
        decoder_forward(c, s, nt, na);
        prefill_logits(S, act, S.probs_rows);
        bool any_beam = false;
        for (int k : act) any_beam |= beam_attempt(S, S.jobs[k]);
        if (any_beam) {  // the same rows again through the top-k form (candidate 0 = the record above)
            ModeScope mode(s, StepMode{S.beam_k, false, false});
            std::vector<std::vector<float>> none;
            if (s->filter_on) {  // the rows the callbacks just edited are on the device: no second call per row
                S.filter_reuse = true;
                try { logits_finish(S, na, false, none); } catch (...) { S.filter_reuse = false; throw; }
                S.filter_reuse = false;
            } else {
                logits_launch(c, s, na);
                logits_finish(S, na, false, none);
            }
        }
    }
    copy_spot_logits(S, act);
    std::vector<KvCopy> copies;
    std::vector<std::pair<int, int>> srows;  // sampled attempts with best_of candidates: {job, row}
    for (int r = 0; r < na; r++) {
        Job& j = S.jobs[act[r]];
        j.no_speech_prob = w.h_tout[r].nosp_prob;
        if (sample_attempt(S, j)) { srows.push_back({act[r], r}); continue; }
        if (beam_attempt(S, j)) {
            beam_start(S, act[r], w.h_cand + (size_t)r * kTopkMax, copies);
            j.phase = PH_BEAM;
            continue;
        }
        if (process_step(S, j, j.seq, w.h_tout[r], S.probs_rows[r].empty() ? nullptr : S.probs_rows[r].data())) j.phase = PH_DECODE;
        else attempt_done(S, j);
    }
    if (!copies.empty()) { ScopeTimer timed{S.t_decode}; beam_gather(S, copies); }  // the prompt's rows to the other beams' slots
    if (!srows.empty()) { ScopeTimer timed{S.t_decode}; sample_start(S, srows); }
    return 0;
}

// Greedy and host-sampled attempts: one decode step for every clip that is decoding, or a pipelined run of steps until
// an attempt ends (decode_pipelined) where the host has nothing to decide per step
static int pass_decode(Sched& S) {
    std::vector<int> act;
    for (int k = 0; k < (int)S.jobs.size(); k++) if (S.jobs[k].phase == PH_DECODE) act.push_back(k);
    if (act.empty()) return 0;
    const bool pipe = pipe_ok(S, act);
    if (abort_asked(S)) { S.aborted = true; return 0; }
    if (pipe) { ScopeTimer timed{S.t_decode}; S.aborted = decode_pipelined(S, act); return 0; }
    { ScopeTimer timed{S.t_decode}; decode_step(S, act, S.probs_rows); }
    copy_spot_logits(S, act);
    for (int r = 0; r < (int)act.size(); r++) {
        Job& j = S.jobs[act[r]];
        if (!process_step(S, j, j.seq, S.s->ws.h_tout[r], S.probs_rows[r].empty() ? nullptr : S.probs_rows[r].data())) attempt_done(S, j);
    }
    return 0;
}

// ---- whisper_full_params.vad: the Silero filter ahead of the mel (vad.h) --------------------------------
std::shared_ptr<VadModel> vad_lookup(Context* c, const char* path) {
    std::lock_guard<std::mutex> lk(c->vad_mu);
    if (path && c->vad && c->vad_path == path) return c->vad;
    std::string err;
    VadModel* m = path ? vad_model_load_file(path, c->device, &err) : nullptr;
    if (!m) {
        fprintf(stderr, "whisper_mi355x: vad model '%s' refused: %s\n", path ? path : "(null)", path ? err.c_str() : "vad is set without vad_model_path");
        return nullptr;  // (the cached model stays)
    }
    const int device = c->device;
    c->vad = std::shared_ptr<VadModel>(m, [device](VadModel* q) { hipSetDevice(device); vad_model_free(q); });
    c->vad_path = path;
    return c->vad;
}

// a job's times from the filtered axis back to the original one: every segment's t0 / t1, and every token's t0, t1 and
// t_dtw that is set
static void vad_map_result(const std::vector<VadPiece>& map, std::vector<Segment>& segs) {
    for (Segment& g : segs) {
        g.t0 = vad_map_time(map, g.t0);
        g.t1 = vad_map_time(map, g.t1);
        for (TokenData& t : g.tokens) {
            if (t.t0 != -1) t.t0 = vad_map_time(map, t.t0);
            if (t.t1 != -1) t.t1 = vad_map_time(map, t.t1);
            if (t.t_dtw != -1) t.t_dtw = vad_map_time(map, t.t_dtw);
        }
    }
}

// The filter step of a call with vad set: the probabilities of every job (frontend, lstm; one copy back), the segments
// and piece tables on the host, the filtered PCM gathered on the device. After it the call reads S.vad_pcm / S.vad_n as
// device clips. 0, or -11 when the model is refused.
static int vad_filter(Sched& S, const float* const* pcm, const int* n, int n_jobs, bool on_device) {
    ScopeTimer timed{S.t_vad};
    const std::shared_ptr<VadModel> model = vad_lookup(S.c, S.p.vad_model_path);
    if (!model) return -11;
    whisper_state* s = S.s;
    struct Timing { whisper_state* s; std::optional<KT> kt; } tm{s, std::nullopt};  // the launch in flight, timed as class K_VAD
    const VadHooks hooks{[](void* u, int kernel, double bytes) { Timing* t = (Timing*)u; t->kt.emplace(t->s, K_VAD, bytes).sub = kernel; },
                         [](void* u) { ((Timing*)u)->kt.reset(); }, &tm};
    std::vector<std::vector<float>> probs;
    vad_probs_run(*model, s->ws.vad, pcm, n, n_jobs, on_device, s->stream, &hooks, probs, nullptr);
    const whisper_vad_params& q = S.p.vad_params;
    const VadParams vp{q.threshold, q.min_speech_duration_ms, q.min_silence_duration_ms, q.max_speech_duration_s, q.speech_pad_ms, q.samples_overlap};
    S.vad_maps.assign(n_jobs, {});
    for (int j = 0; j < n_jobs; j++)
        S.vad_maps[j] = vad_piece_table(vad_segments_from_probs(probs[j].data(), (int)probs[j].size(), vp), n[j], vp.samples_overlap);
    vad_gather_run(s->ws.vad, s->ws.vad.dev_pcm.data(), S.vad_maps, s->stream, &hooks, S.vad_pcm, S.vad_n);
    S.vad_on = true;
    return 0;
}

// the windows that just finished with new segments: DTW alignment, then token_timestamps' t0 / t1 / vlen and max_len wrap
static int pass_token_times(Sched& S) {
    if (S.c->dtw) align_windows(S);
    if (S.p.token_timestamps) token_time_windows(S);
    return 0;
}
// the single-clip API's new-segment callback for the window that just finished
static int pass_new_segment(Sched& S) {
    if (!S.single_api || !S.p.new_segment_callback || S.jobs[0].n_new_segments <= 0) return 0;
    Job& j = S.jobs[0];
    S.s->results[0] = j.result;
    if (S.vad_on) vad_map_result(S.vad_maps[0], S.s->results[0]);
    S.p.new_segment_callback(S.c->owner, S.s, j.n_new_segments, S.p.new_segment_callback_user_data);
    j.n_new_segments = 0;
    return 0;
}

// the call's results and timings into the state and the context
static void publish(Sched& S) {
    whisper_state* s = S.s;
    for (size_t k = 0; k < S.jobs.size(); k++) {
        s->results[k] = std::move(S.jobs[k].result);
        if (S.vad_on) vad_map_result(S.vad_maps[k], s->results[k]);
        s->lang_ids[k] = S.jobs[k].lang_id;
        s->decisions[k] = std::move(S.jobs[k].decisions);
    }
    if (S.single_api && !S.jobs.empty()) {
        s->prompt_past = S.jobs[0].prompt_past;
        s->lang_id = S.jobs[0].lang_id;
    }
    kt_flush(s);
    s->decoded_tokens = S.decoded;
    g_decoded_tokens_total += S.decoded;
    s->phase_ms[0] = S.t_mel; s->phase_ms[1] = S.t_enc; s->phase_ms[2] = S.t_prefill; s->phase_ms[3] = S.t_decode; s->phase_ms[4] = S.t_logits;
    s->align_ms = S.t_align;
    s->tokts_ms = S.t_tokts;
    s->vad_ms = S.t_vad;
    s->vad_maps = std::move(S.vad_maps);
    std::lock_guard<std::mutex> lk(S.c->timings_mu);
    S.c->timings.encode_ms += (float)S.t_enc;
    S.c->timings.decode_ms += (float)S.t_decode;
    S.c->timings.prompt_ms += (float)S.t_prefill;
}

// ---- the deny mask of suppress_nst / suppress_regex (suppress.h) ---------------------------------------
int deny_lookup(Context* c, bool suppress_nst, const char* regex, std::vector<uint32_t>* words) {
    Context::DenyKey key;
    key.nst = suppress_nst;
    key.has_regex = regex != nullptr;
    if (regex) key.regex = regex;
    std::lock_guard<std::mutex> lk(c->deny_mu);
    if (!c->deny_cached || !(c->deny_key == key)) {
        std::vector<uint32_t> built;
        std::string err;
        if (suppress_build(c->vocab.token_to_id, c->hp.n_vocab, suppress_nst, regex, built, &err) != 0) {
            fprintf(stderr, "whisper_mi355x: suppress_regex '%s' does not compile: %s\n", regex, err.c_str());
            return -8;  // (the cached mask stays)
        }
        c->deny_words.swap(built);
        c->deny_key = key;
        c->deny_cached = true;
        c->deny_builds++;
    }
    if (words) *words = c->deny_words;
    return 0;
}

// The rows of a call with a logits_filter_callback, for the workspace's cap_jobs rows (after ensure_ws; kept with the
// workspace: a call without a callback allocates nothing)
static void ensure_filter_rows(Context* c, whisper_state* s) {
    Workspace& w = s->ws;
    const size_t bytes = (size_t)w.cap_jobs * c->hp.n_vocab * sizeof(float);
    if (!w.frows) dalloc(w.frows, bytes);
    if (!w.h_frows) WM_CHECK(hipHostMalloc((void**)&w.h_frows, bytes, 0));
}

// The call's mask into the state's buffer, on its stream, before the first logits launch: nothing when the call has
// no mask, or when the buffer holds this key's words already. (After ensure_ws: the buffer exists.) 0 or -8.
static int deny_prepare(Context* c, whisper_state* s, const whisper_full_params& p) {
    Workspace& w = s->ws;
    Context::DenyKey key;
    key.nst = p.suppress_nst;
    key.has_regex = p.suppress_regex != nullptr;
    if (p.suppress_regex) key.regex = p.suppress_regex;
    s->deny_on = key.on();
    if (!s->deny_on || (w.deny_held && w.deny_key == key)) return 0;
    std::vector<uint32_t> words;
    if (const int r = deny_lookup(c, p.suppress_nst, p.suppress_regex, &words)) return r;
    w.deny_held = false;
    WM_CHECK(hipMemcpyAsync(w.deny, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    WM_CHECK(hipStreamSynchronize(s->stream));  // (`words` goes out of scope; once per change of key)
    w.deny_key = key;
    w.deny_held = true;
    return 0;
}

// ---- whisper_full_params.grammar_rules (grammar.h) ---------------------------------------------------
static_assert(sizeof(whisper_grammar_element) == sizeof(GramElem) && offsetof(whisper_grammar_element, value) == offsetof(GramElem, value),
              "GramElem mirrors whisper_grammar_element");
int grammar_check(const whisper_full_params& p, GrammarRules& rules) {
    std::string err;
    const int r = grammar_compile((const GramElem* const*)p.grammar_rules, p.n_grammar_rules, p.i_start_rule, rules, &err);
    if (r) fprintf(stderr, "whisper_mi355x: grammar_rules refused: %s\n", err.c_str());
    return r;
}
const GramVocab& gram_vocab(Context* c) {
    std::lock_guard<std::mutex> lk(c->gram_mu);
    if (!c->gram_vocab_built) {
        gram_vocab_build(c->vocab.id_to_token, c->hp.n_vocab, c->vocab.token_eot, c->gram_vocab);
        c->gram_vocab_built = true;
    }
    return c->gram_vocab;
}

// the vocabulary's table on the device, built with the first grammar call of the context
static const GramTable& gram_table(Context* c) {
    const GramVocab& v = gram_vocab(c);
    std::lock_guard<std::mutex> lk(c->gram_mu);
    if (!c->gram_tab.off) {
        std::vector<uint32_t> val(v.eot);
        std::vector<int> rem(v.eot);
        for (int i = 0; i < v.eot; i++) {
            val[i] = v.tail[i].value;
            rem[i] = i >= (int)v.strs->size() || (*v.strs)[i].empty() ? kGramTokEmpty : v.tail[i].n_remain;
        }
        const void* src[4] = {v.off.data(), v.cps.data(), val.data(), rem.data()};
        const size_t bytes[4] = {v.off.size() * 4, std::max<size_t>(v.cps.size(), 1) * 4, std::max<size_t>(val.size(), 1) * 4,
                                 std::max<size_t>(rem.size(), 1) * 4};
        const size_t have[4] = {v.off.size() * 4, v.cps.size() * 4, val.size() * 4, rem.size() * 4};
        void* mem[4] = {nullptr, nullptr, nullptr, nullptr};  // published when all four are there
        try {
            for (int k = 0; k < 4; k++) {
                WM_CHECK(hipMalloc(&mem[k], bytes[k]));
                if (have[k]) WM_CHECK(hipMemcpy(mem[k], src[k], have[k], hipMemcpyHostToDevice));
            }
        } catch (...) {
            for (void* q : mem)
                if (q) hipFree(q);
            throw;
        }
        for (int k = 0; k < 4; k++) c->gram_tab_mem[k] = mem[k];
        c->gram_tab = GramTable{(const uint32_t*)c->gram_tab_mem[0], (const uint32_t*)c->gram_tab_mem[1],
                                (const uint32_t*)c->gram_tab_mem[2], (const int*)c->gram_tab_mem[3], v.eot, v.n_vocab};
    }
    return c->gram_tab;
}

void gram_dev_free(GramDev& d) {
    dfree(d.elems); dfree(d.rule_off); dfree(d.rows); dfree(d.over);
    if (d.h_rows) hipHostFree(d.h_rows);
    if (d.h_over) hipHostFree(d.h_over);
    d = GramDev();
}

void gram_dev_rules(GramDev& d, const GrammarRules& g, hipStream_t st) {
    d.host_masks.clear();
    if (g.elems.size() > d.cap_elems || g.rule_off.size() > d.cap_rules) {
        WM_CHECK(hipStreamSynchronize(st));  // (a launch of the last call may still read them)
        dfree(d.elems); dfree(d.rule_off);
        d.cap_elems = d.cap_rules = 0;
        dalloc(d.elems, g.elems.size() * sizeof(GramElem));
        dalloc(d.rule_off, g.rule_off.size() * sizeof(int));
        d.cap_elems = g.elems.size();
        d.cap_rules = g.rule_off.size();
    }
    WM_CHECK(hipMemcpyAsync(d.elems, g.elems.data(), g.elems.size() * sizeof(GramElem), hipMemcpyHostToDevice, st));
    WM_CHECK(hipMemcpyAsync(d.rule_off, g.rule_off.data(), g.rule_off.size() * sizeof(int), hipMemcpyHostToDevice, st));
    WM_CHECK(hipStreamSynchronize(st));  // (the caller's vectors may go; once per call)
}

// a grammar state as bytes: equal states, equal keys (the hash tables below)
static std::string gram_state_key(const Grammar& st) {
    std::string key((const char*)&st.partial.value, sizeof(st.partial.value));
    key.append((const char*)&st.partial.n_remain, sizeof(st.partial.n_remain));
    for (const GramStack& k : st.stacks) {
        const uint16_t n = (uint16_t)k.size();
        key.append((const char*)&n, sizeof(n));
        key.append((const char*)k.data(), k.size() * sizeof(uint16_t));
    }
    return key;
}

// a state's words from the host, through the table of the states this call already built
static const std::vector<uint32_t>& gram_host_mask(Context* c, GramDev& d, const GrammarRules& g, const Grammar& st) {
    std::string key = gram_state_key(st);
    auto it = d.host_masks.find(key);
    if (it == d.host_masks.end()) {
        if (d.host_masks.size() >= 256) d.host_masks.clear();
        it = d.host_masks.emplace(std::move(key), std::vector<uint32_t>(grammar_words(c->hp.n_vocab))).first;
        grammar_reject(g, gram_vocab(c), st, it->second.data());
    }
    return it->second;
}

void gram_masks(Context* c, GramDev& d, const GrammarRules& g, const Grammar* const* states, int n, uint32_t* gram,
                uint32_t* h_stage, int* flags, hipStream_t st, whisper_state* s) {
    if (n <= 0) return;
    const GramTable& tab = gram_table(c);
    const size_t W = grammar_words(c->hp.n_vocab);
    if (n > d.cap_rows) {
        WM_CHECK(hipStreamSynchronize(st));
        dfree(d.rows); dfree(d.over);
        if (d.h_rows) { WM_CHECK(hipHostFree(d.h_rows)); d.h_rows = nullptr; }
        if (d.h_over) { WM_CHECK(hipHostFree(d.h_over)); d.h_over = nullptr; }
        d.cap_rows = 0;
        dalloc(d.rows, (size_t)n * sizeof(GramRow));
        dalloc(d.over, (size_t)n * sizeof(unsigned));
        WM_CHECK(hipHostMalloc((void**)&d.h_rows, (size_t)n * sizeof(GramRow), 0));
        WM_CHECK(hipHostMalloc((void**)&d.h_over, (size_t)n * sizeof(unsigned), 0));
        d.cap_rows = n;
    }
    int n_dev = 0;
    std::unordered_map<std::string, int> first_row;  // of the rows the kernel takes, by state
    for (int r = 0; r < n; r++) {
        const Grammar& q = *states[r];
        GramRow& row = d.h_rows[r];
        bool fits = q.partial.n_remain == 0 && (int)q.stacks.size() <= kGramRowStacks;
        for (size_t k = 0; fits && k < q.stacks.size(); k++) fits = (int)q.stacks[k].size() <= kGramRowDepth;
        row.n_stacks = fits ? (int)q.stacks.size() : -1;
        row.allow_eot = q.allow_eot();
        row.same_as = r;
        if (!fits) continue;
        n_dev++;
        row.same_as = first_row.emplace(gram_state_key(q), r).first->second;  // (the first row with this state, or r)
        for (size_t k = 0; k < q.stacks.size(); k++) {
            row.depth[k] = (uint8_t)q.stacks[k].size();
            std::copy(q.stacks[k].begin(), q.stacks[k].end(), row.stk[k]);
        }
    }
    if (n_dev > 0) {
        WM_CHECK(hipMemcpyAsync(d.rows, d.h_rows, (size_t)n * sizeof(GramRow), hipMemcpyHostToDevice, st));
        WM_CHECK(hipMemsetAsync(d.over, 0, (size_t)n * sizeof(unsigned), st));
        {
            KT kt(s, K_GRAMMAR, (double)n_dev * tab.eot * 8, st, s != nullptr);
            launch_grammar_reject(tab, d.elems, d.rule_off, d.rows, n, gram, d.over, st);
        }
        WM_CHECK(hipMemcpyAsync(d.h_over, d.over, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        WM_CHECK(hipStreamSynchronize(st));  // the one extra synchronisation of a grammar step
    }
    for (int r = 0; r < n; r++) {
        const bool host_only = d.h_rows[r].n_stacks < 0;
        const bool flagged = !host_only && d.h_over[d.h_rows[r].same_as] != 0;
        if (flags) flags[r] = host_only ? 2 : flagged ? 1 : 0;
        (host_only ? d.rows_host : flagged ? d.rows_patched : d.rows_device)++;
        if (!host_only && !flagged) continue;
        const std::vector<uint32_t>& words = gram_host_mask(c, d, g, *states[r]);
        memcpy(h_stage + (size_t)r * W, words.data(), W * sizeof(uint32_t));
        WM_CHECK(hipMemcpyAsync(gram + (size_t)r * W, h_stage + (size_t)r * W, W * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
}

static int full_batch_one(Context* c, whisper_state* s, const whisper_full_params& p, const float* const* pcm, const int* n,
                          int n_jobs, bool on_device, const FullOpts& o, bool single_api) {
    WM_CHECK(hipSetDevice(c->device));
    Sched S;
    S.c = c; S.s = s; S.p = p; S.o = o; S.single_api = single_api;
    if (const int r = check_args(S, n_jobs)) return r;
    s->deny_on = false;
    // a pattern that does not compile ends the call before anything is encoded (the mask is cached for deny_prepare)
    if (p.suppress_nst || p.suppress_regex)
        if (const int r = deny_lookup(c, p.suppress_nst, p.suppress_regex, nullptr)) return r;
    // a malformed or left-recursive grammar ends the call before anything is encoded
    s->gram_on = false;
    if (const int r = grammar_check(p, s->gram_rules)) return r;
    s->gram_on = s->gram_rules.on();
    s->gram_penalty = p.grammar_penalty;
    S.gram0.init(s->gram_rules);
    s->filter_on = p.logits_filter_callback != nullptr;
    s->tdrz_on = p.tdrz_enable;
    ensure_expanded(c, s->stream);  // quantized files: before anything is captured
    S.hyps.resize(S.beam_k > 0 || S.sample_n > 1 ? n_jobs : 0);
    s->beam_info.assign(n_jobs, {});
    s->cand_info.assign(n_jobs, {});
    s->mode = StepMode{};
    s->results.assign(n_jobs, {});
    s->lang_ids.assign(n_jobs, 0);
    s->decisions.assign(n_jobs, {});
    s->align_info.assign(n_jobs, {});
    s->align_ms = s->tokts_ms = 0;
    s->vad_ms = 0;
    s->vad_maps.clear();
    s->decoded_tokens = 0;
    // vad: the clips are filtered on the device first, and the call goes on with the filtered clips (a refused model
    // ends the call before anything is encoded)
    if (p.vad) {
        if (const int r = vad_filter(S, pcm, n, n_jobs, on_device)) return r;
        pcm = S.vad_pcm.data();
        n = S.vad_n.data();
        on_device = true;
    }
    {
        ScopeTimer timed{S.t_mel};
        // beams of one clip share its cross K/V cache slot: beam_k > 1 runs in the cache form, with a self slot per beam
        // (best_of candidates take self slots too, but the call keeps the cross form that it takes with best_of = 1)
        s->direct = S.beam_k > 1 ? false : pick_direct(c, n_jobs);
        ensure_ws(c, s, n_jobs * std::max(1, std::max(S.beam_k, S.sample_n)), n_jobs);
        if (!single_api) s->audio_ctx = 0;  // every clip of the batch API starts as on a fresh state (apply_audio_ctx)
        if (const int r = deny_prepare(c, s, p)) return r;
        if (s->filter_on) ensure_filter_rows(c, s);
        if (s->gram_on) gram_dev_rules(s->ws.gd, s->gram_rules, s->stream);
        compute_mel(c, s, pcm, n, n_jobs, on_device);
    }
    if (p.token_timestamps) { ScopeTimer timed{S.t_tokts}; compute_energy(s, pcm, n, n_jobs, on_device); }
    if (p.temperature_inc > 0.0f && o.fixed_tokens <= 0)
        for (float t = p.temperature; t < 1.0f + 1e-6f; t += p.temperature_inc) S.temps.push_back(t);
    if (S.temps.empty()) S.temps.push_back(p.temperature);
    S.n_max_steps = o.fixed_tokens > 0 ? o.fixed_tokens : c->hp.n_text_ctx / 2 - 4;
    if (const int r = make_jobs(S, n, n_jobs)) return r;
    if (!S.need_lang)
        if (const int r = apply_audio_ctx(S)) return r;
    static int (*const kPasses[])(Sched&) = {pass_encode, pass_lang, pass_prefill, pass_decode, pass_beam, pass_sample, pass_token_times, pass_new_segment};
    int rc = 0;
    while (rc == 0 && !S.aborted && std::any_of(S.jobs.begin(), S.jobs.end(), [](const Job& j) { return j.phase != PH_DONE; }))
        for (auto pass : kPasses)
            if ((rc = pass(S)) != 0 || S.aborted) break;
    if (rc) return rc;
    if (const int r = apply_audio_ctx(S)) return r;  // (if no pass did: no clip had a window to encode, or a stop came first)
    if (o.stopped) *o.stopped = S.aborted;
    publish(S);
    return 0;
}

// ---- whisper_full_parallel (parallel.h) ------------------------------------------------------------------
// The cuts moved to the quietest 20 ms near them: the RMS of the candidate windows of every interior cut comes from the
// device pass of whisper_mi355x_find_silence_boundaries, one short clip per cut (a window's RMS does not depend on the
// windows around it, so only the candidates' samples are read, and from host PCM only they are uploaded), and 4 bytes per
// window come back; the choice is the host's (parallel_snap_pick).
static int snap_cuts(Context* c, const float* pcm, int n_samples, bool on_device, int snap, std::vector<int>& cuts) {
    const int nc = (int)cuts.size() - 1;
    std::vector<SnapRange> rg(nc);
    std::vector<const float*> ptr(nc);
    std::vector<int> len(nc), counts(nc);
    int stride = 1;
    for (int k = 0; k < nc; k++) {
        rg[k] = parallel_snap_range(n_samples, cuts[k + 1], snap);
        ptr[k] = pcm + (size_t)rg[k].w_lo * kParWindow;
        len[k] = rg[k].n_w * kParWindow;
        stride = std::max(stride, rg[k].n_w);
    }
    std::vector<float> rms((size_t)nc * stride);
    if (whisper_mi355x_find_silence_boundaries(c->device, ptr.data(), len.data(), nc, kParRate, on_device, counts.data(), nullptr, 0,
                                               nullptr, rms.data(), stride) != 0)
        return WHISPER_MI355X_ERR_RUNTIME;
    for (int k = 0; k < nc; k++) cuts[k + 1] = parallel_snap_pick(rms.data() + (size_t)k * stride, rg[k], cuts[k + 1]);
    return 0;
}

int full_parallel(Context* c, whisper_state* s, const whisper_full_params& p, const float* pcm, int n_samples,
                  int n_processors, int snap_ms, bool on_device) {
    if (n_processors > kParallelMax) return -1;  // (capi.cpp has said why)
    const int n_per = n_processors > 1 ? parallel_n_per(n_samples, p.offset_ms, n_processors) : 0;
    if (n_processors <= 1 || n_per <= 0) {  // whisper_full (also when offset_ms leaves less than a sample per piece)
        s->par_cuts.assign(1, 0);
        return full_batch(c, s, p, &pcm, &n_samples, 1, on_device, FullOpts(), true);
    }
    WM_CHECK(hipSetDevice(c->device));
    std::vector<int> cuts = parallel_cuts(n_samples, p.offset_ms, n_processors);
    if (const int snap = parallel_snap(snap_ms, n_per); snap > 0)
        if (const int r = snap_cuts(c, pcm, n_samples, on_device, snap, cuts)) return r;
    std::vector<const float*> ptr(n_processors);
    std::vector<int> len(n_processors);
    for (int k = 0; k < n_processors; k++) {
        ptr[k] = pcm + cuts[k];
        len[k] = (k + 1 < n_processors ? cuts[k + 1] : n_samples) - cuts[k];
    }
    // beam search: every beam is a decoder row, so the pieces run in consecutive groups of 32 / beam_size jobs; the
    // single API's job exists in the first group only. (An error of a group ends the call: the state's carried prompt and
    // language are put back, and nothing of the call stays in the state.)
    const int beam_k = p.strategy == WHISPER_SAMPLING_BEAM_SEARCH ? std::max(1, p.beam_search.beam_size) : 1;
    const int group = beam_k > 1 && beam_k <= kBeamMax ? std::max(1, kBeamMaxRows / beam_k) : n_processors;
    const std::vector<int> past0 = s->prompt_past;
    const int lang0 = s->lang_id;
    std::vector<std::vector<Segment>> results(n_processors);
    std::vector<std::vector<whisper_mi355x_window_decision>> decisions(n_processors);
    whisper_state::AlignInfo align0;
    std::vector<whisper_state::BeamRec> beam0, cand0;
    std::vector<VadPiece> vad0;
    int lang_job0 = 0;
    double phase_ms[5] = {0, 0, 0, 0, 0}, align_ms = 0, tokts_ms = 0, vad_ms = 0;
    long decoded = 0;
    bool stopped = false;
    const auto undo = [&] {
        s->prompt_past = past0;
        s->lang_id = lang0;
        s->results.clear();
        s->decisions.clear();
    };
    for (int a = 0; a < n_processors && !stopped; a += group) {
        const int nj = std::min(group, n_processors - a);
        FullOpts o;
        o.pieces = true;
        o.stopped = &stopped;
        int rc = 0;
        try {
            rc = full_batch_one(c, s, p, ptr.data() + a, len.data() + a, nj, on_device, o, a == 0);
        } catch (...) {
            undo();
            throw;
        }
        if (rc) {
            undo();
            return rc;
        }
        for (int j = 0; j < nj; j++) {
            results[a + j] = std::move(s->results[j]);
            decisions[a + j] = std::move(s->decisions[j]);
        }
        if (a == 0) {
            lang_job0 = s->lang_ids[0];
            if (nj == n_processors) align0 = s->align_info[0];  // (a later group's alignment would overwrite its cost matrix)
            beam0 = std::move(s->beam_info[0]);
            cand0 = std::move(s->cand_info[0]);
            if (!s->vad_maps.empty()) vad0 = std::move(s->vad_maps[0]);
        }
        for (int k = 0; k < 5; k++) phase_ms[k] += s->phase_ms[k];
        align_ms += s->align_ms;
        tokts_ms += s->tokts_ms;
        vad_ms += s->vad_ms;
        decoded += s->decoded_tokens;
    }
    // The merge, in piece order, into results[0]: the only thing the whisper_full_* getters see. Piece 0's times are
    // absolute already (its offset_ms was in force, and its new-segment callback ran while it was decoded).
    s->results.assign(1, std::move(results[0]));
    s->decisions.assign(1, std::move(decisions[0]));
    s->lang_ids.assign(1, lang_job0);
    s->align_info.assign(1, align0);
    s->beam_info.assign(1, std::move(beam0));
    s->cand_info.assign(1, std::move(cand0));
    s->vad_maps.clear();
    if (p.vad) s->vad_maps.push_back(std::move(vad0));
    for (int k = 0; k < 5; k++) s->phase_ms[k] = phase_ms[k];
    s->align_ms = align_ms;
    s->tokts_ms = tokts_ms;
    s->vad_ms = vad_ms;
    s->decoded_tokens = decoded;
    std::vector<Segment>& out = s->results[0];
    for (int k = 1; k < n_processors; k++) {
        const int64_t shift = parallel_shift(cuts[k], p.offset_ms);
        parallel_merge_piece(out, results[k], shift, [&] {
            if (p.new_segment_callback) p.new_segment_callback(c->owner, s, 1, p.new_segment_callback_user_data);
        });
        for (whisper_mi355x_window_decision d : decisions[k]) {
            d.seek += (int)shift;
            s->decisions[0].push_back(d);
        }
    }
    s->par_cuts = cuts;
    return 0;
}

int full_batch(Context* c, whisper_state* s, const whisper_full_params& p, const float* const* pcm, const int* n,
               int n_jobs, bool on_device, const FullOpts& o, bool single_api) {
    if (single_api || n_jobs <= kPairMin) return full_batch_one(c, s, p, pcm, n, n_jobs, on_device, o, single_api);
    if (const int r = check_audio_ctx(c, p.audio_ctx)) return r;  // (before the halves start: one line, not one per half)
    if (p.suppress_nst || p.suppress_regex)
        if (const int r = deny_lookup(c, p.suppress_nst, p.suppress_regex, nullptr)) return r;
    {
        GrammarRules rules;
        if (const int r = grammar_check(p, rules)) return r;
    }
    WM_CHECK(hipSetDevice(c->device));
    if (p.vad && !vad_lookup(c, p.vad_model_path)) return -11;  // (one line, not one per half)
    if (!s->twin) s->twin = create_state(c);
    whisper_state* t = s->twin;
    t->ktime_mask = s->ktime_mask;
    const int na = (n_jobs + 1) / 2;
    int ra = 0, rb = 0;
    std::exception_ptr ea, eb;
    // the caller's abort callback need not be thread-safe: both halves reach it through one mutex
    whisper_full_params pp = p;
    struct AbortGate { std::mutex mu; ggml_abort_callback cb; void* ud; } gate{{}, p.abort_callback, p.abort_callback_user_data};
    if (p.abort_callback) {
        pp.abort_callback = [](void* u) -> bool {
            AbortGate* g = (AbortGate*)u;
            std::lock_guard<std::mutex> lk(g->mu);
            return g->cb(g->ud);
        };
        pp.abort_callback_user_data = &gate;
    }
    // ... nor the logits filter callback; both halves report the caller's state (the second half calls it from its own
    // thread: INTEGRATION.md)
    struct FilterGate { std::mutex mu; whisper_logits_filter_callback cb; void* ud; whisper_state* st; }
        fgate{{}, p.logits_filter_callback, p.logits_filter_callback_user_data, s};
    if (p.logits_filter_callback) {
        pp.logits_filter_callback = [](whisper_context* cx, whisper_state*, const whisper_token_data* tokens, int n_tokens,
                                       float* logits, void* u) {
            FilterGate* g = (FilterGate*)u;
            std::lock_guard<std::mutex> lk(g->mu);
            g->cb(cx, g->st, tokens, n_tokens, logits, g->ud);
        };
        pp.logits_filter_callback_user_data = &fgate;
    }
    // teacher forcing (a parity-test hook) by halves: each half sees its own jobs' forced rows, and the spot
    // jobs of the other half never match (-1); both write their own rows of the caller's spot_logits
    FullOpts oa = o, ob = o;
    std::vector<int> spot_a, spot_b;
    if (o.n_spot > 0 && o.spot) {
        for (int k = 0; k < o.n_spot; k++) {
            spot_a.push_back(o.spot[k] < na ? o.spot[k] : -1);
            spot_b.push_back(o.spot[k] >= na ? o.spot[k] - na : -1);
        }
        oa.spot = spot_a.data();
        ob.spot = spot_b.data();
    }
    if (o.forced) ob.forced = o.forced + (long)na * o.fixed_tokens;
    std::thread th([&] {
        try {
            rb = full_batch_one(c, t, pp, pcm + na, n + na, n_jobs - na, on_device, ob, false);
        } catch (...) {
            eb = std::current_exception();
        }
    });
    try {
        ra = full_batch_one(c, s, pp, pcm, n, na, on_device, oa, false);
    } catch (...) {
        ea = std::current_exception();
    }
    th.join();
    if (eb) recover_state(t);
    if (ea) std::rethrow_exception(ea);
    if (eb) std::rethrow_exception(eb);
    if (ra) return ra;
    if (rb) return rb;
    merge_twin(s, t, n_jobs - na);
    return 0;
}

}  // namespace wm
