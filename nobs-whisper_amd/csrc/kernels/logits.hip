// Device-side whisper_process_logits + whisper_sample_token(best=true).
//
// One 1024-thread workgroup per sequence reads its logits row (V = 51864..51866 f32) once, into
// from L2 and returns only a TokOut record (token id, p, plog, tid, pt, ptsum, no-speech prob),
// so the host never copies a [B, V] logits block per step. Rules, in whisper.cpp's order [ext]:
// temperature divide; suppress_blank (initial step: EOT and " "); <|notimestamps|>; optional
// no_timestamps; sot/nosp/solm/translate/transcribe/prev; the 100 language tokens; the deny mask of
// suppress_nst / suppress_regex (masked_deny; only when the call has one); timestamp
// pairing; max_initial_ts; monotonic timestamps; log-softmax; "sum(p(timestamps)) > max p(text)
// => timestamp"; when that rule did not fire, the grammar's penalty on the rejected tokens and the
// log-softmax again (gram_penalized; only when the call has a grammar); probs = exp(logprob). Greedy argmax keeps whisper's first-index tie break over
// the float probs. When temperature > 0 the probs row is also written for host-side sampling
// (std::discrete_distribution, exactly as whisper.cpp samples).
// A call with whisper_full_params.logits_filter_callback runs the rules as two launches with the host's
// callback between them, where upstream calls it: logits_stage_kernel applies the rules up to and including the language
// tokens (pre_logit) and writes the rows for the host; the prefiltered form of the kernels below (PF) applies the rest,
// from the deny mask on (post_logit), to the rows the callback left. With tdrz_enable the launches' VocabIds carry a solm
// id that matches no token.
// This file is compiled with -ffp-contract=off.
#include "../common.h"
#include "../kernels.h"

namespace wm {

static constexpr int LT = 1024;

// masked_logit in the two halves whisper_full_params.logits_filter_callback sits between: pre_logit is
// what the callback's row has been through, post_logit what follows it. A masked entry is -inf and stays -inf, so
// masked_logit(x) = post_logit(pre_logit(x)) in every bit.
__device__ __forceinline__ float pre_logit(float x, int i, const SeqCtl& c, const VocabIds& v) {
    if (c.temperature > 0.0f) x = x / c.temperature;
    // text tokens (every special id is >= eot): only the blank rule reaches them
    if (i < v.eot) {
        if (c.suppress_blank && c.is_initial && i == v.space) return -INFINITY;
        return x;
    }
    if (c.suppress_blank && c.is_initial && (i == v.eot || i == v.space)) return -INFINITY;
    if (i == v.not_) return -INFINITY;
    if (c.no_timestamps && i >= v.beg) return -INFINITY;
    if (i == v.sot || i == v.nosp || i == v.solm || i == v.translate || i == v.transcribe || i == v.prev) return -INFINITY;
    if (i > v.sot && i <= v.sot + v.n_lang) return -INFINITY;
    return x;
}
__device__ __forceinline__ float post_logit(float x, int i, const SeqCtl& c, const VocabIds& v) {
    // text tokens: only the timestamp-pairing rule reaches them
    if (i < v.eot) {
        if (c.last_ts && !c.penult_ts) return -INFINITY;
        return x;
    }
    if (c.suppress_eot && i == v.eot) return -INFINITY;
    if (c.last_ts) {
        if (c.penult_ts) { if (i >= v.beg) return -INFINITY; }
        else if (i < v.eot) return -INFINITY;
    }
    if (c.is_initial && c.tid0_initial >= 0 && i >= v.beg + c.tid0_initial + 1) return -INFINITY;
    if (c.has_ts && i >= v.beg && i < v.beg + c.seek_delta / 2) return -INFINITY;
    return x;
}
__device__ __forceinline__ float masked_logit(float x, int i, const SeqCtl& c, const VocabIds& v) {
    return post_logit(pre_logit(x, i, c, v), i, c, v);
}
// PF: the launch is the prefiltered form: its rows went through pre_logit (the stage kernel) and the caller's
// logits_filter_callback, so only post_logit is left. false: the launch is the one from before the callback existed.
template <bool PF>
__device__ __forceinline__ float rule_logit(float x, int i, const SeqCtl& c, const VocabIds& v) {
    if constexpr (PF) return post_logit(x, i, c, v);
    else return masked_logit(x, i, c, v);
}

// DM: the deny mask of suppress_nst / suppress_regex: bit i & 31 of word i >> 5 set = token i is
// denied, whatever the other rules say. 0: no mask (deny is not read: the code of a launch without one is what it
// was before the mask existed), 1: deny is the device buffer, read through the cache, 2: deny is the workgroup's
// copy in LDS. i < n_vocab.
template <int DM, bool PF = false>
__device__ __forceinline__ float masked_deny(float x, int i, const SeqCtl& c, const VocabIds& v, const uint32_t* deny) {
    if constexpr (DM != 0) {
        if ((deny[i >> 5] >> (i & 31)) & 1u) return -INFINITY;
    }
    return rule_logit<PF>(x, i, c, v);
}

// GM: the grammar's reject mask (whisper_full_params.grammar_rules): gram = the row's words, bit i & 31 of
// word i >> 5 set = token i <= eot loses `penalty` from its filtered logit (-inf stays -inf), after the timestamp rule
// and only when that rule did not mask the text tokens (the callers test mask_text). 0: no grammar (gram is not read:
// the code of a launch without one is what it was before the rule existed), 1: the device words, read through the cache.
template <int GM>
__device__ __forceinline__ float gram_penalized(float x, int i, const VocabIds& v, const uint32_t* gram, float penalty) {
    if constexpr (GM != 0) {
        if (i <= v.eot && ((gram[i >> 5] >> (i & 31)) & 1u)) return x - penalty;
    }
    return x;
}

// Reductions over a workgroup of NW waves (sh: NW elements): a butterfly within the wave, then every thread folds
// the NW wave results in wave order. Each begins with a barrier, so sh can be reused from one call to the next.
template <int NW>
__device__ float blk_max(float x, float* sh) {
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    float r = sh[0];
    for (int i = 1; i < NW; i++) r = fmaxf(r, sh[i]);
    return r;
}
template <int NW, typename T>  // float or double
__device__ T blk_sum(T x, T* sh) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    T r = 0;
    for (int i = 0; i < NW; i++) r += sh[i];
    return r;
}
// argmax with first-index tie break: (value larger) or (equal and index smaller)
__device__ __forceinline__ void argmax_pair(float& v, int& ix, float ov, int oi) {
    if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
}
template <int NW>
__device__ void blk_argmax(float& v, int& ix, float* shv, int* shi) {
    for (int o = 32; o > 0; o >>= 1) argmax_pair(v, ix, __shfl_xor(v, o), __shfl_xor(ix, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = ix; }
    __syncthreads();
    v = shv[0]; ix = shi[0];
    for (int i = 1; i < NW; i++) argmax_pair(v, ix, shv[i], shi[i]);
}

// Per-element exponentials over the whole row use the hardware exp2 (__expf, a few ulp): the GPU's
// logits already differ from the CPU's by ~1e-3, so libm-accurate exp buys no parity there, and its
// ~20-instruction expansion per element made the kernel VALU-bound. The timestamp sum (<= 1501
// elements) uses expf: "sum p(timestamps) > max p(text)" is a threshold decision on that sum alone
// (the log-sum-exp of the row cancels out of it).
// The row is loaded once into registers (NPT values per thread, all loads issued back to back) and
// every pass works on registers: a row re-read per pass from L2 with one load in flight per wave
// made the kernel latency-bound (128 us per step at 128 rows). Per-thread accumulation runs over
// i = tid, tid + LT, ... in ascending order, as before (same bits).
static constexpr int NPT = 51;  // 51 * 1024 >= 51866 (largest Whisper vocabulary)
static constexpr int NPT_LDS = 36;  // values k < NPT_LDS of each thread live in LDS (144 KiB), the rest in VGPRs

// element k of this thread's row slice (compile-time k after unrolling: LDS or a register)
struct RowSlice {
    float* lds;
    float reg[NPT - NPT_LDS];
    __device__ __forceinline__ float get(int k) const { return k < NPT_LDS ? lds[k * LT + threadIdx.x] : reg[k - NPT_LDS]; }
    __device__ __forceinline__ void set(int k, float v) {
        if (k < NPT_LDS) lds[k * LT + threadIdx.x] = v;
        else reg[k - NPT_LDS] = v;
    }
};

// The deny mask in the 1024-thread kernels: the device words (DM 1), or DM 2: the workgroup's copy behind the row's
// LDS part. load() issues the copy's loads (before the row's, so they are in flight together), store() writes them to
// LDS and is followed by the caller's barrier. A thread owns ids tid + 1024 k: bit tid & 31 of the words
// (tid >> 5) + 32 k, so a wave reads two words per k (from LDS one broadcast read) and the test is one AND.
template <int DM>
struct DenyLane {
    static constexpr int NW = (NPT * LT / 32 + LT - 1) / LT;  // words per thread of the copy
    const uint32_t* words = nullptr;                          // what masked_deny reads
    const uint32_t* lane = nullptr;
    uint32_t bit = 0, stage[NW];
    __device__ __forceinline__ void load(const uint32_t* __restrict__ deny, float* s_row, int n) {
        if constexpr (DM == 0) return;
        words = deny;
        if constexpr (DM == 2) {
            words = (const uint32_t*)(s_row + NPT_LDS * LT);
#pragma unroll
            for (int j = 0; j < NW; j++) {
                const int w = threadIdx.x + j * LT;
                stage[j] = w < (n + 31) >> 5 ? deny[w] : 0u;
            }
        }
        lane = words + (threadIdx.x >> 5);
        bit = 1u << (threadIdx.x & 31);
    }
    __device__ __forceinline__ void store(float* s_row, int n) {
        if constexpr (DM == 2) {
            uint32_t* sd = (uint32_t*)(s_row + NPT_LDS * LT);
#pragma unroll
            for (int j = 0; j < NW; j++) {
                const int w = threadIdx.x + j * LT;
                if (w < (n + 31) >> 5) sd[w] = stage[j];
            }
        }
    }
    // id threadIdx.x + k * LT (< n_vocab) is denied
    __device__ __forceinline__ bool denied(int k) const {
        if constexpr (DM == 0) return false;
        else return (lane[k * (LT / 32)] & bit) != 0;
    }
};
static size_t row_lds_bytes(int dm, int n_vocab) {
    return (size_t)NPT_LDS * LT * sizeof(float) + (dm == 2 ? (size_t)((n_vocab + 31) / 32) * sizeof(uint32_t) : 0);
}

// The one-workgroup-per-row form, greedy (TOPK false: launch_logits; out[s], and the probs rows when want_probs)
// and for beam search (TOPK true: launch_logits_topk; probs is not read): the same passes up to the greedy record,
// which becomes candidate 0 (out[s * kTopkMax]); then candidate j = 1 .. topk - 1 is the block
// argmax of the same float probs after the earlier winners were struck from the row (set to -inf), i.e. the
// tokens with p > 0 in (p descending, id ascending) order. A text candidate carries the row's tid / pt / ptsum, a
// timestamp candidate tid = id and pt = p (as the greedy record does); when fewer than topk tokens have p > 0
// the remaining records have id = -1.
// PF (the prefiltered form): filt [n_seq][n_vocab] holds the rows after pre_logit and the caller's callback; the raw row
// is read only for the no-speech probability, the filtered one is then loaded over it.
// Row `row` of the launch into a thread's slice: the register part first, then the LDS part in batches of 12 loads in
// flight (a load -> LDS store pair per element would wait out one memory latency per element)
__device__ __forceinline__ void load_row(RowSlice& x, const float* __restrict__ L, int n) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = NPT_LDS; k < NPT; k++) {
        const int i = tid + k * LT;
        x.set(k, i < n ? L[i] : -INFINITY);
    }
#pragma unroll
    for (int k0 = 0; k0 < NPT_LDS; k0 += 12) {
        float t[12];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int i = tid + (k0 + k) * LT;
            t[k] = i < n ? L[i] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < 12; k++) x.set(k0 + k, t[k]);
    }
}
template <int DM, int GM, bool TOPK, bool PF>
__global__ void __launch_bounds__(LT) logits_kernel(const float* __restrict__ logits, long ld, const SeqCtl* __restrict__ ctl,
                                                    VocabIds v, TokOut* __restrict__ out, float* __restrict__ probs, int topk,
                                                    const uint32_t* __restrict__ deny, const uint32_t* __restrict__ gram,
                                                    float penalty, const float* __restrict__ filt) {
    const int s = blockIdx.x;
    const SeqCtl c = ctl[s];
    const float* R = logits + (long)s * ld;                   // the raw row (the no-speech probability)
    const float* L = PF ? filt + (long)s * v.n_vocab : R;     // the row the rules read
    constexpr int NW = LT / 64;
    const int n = v.n_vocab, tid = threadIdx.x;
    __shared__ float shf[NW];
    __shared__ int shi[NW];
    __shared__ double shd[NW];
    __shared__ TokOut s_top[2];  // TOPK: the greedy record; [1].tid / .pt: the row's tid / pt (a text candidate's)

    extern __shared__ float s_row[];  // [NPT_LDS][LT]
    RowSlice x{s_row};
    DenyLane<DM> dl;
    dl.load(deny, s_row, n);
    const uint32_t* dm = dl.words;
    if constexpr (PF) {
        if (c.want_nosp) load_row(x, R, n);
    } else {
        load_row(x, L, n);
    }
    float nosp_prob = 0.0f;
    if (c.want_nosp) {  // no-speech probability from the raw (unfiltered) logits
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < NPT; k++)
            if (tid + k * LT < n) mx = fmaxf(mx, x.get(k));
        mx = blk_max<NW>(mx, shf);
        float sm = 0.0f;
#pragma unroll
        for (int k = 0; k < NPT; k++)
            if (tid + k * LT < n) sm += __expf(x.get(k) - mx);
        sm = blk_sum<NW>(sm, shf);
        const float lse = logf(sm) + mx;
        nosp_prob = expf(R[v.nosp] - lse);
    }
    if constexpr (PF) load_row(x, L, n);  // (a thread overwrites its own slice only)
    // filtered logits, in place
    dl.store(s_row, n);
    if constexpr (DM == 2) __syncthreads();  // the mask's LDS copy
#pragma unroll
    for (int k = 0; k < NPT; k++) {
        const int i = tid + k * LT;
        if (i < n) x.set(k, dl.denied(k) ? -INFINITY : rule_logit<PF>(x.get(k), i, c, v));
    }
    // log-softmax of the filtered logits
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < NPT; k++) mx = fmaxf(mx, x.get(k));
    mx = blk_max<NW>(mx, shf);
    float sm = 0.0f;
#pragma unroll
    for (int k = 0; k < NPT; k++)
        if (x.get(k) > -INFINITY) sm += __expf(x.get(k) - mx);
    sm = blk_sum<NW>(sm, shf);
    float lse = logf(sm) + mx;
    // timestamp rule
    float mts = -INFINITY, mtext = -INFINITY;
#pragma unroll
    for (int k = 0; k < NPT; k++) {
        const int i = tid + k * LT;
        const float lp = x.get(k) > -INFINITY ? x.get(k) - lse : -INFINITY;
        if (i >= v.beg) mts = fmaxf(mts, lp); else mtext = fmaxf(mtext, lp);
    }
    mts = blk_max<NW>(mts, shf);
    mtext = blk_max<NW>(mtext, shf);
    float sts = 0.0f;
#pragma unroll
    for (int k = 0; k < NPT; k++) {
        const int i = tid + k * LT;
        if (i < v.beg) continue;
        const float lp = x.get(k) > -INFINITY ? x.get(k) - lse : -INFINITY;
        if (lp > -INFINITY) sts += expf(lp - mts);  // libm-accurate: this sum decides the timestamp rule
    }
    sts = blk_sum<NW>(sts, shf);
    const float ts_logprob = sts > 0.0f ? logf(sts) + mts : -INFINITY;
    const bool mask_text = ts_logprob > mtext;
    const uint32_t* grow = nullptr;  // the row's reject words when the grammar rule applies to it (uniform)
    if constexpr (GM != 0) {
        if (!mask_text) {
            // the grammar's penalty, then the log-softmax again with the first pass's expressions: everything below
            // (p, plog, pt, ptsum, the probs rows, the top-k rounds) is taken from the second one, as upstream does
            grow = gram + (long)s * ((n + 31) >> 5);
            const uint32_t* gl = grow + (tid >> 5);
            const uint32_t gbit = 1u << (tid & 31);
#pragma unroll
            for (int k = 0; k < NPT; k++) {
                const int i = tid + k * LT;
                if (i <= v.eot && (gl[k * (LT / 32)] & gbit) != 0) x.set(k, x.get(k) - penalty);
            }
            mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < NPT; k++) mx = fmaxf(mx, x.get(k));
            mx = blk_max<NW>(mx, shf);
            sm = 0.0f;
#pragma unroll
            for (int k = 0; k < NPT; k++)
                if (x.get(k) > -INFINITY) sm += __expf(x.get(k) - mx);
            sm = blk_sum<NW>(sm, shf);
            lse = logf(sm) + mx;
        }
    }
    // probs, argmax (all) and argmax / sum over timestamps
    float best = 0.0f, best_ts = 0.0f;
    int ibest = 0x7fffffff, its = 0x7fffffff;
    double sum_ts = 0.0;
#pragma unroll
    for (int k = 0; k < NPT; k++) {
        const int i = tid + k * LT;
        if (i >= n) continue;
        float xv = x.get(k);
        if (mask_text && i < v.beg) xv = -INFINITY;
        const float p = xv == -INFINITY ? 0.0f : __expf(xv - lse);
        if constexpr (!TOPK) {
            if (c.want_probs) {  // [seq][2][V]: probs, logprobs (host sampling at t > 0)
                probs[(long)s * 2 * n + i] = p;
                probs[(long)s * 2 * n + n + i] = xv == -INFINITY ? -INFINITY : xv - lse;
            }
        }
        if (p > best) { best = p; ibest = i; }
        if (i >= v.beg) {
            sum_ts += (double)p;
            if (p > best_ts) { best_ts = p; its = i; }
        }
    }
    blk_argmax<NW>(best, ibest, shf, shi);
    blk_argmax<NW>(best_ts, its, shf, shi);
    sum_ts = blk_sum<NW>(sum_ts, shd);
    if (tid == 0) {
        TokOut r;
        r.id = best > 0.0f ? ibest : 0;
        r.p = best;
        {
            float xv = masked_deny<DM, PF>(L[r.id], r.id, c, v, dm);
            if constexpr (GM != 0) { if (grow) xv = gram_penalized<GM>(xv, r.id, v, grow, penalty); }
            if (mask_text && r.id < v.beg) xv = -INFINITY;
            r.plog = xv > -INFINITY ? xv - lse : -INFINITY;
        }
        r.tid = best_ts > 0.0f ? its : 0;
        r.pt = (float)((double)best_ts / (sum_ts + 1e-10));
        r.ptsum = (float)sum_ts;
        if constexpr (TOPK) {
            s_top[1].tid = r.tid;
            s_top[1].pt = r.pt;
        }
        if (r.id >= v.beg) { r.tid = r.id; r.pt = r.p; }
        r.nosp_prob = nosp_prob;
        r.pad = 0.0f;
        out[TOPK ? (long)s * kTopkMax : s] = r;
        if constexpr (TOPK) s_top[0] = r;
    }
    if constexpr (TOPK) {
        // best / ibest are the block's in every thread: each round strikes the last winner from the row
        for (int j = 1; j < topk; j++) {
            const bool dead = !(best > 0.0f);  // no token with p > 0 is left (uniform)
            float bj = 0.0f;
            int ij = 0x7fffffff;
            if (!dead) {
#pragma unroll
                for (int k = 0; k < NPT; k++) {
                    const int i = tid + k * LT;
                    if (i == ibest) x.set(k, -INFINITY);
                    if (i >= n) continue;
                    float xv = x.get(k);
                    if (mask_text && i < v.beg) xv = -INFINITY;
                    const float p = xv == -INFINITY ? 0.0f : __expf(xv - lse);
                    if (p > bj) { bj = p; ij = i; }
                }
            }
            blk_argmax<NW>(bj, ij, shf, shi);  // (its first barrier also orders s_top against thread 0's reads below)
            if (tid == 0) {
                TokOut r = s_top[0];
                if (!(bj > 0.0f)) {
                    r.id = -1; r.tid = 0; r.p = 0.0f; r.plog = -INFINITY; r.pt = 0.0f;
                } else {
                    r.id = ij;
                    r.p = bj;
                    r.plog = masked_deny<DM, PF>(L[ij], ij, c, v, dm) - lse;  // p > 0: the filtered logit is finite
                    // (masked_deny a second time, on thread 0 once per round, not a temporary shared with the line
                    // above: through one the GM = 0 instantiations' register allocation changed)
                    if constexpr (GM != 0) {
                        if (grow) r.plog = gram_penalized<GM>(masked_deny<DM, PF>(L[ij], ij, c, v, dm), ij, v, grow, penalty) - lse;
                    }
                    if (ij >= v.beg) { r.tid = ij; r.pt = bj; }
                    else { r.tid = s_top[1].tid; r.pt = s_top[1].pt; }
                }
                out[(long)s * kTopkMax + j] = r;
            }
            best = bj;
            ibest = ij;
        }
    }
}

// ---- split form for few rows (decode steps of <= 16 clips: one 1024-thread workgroup per row leaves
// the chip idle and took 38 us per step at one clip) -------------------------------------------------
// Pass 1: KS workgroups per row, each over a chunk of the vocabulary, write per-chunk statistics of
// the filtered logits x: the max m over all tokens, over the timestamp tokens (m_ts) and over the text
// tokens (m_text), the argmax of all and of the timestamp tokens (lowest index on ties), and the sums
// s = sum exp(x - m), s_ts = sum_ts exp(x - m_ts) (and for no_speech the raw logits' max and sum).
// Pass 2: one workgroup per row combines them in chunk order: lse = log(sum_c s_c e^(m_c - M)) + M,
// the timestamp rule log(S_ts) + M_ts > M_text with S_ts = sum_c s_ts_c e^(m_ts_c - M_ts) (the
// log-softmax shift cancels out of it), the argmax of p = e^(x - lse) as the argmax of x, and
// sum_ts p = S_ts e^(M_ts - lse). The same decisions as logits_kernel; sums associate differently (last
// bits of p, plog, pt), and a near-tie of p under rounding resolves by x instead of by index.
// want_probs rows (sampled attempts) have pass 2 write the probs / logprobs rows as well.
static constexpr int KS = 16, LT2 = 256;
struct LogitRec {
    float m_r, s_r, m, s, m_ts, s_ts, m_text;
    int ix_all, ix_ts, pad;
};

size_t logits_rec_bytes(int n_seq) { return (size_t)std::max(1, n_seq) * KS * sizeof(LogitRec); }

// (DM 0 / 1 in the split form's 256-thread kernels: a chunk workgroup needs ~102 words of the mask once each, so
// they come through the cache)
template <int DM, bool PF>
__global__ void __launch_bounds__(LT2) logits_part_kernel(const float* __restrict__ logits, long ld,
                                                          const SeqCtl* __restrict__ ctl, VocabIds v,
                                                          LogitRec* __restrict__ rec, const uint32_t* __restrict__ dm,
                                                          const float* __restrict__ filt) {
    constexpr int NW = LT2 / 64, PER = 14;  // 14 * 256 * 16 >= 51866
    const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, n = v.n_vocab;
    const SeqCtl q = ctl[s];
    const float* R = logits + (long)s * ld;
    const float* L = PF ? filt + (long)s * n : R;
    const int cs = (n + KS - 1) / KS, i0 = c * cs, i1 = min(n, i0 + cs);
    __shared__ float shf[NW];
    __shared__ int shi[NW];
    float raw[PER];
    if (!PF || q.want_nosp) {  // (PF: the raw row serves the no-speech sums only)
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = i0 + tid + k * LT2;
            raw[k] = i < i1 ? R[i] : -INFINITY;
        }
    }
    uint32_t dw[DM ? PER : 1];  // the mask's words of this thread's ids, in flight with the row
    if constexpr (DM != 0) {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = i0 + tid + k * LT2;
            dw[k] = i < i1 ? dm[i >> 5] : 0u;
        }
    }
    LogitRec r;
    r.m_r = -INFINITY; r.s_r = 0.0f; r.pad = 0;
    if (q.want_nosp) {
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < PER; k++) mx = fmaxf(mx, raw[k]);
        mx = blk_max<NW>(mx, shf);
        float sm = 0.0f;
#pragma unroll
        for (int k = 0; k < PER; k++)
            if (i0 + tid + k * LT2 < i1) sm += __expf(raw[k] - mx);
        r.m_r = mx;
        r.s_r = blk_sum<NW>(sm, shf);
    }
    if constexpr (PF) {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = i0 + tid + k * LT2;
            raw[k] = i < i1 ? L[i] : -INFINITY;
        }
    }
    float m = -INFINITY, mts = -INFINITY, mtx = -INFINITY;
    int ix = 0x7fffffff, its = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = i0 + tid + k * LT2;
        bool denied = false;
        if constexpr (DM != 0) denied = (dw[k] >> (i & 31)) & 1u;
        const float x = i < i1 && !denied ? rule_logit<PF>(raw[k], i, q, v) : -INFINITY;
        raw[k] = x;
        if (x > -INFINITY) {
            argmax_pair(m, ix, x, i);
            if (i >= v.beg) argmax_pair(mts, its, x, i);
            else mtx = fmaxf(mtx, x);
        }
    }
    blk_argmax<NW>(m, ix, shf, shi);
    blk_argmax<NW>(mts, its, shf, shi);
    mtx = blk_max<NW>(mtx, shf);
    float sm = 0.0f, sts = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = i0 + tid + k * LT2;
        if (raw[k] > -INFINITY) {
            sm += __expf(raw[k] - m);
            if (i >= v.beg) sts += expf(raw[k] - mts);
        }
    }
    r.m = m; r.m_ts = mts; r.m_text = mtx; r.ix_all = ix; r.ix_ts = its;
    r.s = blk_sum<NW>(sm, shf);
    r.s_ts = blk_sum<NW>(sts, shf);
    if (tid == 0) rec[(long)s * KS + c] = r;
}

// Pass 2's combine of a row's KS chunk records, in chunk order, by one thread (thread 0 of either combine kernel):
// the greedy record, and what the kernels' other passes need.
struct RowRec {
    TokOut r;
    float lse;
    bool mask_text;
    int win;   // the winner's id, -1: no token has p > 0
    int tid;   // the row's tid / pt (a text candidate's)
    float pt;
};
// (L: the row the rules read, R: the raw row; one row unless the launch is the prefiltered form)
template <int DM, bool PF>
__device__ __forceinline__ RowRec combine_recs(const float* L, const float* R, int s, const SeqCtl& q, const VocabIds& v,
                                               const LogitRec* rec, const uint32_t* dm) {
    const LogitRec* C = rec + (long)s * KS;
    float M = -INFINITY, Mts = -INFINITY, Mtx = -INFINITY, Mr = -INFINITY;
    int ix = 0x7fffffff, its = 0x7fffffff;
    for (int c = 0; c < KS; c++) {
        argmax_pair(M, ix, C[c].m, C[c].ix_all);
        argmax_pair(Mts, its, C[c].m_ts, C[c].ix_ts);
        Mtx = fmaxf(Mtx, C[c].m_text);
        Mr = fmaxf(Mr, C[c].m_r);
    }
    float S = 0.0f, Sts = 0.0f, Sr = 0.0f;
    for (int c = 0; c < KS; c++) {
        if (C[c].m > -INFINITY) S += C[c].s * expf(C[c].m - M);
        if (C[c].m_ts > -INFINITY) Sts += C[c].s_ts * expf(C[c].m_ts - Mts);
        if (q.want_nosp && C[c].m_r > -INFINITY) Sr += C[c].s_r * expf(C[c].m_r - Mr);
    }
    RowRec o;
    const float lse = logf(S) + M;
    const float mts = Mts - lse, mtext = Mtx - lse;
    const float ts_logprob = Sts > 0.0f ? logf(Sts) + mts : -INFINITY;
    const bool mask_text = ts_logprob > mtext;
    TokOut r;
    const float xb = mask_text ? Mts : M;
    const int ib = mask_text ? its : ix;
    const float best = xb > -INFINITY ? __expf(xb - lse) : 0.0f;
    r.id = best > 0.0f ? ib : 0;
    r.p = best;
    {
        float xv = masked_deny<DM, PF>(L[r.id], r.id, q, v, dm);
        if (mask_text && r.id < v.beg) xv = -INFINITY;
        r.plog = xv > -INFINITY ? xv - lse : -INFINITY;
    }
    const float best_ts = Mts > -INFINITY ? __expf(Mts - lse) : 0.0f;
    const double sum_ts = Mts > -INFINITY ? (double)Sts * (double)expf(Mts - lse) : 0.0;
    r.tid = best_ts > 0.0f ? its : 0;
    r.pt = (float)((double)best_ts / (sum_ts + 1e-10));
    r.ptsum = (float)sum_ts;
    o.tid = r.tid;
    o.pt = r.pt;
    if (r.id >= v.beg) { r.tid = r.id; r.pt = r.p; }
    r.nosp_prob = q.want_nosp ? expf(R[v.nosp] - (logf(Sr) + Mr)) : 0.0f;
    r.pad = 0.0f;
    o.r = r;
    o.lse = lse;
    o.mask_text = mask_text;
    o.win = best > 0.0f ? ib : -1;
    return o;
}

template <int DM, bool PF>
__global__ void __launch_bounds__(LT2) logits_combine_kernel(const float* __restrict__ logits, long ld,
                                                             const SeqCtl* __restrict__ ctl, VocabIds v,
                                                             const LogitRec* __restrict__ rec, TokOut* __restrict__ out,
                                                             float* __restrict__ probs, const uint32_t* __restrict__ dm,
                                                             const float* __restrict__ filt) {
    const int s = blockIdx.x, tid = threadIdx.x, n = v.n_vocab;
    const SeqCtl q = ctl[s];
    const float* R = logits + (long)s * ld;
    const float* L = PF ? filt + (long)s * n : R;
    __shared__ float sh_lse;
    __shared__ int sh_mask;
    if (tid == 0) {
        const RowRec c = combine_recs<DM, PF>(L, R, s, q, v, rec, dm);
        out[s] = c.r;
        sh_lse = c.lse;
        sh_mask = c.mask_text;
    }
    if (!q.want_probs) return;
    __syncthreads();
    const float lse = sh_lse;
    const bool mask_text = sh_mask;
    for (int i = tid; i < n; i += LT2) {
        float xv = masked_deny<DM, PF>(L[i], i, q, v, dm);
        if (mask_text && i < v.beg) xv = -INFINITY;
        probs[(long)s * 2 * n + i] = xv == -INFINITY ? 0.0f : __expf(xv - lse);
        probs[(long)s * 2 * n + n + i] = xv == -INFINITY ? -INFINITY : xv - lse;
    }
}

// The split form's pass 2 for top-k rows (beam search): thread 0 combines the chunk records with combine_recs, as
// logits_combine_kernel does (one function, so candidate 0 is that kernel's record bit for bit), while the 1024
// threads hold the filtered row in LDS / registers as logits_kernel does. Candidate
// j > 0 is the block argmax of the filtered logits x (lowest index on ties; text tokens excluded when the
// timestamp rule fired) without the earlier winners, with p = e^(x - lse), plog = x - lse: the split form's own
// key (it orders by x where the one-workgroup form orders by the rounded p). A candidate whose p underflows
// to 0, and every one after it, has id = -1.
template <int DM, bool PF>
__global__ void __launch_bounds__(LT) logits_topk_combine_kernel(const float* __restrict__ logits, long ld,
                                                                 const SeqCtl* __restrict__ ctl, VocabIds v,
                                                                 const LogitRec* __restrict__ rec, TokOut* __restrict__ cand,
                                                                 int topk, const uint32_t* __restrict__ deny,
                                                                 const float* __restrict__ filt) {
    const int s = blockIdx.x, tid = threadIdx.x, n = v.n_vocab;
    const SeqCtl q = ctl[s];
    const float* R = logits + (long)s * ld;
    const float* L = PF ? filt + (long)s * n : R;
    constexpr int NW = LT / 64;
    __shared__ float shf[NW];
    __shared__ int shi[NW];
    __shared__ float sh_lse;
    __shared__ int sh_mask;
    __shared__ TokOut s_top[2];  // candidate 0; [1].tid / .pt: the row's tid / pt (a text candidate's)
    __shared__ int sh_win;       // the last winner (-1: no token with p > 0 is left)
    extern __shared__ float s_row[];  // [NPT_LDS][LT]
    RowSlice x{s_row};
    DenyLane<DM> dl;
    dl.load(deny, s_row, n);
    dl.store(s_row, n);
    const uint32_t* dm = dl.words;
    if constexpr (DM == 2) __syncthreads();  // the mask's LDS copy
#pragma unroll
    for (int k = NPT_LDS; k < NPT; k++) {
        const int i = tid + k * LT;
        x.set(k, i < n ? (dl.denied(k) ? -INFINITY : rule_logit<PF>(L[i], i, q, v)) : -INFINITY);
    }
#pragma unroll
    for (int k0 = 0; k0 < NPT_LDS; k0 += 12) {
        float t[12];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int i = tid + (k0 + k) * LT;
            t[k] = i < n ? L[i] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int i = tid + (k0 + k) * LT;
            x.set(k0 + k, i < n ? (dl.denied(k0 + k) ? -INFINITY : rule_logit<PF>(t[k], i, q, v)) : -INFINITY);
        }
    }
    if (tid == 0) {
        const RowRec c = combine_recs<DM, PF>(L, R, s, q, v, rec, dm);
        s_top[1].tid = c.tid;
        s_top[1].pt = c.pt;
        cand[(long)s * kTopkMax] = c.r;
        s_top[0] = c.r;
        sh_win = c.win;
        sh_lse = c.lse;
        sh_mask = c.mask_text;
    }
    __syncthreads();
    const float lse = sh_lse;
    const bool mask_text = sh_mask;
    int win = sh_win;
    for (int j = 1; j < topk; j++) {
        float bj = -INFINITY;
        int ij = 0x7fffffff;
        if (win >= 0) {
#pragma unroll
            for (int k = 0; k < NPT; k++) {
                const int i = tid + k * LT;
                if (i == win) x.set(k, -INFINITY);
                const float xv = x.get(k);
                if (i >= n || (mask_text && i < v.beg)) continue;
                if (xv > bj) { bj = xv; ij = i; }
            }
        }
        blk_argmax<NW>(bj, ij, shf, shi);
        const float p = bj > -INFINITY ? __expf(bj - lse) : 0.0f;
        if (tid == 0) {
            TokOut r = s_top[0];
            if (!(p > 0.0f)) {
                r.id = -1; r.tid = 0; r.p = 0.0f; r.plog = -INFINITY; r.pt = 0.0f;
            } else {
                r.id = ij;
                r.p = p;
                r.plog = bj - lse;
                if (ij >= v.beg) { r.tid = ij; r.pt = p; }
                else { r.tid = s_top[1].tid; r.pt = s_top[1].pt; }
            }
            cand[(long)s * kTopkMax + j] = r;
        }
        win = p > 0.0f ? ij : -1;
    }
}

// rows up to this count take the split form (16 chunk workgroups per row + a combine)
static const int kLogitsSplitMax = 16;

// the form the 1024-thread kernels read a mask in: 2 (LDS), or 1 (through the cache) under
// WHISPER_MI355X_DENY_GLOBAL=1 (the measurement of DESIGN.md §15; read per launch, a captured step keeps its form)
static int deny_mode(const uint32_t* deny) {
    if (!deny) return 0;
    const char* e = getenv("WHISPER_MI355X_DENY_GLOBAL");
    return e && atoi(e) > 0 ? 1 : 2;
}

// logits_kernel by (deny form, grammar on / off, greedy / top-k, plain / prefiltered)
#define WM_LOGITS_DM_GM_PF(dm, gm, TOPK, PF, ...)                                      \
    do {                                                                               \
        if (gm) {                                                                      \
            if (dm == 2) logits_kernel<2, 1, TOPK, PF> __VA_ARGS__;                    \
            else if (dm == 1) logits_kernel<1, 1, TOPK, PF> __VA_ARGS__;               \
            else logits_kernel<0, 1, TOPK, PF> __VA_ARGS__;                            \
        } else {                                                                       \
            if (dm == 2) logits_kernel<2, 0, TOPK, PF> __VA_ARGS__;                    \
            else if (dm == 1) logits_kernel<1, 0, TOPK, PF> __VA_ARGS__;               \
            else logits_kernel<0, 0, TOPK, PF> __VA_ARGS__;                            \
        }                                                                              \
    } while (0)
#define WM_LOGITS_DM_GM(dm, gm, TOPK, pf, ...)                                         \
    do {                                                                               \
        if (pf) WM_LOGITS_DM_GM_PF(dm, gm, TOPK, true, __VA_ARGS__);                   \
        else WM_LOGITS_DM_GM_PF(dm, gm, TOPK, false, __VA_ARGS__);                     \
    } while (0)
// a split-form kernel K<DM, PF> by (the launch has a mask, plain / prefiltered)
#define WM_LOGITS_SPLIT(K, deny, pf, ...)                                              \
    do {                                                                               \
        if (deny) { if (pf) K<1, true> __VA_ARGS__; else K<1, false> __VA_ARGS__; }    \
        else { if (pf) K<0, true> __VA_ARGS__; else K<0, false> __VA_ARGS__; }         \
    } while (0)

void launch_logits(const float* logits, long ld, const SeqCtl* ctl, int n_seq, const VocabIds& v, TokOut* out, float* probs,
                   void* rec, const uint32_t* deny, const uint32_t* gram, float gram_penalty, hipStream_t st,
                   const float* filtered) {
    if (n_seq <= 0) return;
    if (v.n_vocab > NPT * LT) WM_FAIL("vocabulary %d > %d", v.n_vocab, NPT * LT);
    const bool pf = filtered != nullptr;
    if (!gram && rec && n_seq <= kLogitsSplitMax && v.n_vocab <= 14 * LT2 * KS) {
        WM_LOGITS_SPLIT(logits_part_kernel, deny, pf, <<<dim3(KS, n_seq), LT2, 0, st>>>(logits, ld, ctl, v, (LogitRec*)rec, deny, filtered));
        WM_LOGITS_SPLIT(logits_combine_kernel, deny, pf,
                        <<<n_seq, LT2, 0, st>>>(logits, ld, ctl, v, (const LogitRec*)rec, out, probs, deny, filtered));
        return;
    }
    // (a grammar call always takes the one-workgroup-per-row form: the split form has no second softmax)
    const int dm = deny_mode(deny);
    const size_t lds = row_lds_bytes(dm, v.n_vocab);
    WM_LOGITS_DM_GM(dm, gram != nullptr, false, pf,
                    <<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, out, probs, 1, deny, gram, gram_penalty, filtered));
}

// Top-k after the rules: the form is chosen exactly as launch_logits chooses it for the same n_seq / rec / gram, so
// candidate 0 of a row is the TokOut launch_logits would return for it.
void launch_logits_topk(const float* logits, long ld, const SeqCtl* ctl, int n_seq, const VocabIds& v, TokOut* cand, int k,
                        void* rec, const uint32_t* deny, const uint32_t* gram, float gram_penalty, hipStream_t st,
                        const float* filtered) {
    if (n_seq <= 0) return;
    if (k < 1 || k > kTopkMax) WM_FAIL("top-k %d outside 1..%d", k, kTopkMax);
    if (v.n_vocab > NPT * LT) WM_FAIL("vocabulary %d > %d", v.n_vocab, NPT * LT);
    const bool pf = filtered != nullptr;
    const int dm = deny_mode(deny);
    const size_t lds = row_lds_bytes(dm, v.n_vocab);
    if (!gram && rec && n_seq <= kLogitsSplitMax && v.n_vocab <= 14 * LT2 * KS) {
        const LogitRec* R = (const LogitRec*)rec;
        WM_LOGITS_SPLIT(logits_part_kernel, deny, pf, <<<dim3(KS, n_seq), LT2, 0, st>>>(logits, ld, ctl, v, (LogitRec*)rec, deny, filtered));
        if (pf) {
            if (dm == 2) logits_topk_combine_kernel<2, true><<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, R, cand, k, deny, filtered);
            else if (dm == 1) logits_topk_combine_kernel<1, true><<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, R, cand, k, deny, filtered);
            else logits_topk_combine_kernel<0, true><<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, R, cand, k, nullptr, filtered);
        } else {
            if (dm == 2) logits_topk_combine_kernel<2, false><<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, R, cand, k, deny, nullptr);
            else if (dm == 1) logits_topk_combine_kernel<1, false><<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, R, cand, k, deny, nullptr);
            else logits_topk_combine_kernel<0, false><<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, R, cand, k, nullptr, nullptr);
        }
        return;
    }
    WM_LOGITS_DM_GM(dm, gram != nullptr, true, pf,
                    <<<n_seq, LT, lds, st>>>(logits, ld, ctl, v, cand, nullptr, k, deny, gram, gram_penalty, filtered));
}
#undef WM_LOGITS_SPLIT
#undef WM_LOGITS_DM_GM
#undef WM_LOGITS_DM_GM_PF

// ---- the stage kernel of whisper_full_params.logits_filter_callback -----------------------------------
// out[s][i] = pre_logit(logits[s][i]) for the n_seq rows of a step: the row the caller's callback gets. The raw row is
// left alone (the prefiltered launch reads its no-speech probability from it). HBM-bound at 8 bytes per element. The row
// stride of `out` is n_vocab, odd for 51865, so a row's first 16-byte boundary moves from row to row: a workgroup-uniform
// head of 0..3 scalar elements, 16-byte loads and stores from there, a scalar tail; all scalar when the input and the
// output row are not aligned alike (a caller's ld with another remainder).
static constexpr int ST = 256;  // threads; 4 elements each
__global__ void __launch_bounds__(ST) logits_stage_kernel(const float* __restrict__ logits, long ld,
                                                          const SeqCtl* __restrict__ ctl, VocabIds v, float* __restrict__ out) {
    const int s = blockIdx.y, n = v.n_vocab;
    const SeqCtl c = ctl[s];
    const float* L = logits + (long)s * ld;
    float* O = out + (long)s * n;
    const int mis_l = (int)(((uintptr_t)L >> 2) & 3), mis_o = (int)(((uintptr_t)O >> 2) & 3);
    const int t = blockIdx.x * ST + threadIdx.x;  // the thread's group of 4 along the row
    if (mis_l != mis_o) {
        for (int i = 4 * t; i < min(n, 4 * t + 4); i++) O[i] = pre_logit(L[i], i, c, v);
        return;
    }
    const int head = (4 - mis_l) & 3;  // elements before the first 16-byte boundary
    if (t == 0)
        for (int i = 0; i < min(head, n); i++) O[i] = pre_logit(L[i], i, c, v);
    const int i0 = head + 4 * t;
    if (i0 + 4 <= n) {
        const float4 x = *(const float4*)(L + i0);
        float4 y;
        y.x = pre_logit(x.x, i0, c, v);
        y.y = pre_logit(x.y, i0 + 1, c, v);
        y.z = pre_logit(x.z, i0 + 2, c, v);
        y.w = pre_logit(x.w, i0 + 3, c, v);
        *(float4*)(O + i0) = y;
    } else {
        for (int i = i0; i < n; i++) O[i] = pre_logit(L[i], i, c, v);
    }
}

void launch_logits_stage(const float* logits, long ld, const SeqCtl* ctl, int n_seq, const VocabIds& v, float* out,
                         hipStream_t st) {
    if (n_seq <= 0) return;
    if (((uintptr_t)logits | (uintptr_t)out) & 3) WM_FAIL("logits stage: rows not 4-byte aligned");
    const int groups = (v.n_vocab + 3) / 4 + 1;  // (+1: the head shifts the groups by up to 3 elements)
    logits_stage_kernel<<<dim3((groups + ST - 1) / ST, n_seq), ST, 0, st>>>(logits, ld, ctl, v, out);
}

// ---- device-side step advance (pipelined greedy decoding, engine.cpp decode_pipelined) -----------------------
// After a decode step's logits kernel, in stream order: row r's chosen token becomes its next input and its
// position advances (the layout of decoder_upload: tok | pos | slot | nkv_self | nkv_cross, ct entries each),
// its SeqCtl advances exactly as fill_ctl would rebuild it from the job after process_step appended the
// token (is_initial, last_ts = id >= beg, penult_ts = the previous last_ts or true after the first token;
// has_ts / seek_delta from a timestamp above beg), and the step's TokOut (and the persistent launch's error
// word) is copied to the ring slot the host reads while the next step runs.
__global__ void decode_advance_kernel(int n, int ct, int beg, const TokOut* __restrict__ tout, int* __restrict__ ints,
                                      SeqCtl* __restrict__ ctl, TokOut* __restrict__ ring, const unsigned* __restrict__ err,
                                      unsigned* __restrict__ ring_err) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0) *ring_err = err ? *err : 0u;
    if (r >= n) return;
    const TokOut o = tout[r];
    ring[r] = o;
    const int id = o.id;
    ints[r] = id;                       // tok
    const int pos = ints[ct + r] + 1;   // pos
    ints[ct + r] = pos;
    ints[3 * ct + r] = pos + 1;         // nkv_self
    SeqCtl c = ctl[r];
    c.penult_ts = c.is_initial ? 1 : c.last_ts;
    c.last_ts = id >= beg;
    c.is_initial = 0;
    if (id > beg) {
        c.has_ts = 1;
        c.seek_delta = 2 * (id - beg);
    }
    c.want_nosp = 0;
    ctl[r] = c;
}

void launch_decode_advance(int n, int ct, int beg, const TokOut* tout, int* ints, SeqCtl* ctl, TokOut* ring,
                           const unsigned* err, unsigned* ring_err, hipStream_t st) {
    decode_advance_kernel<<<(std::max(n, 1) + 127) / 128, 128, 0, st>>>(n, ct, beg, tout, ints, ctl, ring, err, ring_err);
    WM_CHECK(hipGetLastError());
}

}  // namespace wm
