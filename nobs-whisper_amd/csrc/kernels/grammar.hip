// The grammar's reject masks on the device (whisper_full_params.grammar_rules; kernels.h
// launch_grammar_reject): per row of a step, one thread per token id runs whisper.cpp's `accept` over the token's code
// points from the row's stack list and applies the acceptance test of csrc/grammar.cpp's grammar_reject; a wave
// assembles its 64 bits by ballot and writes two words of gram[row].
//
// The row's stacks are staged in LDS and read by every thread for its token's first code point (most tokens die there
// and write nothing). The stacks that survive go to the thread's own slice of LDS: two buffers of kGramTokStacks stacks
// of kGramTokDepth 16-bit positions, one read while the other is written (runtime-indexed private arrays would live
// in scratch memory). `advance` is a work list inside the buffer being written: a stack whose top is a rule reference
// is expanded in place for the rule's first alternate and appended for the others; a finished stack equal to an earlier
// one is dropped. A token whose simulation needs more stacks or depth than the slice has sets gram_over[row]: the
// host then takes the row's words from grammar_reject. The kernel never guesses.
#include "../common.h"
#include "../kernels.h"

namespace wm {

static constexpr int GT = 64;  // one wave per workgroup: 64 ids, two words
static constexpr int TS = kGramTokStacks, TD = kGramTokDepth;
static constexpr unsigned GE_END = 0, GE_ALT = 1, GE_RULE_REF = 2, GE_CHAR = 3, GE_CHAR_RNG_UPPER = 5, GE_CHAR_ALT = 6;
static constexpr int kAdvanceMaxSteps = 4096;  // (validated grammars terminate; a bound all the same)

struct TokBuf {
    uint16_t stk[2][TS][TD];
    uint8_t dep[2][TS];
};

__device__ __forceinline__ bool g_end(const uint2* __restrict__ e, int i) { return e[i].x == GE_END || e[i].x == GE_ALT; }

// the class at pos against code point c; *after = the position after the class
__device__ bool g_match_char(const uint2* __restrict__ e, int pos, uint32_t c, int* after) {
    const bool positive = e[pos].x == GE_CHAR;
    bool found = false;
    int i = pos;
    do {
        if (e[i + 1].x == GE_CHAR_RNG_UPPER) {
            found = found || (e[i].y <= c && c <= e[i + 1].y);
            i += 2;
        } else {
            found = found || e[i].y == c;
            i += 1;
        }
    } while (e[i].x == GE_CHAR_ALT);
    *after = i;
    return found == positive;
}

__device__ bool g_match_partial(const uint2* __restrict__ e, int pos, uint32_t value, int n_remain) {
    if (n_remain < 0 || (n_remain == 1 && value < 2)) return false;
    const bool positive = e[pos].x == GE_CHAR;
    uint32_t low = value << (n_remain * 6);
    const uint32_t high = low | ((1u << (n_remain * 6)) - 1u);
    if (low == 0) {
        if (n_remain == 2) low = 1u << 11;
        else if (n_remain == 3) low = 1u << 16;
    }
    bool hit = false;
    int i = pos;
    do {
        if (e[i + 1].x == GE_CHAR_RNG_UPPER) {
            hit = hit || (e[i].y <= high && low <= e[i + 1].y);
            i += 2;
        } else {
            hit = hit || (low <= e[i].y && e[i].y <= high);
            i += 1;
        }
    } while (e[i].x == GE_CHAR_ALT);
    return hit == positive;
}

// `advance` over the stacks [i0, nd) of the buffer being written (the ones before i0 are finished). Returns true when
// a bound was exceeded.
__device__ bool g_advance(const uint2* __restrict__ e, const int* __restrict__ rule_off, uint16_t (*dst)[TD], uint8_t* ddep,
                          int i0, int& nd) {
    int i = i0, steps = 0;
    while (i < nd) {
        const int d = ddep[i];
        if (d > 0 && e[dst[i][d - 1]].x == GE_RULE_REF) {
            if (++steps > kAdvanceMaxSteps) return true;
            const int top = dst[i][d - 1];
            const int first = rule_off[e[top].y];
            int db = d - 1;  // the stack without its top, then the reference's successor unless the sequence ends there
            if (!g_end(e, top + 1)) dst[i][db++] = (uint16_t)(top + 1);
            for (int p = first; e[p].x != GE_END; p++) {  // the rule's other alternates: appended
                if (e[p].x != GE_ALT) continue;
                if (nd >= TS) return true;
                for (int k = 0; k < db; k++) dst[nd][k] = dst[i][k];
                int dn = db;
                if (!g_end(e, p + 1)) {
                    if (dn >= TD) return true;
                    dst[nd][dn++] = (uint16_t)(p + 1);
                }
                ddep[nd++] = (uint8_t)dn;
            }
            if (!g_end(e, first)) {  // its first alternate: in place
                if (db >= TD) return true;
                dst[i][db++] = (uint16_t)first;
            }
            ddep[i] = (uint8_t)db;
            continue;  // (the new top may be a reference again)
        }
        bool dup = false;  // finished: dropped when an earlier finished stack equals it
        for (int q = 0; q < i && !dup; q++) {
            if (ddep[q] != d) continue;
            bool same = true;
            for (int k = 0; k < d && same; k++) same = dst[q][k] == dst[i][k];
            dup = same;
        }
        if (dup) {
            nd--;
            if (i != nd) {
                for (int k = 0; k < ddep[nd]; k++) dst[i][k] = dst[nd][k];
                ddep[i] = ddep[nd];
            }
            continue;
        }
        i++;
    }
    return false;
}

__global__ void __launch_bounds__(GT) grammar_reject_kernel(GramTable t, const uint2* __restrict__ elems,
                                                            const int* __restrict__ rule_off, const GramRow* __restrict__ rows,
                                                            uint32_t* __restrict__ gram, unsigned* __restrict__ over) {
    const int row = blockIdx.y, tid = threadIdx.x;
    const int id = blockIdx.x * GT + tid;
    const int W = (t.n_vocab + 31) >> 5;
    __shared__ GramRow s_row;
    __shared__ TokBuf s_buf[GT];
    if (rows[row].n_stacks < 0 || rows[row].same_as != row) return;  // the host's row, or a copy of another row (uniform)
    static_assert(sizeof(GramRow) % 4 == 0, "GramRow is copied by words");
    for (int i = tid; i < (int)(sizeof(GramRow) / 4); i += GT) ((uint32_t*)&s_row)[i] = ((const uint32_t*)&rows[row])[i];
    __syncthreads();
    const int n_row = min(s_row.n_stacks, kGramRowStacks);
    bool reject = false;
    if (n_row > 0 && id == t.eot && id < t.n_vocab) reject = s_row.allow_eot == 0;
    if (n_row > 0 && id < t.eot) {
        const int rem = t.tail_rem[id];
        if (rem == kGramTokEmpty) {
            reject = false;  // the empty string is never penalised
        } else if (rem < 0) {
            reject = true;  // invalid UTF-8
        } else {
            TokBuf& B = s_buf[tid];
            const uint16_t* src = &s_row.stk[0][0];
            const uint8_t* sdep = s_row.depth;
            int sstride = kGramRowDepth, nsrc = n_row, cur = 0;
            bool ovf = false;
            const uint32_t k1 = t.off[id + 1];
            for (uint32_t k = t.off[id]; k < k1 && nsrc > 0 && !ovf; k++) {
                const uint32_t c = t.cps[k];
                uint16_t(*dst)[TD] = B.stk[cur];
                uint8_t* ddep = B.dep[cur];
                int nd = 0;
                for (int j = 0; j < nsrc && !ovf; j++) {
                    const int d = min((int)sdep[j], sstride);
                    if (d == 0) continue;
                    const int top = src[j * sstride + d - 1];
                    int after;
                    if (!g_match_char(elems, top, c, &after)) continue;
                    if (nd >= TS || d > TD) { ovf = true; break; }
                    for (int q = 0; q < d - 1; q++) dst[nd][q] = src[j * sstride + q];
                    int dn = d - 1;
                    if (!g_end(elems, after)) dst[nd][dn++] = (uint16_t)after;
                    ddep[nd] = (uint8_t)dn;
                    const int i0 = nd++;
                    ovf = g_advance(elems, rule_off, dst, ddep, i0, nd);
                }
                src = &dst[0][0];
                sdep = ddep;
                sstride = TD;
                nsrc = nd;
                cur ^= 1;
            }
            if (ovf) {
                atomicOr(over + row, 1u);
            } else if (nsrc == 0) {
                reject = true;
            } else if (rem > 0) {  // the token ends inside a character: a stack whose top can still match it
                const uint32_t val = t.tail_val[id];
                bool ok = false;
                for (int j = 0; j < nsrc && !ok; j++) {
                    const int d = min((int)sdep[j], sstride);
                    ok = d > 0 && g_match_partial(elems, src[j * sstride + d - 1], val, rem);
                }
                reject = !ok;
            }
        }
    }
    const unsigned long long b = __ballot(reject);
    const int w0 = blockIdx.x * (GT / 32);
    if (tid == 0) {
        if (w0 < W) gram[(long)row * W + w0] = (uint32_t)b;
        if (w0 + 1 < W) gram[(long)row * W + w0 + 1] = (uint32_t)(b >> 32);
    }
}

// the words of the rows that share an earlier row's state
__global__ void grammar_copy_kernel(const GramRow* __restrict__ rows, uint32_t* __restrict__ gram, int W) {
    const int row = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    const int src = rows[row].same_as;
    if (rows[row].n_stacks < 0 || src == row || src < 0 || src > row || i >= W) return;
    gram[(long)row * W + i] = gram[(long)src * W + i];
}

void launch_grammar_reject(const GramTable& t, const GramElem* elems, const int* rule_off, const GramRow* rows, int n_rows,
                           uint32_t* gram, unsigned* over, hipStream_t st) {
    if (n_rows <= 0) return;
    static_assert(sizeof(GramElem) == sizeof(uint2), "elements are read as uint2 {type, value}");
    const int W = (t.n_vocab + 31) / 32;
    const dim3 grid((W + GT / 32 - 1) / (GT / 32), n_rows);
    grammar_reject_kernel<<<grid, GT, 0, st>>>(t, (const uint2*)elems, rule_off, rows, gram, over);
    grammar_copy_kernel<<<dim3((W + 255) / 256, n_rows), 256, 0, st>>>(rows, gram, W);
    WM_CHECK(hipGetLastError());
}

}  // namespace wm
