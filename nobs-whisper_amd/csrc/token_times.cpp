// Token times, host parts (token_times.h). No HIP in this file.
#include "token_times.h"

#include <algorithm>
#include <cmath>

namespace wm {

float tt_voice_length(const std::string& s) {
    float res = 0.0f;
    for (const char ch : s) {
        if (ch == ' ') res += 0.01f;
        else if (ch == ',') res += 2.00f;
        else if (ch == '.' || ch == '!' || ch == '?') res += 3.00f;
        else if (ch >= '0' && ch <= '9') res += 3.00f;
        else res += 1.00f;
    }
    return res;
}

int64_t tt_trunc(double x) {
    if (std::isnan(x)) return 0;
    if (x >= 9223372036854775807.0) return INT64_MAX;
    if (x <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)x;
}

static const std::string& tok_str(const std::vector<std::string>& vocab, int id) {
    static const std::string none;
    return id >= 0 && id < (int)vocab.size() ? vocab[id] : none;
}

void tt_phase1(std::vector<TtTok>& tok, int64_t t0, int64_t t1, TtState& st, int token_beg, float thold_pt, float thold_ptsum,
               const std::vector<std::string>& vocab) {
    const int n = (int)tok.size();
    if (n == 0) return;
    if (n == 1) {
        tok[0].t0 = t0;
        tok[0].t1 = t1;
        return;
    }
    for (int j = 0; j < n; j++) {
        TtTok& t = tok[j];
        if (j == 0) {
            if (t.id == token_beg) {
                tok[0].t0 = t0;
                tok[0].t1 = t0;
                tok[1].t0 = t0;
                st.t_beg = t0;
                st.t_last = t0;
                st.tid_last = token_beg;
            } else {
                tok[0].t0 = st.t_last;
            }
        }
        t.vlen = tt_voice_length(tok_str(vocab, t.id));
        const int64_t tt = st.t_beg + 2 * ((int64_t)t.tid - token_beg);
        if (t.pt > thold_pt && t.ptsum > thold_ptsum && t.tid > st.tid_last && tt <= t1) {
            if (j > 0) tok[j - 1].t1 = tt;
            t.t0 = tt;
            st.tid_last = t.tid;
        }
    }
    tok[n - 2].t1 = t1;
    tok[n - 1].t0 = t1;
    tok[n - 1].t1 = t1;
    st.t_last = t1;

    // unknown intervals: spread by voice length
    int p0 = 0, p1 = 0;
    while (true) {
        while (p1 < n && tok[p1].t1 < 0) p1++;
        if (p1 >= n) p1--;
        if (p1 > p0) {
            double psum = 0.0;
            for (int j = p0; j <= p1; j++) psum += tok[j].vlen;
            const double dt = (double)(tok[p1].t1 - tok[p0].t0);
            for (int j = p0 + 1; j <= p1; j++) {
                const double ct = (double)tok[j - 1].t0 + dt * tok[j - 1].vlen / psum;
                tok[j - 1].t1 = tt_trunc(ct);
                tok[j].t0 = tok[j - 1].t1;
            }
        }
        p1++;
        p0 = p1;
        if (p1 >= n) break;
    }

    for (int j = 0; j < n - 1; j++) {
        if (tok[j].t1 < 0) tok[j + 1].t0 = tok[j].t1;
        if (j > 0 && tok[j - 1].t1 > tok[j].t0) {
            tok[j].t0 = tok[j - 1].t1;
            tok[j].t1 = std::max(tok[j].t0, tok[j].t1);
        }
    }
}

std::vector<TtPiece> tt_wrap(const std::vector<TtTok>& tok, int64_t t0, int64_t t1, int max_len, bool split_on_word,
                             int token_eot, const std::vector<std::string>& vocab) {
    std::vector<TtPiece> out;
    const int n = (int)tok.size();
    TtPiece cur;
    cur.i0 = 0;
    cur.t0 = t0;
    cur.t1 = t1;
    int acc = 0;
    for (int g = 0; g < n; g++) {
        if (tok[g].id >= token_eot) continue;
        const std::string& txt = tok_str(vocab, tok[g].id);
        const int len = (int)txt.size();
        const int i = g - cur.i0;  // index within the current piece
        if (acc + len > max_len && i > 0 && (!split_on_word || (len > 0 && txt[0] == ' '))) {
            cur.i1 = g;
            cur.t1 = tok[g].t0;
            out.push_back(cur);
            cur = TtPiece();
            cur.i0 = g;
            cur.t0 = tok[g].t0;
            cur.t1 = t1;
            acc = 0;
            // the walk restarts over the new piece: token g is its first (i = 0), so it is taken
        }
        acc += len;
        cur.text += txt;
    }
    cur.i1 = n;
    out.push_back(cur);
    return out;
}

}  // namespace wm
