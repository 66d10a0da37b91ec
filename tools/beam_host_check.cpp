// Stand-alone driver of the beam-search bookkeeping (nobs-whisper_amd/csrc/beam.h) for tests/test_beam_host.py:
// no GPU, no HIP. It reads a script of candidate lists (what the top-k kernel would return for every prefix the
// search can reach), runs one clip's beam search with beam_select / beam_copies / beam_schedule / beam_winner and
// the per-token rules of whisper_full (restated below from engine.cpp process_step / score_seq, as
// tests/beam_ref.py restates them), and prints every step's picks and self-cache copies and the final beams.
//
//   g++ -std=c++17 -O1 -g [-fsanitize=address,undefined] -I nobs-whisper_amd/csrc tools/beam_host_check.cpp
//       nobs-whisper_amd/csrc/beam_host.cpp -o beam_host_check && ./beam_host_check < script
//
// Script: "K n_prompt no_timestamps single_segment max_tokens n_max seek_end length_penalty entropy_thold eot beg",
// then "n_rows", then per row "len id.. n_cand (id plog)..".
#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

#include "beam.h"

using namespace wm;

struct Par {
    int K, n_prompt, no_timestamps, single_segment, max_tokens, n_max, seek_end;
    double length_penalty, entropy_thold;
    int eot, beg;
};
struct Tok { int id; float plog; };
struct Beam {
    std::vector<Tok> tokens;
    int result_len = 0;
    double sum_all = 0, avg = -INFINITY, entropy = 0, score = -INFINITY;
    int seek_delta = 3000;
    bool has_ts = false, failed = false, completed = false, ended = false;
    int step = 0;
    bool live() const { return !ended && !failed && !completed; }
    std::vector<int> ids() const {
        std::vector<int> r;
        for (const Tok& t : tokens) r.push_back(t.id);
        return r;
    }
};

static bool process_step(const Par& p, Beam& b, const BeamCand& c) {
    const int i = b.step;
    b.tokens.push_back({c.id, c.plog});
    b.sum_all += c.plog;
    if (c.id > p.beg) {
        const int sd_new = 2 * (c.id - p.beg);
        if (b.has_ts && b.seek_delta > sd_new && b.result_len < i) { b.failed = true; return false; }
        b.seek_delta = sd_new;
        b.result_len = i + 1;
        b.has_ts = true;
    }
    if (c.id == p.eot || (p.max_tokens > 0 && i >= p.max_tokens) || (b.has_ts && b.seek_delta + 10 >= p.seek_end)) {
        if (b.result_len == 0 && !p.no_timestamps) {
            if (b.seek_delta + 10 >= p.seek_end) b.result_len = i + 1;
            else { b.failed = true; return false; }
        }
        if (p.single_segment || p.no_timestamps) { b.result_len = i + 1; b.seek_delta = 3000; }
        b.completed = true;
        return false;
    }
    if (i == p.n_max - 1 && (b.result_len == 0 || b.seek_delta < 1500)) { b.failed = true; return false; }
    return i + 1 < p.n_max;
}

static void score_seq(const Par& p, Beam& b) {
    if (b.result_len == 0) return;
    double sum = 0;
    for (int i = 0; i < b.result_len; i++) sum += b.tokens[i].plog;
    b.avg = sum / b.result_len;
    double pen = b.result_len;
    if (p.length_penalty > 0) pen = pow((5.0 + pen) / 6.0, p.length_penalty);
    b.score = sum / pen;
    std::map<int, int> counts;
    int cnt = 0;
    for (int i = std::max(0, b.result_len - 32); i < b.result_len; i++) { counts[b.tokens[i].id]++; cnt++; }
    b.entropy = 0;
    for (auto& kv : counts) { const double q = kv.second / (double)cnt; b.entropy -= q * log(q); }
}

int main() {
    Par p;
    if (scanf("%d %d %d %d %d %d %d %lf %lf %d %d", &p.K, &p.n_prompt, &p.no_timestamps, &p.single_segment, &p.max_tokens, &p.n_max,
              &p.seek_end, &p.length_penalty, &p.entropy_thold, &p.eot, &p.beg) != 11 || p.K < 1 || p.K > kBeamMax)
        return 2;
    int n_rows = 0;
    if (scanf("%d", &n_rows) != 1) return 2;
    std::map<std::vector<int>, std::vector<BeamCand>> script;
    for (int r = 0; r < n_rows; r++) {
        int len = 0, nc = 0;
        if (scanf("%d", &len) != 1) return 2;
        std::vector<int> prefix(len);
        for (int& t : prefix)
            if (scanf("%d", &t) != 1) return 2;
        if (scanf("%d", &nc) != 1 || nc > p.K) return 2;
        std::vector<BeamCand> cs(p.K, BeamCand{-1, 0, 0.0f, -INFINITY, 0.0f, 0.0f});
        for (int q = 0; q < nc; q++) {
            double plog;
            if (scanf("%d %lf", &cs[q].id, &plog) != 2) return 2;
            cs[q].plog = (float)plog;
            cs[q].p = 1.0f;  // (only p > 0 matters to the bookkeeping)
        }
        script[prefix] = cs;
    }
    const int K = p.K;
    std::vector<Beam> beams(K);
    std::vector<std::vector<int>> held(K);
    std::vector<int> slots(K), prompt(p.n_prompt);
    for (int b = 0; b < K; b++) slots[b] = b;
    for (int i = 0; i < p.n_prompt; i++) prompt[i] = -1 - i;  // (any ids: every beam shares them)
    held[0] = prompt;
    const long upr = 2 * 2 * 2 * 8;  // L = 2, H = 2
    auto reparent = [&](const std::vector<int>& rows, const std::vector<int>& positions, bool first, int step) -> bool {
        std::vector<BeamCand> cands;
        std::vector<double> sums;
        for (int r : rows) {
            auto it = script.find(first ? std::vector<int>() : beams[r].ids());
            if (it == script.end()) { printf("missing prefix\n"); return false; }
            cands.insert(cands.end(), it->second.begin(), it->second.end());
            sums.push_back(first ? 0.0 : beams[r].sum_all);
        }
        const std::vector<BeamPick> picks = beam_select(rows, sums, cands.data(), K, positions);
        std::vector<KvCopy> copies = beam_copies(picks, held, slots);
        const long staged = beam_schedule(copies, upr);
        printf("step %d picks", step);
        for (const BeamPick& k : picks) printf(" %d %d %d", k.beam, k.parent, k.rank);
        printf("\n");
        long off = 0;
        for (const KvCopy& c : copies) {
            printf("copy %d %d %d %d %d\n", c.dst_slot, c.src_slot, c.row0, c.row1, c.mode);
            if (c.mode) {
                if (c.stage_off != off) { printf("bad staging offset\n"); return false; }
                off += (long)(c.row1 - c.row0) * upr;
            }
        }
        if (off != staged) { printf("bad staging size\n"); return false; }
        const std::vector<Beam> old = beams;
        for (const BeamPick& k : picks) {
            if (k.parent < 0) { beams[k.beam].failed = true; continue; }
            Beam nb = old[k.parent];
            if (!first) nb.step++;
            size_t r = 0;
            while (rows[r] != k.parent) r++;
            nb.ended = !process_step(p, nb, cands[r * K + k.rank]);
            beams[k.beam] = nb;
        }
        return true;
    };
    std::vector<int> all;
    for (int b = 0; b < K; b++) all.push_back(b);
    int step = 0;
    if (!reparent({0}, all, true, step++)) return 1;
    for (;;) {
        std::vector<int> live;
        for (int b = 0; b < K; b++)
            if (beams[b].live()) live.push_back(b);
        if (live.empty()) break;
        for (int b : live) held[b].push_back(beams[b].tokens.back().id);
        if (!reparent(live, live, false, step++)) return 1;
    }
    std::vector<double> score(K);
    std::vector<char> failed(K);
    for (int b = 0; b < K; b++) {
        Beam& bm = beams[b];
        printf("beam %d flags %d sum %.9g tokens", b, (bm.completed ? 1 : 0) | (bm.failed ? 2 : 0), bm.sum_all);
        for (const Tok& t : bm.tokens) printf(" %d", t.id);
        printf("\n");
        if (!bm.failed) {
            bm.tokens.resize(bm.result_len);
            score_seq(p, bm);
            if (bm.result_len > 32 && bm.entropy < p.entropy_thold) bm.failed = true;
        }
        score[b] = bm.score;
        failed[b] = bm.failed;
    }
    printf("winner %d\n", beam_winner(score, failed));
    return 0;
}
