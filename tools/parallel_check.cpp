// Host-only driver of nobs-whisper_amd/csrc/parallel.{h,cpp} (whisper_full_parallel's split, snap and merge rules) for
// tests/test_parallel_host.py: builds with a plain C++ compiler, reads cases on stdin, prints integers.
//   cuts  n_samples offset_ms n_processors
//   snap  n_samples offset_ms n_processors snap_ms n_win rms[0] .. rms[n_win - 1]     (rms of every window of the clip)
//   merge offset_ms n_pieces cut[0] .. ; per piece: n_seg; per segment: t0 t1 n_tok; per token: t0 t1 t_dtw
// Output, one line per case: the cuts; the snapped cuts; per merged segment "t0 t1 n_tok (t0 t1 t_dtw)*" joined by " | ".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "parallel.h"

using namespace wm;

struct Tok { int64_t t0, t1, t_dtw; };
struct Seg { int64_t t0, t1; std::vector<Tok> tokens; };

static void print_cuts(const std::vector<int>& c) {
    for (size_t k = 0; k < c.size(); k++) printf(k ? " %d" : "%d", c[k]);
    printf("\n");
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "cuts") {
            int n, off, np;
            std::cin >> n >> off >> np;
            print_cuts(parallel_cuts(n, off, np));
        } else if (cmd == "snap") {
            int n, off, np, snap_ms, n_win;
            std::cin >> n >> off >> np >> snap_ms >> n_win;
            std::vector<float> rms(n_win);
            for (float& r : rms) std::cin >> r;
            std::vector<int> cuts = parallel_cuts(n, off, np);
            const int snap = parallel_snap(snap_ms, parallel_n_per(n, off, np));
            for (int k = 1; k < np && snap > 0; k++) {  // as engine.cpp snap_cuts: the candidates' RMS values only
                const SnapRange r = parallel_snap_range(n, cuts[k], snap);
                if (r.n_w > 0 && r.w_lo + r.n_w > n_win) { printf("range beyond the clip\n"); return 1; }
                cuts[k] = parallel_snap_pick(rms.data() + r.w_lo, r, cuts[k]);
            }
            print_cuts(cuts);
        } else if (cmd == "merge") {
            int off, np;
            std::cin >> off >> np;
            std::vector<int> cuts(np);
            for (int& c : cuts) std::cin >> c;
            std::vector<std::vector<Seg>> pieces(np);
            for (auto& pc : pieces) {
                int ns;
                std::cin >> ns;
                pc.resize(ns);
                for (Seg& g : pc) {
                    int nt;
                    std::cin >> g.t0 >> g.t1 >> nt;
                    g.tokens.resize(nt);
                    for (Tok& t : g.tokens) std::cin >> t.t0 >> t.t1 >> t.t_dtw;
                }
            }
            std::vector<Seg> out = std::move(pieces[0]);
            size_t calls = 0;
            for (int k = 1; k < np; k++)
                parallel_merge_piece(out, pieces[k], parallel_shift(cuts[k], off), [&] { calls++; });
            for (size_t i = 0; i < out.size(); i++) {
                printf(i ? " | %lld %lld %zu" : "%lld %lld %zu", (long long)out[i].t0, (long long)out[i].t1, out[i].tokens.size());
                for (const Tok& t : out[i].tokens) printf(" %lld %lld %lld", (long long)t.t0, (long long)t.t1, (long long)t.t_dtw);
            }
            printf("\n");
        } else {
            fprintf(stderr, "unknown case '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
