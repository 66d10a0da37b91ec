// Stand-alone driver of the token-time host code (nobs-whisper_amd/csrc/token_times.h) for
// tests/test_token_times_host.py: no GPU, no HIP. It reads scripted segments, runs phase 1 on each (the clip state
// carried from segment to segment) and, with max_len > 0, the wrap on phase 1's times, and prints the results.
//
//   g++ -std=c++17 -O1 -g [-fsanitize=address,undefined] -I nobs-whisper_amd/csrc tools/token_times_check.cpp
//       nobs-whisper_amd/csrc/token_times.cpp -o token_times_check && ./token_times_check < script
//
// Script: "beg eot thold_pt thold_ptsum max_len split_on_word n_vocab", then n_vocab token strings as hex bytes
// ("-" = the empty string), then any number of "clip" (a new clip: the state starts over) and
// "seg t0 t1 n" + n lines "id tid pt ptsum".
// Output per segment: "seg n", n lines "tok t0 t1 vlen" (vlen as %a), and with max_len > 0 the pieces
// "piece i0 i1 t0 t1 text-as-hex".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "token_times.h"

using namespace wm;

static std::string unhex(const char* s) {
    std::string r;
    if (strcmp(s, "-") == 0) return r;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        unsigned v = 0;
        sscanf(s + i, "%2x", &v);
        r.push_back((char)v);
    }
    return r;
}

int main() {
    int beg, eot, max_len, sow, n_vocab;
    float thold_pt, thold_ptsum;
    if (scanf("%d %d %f %f %d %d %d", &beg, &eot, &thold_pt, &thold_ptsum, &max_len, &sow, &n_vocab) != 7 || n_vocab < 0) return 2;
    std::vector<std::string> vocab(n_vocab);
    std::vector<char> buf(1 << 16);
    for (int i = 0; i < n_vocab; i++) {
        if (scanf("%65535s", buf.data()) != 1) return 2;
        vocab[i] = unhex(buf.data());
    }
    TtState st;
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (strcmp(cmd, "clip") == 0) {
            st = TtState();
            continue;
        }
        if (strcmp(cmd, "seg") != 0) return 2;
        long long t0, t1;
        int n;
        if (scanf("%lld %lld %d", &t0, &t1, &n) != 3 || n < 0) return 2;
        std::vector<TtTok> tok(n);
        for (TtTok& t : tok)
            if (scanf("%d %d %f %f", &t.id, &t.tid, &t.pt, &t.ptsum) != 4) return 2;
        tt_phase1(tok, t0, t1, st, beg, thold_pt, thold_ptsum, vocab);
        printf("seg %d\n", n);
        for (const TtTok& t : tok) printf("tok %lld %lld %a\n", (long long)t.t0, (long long)t.t1, (double)t.vlen);
        if (max_len > 0) {
            for (const TtPiece& p : tt_wrap(tok, t0, t1, max_len, sow != 0, eot, vocab)) {
                printf("piece %d %d %lld %lld ", p.i0, p.i1, (long long)p.t0, (long long)p.t1);
                if (p.text.empty()) printf("-");
                for (unsigned char ch : p.text) printf("%02x", ch);
                printf("\n");
            }
        }
    }
    return 0;
}
