// Stand-alone driver of the deny-mask host code (nobs-whisper_amd/csrc/suppress.h) for tests/test_suppress_host.py:
// no GPU, no HIP. It reads a vocabulary and a list of (suppress_nst, pattern) queries and prints each query's mask.
//
//   g++ -std=c++17 -O1 -g [-fsanitize=address,undefined] -I nobs-whisper_amd/csrc tools/suppress_check.cpp
//       nobs-whisper_amd/csrc/suppress.cpp -o suppress_check && ./suppress_check < script
//
// Script: "n_vocab n_tokens", then n_tokens token strings as hex bytes ("-" = the empty string; id = position, a
// repeated string keeps its last id, as the engine's token_to_id), then any number of "q nst pattern" with the
// pattern as hex bytes, "-" = the empty pattern, "null" = no pattern.
// Output per query: "rc <code> <build ms>" and, when the code is 0, "words" + the mask's words in hex.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "suppress.h"

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
    int n_vocab, n_tokens;
    if (scanf("%d %d", &n_vocab, &n_tokens) != 2 || n_vocab < 0 || n_tokens < 0) return 2;
    std::map<std::string, int> token_to_id;
    std::vector<char> buf(1 << 16);
    for (int i = 0; i < n_tokens; i++) {
        if (scanf("%65535s", buf.data()) != 1) return 2;
        token_to_id[unhex(buf.data())] = i;
    }
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        int nst;
        if (strcmp(cmd, "q") != 0 || scanf("%d %65535s", &nst, buf.data()) != 2) return 2;
        const bool has = strcmp(buf.data(), "null") != 0;
        const std::string pat = has ? unhex(buf.data()) : std::string();
        std::vector<uint32_t> words;
        std::string err;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = suppress_build(token_to_id, n_vocab, nst != 0, has ? pat.c_str() : nullptr, words, &err);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("rc %d %.3f\n", rc, ms);
        if (rc != 0) {
            if (!words.empty() || err.empty()) return 3;  // a refused pattern leaves no mask and says why
            continue;
        }
        if ((int)words.size() != suppress_words(n_vocab)) return 3;
        printf("words");
        for (uint32_t w : words) printf(" %x", w);
        printf("\n");
    }
    return 0;
}
