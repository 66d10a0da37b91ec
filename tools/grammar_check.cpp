// Stand-alone driver of the grammar host code (nobs-whisper_amd/csrc/grammar.h) for tests/test_grammar_host.py: no GPU,
// no HIP. It reads a vocabulary, grammars and accepted-token prefixes and prints each state's reject mask.
//
//   g++ -std=c++17 -O2 -g [-fsanitize=address,undefined] -I nobs-whisper_amd/csrc tools/grammar_check.cpp
//       nobs-whisper_amd/csrc/grammar.cpp -o grammar_check && ./grammar_check < script
//
// Script: "n_vocab eot n_tokens", then n_tokens token strings as hex bytes ("-" = the empty string; id = position),
// then any number of
//   "g n_rules i_start" + per rule "n_elems type value type value ..." (n_elems = -1: a null rule): sets the grammar,
//       prints "rc <code>" (0 or -9);
//   "s n_accepted id id ..": the state after init and accept_token of the ids, prints "state <n_stacks> <allow_eot>
//       <partial value> <partial n_remain> <mask ms>" and "words" + the mask's words in hex;
//   "t reps": times grammar_reject of the last state, prints "time <ms per mask>".
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "grammar.h"

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

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main() {
    int n_vocab, eot, n_tokens;
    if (scanf("%d %d %d", &n_vocab, &eot, &n_tokens) != 3 || n_vocab < 0 || n_tokens < 0 || n_tokens > n_vocab) return 2;
    std::vector<std::string> id_to_token(n_vocab);
    std::vector<char> buf(1 << 16);
    for (int i = 0; i < n_tokens; i++) {
        if (scanf("%65535s", buf.data()) != 1) return 2;
        id_to_token[i] = unhex(buf.data());
    }
    GramVocab vocab;
    gram_vocab_build(id_to_token, n_vocab, eot, vocab);
    GrammarRules g;
    Grammar st;
    std::vector<uint32_t> words(grammar_words(n_vocab));
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (strcmp(cmd, "g") == 0) {
            int n_rules, i_start;
            if (scanf("%d %d", &n_rules, &i_start) != 2 || n_rules < 0) return 2;
            std::vector<std::vector<GramElem>> rules(n_rules);
            std::vector<const GramElem*> ptrs(n_rules);
            for (int r = 0; r < n_rules; r++) {
                int n;
                if (scanf("%d", &n) != 1) return 2;
                for (int k = 0; k < n; k++) {
                    GramElem e;
                    if (scanf("%d %u", &e.type, &e.value) != 2) return 2;
                    rules[r].push_back(e);
                }
                ptrs[r] = n < 0 ? nullptr : rules[r].data();
            }
            std::string err;
            const int rc = grammar_compile(ptrs.data(), n_rules, i_start, g, &err);
            printf("rc %d\n", rc);
            if (rc != 0 && (g.on() || err.empty())) return 3;  // a refused grammar leaves no rules and says why
        } else if (strcmp(cmd, "s") == 0) {
            int n;
            if (scanf("%d", &n) != 1) return 2;
            st.init(g);
            for (int k = 0; k < n; k++) {
                int id;
                if (scanf("%d", &id) != 1 || id < 0 || id >= n_vocab) return 2;
                st.accept_token(g, id_to_token[id]);
            }
            const double t0 = now_ms();
            grammar_reject(g, vocab, st, words.data());
            printf("state %zu %d %u %d %.3f\nwords", st.stacks.size(), st.allow_eot() ? 1 : 0, st.partial.value,
                   st.partial.n_remain, now_ms() - t0);
            for (uint32_t w : words) printf(" %x", w);
            printf("\n");
        } else if (strcmp(cmd, "t") == 0) {
            int reps;
            if (scanf("%d", &reps) != 1 || reps < 1) return 2;
            const double t0 = now_ms();
            for (int k = 0; k < reps; k++) grammar_reject(g, vocab, st, words.data());
            printf("time %.4f\n", (now_ms() - t0) / reps);
        } else {
            return 2;
        }
    }
    return 0;
}
