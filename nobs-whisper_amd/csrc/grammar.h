// whisper_full_params.grammar_rules: the host part, free of HIP, so tools/grammar_check.cpp builds
// with a plain C++ compiler. Validation, the flat form of the rules, a decoder's grammar state, and the reject mask of
// a state over the vocabulary, which the logits kernels (kernels/logits.hip, GM = 1) turn into a penalty.
// The semantics are whisper.cpp's (restated in tests/grammar_ref.py, which this code is tested against).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace wm {

// whisper_grammar_element's layout (whisper.h; capi.cpp asserts it) and whisper_gretype's values
struct GramElem { int32_t type; uint32_t value; };
enum { GRE_END = 0, GRE_ALT = 1, GRE_RULE_REF = 2, GRE_CHAR = 3, GRE_CHAR_NOT = 4, GRE_CHAR_RNG_UPPER = 5, GRE_CHAR_ALT = 6 };

// The rules of a call in flat form: rule r is elems[rule_off[r] .. rule_off[r + 1]), its END included. A position is
// the index in elems of the first element of a symbol; 16 bits hold it (kGramMaxElems).
constexpr int kGramMaxElems = 65535;
struct GrammarRules {
    std::vector<GramElem> elems;
    std::vector<int> rule_off;  // [n_rules + 1]; empty = the call has no grammar
    int start = 0;
    bool on() const { return !rule_off.empty(); }
    bool operator==(const GrammarRules& o) const;
};

// Validates and flattens. 0; or -9 with the reason in *err: a null rule, i_start >= n_rules, a RULE_REF out of range, a
// CHAR_RNG_UPPER or CHAR_ALT that does not follow a char class, more than kGramMaxElems elements, or left recursion (a
// rule that reaches itself at the leftmost position through references whose preceding symbols are all nullable:
// upstream recurses without end on such a grammar). rules == null or n_rules == 0: 0 and `out` is off.
int grammar_compile(const GramElem* const* rules, size_t n_rules, size_t i_start, GrammarRules& out, std::string* err = nullptr);

// A pending partial UTF-8 sequence: the value so far and the bytes missing (-1: the last token was invalid UTF-8)
struct GramPartial { uint32_t value = 0; int n_remain = 0; };

// Decoded vocabulary: for ids < eot the code points of decode(string, {0, 0}) in CSR form and the trailing partial
// (n_remain -1: an invalid token). The strings stay with the caller (they are read when a state has a pending partial).
struct GramVocab {
    int n_vocab = 0, eot = 0;
    const std::vector<std::string>* strs = nullptr;
    std::vector<uint32_t> off;  // [eot + 1]
    std::vector<uint32_t> cps;
    std::vector<GramPartial> tail;  // [eot]
};
void gram_vocab_build(const std::vector<std::string>& id_to_token, int n_vocab, int eot, GramVocab& out);
// decode(bytes up to the first zero byte, partial_in): the code points into `cps` (cleared first), returns partial_out
GramPartial gram_decode(const std::string& text, GramPartial in, std::vector<uint32_t>& cps);

using GramStack = std::vector<uint16_t>;  // positions, the top last

// The grammar state of one decoder
struct Grammar {
    std::vector<GramStack> stacks;
    GramPartial partial;
    void init(const GrammarRules& g);  // the start state (no stacks when g is off)
    // the token that is fed next: skipped when its string starts with "[_" (every special id) or the stack list is empty
    void accept_token(const GrammarRules& g, const std::string& text);
    bool allow_eot() const;
    bool operator==(const Grammar& o) const {
        return stacks == o.stacks && partial.value == o.partial.value && partial.n_remain == o.partial.n_remain;
    }
};

// pieces (tools/grammar_check.cpp prints them)
void gram_advance(const GrammarRules& g, const GramStack& stack, std::vector<GramStack>& out);
void gram_accept(const GrammarRules& g, const std::vector<GramStack>& stacks, uint32_t c, std::vector<GramStack>& out);
bool gram_match_partial(const GrammarRules& g, int pos, GramPartial p);

inline int grammar_words(int n_vocab) { return (n_vocab + 31) / 32; }
// The reject mask of state `st` over the vocabulary: words[grammar_words(n_vocab)], token i = bit i & 31 of word
// i >> 5. Set: an id < eot with a non-empty string that the state rejects; the EOT bit = !allow_eot; ids above eot 0.
// A state without stacks: all zeros.
void grammar_reject(const GrammarRules& g, const GramVocab& v, const Grammar& st, uint32_t* words);

}  // namespace wm
