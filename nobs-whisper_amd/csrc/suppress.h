// The deny mask of whisper_full_params.suppress_nst and suppress_regex: the host part, free of HIP, so
// tools/suppress_check.cpp builds with a plain C++ compiler. The logits kernels (kernels/logits.hip) give every token
// whose bit is set a logit of -inf.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace wm {

// (n_vocab + 31) / 32 words; token i is bit i & 31 of word i >> 5; bits at and above n_vocab are 0.
inline int suppress_words(int n_vocab) { return (n_vocab + 31) / 32; }

// The mask of a call. suppress_nst: whisper.cpp's non-speech list: every list string s bans the ids of s and of
// " " + s that the vocabulary has, and " -" and " '" are banned too (hyphens and quotes are allowed inside a word,
// not at its start). regex (null = off; an empty string is a pattern like any other): std::regex, ECMAScript; a token
// is banned when std::regex_match accepts its whole string, over every entry of token_to_id, specials included.
// Ids outside [0, n_vocab) are skipped. Returns 0, or -8 when the pattern does not compile (`words` is then empty
// and *err, if given, holds the regex_error's text).
int suppress_build(const std::map<std::string, int>& token_to_id, int n_vocab, bool suppress_nst, const char* regex,
                   std::vector<uint32_t>& words, std::string* err = nullptr);

}  // namespace wm
