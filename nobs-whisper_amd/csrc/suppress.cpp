// suppress.h: the deny mask of suppress_nst / suppress_regex, on the host.
#include "suppress.h"

#include <regex>

namespace wm {

// whisper.cpp's non_speech_tokens [ext]
static const char* const kNonSpeech[] = {
    "\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
    "「", "」", "『", "』", "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))", "[[", "]]",
    "{{", "}}", "♪♪", "♪♪♪", "♩", "♪", "♫", "♬", "♭", "♮", "♯"};

int suppress_build(const std::map<std::string, int>& token_to_id, int n_vocab, bool suppress_nst, const char* regex,
                   std::vector<uint32_t>& words, std::string* err) {
    words.assign((size_t)suppress_words(n_vocab > 0 ? n_vocab : 0), 0u);
    const auto ban = [&](int id) {
        if (id >= 0 && id < n_vocab) words[(size_t)id >> 5] |= 1u << (id & 31);
    };
    const auto ban_str = [&](const std::string& s) {
        const auto it = token_to_id.find(s);
        if (it != token_to_id.end()) ban(it->second);
    };
    if (suppress_nst) {
        for (const char* s : kNonSpeech) {
            ban_str(s);
            ban_str(std::string(" ") + s);
        }
        ban_str(" -");
        ban_str(" '");
    }
    if (regex) {
        try {
            const std::regex re(regex);
            for (const auto& kv : token_to_id)
                if (std::regex_match(kv.first, re)) ban(kv.second);
        } catch (const std::regex_error& e) {
            words.clear();
            if (err) *err = e.what();
            return -8;
        }
    }
    return 0;
}

}  // namespace wm
