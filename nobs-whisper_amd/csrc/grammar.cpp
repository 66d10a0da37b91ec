// whisper_full_params.grammar_rules on the host (grammar.h).
#include "grammar.h"

#include <algorithm>
#include <cstring>
#include <unordered_map>

namespace wm {

bool GrammarRules::operator==(const GrammarRules& o) const {
    return start == o.start && rule_off == o.rule_off && elems.size() == o.elems.size() &&
           (elems.empty() || memcmp(elems.data(), o.elems.data(), elems.size() * sizeof(GramElem)) == 0);
}

static bool is_end(const GramElem& e) { return e.type == GRE_END || e.type == GRE_ALT; }
static bool is_class_head(int t) { return t == GRE_CHAR || t == GRE_CHAR_NOT; }

// the first element of every alternate of rule r (it may be an ALT / END: an empty alternate)
static void alternates(const GrammarRules& g, int r, std::vector<int>& out) {
    out.clear();
    out.push_back(g.rule_off[r]);
    for (int i = g.rule_off[r]; g.elems[i].type != GRE_END; i++)
        if (g.elems[i].type == GRE_ALT) out.push_back(i + 1);
}

static int fail(std::string* err, const std::string& why) {
    if (err) *err = why;
    return -9;
}

int grammar_compile(const GramElem* const* rules, size_t n_rules, size_t i_start, GrammarRules& out, std::string* err) {
    out = GrammarRules();
    if (!rules || n_rules == 0) return 0;
    for (size_t r = 0; r < n_rules; r++)
        if (!rules[r]) return fail(err, "rule " + std::to_string(r) + " is null");
    if (i_start >= n_rules) return fail(err, "i_start_rule " + std::to_string(i_start) + " >= n_grammar_rules " + std::to_string(n_rules));
    GrammarRules g;
    g.start = (int)i_start;
    for (size_t r = 0; r < n_rules; r++) {
        g.rule_off.push_back((int)g.elems.size());
        int prev = -1;
        for (const GramElem* e = rules[r];; e++) {
            const std::string where = "rule " + std::to_string(r) + " element " + std::to_string(e - rules[r]);
            if (e->type < GRE_END || e->type > GRE_CHAR_ALT) return fail(err, where + ": unknown element type");
            if (e->type == GRE_RULE_REF && e->value >= n_rules) return fail(err, where + ": RULE_REF out of range");
            if (e->type == GRE_CHAR_RNG_UPPER && !(is_class_head(prev) || prev == GRE_CHAR_ALT))
                return fail(err, where + ": CHAR_RNG_UPPER does not follow a char");
            if (e->type == GRE_CHAR_ALT && !(is_class_head(prev) || prev == GRE_CHAR_ALT || prev == GRE_CHAR_RNG_UPPER))
                return fail(err, where + ": CHAR_ALT does not follow a char class");
            if ((int)g.elems.size() >= kGramMaxElems) return fail(err, "more than " + std::to_string(kGramMaxElems) + " elements");
            g.elems.push_back(*e);
            prev = e->type;
            if (e->type == GRE_END) break;
        }
    }
    g.rule_off.push_back((int)g.elems.size());
    // left recursion: nullable rules by fixpoint, then a cycle among the "reachable at the leftmost position" edges
    const int n = (int)n_rules;
    std::vector<char> nullable(n, 0);
    std::vector<int> alts;
    for (bool changed = true; changed;) {
        changed = false;
        for (int r = 0; r < n; r++) {
            if (nullable[r]) continue;
            alternates(g, r, alts);
            for (int a : alts) {
                bool all = true;
                for (int i = a; !is_end(g.elems[i]); i++)
                    if (g.elems[i].type != GRE_RULE_REF || !nullable[g.elems[i].value]) { all = false; break; }
                if (all) { nullable[r] = 1; changed = true; break; }
            }
        }
    }
    std::vector<std::vector<int>> edges(n);
    for (int r = 0; r < n; r++) {
        alternates(g, r, alts);
        for (int a : alts)
            for (int i = a; !is_end(g.elems[i]) && g.elems[i].type == GRE_RULE_REF; i++) {
                edges[r].push_back((int)g.elems[i].value);
                if (!nullable[g.elems[i].value]) break;
            }
    }
    for (int r = 0; r < n; r++) {
        std::vector<char> seen(n, 0);
        std::vector<int> todo = edges[r];
        while (!todo.empty()) {
            const int x = todo.back();
            todo.pop_back();
            if (x == r) return fail(err, "rule " + std::to_string(r) + " is left-recursive");
            if (seen[x]) continue;
            seen[x] = 1;
            todo.insert(todo.end(), edges[x].begin(), edges[x].end());
        }
    }
    out = std::move(g);
    return 0;
}

GramPartial gram_decode(const std::string& text, GramPartial in, std::vector<uint32_t>& cps) {
    static const int lookup[16] = {1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 3, 4};
    cps.clear();
    const size_t z = text.find('\0');
    const size_t len = z == std::string::npos ? text.size() : z;  // (upstream walks a C string)
    const unsigned char* p = (const unsigned char*)text.data();
    uint32_t value = in.value;
    int n_remain = in.n_remain;
    size_t i = 0;
    while (i < len && n_remain > 0) {
        if ((p[i] >> 6) != 2) { cps.clear(); return GramPartial{0, -1}; }
        value = (value << 6) + (p[i] & 0x3Fu);
        i++;
        n_remain--;
    }
    if (in.n_remain > 0 && n_remain == 0) cps.push_back(value);
    while (i < len) {
        const unsigned first = p[i];
        n_remain = lookup[first >> 4] - 1;
        if (n_remain < 0) { cps.clear(); return GramPartial{0, -1}; }
        value = first & ((1u << (7 - n_remain)) - 1u);
        i++;
        while (i < len && n_remain > 0) {
            value = (value << 6) + (p[i] & 0x3Fu);
            i++;
            n_remain--;
        }
        if (n_remain == 0) cps.push_back(value);
    }
    if (n_remain > 0) return GramPartial{value, n_remain};
    return GramPartial{0, 0};
}

void gram_vocab_build(const std::vector<std::string>& id_to_token, int n_vocab, int eot, GramVocab& out) {
    out = GramVocab();
    out.n_vocab = n_vocab;
    out.eot = std::min(eot, n_vocab);
    out.strs = &id_to_token;
    std::vector<uint32_t> cps;
    static const std::string empty;
    for (int i = 0; i < out.eot; i++) {
        out.off.push_back((uint32_t)out.cps.size());
        out.tail.push_back(gram_decode(i < (int)id_to_token.size() ? id_to_token[i] : empty, GramPartial{0, 0}, cps));
        out.cps.insert(out.cps.end(), cps.begin(), cps.end());
    }
    out.off.push_back((uint32_t)out.cps.size());
}

static void push_unique(std::vector<GramStack>& out, const GramStack& s) {
    if (std::find(out.begin(), out.end(), s) == out.end()) out.push_back(s);
}

void gram_advance(const GrammarRules& g, const GramStack& stack, std::vector<GramStack>& out) {
    if (stack.empty() || g.elems[stack.back()].type != GRE_RULE_REF) {
        push_unique(out, stack);
        return;
    }
    const int top = stack.back(), rule = (int)g.elems[top].value;
    std::vector<int> alts;
    alternates(g, rule, alts);
    for (int a : alts) {
        GramStack s(stack.begin(), stack.end() - 1);
        if (!is_end(g.elems[top + 1])) s.push_back((uint16_t)(top + 1));
        if (!is_end(g.elems[a])) s.push_back((uint16_t)a);
        gram_advance(g, s, out);
    }
}

// the class at pos against code point c; *after = the position after the class
static bool match_char(const GrammarRules& g, int pos, uint32_t c, int* after) {
    const bool positive = g.elems[pos].type == GRE_CHAR;
    bool found = false;
    int i = pos;
    do {
        if (g.elems[i + 1].type == GRE_CHAR_RNG_UPPER) {
            found = found || (g.elems[i].value <= c && c <= g.elems[i + 1].value);
            i += 2;
        } else {
            found = found || g.elems[i].value == c;
            i += 1;
        }
    } while (g.elems[i].type == GRE_CHAR_ALT);
    *after = i;
    return found == positive;
}

bool gram_match_partial(const GrammarRules& g, int pos, GramPartial p) {
    if (p.n_remain < 0 || (p.n_remain == 1 && p.value < 2)) return false;
    const bool positive = g.elems[pos].type == GRE_CHAR;
    uint32_t low = p.value << (p.n_remain * 6);
    const uint32_t high = low | ((1u << (p.n_remain * 6)) - 1u);
    if (low == 0) {
        if (p.n_remain == 2) low = 1u << 11;
        else if (p.n_remain == 3) low = 1u << 16;
    }
    bool hit = false;
    int i = pos;
    do {
        if (g.elems[i + 1].type == GRE_CHAR_RNG_UPPER) {
            hit = hit || (g.elems[i].value <= high && low <= g.elems[i + 1].value);
            i += 2;
        } else {
            hit = hit || (low <= g.elems[i].value && g.elems[i].value <= high);
            i += 1;
        }
    } while (g.elems[i].type == GRE_CHAR_ALT);
    return hit == positive;
}

void gram_accept(const GrammarRules& g, const std::vector<GramStack>& stacks, uint32_t c, std::vector<GramStack>& out) {
    out.clear();
    for (const GramStack& s : stacks) {
        if (s.empty()) continue;
        int after;
        if (!match_char(g, s.back(), c, &after)) continue;
        GramStack t(s.begin(), s.end() - 1);
        if (!is_end(g.elems[after])) t.push_back((uint16_t)after);
        gram_advance(g, t, out);
    }
}

void Grammar::init(const GrammarRules& g) {
    stacks.clear();
    partial = GramPartial();
    if (!g.on()) return;
    std::vector<int> alts;
    alternates(g, g.start, alts);
    for (int a : alts) {
        GramStack s;
        if (!is_end(g.elems[a])) s.push_back((uint16_t)a);
        gram_advance(g, s, stacks);
    }
}

void Grammar::accept_token(const GrammarRules& g, const std::string& text) {
    if (!g.on() || stacks.empty() || text.rfind("[_", 0) == 0) return;
    std::vector<uint32_t> cps;
    const GramPartial out = gram_decode(text, partial, cps);  // (an invalid token: no code points, {0, -1})
    std::vector<GramStack> next;
    for (uint32_t c : cps) {
        gram_accept(g, stacks, c, next);
        stacks.swap(next);
    }
    partial = out;
}

bool Grammar::allow_eot() const {
    for (const GramStack& s : stacks)
        if (s.empty()) return true;
    return false;
}

void grammar_reject(const GrammarRules& g, const GramVocab& v, const Grammar& st, uint32_t* words) {
    std::fill(words, words + grammar_words(v.n_vocab), 0u);
    if (!g.on() || st.stacks.empty()) return;
    // The stack lists met while the tokens are walked, and accept's result per (list, code point), computed once: most
    // tokens of a vocabulary share their first characters. List 0 is the state's; -1 = no stack is left.
    std::vector<std::vector<GramStack>> lists{st.stacks};
    std::unordered_map<uint64_t, int> trans;
    std::vector<GramStack> next;
    auto step = [&](int from, uint32_t c) -> int {
        const uint64_t key = (uint64_t)from << 32 | c;
        const auto it = trans.find(key);
        if (it != trans.end()) return it->second;
        gram_accept(g, lists[from], c, next);
        int to = -1;
        if (!next.empty()) {
            const auto f = std::find(lists.begin(), lists.end(), next);
            to = (int)(f - lists.begin());
            if (f == lists.end()) lists.push_back(next);
        }
        trans.emplace(key, to);
        return to;
    };
    std::vector<uint32_t> dec;
    for (int id = 0; id < v.eot; id++) {
        if (id >= (int)v.strs->size() || (*v.strs)[id].empty()) continue;
        const uint32_t* cp;
        size_t n_cp;
        GramPartial tail;
        if (st.partial.n_remain > 0) {  // (rare: the last token ended inside a character)
            tail = gram_decode((*v.strs)[id], st.partial, dec);
            cp = dec.data();
            n_cp = dec.size();
        } else {
            tail = v.tail[id];
            cp = v.cps.data() + v.off[id];
            n_cp = v.off[id + 1] - v.off[id];
        }
        int cur = tail.n_remain >= 0 ? 0 : -1;
        for (size_t k = 0; cur >= 0 && k < n_cp; k++) cur = step(cur, cp[k]);
        bool ok = cur >= 0 && tail.n_remain == 0;
        if (cur >= 0 && tail.n_remain > 0)
            for (const GramStack& t : lists[cur])
                if (!t.empty() && gram_match_partial(g, t.back(), tail)) { ok = true; break; }
        if (!ok) words[id >> 5] |= 1u << (id & 31);
    }
    if (v.eot < v.n_vocab && !st.allow_eot()) words[v.eot >> 5] |= 1u << (v.eot & 31);
}

}  // namespace wm
