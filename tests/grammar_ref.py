"""Reference of whisper_full_params.grammar_rules: whisper.cpp's grammar code restated in plain Python
with integers only. csrc/grammar.cpp and the engine are tested against this file; it is written from the semantics,
not from the C++.

A grammar is a list of rules; a rule is a list of (type, value) elements ending in END. Positions are (rule, index)
pairs. A stack is a tuple of positions with the top last; a state is (stacks, partial) with partial = (value,
n_remain).
"""
END, ALT, RULE_REF, CHAR, CHAR_NOT, CHAR_RNG_UPPER, CHAR_ALT = range(7)
GRAMMAR_ERR = -9
_LEN = (1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 3, 4)


# ---- building rules (tests) --------------------------------------------------------------------------------------
def lit(s):
    """The elements of a literal: one CHAR per code point."""
    return [(CHAR, ord(ch)) for ch in s]


def cls(*items, neg=False):
    """A char class: items are code points or (lo, hi) ranges."""
    out = []
    for k, it in enumerate(items):
        lo, hi = it if isinstance(it, tuple) else (it, None)
        out.append(((CHAR_NOT if neg else CHAR) if k == 0 else CHAR_ALT, lo))
        if hi is not None:
            out.append((CHAR_RNG_UPPER, hi))
    return out


def ref(r):
    return [(RULE_REF, r)]


def rule(*alternates):
    """A rule from its alternates (each a list of elements)."""
    out = []
    for k, a in enumerate(alternates):
        if k:
            out.append((ALT, 0))
        out.extend(a)
    out.append((END, 0))
    return out


# ---- validation ---------------------------------------------------------------------------------------------------
def _alternates(r):
    """Index of the first element of each alternate of rule r (it may point at ALT / END: an empty alternate)."""
    out, i = [0], 0
    while r[i][0] != END:
        if r[i][0] == ALT:
            out.append(i + 1)
        i += 1
    return out


def _symbols(r, i):
    """The symbols of the alternate that starts at i: ('ref', rule) or ('char',)."""
    out = []
    while r[i][0] not in (END, ALT):
        if r[i][0] == RULE_REF:
            out.append(("ref", r[i][1]))
            i += 1
        else:
            out.append(("char",))
            i += 1
            while r[i][0] in (CHAR_RNG_UPPER, CHAR_ALT):
                i += 1
    return out


def validate(rules, i_start):
    """0, or GRAMMAR_ERR for a null rule, a start rule or reference out of range, a stray CHAR_RNG_UPPER / CHAR_ALT, or
    left recursion."""
    n = len(rules)
    if n == 0:
        return 0
    if any(r is None for r in rules) or i_start >= n:
        return GRAMMAR_ERR
    for r in rules:
        prev = None
        for t, v in r:
            if t == RULE_REF and not 0 <= v < n:
                return GRAMMAR_ERR
            if t == CHAR_RNG_UPPER and prev not in (CHAR, CHAR_NOT, CHAR_ALT):
                return GRAMMAR_ERR
            if t == CHAR_ALT and prev not in (CHAR, CHAR_NOT, CHAR_ALT, CHAR_RNG_UPPER):
                return GRAMMAR_ERR
            prev = t
            if t == END:
                break
    alts = [[_symbols(r, a) for a in _alternates(r)] for r in rules]
    nullable = [False] * n
    changed = True
    while changed:
        changed = False
        for k in range(n):
            if not nullable[k] and any(all(s[0] == "ref" and nullable[s[1]] for s in a) for a in alts[k]):
                nullable[k] = changed = True
    edges = [set() for _ in range(n)]  # k -> rules reachable at the leftmost position
    for k in range(n):
        for a in alts[k]:
            for s in a:
                if s[0] != "ref":
                    break
                edges[k].add(s[1])
                if not nullable[s[1]]:
                    break
    for k in range(n):  # a cycle through k?
        seen, todo = set(), list(edges[k])
        while todo:
            x = todo.pop()
            if x == k:
                return GRAMMAR_ERR
            if x not in seen:
                seen.add(x)
                todo.extend(edges[x])
    return 0


# ---- the automaton ------------------------------------------------------------------------------------------------
def _el(rules, pos):
    return rules[pos[0]][pos[1]]


def end_of_sequence(rules, pos):
    return _el(rules, pos)[0] in (END, ALT)


def advance(rules, stack, out):
    """Expand rule references at the top of `stack` until every resulting stack is empty or has a char class on top;
    results are appended to `out` (a list without duplicates)."""
    if not stack:
        if stack not in out:
            out.append(stack)
        return
    top = stack[-1]
    t, v = _el(rules, top)
    if t != RULE_REF:
        if stack not in out:
            out.append(stack)
        return
    for a in _alternates(rules[v]):
        new = list(stack[:-1])
        nxt = (top[0], top[1] + 1)
        if not end_of_sequence(rules, nxt):
            new.append(nxt)
        if not end_of_sequence(rules, (v, a)):
            new.append((v, a))
        advance(rules, tuple(new), out)


def init(rules, i_start):
    out = []
    for a in _alternates(rules[i_start]):
        advance(rules, () if end_of_sequence(rules, (i_start, a)) else ((i_start, a),), out)
    return out


def _class_items(rules, pos):
    """(lo, hi) of every value / range of the class at pos."""
    r, i = pos
    items = []
    while True:
        lo = rules[r][i][1]
        if rules[r][i + 1][0] == CHAR_RNG_UPPER:
            items.append((lo, rules[r][i + 1][1]))
            i += 2
        else:
            items.append((lo, lo))
            i += 1
        if rules[r][i][0] != CHAR_ALT:
            return items, (r, i)


def match_char(rules, pos, c):
    items, after = _class_items(rules, pos)
    found = any(lo <= c <= hi for lo, hi in items)
    return found == (_el(rules, pos)[0] == CHAR), after


def match_partial(rules, pos, partial):
    value, n_remain = partial
    if n_remain < 0 or (n_remain == 1 and value < 2):
        return False
    low = value << (6 * n_remain)
    high = low | ((1 << (6 * n_remain)) - 1)
    if low == 0:
        if n_remain == 2:
            low = 1 << 11
        elif n_remain == 3:
            low = 1 << 16
    items, _ = _class_items(rules, pos)
    hit = any(lo <= high and low <= hi for lo, hi in items)
    return hit == (_el(rules, pos)[0] == CHAR)


def accept(rules, stacks, c):
    out = []
    for st in stacks:
        if not st:
            continue
        ok, after = match_char(rules, st[-1], c)
        if not ok:
            continue
        new = list(st[:-1])
        if not end_of_sequence(rules, after):
            new.append(after)
        advance(rules, tuple(new), out)
    return out


def decode(data, partial=(0, 0)):
    """(code points, partial_out) of a token's bytes after a pending partial; an invalid token gives ([], (0, -1))."""
    z = data.find(b"\0")
    if z >= 0:
        data = data[:z]
    value, n_remain = partial
    cps, i = [], 0
    while i < len(data) and n_remain > 0:
        b = data[i]
        if b & 0xC0 != 0x80:
            return [], (0, -1)
        value = (value << 6) + (b & 0x3F)
        i += 1
        n_remain -= 1
    if partial[1] > 0 and n_remain == 0:
        cps.append(value)
    while i < len(data):
        first = data[i]
        n_remain = _LEN[first >> 4] - 1
        if n_remain < 0:
            return [], (0, -1)
        value = first & ((1 << (7 - n_remain)) - 1)
        i += 1
        while i < len(data) and n_remain > 0:
            value = (value << 6) + (data[i] & 0x3F)
            i += 1
            n_remain -= 1
        if n_remain == 0:
            cps.append(value)
    if n_remain > 0:
        return cps, (value, n_remain)
    return cps, (0, 0)


def token_rejected(rules, stacks, partial, data, memo=None):
    """memo: a dict shared by the calls of one mask, {(stack list, code point): accept's result} (the same results,
    computed once per distinct pair: most tokens of a vocabulary share their first characters)."""
    cps, pout = decode(data, partial)
    if pout[1] < 0:
        return True
    cur = tuple(stacks)
    for c in cps:
        if memo is None:
            cur = tuple(accept(rules, cur, c))
        else:
            nxt = memo.get((cur, c))
            if nxt is None:
                nxt = memo[(cur, c)] = tuple(accept(rules, cur, c))
            cur = nxt
        if not cur:
            return True
    for st in cur:
        if pout[1] == 0 or (st and match_partial(rules, st[-1], pout)):
            return False
    return True


def allow_eot(stacks):
    return any(not st for st in stacks)


class State:
    """A decoder's grammar state: init, then accept_token per token that is fed next."""

    def __init__(self, rules, i_start):
        self.rules = rules
        self.stacks = init(rules, i_start) if rules else []
        self.partial = (0, 0)

    def accept_token(self, data):
        """data: the token's bytes. A string that starts with '[_' (every special id) is skipped."""
        if not self.rules or not self.stacks or data.startswith(b"[_"):
            return
        cps, pout = decode(data, self.partial)  # (an invalid token: no code points, partial (0, -1))
        for c in cps:
            self.stacks = accept(self.rules, self.stacks, c)
        self.partial = pout

    def reject(self, vocab, eot):
        """The mask of this state as a list of bools [len(vocab)]: ids < eot with a non-empty string that are rejected,
        the EOT entry = not allow_eot, ids above eot False. Empty stacks: all False."""
        out = [False] * len(vocab)
        if not self.stacks:
            return out
        memo = {}
        for i in range(min(eot, len(vocab))):
            if vocab[i]:
                out[i] = token_rejected(self.rules, self.stacks, self.partial, vocab[i], memo)
        if eot < len(vocab):
            out[eot] = not allow_eot(self.stacks)
        return out


def pack(bits):
    """bools -> uint32 words, token i = bit i & 31 of word i >> 5."""
    words = [0] * ((len(bits) + 31) // 32)
    for i, b in enumerate(bits):
        if b:
            words[i >> 5] |= 1 << (i & 31)
    return words
