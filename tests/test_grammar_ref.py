"""tests/grammar_ref.py (the restated grammar semantics) against answers worked by hand, on the 12-token
toy vocabulary of tests/grammar_cases.py. The C++ host code, the hooks and the end-to-end tests are compared with this
reference, so it is pinned here first."""
import grammar_cases as gc
import grammar_ref as gr
from grammar_ref import cls, lit, ref, rule

G1, G2, G5 = gc.GRAMMARS["G1"][0], gc.GRAMMARS["G2"][0], gc.GRAMMARS["G5"][0]


def test_rule_layout():
    """rule() / lit() / cls() lay elements out as whisper.h documents them."""
    r = rule(lit("ab"), cls((ord("a"), ord("c")), ord("x"), neg=True))
    assert r == [(gr.CHAR, 97), (gr.CHAR, 98), (gr.ALT, 0), (gr.CHAR_NOT, 97), (gr.CHAR_RNG_UPPER, 99), (gr.CHAR_ALT, 120),
                 (gr.END, 0)]
    assert (gr.END, gr.ALT, gr.RULE_REF, gr.CHAR, gr.CHAR_NOT, gr.CHAR_RNG_UPPER, gr.CHAR_ALT) == (0, 1, 2, 3, 4, 5, 6)


def test_advance_and_init():
    # G1: one stack per alternate, each at the alternate's first char
    assert gr.init(G1, 0) == [((0, 0),), ((0, 13),)]
    # G2 root ::= item root | item: the reference to item is replaced by item's first element, over root's next
    # symbol (first alternate) or over nothing (second: the alternate ends after item)
    assert gr.init(G2, 0) == [((0, 1), (1, 0)), ((1, 0),)]
    # an empty alternate gives the empty stack; duplicates are dropped
    g = [rule(ref(1), ref(1)), rule([], lit("a"))]
    assert gr.init(g, 0) == [(), ((1, 1),)]
    out = []
    gr.advance(G2, (), out)
    assert out == [()]


def test_accept():
    s = gr.init(G1, 0)
    s = gr.accept(G1, s, ord(" "))
    assert s == [((0, 1),), ((0, 14),)]
    s = gr.accept(G1, s, ord("h"))
    assert s == [((0, 2),)]
    assert gr.accept(G1, s, ord("x")) == []
    # the last char of an alternate pops to the empty stack
    assert gr.accept(G1, [((0, 11),)], ord("d")) == [()]
    assert gr.accept(G1, [()], ord("d")) == []
    # G2 after " a": letters may go on, or (first alternate of root) a new item may start, or the sentence may end
    # (rule 2 = letters: [a-z] letters | [a-z], its alternates at elements 0 and 4)
    s = gr.accept(G2, gr.init(G2, 0), ord(" "))
    assert s == [((0, 1), (2, 0)), ((0, 1), (2, 4)), ((2, 0),), ((2, 4),)]
    assert not gr.allow_eot(s)
    s = gr.accept(G2, s, ord("a"))
    assert s == [((0, 1), (2, 0)), ((0, 1), (2, 4)), ((0, 1), (1, 0)), ((1, 0),), ((2, 0),), ((2, 4),), ()]
    assert gr.allow_eot(s)
    assert gr.accept(G2, s, ord("A")) == []


def test_decode():
    assert gr.decode(b" he") == ([32, 104, 101], (0, 0))
    assert gr.decode("é♪".encode()) == ([0xE9, 0x266A], (0, 0))
    assert gr.decode("😀".encode()) == ([0x1F600], (0, 0))
    # a valid 2-byte character split over two tokens
    assert gr.decode(b"\xc3") == ([], (3, 1))
    assert gr.decode(b"\xa9", (3, 1)) == ([0xE9], (0, 0))
    assert gr.decode(b"\xa9x", (3, 1)) == ([0xE9, 120], (0, 0))
    assert gr.decode(b"\xe2\x99") == ([], ((2 << 6) | 0x19, 1))
    assert gr.decode(b"\xe2") == ([], (2, 2))
    assert gr.decode(b"", (2, 2)) == ([], (2, 2))
    # invalid: a continuation byte as lead (0x80, 0xa9), a non-continuation byte inside a pending character
    assert gr.decode(b"\x80") == ([], (0, -1))
    assert gr.decode(b"\xa9") == ([], (0, -1))
    assert gr.decode(b"ab\x80") == ([], (0, -1))
    assert gr.decode(b"x", (3, 1)) == ([], (0, -1))
    # a zero byte ends the string; after an invalid token decoding starts afresh
    assert gr.decode(b"a\x00b") == ([97], (0, 0))
    assert gr.decode(b"\x00b") == ([], (0, 0))
    assert gr.decode(b"a", (0, -1)) == ([97], (0, 0))
    # continuation bytes are not checked after a lead byte
    assert gr.decode(b"\xc3A") == ([(3 << 6) + (0x41 & 0x3F)], (0, 0))


def test_match_partial():
    hi = (1, 0)  # [à-ÿ] = [0xE0-0xFF]
    assert gr.match_partial(G5, hi, (3, 1))       # 0xC0..0xFF overlaps
    assert not gr.match_partial(G5, hi, (2, 1))   # 0x80..0xBF
    assert not gr.match_partial(G5, hi, (1, 1))   # value < 2: an overlong form
    assert not gr.match_partial(G5, hi, (0, -1))
    assert gr.match_partial(G5, (0, 0), (3, 1))   # 'é' = 0xE9
    assert gr.match_partial(G5, (0, 1), (2, 2))   # '♪' = 0x266A in 0x2000..0x2FFF
    assert not gr.match_partial(G5, (0, 1), (0, 2))  # low 0 becomes 0x800: 0x800..0xFFF
    assert gr.match_partial(G5, (0, 1), ((2 << 6) | 0x19, 1))  # 0x2640..0x267F
    neg = [rule(cls((ord("a"), ord("z")), neg=True))]
    assert gr.match_partial(neg, (0, 0), (3, 1))  # no overlap with a-z, negated
    wide = [rule(cls((1, 0x10FFFF), neg=True))]
    assert not gr.match_partial(wide, (0, 0), (3, 1))
    # n_remain 3, value 0: low becomes 0x10000
    assert gr.match_partial([rule(cls((0x10000, 0x10FFFF)))], (0, 0), (0, 3))
    assert not gr.match_partial([rule(cls((0x800, 0xFFFF)))], (0, 0), (0, 3))


def bits(rules, accepted, toks=gc.TOY, eot=gc.TOY_EOT):
    st = gr.State(rules, 0)
    for i in accepted:
        st.accept_token(toks[i])
    return [int(b) for b in st.reject(toks, eot)], st


def test_reject_toy_g1():
    #        " hello" " world" " thank" " you" " he" "llo" c3 a9 80 "a\0b" "" "x" EOT SOT
    m, st = bits(G1, [])
    assert m == [0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 0]
    m, st = bits(G1, [4])  # " he"
    assert st.stacks == [((0, 3),)]
    assert m == [1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0]
    m, st = bits(G1, [4, 5])  # " he" "llo"
    assert m == [1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0]
    m, st = bits(G1, [0, 1])  # the sentence is complete: only EOT
    assert st.stacks == [()] and gr.allow_eot(st.stacks)
    assert m == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 0]
    m, st = bits(G1, [1])  # a violating token: no stacks, the grammar is off, nothing is penalised
    assert st.stacks == [] and m == [0] * 14
    m, st = bits(G1, [0, 12, 13])  # specials are skipped
    assert st.stacks == [((0, 6),)]
    assert gr.pack([bool(b) for b in bits(G1, [])[0]]) == [0b01101111101010]


def test_split_character_and_invalid_tokens():
    m, st = bits(G5, [])
    # c3 may begin 'é' (match_partial); a9 and 80 are invalid leads; everything else is rejected; EOT is not allowed
    assert m == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0]
    m, st = bits(G5, [6])  # after c3: a pending partial (3, 1)
    assert st.partial == (3, 1) and st.stacks == [((0, 0),)]
    # only a9 completes 'é'; every token that does not start with a continuation byte is invalid here; 0x80 gives
    # 0xC0, which is not 'é'
    assert m == [1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0]
    m, st = bits(G5, [6, 7])
    assert st.partial == (0, 0) and st.stacks == [((0, 1),)]
    # an invalid token is accepted as nothing: the stacks stay, the partial reads (0, -1), the next token decodes afresh
    m2, st2 = bits(G5, [8])
    assert st2.stacks == gr.init(G5, 0) and st2.partial == (0, -1)
    assert m2 == bits(G5, [])[0]
    # a token that is only a zero byte has no code points and no partial: accepted in every state with stacks
    toks = [b"\x00", b"a\x00b", b"[_EOT_]"]
    assert [int(b) for b in gr.State(G1, 0).reject(toks, 2)] == [0, 1, 1]


def test_validate():
    for name, (rules, start) in gc.GRAMMARS.items():
        assert gr.validate(rules, start) == 0, name
    assert gr.validate(*gc.ACCEPT_ALL) == 0
    assert gr.validate([], 0) == 0
    for name, (rules, start) in gc.INVALID.items():
        assert gr.validate(rules, start) == gr.GRAMMAR_ERR, name
    # right recursion and a nullable rule before a different rule are fine
    assert gr.validate([rule(lit("a") + ref(0), [])], 0) == 0
    assert gr.validate([rule(ref(1) + ref(2)), rule([], lit("z")), rule(lit("q"))], 0) == 0


def test_sentences_are_valid():
    """Each grammar's sentence, spelled by the synthetic vocabulary, is accepted token by token and may end."""
    toks, eot = gc.vocab("synthetic")
    for name, (rules, start) in gc.GRAMMARS.items():
        ids = gc.tokenize(toks, eot, gc.SENTENCES[name].encode())
        assert ids, name
        st = gr.State(rules, start)
        for i in ids:
            assert not gr.token_rejected(rules, st.stacks, st.partial, toks[i]), (name, i)
            st.accept_token(toks[i])
            assert st.stacks, (name, i)
        assert gr.allow_eot(st.stacks) and st.partial == (0, 0), name
