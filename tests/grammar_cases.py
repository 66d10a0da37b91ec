"""Shared inputs of the grammar tests: vocabularies, the grammars G1-G5, invalid grammars, and the
states a grammar is asked about. No test lives here."""
import functools

import grammar_ref as gr
from grammar_ref import cls, lit, ref, rule

# ---- vocabularies ---------------------------------------------------------------------------------------------------
# the 12-token toy vocabulary (eot = 12): words, word pieces, a 2-byte character split over two tokens, an invalid lead
# byte, a string with a zero byte, the empty string
TOY = [b" hello", b" world", b" thank", b" you", b" he", b"llo", b"\xc3", b"\xa9", b"\x80", b"a\x00b", b"", b"x",
       b"[_EOT_]", b"[_SOT_]"]
TOY_EOT = 12
MULTI = ["é", "♪", "à", "ÿ", "é♪", " é", "àÿ", "ß", "日本", "😀", "ñ", "ü", "é♪à", "♪♪", "õ", "þ", "÷", "å", "ç", "ø"]


@functools.lru_cache(None)
def vocab(name):
    """(tokens incl. two specials after eot, eot)"""
    if name == "toy":
        return TOY, TOY_EOT
    from make_model import synthetic_vocab
    toks = synthetic_vocab()
    if name == "synthetic":
        toks = toks[:-1] if toks[-1].startswith(b"<|") else toks
        return toks + [b"[_EOT_]", b"[_SOT_]", b"[_TT_1]"], len(toks)
    assert name == "multi"
    toks = toks[:2000] + [m.encode() for m in MULTI]
    return toks + [b"[_EOT_]", b"[_SOT_]"], len(toks)


VOCABS = ["toy", "synthetic", "multi"]

# ---- grammars -------------------------------------------------------------------------------------------------------
AZ = cls((ord("a"), ord("z")))
D09 = cls((ord("0"), ord("9")))
HI = cls((ord("à"), ord("ÿ")))
GRAMMARS = {
    # root ::= " hello" " world" | " thank" " you"
    "G1": ([rule(lit(" hello world"), lit(" thank you"))], 0),
    # root ::= (" " [a-z]+)+
    "G2": ([rule(ref(1) + ref(0), ref(1)), rule(lit(" ") + ref(2)), rule(AZ + ref(2), AZ)], 0),
    # root ::= [^a-z0-9]* | "x" root   (a nullable, right-recursive start)
    "G3": ([rule(ref(1), lit("x") + ref(0)),
            rule(cls((ord("a"), ord("z")), (ord("0"), ord("9")), neg=True) + ref(1), [])], 0),
    # root ::= expr; expr ::= term ("+" term)*; term ::= [0-9]+ | "(" expr ")"
    "G4": ([rule(ref(1)), rule(ref(2) + ref(3)), rule(ref(4), lit("(") + ref(1) + lit(")")),
            rule(lit("+") + ref(2) + ref(3), []), rule(D09 + ref(4), D09)], 0),
    # root ::= "é♪" [à-ÿ]+
    "G5": ([rule(lit("é♪") + ref(1)), rule(HI + ref(1), HI)], 0),
}
SENTENCES = {"G1": " hello world", "G2": " the cat sat", "G3": "xx!? .", "G4": "(1+2)+34", "G5": "é♪àÿé"}
# root ::= [\x01-\U0010FFFF]*
ACCEPT_ALL = ([rule(cls((1, 0x10FFFF)) + ref(0), [])], 0)

INVALID = {
    "null_rule": ([rule(lit("a")), None], 0),
    "start_out_of_range": ([rule(lit("a"))], 1),
    "ref_out_of_range": ([rule(ref(3))], 0),
    "rng_upper_after_ref": ([rule(ref(1) + [(gr.CHAR_RNG_UPPER, 99)]), rule(lit("a"))], 0),
    "rng_upper_first": ([rule([(gr.CHAR_RNG_UPPER, 99)])], 0),
    "char_alt_first": ([rule([(gr.CHAR_ALT, 99)])], 0),
    "char_alt_after_alt": ([rule(lit("a"), [(gr.CHAR_ALT, 99)])], 0),
    "left_recursive": ([rule(ref(0) + lit("a"), lit("a"))], 0),
    "left_recursive_through_nullable": ([rule(ref(1) + ref(0) + lit("x"), lit("y")), rule([], lit("z"))], 0),
    "left_recursive_indirect": ([rule(ref(1)), rule(ref(2) + lit("b")), rule(ref(0), lit("c"))], 0),
}


def tokenize(toks, eot, data):
    """Greedy longest-prefix token ids of `data` over ids < eot, or None when it cannot be covered."""
    by_first = {}
    for i in range(eot):
        if toks[i]:
            by_first.setdefault(toks[i][0], []).append(i)
    out = []
    while data:
        best = max((i for i in by_first.get(data[0], []) if data.startswith(toks[i])), key=lambda i: len(toks[i]), default=None)
        if best is None:
            return None
        out.append(best)
        data = data[len(toks[best]):]
    return out


def prefixes(vname, gname):
    """The accepted-token lists whose states the tests ask about: 0, 1, 3 and all tokens of the grammar's valid sentence
    (as far as the vocabulary spells it), and one violating token (the first id the init state rejects): empty stacks."""
    toks, eot = vocab(vname)
    rules, start = GRAMMARS[gname]
    ids = tokenize(toks, eot, SENTENCES[gname].encode()) or []
    out = []
    for n in (0, 1, 3, len(ids)):
        if n <= len(ids) and ids[:n] not in out:
            out.append(ids[:n])
    init = gr.State(rules, start).reject(toks, eot)
    bad = next((i for i in range(eot) if init[i]), None)
    if bad is not None:
        out.append([bad])
    return out


@functools.lru_cache(None)
def ref_words(vname, gname, prefix):
    """The reference's mask words (a tuple) of the state after `prefix` (a tuple of ids), and the state."""
    toks, eot = vocab(vname)
    rules, start = GRAMMARS[gname]
    st = gr.State(rules, start)
    for i in prefix:
        st.accept_token(toks[i])
    return tuple(gr.pack(st.reject(toks, eot))), st
