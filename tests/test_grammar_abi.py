"""whisper_rs.py's grammar helpers on the CPU: the ctypes arrays of a Python rule list have whisper_grammar_element's layout,
and FullParams' setters (whisper-rs set_grammar / set_start_rule / set_grammar_penalty) fill the struct's fields and keep
the arrays alive."""
import ctypes as C
import gc as pygc

import grammar_cases as gc
import grammar_ref as gr


def test_element_layout_and_constants(wrs):
    assert C.sizeof(wrs.GrammarElement) == 8 and wrs.GrammarElement.value.offset == 4
    assert (wrs.GRETYPE_END, wrs.GRETYPE_ALT, wrs.GRETYPE_RULE_REF, wrs.GRETYPE_CHAR, wrs.GRETYPE_CHAR_NOT,
            wrs.GRETYPE_CHAR_RNG_UPPER, wrs.GRETYPE_CHAR_ALT) == (gr.END, gr.ALT, gr.RULE_REF, gr.CHAR, gr.CHAR_NOT,
                                                                 gr.CHAR_RNG_UPPER, gr.CHAR_ALT)
    assert wrs.GRAMMAR_ERR == gr.GRAMMAR_ERR == -9


def test_grammar_arrays(wrs):
    rules = gc.GRAMMARS["G4"][0]
    ptrs, elems = wrs.grammar_arrays(rules)
    assert len(ptrs) == len(rules)
    for r, rule in enumerate(rules):
        assert [(ptrs[r][k].type, ptrs[r][k].value) for k in range(len(rule))] == rule
    ptrs, elems = wrs.grammar_arrays(gc.INVALID["null_rule"][0])
    assert bool(ptrs[0]) and not bool(ptrs[1])  # a None rule is a null pointer


def test_setters(wrs):
    p = wrs.reference_full_params("en")
    assert not p.grammar_rules and p.n_grammar_rules == 0 and p.i_start_rule == 0 and p.grammar_penalty == 100.0
    rules, start = gc.GRAMMARS["G2"]
    p.set_grammar(rules, start)
    pygc.collect()
    assert p.n_grammar_rules == len(rules) and p.i_start_rule == start
    arr = C.cast(p.grammar_rules, C.POINTER(C.POINTER(wrs.GrammarElement)))
    for r, rule in enumerate(rules):
        assert [(arr[r][k].type, arr[r][k].value) for k in range(len(rule))] == rule
    p.set_start_rule(2)
    p.set_grammar_penalty(12.5)
    assert p.i_start_rule == 2 and p.grammar_penalty == 12.5
    p.set_grammar(None)
    assert not p.grammar_rules and p.n_grammar_rules == 0 and p.i_start_rule == 0
