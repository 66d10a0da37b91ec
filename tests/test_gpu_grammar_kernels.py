"""kernels/grammar.hip (the reject kernel, with its host fallback) through whisper_mi355x_debug_grammar_reject against
tests/grammar_ref.py bit for bit: G1-G5 with 1, 3 and 17 rows, a different state per row (init, mid-sentence, a
complete sentence that allows EOT, a violated grammar without stacks, a pending partial character); the states of G1,
G2, G4 and G5 must be decided by the kernel (flag 0), the pending partial by the host (flag 2); a rule with more
alternates than the kernel's stacks per token is flagged (flag 1) and patched to the reference's bits.

kernels/logits.hip with the grammar's reject words (whisper_full_params.grammar_rules) through
whisper_mi355x_debug_logits_gram / whisper_mi355x_debug_logits_topk_gram against tests/grammar_logits_ref.py (float64),
and whisper_mi355x_grammar_mask against tests/grammar_ref.py on the context's own token strings. The micro shape's
context (n_vocab 51865).

tests/grammar_logits_cases.py (held on the CPU by tests/test_grammar_logits_ref.py): 17 rows per penalty (100 and 0.5) of
five designs (a rejected leader that an accepted token overtakes under penalty 100 and that still wins under 0.5; the
timestamp mass winning, where the rule does not run; EOT leading with its bit set; an all-zero mask; everything
rejected), at temperatures 0 / 0.2 / 1.0, launched as 1, 16 and 17 rows (a grammar launch always takes the
one-workgroup-per-row form, whatever `form` says), with and without a deny mask.

Per row: id and tid exact; the probs rows 0 / -inf exactly on the reference's suppressed set and finite elsewhere; the
record's p / plog are the probs rows' entries; the rest within test_gpu_logits_rules.py's bars for its "unit" rows and
the project's PLOG_BAR / P_REL_BAR at temperature 0 (imported: the second log-softmax is the first one's arithmetic).
Rows where the timestamp rule fired equal the _deny hook's bit for bit. Top-k, k = 5: candidate 0 is the greedy record bit
for bit, the ids are the reference's in its order. gram == NULL through the new hooks gives the _deny hooks' bits.
"""
import ctypes as C
import json

import numpy as np
import pytest

import beam_ref as br
import grammar_cases as gc
import grammar_logits_cases as glc
import grammar_logits_ref as glr
import grammar_ref as gr
import logits_cases as lc
import logits_ref as lr
import suppress_cases as sc
import suppress_ref as sr
from conftest import model_path
from test_gpu_beam_kernels import P_REL_BAR, PLOG_BAR, Dev
from test_gpu_logits_rules import BARS, rel, seq_ctl

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)
RULE_FIELDS = ("is_initial", "last_ts", "penult_ts", "has_ts", "seek_delta", "suppress_blank", "no_timestamps", "suppress_eot",
               "tid0_initial", "want_nosp")


@pytest.fixture(scope="module")
def ctx(wrs):
    c = wrs.WhisperContext(model_path("micro"), dtype=wrs.F16)
    yield c
    c.close()


def up(a):
    return None if a is None else a.ctypes.data_as(UP)


def launch(wrs, ctx, rows, form, deny_words, gram_words, penalty, hook="gram"):
    L = wrs.lib()
    n = len(rows)
    V = L.whisper_n_vocab(ctx.ptr)
    ctl = (wrs.SeqCtl * n)(*[seq_ctl(wrs, r["ctl"]) for r in rows])
    out = (wrs.Cand * n)()
    probs = np.zeros((n, 2, V), np.float32)
    d = Dev(wrs, ctx)
    try:
        raw = d.up(np.stack([r["raw"] for r in rows]))
        if hook == "gram":
            rc = L.whisper_mi355x_debug_logits_gram(ctx.ptr, raw, n, ctl, form, out, probs.ctypes.data_as(FP), up(deny_words),
                                                    up(gram_words), penalty)
        else:
            rc = L.whisper_mi355x_debug_logits_deny(ctx.ptr, raw, n, ctl, form, out, probs.ctypes.data_as(FP), up(deny_words))
        assert rc == 0
    finally:
        d.free()
    return out, probs


def deny_of(V, rows):
    """A deny mask that takes nothing a row's point needs: random 1 % without the designs' tokens and EOT."""
    deny = np.random.default_rng(11).random(V) < 0.01
    deny[[glc.A_TOK, glc.B_TOK, lc.vocab(V)["eot"]]] = False
    return deny


@pytest.mark.parametrize("with_deny", [False, True], ids=["no-deny", "deny"])
@pytest.mark.parametrize("n", [1, 16, 17])
@pytest.mark.parametrize("pen", glc.PENALTIES)
def test_gram(wrs, ctx, pen, n, with_deny):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    rows = glc.cases(V)[pen][:n] if n > 1 else glc.cases(V)[pen][:1]
    deny = deny_of(V, rows) if with_deny else None
    dw = None if deny is None else sr.words(deny)
    out, probs = launch(wrs, ctx, rows, 1, dw, glc.words(rows, V), pen)
    plain_out, plain_probs = launch(wrs, ctx, rows, 0, dw, None, 0.0, hook="deny")  # (form 0: one workgroup per row)
    bars = BARS["unit"]
    w = dict.fromkeys(("plog_0", "p_0") + tuple(bars), 0.0)
    for r, row in enumerate(rows):
        c, g = row["ctl"], out[r]
        ref = glr.process(row["raw"], c, v, deny, row["gram"], pen) if with_deny else row["ref"]
        where = f"penalty {pen} n {n} deny {with_deny} row {r} ({row['what']})"
        assert sc.decided(ref), where
        assert (g.id, g.tid) == (ref["id"], ref["tid"]), where
        assert g.pad == 0.0 and g.no_speech_prob == 0.0, where
        if not ref["gram_applied"]:  # the timestamp mass won: the launch without the grammar, bit for bit
            assert row["design"] == "ts"
            assert bytes(g) == bytes(plain_out[r]) and probs[r].tobytes() == plain_probs[r].tobytes(), where
        t = "t" if c["temperature"] > 0 else "0"
        assert np.isfinite(g.plog), where
        w["plog_" + t] = max(w["plog_" + t], abs(g.plog - ref["plog"]))
        w["p_" + t] = max(w["p_" + t], abs(g.p / ref["p"] - 1.0))
        w["pt"] = max(w["pt"], rel(g.pt, ref["pt"]))
        w["ptsum"] = max(w["ptsum"], rel(g.ptsum, ref["ptsum"]))
        if not c["want_probs"]:
            assert np.isnan(probs[r]).all(), f"{where}: the probs row of a row without want_probs was written"
            continue
        p, lp = probs[r, 0], probs[r, 1]
        sup = ref["suppressed"]
        assert ((lp == -np.inf) == sup).all(), f"{where}: {int(((lp == -np.inf) != sup).sum())} ids off the suppressed set"
        assert (p[sup] == 0.0).all() and np.isfinite(lp[~sup]).all() and np.isfinite(p).all() and (p >= 0.0).all(), where
        w["lp_row"] = max(w["lp_row"], lr.lp_err(lp, ref["logprobs"]))
        w["p_row"] = max(w["p_row"], float(np.abs(p.astype(np.float64) - ref["probs"]).max()))
        w["sum_p"] = max(w["sum_p"], abs(float(p.astype(np.float64).sum()) - float(ref["probs"].sum())))
        assert (p[g.id], lp[g.id]) == (g.p, g.plog), f"{where}: the record is not the probs row's entry"
    print("grammar-kernels worst " + json.dumps(dict(penalty=pen, n=n, deny=with_deny, **w)))
    assert w["plog_0"] <= PLOG_BAR and w["p_0"] <= P_REL_BAR, w
    over = {k: (w[k], bar) for k, bar in bars.items() if not w[k] <= bar}
    assert not over, f"rows over their bars (measured, bar): {over}"


def topk(wrs, ctx, rows, k, split, deny_words, gram_words, penalty, hook="gram"):
    L = wrs.lib()
    n = len(rows)
    rules = np.array([[r["ctl"][f] for f in RULE_FIELDS] for r in rows], np.int32)
    cand, greedy = (wrs.Cand * (n * k))(), (wrs.Cand * n)()
    d = Dev(wrs, ctx)
    try:
        raw = d.up(np.stack([r["raw"] for r in rows]))
        ip = rules.ctypes.data_as(C.POINTER(C.c_int))
        if hook == "gram":
            rc = L.whisper_mi355x_debug_logits_topk_gram(ctx.ptr, raw, n, ip, None, k, split, cand, greedy, up(deny_words),
                                                         up(gram_words), penalty)
        else:
            rc = L.whisper_mi355x_debug_logits_topk_deny(ctx.ptr, raw, n, ip, None, k, split, cand, greedy, up(deny_words))
        assert rc == 0
    finally:
        d.free()
    return cand, greedy


@pytest.mark.parametrize("with_deny", [False, True], ids=["no-deny", "deny"])
@pytest.mark.parametrize("n", [1, 16, 17])
@pytest.mark.parametrize("pen", glc.PENALTIES)
def test_topk_gram(wrs, ctx, pen, n, with_deny):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    k = sc.K_TOP
    # top-k rows are t = 0 rows: the designs at temperature 0 (the raw rows of t > 0 rows were scaled for their t)
    rows = [dict(r, ctl=dict(r["ctl"], want_probs=0)) for r in glc.cases(V)[pen] if r["ctl"]["temperature"] == 0.0]
    rows = (rows * 4)[:n]
    deny = deny_of(V, rows) if with_deny else None
    dw = None if deny is None else sr.words(deny)
    cand, greedy = topk(wrs, ctx, rows, k, 1, dw, glc.words(rows, V), pen)
    worst_plog = worst_p = 0.0
    checked = 0
    for r, row in enumerate(rows):
        got = [cand[r * k + j] for j in range(k)]
        where = f"penalty {pen} n {n} deny {with_deny} row {r} ({row['what']})"
        assert bytes(got[0]) == bytes(greedy[r]), f"{where}: candidate 0 is not the greedy record"
        ref = glr.process(row["raw"], row["ctl"], v, deny, row["gram"], pen)
        assert (greedy[r].id, greedy[r].tid) == (ref["id"], ref["tid"]), where
        if not sc.topk_decided(ref["logprobs"], ref, k):
            continue
        checked += 1
        want = br.candidates(ref["logprobs"], k, v)
        assert [g.id for g in got] == [c["id"] for c in want] + [-1] * (k - len(want)), where
        for g, c in zip(got, want):
            assert g.tid == c["tid"], where
            worst_plog = max(worst_plog, abs(g.plog - c["plog"]))
            worst_p = max(worst_p, abs(g.p / c["p"] - 1.0))
    print(f"grammar-topk penalty {pen} n {n} deny {with_deny}: worst |dplog| {worst_plog:.3e}, worst |dp/p| {worst_p:.3e}, "
          f"rows compared {checked} of {n}")
    assert checked >= (n + 1) // 2
    assert worst_plog <= PLOG_BAR and worst_p <= P_REL_BAR


@pytest.mark.parametrize("with_deny", [False, True], ids=["no-deny", "deny"])
@pytest.mark.parametrize("form,n", [(0, 16), (1, 16), (1, 17)])
def test_null_gram_is_the_deny_hook(wrs, ctx, form, n, with_deny):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    rows = glc.cases(V)[100.0][:n]
    dw = sr.words(deny_of(V, rows)) if with_deny else None
    old = launch(wrs, ctx, rows, form, dw, None, 0.0, hook="deny")
    new = launch(wrs, ctx, rows, form, dw, None, 100.0)
    assert bytes(new[0]) == bytes(old[0]) and new[1].tobytes() == old[1].tobytes()
    t0 = [dict(r, ctl=dict(r["ctl"], temperature=0.0, want_probs=0)) for r in rows]
    a = topk(wrs, ctx, t0, sc.K_TOP, form, dw, None, 0.0, hook="deny")
    b = topk(wrs, ctx, t0, sc.K_TOP, form, dw, None, 100.0)
    assert (bytes(a[0]), bytes(a[1])) == (bytes(b[0]), bytes(b[1]))


def test_grammar_mask_on_the_contexts_tokens(wrs, ctx):
    """whisper_mi355x_grammar_mask against grammar_ref over whisper_token_to_str of every id: G1-G5 in the states of
    tests/grammar_cases.py; the [_...] specials above eot are never set; invalid grammars give -9."""
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    eot = L.whisper_token_eot(ctx.ptr)
    toks = [ctx.token_str(i) for i in range(V)]
    assert all(t.startswith(b"[_") for t in toks[eot:])
    n_states = 0
    for gname, (rules, start) in gc.GRAMMARS.items():
        ids = gc.tokenize(toks, eot, gc.SENTENCES[gname].encode())
        assert ids, gname
        init = gr.State(rules, start).reject(toks, eot)
        bad = next(i for i in range(1, eot) if init[i])
        for prefix in ([], ids[:1], ids[:3], ids, [bad], ids[:1] + [eot + 1, V - 1]):
            st = gr.State(rules, start)
            for i in prefix:
                st.accept_token(toks[i])
            want = np.array(st.reject(toks, eot))
            got = ctx.grammar_mask(rules, start, prefix)
            assert (got == want).all(), (gname, prefix, np.nonzero(got != want)[0][:8])
            assert not got[eot + 1:].any()
            n_states += 1
        assert ctx.grammar_mask(rules, start, [bad]).sum() == 0  # empty stacks: all zeros
    assert n_states == 30
    assert ctx.grammar_mask(*gc.ACCEPT_ALL, []).sum() == len([t for t in toks[:eot] if t and gr.token_rejected(
        gc.ACCEPT_ALL[0], gr.init(*gc.ACCEPT_ALL), (0, 0), t)])
    for name, (rules, start) in gc.INVALID.items():
        assert ctx.grammar_mask(rules, start, []) == wrs.GRAMMAR_ERR, name
    w = np.zeros(4, np.uint32)
    arrs = wrs.grammar_arrays(gc.GRAMMARS["G1"][0])
    assert L.whisper_mi355x_grammar_mask(ctx.ptr, C.cast(arrs[0], C.c_void_p), 1, 0, None, 0, up(w), 4) == -1


# ---- the reject kernel --------------------------------------------------------------------------------------------------
LEAD_C3 = 0xC3  # the single-byte token 0xC3: no code point, a pending partial (3, 1)


def reject_states(toks, eot, gname):
    """[(accepted ids, what)] of a grammar: init, 1 and 3 (or a few more) tokens into its sentence, the whole sentence (EOT allowed), one
    violating token (no stacks), and the lead byte of a 2-byte character (a pending partial)."""
    rules, start = gc.GRAMMARS[gname]
    ids = gc.tokenize(toks, eot, gc.SENTENCES[gname].encode())
    assert ids and len(ids) >= 2, gname
    init = gr.State(rules, start).reject(toks, eot)
    bad = next(i for i in range(1, eot) if init[i])

    def whole(k):  # the shortest prefix of at least k tokens that ends on a character boundary (G5: single-byte tokens)
        while ref_state(toks, (rules, start), ids[:k]).partial != (0, 0):
            k += 1
        return ids[:k]

    return [([], "init"), (whole(1), "mid"), (whole(3), "mid"), (ids, "eot"), ([bad], "empty"), ([LEAD_C3], "partial")]


def ref_state(toks, grammar, prefix):
    st = gr.State(*grammar)
    for i in prefix:
        st.accept_token(toks[i])
    return st


@pytest.fixture(scope="module")
def ctx_tokens(wrs, ctx):
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    toks = [ctx.token_str(i) for i in range(V)]
    assert toks[0] == b""  # (a C string ends at a NUL: token 0 is the byte 0, a non-empty string without a code point)
    toks[0] = b"\x00"
    return toks, L.whisper_token_eot(ctx.ptr)


_REF_MASKS = {}


def ref_mask(toks, eot, gname, grammar, prefix):
    key = (gname, tuple(prefix))
    if key not in _REF_MASKS:
        st = ref_state(toks, grammar, prefix)
        _REF_MASKS[key] = (np.array(st.reject(toks, eot)), st)
    return _REF_MASKS[key]


@pytest.mark.parametrize("n_rows", [1, 3, 17])
@pytest.mark.parametrize("gname", list(gc.GRAMMARS))
def test_reject_kernel(wrs, ctx, ctx_tokens, gname, n_rows):
    toks, eot = ctx_tokens
    grammar = gc.GRAMMARS[gname]
    states = reject_states(toks, eot, gname)
    pick = {1: [0], 3: [0, 1, 5]}.get(n_rows) or [r % len(states) for r in range(n_rows)]
    rows = [states[k] for k in pick]
    got = ctx.debug_grammar_reject(grammar[0], grammar[1], [p for p, _ in rows])
    assert not isinstance(got, int), got
    masks, flags = got
    for r, (prefix, what) in enumerate(rows):
        want, st = ref_mask(toks, eot, gname, grammar, prefix)
        assert (masks[r] == want).all(), (gname, n_rows, r, what, np.nonzero(masks[r] != want)[0][:8])
        if what == "partial":
            assert st.partial == (3, 1) and st.stacks and flags[r] == 2, (gname, r, flags[r])
        elif what == "empty":
            assert not st.stacks and not want.any() and flags[r] == 0, (gname, r, flags[r])
        else:
            assert st.stacks and st.partial == (0, 0) and want.any()
            assert gr.allow_eot(st.stacks) == (not want[eot])
            if what == "eot":
                assert gr.allow_eot(st.stacks), gname
            if gname != "G3":
                assert flags[r] == 0, f"{gname} row {r} ({what}): not decided by the kernel (flag {flags[r]})"
            assert flags[r] in (0, 1)


def test_reject_kernel_overflow_is_patched(wrs, ctx, ctx_tokens):
    """root ::= "a" x, x ::= one of ten letters: a token that starts with "a" leaves ten stacks, more than the kernel's
    eight per token, so the row is flagged and the host's words replace the kernel's; a row of a grammar within the
    bounds next to it in another launch is not."""
    toks, eot = ctx_tokens
    from grammar_ref import lit, ref, rule
    wide = [rule(lit("a") + ref(1)), rule(*[lit(ch) for ch in "bcdefghijk"])]
    assert gr.validate(wide, 0) == 0
    a = toks.index(b"a")
    masks, flags = ctx.debug_grammar_reject(wide, 0, [[], [a], []])
    assert flags[0] == 1 and flags[2] == 1, flags  # init: the tokens "a", "ab", ... overflow
    assert flags[1] == 0, flags  # after "a": ten row stacks (within a row's 32), every token takes one step
    for r, prefix in enumerate([[], [a], []]):
        st = ref_state(toks, (wide, 0), prefix)
        want = np.array(st.reject(toks, eot))
        assert (masks[r] == want).all(), (r, np.nonzero(masks[r] != want)[0][:8])
    assert not masks[0][a] and not masks[0][toks.index(b"ab")] and masks[0][toks.index(b"b")]
