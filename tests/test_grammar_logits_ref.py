"""tests/grammar_logits_cases.py on the CPU: every row of the kernels' grammar test makes the point it was designed for in
the float64 reference (tests/grammar_logits_ref.py) and is decided by logits_cases.MIN_GAP, with and without the
grammar. The reference itself is checked against a log-softmax written out here."""
import math

import numpy as np
import pytest

import grammar_logits_cases as glc
import grammar_logits_ref as glr
import logits_cases as lc
import logits_ref as lr

V = 51865


@pytest.fixture(scope="module")
def sets():
    return glc.cases(V)


def test_reference_is_a_second_log_softmax():
    v = lc.vocab(V)
    rng = np.random.default_rng(3)
    raw = rng.normal(0, 1, V).astype(np.float32)
    raw[v["beg"]:] -= 6.0
    c = dict(lc.states())["text,text"]
    gram = rng.random(V) < 0.3
    got = glr.process(raw, c, v, None, gram, 2.5)
    assert got["gram_applied"] and not got["ts_fired"]
    x = lr.masked(raw, c, v)
    pen = gram.copy()
    pen[v["eot"] + 1:] = False
    x[pen] -= 2.5
    fin = np.isfinite(x)
    lse = math.log(np.exp(x[fin]).sum())
    assert np.allclose(got["logprobs"][fin], x[fin] - lse, rtol=0, atol=1e-12)
    assert (got["logprobs"][~fin] == -np.inf).all()
    assert got["id"] == int(np.argmax(np.where(fin, x, -np.inf)))
    assert abs(got["probs"].sum() - 1.0) < 1e-12
    # bits above eot change nothing; no mask and penalty 0 are the plain result
    g2 = gram.copy()
    g2[v["eot"] + 1:] = ~g2[v["eot"] + 1:]
    assert (glr.process(raw, c, v, None, g2, 2.5)["logprobs"] == got["logprobs"]).all()
    plain = glr.process(raw, c, v)
    assert not plain["gram_applied"] and plain["id"] == lr.process(raw, c, v)["id"]
    assert np.allclose(glr.process(raw, c, v, None, gram, 0.0)["logprobs"][fin], plain["logprobs"][fin], rtol=0, atol=1e-12)
    # a denied token stays at -inf under the penalty
    deny = np.zeros(V, bool)
    deny[got["id"]] = True
    d = glr.process(raw, c, v, deny, gram, 2.5)
    assert d["logprobs"][got["id"]] == -np.inf and d["id"] != got["id"]


@pytest.mark.parametrize("pen", glc.PENALTIES)
def test_rows_make_their_points(sets, pen):
    v = lc.vocab(V)
    eot = v["eot"]
    rows = sets[pen]
    assert len(rows) == glc.N_ROWS and {r["design"] for r in rows} == set(glc.DESIGNS)
    assert {r["ctl"]["temperature"] for r in rows} == set(lc.TEMPS)
    for r in rows:
        plain, ref, d = r["plain"], r["ref"], r["design"]
        assert lc._decided(plain, None, lc.MIN_GAP) and lc._decided(ref, None, lc.MIN_GAP), r["what"]
        assert r["gram"][eot + 1:].any() or d == "zero"
        if d == "ts":
            assert plain["ts_fired"] and not ref["gram_applied"] and ref["id"] == plain["id"] >= v["beg"]
            assert ref["plog"] == plain["plog"]
            continue
        assert ref["gram_applied"] and not ref["ts_fired"], r["what"]
        if d == "flip":
            assert plain["id"] == glc.A_TOK and r["gram"][glc.A_TOK] and not r["gram"][glc.B_TOK]
            if pen == 100.0:
                assert ref["id"] == glc.B_TOK  # the argmax moves to an accepted token
            else:
                assert ref["id"] == glc.A_TOK and ref["plog"] < plain["plog"] - 0.1  # still wins, its plog moves
        elif d == "eot":
            assert plain["id"] == eot and r["gram"][eot]
            assert (ref["id"] == glc.B_TOK) if pen == 100.0 else (ref["id"] == eot and ref["plog"] < plain["plog"] - 0.1)
        elif d == "zero":
            assert ref["id"] == plain["id"] and ref["plog"] == pytest.approx(plain["plog"], abs=1e-12)
        else:
            assert d == "all" and plain["id"] == glc.A_TOK
            # (penalty 100 leaves the timestamps on top: the rule is soft, it does not ask the timestamp rule again)
            assert (ref["id"] >= v["beg"]) if pen == 100.0 else (ref["id"] == glc.A_TOK)
            assert ref["ptsum"] > plain["ptsum"]  # the timestamps gain what the text loses
