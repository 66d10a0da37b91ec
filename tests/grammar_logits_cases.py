"""Rows for the logits kernels' grammar rule, shared by tests/test_grammar_logits_ref.py (CPU: every row
makes its point and is decided) and tests/test_gpu_grammar_kernels.py. No test lives here.

A case set is 17 rows under one penalty (a launch argument): the designs below in turn, at temperatures 0, 0.2 and 1.0
(t > 0 rows ask for their probs rows). Every mask also has random bits above eot, which the rule must ignore.
  flip   a rejected text token leads an accepted one by 2 nats: penalty 100 moves the argmax, penalty 0.5 does not
  ts     the timestamp mass beats the best text token (logits_cases._mass_row): the rule does not run
  eot    EOT leads and its bit is set (the grammar may not end here)
  zero   an all-zero mask
  all    every text token and EOT rejected: the order among them stays, the timestamps gain (and lead under penalty 100)
"""
import numpy as np

import grammar_logits_ref as glr
import logits_cases as lc
import logits_ref as lr

N_ROWS = 17
DESIGNS = ("flip", "ts", "eot", "zero", "all")
PENALTIES = (100.0, 0.5)
A_TOK, B_TOK = 1000, 2000  # the rejected leader and the accepted runner-up of "flip"


def _make(design, rng, V, v, c, t):
    beg, eot = v["beg"], v["eot"]
    gram = np.zeros(V, bool)
    gram[eot + 1:] = rng.random(V - eot - 1) < 0.5  # ignored by the rule
    scale = t if t > 0 else 1.0
    if design == "ts":
        x = lc._mass_row(rng, V, v, c, +1, t)
        gram[:eot + 1] = True
        return x, gram
    x = rng.normal(0.0, 1.0, V)
    x[beg:] -= 6.0  # little timestamp mass: the rule runs
    if design == "flip":
        x[A_TOK], x[B_TOK] = 8.0, 6.0
        gram[:eot] = rng.random(eot) < 0.5
        gram[A_TOK], gram[B_TOK] = True, False
    elif design == "eot":
        x[eot], x[B_TOK] = 9.0, 6.0
        gram[:eot] = rng.random(eot) < 0.5
        gram[eot], gram[B_TOK] = True, False
    elif design == "all":
        x[A_TOK] = 8.0
        gram[:eot + 1] = True
    else:
        assert design == "zero"
        x[A_TOK] = 8.0
        gram[:] = False
    return x * scale, gram


_BUILT = {}


def cases(V: int) -> dict:
    """{penalty: [17 x dict(raw, ctl, gram, design, what, plain, ref)]}: plain = the reference without the grammar, ref =
    with it. Every row is decided (logits_cases.MIN_GAP) in both."""
    if V in _BUILT:
        return _BUILT[V]
    v = lc.vocab(V)
    base = dict(lc.states())["text,text"]
    out = {}
    for pen in PENALTIES:
        rows = []
        for r in range(N_ROWS):
            design = DESIGNS[r % len(DESIGNS)]
            t = lc.TEMPS[(r // len(DESIGNS)) % 3]
            c = lc._with_temp(base, t)
            for attempt in range(50):
                rng = np.random.default_rng(7000 + 100 * r + 10000 * attempt)
                raw, gram = _make(design, rng, V, v, c, t)
                raw = np.asarray(raw, np.float32)
                plain = glr.process(raw, c, v)
                ref = glr.process(raw, c, v, None, gram, pen)
                if lc._decided(plain, None) and lc._decided(ref, None):
                    break
            else:
                raise AssertionError(f"no decided row {r} ({design})")
            rows.append(dict(raw=raw, ctl=c, gram=gram, design=design, what=f"{design} t={t}", plain=plain, ref=ref))
        out[pen] = rows
    _BUILT[V] = out
    return out


def words(rows, V):
    """The rows' masks as the hooks take them: uint32 [n][(V + 31) // 32]."""
    W = (V + 31) // 32
    bits = np.zeros((len(rows), W * 32), np.uint8)
    for r, row in enumerate(rows):
        bits[r, :V] = row["gram"]
    return np.packbits(bits.reshape(len(rows), W, 32), axis=2, bitorder="little").view("<u4").reshape(len(rows), W).copy()
