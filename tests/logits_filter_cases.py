"""The rows of the logits_filter_callback tests (tests/test_logits_filter_ref.py on the CPU,
tests/test_gpu_logits_filter_kernels.py on the device): per vocabulary two sets of 17 rows (16 + 1: the 17th row puts the
launcher past its split-form limit), one per value of the launch's tdrz flag. A row is a raw N(0, 6^2) logits row, a
SeqCtl (the rule states of logits_cases.states() but "all masked", the temperatures of logits_cases.TEMPS in turn), the
row after logits_filter_ref.pre and one edit a callback could make, and the reference's answer for the edited row
(logits_filter_ref.post). The edits, in turn:
    ban 1      the reference's best token of the unedited row set to -inf
    ban 8      its best 8
    boost      +5 on its runner-up, which then wins by ~5 - (the old gap)
    solm       row[solm] += 1e4: with tdrz the token wins with p = 1; without, -inf + 1e4 changes nothing
    all -inf   every entry -inf: the row without a token (id 0, p 0, plog -inf)
    tie        two text ids set to the same value 5 above the maximum: the lower id wins
A row's seed is the first of its series whose edited row is decided by logits_cases.MIN_GAP in the reference (or is the
planted tie), by logits_cases' own test; nothing here looks at a kernel.
"""
import numpy as np

import logits_cases as lc
import logits_filter_ref as fr

EDITS = ("ban 1", "ban 8", "boost", "solm", "all -inf", "tie")
TIE_IDS = (300, 7000)  # two chunks of the split form


def edit(kind: str, f, ref0: dict, v: dict):
    """The filtered row f (float32, edited in place) as a callback of this kind leaves it; ref0: the reference's answer
    for the unedited row. Returns the tie class for logits_cases._decided."""
    order = np.argsort(-ref0["logprobs"], kind="stable")
    if kind == "ban 1":
        f[order[:1]] = -np.inf
    elif kind == "ban 8":
        f[order[:8]] = -np.inf
    elif kind == "boost":
        f[order[1]] += np.float32(5.0)
    elif kind == "solm":
        f[v["solm"]] += np.float32(1e4)
    elif kind == "all -inf":
        f[:] = -np.inf
    elif kind == "tie":
        f[list(TIE_IDS)] = np.float32(f[np.isfinite(f)].max() + 5.0)
        return "top"
    else:
        raise AssertionError(kind)
    return None


def _row(V: int, v: dict, c: dict, tdrz: bool, kind: str, seed: int) -> dict:
    for attempt in range(50):
        rng = np.random.default_rng(seed + 1000 * attempt)
        raw = rng.normal(0.0, 6.0, V).astype(np.float32)
        f = fr.pre(raw, c, v, tdrz)
        ref0 = fr.post(f, raw, c, v)
        if np.isfinite(ref0["logprobs"]).sum() < 16:
            continue
        tie = edit(kind, f, ref0, v)
        ref = fr.post(f, raw, c, v)
        if lc._decided(ref, tie):
            return dict(raw=raw, ctl=c, tdrz=tdrz, filtered=f, ref=ref, ref0=ref0, what=kind, tie=tie, scale="unit")
    raise AssertionError(f"no decided row for {kind}")


def build_vocab(V: int) -> dict:
    """{tdrz: [17 rows]}"""
    v = lc.vocab(V)
    st = [c for name, c in lc.states() if name != "all masked"]
    sets = {}
    for tdrz in (False, True):
        rows = []
        for r in range(17):
            t = lc.TEMPS[(r + int(tdrz)) % 3]
            c = lc._with_temp(st[(r + 3 * int(tdrz)) % len(st)], t)
            if r % 5 == 3:
                c["want_nosp"] = 1
            kind = EDITS[r % len(EDITS)]
            if kind == "tie":  # (a text-token tie needs a state that keeps the text tokens)
                c = lc._with_temp(dict(st[2], want_nosp=c["want_nosp"]), t)
            rows.append(_row(V, v, c, tdrz, kind, 700000 + 50000 * int(tdrz) + 17 * r + V % 7))
        sets[tdrz] = rows
    return sets


_BUILT = {}


def matrix(V: int) -> dict:
    if V not in _BUILT:
        _BUILT[V] = build_vocab(V)
    return _BUILT[V]
