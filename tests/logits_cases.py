"""The input matrix of the logits-rule tests (tests/test_logits_ref.py on the CPU, tests/test_gpu_logits_rules.py on
the device): per vocabulary 9 sets of 16 rows + 1 (the 17th row puts the launcher past its split-form limit), every
row a raw logits row, a SeqCtl and what the row is built to show. Built once per vocabulary, with the float64
reference's answer for every row (tests/logits_ref.py); nothing here looks at a kernel.

A row's seed is the first of its series whose reference answer is decided by MIN_GAP (top-2 gap, timestamp-rule gap,
the gap between the two best timestamps) and whose best timestamp's probability is clear of float's underflow (the
oracle's expf keeps denormals, the device's exp2 flushes them: tid of such a row is 0 on one side and a timestamp on
the other, and neither is wrong).
"""
import math

import numpy as np

import beam_ref as br
import logits_ref as lr
from make_model import synthetic_vocab

MIN_GAP = 1e-3
# the N(0, 30^2) rows are held to a larger gap: at t = 0.2 their log-sum-exp is ~650, a float there is a multiple of
# 6.1e-5, and the kernels' bars for these rows (4 x the measured error, tests/test_gpu_logits_rules.py) follow from it
WIDE_MIN_GAP = 1e-2
TEMPS = (0.0, 0.2, 1.0)
KINDS = ("random", "wide", "planted")
# float p = exp(lp) is > 0 on every implementation above, and 0 on every one below
TID_LP_CLEAR = (-80.0, -110.0)

_SPACE = None


def vocab(V: int) -> dict:
    global _SPACE
    if _SPACE is None:
        _SPACE = synthetic_vocab().index(b" ")
    return br.vocab_ids(V, _SPACE)


def states() -> list:
    c = lr.ctl
    return [
        ("initial+blank", c(is_initial=1, penult_ts=1, suppress_blank=1, tid0_initial=50, want_nosp=1)),
        ("initial", c(is_initial=1, penult_ts=1, suppress_blank=0, tid0_initial=-1)),
        ("text,text", c()),
        ("text,ts", c(last_ts=1, penult_ts=0, has_ts=1, seek_delta=20)),
        ("ts,ts", c(last_ts=1, penult_ts=1, has_ts=1, seek_delta=20)),
        ("has_ts 20", c(penult_ts=1, has_ts=1, seek_delta=20)),
        ("has_ts 21", c(has_ts=1, seek_delta=21)),
        ("has_ts 2998", c(has_ts=1, seek_delta=2998)),
        ("no_timestamps", c(no_timestamps=1)),
        ("suppress_eot", c(suppress_eot=1)),
        ("all masked", c(no_timestamps=1, suppress_eot=1, last_ts=1, penult_ts=0)),
    ]


def _with_temp(c: dict, t: float) -> dict:
    c = dict(c)
    c["temperature"] = t
    c["want_probs"] = int(t > 0)
    return c


def _decided(ref: dict, tie, min_gap=MIN_GAP) -> bool:
    """tie: "top" = the row's two largest logits are equal on purpose (the top-2 gap is 0 by construction), "ts" = its
    two best timestamps are; "top+ts": both."""
    tie = tie or ""
    if ref["ts_gap"] < min_gap or ("top" not in tie and ref["top2_gap"] < min_gap):
        return False
    if TID_LP_CLEAR[1] <= ref["tid_lp"] <= TID_LP_CLEAR[0]:
        return False
    return "ts" in tie or ref["tid_lp"] < TID_LP_CLEAR[1] or ref["tid_gap"] >= min_gap


def _row(V, v, make, c, seed, what, tie=None, expect=None, scale="unit"):
    """make(rng) -> raw row; the first seed of seed, seed + 1000, ... whose row is decided."""
    for attempt in range(50):
        raw = np.asarray(make(np.random.default_rng(seed + 1000 * attempt)), np.float32)
        ref = lr.process(raw, c, v)
        if _decided(ref, tie, WIDE_MIN_GAP if scale == "wide" else MIN_GAP) and \
                (expect is None or all(ref[k] == e for k, e in expect.items())):
            return dict(raw=raw, ctl=c, ref=ref, what=what, tie=tie, expect=expect or {}, scale=scale)
    raise AssertionError(f"no decided row for {what}")


def _mass_row(rng, V, v, c, sign, t):
    """Timestamp mass against the best text token: every allowed timestamp carries moderate mass, none beats the best
    text token, and log(sum p(timestamps)) sits 4e-3 nats above (sign = +1) or below it: the sum alone decides."""
    beg = v["beg"]
    x = rng.normal(0.0, 1.0, V)
    x[1000] = 8.0
    probe = lr.masked(np.zeros(V, np.float32), dict(c, temperature=0.0), v)
    ok = np.nonzero(np.isfinite(probe[beg:]))[0] + beg
    assert ok.size > 100
    ts = rng.normal(0.0, 0.3, ok.size)
    ts[ok.size // 3] += 2.0  # the best timestamp
    m = ts.max()
    ts += 8.0 + sign * 4e-3 - (math.log(np.exp(ts - m).sum()) + m)
    assert ts.max() < 7.0
    x[ok] = ts
    return x * (t if t > 0 else 1.0)  # the kernel divides by t first


def build_vocab(V: int) -> dict:
    """{(kind, rot): [17 rows]}; row r of set (kind, rot) runs at TEMPS[(r + rot) % 3], an N(0, 30^2) row (scale
    "wide") at 0.2 or 1.0 only: its log-sum-exp is >= 128 at any temperature, where a float logprob cannot meet the
    project's absolute bar for t = 0 rows (half a float step there is 7.6e-6, the bar 6.8e-6)."""
    v = vocab(V)
    beg, eot = v["beg"], v["eot"]
    cs = (V + 15) // 16
    seam = 36 * 1024
    st = states()
    text = st[2][1]
    sets = {}
    for ki, kind in enumerate(KINDS):
        for rot in range(3):
            rows = []

            def add(make, c, what, **kw):
                r = len(rows)
                t = TEMPS[1 + (r + rot) % 2] if kw.get("scale") == "wide" else TEMPS[(r + rot) % 3]
                c = _with_temp(c, t)
                if r % 5 == 3:
                    c["want_nosp"] = 1
                seed = 100000 * ki + 10000 * rot + 17 * r + V % 7
                rows.append(_row(V, v, lambda rng: make(rng, c, t), c, seed, f"{kind}/{what}", **kw))

            if kind in ("random", "wide"):
                sd = 6.0 if kind == "random" else 30.0
                for name, c in st:
                    add(lambda rng, c, t: rng.normal(0.0, sd, V), c, name, scale="wide" if kind == "wide" else "unit",
                        expect=dict(id=0, p=0.0, plog=-math.inf, ptsum=0.0) if name == "all masked" else None)
            if kind == "random":
                def holes(rng, c, t):
                    x = rng.normal(0.0, 6.0, V)
                    x[rng.random(V) < 0.3] = -np.inf
                    return x

                def three(rng, c, t):
                    x = np.full(V, -np.inf)
                    x[[11, 4242, 40000]] = [0.5, 2.0, -1.0]
                    return x

                def no_chunk(rng, c, t):
                    x = rng.normal(0.0, 6.0, V)
                    x[cs:2 * cs] = -np.inf
                    return x

                def no_ts(rng, c, t):
                    x = rng.normal(0.0, 6.0, V)
                    x[beg:] = -np.inf
                    return x

                add(holes, text, "raw -inf 30%")
                add(holes, st[0][1], "raw -inf 30%, initial")
                add(three, text, "3 finite logits", expect=dict(id=4242))
                add(no_chunk, st[5][1], "chunk 1 raw -inf")
                add(no_ts, st[7][1], "timestamps raw -inf", expect=dict(tid=0))
            if kind == "wide":
                add(lambda rng, c, t: _mass_row(rng, V, v, c, +1, t), text, "mass above", expect=dict(ts_fired=True))
                add(lambda rng, c, t: _mass_row(rng, V, v, c, -1, t), text, "mass below", expect=dict(ts_fired=False, id=1000))
                add(lambda rng, c, t: _mass_row(rng, V, v, c, +1, t), st[6][1], "mass above, has_ts", expect=dict(ts_fired=True))
                add(lambda rng, c, t: _mass_row(rng, V, v, c, -1, t), st[6][1], "mass below, has_ts",
                    expect=dict(ts_fired=False, id=1000))
                add(lambda rng, c, t: rng.normal(0.0, 6.0, V), st[4][1], "random, ts,ts")
            if kind == "planted":
                def planted(idx):
                    def make(rng, c, t):
                        x = rng.normal(0.0, 6.0, V)
                        x[idx] = x.max() + 5.0
                        return x
                    return make

                def planted_ts(idx):
                    def make(rng, c, t):
                        x = rng.normal(0.0, 6.0, V)
                        x[idx] = x[beg:].max() + 3.0
                        return x
                    return make

                def tie(a, b, ts_only=False):
                    def make(rng, c, t):
                        x = rng.normal(0.0, 6.0, V)
                        x[[a, b]] = np.float32((x[beg:].max() + 2.0) if ts_only else (x.max() + 5.0))
                        return x
                    return make

                for idx in (0, cs - 1, cs, seam - 1, seam, eot - 1, beg, V - 1):
                    add(planted(idx), text, f"max at {idx}", expect=dict(id=idx))
                for idx in (beg, V - 1):
                    add(planted_ts(idx), text, f"best timestamp at {idx}", expect=dict(tid=idx, ts_fired=False))
                add(tie(300, 7000), text, "tie across chunks", tie="top", expect=dict(id=300))
                add(tie(70, 261), text, "tie across waves", tie="top", expect=dict(id=70))
                add(tie(seam - 1, seam), text, "tie across the seam", tie="top", expect=dict(id=seam - 1))
                add(tie(seam - 924, seam + 100), text, "tie across the seam, one thread", tie="top", expect=dict(id=seam - 924))
                add(tie(beg + 3, beg + 900, ts_only=True), text, "tie among timestamps", tie="ts",
                    expect=dict(tid=beg + 3, ts_fired=False))
                add(tie(beg + 3, beg + 900), text, "tie among timestamps, rule fired", tie="top+ts",
                    expect=dict(id=beg + 3, tid=beg + 3, ts_fired=True))
            add(lambda rng, c, t: rng.normal(0.0, 6.0, V), text, "row 17")
            assert len(rows) == 17, (kind, len(rows))
            sets[(kind, rot)] = rows
    return sets


_BUILT = {}


def matrix(V: int) -> dict:
    if V not in _BUILT:
        _BUILT[V] = build_vocab(V)
    return _BUILT[V]


def history(c: dict, v: dict) -> list:
    """A token history whose fill_ctl state is c's (is_initial, last_ts, penult_ts)."""
    if c["is_initial"]:
        return []
    last = v["beg"] + 10 if c["last_ts"] else 101
    if c["penult_ts"] and not c["last_ts"] and not c["has_ts"]:
        return [last]  # one token: penult_ts by "fewer than two tokens"
    return [v["beg"] + 5 if c["penult_ts"] else 100, last]
