"""tests/logits_ref.py, the float64 restatement the logits kernels are tested against, held to the oracle's
process_logits + sample_token(best) (oracle_process_logits) on every row of the kernel tests' matrix
(tests/logits_cases.py: three vocabularies, 9 sets of 17 rows each), and to tests/beam_ref.py's rules.

Against the oracle: the same suppressed set, id and tid exactly; logprobs against the oracle's float values by
logits_ref.lp_err (absolute for |logprob| <= 1, relative beyond), and the greedy record's plog (absolute), p, pt and
ptsum (relative) under the same bar.
    worst over the matrix, measured: logprobs 3.89e-05, the record 3.89e-05 -> LP_BAR 1.6e-04 (4 x 3.89e-05)
This is the oracle's error, not the reference's: it sums up to 51866 float terms one after the other into a float
log-sum-exp, which shifts a whole row by one amount (so no decision of the oracle's moves with it).
Against beam_ref.rules: bit-equal logprobs on test_topk's four rows.
The inputs: every row's top-2 gap, timestamp-rule gap and gap between its two best timestamps are at least MIN_GAP,
(WIDE_MIN_GAP for the N(0, 30^2) rows) except the gap a tie row zeroes on purpose, and every row shows what it was
built to show.
"""
import ctypes as C
import math

import numpy as np
import pytest

import logits_cases as lc
import logits_ref as lr
from conftest import model_path
from oracle_py import reference_params, shared_oracle

LP_BAR = 1.6e-4
SHAPES = {51865: "micro", 51864: "tiny.en", 51866: "large-v3-2L"}


def oracle_row(o, v, row):
    c = row["ctl"]
    p = reference_params("en")
    p.suppress_blank = c["suppress_blank"]
    p.no_timestamps = c["no_timestamps"]
    p.fixed_tokens = 1 if c["suppress_eot"] else 0
    precision = np.float32(30) / np.float32(o.n_audio_ctx)
    p.max_initial_ts = float(np.float32(c["tid0_initial"]) * precision) if c["tid0_initial"] >= 0 else 0.0
    return o.process_logits(row["raw"], lc.history(c, v), c["has_ts"], c["seek_delta"], p, c["temperature"])


@pytest.mark.parametrize("V", list(SHAPES))
def test_reference_matches_oracle(V):
    o = shared_oracle(model_path(SHAPES[V]))
    assert o.n_vocab == V
    v = lc.vocab(V)
    for k in ("eot", "sot", "translate", "transcribe", "solm", "prev", "nosp", "not", "beg"):
        assert o.token(k) == v["not_" if k == "not" else k], k
    worst = worst_td = 0.0
    for key, rows in lc.matrix(V).items():
        for r, row in enumerate(rows):
            ref = row["ref"]
            lp, pr, td = oracle_row(o, v, row)
            where = f"{V} {key} row {r} ({row['what']})"
            assert ((lp == -np.inf) == ref["suppressed"]).all(), where
            assert ((pr == 0)[ref["suppressed"]]).all(), where
            assert td["id"] == ref["id"] and td["tid"] == ref["tid"], where
            worst = max(worst, lr.lp_err(lp, ref["logprobs"]))
            if ref["p"] > 0:
                worst_td = max(worst_td, abs(td["plog"] - ref["plog"]), abs(td["p"] / ref["p"] - 1.0),
                               abs(td["pt"] - ref["pt"]) / (ref["pt"] + 1e-30), abs(td["ptsum"] - ref["ptsum"]) / (ref["ptsum"] + 1e-30))
    print(f"vocabulary {V}: worst logprob error against the oracle {worst:.3e} (bar {LP_BAR:.1e}), "
          f"worst error of the greedy record's plog / p / pt / ptsum {worst_td:.3e}")
    assert worst <= LP_BAR and worst_td <= LP_BAR


def test_reference_matches_beam_ref():
    from test_gpu_beam_kernels import topk_rows
    V = 51865
    vid, raw, rules, lps = topk_rows(V)
    assert vid == lc.vocab(V)
    for r in range(4):
        q = [int(x) for x in rules[r]]
        c = lr.ctl(is_initial=q[0], last_ts=q[1], penult_ts=q[2], has_ts=q[3], seek_delta=q[4], suppress_blank=q[5],
                   no_timestamps=q[6], suppress_eot=q[7], tid0_initial=q[8], want_nosp=q[9])
        ref = lr.process(raw[r], c, vid)
        lp, gap = lps[r]
        assert ref["logprobs"].tobytes() == np.asarray(lp, np.float64).tobytes(), r
        assert ref["ts_gap"] == gap, r


@pytest.mark.parametrize("V", list(SHAPES))
def test_inputs_decide(V):
    n_tie = 0
    for key, rows in lc.matrix(V).items():
        assert len(rows) == 17
        for r, row in enumerate(rows):
            ref = row["ref"]
            where = f"{V} {key} row {r} ({row['what']})"
            min_gap = lc.WIDE_MIN_GAP if row["scale"] == "wide" else lc.MIN_GAP
            assert (row["scale"] == "wide") == (key[0] == "wide" and r < 11), where
            assert ref["ts_gap"] >= min_gap, where
            tie = row["tie"] or ""
            if "top" in tie:
                assert ref["top2_gap"] == 0.0, where
                n_tie += 1
            else:
                assert ref["top2_gap"] >= min_gap, where
            assert not (lc.TID_LP_CLEAR[1] <= ref["tid_lp"] <= lc.TID_LP_CLEAR[0]), where
            if "ts" in tie:
                assert ref["tid_gap"] == 0.0, where
            elif ref["tid_lp"] >= lc.TID_LP_CLEAR[1]:  # (below it every timestamp's float p is 0: tid = 0)
                assert ref["tid_gap"] >= min_gap, where
            for k, e in row["expect"].items():
                assert ref[k] == e, (where, k)
            assert row["ctl"]["want_probs"] == (row["ctl"]["temperature"] > 0)
    assert n_tie == 15  # 5 exact ties of the row's two largest logits in each of the 3 planted sets
    # every rule state at every temperature, and both sides of the timestamp-mass rule at every temperature
    seen = {(row["what"], row["ctl"]["temperature"]) for rows in lc.matrix(V).values() for row in rows}
    for name, _ in lc.states():
        for t in lc.TEMPS:
            assert (f"random/{name}", t) in seen and (t == 0 or (f"wide/{name}", t) in seen)
    for t in lc.TEMPS:
        assert ("wide/mass above", t) in seen and ("wide/mass below", t) in seen


def test_advance_restates_fill_ctl():
    """logits_ref.advance against a token list walked the way fill_ctl reads it."""
    beg = 50364
    toks = []
    c = lr.ctl(is_initial=1, penult_ts=1, want_nosp=1, temperature=0.4, want_probs=1)
    ints = np.arange(5 * 4, dtype=np.int32)
    has_ts, seek_delta = 0, 3000
    for tok in (beg, 17, beg + 7, beg + 7, 99, 100, beg + 3):
        pos = int(ints[4 + 1])
        c = lr.advance(c, ints, 4, 1, tok, beg)
        toks.append(tok)
        if tok > beg:
            has_ts, seek_delta = 1, 2 * (tok - beg)
        assert c["is_initial"] == 0 and c["want_nosp"] == 0
        assert c["last_ts"] == int(toks[-1] >= beg)
        assert c["penult_ts"] == int(len(toks) < 2 or toks[-2] >= beg)
        assert (c["has_ts"], c["seek_delta"]) == (has_ts, seek_delta)
        assert (c["temperature"], c["want_probs"], c["suppress_blank"], c["tid0_initial"]) == (0.4, 1, 1, 50)
        assert ints[1] == tok and ints[4 + 1] == pos + 1 and ints[12 + 1] == pos + 2
    untouched = np.arange(20, dtype=np.int32)
    keep = np.ones(20, bool)
    keep[[1, 5, 13]] = False
    assert (ints[keep] == untouched[keep]).all()


def test_hooks_refuse_bad_arguments(wrs):
    """Both hooks return -1 before touching a device."""
    L = wrs.lib()
    assert C.sizeof(wrs.SeqCtl) == 48
    assert L.whisper_mi355x_debug_logits(None, None, 0, None, 0, None, None) == -1
    ctl = (wrs.SeqCtl * 1)()
    out = (wrs.Cand * 1)()
    assert L.whisper_mi355x_debug_logits(None, None, 1, ctl, 0, out, None) == -1
    assert L.whisper_mi355x_debug_decode_advance(None, 0, 0, 0, None, None, None, None, None, None) == -1
    ints = (C.c_int * 5)()
    err = C.c_uint(0)
    assert L.whisper_mi355x_debug_decode_advance(None, 1, 1, 50364, out, ints, ctl, None, out, C.byref(err)) == -1
    assert not math.isnan(out[0].p) and list(ints) == [0] * 5
