"""The numpy restatement of the beam-search contract (tests/beam_ref.py), checked on the CPU:
A.1 with K = 1 and the oracle's logits it reproduces the oracle's greedy window (so the restated logits rules and
    per-token rules are the oracle's);
A.2 on hand-made logits tables the beams are the ones worked out by hand below.
"""
import math

import numpy as np
import pytest

import beam_ref as br
from conftest import model_path
from make_model import synthetic_pcm, synthetic_vocab
from oracle_py import Oracle, reference_params

V = 51865
SPACE = synthetic_vocab().index(b" ")
VID = br.vocab_ids(V, SPACE)
EOT = VID["eot"]
A, B, C_, D, E, F, X, Y = 10, 11, 12, 13, 14, 15, 20, 17


def table_fn(table, default=None):
    """logits_fn over a dict prefix -> {token: logit}; every other entry of the row is -inf."""
    def fn(prefix):
        row = np.full(V, -np.inf, np.float32)
        for tok, val in (table[prefix] if prefix in table else default).items():
            row[tok] = val
        return row
    return fn


def lsm(d):
    """log-softmax of a {token: logit} row (the hand calculation's helper)."""
    m = max(d.values())
    z = m + math.log(sum(math.exp(x - m) for x in d.values()))
    return {k: x - z for k, x in d.items()}


# ---- A.2: the hand-made cases (also the scripts of tests/test_beam_host.py) --------------------------------------
def case_overtaken():
    """K = 2. Greedy takes A first (p 0.60 vs 0.40), but B's continuation is certain and A's is split, so (B, C) overtakes
    both of A's: position 0 takes beam 1's sequence and position 1 beam 0's, a swap of their self-cache rows."""
    t = {(): {A: 1.0, B: 0.6}, (A,): {C_: 0.0, D: -0.1}, (B,): {C_: 5.0, D: -5.0}, (A, C_): {EOT: 0.0}, (B, C_): {EOT: 0.0}}
    P = br.Params(K=2, no_timestamps=True)
    beams = [[B, C_, EOT], [A, C_, EOT]]
    return t, None, P, beams, 0


def case_eot_shrinks():
    """K = 3. Beam 0 ends with EOT at step 1 while beams 1 and 2 go on (n = 2); at step 2 both of beam 1's candidates beat
    beam 2's, so position 2 is re-parented to beam 1 (a fan-out: rows of [B, D] go to beam 2's slot)."""
    t = {(): {A: 2.0, B: 1.0, C_: 0.0}, (A,): {EOT: 3.0, D: 0.0}, (B,): {D: 0.0}, (C_,): {D: 0.0},
         (B, D): {E: 0.0, F: -0.5}, (C_, D): {E: 0.0}, (B, D, E): {EOT: 0.0}, (B, D, F): {EOT: 0.0}}
    P = br.Params(K=3, no_timestamps=True)
    beams = [[A, EOT], [B, D, E, EOT], [B, D, F, EOT]]
    return t, None, P, beams, 0


def case_ties():
    """K = 2. Every key ties: the order is (parent index, rank), so both positions continue beam 0 with its candidates in id
    order, and the equal scores at the end give the lowest index."""
    t = {(): {A: 0.0, B: 0.0}, (A,): {C_: 0.0, D: 0.0}, (B,): {C_: 0.0, D: 0.0}, (A, C_): {EOT: 0.0}, (A, D): {EOT: 0.0}}
    P = br.Params(K=2, no_timestamps=True)
    beams = [[A, C_, EOT], [A, D, EOT]]
    return t, None, P, beams, 0


def case_all_fail():
    """K = 2, timestamps on, a 3-step window: no beam has produced a timestamp by the last step, so every beam fails."""
    t = {(): {A: 1.0, B: 0.0}}
    P = br.Params(K=2, n_max=3)
    beams = [[A, X, X], [B, X, X]]
    return t, {X: 0.0}, P, beams, -1


def case_length_penalty(lp):
    """K = 2. [A, EOT] sums to -1.001 over 2 tokens, [B, D, E, EOT] to -1.416 over 4: the average (default) prefers the long
    beam (-0.354 vs -0.501), length_penalty = 1 divides by (5 + len) / 6 and prefers the short one (-0.858 vs -0.944)."""
    t = {(): {A: 0.7, B: 0.0}, (A,): {EOT: 0.0, Y: -0.2}, (B,): {D: 0.0}, (B, D): {E: 0.0, F: -1.0}, (B, D, E): {EOT: 0.0}}
    P = br.Params(K=2, no_timestamps=True, length_penalty=lp)
    beams = [[A, EOT], [B, D, E, EOT]]
    return t, None, P, beams, 0 if lp > 0 else 1


CASES = {
    "overtaken": case_overtaken,
    "eot_shrinks": case_eot_shrinks,
    "ties": case_ties,
    "all_fail": case_all_fail,
    "length_penalty_off": lambda: case_length_penalty(-1.0),
    "length_penalty_on": lambda: case_length_penalty(1.0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_hand_tables(name):
    table, default, P, beams, winner = CASES[name]()
    r = br.beam_search(table_fn(table, default), P, VID, n_prompt=3)
    assert [b["tokens"] for b in r.beams] == beams
    assert r.winner == winner
    assert [b["winner"] for b in r.beams] == [i == winner for i in range(P.K)]
    if name == "all_fail":
        assert all(b["failed"] for b in r.beams) and r.failed0 and r.tokens == []
    else:
        assert all(b["completed"] and not b["failed"] for b in r.beams)
        assert r.tokens == beams[winner]


def test_hand_tables_details():
    """The sums, the greedy choice, and the copy lists of the cases above, by the hand calculation."""
    table, _, P, _, _ = case_overtaken()
    r = br.beam_search(table_fn(table), P, VID, n_prompt=3)
    s_b = lsm(table[()])[B] + lsm(table[(B,)])[C_]
    s_a = lsm(table[()])[A] + lsm(table[(A,)])[C_]
    assert r.beams[0]["sum_logprobs_all"] == pytest.approx(s_b, abs=1e-6)
    assert r.beams[1]["sum_logprobs_all"] == pytest.approx(s_a, abs=1e-6)
    assert r.picks[1] == [(0, 1, 0), (1, 0, 0)]
    assert r.copies[0] == [(1, 0, 0, 3)]                      # the prompt's rows to beam 1
    assert sorted(r.copies[1]) == [(0, 1, 3, 4), (1, 0, 3, 4)]  # the swap: row0 = the common prefix (the prompt)
    g = br.beam_search(table_fn(table), br.Params(K=1, no_timestamps=True), VID)
    assert g.tokens == [A, C_, EOT]  # greedy keeps its first choice
    table, _, P, _, _ = case_eot_shrinks()
    r = br.beam_search(table_fn(table), P, VID, n_prompt=3)
    assert r.picks[1] == [(0, 0, 0), (1, 1, 0), (2, 2, 0)] and r.copies[1] == []
    assert r.picks[2] == [(1, 1, 0), (2, 1, 1)]              # two live positions only
    assert r.copies[2] == [(2, 1, 3, 5)]                     # [C, D] vs [B, D]: nothing in common after the prompt
    table, _, P, _, _ = case_ties()
    r = br.beam_search(table_fn(table), P, VID, n_prompt=3)
    assert r.picks[1] == [(0, 0, 0), (1, 0, 1)] and r.copies[1] == [(1, 0, 3, 4)]


def test_common_prefix_rule():
    """A re-parented position that already shares its parent's first tokens receives only the rows after them."""
    t = {(): {A: 0.0, B: -3.0}, (A,): {C_: 0.0, D: -0.1}, (B,): {C_: 0.0}, (A, C_): {E: 0.0, F: -0.05},
         (A, D): {E: 0.0, F: 0.0, X: 0.0, Y: 0.0},         (A, C_, E): {EOT: 0.0}, (A, C_, F): {EOT: 0.0}}
    r = br.beam_search(table_fn(t), br.Params(K=2, no_timestamps=True), VID, n_prompt=3)
    assert r.picks[1] == [(0, 0, 0), (1, 0, 1)]   # [A, C], [A, D]
    assert r.picks[2] == [(0, 0, 0), (1, 0, 1)]   # [A, C, E], [A, C, F]
    assert r.copies[2] == [(1, 0, 4, 5)]          # beam 1 held [A, D]: the prompt and A stay, the row of C moves


# ---- A.1: K = 1 over the oracle's logits = the oracle's greedy window -------------------------------------------
@pytest.mark.parametrize("clip", [0, 1])
def test_k1_is_oracle_greedy(clip):
    path = model_path("micro+conf")
    pcm = synthetic_pcm(clip)
    o = Oracle(path, mode=1, n_threads=8)
    rp = reference_params("en")
    rp.temperature_inc = 0.0
    res = o.full(pcm, rp)
    want = [t for t, s in zip(res["step_tokens"], res["step_seeks"]) if s == 0]
    d0 = res["decisions"][0]
    o.new_state()
    _, n_org = o.mel(pcm)
    o.encode(0)
    sot = o.token("sot")
    prompt = [sot, sot + 1, o.token("transcribe")]
    state = {"prefix": None}

    def logits_fn(prefix):
        if state["prefix"] is not None and prefix[:-1] == state["prefix"] and len(prefix) > 0:
            row = o.decode([prefix[-1]], len(prompt) + len(prefix) - 1)[-1]
        else:
            o.kv_clear()
            row = o.decode(prompt + list(prefix), 0)[-1]
        state["prefix"] = prefix
        return row

    vid = br.vocab_ids(o.n_vocab, SPACE)
    assert (vid["eot"], vid["beg"], vid["not_"]) == (o.token("eot"), o.token("beg"), o.token("not"))
    P = br.Params(K=1, n_max=o.n_text_ctx // 2 - 4, seek_end=n_org, n_audio_ctx=o.n_audio_ctx)
    r = br.beam_search(logits_fn, P, vid, n_prompt=len(prompt))
    o.close()
    assert r.beams[0]["tokens"] == want
    assert (int(r.failed0), r.result_len) == (d0["failed0"], d0["result_len0"])
    if r.result_len:
        assert r.avg_logprobs == pytest.approx(d0["avg_logprob0"], abs=1e-4)
        assert r.entropy == pytest.approx(d0["entropy0"], abs=1e-5)
