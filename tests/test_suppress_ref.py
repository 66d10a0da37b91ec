"""tests/suppress_ref.py and tests/suppress_cases.py on the CPU: the reference with an empty mask is logits_ref.process
exactly; a denied id is suppressed whatever the rules say and the no-speech probability does not move; and the cases
the GPU test launches are decided (every kept row has its gaps) and make the points they are named for."""
import math

import numpy as np
import pytest

import logits_cases as lc
import logits_ref as lr
import suppress_cases as sc
import suppress_ref as sr

VOCABS = (51865, 51864, 51866)


def same(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])), k


def test_empty_mask_is_logits_ref():
    V = 51865
    v = lc.vocab(V)
    none = np.zeros(V, bool)
    for row in lc.matrix(V)[("random", 0)] + lc.matrix(V)[("planted", 1)][:4]:
        same(sr.process(row["raw"], row["ctl"], v, none), lr.process(row["raw"], row["ctl"], v))


def test_denied_ids_and_nosp():
    V = 51866
    v = lc.vocab(V)
    row = lc.matrix(V)[("random", 0)][0]  # initial + blank, want_nosp
    plain = lr.process(row["raw"], row["ctl"], v)
    deny = np.zeros(V, bool)
    deny[[plain["id"], 5, V - 1, v["nosp"]]] = True
    got = sr.process(row["raw"], row["ctl"], v, deny)
    assert got["suppressed"][deny].all() and (got["probs"][deny] == 0).all()
    assert (got["suppressed"] == (plain["suppressed"] | deny)).all() or got["ts_fired"] != plain["ts_fired"]
    assert got["id"] != plain["id"]
    assert got["nosp_prob"] == plain["nosp_prob"] > 0
    assert abs(got["probs"].sum() - (got["ptsum"] if got["ts_fired"] else 1.0)) < 1e-12
    every = sr.process(row["raw"], row["ctl"], v, np.ones(V, bool))
    assert (every["id"], every["tid"], every["p"], every["plog"], every["ptsum"]) == (0, 0, 0.0, -math.inf, 0.0)
    assert every["suppressed"].all() and every["nosp_prob"] == plain["nosp_prob"]


def test_words_layout():
    deny = np.zeros(51866, bool)
    deny[[0, 31, 32, 51865]] = True
    w = sr.words(deny)
    assert w.dtype == np.uint32 and len(w) == 1621
    assert (int(w[0]), int(w[1]), int(w[-1])) == (0x80000001, 1, 1 << (51865 & 31)) and int(w[2:-1].sum()) == 0


@pytest.mark.parametrize("V", VOCABS)
def test_cases_are_decided_and_bite(V):
    v = lc.vocab(V)
    beg, eot = v["beg"], v["eot"]
    cs = sc.cases(V)
    assert tuple(cs) == sc.MASKS
    sm = sc.seams(V, v)
    assert sm == [0, 31, 32, (V + 15) // 16 - 1, (V + 15) // 16, 36863, 36864, eot - 1, eot, beg, V - 1]
    for name, case in cs.items():
        deny, rows = case["deny"], case["rows"]
        assert len(rows) == sc.N_ROWS
        assert {r["ctl"]["temperature"] for r in rows} >= {0.0} and any(r["ctl"]["want_probs"] for r in rows)
        for r in rows:
            ref = r["ref"]
            assert sc.decided(ref), (name, r["what"])
            assert min(ref["top2_gap"], ref["ts_gap"]) >= lc.MIN_GAP
            assert ref["tid_lp"] < lc.TID_LP_CLEAR[1] or ref["tid_gap"] >= lc.MIN_GAP
            assert ref["suppressed"][deny].all()
            if ref["p"] > 0:
                assert not deny[ref["id"]] and (ref["tid"] == 0 or not deny[ref["tid"]])
    by = {name: {r["what"]: r for r in case["rows"]} for name, case in cs.items()}
    # the raw argmax is denied: the runner-up wins, in every kept row
    for r in cs["argmax"]["rows"]:
        assert r["ref"]["id"] != r["plain"]["id"]
    # the seam bits: the planted maxima lose under every mask that carries them
    for name in ("argmax", "best text", "best timestamp", "eot", "random 1%"):
        assert cs[name]["deny"][sm].all()
        hit = [r for r in cs[name]["rows"] if r["what"].startswith("max at")]
        assert len(hit) >= 9 and all(r["ref"]["id"] != r["plain"]["id"] for r in hit), name
    # the best text token is denied: the timestamp mass now exceeds the best text token that is left
    mass = by["best text"]["mass below"]
    assert not mass["plain"]["ts_fired"] and mass["ref"]["ts_fired"] and mass["ref"]["id"] >= beg
    # the best timestamp is denied: tid moves
    moved = [r for r in cs["best timestamp"]["rows"] if r["plain"]["tid"] >= beg]
    assert moved and all(r["ref"]["tid"] != r["plain"]["tid"] for r in moved)
    # all text denied: only eot and timestamps are left
    assert all(r["ref"]["id"] >= eot or r["ref"]["p"] == 0 for r in cs["all text"]["rows"])
    assert any(r["ref"]["p"] > 0 for r in cs["all text"]["rows"])
    # everything denied: kernels.h's all-masked record
    assert all((r["ref"]["id"], r["ref"]["p"], r["ref"]["plog"]) == (0, 0.0, -math.inf) for r in cs["everything"]["rows"])
    # eot denied on an initial row that would take it
    ini = by["eot"]["initial, max at eot"]
    assert ini["ctl"]["is_initial"] and ini["plain"]["id"] == eot and ini["ref"]["id"] != eot
    # the empty mask changes nothing; the random one denies about 1 %
    assert not cs["empty"]["deny"].any()
    for r in cs["empty"]["rows"]:
        same(r["ref"], r["plain"])
    assert 0.005 * V < cs["random 1%"]["deny"].sum() < 0.015 * V


@pytest.mark.parametrize("V", VOCABS)
def test_topk_cases(V):
    v = lc.vocab(V)
    tk = sc.topk_cases(V)
    assert sum(r["check"] for r in tk["random 1%"]["rows"]) >= 12
    left = tk["3 tokens left"]
    assert int((~left["deny"]).sum()) == 3
    n_alive = [int((r["ref"]["probs"].astype(np.float32) > 0).sum()) for r in left["rows"]]
    assert max(n_alive) == 3 and min(n_alive) < 3  # rows with 3 tokens, and rows whose rules take more away
    assert sum(r["check"] for r in left["rows"]) >= 8
