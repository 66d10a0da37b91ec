"""tests/logits_filter_ref.py (the two halves of the logits rules around logits_filter_callback) against
tests/logits_ref.py, and the rows of tests/logits_filter_cases.py: no device.

- post(pre(raw)) is logits_ref.process(raw) exactly (every entry of the record, the logprobs and probs rows and the
  suppressed set), over logits_cases.matrix(V) for V in 51864 / 51865 / 51866, which runs every row at every
  temperature of logits_cases.TEMPS;
- pre() touches nothing but the divide and the ids of its rules, and with tdrz differs from itself in the solm entry only;
- every edited row of logits_filter_cases is decided by logits_cases.MIN_GAP in the reference, or is the planted tie, and
  answers what its edit is built to show.
"""
import math

import numpy as np
import pytest

import logits_cases as lc
import logits_filter_cases as fc
import logits_filter_ref as fr
import logits_ref as lr

VOCABS = (51864, 51865, 51866)


def same(a: dict, b: dict, where: str):
    assert a.keys() == b.keys(), where
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), f"{where}: {k}"
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), f"{where}: {k} {a[k]} != {b[k]}"


@pytest.mark.parametrize("V", VOCABS)
def test_post_of_pre_is_process(V):
    v = lc.vocab(V)
    seen = set()
    for (kind, rot), rows in lc.matrix(V).items():
        for r, row in enumerate(rows):
            c = row["ctl"]
            seen.add(c["temperature"])
            f = fr.pre(row["raw"], c, v)
            assert f.dtype == np.float32 and f.shape == (V,)
            same(fr.post(f, row["raw"], c, v), lr.process(row["raw"], c, v), f"{V} {kind} {rot} row {r} ({row['what']})")
    assert seen == set(lc.TEMPS)


def pre_ids(c: dict, v: dict, tdrz: bool) -> np.ndarray:
    """the ids the pre-callback rules suppress, written out from the contract (include/whisper.h)"""
    ids = [v[k] for k in ("not_", "sot", "nosp", "translate", "transcribe", "prev")] + list(range(v["sot"] + 1, v["sot"] + 1 + v["n_lang"]))
    if not tdrz:
        ids.append(v["solm"])
    if c["suppress_blank"] and c["is_initial"]:
        ids += [v["eot"], v["space"]]
    if c["no_timestamps"]:
        ids += list(range(v["beg"], v["n_vocab"]))
    return np.unique(ids)


@pytest.mark.parametrize("V", VOCABS)
def test_pre(V):
    v = lc.vocab(V)
    rng = np.random.default_rng(V)
    raw = rng.normal(0.0, 6.0, V).astype(np.float32)
    for name, c0 in lc.states():
        for t in lc.TEMPS:
            c = lc._with_temp(c0, t)
            plain, tdrz = fr.pre(raw, c, v, False), fr.pre(raw, c, v, True)
            for f, flag in ((plain, False), (tdrz, True)):
                ids = pre_ids(c, v, flag)
                assert (f[ids] == -np.inf).all(), (name, t, flag)
                keep = np.ones(V, bool)
                keep[ids] = False
                want = raw / np.float32(t) if t > 0 else raw
                assert want.dtype == np.float32
                assert np.array_equal(f[keep].view(np.uint32), want[keep].view(np.uint32)), (name, t, flag)
            diff = np.nonzero(plain.view(np.uint32) != tdrz.view(np.uint32))[0]
            assert list(diff) == [v["solm"]], (name, t, diff)
            assert plain[v["solm"]] == -np.inf and tdrz[v["solm"]] == (raw / np.float32(t) if t > 0 else raw)[v["solm"]]


@pytest.mark.parametrize("V", VOCABS)
def test_edited_rows_are_decided(V):
    v = lc.vocab(V)
    sets = fc.matrix(V)
    assert set(sets) == {False, True}
    for tdrz, rows in sets.items():
        assert len(rows) == 17
        assert {r["what"] for r in rows} == set(fc.EDITS)
        assert {r["ctl"]["temperature"] for r in rows} == set(lc.TEMPS)
        for r, row in enumerate(rows):
            where = f"{V} tdrz {tdrz} row {r} ({row['what']})"
            ref, ref0, c = row["ref"], row["ref0"], row["ctl"]
            assert lc._decided(ref, row["tie"]), where  # MIN_GAP, or the exact planted tie
            same(ref, fr.post(row["filtered"], row["raw"], c, v), where)
            assert ref["nosp_prob"] == lr.process(row["raw"], c, v)["nosp_prob"], where  # the raw row's, whatever the edit
            order = np.argsort(-ref0["logprobs"], kind="stable")
            if row["what"] == "ban 1":
                assert ref["id"] != order[0] and ref["suppressed"][order[0]], where
                assert ref["id"] == order[1] or ref["ts_fired"] != ref0["ts_fired"], where
            elif row["what"] == "ban 8":  # (the next best token, unless the ban moved the timestamp rule)
                assert ref["id"] not in order[:8] and ref["suppressed"][order[:8]].all(), where
                assert ref["id"] == order[8] or ref["ts_fired"] != ref0["ts_fired"], where
            elif row["what"] == "boost":
                assert ref["id"] == order[1] and ref0["id"] == order[0], where
            elif row["what"] == "solm":
                if tdrz:
                    assert ref["id"] == v["solm"] and ref["p"] == 1.0 and not ref["ts_fired"], where
                else:
                    same(ref, ref0, where)
                    assert ref["suppressed"][v["solm"]], where
            elif row["what"] == "all -inf":
                assert (ref["id"], ref["tid"], ref["p"], ref["plog"], ref["ptsum"]) == (0, 0, 0.0, -math.inf, 0.0), where
                assert ref["suppressed"].all(), where
            elif row["what"] == "tie":
                assert row["tie"] == "top" and ref["id"] == min(fc.TIE_IDS), where
                assert ref["logprobs"][fc.TIE_IDS[0]] == ref["logprobs"][fc.TIE_IDS[1]], where
