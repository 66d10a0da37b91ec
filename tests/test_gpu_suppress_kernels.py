"""kernels/logits.hip with a deny mask (suppress_nst / suppress_regex): every kernel form through
whisper_mi355x_debug_logits_deny / whisper_mi355x_debug_logits_topk_deny against tests/suppress_ref.py (float64),
never against another kernel form.

tests/suppress_cases.py (held on the CPU by tests/test_suppress_ref.py): the vocabularies 51865 (micro), 51864 (tiny.en)
and 51866 (large-v3-2L: no multiple of 32), 8 masks (the rows' argmax, best text token and best timestamp denied, all
text, everything, eot, an empty non-null mask, a random 1 %; the bits of the seam ids 0, 31, 32, cs - 1, cs,
36 * 1024 - 1, 36 * 1024, eot - 1, eot, beg, V - 1 set, and rows whose maximum sits on each of them), 17 decided rows per
mask at temperatures 0 / 0.2 / 1.0, in test_gpu_logits_rules.py's three arrangements: form 0 with 16 rows, form 1 with 16
(the split form) and form 1 with 17 (past the switch).

Per row: id and tid exact; the probs rows 0 / -inf exactly on the reference's suppressed set, which includes the mask,
and finite elsewhere; the record's p / plog are the probs rows' entries; the rest within test_gpu_logits_rules.py's
bars for its "unit" rows and the project's PLOG_BAR / P_REL_BAR at temperature 0 (imported: a mask only removes terms
from the sums those bars were measured on). Top-k, k = 5, both forms: candidate 0 is the greedy record bit for bit, no
candidate is denied, the ids are the reference's in its order, id = -1 where fewer than k tokens are left (a mask that
leaves 3). A NULL mask through the new hooks gives the old hooks' bits.

Worst values measured on an MI355X over all cases, vocabularies and arrangements (bar): plog at t = 0 1.80e-6 (6.8e-6),
p at t = 0 1.79e-6 (6.7e-6); plog, p, the logprobs row, the probs row and the sum of probs at t > 0 6.73e-6 (2.8e-5);
pt 7.81e-6 (2.2e-5); ptsum 7.78e-6 (2.4e-5); nosp_prob 1.89e-6 (9.5e-6); top-k plog 1.91e-6 (6.8e-6), p 2.22e-6 (6.7e-6).
"""
import ctypes as C
import json

import numpy as np
import pytest

import beam_ref as br
import logits_cases as lc
import logits_ref as lr
import suppress_cases as sc
import suppress_ref as sr
from conftest import model_path
from test_gpu_beam_kernels import P_REL_BAR, PLOG_BAR, Dev
from test_gpu_logits_rules import ARRANGEMENTS, BARS, SHAPES, rel, seq_ctl

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module", params=list(SHAPES))
def ctx(request, wrs):
    c = wrs.WhisperContext(model_path(request.param), dtype=wrs.F16)
    assert wrs.lib().whisper_n_vocab(c.ptr) == SHAPES[request.param]
    yield c
    c.close()


def launch(wrs, ctx, rows, form, deny_words, hook="deny"):
    L = wrs.lib()
    n = len(rows)
    V = L.whisper_n_vocab(ctx.ptr)
    ctl = (wrs.SeqCtl * n)(*[seq_ctl(wrs, r["ctl"]) for r in rows])
    out = (wrs.Cand * n)()
    probs = np.zeros((n, 2, V), np.float32)
    d = Dev(wrs, ctx)
    try:
        raw = d.up(np.stack([r["raw"] for r in rows]))
        if hook == "deny":
            rc = L.whisper_mi355x_debug_logits_deny(ctx.ptr, raw, n, ctl, form, out, probs.ctypes.data_as(FP),
                                                    None if deny_words is None else deny_words.ctypes.data_as(UP))
        else:
            rc = L.whisper_mi355x_debug_logits(ctx.ptr, raw, n, ctl, form, out, probs.ctypes.data_as(FP))
        assert rc == 0
    finally:
        d.free()
    return out, probs


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("mask", sc.MASKS)
def test_deny(wrs, ctx, mask, arrangement):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    form, n = ARRANGEMENTS[arrangement]
    case = sc.cases(V)[mask]
    rows, deny = case["rows"][:n], case["deny"]
    out, probs = launch(wrs, ctx, rows, form, sr.words(deny))
    bars = BARS["unit"]
    w = dict.fromkeys(("plog_0", "p_0") + tuple(bars), 0.0)
    for r, row in enumerate(rows):
        ref, c, g = row["ref"], row["ctl"], out[r]
        where = f"{V} {mask} {arrangement} row {r} ({row['what']})"
        assert (g.id, g.tid) == (ref["id"], ref["tid"]), where
        assert g.pad == 0.0, where
        if c["want_nosp"]:
            w["nosp"] = max(w["nosp"], rel(g.no_speech_prob, ref["nosp_prob"]))
        else:
            assert g.no_speech_prob == 0.0, where
        if ref["p"] == 0.0:  # no token left: kernels.h's promise
            assert (g.id, g.tid, g.p, g.plog, g.pt, g.ptsum) == (0, 0, 0.0, -np.inf, 0.0, 0.0), where
        else:
            assert not deny[g.id], where
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
        assert sup[deny].all()
        assert ((lp == -np.inf) == sup).all(), f"{where}: {int(((lp == -np.inf) != sup).sum())} ids off the suppressed set"
        assert (p[sup] == 0.0).all(), where
        assert np.isfinite(lp[~sup]).all() and np.isfinite(p).all() and (p >= 0.0).all(), where
        w["lp_row"] = max(w["lp_row"], lr.lp_err(lp, ref["logprobs"]))
        w["p_row"] = max(w["p_row"], float(np.abs(p.astype(np.float64) - ref["probs"]).max()))
        if ref["p"] > 0.0:
            want_sum = float(ref["probs"].sum())
            assert want_sum == pytest.approx(ref["ptsum"] if ref["ts_fired"] else 1.0, abs=1e-12), where
            w["sum_p"] = max(w["sum_p"], abs(float(p.astype(np.float64).sum()) - want_sum))
            assert (p[g.id], lp[g.id]) == (g.p, g.plog), f"{where}: the record is not the probs row's entry"
    print("suppress-kernels worst " + json.dumps(dict(V=V, mask=mask, arrangement=arrangement, **w)))
    assert w["plog_0"] <= PLOG_BAR and w["p_0"] <= P_REL_BAR, w
    over = {k: (w[k], bar) for k, bar in bars.items() if not w[k] <= bar}
    assert not over, f"rows over their bars (measured, bar): {over}"


@pytest.mark.parametrize("split", [0, 1], ids=["one-wg", "split"])
@pytest.mark.parametrize("mask", ["random 1%", "3 tokens left"])
def test_topk_deny(wrs, ctx, mask, split):
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    k = sc.K_TOP
    case = sc.topk_cases(V)[mask]
    rows, deny = case["rows"], case["deny"]
    n = len(rows)
    rules = np.array([[r["ctl"][f] for f in ("is_initial", "last_ts", "penult_ts", "has_ts", "seek_delta", "suppress_blank",
                                            "no_timestamps", "suppress_eot", "tid0_initial", "want_nosp")] for r in rows], np.int32)
    cand = (wrs.Cand * (n * k))()
    greedy = (wrs.Cand * n)()
    d = Dev(wrs, ctx)
    try:
        rc = L.whisper_mi355x_debug_logits_topk_deny(ctx.ptr, d.up(np.stack([r["raw"] for r in rows])), n,
                                                     rules.ctypes.data_as(C.POINTER(C.c_int)), None, k, split, cand, greedy,
                                                     sr.words(deny).ctypes.data_as(UP))
        assert rc == 0
    finally:
        d.free()
    worst_plog = worst_p = 0.0
    short = 0
    for r, row in enumerate(rows):
        got = [cand[r * k + j] for j in range(k)]
        where = f"{V} {mask} split {split} row {r} ({row['what']})"
        assert bytes(got[0]) == bytes(greedy[r]), f"{where}: candidate 0 is not the greedy record"
        # (a row without a token: the all-masked record, id 0 with p 0)
        assert all(g.id == -1 or (j == 0 and g.p == 0.0) or not deny[g.id] for j, g in enumerate(got)), f"{where}: a denied candidate"
        ref = row["ref"]
        if not row["check"]:
            continue
        assert (greedy[r].id, greedy[r].tid) == (ref["id"], ref["tid"]), where
        want = br.candidates(ref["logprobs"], k, v)
        if not want:
            assert [g.id for g in got] == [0] + [-1] * (k - 1) and got[0].p == 0.0, where
            continue
        assert [g.id for g in got] == [c["id"] for c in want] + [-1] * (k - len(want)), where
        short += len(want) < k
        for g, c in zip(got, want):
            assert g.tid == c["tid"], where
            worst_plog = max(worst_plog, abs(g.plog - c["plog"]))
            worst_p = max(worst_p, abs(g.p / c["p"] - 1.0))
    print(f"suppress-topk {V} {mask} split {split}: worst |dplog| {worst_plog:.3e}, worst |dp/p| {worst_p:.3e}, short rows {short}")
    if mask == "3 tokens left":
        assert short >= 8
    assert worst_plog <= PLOG_BAR and worst_p <= P_REL_BAR


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_null_mask_is_the_old_hook(wrs, ctx, arrangement):
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    form, n = ARRANGEMENTS[arrangement]
    rows = sc.cases(V)["empty"]["rows"][:n]
    old = launch(wrs, ctx, rows, form, None, hook="old")
    new = launch(wrs, ctx, rows, form, None)
    zero = launch(wrs, ctx, rows, form, sr.words(np.zeros(V, bool)))
    assert bytes(new[0]) == bytes(old[0]) and new[1].tobytes() == old[1].tobytes()
    assert bytes(zero[0]) == bytes(old[0]) and zero[1].tobytes() == old[1].tobytes()  # (an all-zero mask removes nothing)
    k = sc.K_TOP
    t0 = [dict(r, ctl=dict(r["ctl"], temperature=0.0, want_probs=0)) for r in rows]
    rules = np.array([[r["ctl"][f] for f in ("is_initial", "last_ts", "penult_ts", "has_ts", "seek_delta", "suppress_blank",
                                            "no_timestamps", "suppress_eot", "tid0_initial", "want_nosp")] for r in t0], np.int32)
    res = []
    d = Dev(wrs, ctx)
    try:
        raw = d.up(np.stack([r["raw"] for r in t0]))
        ip = rules.ctypes.data_as(C.POINTER(C.c_int))
        for hook in ("old", "new"):
            cand, greedy = (wrs.Cand * (n * k))(), (wrs.Cand * n)()
            if hook == "old":
                rc = L.whisper_mi355x_debug_logits_topk(ctx.ptr, raw, n, ip, None, k, form, cand, greedy)
            else:
                rc = L.whisper_mi355x_debug_logits_topk_deny(ctx.ptr, raw, n, ip, None, k, form, cand, greedy, None)
            assert rc == 0
            res.append((bytes(cand), bytes(greedy)))
    finally:
        d.free()
    assert res[0] == res[1]
