"""kernels/logits.hip rule by rule: the greedy logits kernels in both forms and decode_advance_kernel, through
whisper_mi355x_debug_logits / whisper_mi355x_debug_decode_advance, against tests/logits_ref.py (float64; held to the
oracle by tests/test_logits_ref.py), never against another kernel form.

The matrix (tests/logits_cases.py), for the vocabularies 51865 (micro), 51864 (tiny.en) and 51866 (large-v3-2L): 9 sets
of 16 rows + 1, each set in three arrangements: form 0 (one workgroup per row), form 1 with 16 rows (the split form)
and form 1 with 17 rows (past the launcher's switch: one workgroup per row). A set mixes the rule states and the
temperatures 0, 0.2 and 1.0 (t > 0 rows with want_probs) in one launch; over a kind's three sets every row meets every
temperature (the N(0, 30^2) rows: 0.2 and 1.0). Rows: N(0, 6^2) and N(0, 30^2) per rule state (initial step with and
without suppress_blank / max_initial_ts, text-text, text-timestamp, timestamp-timestamp, has_ts with seek_delta
20 / 21 / 2998, no_timestamps, suppress_eot, everything masked), raw -inf entries, timestamp mass 4e-3 nats above / below the best text token,
the maximum planted at 0, cs - 1, cs, 36 * 1024 - 1, 36 * 1024, eot - 1, beg, V - 1 (cs = ceil(V / 16), the split
form's chunk), the best timestamp at beg and V - 1, and exact ties across chunks, waves, the LDS / register seam and
among timestamps.

Per row: id and tid exact; the probs rows are -inf / 0 exactly on the reference's suppressed set and finite elsewhere,
and untouched (NaN from the hook's fill) without want_probs; the record's p / plog are the probs rows' entries;
nosp_prob is 0 without want_nosp; the all-masked row is id 0, p 0, plog -inf, ptsum 0. The rest within bars. At
temperature 0, p and plog are under the project's PLOG_BAR / P_REL_BAR (test_gpu_beam_kernels.py; measured here 1.83e-6
and 1.81e-6). The others are 4 x the worst value measured on an MI355X over the matrix, all vocabularies and
arrangements (both forms gave the same worst value to three digits, but for ptsum). Relative errors are
|got - ref| / (ref + 1e-30), so a probability that one side flushes to 0 counts as its absolute size; the logprobs row
is measured by logits_ref.lp_err (absolute up to |logprob| = 1, relative beyond); the probs row sums to 1, or to ptsum
when the timestamp rule struck the text tokens after the softmax, and is compared with the reference's sum.
The bars come in two classes, because a float logprob x - lse cannot be better than half a float step of lse: the
N(0, 30^2) rows (class "wide"; t = 0.2 and 1.0 only, lse ~650 at 0.2: half a step is 3.05e-5) and every other row
(class "unit", lse < 256: 7.6e-6).
                            unit: measured -> bar        wide: measured -> bar
    plog at t > 0  |d|      6.86e-6 -> 2.8e-5            2.87e-5 -> 1.15e-4
    p at t > 0     rel      6.86e-6 -> 2.8e-5            2.86e-5 -> 1.15e-4
    pt             rel      5.34e-6 -> 2.2e-5            7.36e-6 -> 3.0e-5
    ptsum          rel      5.78e-6 -> 2.4e-5            7.34e-6 -> 3.0e-5
    nosp_prob      rel      2.37e-6 -> 9.5e-6            6.16e-9 -> 2.5e-8   (wide: probabilities below 1e-20)
    logprobs row   lp_err   6.86e-6 -> 2.8e-5            2.87e-5 -> 1.15e-4
    probs row      |d|      6.86e-6 -> 2.8e-5            2.48e-5 -> 1.0e-4
    sum of probs   |d|      6.86e-6 -> 2.8e-5            2.87e-5 -> 1.15e-4
Ten times each logprob bar is at most the least gap of any decision of the class's inputs (test_logits_ref.py):
MIN_GAP = 1e-3 for the unit rows, WIDE_MIN_GAP = 1e-2 for the wide rows.

decode_advance_kernel: exact against logits_ref.advance (restated from process_step and fill_ctl), n in {1, 5, 128, 130},
ct = n + 3, applied twice.
"""
import ctypes as C
import json

import numpy as np
import pytest

import logits_cases as lc
import logits_ref as lr
from conftest import model_path
from test_gpu_beam_kernels import P_REL_BAR, PLOG_BAR, Dev

pytestmark = pytest.mark.gpu

# scale class of a row (logits_cases) -> metric -> bar
BARS = {
    "unit": dict(plog_t=2.8e-5, p_t=2.8e-5, pt=2.2e-5, ptsum=2.4e-5, nosp=9.5e-6, lp_row=2.8e-5, p_row=2.8e-5, sum_p=2.8e-5),
    "wide": dict(plog_t=1.15e-4, p_t=1.15e-4, pt=3.0e-5, ptsum=3.0e-5, nosp=2.5e-8, lp_row=1.15e-4, p_row=1.0e-4, sum_p=1.15e-4),
}
MIN_GAPS = {"unit": lc.MIN_GAP, "wide": lc.WIDE_MIN_GAP}

SHAPES = {"micro": 51865, "tiny.en": 51864, "large-v3-2L": 51866}
ARRANGEMENTS = {"one-wg": (0, 16), "split-16": (1, 16), "switch-17": (1, 17)}


@pytest.fixture(scope="module", params=list(SHAPES))
def ctx(request, wrs):
    c = wrs.WhisperContext(model_path(request.param), dtype=wrs.F16)
    assert wrs.lib().whisper_n_vocab(c.ptr) == SHAPES[request.param]
    yield c
    c.close()


def seq_ctl(wrs, c: dict):
    return wrs.SeqCtl(*[c[f] for f in lr.CTL_FIELDS])


def ctl_dict(s) -> dict:
    return {f: getattr(s, f) for f in lr.CTL_FIELDS}


def rel(got, ref) -> float:
    return abs(float(got) - ref) / (ref + 1e-30)


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("kind", lc.KINDS)
def test_rules(wrs, ctx, kind, rot, arrangement):
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    form, n = ARRANGEMENTS[arrangement]
    rows = lc.matrix(V)[(kind, rot)][:n]
    raw = np.stack([r["raw"] for r in rows])
    ctl = (wrs.SeqCtl * n)(*[seq_ctl(wrs, r["ctl"]) for r in rows])
    out = (wrs.Cand * n)()
    probs = np.zeros((n, 2, V), np.float32)
    d = Dev(wrs, ctx)
    try:
        rc = L.whisper_mi355x_debug_logits(ctx.ptr, d.up(raw), n, ctl, form, out, probs.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == 0
    finally:
        d.free()
    worst = {cls: dict.fromkeys(("plog_0", "p_0") + tuple(BARS[cls]), 0.0) for cls in BARS}
    for r, row in enumerate(rows):
        ref, c, g, w = row["ref"], row["ctl"], out[r], worst[row["scale"]]
        where = f"{V} {kind} {rot} {arrangement} row {r} ({row['what']})"
        assert (g.id, g.tid) == (ref["id"], ref["tid"]), where
        assert g.pad == 0.0, where
        if c["want_nosp"]:
            w["nosp"] = max(w["nosp"], rel(g.no_speech_prob, ref["nosp_prob"]))
        else:
            assert g.no_speech_prob == 0.0, where
        if ref["p"] == 0.0:  # no token left: kernels.h's promise
            assert (g.id, g.tid, g.p, g.plog, g.pt, g.ptsum) == (0, 0, 0.0, -np.inf, 0.0, 0.0), where
        else:
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
        assert (p[sup] == 0.0).all(), where
        assert np.isfinite(lp[~sup]).all() and np.isfinite(p).all() and (p >= 0.0).all(), where
        w["lp_row"] = max(w["lp_row"], lr.lp_err(lp, ref["logprobs"]))
        w["p_row"] = max(w["p_row"], float(np.abs(p.astype(np.float64) - ref["probs"]).max()))
        if ref["p"] > 0.0:
            # the row sums to 1, or to ptsum when the timestamp rule struck the text tokens after the softmax
            want_sum = float(ref["probs"].sum())
            assert want_sum == pytest.approx(ref["ptsum"] if ref["ts_fired"] else 1.0, abs=1e-12), where
            w["sum_p"] = max(w["sum_p"], abs(float(p.astype(np.float64).sum()) - want_sum))
            assert (p[g.id], lp[g.id]) == (g.p, g.plog), f"{where}: the record is not the probs row's entry"
    print("logits-rules worst " + json.dumps(dict(V=V, kind=kind, rot=rot, arrangement=arrangement, **worst)))
    assert 10 * PLOG_BAR <= lc.MIN_GAP
    for cls, bars in BARS.items():
        assert 10 * bars["plog_t"] <= MIN_GAPS[cls] and 10 * bars["lp_row"] <= MIN_GAPS[cls]
        w = worst[cls]
        assert w["plog_0"] <= PLOG_BAR and w["p_0"] <= P_REL_BAR, (cls, w)
        over = {k: (w[k], bar) for k, bar in bars.items() if not w[k] <= bar}
        assert not over, f"{cls} rows over their bars (measured, bar): {over}"


# ---- decode_advance -----------------------------------------------------------------------------------------------
def _advance_inputs(wrs, n: int, ct: int, beg: int, eot: int):
    rng = np.random.default_rng(1000 + n)
    states = [c for _, c in lc.states()]
    ctl = []
    for r in range(ct):
        c = dict(states[r % len(states)])
        c.update(temperature=float(np.float32((0.0, 0.2, 1.0)[r % 3])), want_probs=int(r % 3 > 0), want_nosp=int(r % 2 == 0),
                 suppress_blank=int(r % 4 != 1), suppress_eot=int(r % 5 == 2), tid0_initial=(50, -1, 7)[r % 3])
        ctl.append(c)
    ints = rng.integers(0, 400, 5 * ct).astype(np.int32)
    toks = [(1234, beg, beg + 7, eot, 17, beg + 1499, beg + 1)[(r + s) % 7] for s in range(2) for r in range(n)]
    return ctl, ints, np.asarray(toks, np.int32).reshape(2, n), rng


@pytest.mark.parametrize("n", [1, 5, 128, 130])
def test_decode_advance(wrs, ctx, n):
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    beg, ct = v["beg"], n + 3
    assert beg == L.whisper_token_beg(ctx.ptr)
    ctl, ints, toks, rng = _advance_inputs(wrs, n, ct, beg, v["eot"])
    d_ctl = (wrs.SeqCtl * ct)(*[seq_ctl(wrs, c) for c in ctl])
    ring = np.frombuffer(rng.bytes(32 * ct), np.uint8).copy()
    for step, err in enumerate((None, 0x1234abcd)):
        tout = (wrs.Cand * n)()
        np.frombuffer(tout, np.uint8)[:] = np.frombuffer(rng.bytes(32 * n), np.uint8)  # every bit of a record is copied
        for r in range(n):
            tout[r].id = int(toks[step, r])
        want_ints = ints.copy()
        want_ctl = list(ctl)
        for r in range(n):
            want_ctl[r] = lr.advance(ctl[r], want_ints, ct, r, int(toks[step, r]), beg)
            for f in lr.CTL_FIELDS:
                if f not in lr.CTL_ADVANCED:
                    assert want_ctl[r][f] == ctl[r][f]
        want_ring = ring.copy()
        want_ring[:32 * n] = np.frombuffer(tout, np.uint8)
        ring_err = C.c_uint(0xdeadbeef)
        word = C.c_uint(err) if err is not None else None
        rc = L.whisper_mi355x_debug_decode_advance(ctx.ptr, n, ct, beg, tout, ints.ctypes.data_as(C.POINTER(C.c_int)), d_ctl,
                                                   C.byref(word) if word is not None else None,
                                                   ring.ctypes.data_as(C.POINTER(wrs.Cand)), C.byref(ring_err))
        assert rc == 0
        assert ring_err.value == (err or 0)
        bad = np.nonzero(ints != want_ints)[0]
        assert bad.size == 0, f"step {step}: ints differ at {bad[:8]} (region, row: {[(int(i) // ct, int(i) % ct) for i in bad[:8]]})"
        for r in range(ct):
            got = ctl_dict(d_ctl[r])
            assert got == want_ctl[r], f"step {step} row {r}{' (not a row of the step)' if r >= n else ''}: {got} != {want_ctl[r]}"
            if r < n:
                assert got["want_nosp"] == 0
        assert (ring == want_ring).all(), f"step {step}: ring differs at record {int(np.nonzero(ring != want_ring)[0][0]) // 32}"
        ctl = want_ctl
    # the transition the issue names: beg itself is a timestamp that moves no window; beg + 7 gives seek_delta 14
    for r in range(n):
        first, second = int(toks[0, r]), int(toks[1, r])
        assert ctl[r]["penult_ts"] == int(first >= beg) and ctl[r]["last_ts"] == int(second >= beg)
        if second == beg + 7:
            assert (ctl[r]["has_ts"], ctl[r]["seek_delta"]) == (1, 14)
