"""The device halves of a logits launch around whisper_full_params.logits_filter_callback (kernels/logits.hip,
DESIGN.md §20) through whisper_mi355x_debug_logits_stage / _logits_ex / _logits_topk_ex, for the vocabularies 51865
(micro), 51864 (tiny.en) and 51866 (large-v3-2L), with 1, 16 and 17 rows per launch: the split form, the one-workgroup
form and the launcher's switch between them.

- stage: every row equals logits_filter_ref.pre bit for bit, at t = 0 and at t > 0 (numpy's float32 quotient: both are
  correctly rounded divisions, the file is built without fast-math), with and without the tdrz flag, whose only effect is
  the solm entry. The rows are written into a buffer of canaries: nothing behind the last row changes; and row by row
  into a buffer of canaries at element offsets 0, V, 2 V, 3 V (every alignment an odd row stride produces) and from an
  input that is aligned differently from the output (the all-scalar path): nothing before or behind a row changes.
- prefiltered(pre(raw)) is the plain form's record and probs rows bit for bit, over logits_cases' whole matrix: the engine
  against itself, same instantiation family, same accumulation order.
- prefiltered(edited rows) against logits_filter_ref.post over logits_filter_cases' rows: id, tid and the suppressed set
  exact, p / plog under the bars DESIGN.md §11 records for these kernels against logits_ref (PLOG_BAR / P_REL_BAR at
  t = 0, 2.8e-5 at t > 0), nosp_prob the raw row's.
- top-k, k in {1, 5, 8}, over the edited rows: candidate 0 is the greedy record bit for bit, and candidate j is the
  reference's j-th most probable token (its logprob within the bar of the reference's j-th largest).
"""
import ctypes as C

import numpy as np
import pytest

import logits_cases as lc
import logits_filter_cases as fc
import logits_filter_ref as fr
from conftest import model_path
from test_gpu_beam_kernels import P_REL_BAR, PLOG_BAR, Dev
from test_gpu_logits_rules import ARRANGEMENTS, BARS, SHAPES, seq_ctl

pytestmark = pytest.mark.gpu

CANARY = np.uint32(0x7FC0DEAD)  # a NaN no rule produces
T_BAR = BARS["unit"]["plog_t"]  # 2.8e-5: p (relative) and plog at t > 0, DESIGN.md §11


@pytest.fixture(scope="module", params=list(SHAPES))
def ctx(request, wrs):
    c = wrs.WhisperContext(model_path(request.param), dtype=wrs.F16)
    assert wrs.lib().whisper_n_vocab(c.ptr) == SHAPES[request.param]
    yield c
    c.close()


def ctl_array(wrs, rows):
    return (wrs.SeqCtl * len(rows))(*[seq_ctl(wrs, r["ctl"]) for r in rows])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stage(wrs, ctx, d, d_raw, ctl, n, flags, d_out):
    assert wrs.lib().whisper_mi355x_debug_logits_stage(ctx.ptr, d_raw, n, ctl, flags, d_out) == 0


def logits_ex(wrs, ctx, d_raw, d_filt, ctl, n, form, flags, V):
    out = (wrs.Cand * n)()
    probs = np.zeros((n, 2, V), np.float32)
    rc = wrs.lib().whisper_mi355x_debug_logits_ex(ctx.ptr, d_raw, d_filt, n, ctl, form, flags, out,
                                                  probs.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return np.frombuffer(out, np.uint8).reshape(n, 32).copy(), out, probs


@pytest.mark.parametrize("tdrz", [0, 1])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_stage_rows(wrs, ctx, n, tdrz):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    rows = lc.matrix(V)[("random", n % 3)][:n]
    assert n == 1 or {r["ctl"]["temperature"] for r in rows} == set(lc.TEMPS)
    raw = np.stack([r["raw"] for r in rows])
    want = np.stack([fr.pre(r["raw"], r["ctl"], v, bool(tdrz)) for r in rows])
    d = Dev(wrs, ctx)
    try:
        d_raw = d.up(raw)
        buf = np.full(n * V + 64, CANARY, np.uint32)
        d_out = d.up(buf)
        stage(wrs, ctx, d, d_raw, ctl_array(wrs, rows), n, tdrz, d_out)
        got = d.down(d_out, buf)
        assert (d.down(d_raw, raw).view(np.uint32) == bits(raw)).all(), "the raw rows were written"
    finally:
        d.free()
    assert (got[n * V:] == CANARY).all(), "written behind the last row"
    got = got[:n * V].reshape(n, V)
    for r, row in enumerate(rows):
        bad = np.nonzero(got[r] != bits(want[r]))[0]
        assert bad.size == 0, f"{V} n {n} tdrz {tdrz} row {r} ({row['what']}, t {row['ctl']['temperature']}): {bad.size} entries differ, first {bad[:4]}"
    if tdrz:
        plain = np.stack([fr.pre(r["raw"], r["ctl"], v, False) for r in rows])
        for r in range(n):
            # (a row whose raw solm entry is -inf already shows no difference)
            assert list(np.nonzero(bits(plain[r]) != got[r])[0]) == ([v["solm"]] if np.isfinite(raw[r, v["solm"]]) else [])


def test_stage_canaries_every_alignment(wrs, ctx):
    """One row per launch at element offsets k V of a canary buffer (input and output aligned alike: the head / 16-byte
    body / tail path) and at offset k V + 1 from an input at k V (aligned differently: the scalar path)."""
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    rows = lc.matrix(V)[("random", 1)][:4]
    raw = np.stack([r["raw"] for r in rows])
    d = Dev(wrs, ctx)
    try:
        d_raw = d.up(raw)
        for shift in (0, 1):
            buf = np.full(4 * V + 72, CANARY, np.uint32)
            d_out = d.up(buf)
            for k, row in enumerate(rows):
                stage(wrs, ctx, d, d_raw + 4 * k * V, ctl_array(wrs, [row]), 1, 0, d_out + 4 * (8 + k * V + shift))
                got = d.down(d_out, buf)
                lo = 8 + k * V + shift
                want = bits(fr.pre(row["raw"], row["ctl"], v))
                assert (got[lo:lo + V] == want).all(), (V, shift, k)
                assert (got[lo - 8:lo] == CANARY).all() or k > 0, (V, shift, k)
                assert (got[lo + V:] == CANARY).all(), f"{V} shift {shift} row {k}: written behind the row"
                if k > 0:  # the row before it is intact
                    prev = bits(fr.pre(rows[k - 1]["raw"], rows[k - 1]["ctl"], v))
                    assert (got[lo - V:lo] == prev).all(), (V, shift, k)
    finally:
        d.free()


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_prefiltered_of_pre_is_plain(wrs, ctx, arrangement):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    form, n = ARRANGEMENTS[arrangement]
    for (kind, rot), all_rows in lc.matrix(V).items():
        rows = all_rows[:n]
        raw = np.stack([r["raw"] for r in rows])
        ctl = ctl_array(wrs, rows)
        d = Dev(wrs, ctx)
        try:
            d_raw = d.up(raw)
            d_filt = d.up(np.full(n * V, CANARY, np.uint32))
            stage(wrs, ctx, d, d_raw, ctl, n, 0, d_filt)
            rec_p, _, probs_p = logits_ex(wrs, ctx, d_raw, None, ctl, n, form, 0, V)
            rec_f, _, probs_f = logits_ex(wrs, ctx, d_raw, d_filt, ctl, n, form, 0, V)
            old = (wrs.Cand * n)()
            probs_o = np.zeros((n, 2, V), np.float32)
            assert wrs.lib().whisper_mi355x_debug_logits(ctx.ptr, d_raw, n, ctl, form, old,
                                                         probs_o.ctypes.data_as(C.POINTER(C.c_float))) == 0
        finally:
            d.free()
        where = f"{V} {kind} {rot} {arrangement}"
        assert (rec_p == np.frombuffer(old, np.uint8).reshape(n, 32)).all(), f"{where}: _ex without rows is not the plain hook"
        assert (bits(probs_p) == bits(probs_o)).all(), where
        bad = np.nonzero((rec_f != rec_p).any(axis=1))[0]
        assert bad.size == 0, f"{where}: records of rows {bad} differ ({[rows[r]['what'] for r in bad]})"
        bad = np.nonzero((bits(probs_f) != bits(probs_p)).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, f"{where}: probs rows {bad} differ"


@pytest.mark.parametrize("tdrz", [False, True])
@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_prefiltered_edited_rows(wrs, ctx, arrangement, tdrz):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    form, n = ARRANGEMENTS[arrangement]
    rows = fc.matrix(V)[tdrz][:n]
    ctl = ctl_array(wrs, rows)
    d = Dev(wrs, ctx)
    try:
        d_raw = d.up(np.stack([r["raw"] for r in rows]))
        d_filt = d.up(np.stack([r["filtered"] for r in rows]))
        _, out, probs = logits_ex(wrs, ctx, d_raw, d_filt, ctl, n, form, int(tdrz), V)
    finally:
        d.free()
    worst = dict(plog_0=0.0, p_0=0.0, plog_t=0.0, p_t=0.0, nosp=0.0)
    for r, row in enumerate(rows):
        ref, c, g = row["ref"], row["ctl"], out[r]
        where = f"{V} {arrangement} tdrz {tdrz} row {r} ({row['what']}, t {c['temperature']})"
        assert (g.id, g.tid) == (ref["id"], ref["tid"]), where
        if c["want_nosp"]:
            worst["nosp"] = max(worst["nosp"], abs(g.no_speech_prob - ref["nosp_prob"]) / (ref["nosp_prob"] + 1e-30))
        else:
            assert g.no_speech_prob == 0.0, where
        if ref["p"] == 0.0:
            assert (g.id, g.tid, g.p, g.plog, g.pt, g.ptsum) == (0, 0, 0.0, -np.inf, 0.0, 0.0), where
        else:
            t = "t" if c["temperature"] > 0 else "0"
            assert np.isfinite(g.plog), where
            worst["plog_" + t] = max(worst["plog_" + t], abs(g.plog - ref["plog"]))
            worst["p_" + t] = max(worst["p_" + t], abs(g.p / ref["p"] - 1.0))
        if not c["want_probs"]:
            assert np.isnan(probs[r]).all(), where
            continue
        lp = probs[r, 1]
        sup = ref["suppressed"]
        assert ((lp == -np.inf) == sup).all(), f"{where}: {int(((lp == -np.inf) != sup).sum())} ids off the suppressed set"
        assert (probs[r, 0][sup] == 0.0).all(), where
    print("logits-filter worst", V, arrangement, tdrz, worst)
    assert worst["plog_0"] <= PLOG_BAR and worst["p_0"] <= P_REL_BAR, worst
    assert worst["plog_t"] <= T_BAR and worst["p_t"] <= T_BAR, worst
    assert worst["nosp"] <= BARS["unit"]["nosp"], worst


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("split,n", [(1, 16), (1, 17), (0, 1)])
def test_prefiltered_topk(wrs, ctx, split, n, k):
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    rows = [dict(r, ctl=dict(r["ctl"], temperature=0.0, want_probs=0)) for r in fc.matrix(V)[True][:n]]  # beam rows are t = 0 rows
    ctl = ctl_array(wrs, rows)
    cand, greedy = (wrs.Cand * (n * k))(), (wrs.Cand * n)()
    d = Dev(wrs, ctx)
    try:
        d_raw = d.up(np.stack([r["raw"] for r in rows]))
        d_filt = d.up(np.stack([r["filtered"] for r in rows]))
        assert wrs.lib().whisper_mi355x_debug_logits_topk_ex(ctx.ptr, d_raw, d_filt, n, ctl, k, split, 1, cand, greedy) == 0
        _, single, _ = logits_ex(wrs, ctx, d_raw, d_filt, ctl, n, split, 1, V)
    finally:
        d.free()
    g8 = np.frombuffer(greedy, np.uint8).reshape(n, 32)
    c8 = np.frombuffer(cand, np.uint8).reshape(n, k, 32)
    assert (g8 == np.frombuffer(single, np.uint8).reshape(n, 32)).all(), "the hook's greedy record is not logits_ex's"
    for r, row in enumerate(rows):
        where = f"{V} split {split} n {n} k {k} row {r} ({row['what']})"
        assert (c8[r, 0] == g8[r]).all(), f"{where}: candidate 0 is not the greedy record"
        ref = row["ref"]
        best = np.sort(ref["logprobs"])[::-1]
        seen = set()
        for j in range(k):
            c = cand[r * k + j]
            alive = j < int((ref["probs"].astype(np.float32) > 0).sum())
            if ref["p"] == 0.0:
                assert c.id == (0 if j == 0 else -1), where
                continue
            if not alive or c.id < 0:  # (float p underflows where the reference's p is denormal: either may stop first)
                assert best[j] < -80.0, f"{where}: candidate {j} is missing"
                assert all(cand[r * k + q].id == -1 for q in range(j + 1, k) if c.id < 0), where
                continue
            assert c.id not in seen and not ref["suppressed"][c.id], f"{where}: candidate {j} id {c.id}"
            seen.add(c.id)
            # in order: candidate j carries the reference's j-th largest logprob
            assert abs(ref["logprobs"][c.id] - best[j]) <= 2 * PLOG_BAR, f"{where}: candidate {j} id {c.id} is out of order"
            assert abs(c.plog - ref["logprobs"][c.id]) <= PLOG_BAR, where
            if j > 0:
                assert c.p <= cand[r * k + j - 1].p, where
