"""whisper_full_parallel / whisper_mi355x_full_parallel on the device: the pieces of one recording as one
batch, merged on the recording's axis.

Every result is compared with two references:
  * the CPU oracle's whisper_full of each piece (piece 0 with the caller's offset_ms, the others with 0, each on a fresh
    state), merged by tests/parallel_ref.py: segment texts, t0 / t1, token ids and the window decisions. The oracle has no
    token_timestamps, so token t0 / t1 are compared with the second reference only;
  * as many whisper_full_with_state calls on the device, piece 0 on the state the parallel call runs on and the others on
    fresh states, merged by parallel_ref: everything above and every token's t0 / t1 / t_dtw.
The inputs (tests/parallel_cases.py) are such that the oracle decides every window of every piece at t = 0 and no greedy
step is closer than 0.05 nats to a tie; parallel_cases.check_oracle asserts it for every oracle result used here.
Beam search, the carried prompt on the second call and vad have no oracle: they are compared with the separate calls.
"""
import ctypes as C

import numpy as np
import pytest

import make_vad_model as mk
import parallel_cases as pc
import parallel_ref as pr
from conftest import model_path
from margin_gate import DEC_KEYS
from test_gpu_callbacks import ABORT_CB, ENC_CB, PROG_CB, SEG_CB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def path():
    return model_path(pc.SHAPE)


@pytest.fixture(scope="module")
def ctx(wrs, path):
    c = wrs.WhisperContext(path, dtype=wrs.F16)
    yield c
    c.close()


def params(wrs, beam=0, **kw):
    p = wrs.beam_full_params(beam) if beam else wrs.reference_full_params("en")
    p.max_tokens = pc.MAX_TOKENS
    p.token_timestamps = True
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def result(st):
    """The state's whisper_full_* view as parallel_ref's segments."""
    return [dict(t0=s.t0, t1=s.t1, text=s.text, tokens=[dict(id=d["id"], t0=d["t0"], t1=d["t1"], t_dtw=d["t_dtw"]) for d in td])
            for s, td in zip(st.segments(), st.token_data(0))]


def plain(segs):
    return [(s["t0"], s["t1"], s["text"], [t["id"] if isinstance(t, dict) else t for t in s["tokens"]]) for s in segs]


def dec_ints(decs):
    return [tuple(d[k] for k in DEC_KEYS) for d in decs]


def separate(ctx, make_params, rec, cuts, offset_ms=0, st0=None):
    """One whisper_full_with_state per piece: piece 0 on st0 (or a fresh state), the others on fresh states."""
    segs, decs = [], []
    for k, x in enumerate(pc.piece_pcm(rec, cuts)):
        st = st0 if k == 0 and st0 is not None else ctx.create_state()
        p = make_params()
        p.offset_ms = offset_ms if k == 0 else 0
        assert st.full(p, x) == 0
        segs.append(result(st))
        decs.append(st.decisions())
        if st is not st0:
            st.close()
    return segs, decs


@pytest.mark.parametrize("name,n,offset_ms", [("rec40", 3, 0), ("rec70", 2, 0), ("rec40", 3, 2000)])
def test_merge_parity(wrs, ctx, path, name, n, offset_ms):
    rec = pc.recording(name)
    cuts = pr.cuts(len(rec), offset_ms, n)
    ora = pc.oracle_pieces(path, name, cuts, offset_ms)
    pc.check_oracle(ora)
    if name == "rec70":
        assert all(len(r["decisions"]) > 1 for r in ora)      # each piece runs its own seek loop ...
    else:
        assert all(len(r["decisions"]) == 1 for r in ora)     # ... or is one window
    want_ora = pr.merge(pc.oracle_segments(ora), cuts, offset_ms)
    want_ora_dec = pr.merge_decisions([r["decisions"] for r in ora], cuts, offset_ms)

    st = ctx.create_state()
    assert st.full_parallel(params(wrs, offset_ms=offset_ms), rec, n) == 0
    got, got_dec = result(st), st.decisions()
    assert st.parallel_cuts() == cuts
    st.close()
    sep, sep_dec = separate(ctx, lambda: params(wrs), rec, cuts, offset_ms)
    want = pr.merge(sep, cuts, offset_ms)
    print(f"{name} n={n} offset {offset_ms}: {len(got)} segments, pieces {[len(s) for s in sep]}, windows {[len(d) for d in sep_dec]}")
    assert len(got) >= n and all(len(s) > 0 for s in sep)
    assert plain(got) == plain(want_ora)
    assert dec_ints(got_dec) == dec_ints(want_ora_dec)
    assert got == want
    assert dec_ints(got_dec) == dec_ints(pr.merge_decisions(sep_dec, cuts, offset_ms))
    # token times are there, and those of the later pieces lie on the recording's axis
    last = [t for t in got[-1]["tokens"] if t["t0"] >= 0]
    assert last and all(t["t0"] >= pr.shift(cuts[-1], offset_ms) for t in last)
    assert all(a["t1"] <= b["t0"] for a, b in zip(got, got[1:]))


def test_carried_prompt(wrs, ctx):
    """no_context = false: piece 0 of a second call starts from what the first call left in the state's prompt_past, the
    other pieces from nothing."""
    rec = pc.recording("rec40")
    cuts = pr.cuts(len(rec), 0, 3)
    st = ctx.create_state()
    got = []
    for _ in range(2):
        assert st.full_parallel(params(wrs), rec, 3) == 0
        got.append(result(st))
    st.close()
    st0 = ctx.create_state()
    want, sep0 = [], []
    for _ in range(2):
        sep, _dec = separate(ctx, lambda: params(wrs), rec, cuts, st0=st0)
        sep0.append(sep[0])
        want.append(pr.merge(sep, cuts))
    st0.close()
    assert got[0] == want[0] and got[1] == want[1]
    print("piece 0, first / second call:", plain(sep0[0]), plain(sep0[1]))


def install(p, log, state_view=None, abort_at=None):
    def on_seg(_c, s, n_new, _u):
        log.append(("new_segment", n_new, state_view(s) if state_view else None))

    def on_prog(_c, _s, prog, _u):
        log.append(("progress", prog))

    def on_enc(_c, _s, _u):
        log.append(("encoder_begin",))
        return True

    def on_abort(_u):
        log.append(("abort",))
        return abort_at is not None and sum(1 for e in log if e[0] == "abort") >= abort_at
    keep = [SEG_CB(on_seg), PROG_CB(on_prog), ENC_CB(on_enc), ABORT_CB(on_abort)]
    p.new_segment_callback, p.progress_callback, p.encoder_begin_callback, p.abort_callback = (C.cast(f, C.c_void_p) for f in keep)
    return keep


def test_callbacks(wrs, ctx):
    L = wrs.lib()
    rec = pc.recording("rec70")
    cuts = pr.cuts(len(rec), 0, 2)

    def view(s):   # the newest segment through the getters, at the time of the callback
        n = L.whisper_full_n_segments_from_state(s)
        return (n, L.whisper_full_get_segment_t0_from_state(s, n - 1), L.whisper_full_get_segment_t1_from_state(s, n - 1),
                L.whisper_full_get_segment_text_from_state(s, n - 1))
    st = ctx.create_state()
    p, log = params(wrs), []
    keep = install(p, log, view)
    assert st.full_parallel(p, rec, 2) == 0
    segs, decs = st.segments(), st.decisions()
    st.close()
    seg_events = [e for e in log if e[0] == "new_segment"]
    assert sum(e[1] for e in seg_events) == len(segs) > 2
    seen = 0
    for _, n_new, (n_now, t0, t1, text) in seg_events:
        seen += n_new
        assert n_now == seen and (t0, t1, text) == (segs[seen - 1].t0, segs[seen - 1].t1, segs[seen - 1].text)
    # the pieces' segments come one by one after the batch, piece 0's as its windows finish
    n0 = sum(1 for s in segs if s.t0 < pr.shift(cuts[1], 0))
    assert [e[1] for e in seg_events if e[2][0] > n0] == [1] * (len(segs) - n0)
    # the progress callback only ever reports piece 0: what a lone call on piece 0 reports
    lone = ctx.create_state()
    p0, log0 = params(wrs), []
    keep0 = install(p0, log0)
    assert lone.full(p0, rec[:cuts[1]]) == 0
    lone.close()
    prog = [e for e in log if e[0] == "progress"]
    assert prog == [e for e in log0 if e[0] == "progress"] and len(prog) >= 2
    # encoder_begin_callback holds for every piece: once per window
    assert sum(1 for e in log if e[0] == "encoder_begin") == len(decs)
    del keep, keep0

    st = ctx.create_state()
    p, log = params(wrs), []
    keep = install(p, log, view, abort_at=1)
    assert st.full_parallel(p, rec, 2) == 0
    assert st.full_n_segments() == 0 and st.decisions() == []
    assert sum(1 for e in log if e[0] == "abort") == 1 and not any(e[0] == "new_segment" for e in log)
    st.close()
    del keep


def test_one_processor_is_whisper_full(wrs, ctx, path):
    rec = pc.recording("rec40")
    a = ctx.create_state()
    assert a.full(params(wrs), rec) == 0
    want, want_dec = result(a), a.decisions()
    a.close()
    for n in (1, 0):
        b = ctx.create_state()
        assert b.full_parallel(params(wrs), rec, n) == 0
        assert result(b) == want and b.decisions() == want_dec and b.parallel_cuts() == [0]
        b.close()
    assert len(want) > 1 and len(want_dec) >= 2
    # whisper.h's own entry point, on the default state
    c = wrs.WhisperContext.new_with_default_state(path)
    assert c.full_parallel(params(wrs), rec, 1) == 0
    assert c.default_segments() == [(s["t0"], s["t1"], s["text"]) for s in want]
    assert c.full_parallel(params(wrs, no_context=True), rec, 3) == 0
    three = c.default_segments()
    c.close()
    st = ctx.create_state()
    assert st.full_parallel(params(wrs, no_context=True), rec, 3) == 0
    assert three == [(s["t0"], s["t1"], s["text"]) for s in result(st)] != [(s["t0"], s["t1"], s["text"]) for s in want]
    st.close()


def test_beam_groups(wrs, ctx, capfd):
    """beam_size 5 x 8 pieces = 40 rows > 32: groups of 6 and 2 jobs."""
    rec = pc.recording("rec40")
    cuts = pr.cuts(len(rec), 0, 8)
    mk_p = lambda: params(wrs, beam=5, temperature_inc=0.0)
    st = ctx.create_state()
    assert st.full_parallel(mk_p(), rec, 8) == 0
    got, got_dec = result(st), st.decisions()
    assert len(st.beam_info(0)) == 5      # piece 0's beams, as after a lone call
    sep, sep_dec = separate(ctx, mk_p, rec, cuts)
    assert all(len(s) > 0 for s in sep)
    assert got == pr.merge(sep, cuts)
    assert dec_ints(got_dec) == dec_ints(pr.merge_decisions(sep_dec, cuts))   # (the integer outcomes: a row's low bits depend on the step's row count)
    capfd.readouterr()
    assert st.full_batch(mk_p(), pc.piece_pcm(rec, cuts)) == -1      # the batch API is as it was
    assert "exceeds 32 decoder rows" in capfd.readouterr().err
    st.close()


def test_snap(wrs, ctx, path):
    rec = pc.recording("rec40")
    n, snap_ms = 3, 1000
    equal = pr.cuts(len(rec), 0, n)
    cuts = pr.snapped_cuts(pr.window_rms(rec), len(rec), 0, n, snap_ms)
    # the pauses do not sit at the equal cuts: both interior cuts move
    assert all(a != b for a, b in zip(cuts[1:], equal[1:])) and all(abs(a - b) <= 16 * snap_ms + 160 for a, b in zip(cuts, equal))
    ora = pc.oracle_pieces(path, "rec40", cuts)
    pc.check_oracle(ora)
    st = ctx.create_state()
    assert st.mi355x_full_parallel(params(wrs), rec, n, snap_ms) == 0
    assert st.parallel_cuts() == cuts
    got, got_dec = result(st), st.decisions()
    sep, sep_dec = separate(ctx, lambda: params(wrs), rec, cuts)
    assert got == pr.merge(sep, cuts) and dec_ints(got_dec) == dec_ints(pr.merge_decisions(sep_dec, cuts))
    assert plain(got) == plain(pr.merge(pc.oracle_segments(ora), cuts))
    # PCM already in HBM: the same cuts and the same result
    L = wrs.lib()
    x = np.ascontiguousarray(rec, np.float32)
    d = L.whisper_mi355x_dev_alloc(ctx.ptr, x.nbytes)
    assert d and L.whisper_mi355x_memcpy(ctx.ptr, C.c_void_p(d), x.ctypes.data, x.nbytes, 1) == 0
    assert st.mi355x_full_parallel(params(wrs, no_context=True), (d, len(x)), n, snap_ms, on_device=True) == 0
    L.whisper_mi355x_dev_free(ctx.ptr, C.c_void_p(d))
    assert st.parallel_cuts() == cuts and result(st) == got
    # snap_ms = 0: upstream's cuts
    assert st.mi355x_full_parallel(params(wrs, no_context=True), rec, n, 0) == 0
    assert st.parallel_cuts() == equal
    st.close()


def test_vad_two_pieces(wrs, ctx, tmp_path):
    """Every piece is filtered and mapped back on its own; then the merge shifts the mapped times."""
    vad_path = str(tmp_path / "gate.bin")
    mk.write_vad_model(vad_path, "gate", 0)
    x = mk.burst_signal(12.0, seed=0, bursts=((1.0, 3.5), (5.0, 7.5), (9.0, 11.0)))
    cuts = pr.cuts(len(x), 0, 2)
    mk_p = lambda: params(wrs, temperature_inc=0.0, vad=True, vad_model_path=vad_path.encode())
    st = ctx.create_state()
    assert st.full_parallel(mk_p(), x, 2) == 0
    got = result(st)
    st.close()
    sep, _ = separate(ctx, mk_p, x, cuts)
    assert all(len(s) > 0 for s in sep)
    assert got == pr.merge(sep, cuts)
    # on the original axis: piece 1's segments begin at its first burst's place in the recording, not at its cut
    first = got[len(sep[0])]
    assert first["t0"] >= pr.shift(cuts[1], 0) and got[-1]["t1"] <= len(x) // 160
    plain_st = ctx.create_state()
    assert plain_st.full_parallel(params(wrs, temperature_inc=0.0), x, 2) == 0
    assert result(plain_st) != got       # the filter ran
    plain_st.close()
