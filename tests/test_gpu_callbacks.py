"""The callbacks of whisper_full_params and the early error returns of a full call (engine.cpp full_batch_one and
its passes): what a caller of whisper.h observes of the scheduler besides the results.

whisper_full_with_state asks, per window and in this order: the progress callback, the encoder-begin callback
(false stops the call), the abort callback; then the abort callback again before the prefill and before every
decode step; the new-segment callback once the window's segments are stored. A stopped call returns 0 with the
windows finished so far. The batch API asks the abort callback only. Every case runs the tiny fixture model in
f16 on one 45 s clip (more than one window), greedy at t = 0 (temperature_inc = 0)."""
import ctypes as C

import numpy as np
import pytest

from make_model import synthetic_pcm

pytestmark = pytest.mark.gpu

SEG_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)  # whisper_new_segment_callback
PROG_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)  # whisper_progress_callback
ENC_CB = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.c_void_p)  # whisper_encoder_begin_callback
ABORT_CB = C.CFUNCTYPE(C.c_bool, C.c_void_p)  # ggml_abort_callback


def seg_ints(segs):
    return [([t[0] for t in s.tokens], s.t0, s.t1, s.text) for s in segs]


def params(wrs, language="en"):
    p = wrs.reference_full_params(language)
    p.temperature_inc = 0.0
    return p


def install(p, events, enc_false_at=None, abort_at=None):
    """All four callbacks on p, each appending to events; the encoder-begin callback returns false on its
    enc_false_at-th call, the abort callback true from its abort_at-th. Returns the ctypes objects to keep alive."""
    def count(name):
        return sum(1 for e in events if e[0] == name)

    def on_seg(_c, _s, n_new, _u):
        events.append(("new_segment", n_new))

    def on_prog(_c, _s, prog, _u):
        events.append(("progress", prog))

    def on_enc(_c, _s, _u):
        events.append(("encoder_begin",))
        return not (enc_false_at is not None and count("encoder_begin") == enc_false_at)

    def on_abort(_u):
        events.append(("abort",))
        return abort_at is not None and count("abort") >= abort_at
    keep = [SEG_CB(on_seg), PROG_CB(on_prog), ENC_CB(on_enc), ABORT_CB(on_abort)]
    p.new_segment_callback, p.progress_callback, p.encoder_begin_callback, p.abort_callback = \
        (C.cast(f, C.c_void_p) for f in keep)
    return keep


def windows(events):
    """The event list cut before every progress event."""
    out = []
    for e in events:
        if e[0] == "progress" or not out:
            out.append([])
        out[-1].append(e)
    return out


@pytest.fixture(scope="module")
def pcm():
    return synthetic_pcm(0, seconds=45.0)


@pytest.fixture(scope="module")
def unaborted(wrs, tiny_model, pcm):
    """The run no callback stops: (events, segments, decisions, n_len)."""
    L = wrs.lib()
    L.whisper_n_len_from_state.restype = C.c_int
    L.whisper_n_len_from_state.argtypes = [C.c_void_p]
    ctx = wrs.WhisperContext(tiny_model, dtype=wrs.F16)
    st = ctx.create_state()
    p = params(wrs)
    events = []
    keep = install(p, events)
    assert st.full(p, pcm) == 0
    out = (events, seg_ints(st.segments()), st.decisions(), L.whisper_n_len_from_state(st.ptr))
    del keep
    st.close()
    ctx.close()
    return out


def test_callback_order(unaborted, pcm):
    events, segs, dec, n_len = unaborted
    print("events:", events)
    assert n_len == 1 + (len(pcm) - 200) // 160
    assert len(dec) >= 2 and len(segs) > 0
    win = windows(events)
    assert len(win) == len(dec)
    assert sum(1 for e in events if e[0] == "progress") == len(dec)
    assert sum(1 for e in events if e[0] == "encoder_begin") == len(dec)
    for w, d in zip(win, dec):
        assert [e[0] for e in w[:3]] == ["progress", "encoder_begin", "abort"], w
        assert w[0][1] == 100 * (d["seek"] - 0) // max(1, n_len - 0), (w[0], d["seek"])
        # its new-segment event (if any) follows the window's last abort call and precedes the next progress
        names = [e[0] for e in w[3:]]
        n_seg = names.count("new_segment")
        assert n_seg <= 1 and names == ["abort"] * (len(names) - n_seg) + ["new_segment"] * n_seg, w
    assert sum(e[1] for e in events if e[0] == "new_segment") == len(segs)


def test_encoder_begin_false_stops(wrs, tiny_model, pcm, unaborted):
    ref_events, ref_segs, _, _ = unaborted
    n_first = sum(e[1] for e in windows(ref_events)[0] if e[0] == "new_segment")
    ctx = wrs.WhisperContext(tiny_model, dtype=wrs.F16)
    st = ctx.create_state()
    p = params(wrs)
    events = []
    keep = install(p, events, enc_false_at=2)
    assert st.full(p, pcm) == 0
    assert seg_ints(st.segments()) == ref_segs[:n_first]
    assert events[-1] == ("encoder_begin",) and sum(1 for e in events if e[0] == "encoder_begin") == 2, events[-4:]
    assert events == ref_events[:len(events)]
    del keep
    st.close()
    ctx.close()


def test_abort_at_first_call(wrs, tiny_model, pcm):
    ctx = wrs.WhisperContext(tiny_model, dtype=wrs.F16)
    st = ctx.create_state()
    p = params(wrs)
    events = []
    keep = install(p, events, abort_at=1)
    assert st.full(p, pcm) == 0
    assert st.full_n_segments() == 0
    assert events == [("progress", 0), ("encoder_begin",), ("abort",)]
    del keep
    assert st.full(params(wrs), pcm) == 0  # the same state, no callbacks
    assert st.full_n_segments() > 0
    st.close()
    ctx.close()


def test_batch_api_makes_no_single_clip_callbacks(wrs, tiny_model, pcm):
    ctx = wrs.WhisperContext(tiny_model, dtype=wrs.F16)
    st = ctx.create_state()
    p = params(wrs)
    events = []
    keep = install(p, events)
    assert st.full_batch(p, [pcm, synthetic_pcm(1)]) == 0
    assert len(st.batch_segments(0)) > 0 and len(st.batch_segments(1)) > 0
    assert events and set(events) == {("abort",)}, set(events)
    del keep
    st.close()
    ctx.close()


# ---- error returns ------------------------------------------------------------------------------------------------
def transcribes(wrs, st, pcm):
    """The state is usable after the error: it transcribes a real clip."""
    assert st.full(params(wrs), pcm) == 0
    return st.full_n_segments() > 0


def test_unknown_strategy_returns_minus_100(wrs, tiny_model, pcm):
    ctx = wrs.WhisperContext(tiny_model, dtype=wrs.F16)
    st = ctx.create_state()
    p = params(wrs)
    p.strategy = 7
    assert st.full(p, pcm) == -100
    assert st.full_batch(p, [pcm]) == -100
    assert transcribes(wrs, st, pcm)
    st.close()
    ctx.close()


def test_unknown_language_returns_minus_7(wrs, tiny_model, pcm):
    """A language code that is not in the table, on a multilingual model: the prompt cannot be built."""
    ctx = wrs.WhisperContext(tiny_model, dtype=wrs.F16)
    assert ctx.L.whisper_is_multilingual(ctx.ptr) == 1
    st = ctx.create_state()
    assert st.full(params(wrs, "zz"), pcm) == -7
    assert st.full_n_segments() == 0
    assert st.full_batch(params(wrs, "zz"), [pcm]) == -7
    assert transcribes(wrs, st, pcm)
    st.close()
    ctx.close()


def test_auto_detect_without_audio(wrs, tiny_model, pcm):
    """Language auto-detection on 40 samples (no mel frame): whisper_full_with_state fails with -3; the batch API
    ends that clip without a result."""
    ctx = wrs.WhisperContext(tiny_model, dtype=wrs.F16)
    st = ctx.create_state()
    p = params(wrs, None)
    none = np.zeros(40, np.float32)
    assert st.full(p, none) == -3
    assert st.full_n_segments() == 0
    assert transcribes(wrs, st, pcm)
    assert st.full_batch(p, [none]) == 0
    assert len(st.batch_segments(0)) == 0
    assert transcribes(wrs, st, pcm)
    st.close()
    ctx.close()
