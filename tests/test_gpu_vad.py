"""whisper_full_params.vad and the whisper_vad_* block end to end on the device, with the "gate" model of
tools/make_vad_model.py (an energy detector) and the tiny+conf Whisper model.

Condition of the exact comparisons, asserted on the CPU reference before the GPU is used: no window of a test signal has a
probability within 1e-3 of threshold or neg_threshold (the kernels agree with the reference to about 1e-6). With it the
device's segments, piece tables and filtered audio equal the reference's exactly."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, model_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_vad_model as mk  # noqa: E402
import vad_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu

K_GEMM_ENC, K_VAD = 0, 17
LAYOUTS = [((1.0, 3.5), (5.0, 7.5), (9.0, 11.0)), ((0.0, 2.0), (2.6, 4.0)), ()]
SECONDS = [12.0, 6.0, 3.0]


def clip(k):
    return mk.burst_signal(SECONDS[k], seed=k, bursts=LAYOUTS[k])


@pytest.fixture(scope="module")
def env(wrs, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vad_e2e") / "gate.bin")
    model = mk.write_vad_model(path, "gate", 0)
    ctx = wrs.WhisperContext(model_path("tiny+conf"))
    ref = []
    for k in range(3):
        x = clip(k)
        p = vr.probs(model, x, np.float64)
        assert np.abs(p - 0.5).min() > 1e-3 and np.abs(p - 0.35).min() > 1e-3, k   # the condition
        segs = vr.segments_from_probs(p, vr.default_params())
        ref.append(dict(x=x, p=p, segs=segs, table=vr.piece_table(segs, len(x), 0.1)))
    assert [len(r["segs"]) for r in ref] == [3, 2, 0]
    yield dict(path=path, model=model, ctx=ctx, ref=ref)
    ctx.close()


def params(wrs, vad_path=None, **kw):
    p = wrs.reference_full_params("en")
    p.temperature_inc = 0.0   # one greedy attempt per window: nothing is drawn, so runs compare token for token
    p.token_timestamps = True
    for k, v in kw.items():
        setattr(p, k, v)
    if vad_path is not None:
        p.vad = True
        p.vad_model_path = vad_path.encode() if isinstance(vad_path, str) else vad_path
    return p


def result(st, job=0):
    segs = st.batch_segments(job)
    toks = st.token_data(job)
    return [(s.t0, s.t1, s.text, [(d["id"], d["p"], d["plog"], d["t0"], d["t1"], d["t_dtw"]) for d in td]) for s, td in zip(segs, toks)]


def mapped(res, table):
    m = lambda t: t if t == -1 else vr.map_time(table, t)
    return [(vr.map_time(table, t0), vr.map_time(table, t1), text, [(i, p, pl, m(a), m(b), m(c)) for i, p, pl, a, b, c in toks])
            for t0, t1, text, toks in res]


def test_segments_equal_the_reference(wrs, env):
    v = wrs.VadContext(env["path"])
    for r in env["ref"]:
        want = [(float(a), float(b)) for a, b in vr.segment_times(r["segs"])]
        assert v.segments_from_samples(r["x"]) == want
        assert v.detect_speech(r["x"]) and v.segments_from_probs() == want
        assert np.abs(v.probs() - r["p"]).max() < 1e-5
    # other parameters than the defaults go through as well
    q = wrs.lib().whisper_vad_default_params()
    q.min_silence_duration_ms, q.speech_pad_ms, q.max_speech_duration_s = 300, 100, 1.0
    prm = dict(vr.default_params(), min_silence_duration_ms=300, speech_pad_ms=100, max_speech_duration_s=1.0)
    r = env["ref"][0]
    want = [(float(a), float(b)) for a, b in vr.segment_times(vr.segments_from_probs(r["p"], prm))]
    assert len(want) > 3 and v.segments_from_samples(r["x"], q) == want
    v.close()


def test_full_with_vad_equals_full_on_the_filtered_audio(wrs, env):
    r = env["ref"][0]
    ctx = env["ctx"]
    plain = ctx.create_state()
    assert plain.full(params(wrs), vr.filtered_pcm(r["x"], r["table"])) == 0
    want, want_dec = result(plain), plain.decisions()
    assert plain.vad_ms() == 0 and plain.vad_map() == []
    plain.close()
    assert len(want) > 0 and any(t[3] >= 0 for s in want for t in s[3])
    st = ctx.create_state()
    assert st.full(params(wrs, env["path"]), r["x"]) == 0
    got, dec = result(st), st.decisions()
    assert st.vad_map() == r["table"]
    assert st.vad_ms() > 0
    st.close()
    assert dec == want_dec                      # (seek stays on the filtered axis)
    assert got == mapped(want, r["table"])
    assert got != want                          # the times moved: this fails where vad is ignored
    assert all(s[0] <= s[1] <= len(r["x"]) // 160 for s in got)   # (a time beyond the filtered audio maps to the last piece's end)


def test_offset_and_duration_apply_to_the_filtered_audio(wrs, env):
    r = env["ref"][0]
    ctx = env["ctx"]
    plain = ctx.create_state()
    assert plain.full(params(wrs, offset_ms=1000, duration_ms=2500), vr.filtered_pcm(r["x"], r["table"])) == 0
    want = result(plain)
    plain.close()
    st = ctx.create_state()
    assert st.full(params(wrs, env["path"], offset_ms=1000, duration_ms=2500), r["x"]) == 0
    assert result(st) == mapped(want, r["table"]) and len(want) > 0
    st.close()


def test_all_silence(wrs, env):
    r = env["ref"][2]
    st = env["ctx"].create_state()
    L = wrs.lib()
    assert L.whisper_mi355x_kernel_timing(st.ptr, (1 << K_GEMM_ENC) | (1 << K_VAD)) == 0
    assert st.full(params(wrs, env["path"]), r["x"]) == 0
    assert st.full_n_segments() == 0 and st.vad_map() == [] and st.vad_ms() > 0
    out = (3 * __import__("ctypes").c_double)()
    assert L.whisper_mi355x_kernel_stats(st.ptr, K_GEMM_ENC, out) == 0 and out[1] == 0      # nothing was encoded
    assert L.whisper_mi355x_kernel_stats(st.ptr, K_VAD, out) == 0 and out[1] >= 2 and out[0] > 0
    split = st.vad_kernel_stats()   # class 17 by kernel: one launch of each, and the parts add up to the class
    assert [split[k][1] for k in ("frontend", "lstm", "gather")] == [1, 1, 1]
    assert abs(sum(v[0] for v in split.values()) - out[0]) < 1e-6
    # language detection on a clip without speech: no audio is left to detect on, and the call still returns 0
    assert st.full(params(wrs, env["path"], language=None), r["x"]) == 0 and st.full_n_segments() == 0
    st.close()


def test_bad_model_path(wrs, env, tmp_path, capfd):
    r = env["ref"][1]
    kw = dict(no_context=True, token_timestamps=False)   # nothing of a call is carried to the state's next call
    st = env["ctx"].create_state()
    assert st.full(params(wrs, **kw), r["x"]) == 0
    want = result(st)
    bad = tmp_path / "truncated.bin"
    bad.write_bytes(open(env["path"], "rb").read()[:5000])
    capfd.readouterr()
    for path in (str(tmp_path / "missing.bin"), str(bad)):
        assert st.full(params(wrs, path, **kw), r["x"]) == wrs.VAD_ERR == -11
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and "vad model" in err
    p = params(wrs, **kw)
    p.vad = True   # vad without a path
    assert st.full(p, r["x"]) == -11
    assert st.full(params(wrs, **kw), r["x"]) == 0 and result(st) == want      # the state stays usable
    st.close()


def test_batch_equals_single_calls(wrs, env):
    ctx = env["ctx"]
    single = []
    for r in env["ref"]:
        st = ctx.create_state()
        assert st.full(params(wrs, env["path"]), r["x"]) == 0
        single.append((result(st), st.vad_map()))
        st.close()
    st = ctx.create_state()
    assert st.full_batch(params(wrs, env["path"]), [r["x"] for r in env["ref"]]) == 0
    for j, (res, table) in enumerate(single):
        assert result(st, j) == res and st.vad_map(j) == table == env["ref"][j]["table"]
    assert single[2][0] == [] and len(single[0][0]) > 0 and len(single[1][0]) > 0
    st.close()


def test_vad_off_is_unchanged_by_a_vad_call(wrs, env):
    r = env["ref"][1]
    kw = dict(no_context=True, token_timestamps=False)   # nothing of a call is carried to the state's next call
    st = env["ctx"].create_state()
    assert st.full(params(wrs, **kw), r["x"]) == 0
    before = result(st)
    assert st.full(params(wrs, env["path"], **kw), r["x"]) == 0 and st.vad_ms() > 0
    assert st.full(params(wrs, **kw), r["x"]) == 0
    assert result(st) == before and st.vad_ms() == 0 and st.vad_map() == []
    st.close()


def test_paired_batch_filters_each_half(wrs, env):
    """more than 128 clips run as two halves on two states: each half filters its own jobs, and the maps come back in
    job order. (Probabilities differ in the last digits between batch sizes, which take other GEMM and attention forms:
    token ids, texts, times and maps are compared.)"""
    ids = lambda res: [(t0, t1, text, [(i, a, b, c) for i, _, _, a, b, c in toks]) for t0, t1, text, toks in res]
    a, b = env["ref"][1], env["ref"][2]
    n = 130
    clips = [(a if j % 3 else b)["x"] for j in range(n)]
    st = env["ctx"].create_state()
    assert st.full_batch(params(wrs, env["path"]), clips) == 0
    small = env["ctx"].create_state()
    assert small.full_batch(params(wrs, env["path"]), [a["x"], b["x"]]) == 0
    want = {True: (ids(result(small, 0)), a["table"]), False: (ids(result(small, 1)), b["table"])}
    small.close()
    for j in (0, 1, 64, 65, 66, 128, 129):
        res, table = want[bool(j % 3)]
        assert st.vad_map(j) == table and ids(result(st, j)) == res, j
    assert st.vad_ms() > 0
    st.close()
