"""whisper_full_params.audio_ctx on the GPU: the encoder, the cross K/V and every cross attention of a
call work on the first A = audio_ctx positions of each window.

The reference is the CPU oracle on a model file truncated to n_audio_ctx = A (tests/audio_ctx_ref.py): that file IS
whisper.cpp at audio_ctx = A. All cases are f16 with language "en" (unless the case is about the detection), no prompt,
temperature_inc = 0 on both sides (unless the case is about the fallback) and synthetic_pcm(clip) at 30 s, which has
speech at frame 2A for every A here: a right pad that is not zero fails the encoder case.

Tolerances are the project's own: the encoder bars of test_gpu_parity.py::test_encoder_matches_oracle, the logits bar
of test_decoder_logits_match_oracle, and F16_GAP = 0.05 nats of test_gpu_pdec.py / test_quant.py /
test_gpu_fulldepth.py: where the oracle decides every kept token by more than that, token ids, t0 / t1, text and
window decisions must equal the oracle's.
"""
import ctypes as C

import numpy as np
import pytest

from audio_ctx_ref import oracle_full_at, truncated_model
from conftest import model_path
from make_model import synthetic_pcm
from margin_gate import assert_closed_before_divergence, assert_diverges_only_at_close_calls, kept_token_margins
from oracle_py import Oracle

pytestmark = pytest.mark.gpu

K_PDEC = 7
F16_GAP = 0.05
DEC_KEYS = ("seek", "temp_idx", "failed0", "logprob_fail0", "result_len0", "no_speech")

_CTX = {}
_PCM = {}


def get_ctx(wrs, shape, **kw):
    key = (shape, tuple(sorted(kw.items())))
    if key not in _CTX:
        _CTX[key] = wrs.WhisperContext(model_path(shape), dtype=wrs.F16, **kw)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_ctxs():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    _PCM.clear()


def pcm_of(clip, seconds=30.0):
    if (clip, seconds) not in _PCM:
        _PCM[(clip, seconds)] = synthetic_pcm(clip, seconds=seconds)
    return _PCM[(clip, seconds)]


def params(wrs, A, lang="en", t_inc=0.0):
    p = wrs.reference_full_params(lang)
    p.temperature_inc = t_inc
    p.audio_ctx = A
    return p


def ints(segs):
    return [([t[0] for t in s.tokens], s.t0, s.t1) for s in segs]


def ref_ints(ref):
    return [(s["tokens"], s["t0"], s["t1"]) for s in ref["segments"]]


def bits(st, job=0):
    """everything a call leaves for a job: segment times and text, every whisper_token_data field, the decisions"""
    segs = st.batch_segments(job)
    return [(s.t0, s.t1, s.text) for s in segs], st.token_data(job), st.decisions(job)


def pdec_launches(wrs, st):
    out = (C.c_double * 3)()
    assert wrs.lib().whisper_mi355x_kernel_stats(st.ptr, K_PDEC, out) == 0
    return int(out[1])


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- 1. encoder output ----------------------------------------------------------------------------------------------
_ENC_REF = {}


def encoder_ref(A):
    if A not in _ENC_REF:
        o = Oracle(truncated_model(model_path("tiny"), A), mode=1)
        o.mel(pcm_of(0))
        _ENC_REF[A] = o.encode(0)
        o.close()
    return _ENC_REF[A]


def gpu_encode(wrs, ctx, st, A, pcm):
    L = wrs.lib()
    assert st.set_audio_ctx(A) == 0
    a = np.ascontiguousarray(pcm, np.float32)
    assert L.whisper_pcm_to_mel_with_state(ctx.ptr, st.ptr, fptr(a), len(a), 1) == 0
    assert L.whisper_encode_with_state(ctx.ptr, st.ptr, 0, 1) == 0
    n = A if A > 0 else 1500
    out = np.empty((n, 384), np.float32)
    assert L.whisper_mi355x_get_encoder_out(st.ptr, fptr(out), out.size) == 0
    if n > 1:  # the output is n rows: a buffer one row short is refused
        assert L.whisper_mi355x_get_encoder_out(st.ptr, fptr(out), out.size - 384) == -1
    return out


def check_encoder(out, A):
    ref = encoder_ref(A)
    assert ref.shape == out.shape == (A, 384)
    err = np.abs(out - ref)
    print(f"A {A}: encoder max abs {err.max():.3e}, mean abs {err.mean():.3e}")
    assert err.max() < 2e-2, err.max()
    assert err.mean() < 2e-3, err.mean()


@pytest.mark.parametrize("A", [750, 256, 100, 37, 1])
def test_encoder_matches_truncated_oracle(wrs, A):
    """A = 256: one full query block; 100, 37: a partial query block and a partial last K/V tile; 1: one position."""
    ctx = get_ctx(wrs, "tiny")
    st = ctx.create_state()
    out = gpu_encode(wrs, ctx, st, A, pcm_of(0))
    st.close()
    check_encoder(out, A)


def test_encoder_after_a_full_context_encode(wrs):
    """The same state encodes at the full context first: stale rows of the conv images must not reach A = 37."""
    ctx = get_ctx(wrs, "tiny")
    st = ctx.create_state()
    gpu_encode(wrs, ctx, st, 0, pcm_of(1))
    out = gpu_encode(wrs, ctx, st, 37, pcm_of(0))
    st.close()
    check_encoder(out, 37)


# ---- 2. prefill logits ----------------------------------------------------------------------------------------------
def test_prefill_logits_match_truncated_oracle(wrs, monkeypatch):
    monkeypatch.setenv("WHISPER_MI355X_CROSS", "cache")
    A = 100
    L = wrs.lib()
    ctx = get_ctx(wrs, "tiny")
    st = ctx.create_state()
    gpu_encode(wrs, ctx, st, A, pcm_of(0))
    sot = L.whisper_token_sot(ctx.ptr)
    toks = [sot, sot + 1, L.whisper_token_transcribe(ctx.ptr), L.whisper_token_beg(ctx.ptr), 400, 1000, 77]
    arr = (C.c_int * len(toks))(*toks)
    assert L.whisper_decode_with_state(ctx.ptr, st.ptr, arr, len(toks), 0, 1) == 0
    V = L.whisper_n_vocab(ctx.ptr)
    g = np.ctypeslib.as_array(L.whisper_get_logits_from_state(st.ptr), shape=(len(toks) * V,)).reshape(len(toks), V)[-1].copy()
    st.close()
    o = Oracle(truncated_model(model_path("tiny"), A), mode=1)
    o.mel(pcm_of(0))
    o.encode(0)
    o.kv_clear()
    ref = o.decode(toks, 0)[-1]
    o.close()
    diff = np.abs(g - ref).max()
    print(f"prefill logits at A {A}: max abs {diff:.3e} (max |ref| {np.abs(ref).max():.2f})")
    assert diff < 1e-2 * max(1.0, np.abs(ref).max() / 5), diff
    assert int(np.argmax(g)) == int(np.argmax(ref))


# ---- 3. whisper_full: integer outputs exact -----------------------------------------------------------------------
# (shape, A, clip): the oracle decides every kept token of these by more than F16_GAP (asserted below)
ROWS = [("tiny.en+conf", 512, 2), ("tiny.en+conf", 512, 3), ("tiny.en+conf", 100, 0), ("tiny.en+conf", 100, 1),
        ("base+conf", 750, 2), ("base+conf", 512, 1), ("base+conf", 100, 2),
        ("small-4L+conf", 512, 0), ("small-4L+conf", 512, 2), ("small-4L+conf", 512, 3), ("small-4L+conf", 100, 1),
        ("small-4L+conf", 37, 3),
        ("large-v3-2L+conf", 750, 0), ("large-v3-2L+conf", 100, 2), ("large-v3-2L+conf", 100, 3),
        ("large-v3-2L+conf", 37, 0), ("large-v3-2L+conf", 37, 1), ("large-v3-2L+conf", 37, 2), ("large-v3-2L+conf", 37, 3)]
ROWS_WIDE = [r for r in ROWS if r[0] in ("base+conf", "large-v3-2L+conf")]


def run_exact(wrs, monkeypatch, shape, A, clip, cross, pdec):
    ref = oracle_full_at(shape, A, clip)
    exp, margins = kept_token_margins(ref)
    print(f"{shape} A {A} clip {clip}: oracle {len(exp)} kept tokens, smallest margin {min(margins):.3f}")
    assert min(margins) > F16_GAP, "the fixture changed: this clip is no exact case any more"
    monkeypatch.setenv("WHISPER_MI355X_CROSS", cross)
    if not pdec:
        monkeypatch.setenv("WHISPER_MI355X_PDEC", "0")
    ctx = get_ctx(wrs, shape)
    st = ctx.create_state()
    wrs.lib().whisper_mi355x_kernel_timing(st.ptr, 1 << K_PDEC)
    assert st.full(params(wrs, A), pcm_of(clip)) == 0
    n, gave_up = pdec_launches(wrs, st), st.pdec_give_ups()
    segs, dec, direct = st.segments(), st.decisions(), st.info()["direct"]
    st.close()
    assert direct == (cross == "direct")
    if pdec and cross == "cache":
        assert n > 0, "the persistent decode step did not run"
    else:
        assert n == 0
    assert gave_up == 0
    assert ints(segs) == ref_ints(ref)
    assert [s.text for s in segs] == [s["text"] for s in ref["segments"]]
    assert [tuple(d[k] for k in DEC_KEYS) for d in dec] == [tuple(d[k] for k in DEC_KEYS) for d in ref["decisions"]]


@pytest.mark.parametrize("shape,A,clip", ROWS)
def test_full_exact_persistent_step(wrs, monkeypatch, shape, A, clip):
    run_exact(wrs, monkeypatch, shape, A, clip, "cache", True)


@pytest.mark.parametrize("shape,A,clip", ROWS_WIDE)
def test_full_exact_small_m_chain(wrs, monkeypatch, shape, A, clip):
    run_exact(wrs, monkeypatch, shape, A, clip, "cache", False)


@pytest.mark.parametrize("shape,A,clip", ROWS_WIDE)
def test_full_exact_direct_form(wrs, monkeypatch, shape, A, clip):
    run_exact(wrs, monkeypatch, shape, A, clip, "direct", True)


# ---- 4. the split-K chain (more than 4 clips) -----------------------------------------------------------------------
def check_clip_by_rule(segs, dec, ref, what):
    """the rule of test_gpu_pdec.py::test_pdec_full_f16_exact; returns whether the clip was an exact case"""
    exp, margins = kept_token_margins(ref)
    if min(margins) > F16_GAP:
        assert ints(segs) == ref_ints(ref), what
        assert [s.text for s in segs] == [s["text"] for s in ref["segments"]], what
        assert [tuple(d[k] for k in DEC_KEYS) for d in dec] == [tuple(d[k] for k in DEC_KEYS) for d in ref["decisions"]], what
        return True
    got = [t for sg in ints(segs) for t in sg[0]]
    k = assert_diverges_only_at_close_calls(got, exp, margins, F16_GAP, 4)
    assert_closed_before_divergence(segs, dec, ref, k)
    print(f"{what}: {k} of {len(exp)} tokens identical (oracle near tie {min(margins):.4f} nats)")
    return False


@pytest.mark.parametrize("A,cross,clips,min_exact", [(100, "cache", (2, 3, 1, 2, 3, 1), 2), (37, "direct", (0, 1, 2, 3, 0, 1), 3)])
def test_batch_of_six_split_k_chain(wrs, monkeypatch, A, cross, clips, min_exact):
    shape = "large-v3-2L+conf"
    monkeypatch.setenv("WHISPER_MI355X_CROSS", cross)
    ctx = get_ctx(wrs, shape)
    st = ctx.create_state()
    assert st.full_batch(params(wrs, A), [pcm_of(c) for c in clips]) == 0
    exact = set()
    for j, c in enumerate(clips):
        if check_clip_by_rule(st.batch_segments(j), st.decisions(j), oracle_full_at(shape, A, c), f"A {A} job {j} clip {c}"):
            exact.add(c)
    assert st.info()["direct"] == (cross == "direct")
    st.close()
    assert len(exact) >= min_exact, exact


# ---- 5. identity and errors -------------------------------------------------------------------------------------------
def test_model_context_and_non_positive_values_change_nothing(wrs):
    ctx = get_ctx(wrs, "tiny.en+conf")
    out = []
    for A in (0, 1500, -3):
        st = ctx.create_state()
        assert st.full(params(wrs, A, t_inc=0.2), pcm_of(2)) == 0
        out.append(bits(st))
        st.close()
    assert out[0][0] and out[0][1]
    assert out[1] == out[0]
    assert out[2] == out[0]


def test_too_large_is_minus_5(wrs, capfd):
    ctx = get_ctx(wrs, "tiny.en+conf")
    st = ctx.create_state()
    assert st.full(params(wrs, 1501), pcm_of(2)) == -5
    assert "audio_ctx" in capfd.readouterr().err
    assert st.full_batch(params(wrs, 1501), [pcm_of(2), pcm_of(3)]) == -5
    assert st.full_batch(params(wrs, 1501), [pcm_of(k % 4) for k in range(10)]) == -5
    assert st.set_audio_ctx(1501) == -5
    assert st.set_audio_ctx(1500) == 0 and st.set_audio_ctx(0) == 0
    assert wrs.lib().whisper_mi355x_set_audio_ctx(None, 100) == -1
    assert st.full(params(wrs, 512), pcm_of(2)) == 0
    after = bits(st)
    st.close()
    st = ctx.create_state()
    assert st.full(params(wrs, 512), pcm_of(2)) == 0
    assert bits(st) == after and after[0]
    st.close()


# ---- 6. no stale state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", ["cache", "direct"])
def test_one_state_full_short_full(wrs, monkeypatch, cross):
    """cache rows >= A of the slot hold the first call's keys, its decode graphs its split counts, its conv images
    its frames: the A = 100 call must see none of them, and the third call none of the second's."""
    monkeypatch.setenv("WHISPER_MI355X_CROSS", cross)
    ctx = get_ctx(wrs, "base+conf")
    st = ctx.create_state()
    runs = []

    def call(st, A):  # no_context: a state's earlier text is no prompt of its next call (the calls compare bit for bit)
        p = params(wrs, A)
        p.no_context = True
        assert st.full(p, pcm_of(2)) == 0
        return bits(st)
    for A in (0, 100, 0):
        runs.append(call(st, A))
    st.close()
    st = ctx.create_state()
    fresh = call(st, 100)
    st.close()
    assert fresh[0] and runs[1] == fresh
    assert runs[2] == runs[0]
    assert runs[1][1] != runs[0][1]


# ---- 7. auto language ---------------------------------------------------------------------------------------------------
def test_auto_language(wrs):
    """whisper_full detects the language before it stores audio_ctx: at the full context on a fresh state, and
    window 0 is then encoded again at A."""
    L = wrs.lib()
    ctx = get_ctx(wrs, "tiny+conf")
    A = 100
    st = ctx.create_state()
    assert st.full(params(wrs, 0, lang=None), pcm_of(1)) == 0
    lang_full = L.whisper_full_lang_id_from_state(st.ptr)
    st.close()
    st = ctx.create_state()
    assert st.full(params(wrs, A, lang=None), pcm_of(1)) == 0
    lang_a, auto = L.whisper_full_lang_id_from_state(st.ptr), bits(st)
    st.close()
    assert lang_a == lang_full
    st = ctx.create_state()
    assert st.full(params(wrs, A, lang=L.whisper_lang_str(lang_a).decode()), pcm_of(1)) == 0
    explicit = bits(st)
    st.close()
    assert auto[0] and auto == explicit
    # the batch API detects at the full context too (every clip as on a fresh state), also on a state that just ran at A
    st = ctx.create_state()
    assert st.full_batch(params(wrs, A, lang=None), [pcm_of(1), pcm_of(2)]) == 0
    assert st.full_batch(params(wrs, A, lang=None), [pcm_of(1), pcm_of(2)]) == 0
    assert L.whisper_mi355x_batch_lang_id(st.ptr, 0) == lang_full
    assert bits(st, 0) == explicit
    st.close()
    # the low-level call works at the state's value: the truncated oracle's detection
    st = ctx.create_state()
    a = np.ascontiguousarray(pcm_of(1), np.float32)
    assert st.set_audio_ctx(A) == 0
    assert L.whisper_pcm_to_mel_with_state(ctx.ptr, st.ptr, fptr(a), len(a), 1) == 0
    got = L.whisper_lang_auto_detect_with_state(ctx.ptr, st.ptr, 0, 1, None)
    st.close()
    o = Oracle(truncated_model(model_path("tiny+conf"), A), mode=1)
    o.mel(a)
    want = o.L.oracle_lang_detect(o.m, o.s)
    o.close()
    assert got == want


# ---- 8. batch equals single -----------------------------------------------------------------------------------------
def test_batch_equals_single(wrs):
    ctx = get_ctx(wrs, "base+conf")
    clips = [pcm_of(0), pcm_of(1, 12.0), pcm_of(2)]
    p = params(wrs, 512)
    single = []
    for c in clips:
        st = ctx.create_state()
        assert st.full(p, c) == 0
        single.append(bits(st))
        st.close()
    st = ctx.create_state()
    assert st.full_batch(p, clips) == 0
    batch = [bits(st, j) for j in range(3)]
    st.close()
    assert all(s[0] for s in single) and batch == single


# ---- 9. the other strategies, one case each at A = 100 ------------------------------------------------------------------
def test_beam_1_is_greedy(wrs):
    ctx = get_ctx(wrs, "tiny+conf")
    out = []
    for p in (wrs.reference_full_params("en"), wrs.beam_full_params(1, "en")):
        p.audio_ctx = 100
        st = ctx.create_state()
        assert st.full(p, pcm_of(2)) == 0
        out.append(bits(st))
        st.close()
    assert out[0][0] and out[1] == out[0]


def test_beam_3(wrs):
    """The harness of tests/test_gpu_beam.py at audio_ctx = 100: tests/beam_ref.py over the engine's own teacher-forced
    logits (of calls with the same audio_ctx); the step-0 logits of that harness are checked against the truncated
    oracle's, so the reference search runs over logits of the shortened context."""
    import beam_ref as br
    from test_gpu_beam import MIN_GAP, SPACE, EngineLogits, beam_params, check_job
    A, K, clip = 100, 3, 24
    ctx = get_ctx(wrs, "tiny+conf")
    pcm = pcm_of(clip)
    src = EngineLogits(wrs, ctx, pcm, K, False, 12)
    src.p.audio_ctx = A
    vid = br.vocab_ids(src.V, SPACE)
    n_org = 1 + (len(pcm) + 200 - 400) // 160
    ref = br.beam_search(src, br.Params(K=K, max_tokens=12, single_segment=True, no_timestamps=False, seek_end=n_org), vid,
                         n_prompt=3)
    first = src(())
    src.close()
    o = Oracle(truncated_model(model_path("tiny+conf"), A), mode=1)
    o.mel(pcm)
    o.encode(0)
    o.kv_clear()
    sot = o.token("sot")
    want = o.decode([sot, sot + 1, o.token("transcribe")], 0)[-1]
    o.close()
    assert np.abs(first - want).max() < 1e-2 * max(1.0, np.abs(want).max() / 5)
    print(f"beam 3 at A {A}: min gap {ref.min_gap():.4f}, winner {ref.winner}")
    assert ref.min_gap() > MIN_GAP
    p = beam_params(wrs, K)
    p.audio_ctx = A
    st = ctx.create_state()
    assert st.full(p, pcm) == 0
    check_job(st, 0, ref, st.segments())
    st.close()


def failing_clip(shape, A):
    """the first clip whose t = 0 attempt fails in the oracle at audio_ctx = A"""
    for clip in range(8):
        d = oracle_full_at(shape, A, clip)["decisions"]
        if d and d[0]["failed0"]:
            return clip, d[0]
    raise AssertionError(f"no clip of 0..7 fails at t = 0 on {shape} at audio_ctx {A}")


def test_best_of_3(wrs):
    A, shape = 100, "base+conf"  # (clip 1: the oracle's greedy attempt fails the entropy rule at this context)
    clip, d0 = failing_clip(shape, A)
    ctx = get_ctx(wrs, shape)
    runs = []
    for _ in range(2):
        st = ctx.create_state()
        st.set_sample_seed(7)
        p = params(wrs, A, t_inc=0.2)
        p.greedy.best_of = 3
        assert st.full(p, pcm_of(clip)) == 0
        runs.append((bits(st), st.cand_info(0)))
        st.close()
    dec = runs[0][0][2]
    # the t = 0 attempt of the first window is the oracle's (the sampled attempts that follow draw on the device)
    # (its length only where the oracle decided every step of it by more than F16_GAP)
    t0_keys = ("seek", "failed0", "logprob_fail0")
    if min(float(m) for m in oracle_full_at(shape, A, clip)["margins"]) > F16_GAP:
        t0_keys += ("result_len0",)
    assert tuple(dec[0][k] for k in t0_keys) == tuple(d0[k] for k in t0_keys)
    assert dec[0]["temp_idx"] >= 1 and len(runs[0][1]) == 3
    assert runs[1] == runs[0]


def test_dtw(wrs):
    from test_gpu_dtw import FIG, TINY_HEADS, check_job
    A, shape = 100, "tiny+conf"
    ctx = get_ctx(wrs, shape, dtw_preset="TINY")
    st = ctx.create_state()
    pcm = pcm_of(0)
    assert st.full(params(wrs, A, t_inc=0.2), pcm) == 0
    assert st.align_ms() > 0
    N, F = check_job(wrs, st, 0, truncated_model(model_path(shape), A), ("clip", 0, 30.0), pcm, TINY_HEADS, "f16", FIG)
    st.close()
    n_frames = 1 + (len(pcm) + 200 - 400) // 160
    assert F == min(n_frames // 2, A)


def test_quantized_file(wrs, monkeypatch):
    shape, A = "large-v3-2L+conf+q5_0", 100
    monkeypatch.setenv("WHISPER_MI355X_CROSS", "cache")
    best, conf = None, -1
    for clip in range(4):
        _, margins = kept_token_margins(oracle_full_at(shape, A, clip))
        n = sum(1 for m in margins if m > F16_GAP)
        if n > conf:
            best, conf = clip, n
    assert conf >= 4, conf
    ctx = get_ctx(wrs, shape)
    st = ctx.create_state()
    wrs.lib().whisper_mi355x_kernel_timing(st.ptr, 1 << K_PDEC)
    assert st.full(params(wrs, A), pcm_of(best)) == 0
    assert pdec_launches(wrs, st) > 0
    check_clip_by_rule(st.segments(), st.decisions(), oracle_full_at(shape, A, best), f"{shape} A {A} clip {best}")
    st.close()
