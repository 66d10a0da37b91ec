"""Sampled fallback attempts with greedy.best_of candidates drawn on the device, through
whisper_full_with_state / whisper_mi355x_full_batch.

Setup: tiny+conf, the reference's FullParams with greedy.best_of = N, temperature_inc = 0.6 (attempts at t = 0 and 0.6,
temp_idx 1), logprob_thold = 0 (every attempt falls through, the t = 0.6 winner is kept), no_speech_thold = 1,
single_segment, max_tokens = 12.

Exact runs: the reference is tests/sample_ref.py over the engine's own raw logits (EngineLogits of tests/test_gpu_beam.py:
teacher-forced calls on the split-K launch chain in the cache form, as a sampled step runs). Every candidate's tokens and
flags, the winner and the segments must equal the reference; sum_logprobs_all within 2.8e-5 x length (DESIGN.md §11's
measured bar for the probs / logprobs rows at t > 0, 4 x 6.86e-6). A logprob error d moves a CDF boundary by at most d x S,
so the reference's smallest draw margin must be at least 1.12e-4 (4 x the bar) and the winner's score must lead every
candidate with other tokens by 1e-3 (beam search's MIN_GAP), else the test fails.

Clips: synthetic_pcm 5 and 9 (tools/bestof_pick_clips.py over the oracle's logits, seed 0, N = 5: min margin 2.95e-4,
score gaps 0.06 and 0.08; clip 9 has a candidate that ends two tokens early). Clip 7 has the same margin but its two best
candidates score within 3e-4 of each other (9e-4 over the engine's f16 logits), so it is only used where no winner is
compared with the reference (the batch test).
"""
import numpy as np
import pytest

import beam_ref as br
import sample_ref as sr
from conftest import model_path
from make_model import synthetic_pcm
from test_gpu_beam import SPACE, EngineLogits

pytestmark = pytest.mark.gpu

CLIPS = (5, 9)
T_INC = 0.6
PLOG_BAR = 2.8e-5      # per token (4 x 6.86e-6)
MIN_MARGIN = 1.12e-4   # 4 x PLOG_BAR
MIN_GAP = 1e-3
CLIP_T0 = 0            # decided at t = 0 with the app's thresholds (the smoke test's clip)
CLIPS_T0 = (0, 2, 3, 4)

_CTX = {}


def get_ctx(wrs, dtype, **kw):
    key = (dtype, tuple(sorted(kw.items())))
    if key not in _CTX:
        _CTX[key] = wrs.WhisperContext(model_path("tiny+conf"), dtype=getattr(wrs, dtype), **kw)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_ctxs():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def fallback(p, N):
    p.greedy.best_of = N
    p.temperature_inc = T_INC
    p.logprob_thold = 0.0
    p.no_speech_thold = 1.0
    p.single_segment = True
    p.max_tokens = 12
    return p


def bo_params(wrs, N):
    return fallback(wrs.reference_full_params("en"), N)


def segs_of(segs):
    return [(s.t0, s.t1, s.text, s.tokens) for s in segs]


_REF = {}


def reference(wrs, ctx, dtype, clip, N, seed=0):
    k = (dtype, clip, N, seed)
    if k not in _REF:
        pcm = synthetic_pcm(clip)
        src = EngineLogits(wrs, ctx, pcm, N, False, 12)
        vid = br.vocab_ids(src.V, SPACE)
        n_org = 1 + (len(pcm) + 200 - 400) // 160
        P = br.Params(K=1, max_tokens=12, single_segment=True, seek_end=n_org, logprob_thold=0.0)
        _REF[k] = sr.sample_candidates(src, P, vid, N, np.float32(T_INC), seed=seed, temp_idx=1)
        src.close()
    return _REF[k]


def check_job(st, job, ref, segs):
    info = st.cand_info(job)
    assert len(info) == len(ref.cands)
    for b, (got, want) in enumerate(zip(info, ref.cands)):
        assert got["tokens"] == want["tokens"], f"candidate {b}"
        assert (got["completed"], got["failed"], got["winner"]) == (want["completed"], want["failed"], want["winner"]), f"candidate {b}"
        tol = PLOG_BAR * max(1, len(want["tokens"]))
        assert abs(got["sum_logprobs_all"] - want["sum_logprobs_all"]) <= tol, (b, got["sum_logprobs_all"], want["sum_logprobs_all"])
    assert ref.winner >= 0
    assert len(segs) == 1 and [t[0] for t in segs[0].tokens] == ref.tokens
    d = st.decisions(job)
    assert [x["temp_idx"] for x in d] == [1]


def check_ref(ref, what):
    print(f"{what}: min margin {ref.min_margin():.3e} over {len(ref.margins)} draws, score gap {ref.score_gap:.4f}, "
          f"winner {ref.winner}, distinct {len({tuple(c['tokens']) for c in ref.cands})}")
    assert ref.min_margin() >= MIN_MARGIN, sorted(ref.margins)[:3]
    assert ref.score_gap >= MIN_GAP, ref.score_gap


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
@pytest.mark.parametrize("clip", CLIPS)
def test_best_of_5_exact(wrs, dtype, clip):
    ctx = get_ctx(wrs, dtype)
    ref = reference(wrs, ctx, dtype, clip, 5)
    check_ref(ref, f"clip {clip} {dtype}")
    st = ctx.create_state()
    assert st.full(bo_params(wrs, 5), synthetic_pcm(clip)) == 0
    check_job(st, 0, ref, st.segments())
    st.close()


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_best_of_3_batch_equals_single(wrs, dtype):
    """Clips (7, 5) as one batch: the candidates, sums and segments of the two single-clip runs, bit for bit."""
    ctx = get_ctx(wrs, dtype)
    clips = (7, 5)
    st = ctx.create_state()
    assert st.full_batch(bo_params(wrs, 3), [synthetic_pcm(c) for c in clips]) == 0
    batch = [(st.cand_info(j), segs_of(st.batch_segments(j))) for j in range(2)]
    st.close()
    for j, clip in enumerate(clips):
        st = ctx.create_state()
        assert st.full(bo_params(wrs, 3), synthetic_pcm(clip)) == 0
        single = (st.cand_info(0), segs_of(st.segments()))
        st.close()
        assert len(single[0]) == 3 and sum(c["winner"] for c in single[0]) == 1 and single[1]
        assert single == batch[j], clip


def test_t0_untouched_one_clip(wrs):
    """The app's thresholds on a clip decided at t = 0: best_of = 5 gives best_of = 1's bits (one clip: the persistent
    step), and there are no candidates to report."""
    ctx = get_ctx(wrs, "F16")
    out = []
    for N in (1, 5):
        p = wrs.reference_full_params("en")
        p.greedy.best_of = N
        st = ctx.create_state()
        assert st.full(p, synthetic_pcm(CLIP_T0)) == 0
        out.append((segs_of(st.segments()), st.decisions(), st.token_times()))
        assert st.cand_info(0) == []
        assert wrs.lib().whisper_mi355x_cand_info(st.ptr, 0, 0, None, 0, None, None) == -1
        st.close()
    assert out[0][0] and all(d["temp_idx"] == 0 for d in out[0][1])
    assert out[1] == out[0]


def test_t0_untouched_batch(wrs):
    ctx = get_ctx(wrs, "F16")
    pcm = [synthetic_pcm(c) for c in CLIPS_T0]
    out = []
    for N in (1, 5):
        p = wrs.reference_full_params("en")
        p.greedy.best_of = N
        st = ctx.create_state()
        assert st.full_batch(p, pcm) == 0
        out.append([(segs_of(st.batch_segments(j)), st.decisions(j)) for j in range(len(pcm))])
        for j in range(len(pcm)):
            assert wrs.lib().whisper_mi355x_cand_info(st.ptr, j, 0, None, 0, None, None) == -1
        st.close()
    assert all(job[0] and all(d["temp_idx"] == 0 for d in job[1]) for job in out[0])
    assert out[1] == out[0]


def _run5(wrs, ctx, clip, seed=None, N=5):
    st = ctx.create_state()
    if seed is not None:
        st.set_sample_seed(seed)
    assert st.full(bo_params(wrs, N), synthetic_pcm(clip)) == 0
    out = (st.cand_info(0), segs_of(st.segments()), st.decisions())
    st.close()
    return out


def test_seed(wrs):
    ctx = get_ctx(wrs, "F16")
    a, b = _run5(wrs, ctx, 5), _run5(wrs, ctx, 5, seed=0)
    assert len(a[0]) == 5 and a == b
    c, d = _run5(wrs, ctx, 5, seed=1), _run5(wrs, ctx, 5, seed=1)
    assert c == d
    assert [x["tokens"] for x in c[0]] != [x["tokens"] for x in a[0]]
    big = _run5(wrs, ctx, 5, seed=0x0123456789abcdef)   # both halves of the seed are key words
    assert [x["tokens"] for x in big[0]] != [x["tokens"] for x in _run5(wrs, ctx, 5, seed=0x89abcdef)[0]]


def test_recycled_state(wrs):
    """A state recycled after a best_of call is a fresh one: the seed is 0 again, and a following best_of = 1 call
    samples on the host as on a fresh context."""
    shared = get_ctx(wrs, "F16")
    want5 = _run5(wrs, shared, 5)
    fresh = wrs.WhisperContext(model_path("tiny+conf"), dtype=wrs.F16)
    want1 = _run5(wrs, fresh, 5, N=1)
    fresh.close()
    assert want1[0] == [] and want1[1]
    ctx = wrs.WhisperContext(model_path("tiny+conf"), dtype=wrs.F16)
    first = _run5(wrs, ctx, 5, seed=1)
    assert first[0] != want5[0]
    st = ctx.create_state()
    assert st.info()["pooled"] and st.cand_info(0) == []
    st.close()
    assert _run5(wrs, ctx, 5) == want5
    assert _run5(wrs, ctx, 5, N=1) == want1
    ctx.close()


def test_best_of_9_is_refused(wrs):
    ctx = get_ctx(wrs, "F16")
    st = ctx.create_state()
    assert st.full(bo_params(wrs, 9), synthetic_pcm(5)) == -4
    assert st.full(bo_params(wrs, 5), synthetic_pcm(5)) == 0
    assert len(st.cand_info(0)) == 5
    st.close()


def test_row_limit_falls_back_to_one_host_candidate(wrs, capfd):
    """7 clips x best_of 5 exceed the 32 decoder rows: one host-sampled candidate per clip, exactly best_of = 1's
    results, no candidates to report, and one stderr line per process."""
    ctx = get_ctx(wrs, "F16")
    pcm = [synthetic_pcm(c) for c in range(7)]
    out = []
    capfd.readouterr()
    for N in (5, 1, 5):
        st = ctx.create_state()
        assert st.full_batch(bo_params(wrs, N), pcm) == 0
        out.append([(segs_of(st.batch_segments(j)), st.decisions(j)) for j in range(7)])
        for j in range(7):
            assert wrs.lib().whisper_mi355x_cand_info(st.ptr, j, 0, None, 0, None, None) == -1
        st.close()
    err = capfd.readouterr().err
    assert err.count("decoder rows per step: fallback attempts sample 1 candidate") == 1, err
    assert all(job[1] and job[1][0]["temp_idx"] == 1 for job in out[1])
    assert out[0] == out[1] and out[2] == out[1]


def test_beam_strategy_samples_best_of_candidates(wrs):
    """Beam search whose t = 0 attempt falls through: the t > 0 attempt decodes greedy.best_of candidates."""
    ctx = get_ctx(wrs, "F16")
    p = fallback(wrs.beam_full_params(3, "en"), 3)
    st = ctx.create_state()
    assert st.full(p, synthetic_pcm(5)) == 0
    beams, cands = st.beam_info(0), st.cand_info(0)
    assert len(beams) == 3 and len(cands) == 3
    assert sum(c["winner"] for c in cands) == 1
    assert [d["temp_idx"] for d in st.decisions()] == [1]
    win = next(c for c in cands if c["winner"])
    segs = st.segments()
    assert len(segs) == 1 and [t[0] for t in segs[0].tokens] == win["tokens"][:len(segs[0].tokens)]
    st.close()
    # the default of the beam strategy (best_of = -1) is one host-sampled decoder
    p = fallback(wrs.beam_full_params(3, "en"), -1)
    st = ctx.create_state()
    assert st.full(p, synthetic_pcm(5)) == 0
    assert st.cand_info(0) == [] and len(st.beam_info(0)) == 3
    st.close()


def test_direct_cross_form(wrs, monkeypatch):
    """WHISPER_MI355X_CROSS=direct: the call keeps the direct form (t = 0 attempt, prefills), the sampled steps run in
    the cache form over cross K/V computed on demand. The prefill's logits differ in the last bits between the forms, so
    the candidates' tokens (margins 2.95e-4) are the cache-form run's and the sums agree to the forms' difference
    (5e-2, as test_gpu_beam.py::test_six_clips_five_beams allows between kernel forms)."""
    ctx = get_ctx(wrs, "F16")
    want = _run5(wrs, ctx, 5, N=3)
    monkeypatch.setenv("WHISPER_MI355X_CROSS", "direct")
    st = ctx.create_state()
    assert st.full_batch(bo_params(wrs, 3), [synthetic_pcm(5), synthetic_pcm(9)]) == 0
    assert st.info()["direct"]
    got = st.cand_info(0)
    assert len(got) == 3 and len(st.cand_info(1)) == 3 and sum(c["winner"] for c in got) == 1
    for g, w_ in zip(got, want[0]):
        assert {k: v for k, v in g.items() if k != "sum_logprobs_all"} == {k: v for k, v in w_.items() if k != "sum_logprobs_all"}
        assert g["sum_logprobs_all"] == pytest.approx(w_["sum_logprobs_all"], abs=5e-2)
    assert [t[0] for t in st.batch_segments(0)[0].tokens] == [t[0] for t in want[1][0][3]]
    st.close()


def test_dtw_on_the_winner(wrs):
    ctx = get_ctx(wrs, "F16", dtw_n_top=2)
    st = ctx.create_state()
    assert st.full(bo_params(wrs, 5), synthetic_pcm(5)) == 0
    cands = st.cand_info(0)
    win = next(c for c in cands if c["winner"])
    segs, times = st.segments(), st.token_times()
    assert len(segs) == 1 and [t[0] for t in segs[0].tokens] == win["tokens"][:len(segs[0].tokens)]
    assert any(t >= 0 for seg in times for _, t in seg)
    st.close()
    plain = _run5(wrs, get_ctx(wrs, "F16"), 5)
    assert [c["tokens"] for c in cands] == [c["tokens"] for c in plain[0]]


def _mixed_params(wrs, logprob_thold):
    p = fallback(wrs.beam_full_params(2, "en"), 2)
    p.logprob_thold = logprob_thold
    return p


def _mixed_out(st, job, single):
    segs = st.segments() if single else st.batch_segments(job)
    return dict(segments=segs_of(segs), decisions=st.decisions(job), beam_info=st.beam_info(job), cand_info=st.cand_info(job))


def test_beam_and_sampled_steps_in_one_pass(wrs):
    """Beam steps and sampled steps of different clips in the same scheduler passes, over the same host staging rows.
    Three 40 s clips (two windows each) in one batch, BeamSearch{beam_size: 2} with best_of = 2 and temperature_inc = 0.6.
    A first run without fallback (logprob_thold = -1e9) gives every clip's avg_logprob0 of window 0; logprob_thold is then
    the midpoint of the widest gap between two of them, so at least one clip falls back at window 0 (its two sampled
    candidates decode) while another goes on to the beam attempt of its window 1 in the same passes. Every clip's segments
    (token ids, tid, p, plog), decisions, beam_info and cand_info in the batch must equal that clip run alone."""
    ctx = get_ctx(wrs, "F16")
    pcm = [synthetic_pcm(c, seconds=40.0) for c in (5, 7, 9)]
    st = ctx.create_state()
    assert st.full_batch(_mixed_params(wrs, -1e9), pcm) == 0
    first = [st.decisions(j) for j in range(3)]
    st.close()
    assert all(len(d) == 2 and all(w["temp_idx"] == 0 for w in d) for d in first), first
    lp = sorted(d[0]["avg_logprob0"] for d in first)
    gap, lo = max((lp[i + 1] - lp[i], i) for i in range(2))
    thold = 0.5 * (lp[lo] + lp[lo + 1])
    print(f"avg_logprob0 of window 0: {lp}, logprob_thold {thold:.6f}")
    assert lp[lo] < thold < lp[lo + 1], lp
    st = ctx.create_state()
    assert st.full_batch(_mixed_params(wrs, thold), pcm) == 0
    batch = [_mixed_out(st, j, False) for j in range(3)]
    st.close()
    idx0 = [b["decisions"][0]["temp_idx"] for b in batch]
    print(f"temp_idx of window 0: {idx0}, windows {[len(b['decisions']) for b in batch]}")
    assert set(idx0) == {0, 1}, idx0   # (the precondition: a clip fell back at window 0, another did not)
    # a clip decided at t = 0 went on to a second window: its beam steps ran beside the other clip's sampled steps
    assert any(i == 0 and len(b["decisions"]) == 2 for i, b in zip(idx0, batch)), batch
    for j in range(3):
        st = ctx.create_state()
        assert st.full(_mixed_params(wrs, thold), pcm[j]) == 0
        single = _mixed_out(st, 0, True)
        st.close()
        assert single["segments"] and len(single["beam_info"]) == 2
        assert (len(single["cand_info"]) == 2) == any(d["temp_idx"] == 1 for d in single["decisions"])
        assert single == batch[j], j
