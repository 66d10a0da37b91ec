"""suppress_nst / suppress_regex end to end through whisper_full_with_state / whisper_mi355x_full_batch on
tiny+conf, f16: a pattern that matches nothing changes nothing; banned tokens appear in no decoding mode (greedy with 1, 5
and 17 clips: the persistent pipelined step, the split logits form, one workgroup per row; beam search; best_of candidates of
a forced fallback); a banned fixed-token run is exact against tests/suppress_ref.py over the engine's own raw logits
(test_gpu_beam.py's method: teacher-forced, the small-M path and the persistent step off, so a row does not depend on
its neighbours); a pattern that does not compile returns -8 and leaves the state usable; a state that ran with a ban runs
without one next; suppress_nst bans the synthetic vocabulary's 23 single-byte list tokens and " -".

The mask itself (whisper_mi355x_suppress_mask; the context needs the device, so it is tested here) equals
suppress_ref.mask over whisper_token_to_str of every id for micro.

CLIPS_EXACT: synthetic_pcm seeds for which the CPU oracle's own logits leave at most 2 of the 24 banned steps under
logits_cases.MIN_GAP (tools/suppress_pick_clips.py: clips 0..4 have 0 such steps each); the test asserts the cap over the
engine's logits.
"""
from collections import Counter

import numpy as np
import pytest

import logits_cases as lc
import logits_ref as lr
import suppress_cases as sc
import suppress_ref as sr
from conftest import model_path
from make_model import synthetic_pcm, synthetic_vocab

pytestmark = pytest.mark.gpu

SHAPE = "tiny+conf"
N_FIXED = 24
CLIPS_EXACT = (0, 1, 2, 3, 4)
MAX_UNDECIDED = 2

_CTX = {}


def get_ctx(wrs, shape=SHAPE):
    if shape not in _CTX:
        _CTX[shape] = wrs.WhisperContext(model_path(shape), dtype=wrs.F16)
    return _CTX[shape]


@pytest.fixture(scope="module", autouse=True)
def _close_ctxs():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def params(wrs, regex=None, nst=False, **kw):
    p = kw.pop("base", None) or wrs.reference_full_params("en")
    p.suppress_regex = None if regex is None else regex.encode()
    p.suppress_nst = nst
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def seg_rows(segs):
    return [(s.t0, s.t1, s.text, s.tokens) for s in segs]


def run_single(ctx, p, clip):
    st = ctx.create_state()
    assert st.full(p, synthetic_pcm(clip)) == 0
    out = seg_rows(st.segments()), st.decisions()
    st.close()
    return out


def run_batch(ctx, p, clips, fixed=0):
    st = ctx.create_state()
    assert st.full_batch(p, [synthetic_pcm(c) for c in clips], fixed_tokens=fixed) == 0
    out = [(seg_rows(st.batch_segments(j)), st.decisions(j)) for j in range(len(clips))]
    st.close()
    return out


def ids_of(result):
    return [t[0] for seg in result[0] for t in seg[3]]


def escaped(tok: bytes) -> str:
    return "".join(chr(b) if chr(b).isalnum() and b < 128 else f"\\x{b:02x}" for b in tok)


def ban_of(ctx, runs, eot, n=8):
    """The n most frequent text tokens of the runs (ties: the lower id) and the alternation that bans exactly them."""
    cnt = Counter(i for r in runs for i in ids_of(r) if i < eot)
    ids = [i for i, _ in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))[:n]]
    assert len(ids) == n
    regex = "|".join(escaped(ctx.token_str(i)) for i in ids)
    m = ctx.suppress_mask(False, regex)
    assert np.nonzero(m)[0].tolist() == sorted(ids), "the alternation bans exactly the chosen tokens"
    return ids, regex


_PLAIN = {}


def plain17(wrs):
    if "p" not in _PLAIN:
        _PLAIN["p"] = run_batch(get_ctx(wrs), params(wrs), range(17))
    return _PLAIN["p"]


# ---- the mask through the C interface ---------------------------------------------------------------------------------
def test_mask_matches_reference(wrs):
    ctx = get_ctx(wrs, "micro")
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    toks = [ctx.token_str(i) for i in range(V)]
    file_toks = synthetic_vocab()  # (a C string ends at a NUL: token 0 is the byte 0)
    assert toks[:len(file_toks)] == [t.split(b"\0")[0] for t in file_toks]
    toks[:len(file_toks)] = file_toks
    assert len(set(toks)) == V
    for nst, rx in ((True, None), (False, "[0-9]+"), (False, r"\[_TT_.*\]"), (True, " ?[A-Z][a-z]*"), (False, ""), (False, ".*")):
        got = ctx.suppress_mask(nst, rx)
        want = sr.mask(toks, nst, rx)
        assert (got == want).all(), (nst, rx, np.nonzero(got != want)[0][:8])
    assert int(ctx.suppress_mask(True, None).sum()) == 24
    assert int(ctx.suppress_mask(False, r"\[_TT_.*\]").sum()) == 1500
    assert ctx.suppress_mask(False, "(") == -8
    assert ctx.suppress_mask(True, "(") == -8
    # the cache: the same key builds nothing, another key builds once
    n0 = L.whisper_mi355x_suppress_builds(ctx.ptr)
    for _ in range(3):
        ctx.suppress_mask(True, "[0-9]+")
    assert L.whisper_mi355x_suppress_builds(ctx.ptr) == n0 + 1
    ctx.suppress_mask(False, "[0-9]+")
    assert L.whisper_mi355x_suppress_builds(ctx.ptr) == n0 + 2
    import ctypes as C
    w = np.zeros(4, np.uint32)
    assert L.whisper_mi355x_suppress_mask(ctx.ptr, True, None, w.ctypes.data_as(C.POINTER(C.c_uint32)), 4) == -1


# ---- 1. a pattern that matches nothing ------------------------------------------------------------------------------------
def test_noop_pattern(wrs):
    ctx = get_ctx(wrs)
    assert not ctx.suppress_mask(False, "(?!)").any()
    assert run_single(ctx, params(wrs, "(?!)"), 0) == run_single(ctx, params(wrs), 0)
    clips = range(5)
    got = run_batch(ctx, params(wrs, "(?!)"), clips)
    assert got == run_batch(ctx, params(wrs), clips)
    assert all(r[0] for r in got)


# ---- 2. the mask bites ------------------------------------------------------------------------------------------------------
def test_banned_tokens_never_appear(wrs):
    ctx = get_ctx(wrs)
    eot = wrs.lib().whisper_token_eot(ctx.ptr)
    plain = plain17(wrs)
    ids, regex = ban_of(ctx, plain, eot)
    banned = set(ids)
    print(f"banned {ids} = {[ctx.token_str(i) for i in ids]}")
    changed = 0
    one = run_single(ctx, params(wrs, regex), 0)  # 1 clip: the persistent, pipelined step
    assert ids_of(one) and not banned & set(ids_of(one))
    for n in (5, 17):  # the split logits form; one workgroup per row
        got = run_batch(ctx, params(wrs, regex), range(n))
        for j, r in enumerate(got):
            assert ids_of(r), (n, j)
            assert not banned & set(ids_of(r)), (n, j)
            changed += [s[2] for s in r[0]] != [s[2] for s in plain[j][0]]
    assert changed > 0, "no clip's text differs from the plain run"
    assert banned & set(i for r in plain for i in ids_of(r))
    # beam search
    st = ctx.create_state()
    bp = params(wrs, regex, base=wrs.beam_full_params(3, "en"), temperature_inc=0.0, single_segment=True, max_tokens=24)
    assert st.full_batch(bp, [synthetic_pcm(c) for c in (0, 1)]) == 0
    for j in range(2):
        info = st.beam_info(j)
        assert len(info) == 3
        assert all(b["tokens"] and not banned & set(b["tokens"]) for b in info), j
        assert not banned & set(t[0] for s in st.batch_segments(j) for t in s.tokens)
    st.close()
    # best_of candidates of a forced fallback (test_gpu_bestof.py's set-up)
    st = ctx.create_state()
    fp = params(wrs, regex, temperature_inc=0.6, logprob_thold=0.0, no_speech_thold=1.0, single_segment=True, max_tokens=24)
    fp.greedy.best_of = 3
    assert st.full(fp, synthetic_pcm(5)) == 0
    assert [d["temp_idx"] for d in st.decisions()] == [1]
    info = st.cand_info(0)
    assert len(info) == 3
    assert all(c["tokens"] and not banned & set(c["tokens"]) for c in info)
    assert not banned & set(t[0] for s in st.segments() for t in s.tokens)
    st.close()
    # host sampling (best_of 1) of the same fallback
    fp.greedy.best_of = 1
    hs = run_single(ctx, fp, 5)
    assert ids_of(hs) and not banned & set(ids_of(hs))


# ---- 3. exact against the reference ---------------------------------------------------------------------------------------
def test_banned_run_is_the_reference(wrs, monkeypatch):
    monkeypatch.setenv("WHISPER_MI355X_PDEC", "0")
    monkeypatch.setenv("WHISPER_MI355X_SMALLM", "0")
    ctx = get_ctx(wrs)
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    beg, eot = v["beg"], v["eot"]
    assert (beg, eot) == (L.whisper_token_beg(ctx.ptr), L.whisper_token_eot(ctx.ptr))
    # (single_segment: a segment per timestamp pair leaves the pair's second token out of the segments)
    ids, regex = ban_of(ctx, run_batch(ctx, params(wrs, single_segment=True), CLIPS_EXACT, fixed=N_FIXED), eot)
    deny = ctx.suppress_mask(False, regex)
    got = run_batch(ctx, params(wrs, regex, single_segment=True), CLIPS_EXACT, fixed=N_FIXED)
    toks = np.array([ids_of(r)[:N_FIXED] for r in got], np.int32)
    assert toks.shape == (len(CLIPS_EXACT), N_FIXED)
    assert not set(ids) & set(toks.ravel().tolist())
    st = ctx.create_state()
    rc, raw = st.full_batch_forced(params(wrs, regex, single_segment=True), [synthetic_pcm(c) for c in CLIPS_EXACT], N_FIXED, toks,
                                   list(range(len(CLIPS_EXACT))), V)
    st.close()
    assert rc == 0
    denied_best = 0
    for j, clip in enumerate(CLIPS_EXACT):
        c = lr.ctl(is_initial=1, penult_ts=1, suppress_blank=1, tid0_initial=50, suppress_eot=1, want_nosp=1)
        ints = np.zeros(5, np.int64)
        low = []
        for i in range(N_FIXED):
            assert np.isfinite(raw[i, j]).all(), "the forced hook returns raw logits"
            ref = sr.process(raw[i, j], c, v, deny)
            if sc.decided(ref):
                assert ref["id"] == int(toks[j, i]), f"clip {clip} step {i}: engine {int(toks[j, i])}, reference {ref['id']}"
            else:
                low.append(i)
            denied_best += bool(deny[lr.process(raw[i, j], c, v)["id"]])
            c = lr.advance(c, ints, 1, 0, int(toks[j, i]), beg)
        print(f"clip {clip}: steps under the gap {low}")
        assert len(low) <= MAX_UNDECIDED, (clip, low)
    assert denied_best > 0, "the ban never changed a step's choice"


# ---- 4. errors and reuse ------------------------------------------------------------------------------------------------------
def test_bad_pattern_and_reuse(wrs):
    ctx = get_ctx(wrs)
    eot = wrs.lib().whisper_token_eot(ctx.ptr)
    ids, regex = ban_of(ctx, plain17(wrs), eot)
    st = ctx.create_state()
    pcm = synthetic_pcm(0)
    assert st.full(params(wrs, "("), pcm) == -8
    assert st.full_batch(params(wrs, "("), [pcm] * 5) == -8
    assert st.full_batch(params(wrs, "(", nst=True), [pcm] * 17) == -8
    # (no_context: whisper_full would carry the last call's text into the next as its prompt)
    fresh_ban = run_single(ctx, params(wrs, regex, no_context=True), 0)
    fresh_plain = run_single(ctx, params(wrs, no_context=True), 0)
    assert fresh_ban[0] and fresh_plain[0] and fresh_ban != fresh_plain
    # one state: ban, no ban, the ban again (the step graphs are keyed by deny on / off, the buffer keeps its words)
    for rx, want in ((regex, fresh_ban), (None, fresh_plain), (regex, fresh_ban)):
        assert st.full(params(wrs, rx, no_context=True), pcm) == 0
        assert (seg_rows(st.segments()), st.decisions()) == want
    st.close()


# ---- 5. suppress_nst ----------------------------------------------------------------------------------------------------------
def test_suppress_nst(wrs):
    ctx = get_ctx(wrs)
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    m = ctx.suppress_mask(True, None)
    want = sorted([ord(ch) for ch in '"#()*+/:;<=>@[\\]^_`{|}~'] + [[ctx.token_str(i) for i in range(V)].index(b" -")])
    assert len(want) == 24 and np.nonzero(m)[0].tolist() == want
    got = run_batch(ctx, params(wrs, nst=True, single_segment=True), range(5), fixed=N_FIXED)
    for j, r in enumerate(got):
        assert len(ids_of(r)) == N_FIXED and not set(want) & set(ids_of(r)), j
