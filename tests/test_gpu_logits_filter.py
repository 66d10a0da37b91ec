"""whisper_full_params.logits_filter_callback and tdrz_enable end to end through whisper_full_with_state,
whisper_full_parallel and whisper_mi355x_full_batch on tiny+conf, f16, synthetic_pcm clips, max_tokens = 24.

- recorder: the callback's (n_tokens, token ids, row) per call on one clip, greedy, t = 0: the k-th call of the attempt has
  n_tokens == k and the attempt's token prefix, which ends in the returned segment's tokens; in every row the ids of the
  rules that precede the callback are -inf (sot, nosp, solm, translate, transcribe, prev, <|notimestamps|>, the 100
  languages; EOT and " " iff n_tokens == 0) and every other entry is the raw logit bit for bit (from a teacher-forced
  full_batch_forced run of the same tokens; both runs with the persistent step and the small-M path off, as
  test_gpu_suppress.py's exact test sets them, so a row's bits do not depend on the path).
- a ban of 8 tokens through the callback is the ban through suppress_regex: segments, token ids, times, p / plog and window
  decisions, for 1, 5 and 17 clips (the persistent step, the split logits form, one workgroup per row), beam search K = 3
  and a forced fallback with best_of = 3 (test_gpu_bestof.py's set-up). Everything is compared exactly: both runs sum the
  same finite set in the same order.
- a callback that touches nothing gives the run without one bit for bit (greedy with 1 and 5 clips, beam search, the forced
  best_of fallback at t = 0.6, a grammar call). This one passes without the feature: it guards the split.
- launch counts: the stage kernel's class counts nothing in a call without a callback and one launch per logits launch in a
  call with one (beam search: but the prefill's top-k pass, which reads the rows already staged); a state that ran with a
  callback runs without one next and matches a fresh state.
- the callback's ctx, state and user_data are the call's, the rows of a step come in staged order, and a fixed-work
  teacher-forced run calls every row of every step with the forced tokens as its history.
- tdrz: a callback that adds 1e4 to row[solm] when n_tokens == 3. With tdrz_enable the segment that holds the token
  reports speaker_turn_next through the state getter, the context getter, the batch getter and after
  whisper_full_parallel's merge, and its text has no [_SOLM_] (single_segment: on this model the token at index 3 stands
  alone between two timestamp pairs, and a segment without text is dropped, as upstream drops it); with segments per
  timestamp pair and print_special the segment that holds it shows [_SOLM_] and reports the turn and the other segments
  report false, and without print_special no segment holds it and none reports one; without tdrz_enable the callback
  changes nothing (-inf + 1e4) and every segment reports false.
"""
import numpy as np
import pytest

import grammar_cases as gc
import logits_cases as lc
from conftest import model_path
from make_model import synthetic_pcm
from test_gpu_suppress import ban_of, ids_of, seg_rows

pytestmark = pytest.mark.gpu

SHAPE = "tiny+conf"
K_LOGITS, K_TOPK, K_STAGE = 5, 12, 18

_CTX = {}


def get_ctx(wrs):
    if "c" not in _CTX:
        _CTX["c"] = wrs.WhisperContext(model_path(SHAPE), dtype=wrs.F16)
    return _CTX["c"]


@pytest.fixture(scope="module", autouse=True)
def _close_ctxs():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def params(wrs, cb=None, base=None, **kw):
    p = base or wrs.reference_full_params("en")
    p.max_tokens = 24
    for k, v in kw.items():
        setattr(p, k, v)
    if cb is not None:
        p.set_filter_logits_callback(cb)
    return p


class Guard:
    """A callback whose exceptions are kept (ctypes would print and drop them) and whose calls are counted."""

    def __init__(self, fn):
        self.fn, self.errors, self.calls = fn, [], 0

    def __call__(self, tokens, row):
        self.calls += 1
        try:
            self.fn(tokens, row)
        except Exception as e:  # noqa: BLE001
            self.errors.append(repr(e))


def identity():
    return Guard(lambda tokens, row: None)


def banner(ids):
    def fn(tokens, row):
        row[ids] = -np.inf
    return Guard(fn)


def run_single(ctx, p, clip):
    st = ctx.create_state()
    assert st.full(p, synthetic_pcm(clip)) == 0
    out = seg_rows(st.segments()), st.decisions()
    st.close()
    return out


def run_batch(ctx, p, clips):
    st = ctx.create_state()
    assert st.full_batch(p, [synthetic_pcm(c) for c in clips]) == 0
    out = [(seg_rows(st.batch_segments(j)), st.decisions(j)) for j in range(len(clips))]
    st.close()
    return out


def run_beam(wrs, ctx, cb=None, **kw):
    st = ctx.create_state()
    bp = params(wrs, cb, base=wrs.beam_full_params(3, "en"), temperature_inc=0.0, single_segment=True, **kw)
    assert st.full_batch(bp, [synthetic_pcm(0)]) == 0
    out = seg_rows(st.batch_segments(0)), st.decisions(0), st.beam_info(0)
    st.close()
    assert len(out[2]) == 3
    return out


def run_bestof(wrs, ctx, cb=None, **kw):
    """test_gpu_bestof.py's forced fallback: the t = 0 attempt fails logprob_thold = 0, the t = 0.6 attempt draws 3 candidates"""
    st = ctx.create_state()
    fp = params(wrs, cb, temperature_inc=0.6, logprob_thold=0.0, no_speech_thold=1.0, single_segment=True, **kw)
    fp.greedy.best_of = 3
    assert st.full(fp, synthetic_pcm(5)) == 0
    out = seg_rows(st.segments()), st.decisions(), st.cand_info(0)
    st.close()
    assert [d["temp_idx"] for d in out[1]] == [1] and len(out[2]) == 3
    return out


_PLAIN = {}


def plain17(wrs):
    if "p" not in _PLAIN:
        _PLAIN["p"] = run_batch(get_ctx(wrs), params(wrs), range(17))
    return _PLAIN["p"]


def the_ban(wrs):
    ctx = get_ctx(wrs)
    return ban_of(ctx, plain17(wrs), wrs.lib().whisper_token_eot(ctx.ptr))


# ---- 1. what the callback is given ------------------------------------------------------------------------------------------
def test_recorder(wrs, monkeypatch):
    monkeypatch.setenv("WHISPER_MI355X_PDEC", "0")
    monkeypatch.setenv("WHISPER_MI355X_SMALLM", "0")
    ctx = get_ctx(wrs)
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    calls = []
    rec = Guard(lambda tokens, row: calls.append((len(tokens), [t.id for t in tokens], row.copy())))
    kw = dict(single_segment=True, temperature_inc=0.0)  # one window, one attempt
    segs, dec = run_single(ctx, params(wrs, rec, **kw), 0)
    assert not rec.errors, rec.errors[:3]
    assert len(segs) == 1 and len(dec) == 1 and dec[0]["temp_idx"] == 0
    assert len(calls) >= 8 and calls[0][0] == 0
    for k, (n, ids, row) in enumerate(calls):
        assert n == k and len(ids) == k, f"call {k}: n_tokens {n}"
        assert row.dtype == np.float32 and row.shape == (V,)
        if k:
            assert ids[:-1] == calls[k - 1][1], f"call {k}: the history is not the last call's plus one token"
    seg_ids = [t[0] for t in segs[0][3]]
    last = calls[-1][1]
    assert len(seg_ids) <= len(last) + 1 and seg_ids[:len(last)] == last[:len(seg_ids)], (seg_ids, last)
    # the rows: the pre-callback ids are -inf, the rest is the raw row
    K = len(calls)
    forced = np.asarray((last + [seg_ids[-1] if len(seg_ids) > len(last) else v["eot"]])[:K], np.int32).reshape(1, K)
    st = ctx.create_state()
    rc, raw = st.full_batch_forced(params(wrs, **kw), [synthetic_pcm(0)], K, forced, [0], V)
    st.close()
    assert rc == 0
    pre = [v[k] for k in ("sot", "nosp", "solm", "translate", "transcribe", "prev", "not_")] + \
        list(range(v["sot"] + 1, v["sot"] + 1 + v["n_lang"]))
    assert len(set(pre)) >= 7 + 99  # (logits_cases' language range may reach the translate token: masked either way)
    for k, (n, ids, row) in enumerate(calls):
        masked = np.zeros(V, bool)
        masked[pre] = True
        if n == 0:
            masked[[v["eot"], v["space"]]] = True
        assert (row[masked] == -np.inf).all(), f"call {k}: a pre-callback id is not -inf"
        assert np.isfinite(raw[k, 0]).all()
        bad = np.nonzero(row[~masked].view(np.uint32) != raw[k, 0][~masked].view(np.uint32))[0]
        assert bad.size == 0, f"call {k}: {bad.size} entries are not the raw logits (first {bad[:4]})"


# ---- 2. a ban through the callback is the ban through suppress_regex ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 17])
def test_ban_equals_regex_greedy(wrs, n):
    ctx = get_ctx(wrs)
    ids, regex = the_ban(wrs)
    cb = banner(ids)
    if n == 1:
        got = [run_single(ctx, params(wrs, cb), 0)]
        want = [run_single(ctx, params(wrs, suppress_regex=regex.encode()), 0)]
    else:
        got = run_batch(ctx, params(wrs, cb), range(n))
        want = run_batch(ctx, params(wrs, suppress_regex=regex.encode()), range(n))
    assert not cb.errors and cb.calls > 0
    for j in range(n):
        assert ids_of(got[j]) and not set(ids) & set(ids_of(got[j])), j
        assert got[j] == want[j], f"{n} clips, clip {j}"
    assert any(got[j] != plain17(wrs)[j] for j in range(n)), "the ban changed nothing"


def test_ban_equals_regex_beam(wrs):
    ctx = get_ctx(wrs)
    ids, regex = the_ban(wrs)
    cb = banner(ids)
    got = run_beam(wrs, ctx, cb)
    assert not cb.errors and cb.calls > 0
    assert got == run_beam(wrs, ctx, suppress_regex=regex.encode())
    assert all(b["tokens"] and not set(ids) & set(b["tokens"]) for b in got[2])


def test_ban_equals_regex_bestof(wrs):
    ctx = get_ctx(wrs)
    ids, regex = the_ban(wrs)
    cb = banner(ids)
    got = run_bestof(wrs, ctx, cb)
    assert not cb.errors and cb.calls > 0
    assert got == run_bestof(wrs, ctx, suppress_regex=regex.encode())
    assert all(c["tokens"] and not set(ids) & set(c["tokens"]) for c in got[2])


# ---- 3. a callback that touches nothing ----------------------------------------------------------------------------------------
def test_identity_callback(wrs):
    ctx = get_ctx(wrs)
    cb = identity()
    assert run_single(ctx, params(wrs, cb), 0) == run_single(ctx, params(wrs), 0)
    assert run_batch(ctx, params(wrs, cb), range(5)) == run_batch(ctx, params(wrs), range(5))
    assert run_beam(wrs, ctx, cb) == run_beam(wrs, ctx)
    assert run_bestof(wrs, ctx, cb) == run_bestof(wrs, ctx)
    G2 = gc.GRAMMARS["G2"]
    gp = [params(wrs, c, single_segment=True) for c in (cb, None)]
    for p in gp:
        p.set_grammar(G2[0], G2[1])
    assert run_single(ctx, gp[0], 0) == run_single(ctx, gp[1], 0)
    assert not cb.errors


# ---- 4. launch counts, and a state after a callback -------------------------------------------------------------------------
def test_launch_counts_and_reuse(wrs):
    import ctypes as C
    ctx = get_ctx(wrs)
    L = wrs.lib()
    pcm = synthetic_pcm(0)
    out = (C.c_double * 3)()

    def count(st, cls):
        assert L.whisper_mi355x_kernel_stats(st.ptr, cls, out) == 0
        return int(out[1])

    fresh = run_single(ctx, params(wrs, no_context=True), 0)
    st = ctx.create_state()
    mask = (1 << K_LOGITS) | (1 << K_TOPK) | (1 << K_STAGE)
    assert L.whisper_mi355x_kernel_timing(st.ptr, mask) == 0
    assert st.full(params(wrs, no_context=True), pcm) == 0
    n_plain = count(st, K_LOGITS)
    assert n_plain > 0 and count(st, K_STAGE) == 0 and st.logits_stage_stats()[1] == 0
    cb = identity()
    assert L.whisper_mi355x_kernel_timing(st.ptr, mask) == 0  # (resets the counts)
    assert st.full(params(wrs, cb, no_context=True), pcm) == 0
    assert not cb.errors
    ms, launches, work = st.logits_stage_stats()
    # one clip: one row per launch (the plain run's count may hold the pipelined path's speculative steps, so it is
    # not compared)
    assert launches == count(st, K_STAGE) == count(st, K_LOGITS) == cb.calls and count(st, K_TOPK) == 0
    assert work == launches * 8.0 * L.whisper_n_vocab(ctx.ptr) and ms > 0
    assert (seg_rows(st.segments()), st.decisions()) == fresh
    assert L.whisper_mi355x_kernel_timing(st.ptr, mask) == 0
    assert st.full(params(wrs, no_context=True), pcm) == 0
    assert count(st, K_STAGE) == 0 and count(st, K_LOGITS) == n_plain
    assert (seg_rows(st.segments()), st.decisions()) == fresh
    # beam search: every logits launch has its stage launch, but the prefill's top-k pass, which reads the rows the
    # callbacks of the prefill's greedy pass just left (one callback per row, not two): one per attempt
    bp = params(wrs, cb, base=wrs.beam_full_params(3, "en"), temperature_inc=0.0, single_segment=True)
    assert L.whisper_mi355x_kernel_timing(st.ptr, mask) == 0
    assert st.full_batch(bp, [pcm]) == 0
    attempts = len(st.decisions(0))  # (temperature_inc = 0: one attempt per window)
    assert attempts >= 1 and count(st, K_TOPK) > attempts
    assert count(st, K_STAGE) == count(st, K_LOGITS) + count(st, K_TOPK) - attempts
    assert count(st, K_LOGITS) == attempts  # (the prefills' greedy passes)
    st.close()


# ---- 4b. the callback's ctx and state, and a fixed-work forced run ------------------------------------------------------------
def test_ctx_state_and_forced(wrs):
    import ctypes as C
    ctx = get_ctx(wrs)
    V = wrs.lib().whisper_n_vocab(ctx.ptr)
    seen = []

    def raw_cb(c, s, tokens, n_tokens, logits, user_data):
        seen.append((c, s, n_tokens, [tokens[i].id for i in range(n_tokens)], user_data))

    tramp = wrs.LOGITS_FILTER_CALLBACK(raw_cb)
    st = ctx.create_state()
    p = params(wrs, temperature_inc=0.0, single_segment=True)
    p.logits_filter_callback = C.cast(tramp, C.c_void_p)
    p.logits_filter_callback_user_data = 0x1234
    assert st.full_batch(p, [synthetic_pcm(c) for c in range(5)]) == 0
    assert seen and all((c, s, u) == (ctx.ptr, st.ptr, 0x1234) for c, s, _, _, u in seen)
    assert [n for _, _, n, _, _ in seen[:5]] == [0] * 5 and [n for _, _, n, _, _ in seen[5:10]] == [1] * 5  # staged order
    # fixed-work, teacher-forced: every row of every step is called, with the forced tokens as its history
    del seen[:]
    K = 6
    forced = (np.arange(2 * K, dtype=np.int32).reshape(2, K) * 37 + 1000)
    rc, _ = st.full_batch_forced(p, [synthetic_pcm(c) for c in range(2)], K, forced, [0], V)
    assert rc == 0
    assert [(n, ids) for _, _, n, ids, _ in seen] == [(k, forced[j, :k].tolist()) for k in range(K) for j in range(2)]
    assert all((c, s) == (ctx.ptr, st.ptr) for c, s, _, _, _ in seen)
    st.close()


# ---- 5. tdrz ------------------------------------------------------------------------------------------------------------------
def test_tdrz(wrs):
    import ctypes as C
    ctx = get_ctx(wrs)
    L = wrs.lib()
    solm = lc.vocab(L.whisper_n_vocab(ctx.ptr))["solm"]
    assert ctx.token_str(solm) == b"[_SOLM_]"

    def turn():
        def fn(tokens, row):
            if len(tokens) == 3:
                row[solm] += np.float32(1e4)
        return Guard(fn)

    def flags_ok(segs, where):
        """every segment's flag says whether solm lies in its token range; returns the flags"""
        for i, s in enumerate(segs):
            assert s.speaker_turn_next == (solm in [t[0] for t in s.tokens]), (where, i)
        return [s.speaker_turn_next for s in segs]

    # On this model a text token is always followed by a timestamp pair, so the token at index 3 stands alone between two
    # pairs. single_segment: the window's one segment holds it. Segments per timestamp pair: a segment without text is
    # dropped, as upstream drops it, so the token is in a segment's range only with print_special, which gives it a text.
    kw = dict(temperature_inc=0.0)
    one = dict(single_segment=True, **kw)
    plain = run_batch(ctx, params(wrs, **kw), range(5))
    # tdrz_enable with the callback: one state, single API
    cb = turn()
    st = ctx.create_state()
    assert st.full(params(wrs, cb, tdrz_enable=True, **one), synthetic_pcm(0)) == 0
    single = st.segments()
    st.close()
    assert not cb.errors and flags_ok(single, "single") == [True]
    assert b"[_SOLM_]" not in single[0].text and single[0].text
    # the batch getter, 5 clips
    st = ctx.create_state()
    assert st.full_batch(params(wrs, cb, tdrz_enable=True, **one), [synthetic_pcm(c) for c in range(5)]) == 0
    for j in range(5):
        assert flags_ok(st.batch_segments(j), f"batch clip {j}") == [True]
    st.close()
    # whisper_full_parallel's merge carries the field
    st = ctx.create_state()
    # (two 30 s pieces: a 15 s piece's attempt ends with its first timestamp, before its fourth token)
    assert st.full_parallel(params(wrs, cb, tdrz_enable=True, **one), np.concatenate([synthetic_pcm(0), synthetic_pcm(1)]), 2) == 0
    f = flags_ok(st.segments(), "parallel")
    assert len(f) == 2 and any(f), f
    st.close()
    # the context's getter (the default state)
    dctx = wrs.WhisperContext.new_with_default_state(model_path(SHAPE))
    try:
        assert dctx.full_parallel(params(wrs, cb, tdrz_enable=True, **one), synthetic_pcm(0), 1) == 0
        L.whisper_full_n_tokens.argtypes = [C.c_void_p, C.c_int]
        L.whisper_full_get_token_id.argtypes = [C.c_void_p, C.c_int, C.c_int]
        n_seg = L.whisper_full_n_segments(dctx.ptr)
        got = [bool(L.whisper_full_get_segment_speaker_turn_next(dctx.ptr, i)) for i in range(n_seg)]
        want = [solm in [L.whisper_full_get_token_id(dctx.ptr, i, t) for t in range(L.whisper_full_n_tokens(dctx.ptr, i))]
                for i in range(n_seg)]
        assert got == want == [True]
        assert all(b"[_SOLM_]" not in text for _, _, text in dctx.default_segments())
    finally:
        dctx.close()
    # segments per timestamp pair, print_special: the segment that holds the token reports the turn and shows it, the
    # other segments report false
    st = ctx.create_state()
    assert st.full_batch(params(wrs, cb, tdrz_enable=True, print_special=True, **kw), [synthetic_pcm(c) for c in range(5)]) == 0
    for j in range(5):
        segs = st.batch_segments(j)
        f = flags_ok(segs, f"print_special clip {j}")
        assert f.count(True) >= 1 and f.count(False) >= 2, (j, f)
        assert [b"[_SOLM_]" in s.text for s in segs] == f, j
    st.close()
    # a further scenario: the token raised at n_tokens == 1 follows the window's first text token, so it lies in that
    # segment's range; its text is hidden, and of the several segments only that one reports the turn
    def early(tokens, row):
        if len(tokens) == 1:
            row[solm] += np.float32(1e4)
    cb1 = Guard(early)
    st = ctx.create_state()
    assert st.full(params(wrs, cb1, tdrz_enable=True, **kw), synthetic_pcm(0)) == 0
    f = flags_ok(st.segments(), "n_tokens == 1")
    assert not cb1.errors and f[0] and f.count(False) >= 2, f
    assert all(b"[_SOLM_]" not in s.text for s in st.segments())
    st.close()
    # ... and without print_special no segment holds it: none reports a turn
    st = ctx.create_state()
    assert st.full(params(wrs, cb, tdrz_enable=True, **kw), synthetic_pcm(0)) == 0
    f = flags_ok(st.segments(), "no print_special")
    assert len(f) >= 2 and not any(f) and all(b"[_SOLM_]" not in s.text for s in st.segments())
    st.close()
    # tdrz_enable off: -inf + 1e4 is -inf
    st = ctx.create_state()
    assert st.full_batch(params(wrs, cb, **kw), [synthetic_pcm(c) for c in range(5)]) == 0
    for j in range(5):
        segs = st.batch_segments(j)
        assert (seg_rows(segs), st.decisions(j)) == plain[j], j
        assert not any(s.speaker_turn_next for s in segs), j
        assert solm not in [t[0] for s in segs for t in s.tokens]
    st.close()
    assert not cb.errors
    # tdrz_enable alone suppresses nothing else and reports no turn on a model that never emits the token
    st = ctx.create_state()
    assert st.full(params(wrs, tdrz_enable=True, **kw), synthetic_pcm(0)) == 0
    assert not any(s.speaker_turn_next for s in st.segments())
    st.close()
