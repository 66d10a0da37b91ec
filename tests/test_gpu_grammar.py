"""whisper_full_params.grammar_rules end to end through whisper_full_with_state / whisper_mi355x_full_batch
on tiny+conf, f16, with the grammars of tests/grammar_cases.py.

1. The constraint holds: under G2 (penalty 100) every sequence of every decoding mode (greedy with 1, 5 and 17 clips, beam
   search, best_of candidates of a forced fallback, host sampling) replays through tests/grammar_ref.py with a non-empty
   stack list after every text token, and EOT only where the grammar may end; the plain run of the same clips violates
   G2. Fails without the feature.
2. A fixed-token run under G2 and G4 is exact against tests/grammar_logits_ref.py over the engine's own raw logits
   (test_gpu_suppress.py's method: teacher-forced, the small-M path and the persistent step off).
3. An accept-everything grammar gives the plain run's tokens and text.
4. Every invalid grammar returns -9 (single and batch API, a 40-clip batch included) and leaves the state usable; one state
   runs grammar, plain, grammar; rules with n_grammar_rules = 0 are a plain call.
5. / 6. Penalty 0: the first step has the plain call's token, the model violates G1 at once and the rest of the run is
   the plain run's.
7. whisper_mi355x_grammar_stats: every row of a G2 call is decided by the reject kernel, a paired batch counts both halves.

CLIPS_EXACT: synthetic_pcm seeds for which the CPU oracle's own logits leave no step of the 24 under
logits_cases.MIN_GAP for G2 and G4 (tools/grammar_pick_clips.py); the test asserts a cap of 2 over the engine's logits.
"""
import numpy as np
import pytest

import grammar_cases as gc
import grammar_logits_ref as glr
import grammar_ref as gr
import logits_cases as lc
import logits_ref as lr
import suppress_cases as sc
from conftest import model_path
from make_model import synthetic_pcm

pytestmark = pytest.mark.gpu

SHAPE = "tiny+conf"
N_FIXED = 24
CLIPS_EXACT = (0, 1, 2, 3, 4)
MAX_UNDECIDED = 2

_CTX = {}
_TOKS = {}


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


def params(wrs, grammar=None, penalty=None, **kw):
    """grammar: (rules, start) or None."""
    p = kw.pop("base", None) or wrs.reference_full_params("en")
    if grammar is not None:
        p.set_grammar(grammar[0], grammar[1])
    if penalty is not None:
        p.set_grammar_penalty(penalty)
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


def texts(result):
    return [s[2] for s in result[0]]


def tokens_of(wrs, ctx):
    if "toks" not in _TOKS:
        L = wrs.lib()
        _TOKS["toks"] = [ctx.token_str(i) for i in range(L.whisper_n_vocab(ctx.ptr))]
    return _TOKS["toks"]


def follows(toks, eot, grammar, ids):
    """The sequence replayed from the init state: None when the stack list is non-empty after every text token and EOT
    appears only where the grammar may end, else the index of the first offending token."""
    st = gr.State(*grammar)
    for k, i in enumerate(ids):
        if i == eot:
            if not gr.allow_eot(st.stacks):
                return k
            continue
        st.accept_token(toks[i])
        if not st.stacks:
            return k
    return None


# single_segment: one segment per window, so a segment's tokens are one attempt's sequence (every attempt starts from
# the init state)
def check_segments(toks, eot, grammar, result, where):
    n = 0
    for seg in result[0]:
        ids = [t[0] for t in seg[3]]
        assert follows(toks, eot, grammar, ids) is None, (where, [toks[i] for i in ids])
        n += sum(i < eot for i in ids)
    return n


def test_constraint_holds(wrs):
    ctx = get_ctx(wrs)
    L = wrs.lib()
    eot = L.whisper_token_eot(ctx.ptr)
    V = L.whisper_n_vocab(ctx.ptr)
    toks = tokens_of(wrs, ctx)
    G2 = gc.GRAMMARS["G2"]
    # penalty 100 decides: a raw row of the model spans less
    st = ctx.create_state()
    forced = np.zeros((1, 2), np.int32) + toks.index(b" the")
    rc, raw = st.full_batch_forced(params(wrs, single_segment=True), [synthetic_pcm(0)], 2, forced, [0], V)
    st.close()
    assert rc == 0 and float(raw[0, 0].max() - raw[0, 0].min()) < 100.0
    kw = dict(single_segment=True)
    plain = run_batch(ctx, params(wrs, **kw), range(17))
    assert all(ids_of(r) for r in plain)
    assert all(any(follows(toks, eot, G2, [t[0] for t in seg[3]]) is not None for seg in r[0]) for r in plain), \
        "a plain run follows G2 already"
    one = run_single(ctx, params(wrs, G2, **kw), 0)  # 1 clip
    assert check_segments(toks, eot, G2, one, "1 clip") > 0
    assert texts(one) != texts(plain[0])
    for n in (5, 17):
        got = run_batch(ctx, params(wrs, G2, **kw), range(n))
        for j, r in enumerate(got):
            assert check_segments(toks, eot, G2, r, f"{n} clips, clip {j}") > 0
            assert texts(r) != texts(plain[j]), (n, j)
    # beam search: every beam
    st = ctx.create_state()
    bp = params(wrs, G2, base=wrs.beam_full_params(3, "en"), temperature_inc=0.0, single_segment=True, max_tokens=24)
    assert st.full_batch(bp, [synthetic_pcm(c) for c in (0, 1)]) == 0
    for j in range(2):
        info = st.beam_info(j)
        assert len(info) == 3
        for b in info:
            assert b["tokens"] and follows(toks, eot, G2, b["tokens"]) is None, (j, [toks[i] for i in b["tokens"]])
        check_segments(toks, eot, G2, (seg_rows(st.batch_segments(j)),), f"beam clip {j}")
    st.close()
    # best_of candidates of a forced fallback (test_gpu_bestof.py's set-up), then host sampling of the same fallback
    st = ctx.create_state()
    fp = params(wrs, G2, temperature_inc=0.6, logprob_thold=0.0, no_speech_thold=1.0, single_segment=True, max_tokens=24)
    fp.greedy.best_of = 3
    assert st.full(fp, synthetic_pcm(5)) == 0
    assert [d["temp_idx"] for d in st.decisions()] == [1]
    info = st.cand_info(0)
    assert len(info) == 3
    for c in info:
        assert c["tokens"] and follows(toks, eot, G2, c["tokens"]) is None, [toks[i] for i in c["tokens"]]
    check_segments(toks, eot, G2, (seg_rows(st.segments()),), "best_of winner")
    st.close()
    fp.greedy.best_of = 1
    hs = run_single(ctx, fp, 5)
    assert check_segments(toks, eot, G2, hs, "host sampling") > 0


@pytest.mark.parametrize("gname", ["G2", "G4"])
def test_grammar_run_is_the_reference(wrs, monkeypatch, gname):
    monkeypatch.setenv("WHISPER_MI355X_PDEC", "0")
    monkeypatch.setenv("WHISPER_MI355X_SMALLM", "0")
    ctx = get_ctx(wrs)
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    v = lc.vocab(V)
    beg, eot = v["beg"], v["eot"]
    vocab_toks = tokens_of(wrs, ctx)
    G = gc.GRAMMARS[gname]
    pcm = [synthetic_pcm(c) for c in CLIPS_EXACT]
    got = run_batch(ctx, params(wrs, G, single_segment=True), CLIPS_EXACT, fixed=N_FIXED)
    toks = np.array([ids_of(r)[:N_FIXED] for r in got], np.int32)
    assert toks.shape == (len(CLIPS_EXACT), N_FIXED)
    st = ctx.create_state()
    rc, raw = st.full_batch_forced(params(wrs, G, single_segment=True), pcm, N_FIXED, toks, list(range(len(CLIPS_EXACT))), V)
    st.close()
    assert rc == 0
    masks = {}
    changed = 0
    for j, clip in enumerate(CLIPS_EXACT):
        c = lr.ctl(is_initial=1, penult_ts=1, suppress_blank=1, tid0_initial=50, suppress_eot=1, want_nosp=1)
        ints = np.zeros(5, np.int64)
        gs = gr.State(*G)
        low = []
        for i in range(N_FIXED):
            assert np.isfinite(raw[i, j]).all(), "the forced hook returns raw logits"
            gram = None
            if gs.stacks:
                key = (tuple(gs.stacks), gs.partial)
                if key not in masks:
                    masks[key] = np.array(gs.reject(vocab_toks, eot))
                gram = masks[key]
            ref = glr.process(raw[i, j], c, v, None, gram, 100.0)
            if sc.decided(ref):
                assert ref["id"] == int(toks[j, i]), f"clip {clip} step {i}: engine {int(toks[j, i])}, reference {ref['id']}"
            else:
                low.append(i)
            changed += ref["id"] != lr.process(raw[i, j], c, v)["id"]
            gs.accept_token(vocab_toks[int(toks[j, i])])
            c = lr.advance(c, ints, 1, 0, int(toks[j, i]), beg)
        print(f"{gname} clip {clip}: steps under the gap {low}, states met {len(masks)}")
        assert gs.stacks, "the run left the grammar"
        assert len(low) <= MAX_UNDECIDED, (clip, low)
    assert changed > 0, "the grammar never changed a step's choice"


def test_accept_everything_grammar(wrs):
    ctx = get_ctx(wrs)
    toks = tokens_of(wrs, ctx)
    clips = range(5)
    kw = dict(single_segment=True)
    plain = run_batch(ctx, params(wrs, **kw), clips)
    got = run_batch(ctx, params(wrs, gc.ACCEPT_ALL, **kw), clips)
    compared = 0
    for j in clips:
        ids = ids_of(plain[j])
        if any(len(toks[i]) == 1 and toks[i][0] >= 0x80 for i in ids):  # an invalid-UTF-8 single-byte token: rejected
            continue
        compared += 1
        assert ids_of(got[j]) == ids and texts(got[j]) == texts(plain[j]), j
    assert compared >= 3


def test_errors_and_reuse(wrs):
    ctx = get_ctx(wrs)
    G2 = gc.GRAMMARS["G2"]
    st = ctx.create_state()
    pcm = synthetic_pcm(0)
    for name, g in gc.INVALID.items():
        assert st.full(params(wrs, g), pcm) == wrs.GRAMMAR_ERR, name
        assert st.full_batch(params(wrs, g), [pcm] * 5) == wrs.GRAMMAR_ERR, name
    assert st.full_batch(params(wrs, gc.INVALID["left_recursive"]), [pcm[:16000]] * 40) == wrs.GRAMMAR_ERR
    # (no_context: whisper_full would carry the last call's text into the next as its prompt)
    fresh_gram = run_single(ctx, params(wrs, G2, no_context=True), 0)
    fresh_plain = run_single(ctx, params(wrs, no_context=True), 0)
    assert fresh_gram[0] and fresh_plain[0] and fresh_gram != fresh_plain
    # one state, after the refused calls: plain; then grammar, plain, grammar (the step graphs are keyed by the grammar)
    for g, want in ((None, fresh_plain), (G2, fresh_gram), (None, fresh_plain), (G2, fresh_gram)):
        assert st.full(params(wrs, g, no_context=True), pcm) == 0
        assert (seg_rows(st.segments()), st.decisions()) == want
    # rules given, n_grammar_rules = 0: a plain call
    p = params(wrs, G2, no_context=True)
    p.n_grammar_rules = 0
    assert st.full(p, pcm) == 0
    assert (seg_rows(st.segments()), st.decisions()) == fresh_plain
    st.close()


def test_penalty_zero_is_the_plain_run(wrs):
    """Penalty 0 with G1: the first step has the plain call's token (the rule is soft from the first step), the model
    violates G1 at once, the stack list empties, and the whole run is the plain run's tokens."""
    ctx = get_ctx(wrs)
    L = wrs.lib()
    eot = L.whisper_token_eot(ctx.ptr)
    toks = tokens_of(wrs, ctx)
    G1 = gc.GRAMMARS["G1"]
    kw = dict(single_segment=True)
    plain = run_batch(ctx, params(wrs, **kw), range(5))
    got = run_batch(ctx, params(wrs, G1, 0.0, **kw), range(5))
    for j in range(5):
        first = next(i for i in ids_of(plain[j]) if i < eot)
        assert follows(toks, eot, G1, [first]) is not None, "the plain run's first text token follows G1"
        assert ids_of(got[j]) == ids_of(plain[j]) and texts(got[j]) == texts(plain[j]), j
    # and with the default penalty the first text token does follow it
    pen = run_batch(ctx, params(wrs, G1, **kw), range(5))
    for j in range(5):
        first = next(i for i in ids_of(pen[j]) if i < eot)
        assert follows(toks, eot, G1, [first]) is None, j


def test_stats(wrs):
    """Every row of a G2 call (the grammar of test 1) is decided by the reject kernel: none patched, none built by the
    host; the kernel's launches are timed under class 16 (K_GRAMMAR). A paired batch (more than 128 clips) counts both
    halves."""
    ctx = get_ctx(wrs)
    L = wrs.lib()
    st = ctx.create_state()
    zero = {"rows_device": 0, "rows_patched": 0, "rows_host": 0, "kernel_ms": 0.0, "kernel_launches": 0}
    assert st.grammar_stats() == zero
    assert L.whisper_mi355x_kernel_timing(st.ptr, 1 << 16) == 0
    assert st.full_batch(params(wrs, single_segment=True), [synthetic_pcm(c) for c in range(3)]) == 0
    assert st.grammar_stats() == zero
    assert st.full_batch(params(wrs, gc.GRAMMARS["G2"], single_segment=True), [synthetic_pcm(c) for c in range(3)]) == 0
    s = st.grammar_stats()
    n_tok = sum(len(seg.tokens) for j in range(3) for seg in st.batch_segments(j))
    print("grammar stats", s)
    assert s["rows_device"] >= n_tok > 0 and s["rows_patched"] == 0 and s["rows_host"] == 0  # every step's row had a mask
    assert s["kernel_launches"] > 0 and s["kernel_ms"] > 0.0
    print(f"K_GRAMMAR: {1e3 * s['kernel_ms'] / s['kernel_launches']:.1f} us per launch of 3 rows")
    assert L.whisper_mi355x_kernel_timing(st.ptr, 0) == 0
    st.close()
    st = ctx.create_state()
    pcm = synthetic_pcm(0)[:16000 * 3]
    assert st.full_batch(params(wrs, gc.GRAMMARS["G2"], single_segment=True, max_tokens=4), [pcm] * 130) == 0
    s = st.grammar_stats()
    assert s["rows_device"] >= 130 * 2 and s["rows_patched"] == 0 and s["rows_host"] == 0, s
    st.close()
