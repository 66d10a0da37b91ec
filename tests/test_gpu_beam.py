"""Beam search through whisper_full_with_state / whisper_mi355x_full_batch on the GPU.

Exact runs: the reference is tests/beam_ref.py driven by the engine's own raw logits. For the live prefixes of a step
one teacher-forced call (whisper_mi355x_full_batch_forced) decodes K copies of the clip along those prefixes and
returns the spot logits of the step; like a beam step it runs the split-K launch chain in the cache form (the small-M
path and the persistent step are switched off for these calls), where a row's results do not depend on the step's
other rows. So every beam's tokens, flags and the winner must equal the reference exactly, sum_logprobs_all within
the top-k kernel's plog bar (tests/test_gpu_beam_kernels.py) times the sequence length, and the segments are the winner's.
That pins the self-cache gather and its common-prefix rule: a wrong or missing row changes the logits of every later step.

The clips were picked on the CPU by running the same reference over the oracle's logits (tools/beam_pick_clips.py);
the reference's smallest deciding gap on the engine's logits must exceed 1e-3 nats, else the test fails.

K = 1 must give greedy's bits, and the edges: beam_size 9, a forced fallback, a recycled state.
"""
import os

import numpy as np
import pytest

import beam_ref as br
from conftest import model_path
from make_model import synthetic_pcm, synthetic_vocab
from test_gpu_beam_kernels import PLOG_BAR

pytestmark = pytest.mark.gpu

SPACE = synthetic_vocab().index(b" ")
# synthetic_pcm indices whose beam searches are decided by the widest gaps over the oracle's logits
# (tools/beam_pick_clips.py over clips 0..95): tiny+conf with timestamps, K = 5 (0.059, 0.051 nats) and K = 3 (0.082,
# 0.054). tiny+conf+eot without timestamps, K = 5: 25 tokens x 5 beams leave no clip of 0..99 above 0.006 there; clip 6
# has the widest gap over the engine's own logits in both types (0.0031 f16, 0.0024 bf16; MIN_GAP is asserted below).
CLIPS_K5 = (79, 77)
CLIPS_K3 = (24, 23)
CLIP_EOT = 6
MIN_GAP = 1e-3

_CTX = {}


def get_ctx(wrs, shape, dtype, **kw):
    key = (shape, dtype, tuple(sorted(kw.items())))
    if key not in _CTX:
        _CTX[key] = wrs.WhisperContext(model_path(shape), dtype=getattr(wrs, dtype), **kw)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_ctxs():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def beam_params(wrs, K, no_timestamps=False, max_tokens=12):
    p = wrs.beam_full_params(K, "en")
    p.temperature_inc = 0.0
    p.single_segment = True
    p.max_tokens = max_tokens
    p.no_timestamps = no_timestamps
    return p


class EngineLogits:
    """logits_fn of beam_ref over the engine's raw logits: one forced call per step for all live prefixes."""

    def __init__(self, wrs, ctx, pcm, K, no_timestamps, max_tokens):
        self.wrs, self.ctx, self.pcm, self.K = wrs, ctx, pcm, K
        self.V = wrs.lib().whisper_n_vocab(ctx.ptr)
        self.p = wrs.reference_full_params("en")
        self.p.temperature_inc = 0.0
        self.p.single_segment = True
        self.p.max_tokens = max_tokens
        self.p.no_timestamps = no_timestamps
        self.st = ctx.create_state()
        self.cache = {}

    def prefetch(self, prefixes):
        need = [p for p in prefixes if p not in self.cache]
        if not need:
            return
        i = len(need[0])
        assert all(len(p) == i for p in need) and len(need) <= self.K
        rows = (need + [need[0]] * self.K)[:self.K]
        forced = np.zeros((self.K, i + 1), np.int32)
        for j, p in enumerate(rows):
            forced[j, :i] = p
        old = {k: os.environ.get(k) for k in ("WHISPER_MI355X_PDEC", "WHISPER_MI355X_SMALLM")}
        os.environ["WHISPER_MI355X_PDEC"] = "0"
        os.environ["WHISPER_MI355X_SMALLM"] = "0"
        try:
            rc, out = self.st.full_batch_forced(self.p, [self.pcm] * self.K, i + 1, forced, list(range(self.K)), self.V)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        assert rc == 0
        for j, p in enumerate(rows):
            self.cache[p] = out[i, j].copy()

    def __call__(self, prefix):
        self.prefetch([prefix])
        return self.cache[prefix]

    def close(self):
        self.st.close()


_REF = {}


def reference(wrs, ctx, key, clip, K, no_timestamps=False, max_tokens=12):
    """beam_ref over the engine's logits for one clip (computed once per (model, dtype, clip, K))."""
    k = (key, clip, K, no_timestamps, max_tokens)
    if k not in _REF:
        pcm = synthetic_pcm(clip)
        src = EngineLogits(wrs, ctx, pcm, K, no_timestamps, max_tokens)
        V = src.V
        vid = br.vocab_ids(V, SPACE)
        n_org = 1 + (len(pcm) + 200 - 400) // 160
        P = br.Params(K=K, max_tokens=max_tokens, single_segment=True, no_timestamps=no_timestamps, seek_end=n_org)
        _REF[k] = br.beam_search(src, P, vid, n_prompt=4 if no_timestamps else 3)
        src.close()
    return _REF[k]


def check_job(st, job, ref, segs):
    info = st.beam_info(job)
    assert len(info) == len(ref.beams)
    for b, (got, want) in enumerate(zip(info, ref.beams)):
        assert got["tokens"] == want["tokens"], f"beam {b}"
        assert (got["completed"], got["failed"], got["winner"]) == (want["completed"], want["failed"], want["winner"]), f"beam {b}"
        tol = PLOG_BAR * max(1, len(want["tokens"]))
        assert abs(got["sum_logprobs_all"] - want["sum_logprobs_all"]) <= tol, (b, got["sum_logprobs_all"], want["sum_logprobs_all"])
    if ref.winner >= 0:
        assert len(segs) == 1 and [t[0] for t in segs[0].tokens] == ref.tokens
    else:
        assert segs == []
    d = st.decisions(job)[0]
    assert (d["temp_idx"], d["failed0"], d["result_len0"]) == (0, int(ref.failed0), ref.result_len)
    if ref.result_len:
        assert d["avg_logprob0"] == pytest.approx(ref.avg_logprobs, abs=1e-4)


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
@pytest.mark.parametrize("clip", CLIPS_K5)
def test_beam5_exact(wrs, dtype, clip):
    ctx = get_ctx(wrs, "tiny+conf", dtype)
    ref = reference(wrs, ctx, ("tiny+conf", dtype), clip, 5)
    print(f"clip {clip} {dtype}: min gap {ref.min_gap():.4f}, copies {sum(len(c) for c in ref.copies)}, winner {ref.winner}")
    assert ref.min_gap() > MIN_GAP, sorted(ref.gaps, key=lambda g: g[1])[:3]
    st = ctx.create_state()
    assert st.full(beam_params(wrs, 5), synthetic_pcm(clip)) == 0
    check_job(st, 0, ref, st.segments())
    st.close()


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_beam3_batch_equals_single(wrs, dtype):
    ctx = get_ctx(wrs, "tiny+conf", dtype)
    refs = [reference(wrs, ctx, ("tiny+conf", dtype), clip, 3) for clip in CLIPS_K3]
    for clip, ref in zip(CLIPS_K3, refs):
        print(f"clip {clip} {dtype}: min gap {ref.min_gap():.4f}, copies {sum(len(c) for c in ref.copies)}")
        assert ref.min_gap() > MIN_GAP, sorted(ref.gaps, key=lambda g: g[1])[:3]
    st = ctx.create_state()
    assert st.full_batch(beam_params(wrs, 3), [synthetic_pcm(c) for c in CLIPS_K3]) == 0
    batch = [st.beam_info(j) for j in range(len(CLIPS_K3))]
    for j, ref in enumerate(refs):
        check_job(st, j, ref, st.batch_segments(j))
    st.close()
    for j, clip in enumerate(CLIPS_K3):  # and the single-clip calls give the batch's beams
        st = ctx.create_state()
        assert st.full(beam_params(wrs, 3), synthetic_pcm(clip)) == 0
        single = st.beam_info(0)
        st.close()
        assert single == batch[j]


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_beam5_eot_no_timestamps(wrs, dtype):
    """tiny+conf+eot without timestamps, max_tokens 24 (25 tokens per beam, about 45 self-cache copies). On the synthetic
    clips no beam takes EOT within 24 tokens (nor within 64) with this model's EOT boost, so the beams end together;
    test_beam5_rows_shrink below is the case whose beams end at different steps."""
    ctx = get_ctx(wrs, "tiny+conf+eot", dtype)
    ref = reference(wrs, ctx, ("tiny+conf+eot", dtype), CLIP_EOT, 5, no_timestamps=True, max_tokens=24)
    lens = [len(b["tokens"]) for b in ref.beams]
    print(f"{dtype}: min gap {ref.min_gap():.4f}, lengths {lens}, copies {sum(len(c) for c in ref.copies)}")
    assert ref.min_gap() > MIN_GAP, sorted(ref.gaps, key=lambda g: g[1])[:3]
    st = ctx.create_state()
    assert st.full(beam_params(wrs, 5, no_timestamps=True, max_tokens=24), synthetic_pcm(CLIP_EOT)) == 0
    check_job(st, 0, ref, st.segments())
    st.close()


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_beam5_rows_shrink(wrs, dtype):
    """tiny+conf+eot23 (tools/make_model.py: the EOT row boosted to 23, so EOT is often among a beam's best candidates),
    no timestamps, K = 5, clip 0 (smallest deciding gap 0.075 nats over the oracle's logits): three beams take EOT at
    step 1 and two go on to step 5. The later steps have two rows (beams 2 and 3: row r is not beam r), the completed
    beams keep their self slots while the live ones are re-parented, and the step graph and logits form are those of
    the smaller row count."""
    ctx = get_ctx(wrs, "tiny+conf+eot23", dtype)
    ref = reference(wrs, ctx, ("tiny+conf+eot23", dtype), 0, 5, no_timestamps=True, max_tokens=24)
    lens = [len(b["tokens"]) for b in ref.beams]
    print(f"{dtype}: min gap {ref.min_gap():.4f}, lengths {lens}, copies {sum(len(c) for c in ref.copies)}, winner {ref.winner}")
    assert ref.min_gap() > MIN_GAP, sorted(ref.gaps, key=lambda g: g[1])[:3]
    assert len(set(lens)) > 1, "the beams of this case must end at different steps"
    assert any(len(step) < 5 for step in ref.picks[1:]), "no step with fewer rows than beams"
    st = ctx.create_state()
    assert st.full(beam_params(wrs, 5, no_timestamps=True, max_tokens=24), synthetic_pcm(0)) == 0
    check_job(st, 0, ref, st.segments())
    st.close()


def test_k1_batch_is_greedy_batch(wrs):
    """beam_size 1 over several clips (no row limit applies): the greedy batch's segments and decisions, bit for bit."""
    ctx = get_ctx(wrs, "tiny+conf", "F16")
    pcm = [synthetic_pcm(c) for c in (2, 3, 4)]
    out = []
    for p in (wrs.reference_full_params("en"), wrs.beam_full_params(1, "en")):
        st = ctx.create_state()
        assert st.full_batch(p, pcm) == 0
        out.append([([(s.t0, s.t1, s.text, s.tokens) for s in st.batch_segments(j)], st.decisions(j)) for j in range(3)])
        st.close()
    assert all(job[0] for job in out[0]) and out[1] == out[0]


def test_six_clips_five_beams(wrs):
    """The documented limit: 6 clips x 5 beams run (30 rows), 7 x 5 is refused with -1 and the state stays usable."""
    ctx = get_ctx(wrs, "tiny+conf", "F16")
    st = ctx.create_state()
    pcm = [synthetic_pcm(c) for c in range(6)]
    assert st.full_batch(beam_params(wrs, 5), pcm) == 0
    for j in range(6):
        info = st.beam_info(j)
        assert len(info) == 5 and sum(b["winner"] for b in info) == 1
    # the 30-row steps take the 256-thread cross-attention kernel, a single clip's 5 rows the 1024-thread one
    # (attn.hip picks by the step's rows): the same beams; the sums of 13 f16 log-probabilities differ by the
    # kernels' rounding (3.5e-3 measured; f16 logits move by up to ~1e-2 between kernel forms)
    for got, want in zip(st.beam_info(0), _single_info(wrs, ctx, 0)):
        assert {k: v for k, v in got.items() if k != "sum_logprobs_all"} == {k: v for k, v in want.items() if k != "sum_logprobs_all"}
        assert got["sum_logprobs_all"] == pytest.approx(want["sum_logprobs_all"], abs=5e-2)
    assert st.full_batch(beam_params(wrs, 5), pcm + [synthetic_pcm(6)]) == -1
    assert st.full_batch(beam_params(wrs, 5), pcm[:1]) == 0
    st.close()


def _single_info(wrs, ctx, clip):
    st = ctx.create_state()
    assert st.full(beam_params(wrs, 5), synthetic_pcm(clip)) == 0
    info = st.beam_info(0)
    st.close()
    return info


# ---- K = 1 is greedy ----------------------------------------------------------------------------------------------
def _run(st, params, pcm):
    assert st.full(params, pcm) == 0
    segs = [(s.t0, s.t1, s.text, s.tokens) for s in st.segments()]
    return segs, st.decisions(), st.token_times()


@pytest.mark.parametrize("prompt", [None, "one two three"])
@pytest.mark.parametrize("dtw", [False, True])
def test_k1_is_greedy(wrs, prompt, dtw):
    ctx = get_ctx(wrs, "tiny+conf", "F16", **({"dtw_n_top": 2} if dtw else {}))
    pcm = synthetic_pcm(2)
    st = ctx.create_state()
    greedy = _run(st, wrs.reference_full_params("en", prompt), pcm)
    st.close()
    st = ctx.create_state()
    beam = _run(st, wrs.beam_full_params(1, "en", prompt), pcm)
    info = st.beam_info(0)
    st.close()
    assert greedy[0] and beam[0] == greedy[0]   # t0, t1, text, (id, tid, p, plog) of every token: the same bits
    assert beam[1] == greedy[1]
    assert beam[2] == greedy[2]
    if dtw:
        assert any(t >= 0 for seg in beam[2] for _, t in seg)
    assert len(info) == 1


# ---- edges ----------------------------------------------------------------------------------------------------------
def test_beam_size_9_is_refused(wrs):
    ctx = get_ctx(wrs, "tiny+conf", "F16")
    pcm = synthetic_pcm(2)
    st = ctx.create_state()
    assert st.full(wrs.beam_full_params(9, "en"), pcm) == -4
    after = _run(st, wrs.reference_full_params("en"), pcm)
    st.close()
    st = ctx.create_state()
    fresh = _run(st, wrs.reference_full_params("en"), pcm)
    st.close()
    assert after == fresh and fresh[0]


def test_forced_fallback_equals_greedy(wrs):
    """entropy_thold so high that every beam fails at t = 0: the sampled attempts that follow are the greedy strategy's.
    (The entropy rule applies to sequences of more than 32 tokens, as in greedy decoding: 41 tokens without timestamps.)"""
    ctx = get_ctx(wrs, "tiny+conf", "F16")
    pcm = synthetic_pcm(2)
    out = []
    for p in (wrs.beam_full_params(3, "en"), wrs.reference_full_params("en")):
        p.entropy_thold = 1e9
        p.temperature_inc = 0.2
        p.no_timestamps = True
        p.max_tokens = 40
        st = ctx.create_state()
        out.append(_run(st, p, pcm))
        if p.strategy == wrs.BEAM_SEARCH:
            info = st.beam_info(0)
            assert len(info) == 3 and all(b["failed"] and not b["winner"] for b in info)
        st.close()
    assert out[0][1] and all(d["failed0"] == 1 and d["temp_idx"] >= 1 for d in out[0][1])
    assert [(d["seek"], d["temp_idx"], d["no_speech"]) for d in out[0][1]] == [(d["seek"], d["temp_idx"], d["no_speech"]) for d in out[1][1]]
    assert out[0][0] == out[1][0]


def test_recycled_state_after_beam(wrs):
    ctx = get_ctx(wrs, "tiny+conf", "F16")
    pcm = synthetic_pcm(2)
    st = ctx.create_state()
    fresh = _run(st, wrs.reference_full_params("en"), pcm)
    st.close()
    st = ctx.create_state()
    assert st.full(beam_params(wrs, 5), pcm) == 0
    st.close()
    st = ctx.create_state()
    assert st.info()["pooled"]
    assert st.beam_info(0) == []
    again = _run(st, wrs.reference_full_params("en"), pcm)
    st.close()
    assert again == fresh
