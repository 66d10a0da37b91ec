"""Token-level timestamps from cross-attention DTW on the device (kernels/align.hip, engine.cpp align_windows;
DESIGN.md "Token timestamps (DTW)").

Kernels against numpy (tests/dtw_ref.py): the score and cost kernels against float64 within a recorded bar that
must also discriminate (a wrong head / an omitted median filter differs by >= 10x the bar); the DTW kernel
exactly (first frames and the whole path equal the sequential float32 loop).

Whole runs (tiny+conf, language en, the reference's FullParams): the engine's cost matrix of a job's last
aligned window against a float64 decoder forward built from the oracle's tensors over the oracle's encoder
output; t_dtw of every text token of that window == the float32 numpy DTW of the engine's own cost matrix + seek.

Bars (measured max |difference| x 4, rounded up to one digit; figures in DESIGN.md):
  SCORE_BAR  softmaxed score rows, f32 kernel against float64 on identical f16 / bf16 inputs
  COST_BAR   cost matrix, f32 kernels against float64 on identical f32 inputs
  RUN_BAR    whole-run cost matrix against the independent float64 reference, per compute type
"""
import ctypes as C

import numpy as np
import pytest

from conftest import model_path
from dtw_ref import DecoderRef, cost_matrix, dtw_f32
from make_model import synthetic_pcm
from oracle_py import shared_oracle

pytestmark = pytest.mark.gpu

T_CTX, D, H, L = 1500, 384, 6, 4   # the tiny shape
# measured on an MI355X over this file's cases -> x 4, rounded up to one digit:
SCORE_BAR = 2e-6   # 4.60e-7 (f16 inputs), 3.83e-7 (bf16 inputs); a shifted head differs by >= 0.29
COST_BAR = 2e-6    # 4.37e-7; the unfiltered reference differs by 5.2
# largest of the whole-run cases: f16 3.41e-3 (custom heads; 1.6e-3 .. 3.0e-3 elsewhere), bf16 1.87e-2 (the
# bf16 encoder and cross K against the oracle's f16 numerics); a wrong head list differs by 0.64 .. 2.9
RUN_BAR = {"f16": 2e-2, "bf16": 8e-2}
TINY_HEADS = [(2, 2), (3, 0), (3, 2), (3, 3), (3, 4), (3, 5)]


def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return b, (b.astype(np.uint32) << 16).view(np.float32)


def _to_t(x, bf):
    if bf:
        return _bf16(x)
    h = np.ascontiguousarray(x, np.float32).astype(np.float16)
    return h.view(np.uint16), h.astype(np.float32)


def _ints(a):
    return np.ascontiguousarray(a, np.int32)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class Dev:
    """device buffers of one context, freed together"""

    def __init__(self, wrs, ctx):
        self.L, self.ctx, self.ptrs = wrs.lib(), ctx, []

    def up(self, a):
        p = self.alloc(a.nbytes)
        assert self.L.whisper_mi355x_memcpy(self.ctx.ptr, C.c_void_p(p), a.ctypes.data, a.nbytes, 1) == 0
        return p

    def alloc(self, nbytes):
        p = self.L.whisper_mi355x_dev_alloc(self.ctx.ptr, max(16, nbytes))
        assert p
        self.ptrs.append(p)
        return p

    def down(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        assert self.L.whisper_mi355x_memcpy(self.ctx.ptr, out.ctypes.data, C.c_void_p(p), out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.L.whisper_mi355x_dev_free(self.ctx.ptr, C.c_void_p(p))
        self.ptrs = []


@pytest.fixture(scope="module")
def kctx(wrs):
    c = {"f16": wrs.WhisperContext(model_path("tiny"), dtype=wrs.F16),
         "bf16": wrs.WhisperContext(model_path("tiny"), dtype=wrs.BF16)}
    yield c
    for x in c.values():
        x.close()


# ---- kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_scores_kernel(wrs, kctx, dtype):
    """two clips per launch at non-identity slots, rows from {1, 5, 65, 224}; the head list repeats a layer and
    holds head 0 and head H - 1"""
    bf = dtype == "bf16"
    ctx = kctx[dtype]
    heads = [(1, 0), (3, H - 1), (1, H - 1), (2, 3)]
    n_slots = 4
    rng = np.random.default_rng(17 + bf)
    K_b, K = _to_t(rng.standard_normal((n_slots, L, H, T_CTX, 64), dtype=np.float32), bf)
    cache = np.zeros((n_slots, L, 2, H, T_CTX, 64), np.uint16)
    cache[:, :, 0] = K_b
    worst, least_wrong = 0.0, np.inf
    for rows, frames, slots in (((1, 224), (1500, 37), (2, 0)), ((65, 5), (155, 1), (3, 1))):
        tot = sum(rows)
        q_b, q = _to_t(0.5 * rng.standard_normal((L, tot, D), dtype=np.float32), bf)
        dev = Dev(wrs, ctx)
        n_p = sum(len(heads) * n * f for n, f in zip(rows, frames))
        dP = dev.alloc(n_p * 4)
        rc = dev.L.whisper_mi355x_debug_align_scores(
            ctx.ptr, dev.up(q_b), dev.up(cache), n_slots, 2, _ip(_ints(slots)), _ip(_ints(rows)), _ip(_ints(frames)),
            len(heads), _ip(_ints([l for l, _ in heads])), _ip(_ints([h for _, h in heads])), dP)
        assert rc == 0
        got = dev.down(dP, (n_p,), np.float32)
        dev.free()
        assert np.isfinite(got).all()
        off = row0 = 0
        for n, F, sl in zip(rows, frames, slots):
            g = got[off:off + len(heads) * n * F].reshape(len(heads), n, F)
            off += g.size
            for a, (l, h) in enumerate(heads):
                def ref(hh):
                    s = q[l, row0:row0 + n, hh * 64:(hh + 1) * 64].astype(np.float64) @ K[sl, l, hh].astype(np.float64).T
                    e = np.exp(s - s.max(-1, keepdims=True))
                    return (e / e.sum(-1, keepdims=True))[:, :F]
                worst = max(worst, np.abs(g[a] - ref(h)).max())
                if F >= 37:  # every head of every clip with frames to compare: a head index shifted by one
                    least_wrong = min(least_wrong, np.abs(g[a] - ref((h + 1) % H)).max())
            row0 += n
    print(f"scores {dtype}: max |P - P64| = {worst:.3e}; least difference to a shifted head = {least_wrong:.3e}")
    assert worst <= SCORE_BAR, worst
    assert least_wrong >= 10 * SCORE_BAR, least_wrong


def test_cost_kernel(wrs, kctx):
    """A in {1, 6, 24} heads, N_all in {4, 70, 224} rows, F in {1, 3, 5, 37, 1500} frames: every pair as one clip
    of a launch"""
    ctx = kctx["f16"]
    rng = np.random.default_rng(23)
    worst, least_wrong = 0.0, 0.0
    for A in (1, 6, 24):
        shapes = [(n, F) for n in (4, 70, 224) for F in (1, 3, 5, 37, 1500)]
        n_sot = [1 + (k & 1) for k in range(len(shapes))]
        Ps = []
        for n, F in shapes:
            p = rng.random((A, n, F)) ** 4
            Ps.append((p * (0.9 / p.sum(-1).max())).astype(np.float32))  # positive, rows sum to <= 0.9
        dev = Dev(wrs, ctx)
        n_cost = sum((n - s - 1) * F for (n, F), s in zip(shapes, n_sot))
        dC = dev.alloc(n_cost * 4)
        rc = dev.L.whisper_mi355x_debug_align_cost(
            ctx.ptr, dev.up(np.concatenate([p.ravel() for p in Ps])), len(shapes), _ip(_ints([n for n, _ in shapes])),
            _ip(_ints(n_sot)), _ip(_ints([F for _, F in shapes])), A, dC)
        assert rc == 0
        got = dev.down(dC, (n_cost,), np.float32)
        dev.free()
        assert np.isfinite(got).all()
        off = 0
        for (n, F), s, p in zip(shapes, n_sot, Ps):
            g = got[off:off + (n - s - 1) * F].reshape(n - s - 1, F)
            off += g.size
            worst = max(worst, np.abs(g - cost_matrix(p, s)).max())
            if F >= 37:
                least_wrong = max(least_wrong, np.abs(g - cost_matrix(p, s, median=False)).max())
    print(f"cost: max |cost - cost64| = {worst:.3e}; difference to the unfiltered reference = {least_wrong:.3e}")
    assert worst <= COST_BAR, worst
    assert least_wrong >= 10 * COST_BAR, least_wrong


def test_dtw_kernel_exact(wrs, kctx):
    """(N, F) of (2, 1), (2, 5), (9, 3), (70, 37), (221, 1500) in one launch; the (70, 37) clip has costs from
    {-1, 0, 1} (exact sums: the tie rule decides). First frames and the whole path == the float32 numpy loop."""
    ctx = kctx["f16"]
    rng = np.random.default_rng(31)
    shapes = [(2, 1), (2, 5), (9, 3), (70, 37), (221, 1500)]
    costs = [rng.integers(-1, 2, s).astype(np.float32) if s == (70, 37) else rng.standard_normal(s).astype(np.float32)
             for s in shapes]
    dev = Dev(wrs, ctx)
    n_fr = sum(n for n, _ in shapes)
    n_path = sum(n + f for n, f in shapes)
    fr = np.full(n_fr, -7, np.int32)
    path = np.full((n_path, 2), -7, np.int32)
    plen = np.zeros(len(shapes), np.int32)
    rc = dev.L.whisper_mi355x_debug_align_dtw(ctx.ptr, dev.up(np.concatenate([c.ravel() for c in costs])), len(shapes),
                                              _ip(_ints([n for n, _ in shapes])), _ip(_ints([f for _, f in shapes])),
                                              _ip(fr), _ip(path), _ip(plen))
    dev.free()
    assert rc == 0
    o_fr = o_path = 0
    for k, ((n, f), c) in enumerate(zip(shapes, costs)):
        want_fr, want_path, _ = dtw_f32(c)
        assert fr[o_fr:o_fr + n].tolist() == want_fr.tolist(), (n, f)
        assert plen[k] == len(want_path), (n, f)
        assert [tuple(x) for x in path[o_path:o_path + plen[k]].tolist()] == want_path, (n, f)
        o_fr += n
        o_path += n + f
    assert len({x for x in fr[n_fr - 221:].tolist()}) > 50  # the long clip's rows spread over the frames


# ---- whole runs ---------------------------------------------------------------------------------------------
def clip(seed, seconds):
    return synthetic_pcm(seed, seconds=seconds)


_ENC = {}


def oracle_enc(path, pcm_key, pcm, seek):
    """Oracle.encode of one window (shared by the cases that align the same window)"""
    key = (path, pcm_key, seek)
    if key not in _ENC:
        o = shared_oracle(path)
        o.new_state()
        o.mel(pcm)
        _ENC[key] = o.encode(seek).astype(np.float64)
    return _ENC[key]


def job_windows(st, job, eot):
    """per window of the job (by the decisions' seeks): (seek, [(id, t_dtw) of its tokens])"""
    seeks = [d["seek"] for d in st.decisions(job)]
    segs = st.batch_segments(job)
    times = st.token_times(job)
    out = [(s, []) for s in seeks]
    w = 0
    for sg, tt in zip(segs, times):
        assert [t[0] for t in sg.tokens] == [t[0] for t in tt]
        # segments come in window order; one that starts at the next window's seek and reaches past it is that
        # window's (an empty segment at the boundary closes the earlier window: sampled fallback attempts end so)
        while w + 1 < len(seeks) and sg.t0 >= seeks[w + 1] and sg.t1 > seeks[w + 1]:
            w += 1
        out[w][1].extend(tt)
    return out


def check_job(wrs, st, job, path, pcm_key, pcm, heads, dtype, figures, wrong_heads=None):
    """the exact and the reference checks of one job's last aligned window; the range checks of every window"""
    o = shared_oracle(path)
    eot, sot, not_, beg = o.token("eot"), o.token("sot"), o.token("not"), o.token("beg")
    wins = job_windows(st, job, eot)
    n_len_org = 1 + (len(pcm) + 200 - 400) // 160
    last = None
    for seek, toks in wins:
        text = [(i, t) for i, t in toks if i < eot]
        assert all(t == -1 for i, t in toks if i >= eot), "timestamp / special tokens carry no t_dtw"
        if not text:
            continue
        F_max = min(3000, n_len_org - seek) // 2
        ts = [t for _, t in text]
        assert all(seek <= t < seek + 2 * F_max for t in ts), (seek, F_max, ts)
        assert all(b >= a for a, b in zip(ts, ts[1:])), ts
        assert all((t - seek) % 2 == 0 for t in ts)
        last = (seek, text)
    assert last is not None
    seek, text = last
    cost = st.align_cost(job)
    assert cost is not None and cost.shape[0] == len(text) + 1
    N, F = cost.shape
    assert 1 <= F <= min(3000, n_len_org - seek) // 2
    fr, _, _ = dtw_f32(cost)
    assert [t for _, t in text] == [seek + 2 * int(f) for f in fr[1:]], "t_dtw == numpy f32 DTW of the engine's cost + seek"
    # the independent float64 reference over the engine's own alignment token sequence
    seq = [sot, sot + 1, not_] + [i for i, _ in text] + [eot]  # language en = sot + 1 + 0; n_sot = 2
    dec = DecoderRef(o)
    enc = oracle_enc(path, pcm_key, pcm, seek)
    ref = dec.cost(seq, enc, heads, 2, F)
    diff = np.abs(cost - ref).max()
    figures.append((dtype, diff))
    print(f"run {dtype} job {job} seek {seek} N {N} F {F}: max |cost - ref| = {diff:.3e}")
    assert diff <= RUN_BAR[dtype], diff
    if wrong_heads is not None:
        wrong = np.abs(cost - dec.cost(seq, enc, wrong_heads, 2, F)).max()
        print(f"   difference to the reference with a wrong head list = {wrong:.3e}")
        assert wrong >= 10 * RUN_BAR[dtype], wrong
    return N, F


FIG = []


def run_single(wrs, shape, dtype, pcm_key, pcm, heads, **kw):
    path = model_path(shape)
    ctx = wrs.WhisperContext(path, dtype=wrs.BF16 if dtype == "bf16" else wrs.F16, **kw)
    st = ctx.create_state()
    assert st.full(wrs.reference_full_params("en"), pcm) == 0
    assert st.align_ms() > 0
    shifted = [(l, (h + 1) % H) for l, h in heads]  # a wrong head list: every head index shifted by one,
    if set(shifted) == set(heads):                  # or, where that is the same set, every layer
        shifted = [((l + L - 1) % L, h) for l, h in heads]
    out = check_job(wrs, st, 0, path, pcm_key, pcm, heads, dtype, FIG, wrong_heads=shifted)
    windows = len(st.decisions(0))
    st.close()
    ctx.close()
    return out, windows


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_full_30s(wrs, dtype):
    """one 30 s clip through whisper_full_with_state, preset TINY"""
    run_single(wrs, "tiny+conf", dtype, ("clip", 0, 30.0), clip(0, 30.0), TINY_HEADS, dtw_preset="TINY")


def test_full_short_clip(wrs):
    """3.1 s: a small F"""
    (N, F), _ = run_single(wrs, "tiny+conf", "f16", ("clip", 1, 3.1), clip(1, 3.1), TINY_HEADS, dtw_preset="TINY")
    assert F <= 155


def test_full_two_windows(wrs):
    """45 s: two windows, the aligned last one has seek > 0"""
    path = model_path("tiny+conf")
    pcm = clip(2, 45.0)
    ctx = wrs.WhisperContext(path, dtw_preset="TINY")
    st = ctx.create_state()
    assert st.full(wrs.reference_full_params("en"), pcm) == 0
    seeks = [d["seek"] for d in st.decisions(0)]
    assert len(seeks) >= 2 and seeks[-1] > 0
    check_job(wrs, st, 0, path, ("clip", 2, 45.0), pcm, TINY_HEADS, "f16", FIG)
    st.close()
    ctx.close()


def seg_full(segs):
    return [([tuple(t) for t in s.tokens], s.t0, s.t1, s.text) for s in segs]


def test_batch_of_three_and_off_means_off(wrs):
    """a 3-clip full_batch of unequal lengths; with DTW off the segments, tokens and p / plog are the same bits,
    align_ms is 0 and every t_dtw is -1"""
    path = model_path("tiny+conf")
    clips = [clip(3, 30.0), clip(4, 12.5), clip(5, 21.0)]
    keys = [("clip", 3, 30.0), ("clip", 4, 12.5), ("clip", 5, 21.0)]
    p = wrs.reference_full_params("en")
    ctx = wrs.WhisperContext(path, dtw_preset="TINY")
    st = ctx.create_state()
    assert st.full_batch(p, clips) == 0
    on = [seg_full(st.batch_segments(j)) for j in range(3)]
    assert st.align_ms() > 0
    for j in range(3):
        check_job(wrs, st, j, path, keys[j], clips[j], TINY_HEADS, "f16", FIG)
    st.close()
    ctx.close()
    ctx = wrs.WhisperContext(path)
    st = ctx.create_state()
    assert st.full_batch(p, clips) == 0
    assert [seg_full(st.batch_segments(j)) for j in range(3)] == on
    assert st.align_ms() == 0
    for j in range(3):
        assert all(t == -1 for seg in st.token_times(j) for _, t in seg)
        assert st.align_cost(j) is None
    st.close()
    ctx.close()


def test_batch_of_34_direct_form(wrs):
    """34 clips: the direct cross form, whose aligned clips get their cross K/V on demand; clips 0 and 33"""
    path = model_path("tiny+conf")
    secs = [30.0 - 0.5 * (k % 5) for k in range(34)]
    clips = [clip(k % 20, secs[k]) for k in range(34)]
    ctx = wrs.WhisperContext(path, dtw_preset="TINY")
    st = ctx.create_state()
    assert st.full_batch(wrs.reference_full_params("en"), clips) == 0
    info = (C.c_int * 5)()
    assert wrs.lib().whisper_mi355x_state_info(st.ptr, info) == 5 and info[0] == 1
    for j in (0, 33):
        check_job(wrs, st, j, path, ("clip", j % 20, secs[j]), clips[j], TINY_HEADS, "f16", FIG)
    st.close()
    ctx.close()


def test_quantized_file(wrs):
    run_single(wrs, "tiny+conf+q5_0", "f16", ("clip", 0, 30.0), clip(0, 30.0), TINY_HEADS, dtw_preset="TINY")


def test_n_top_most(wrs):
    heads = [(l, h) for l in (2, 3) for h in range(H)]
    run_single(wrs, "tiny+conf", "f16", ("clip", 0, 30.0), clip(0, 30.0), heads, dtw_n_top=2)


def test_custom_heads(wrs):
    heads = [(1, 0), (3, 5), (2, 2)]
    run_single(wrs, "tiny+conf", "f16", ("clip", 0, 30.0), clip(0, 30.0), heads, dtw_heads=heads)


@pytest.mark.parametrize("kw", [dict(dtw_preset="NONE"), dict(dtw_n_top=0), dict(dtw_n_top=5), dict(dtw_heads=[(4, 0)]),
                                dict(dtw_heads=[(0, 6)]), dict(dtw_preset="LARGE_V3"), dict(dtw_heads=[])])
def test_bad_configurations_return_null(wrs, kw):
    with pytest.raises(RuntimeError):
        wrs.WhisperContext(model_path("tiny+conf"), **kw)
