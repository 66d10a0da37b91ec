"""token_timestamps / max_len / split_on_word on the device and through whisper.h (kernels/tokts.hip,
csrc/token_times.cpp, engine.cpp token_time_windows) against tests/tokts_ref.py.

Kernels: the energy kernel equals the reference bit for bit; the adjust kernel equals it exactly (integers) on
hand-built energy signals. (Its threshold sums in f64 in another order than numpy: the f32 threshold can differ only by
a double-rounding coincidence, about 1e-6 per token, and then only matters if a sample lies between the two values.)

Whole runs (tiny+conf, language en, the reference app's FullParams): exact, no token excluded. The yardstick is the
reference fed the engine's own tokens (id, tid, pt, ptsum) and segment times from the same inputs with
token_timestamps = false, plus the PCM."""
import ctypes as C

import numpy as np
import pytest

import tokts_ref as tr
from conftest import model_path
from make_model import synthetic_pcm

pytestmark = pytest.mark.gpu

T = 1024      # kEnergyTile (kernels.h): samples per workgroup of the energy kernel
CHUNK = 256   # kVadChunk: samples per round of the adjust kernel's walks


@pytest.fixture(scope="module")
def kctx(wrs):
    c = wrs.WhisperContext(model_path("tiny+conf"))
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- energy kernel ----------------------------------------------------------------------------------------------
def check_energy(kctx, clips):
    got = kctx.debug_signal_energy(clips)
    assert isinstance(got, list), got
    for x, g in zip(clips, got):
        ref = tr.energy(x)
        assert g.shape == ref.shape
        bad = np.nonzero(bits(g) != bits(ref))[0]
        assert bad.size == 0, (len(x), bad[:8], g[bad[:8]], ref[bad[:8]])


def test_energy_tile_edges(kctx):
    rng = np.random.default_rng(5)
    lens = [1, 32, 33, 65, 66, T - 1, T, T + 1, 2 * T + 33]
    check_energy(kctx, [(rng.standard_normal(n) * 0.3).astype(np.float32) for n in lens])


def test_energy_three_clips_and_silence(kctx):
    rng = np.random.default_rng(6)
    clips = [synthetic_pcm(0, 1.3), (rng.standard_normal(5000) * 1e-3).astype(np.float32),
             np.zeros(3 * T + 7, np.float32), (rng.random(777) * 4 - 2).astype(np.float32)]
    check_energy(kctx, clips)


# ---- adjust kernel ----------------------------------------------------------------------------------------------
def check_vad(kctx, energies, segs):
    got = kctx.debug_token_vad(energies, segs)
    assert isinstance(got, list), got
    ref = [tr.vad(energies[c], toks) for c, toks in segs]
    assert got == ref
    return got


def rand_spans(rng, n, t_max, p_special=0.15):
    cuts = np.sort(rng.integers(0, t_max + 1, n + 1))
    return [(int(cuts[i]), int(cuts[i + 1]), int(rng.random() >= p_special)) for i in range(n)]


def box(N=1600, a=320, b=960):
    e = np.zeros(N, np.float32)
    e[a:b] = 1.0
    return e


@pytest.mark.parametrize("N", [1, 2000, 4001])
def test_vad_small_clips(kctx, N):
    rng = np.random.default_rng(N)
    e = (rng.random(N) ** 3).astype(np.float32)
    t_max = N // 160 + 2
    check_vad(kctx, [e], [(0, rand_spans(rng, n, t_max)) for n in (2, 3, 7)])


def test_vad_silence_moves_nothing(kctx):
    spans = [(0, 3, 1), (3, 3, 1), (3, 9, 1)]
    assert check_vad(kctx, [np.zeros(1600, np.float32)], [(0, spans)]) == [[(a, b) for a, b, _ in spans]]


def test_vad_walks_to_both_ends(kctx):
    """a loud clip with one quiet sample: the walks stop only at k = 0, at the quiet sample and at k = N - 1"""
    N = 50000
    e = np.ones(N, np.float32)
    e[25000] = 0.0
    got = check_vad(kctx, [e], [(0, [(0, 10, 1), (20, 30, 1)]), (0, [(170, 180, 1), (200, 250, 1)])])
    # token 0's end walks up to the quiet sample and is clamped to the next t0 = 20; token 1 walks down to k = 0
    # (clamped to that t1) and up to the quiet sample
    assert got[0] == [(0, 20), (20, 25000 // 160)]
    # second segment: token 0's end walks up to k = N - 1 (clamped to 200); token 1 walks down to the quiet sample
    # (clamped) and up to k = N - 1
    assert got[1] == [(170, 200), (200, (N - 1) // 160)]


@pytest.mark.parametrize("d", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_vad_crossing_at_the_chunk_boundary(kctx, d):
    """the walks stop d samples from their start: at, one before and one after a round's last lane, and 3 rounds on"""
    N = 16000
    s0, s1 = 1600 * 3, 1600 * 6  # t = 30, 60
    down = np.zeros(N, np.float32)
    down[s0 - d + 1:s1 - d] = 1.0       # start walks down from s0 to s0 - d; end walks down from s1 to s1 - d - 1
    up = np.zeros(N, np.float32)
    up[s0 + d:s1 + d] = 1.0             # start walks up from s0 to s0 + d; end walks up from s1 to s1 + d
    segs = [(0, [(0, 0, 1), (30, 60, 1)]), (1, [(0, 0, 1), (30, 60, 1)])]
    got = check_vad(kctx, [down, up], segs)
    assert got[0][1] == ((s0 - d) // 160, (s1 - d - 1) // 160)
    assert got[1][1] == ((s0 + d) // 160, (s1 + d) // 160)


def test_vad_clamps_and_first_token(kctx):
    e = box()
    got = check_vad(kctx, [e], [(0, [(0, 5, 1), (5, 10, 1)]), (0, [(4, 5, 1), (7, 8, 1)]), (0, [(0, 1, 1), (3, 5, 1)])])
    assert got[0] == [(2, 5), (5, 5)]   # t1 > next.t0 and t0 < prev.t1, both clamped
    assert got[1][0] == (4, 6)          # j = 0 on a loud start takes the else branch
    assert got[2] == [(1, 1), (1, 6)]


def test_vad_specials_equal_times_and_times_past_the_end(kctx):
    e = box()
    got = check_vad(kctx, [e, np.ones(1, np.float32)], [
        (0, [(0, 5, 1), (5, 5, 0), (5, 10, 1), (10, 10, 0)]),   # a special in the middle and one at the end
        (0, [(3, 3, 1), (3, 3, 1), (4, 4, 1)]),                 # t0 == t1
        (0, [(-1, 99, 1), (99, 120, 1), (5000, 6000, 1)]),      # past the clip end
        (0, [(9, 2, 1), (60, 1, 1)]),                           # t1 < t0
        (1, [(0, 0, 1), (0, 7, 1)])])
    assert got[0] == [(2, 5), (5, 5), (5, 5), (10, 10)]
    assert got[2][:2] == [(2, 5), (9, 9)]


def test_vad_token_spanning_a_whole_clip(kctx):
    N = 480000
    rng = np.random.default_rng(9)
    e = (rng.random(N) ** 2).astype(np.float32)
    e[:700] = 0.0
    e[-900:] = 0.0
    got = check_vad(kctx, [e], [(0, [(0, 3000, 1), (3000, 3000, 0)]), (0, [(0, 0, 0), (0, 2999, 1)])])
    assert got[0][0] == (700 // 160, (N - 901) // 160)


def test_vad_three_clips_six_segments(kctx):
    rng = np.random.default_rng(11)
    energies = [tr.energy(synthetic_pcm(7, 6.0)), (rng.random(33333) ** 4).astype(np.float32), tr.energy(synthetic_pcm(8, 2.5))]
    segs = []
    for c, n in zip([0, 1, 2, 1, 0, 2], [2, 3, 2, 40, 224, 5]):
        segs.append((c, rand_spans(rng, n, len(energies[c]) // 160 + 3)))
    got = check_vad(kctx, energies, segs)
    moved = sum(g != (a, b) for (_, toks), gs in zip(segs, got) for g, (a, b, _) in zip(gs, toks))
    assert moved > 50


def test_bad_arguments(kctx):
    e = box()
    ok = [(0, [(0, 5, 1), (5, 10, 1)])]
    assert isinstance(kctx.debug_token_vad([e], ok), list)
    assert kctx.debug_token_vad([e], [(1, ok[0][1])]) == -1                  # clip index out of range
    assert kctx.debug_token_vad([e], [(-1, ok[0][1])]) == -1
    assert kctx.debug_token_vad([e, e[:0]], ok) == -1                         # n_samples < 1
    assert kctx.debug_token_vad([e], ok + [(0, [(0, 5, 1)])]) == -1           # a segment of fewer than 2 tokens
    assert kctx.debug_token_vad([e], []) == -1
    assert kctx.debug_signal_energy([e, e[:0]]) == -1
    assert kctx.debug_signal_energy([]) == -1


# ---- whole runs -------------------------------------------------------------------------------------------------
def clips():
    return [synthetic_pcm(k) for k in range(4)] + [synthetic_pcm(4, 70.0), synthetic_pcm(5, 1.0)]


_CLIPS = None
_ENERGY = {}


def the_clips():
    global _CLIPS
    if _CLIPS is None:
        _CLIPS = clips()
    return _CLIPS


def clip_energy(k):
    if k not in _ENERGY:
        _ENERGY[k] = tr.energy(the_clips()[k])
    return _ENERGY[k]


def params(wrs, beam=0, **kw):
    p = wrs.beam_full_params(beam) if beam else wrs.reference_full_params("en")
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def seg_full(segs):
    return [([tuple(t) for t in s.tokens], s.t0, s.t1, s.text) for s in segs]


def job_result(st, job):
    """[(t0, t1, text, [token dicts])] of a job"""
    return [(s.t0, s.t1, s.text, d) for s, d in zip(st.batch_segments(job), st.token_data(job))]


def reference_job(ctx, off, energy, p, eot, beg):
    """the reference's token times of a job from its result with token_timestamps off: per segment, token dicts"""
    state = tr.new_state()
    out = []
    for t0, t1, _, toks in off:
        tok = tr.phase1([dict(id=d["id"], tid=d["tid"], pt=d["pt"], ptsum=d["ptsum"]) for d in toks], t0, t1, state, beg,
                        p.thold_pt, p.thold_ptsum, ctx.token_str)
        if len(tok) >= 2 and len(energy) > 0:
            adj = tr.vad(energy, [(t["t0"], t["t1"], t["id"] < eot) for t in tok])
            for t, (a, b) in zip(tok, adj):
                t["t0"], t["t1"] = a, b
        out.append(tok)
    return out


class Run:
    """one context + the batch result with token_timestamps off, per (dtype, beam, dtw)"""
    cache = {}

    def __init__(self, wrs, dtype, beam=0, dtw=False):
        self.wrs = wrs
        kw = dict(dtw_preset="TINY") if dtw else {}
        self.ctx = wrs.WhisperContext(model_path("tiny+conf"), dtype=wrs.BF16 if dtype == "bf16" else wrs.F16, **kw)
        L = wrs.lib()
        self.eot, self.beg = L.whisper_token_eot(self.ctx.ptr), L.whisper_token_beg(self.ctx.ptr)
        self.beam = beam
        self.off = self.batch()
        self.ref = None

    def batch(self, **kw):
        st = self.ctx.create_state()
        assert st.full_batch(params(self.wrs, self.beam, **kw), the_clips()) == 0
        out = [job_result(st, j) for j in range(len(the_clips()))]
        self.ms = st.token_times_ms()
        st.close()
        return out

    def reference(self):
        if self.ref is None:
            p = params(self.wrs)
            self.ref = [reference_job(self.ctx, self.off[j], clip_energy(j), p, self.eot, self.beg) for j in range(len(self.off))]
        return self.ref


@pytest.fixture(scope="module")
def runs(wrs):
    made = {}

    def get(dtype, beam=0, dtw=False):
        key = (dtype, beam, dtw)
        if key not in made:
            made[key] = Run(wrs, dtype, beam, dtw)
        return made[key]

    yield get
    for r in made.values():
        r.ctx.close()


def plain(res):
    """a job's result without the token times"""
    return [(t0, t1, text, [(d["id"], d["tid"], d["p"], d["plog"], d["pt"], d["ptsum"]) for d in toks]) for t0, t1, text, toks in res]


def check_times(run, on):
    ref = run.reference()
    n_tok = n_known = 0
    for j, (res, rj) in enumerate(zip(on, ref)):
        assert plain(res) == plain(run.off[j]), j
        for (_, _, _, toks), rt in zip(res, rj):
            got = [(d["t0"], d["t1"], d["vlen"]) for d in toks]
            want = [(t["t0"], t["t1"], float(t["vlen"])) for t in rt]
            assert got == want, (j, got, want)
            n_tok += len(got)
            n_known += sum(a >= 0 and b >= a for a, b, _ in got)
    assert n_tok > 0 and n_known > n_tok // 2


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_token_times(runs, dtype):
    """(1) max_len = 0: segments, texts, ids, p, plog as without it; every token's (t0, t1, vlen) is the reference's"""
    run = runs(dtype)
    assert len(run.off[4]) > 0 and max(s[1] for s in run.off[4]) > 3000, "the 70 s clip has windows at seek > 0"
    assert run.ms == 0
    assert all(d["t0"] == -1 and d["t1"] == -1 and d["vlen"] == 0 for job in run.off for s in job for d in s[3])
    on = run.batch(token_timestamps=True)
    assert run.ms > 0
    check_times(run, on)


def wrapped_reference(run, max_len, sow):
    out = []
    for rj, off in zip(run.reference(), run.off):
        pieces = []
        for tok, (t0, t1, _, _) in zip(rj, off):
            for p in tr.wrap(tok, t0, t1, max_len, sow, run.eot, run.ctx.token_str):
                pieces.append((p["t0"], p["t1"], p["text"], [(t["id"], t["t0"], t["t1"]) for t in p["tokens"]]))
        out.append(pieces)
    return out


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("sow", [False, True])
@pytest.mark.parametrize("max_len", [1, 8, 20])
def test_wrap(runs, dtype, max_len, sow):
    """(2) texts, t0 / t1 and token lists of the pieces are the reference's wrap; the pieces' texts add up"""
    run = runs(dtype)
    on = run.batch(token_timestamps=True, max_len=max_len, split_on_word=sow)
    got = [[(t0, t1, text, [(d["id"], d["t0"], d["t1"]) for d in toks]) for t0, t1, text, toks in job] for job in on]
    assert got == wrapped_reference(run, max_len, sow)
    for j, job in enumerate(on):
        assert b"".join(s[2] for s in job) == b"".join(s[2] for s in run.off[j])
    assert sum(len(j) for j in on) > sum(len(j) for j in run.off)


def test_single_clip_api_and_callback(wrs, runs):
    """(3) whisper_full_with_state on clip 4 (three windows) equals job 4 of the batch; the callback's n_new add up"""
    run = runs("f16")
    on = run.batch(token_timestamps=True, max_len=8, split_on_word=True)
    st = run.ctx.create_state()
    seen = []
    cb = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)(lambda c, s, n, u: seen.append(n))
    p = params(wrs, token_timestamps=True, max_len=8, split_on_word=True)
    p.new_segment_callback = C.cast(cb, C.c_void_p)
    assert st.full(p, the_clips()[4]) == 0
    assert job_result(st, 0) == on[4]
    L = wrs.lib()
    n_seg = st.full_n_segments()
    assert sum(seen) == n_seg == len(on[4]) and len(seen) >= 2
    d = L.whisper_full_get_token_data_from_state(st.ptr, n_seg - 1, 0)
    assert (d.t0, d.t1, d.vlen) == (on[4][-1][3][0]["t0"], on[4][-1][3][0]["t1"], on[4][-1][3][0]["vlen"])
    st.close()


def test_dtw_times_survive_the_wrap(runs):
    """(4) with dtw_token_timestamps on, every token's t_dtw after wrapping is the one without token_timestamps"""
    run = runs("f16", dtw=True)
    on = run.batch(token_timestamps=True, max_len=8)
    flat = lambda res: [[(d["id"], d["t_dtw"]) for s in job for d in s[3]] for job in res]
    assert flat(on) == flat(run.off)
    assert any(t >= 0 for job in flat(on) for _, t in job)
    assert sum(len(j) for j in on) > sum(len(j) for j in run.off)


def test_beam_search(runs):
    """(5) beam_size = 2: the winner's tokens are placed"""
    run = runs("f16", beam=2)
    check_times(run, run.batch(token_timestamps=True))


def test_recycled_state(wrs, runs):
    """(6) a state from the context's pool starts from t_beg = t_last = tid_last = 0: as a fresh context"""
    run = runs("f16")
    p = params(wrs, token_timestamps=True, max_len=20)
    first = run.ctx.create_state()
    assert first.full(p, the_clips()[4]) == 0
    a = job_result(first, 0)
    first.close()
    again = run.ctx.create_state()
    assert again.info()["pooled"]
    assert again.token_times_ms() == 0
    assert again.full(p, the_clips()[1]) == 0
    b = job_result(again, 0)
    again.close()
    fresh = wrs.WhisperContext(model_path("tiny+conf"))
    st = fresh.create_state()
    assert st.full(p, the_clips()[1]) == 0
    assert job_result(st, 0) == b
    assert st.full(p, the_clips()[4]) == 0
    assert job_result(st, 0) == a
    st.close()
    fresh.close()


def test_pcm_on_device(wrs, runs):
    """PCM already in HBM (pcm_on_device): the energy comes from the caller's buffers; clips 1 and 5, as from the host"""
    run = runs("f16")
    L = wrs.lib()
    picked = [1, 5]
    host = run.ctx.create_state()
    assert host.full_batch(params(wrs, token_timestamps=True, max_len=20), [the_clips()[k] for k in picked]) == 0
    want = [job_result(host, j) for j in range(len(picked))]
    host.close()
    assert any(d["t1"] > d["t0"] >= 0 for s in want[0] for d in s[3])
    ptrs = []
    for k in picked:
        x = np.ascontiguousarray(the_clips()[k], np.float32)
        p = L.whisper_mi355x_dev_alloc(run.ctx.ptr, x.nbytes)
        assert p and L.whisper_mi355x_memcpy(run.ctx.ptr, C.c_void_p(p), x.ctypes.data, x.nbytes, 1) == 0
        ptrs.append((p, len(x)))
    st = run.ctx.create_state()
    assert st.full_batch(params(wrs, token_timestamps=True, max_len=20), ptrs, on_device=True) == 0
    got = [job_result(st, j) for j in range(len(picked))]
    st.close()
    for p, _ in ptrs:
        L.whisper_mi355x_dev_free(run.ctx.ptr, C.c_void_p(p))
    assert got == want


def test_off_means_off(runs):
    """(7) token_timestamps = false with max_len = 8: nothing is wrapped, every token has t0 = t1 = -1, vlen = 0 (what
    the getters returned before the feature existed) and no pass runs"""
    run = runs("f16")
    res = run.batch(max_len=8, split_on_word=True)
    assert res == run.off
    assert run.ms == 0
    assert all((d["t0"], d["t1"], d["vlen"]) == (-1, -1, 0.0) for job in res for s in job for d in s[3])
