"""The VAD kernels (nobs-whisper_amd/csrc/kernels/vad.hip) against tests/vad_ref.py on synthetic model
files written into pytest's tmp dir by tools/make_vad_model.py.

The bar of the numerical tests, computed in the test on the same input: the GPU's max |v - v_f64| is at most 16 x the
distance of the reference's own f32 form from its f64 form, with a floor of 16 f32 ulps of the values' magnitude (1e-6
for a probability; 16 * 2^-23 * max |xg| for the LSTM inputs): the arithmetic is the same f32, only the summation order
and the transcendental implementations differ. Both distances are printed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, model_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_vad_model as mk  # noqa: E402
import vad_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu

# 1 sample; one short of, exactly, and one past a window (the zero-padded tail, the reflect pad reading both edges); three
# windows; five windows = one past a tile of four
SHORT = [1, 511, 512, 513, 1061, 2100]


def signal(n):
    """n samples around the first burst's onset (sample 12800 of the burst signal)"""
    return mk.burst_signal()[12500:12500 + n].copy()


@pytest.fixture(scope="module")
def env(wrs, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vad_models")
    out = {}
    for shape in ("rand", "gate"):
        path = str(tmp / f"{shape}.bin")
        model = mk.write_vad_model(path, shape, 0)
        out[shape] = (model, wrs.VadContext(path))
    yield out
    for _, v in out.values():
        v.close()


@pytest.fixture(scope="module")
def refs(env):
    """(shape, name) -> (signal, p_f64, p_f32), computed once"""
    out = {}
    for shape, (model, _) in env.items():
        for name, x in [("burst", mk.burst_signal())] + [(n, signal(n)) for n in SHORT]:
            out[shape, name] = (x, vr.probs(model, x, np.float64), vr.probs(model, x, np.float32))
    return out


@pytest.mark.parametrize("n", SHORT)
def test_frontend_matches_reference(env, n):
    model, v = env["rand"]
    x = signal(n)
    x64, x32 = vr.frontend(model, x, np.float64), vr.frontend(model, x, np.float32)
    got = v.debug_frontend(x)
    assert got.shape == x64.shape == ((n + 511) // 512, 512)
    d_gpu, d_np = float(np.abs(got - x64).max()), float(np.abs(x32 - x64).max())
    floor = 16 * 2.0 ** -23 * float(np.abs(x64).max())
    print(f"frontend n={n}: gpu-f64 {d_gpu:.3e}  numpy f32-f64 {d_np:.3e}  floor {floor:.3e}")
    assert d_gpu <= max(16 * d_np, floor)


@pytest.mark.parametrize("name", ["burst"] + SHORT)
@pytest.mark.parametrize("shape", ["rand", "gate"])
def test_probs_match_reference(env, refs, shape, name):
    x, p64, p32 = refs[shape, name]
    v = env[shape][1]
    assert v.detect_speech(x)
    got = v.probs()
    assert got.dtype == np.float32 and len(got) == len(p64) == (len(x) + 511) // 512
    d_gpu, d_np = float(np.abs(got - p64).max()), float(np.abs(p32 - p64).max())
    print(f"probs {shape} {name}: gpu-f64 {d_gpu:.3e}  numpy f32-f64 {d_np:.3e}")
    assert d_gpu <= max(16 * d_np, 1e-6)


def test_zero_samples(env):
    v = env["rand"][1]
    assert v.detect_speech(np.zeros(0, np.float32)) and len(v.probs()) == 0
    assert v.segments_from_probs() == []
    assert v.probs_batch([np.zeros(0, np.float32), signal(513)])[0].size == 0


def test_state_resets_between_calls(env):
    v = env["gate"][1]
    x = mk.burst_signal()
    assert v.detect_speech(x)
    a = v.probs()
    assert v.detect_speech(signal(2100))   # another clip in between leaves nothing behind
    assert v.detect_speech(x)
    assert np.array_equal(a.view(np.uint32), v.probs().view(np.uint32))


@pytest.mark.parametrize("shape", ["rand", "gate"])
def test_batch_is_bit_identical_to_single_clips(wrs, env, shape):
    v = env[shape][1]
    big = np.tile(mk.burst_signal(), 1)
    clips = [big[12500:12500 + 513], big[10000:15000], big[:32000]]
    single = []
    for c in clips:
        assert v.detect_speech(c)
        single.append(v.probs())
    host = v.probs_batch(clips)
    L = wrs.lib()
    ctx = wrs.WhisperContext(model_path("micro"))
    ptrs = []
    for c in clips:
        a = np.ascontiguousarray(c, np.float32)
        p = L.whisper_mi355x_dev_alloc(ctx.ptr, a.nbytes)
        assert p and L.whisper_mi355x_memcpy(ctx.ptr, C.c_void_p(p), a.ctypes.data, a.nbytes, 1) == 0
        ptrs.append((p, len(a)))
    dev = v.probs_batch(ptrs, on_device=True)
    for p, _ in ptrs:
        L.whisper_mi355x_dev_free(ctx.ptr, C.c_void_p(p))
    ctx.close()
    for s, h, d in zip(single, host, dev):
        assert len(s) > 0
        assert np.array_equal(s.view(np.uint32), h.view(np.uint32)) and np.array_equal(s.view(np.uint32), d.view(np.uint32))


def test_gather_is_exact(wrs):
    ctx = wrs.WhisperContext(model_path("micro"))
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(9000).astype(np.float32), rng.standard_normal(700).astype(np.float32)
    # clip a: a piece whose overlap is clamped at the next start, a piece of 1 sample, a piece that ends with the clip
    ta = vr.piece_table([(100, 2000), (2300, 2301), (8000, 9500)], len(a), 0.1)
    assert ta == [(100, 2300, 0, 2200), (2300, 3901, 3800, 5401), (8000, 9000, 7001, 8001)]
    ta1 = vr.piece_table([(100, 2000), (2300, 2301), (8000, 9500)], len(a), 0.0)
    assert ta1[1] == (2300, 2301, 3500, 3501)
    tb = vr.piece_table([(0, 700)], len(b), 0.1)
    got = ctx.debug_vad_gather([a, a, b, b], [ta, ta1, tb, []])
    want = [vr.filtered_pcm(a, ta), vr.filtered_pcm(a, ta1), vr.filtered_pcm(b, tb), np.zeros(0, np.float32)]
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    # pieces that would read or write out of bounds are refused before the device is touched
    assert ctx.debug_vad_gather([b], [[(0, 701, 0, 701)]]) == -1
    assert ctx.debug_vad_gather([b], [[(10, 20, 0, 11)]]) == -1
    assert ctx.debug_vad_gather([b], [[(10, 20, 5, 15), (30, 40, 14, 24)]]) == -1
    assert ctx.debug_vad_gather([b], [[(-1, 20, 0, 21)]]) == -1
    ctx.close()
