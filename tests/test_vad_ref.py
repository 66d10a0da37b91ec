"""tests/vad_ref.py itself (the reference of the VAD tests), on the CPU: f32 against f64 on the burst
signal, the gate model's separation, hand cases of get_speech_timestamps, the piece table and the time map."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_vad_model as mk  # noqa: E402
import vad_ref as vr  # noqa: E402

BURSTS = ((0.8, 1.6), (2.6, 3.4), (4.4, 5.2))


def runs(*pairs):
    return [p for n, p in pairs for _ in range(n)]


def prm(**kw):
    d = vr.default_params()
    d.update(kw)
    return d


HI, LO = 0.9, 0.05
# (name, probs, params, expected segments in samples); windows are 512 samples, the defaults are threshold 0.5 (so
# neg_threshold 0.35), min_speech 4000, min_silence 1600 and pad 480 samples
HAND = [
    ("empty", [], prm(), []),
    ("all_silence", runs((20, LO)), prm(), []),
    ("all_speech", runs((20, HI)), prm(), [(0, 10240)]),
    # 5 windows of speech = 2560 samples <= min_speech: dropped
    ("min_speech_drop", runs((5, LO), (5, HI), (10, LO)), prm(), []),
    ("one_segment", runs((5, LO), (10, HI), (10, LO)), prm(), [(2080, 8160)]),
    # 3 silent windows (1536 < 1600 samples by the time speech returns) do not end the segment
    ("min_silence_merge", runs((5, LO), (10, HI), (3, LO), (10, HI), (10, LO)), prm(), [(2080, 14816)]),
    # 5 silent windows do; the gap of 2560 >= 2 pad: both sides get the whole pad
    ("pad_full", runs((5, LO), (10, HI), (5, LO), (10, HI), (10, LO)), prm(), [(2080, 8160), (9760, 15840)]),
    # a gap of 1024 < 2 pad (pad 640): split in half
    ("pad_half", runs((5, LO), (10, HI), (2, LO), (10, HI), (5, LO)), prm(min_silence_duration_ms=32, speech_pad_ms=40),
     [(1920, 8192), (8192, 14464)]),
    # speech to the last window: closed at the audio length, where the pad is clamped
    ("runs_to_end", runs((5, LO), (20, HI)), prm(), [(2080, 12800)]),
    # between the thresholds (0.4) neither starts nor ends a segment
    ("hysteresis", runs((5, 0.4), (10, HI), (10, 0.4)), prm(), [(2080, 10240 + 2560)]),
    # max_speech = 16000 - 512 - 960 = 14528 samples, no silence seen: cut at the window that exceeds it
    ("max_split_no_prev_end", runs((40, HI)), prm(max_speech_duration_s=1.0), [(0, 15104), (15104, 20480)]),
    # a silence of 5 windows (> 98 ms, < min_silence 300 ms) leaves prev_end = 5120 and next_start = 7680: cut there
    ("max_split_prev_end", runs((10, HI), (5, LO), (25, HI)), prm(max_speech_duration_s=1.0, min_silence_duration_ms=300),
     [(0, 5600), (7200, 20480)]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_segments_hand_cases(case):
    _, p, params, want = case
    assert vr.segments_from_probs(np.asarray(p, dtype=np.float32), params) == want


@pytest.fixture(scope="module")
def burst():
    x = mk.burst_signal()
    out = {}
    for shape in ("rand", "gate"):
        m = mk.make_tensors(shape, 0)
        out[shape] = (vr.probs(m, x, np.float64), vr.probs(m, x, np.float32))
    return x, out


def test_f32_against_f64(burst):
    x, out = burst
    for shape, (p64, p32) in out.items():
        assert p32.dtype == np.float32 and len(p64) == 188
        d = float(np.abs(p32 - p64).max())
        print(shape, "numpy f32 - f64:", d)
        assert d < 1e-6  # 16 f32 ulps at 1.0


def test_gate_model_separates(burst):
    x, out = burst
    p = out["gate"][0]
    w = np.arange(len(p)) * 512
    speech = np.zeros(len(p), dtype=bool)
    silence = np.ones(len(p), dtype=bool)
    for a, b in BURSTS:
        a, b = int(a * 16000), int(b * 16000)
        speech |= (w >= a) & (w + 512 <= b)                 # windows wholly inside a burst
        silence &= ~((w + 512 > a) & (w < b + 8 * 512))     # not in a burst, nor in the 8 windows of decay after it
    assert speech.sum() > 60 and silence.sum() > 60
    assert p[speech].min() > 0.9 and p[silence].max() < 0.2
    # the end-to-end tests need every window clear of both thresholds
    assert np.abs(p - 0.5).min() > 1e-3 and np.abs(p - 0.35).min() > 1e-3
    segs = vr.segments_from_probs(p, vr.default_params())
    assert len(segs) == 3
    for (s, e), (a, b) in zip(segs, BURSTS):
        assert abs(s - a * 16000) < 1024 and 0 <= e - b * 16000 < 10 * 512  # 8 windows of decay, the window grid, the pad


def test_zero_samples():
    m = mk.make_tensors("rand", 0)
    assert len(vr.probs(m, np.zeros(0, dtype=np.float32))) == 0
    assert len(vr.probs(m, np.zeros(1, dtype=np.float32))) == 1 and len(vr.probs(m, np.zeros(513, dtype=np.float32))) == 2


def test_f16_file_tensors_round_trip(tmp_path):
    t = mk.write_vad_model(str(tmp_path / "v.bin"), "rand", 3, f16=True)
    raw = mk.make_tensors("rand", 3)
    assert np.array_equal(t["_model.decoder.rnn.bias_ih"], raw["_model.decoder.rnn.bias_ih"])
    w = "_model.decoder.rnn.weight_hh"
    assert not np.array_equal(t[w], raw[w]) and np.allclose(t[w], raw[w], rtol=1e-3, atol=1e-6)


def test_piece_table_and_map():
    segs = [(1000, 5000), (5800, 9000), (20000, 20001), (30000, 40000)]
    tab = vr.piece_table(segs, 36000, 0.1)
    # overlap 1600: clamped at the next start (5800), whole after the second and after the 1-sample segment, the end clamped to the audio
    assert tab == [(1000, 5800, 0, 4800), (5800, 10600, 6400, 11200), (20000, 21601, 12800, 14401), (30000, 36000, 16001, 22001)]
    assert vr.filtered_len(tab) == 22001
    pcm = np.arange(36000, dtype=np.float32)
    f = vr.filtered_pcm(pcm, tab)
    assert len(f) == 22001 and f[0] == 1000 and f[4799] == 5799 and f[4800] == 0 and f[6399] == 0 and f[6400] == 5800
    assert f[12800] == 20000 and f[14400] == 21600 and f[14401] == 0 and f[16001] == 30000 and f[-1] == 35999
    assert vr.piece_table([(5, 6), (9, 20)], 100, 0.0) == [(5, 6, 0, 1), (9, 20, 1601, 1612)]   # a piece of 1 sample
    ts = [vr.map_time(tab, t) for t in range(0, 140)]
    assert all(b >= a for a, b in zip(ts, ts[1:]))                      # monotone
    for s, e, vs, ve in tab:                                            # identity inside a piece
        for x in range(vs, ve, 160):
            if x % 160 == 0:
                assert vr.map_time(tab, x // 160) == (s + x - vs) // 160
    assert vr.map_time(tab, 31) == 5800 // 160                          # in the first gap (4960): the first piece's end
    assert vr.map_time(tab, 1000) == 36000 // 160                       # beyond the last piece: its end
    assert vr.piece_table([], 1000, 0.1) == [] and vr.map_time([], 17) == 17
    # a segment wholly beyond the audio leaves no piece
    assert vr.piece_table([(0, 512), (1024, 2048)], 600, 0.0) == [(0, 512, 0, 512)]
