"""Hand-made cases for tests/parallel_ref.py, the restatement of whisper_full_parallel's split, snap and merge rules
(DESIGN.md §19). The expected values are worked out by hand from the rules, not taken from the code."""
import numpy as np

import parallel_ref as pr

# (name, n_samples, offset_ms, n_processors) -> cuts, pieces
SPLIT = [
    ("remainder goes to the last piece", 100003, 0, 4, [0, 25000, 50000, 75000],
     [(0, 25000), (25000, 50000), (50000, 75000), (75000, 100003)]),
    # offset_samples = 16000, n_per = (100000 - 16000) / 3 = 28000: piece 0 keeps the offset's audio in front of it
    ("offset_ms > 0", 100000, 1000, 3, [0, 44000, 72000], [(0, 44000), (44000, 72000), (72000, 100000)]),
    # 16000 * 1234 / 1000 = 19744, n_per = (640000 - 19744) / 2 = 310128
    ("offset with a fraction", 640000, 1234, 2, [0, 329872], [(0, 329872), (329872, 640000)]),
]


def test_split():
    for name, n, off, np_, cuts, pieces in SPLIT:
        assert pr.cuts(n, off, np_) == cuts, name
        assert pr.pieces(n, cuts) == pieces, name


def test_shift():
    # upstream: 100 * ((k) * n_per) / 16000 + offset_ms / 10
    assert pr.shift(25000, 0) == 156            # 2500000 / 16000 = 156.25
    assert pr.shift(44000, 1000) == 175 + 100   # 100 * 28000 / 16000 = 175
    assert pr.shift(329872, 1234) == 1938 + 123  # 100 * 310128 / 16000 = 1938.3


def seg(t0, t1, toks=(), **kw):
    return dict(t0=t0, t1=t1, tokens=[dict(id=i, t0=a, t1=b, t_dtw=d) for i, (a, b, d) in enumerate(toks)], **kw)


def test_merge_shifts_and_clamps():
    cuts = [0, 25000, 50000]
    p0 = [seg(0, 100, [(0, 50, 10), (50, 100, 60)], text="a"), seg(100, 160, text="b")]
    # piece 1's first segment starts at 2 -> 158, before the previous t1 = 160: t0 is raised to 160, t1 stays 206;
    # its tokens are shifted, not clamped, and the -1 of an unset time stays
    p1 = [seg(2, 50, [(2, 30, -1), (-1, -1, 7)], text="c"), seg(50, 90, text="d")]
    p2 = [seg(0, 10, text="e")]
    out = pr.merge([p0, p1, p2], cuts)
    assert [(s["t0"], s["t1"], s["text"]) for s in out] == [(0, 100, "a"), (100, 160, "b"), (160, 206, "c"), (206, 246, "d"),
                                                             (312, 322, "e")]
    assert [(t["t0"], t["t1"], t["t_dtw"]) for t in out[2]["tokens"]] == [(158, 186, -1), (-1, -1, 163)]
    assert [(t["t0"], t["t1"], t["t_dtw"]) for t in out[0]["tokens"]] == [(0, 50, 10), (50, 100, 60)]
    assert p1[0]["t0"] == 2 and p1[0]["tokens"][0]["t0"] == 2   # the inputs are left alone


def test_merge_empty_pieces_and_offset():
    # piece 0 empty: nothing to clamp against; offset_ms = 1000 adds 100 to every later piece
    out = pr.merge([[], [seg(5, 20)], [], [seg(0, 9)]], [0, 44000, 72000, 100000], offset_ms=1000)
    assert [(s["t0"], s["t1"]) for s in out] == [(5 + 275, 20 + 275), (0 + 625, 9 + 625)]   # 100 * 84000 / 16000 = 525
    dec = pr.merge_decisions([[dict(seek=100, temp_idx=0)], [dict(seek=0, temp_idx=1), dict(seek=2900, temp_idx=0)]],
                             [0, 44000], offset_ms=1000)
    assert dec == [dict(seek=100, temp_idx=0), dict(seek=275, temp_idx=1), dict(seek=3175, temp_idx=0)]


def test_snap_bound():
    assert pr.snap_bound(500, 160000) == 500          # 1000 * (80000 - 320) / 16000 = 4980
    assert pr.snap_bound(5000, 160000) == 4980        # clipped by n_per / 2
    assert pr.snap_bound(500, 640) == 0               # 320 - 320: nothing moves
    assert pr.snap_bound(500, 600) == 0
    assert pr.snap_bound(500, 1000) == 11             # 1000 * 180 / 16000 = 11.25
    assert pr.snap_bound(0, 160000) == 0


def test_snap_lowest_rms_wins():
    n = 32000                                          # 100 windows
    rms = np.full(100, 0.5, np.float32)
    rms[47] = 0.01
    rms[55] = 0.001                                    # quieter, but |320 * 55 - 16000| = 1600 > 16 * 60 = 960
    # cut 16000 = window 50; snap 60 ms: windows 47..53 (|320 w - 16000| <= 960)
    assert pr.snap_candidates(n, 16000, 60) == [47, 48, 49, 50, 51, 52, 53]
    assert pr.snap_cut(rms, n, 16000, 60) == 320 * 47 + 160
    assert pr.snap_cut(rms, n, 16000, 100) == 320 * 55 + 160   # 16 * 100 = 1600: window 55 is a candidate now


def test_snap_ties():
    n = 32000
    rms = np.full(100, 0.5, np.float32)
    rms[48] = rms[51] = rms[52] = 0.25
    # equal RMS: 51 (distance 320) beats 48 and 52 (640)
    assert pr.snap_cut(rms, n, 16000, 60) == 320 * 51 + 160
    rms[49] = 0.25
    # 49 and 51 are equally near: the smaller w
    assert pr.snap_cut(rms, n, 16000, 60) == 320 * 49 + 160
    # all equal: the window the cut is the start of
    assert pr.snap_cut(np.ones(100, np.float32), n, 16000, 60) == 320 * 50 + 160
    # a cut that is no multiple of 320: 16100 lies in window 50; distances 100 (w = 50) and 220 (w = 51)
    assert pr.snap_cut(np.ones(100, np.float32), n, 16100, 60) == 320 * 50 + 160


def test_snap_range_clipped_by_half_a_piece():
    # n_per = 1600: snap = min(500, 1000 * (800 - 320) / 16000 = 30) = 30 ms -> |320 w - cut| <= 480
    n, np_ = 6400, 4
    assert pr.n_per(n, 0, np_) == 1600 and pr.snap_bound(500, 1600) == 30
    rms = np.ones(20, np.float32)
    rms[2] = 0.0          # 640: 960 away from the cut at 1600, outside 480
    rms[4] = 0.5          # 1280: 320 away
    rms[12] = 0.1         # 3840: 640 from 3200, outside; 960 from 4800, outside
    got = pr.snapped_cuts(rms, n, 0, np_, 500)
    assert got == [0, 320 * 4 + 160, 3200 + 160, 4800 + 160]
    assert all(b > a for a, b in zip(got, got[1:]))


def test_snap_windows_at_the_clip_end():
    # 10 whole windows + 100 samples: window 10 is not whole, so it is no candidate even though it is the quietest place
    n = 3300
    rms = np.ones(10, np.float32)
    rms[9] = 0.5
    assert pr.snap_candidates(n, 3000, 60) == [7, 8, 9]          # 320 w in [2040, 3960], w <= 9
    assert pr.snap_cut(rms, n, 3000, 60) == 320 * 9 + 160
    assert pr.snap_candidates(n, 3290, 1) == []                   # |320 w - 3290| <= 16: none inside
    assert pr.snap_cut(rms, n, 3290, 1) == 3290
    assert pr.snap_candidates(n, 100, 60) == [0, 1, 2, 3]         # ... and at the clip's start: w >= 0


def test_window_rms_is_calculate_rms():
    from oracle_py import rms_f32
    x = (np.random.default_rng(3).standard_normal(1000) * 0.1).astype(np.float32)
    r = pr.window_rms(x)
    assert len(r) == 3 and all(r[w] == rms_f32(x[320 * w:320 * w + 320]) for w in range(3))
