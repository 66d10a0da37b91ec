"""tests/tokts_ref.py (the reference of token_timestamps / max_len / split_on_word) against cases
worked out by hand. CPU only."""
import numpy as np

import tokts_ref as tr

# a toy vocabulary: text ids < EOT, specials from EOT, timestamps from BEG
EOT, BEG = 90, 100
TEXT = {0: b" hello", 1: b" world.", 2: b",", 3: b" 42", 4: b"ing", 5: b" a", 6: b"!", 7: b"", 8: b"x?y"}


def tok_str(i: int) -> bytes:
    if i in TEXT:
        return TEXT[i]
    if i >= BEG:
        return b"[_TT_%d]" % (i - BEG)
    if i == EOT:
        return b"[_EOT_]"
    return b"[_extra_token_%d]" % i


def T(i, tid=BEG, pt=0.0, ptsum=0.0):
    return dict(id=i, tid=tid, pt=pt, ptsum=ptsum)


def TS(k, p=0.9):  # the timestamp token BEG + k
    return dict(id=BEG + k, tid=BEG + k, pt=p, ptsum=p)


def times(tok):
    return [(t["t0"], t["t1"]) for t in tok]


def run(tokens, t0, t1, state=None):
    return tr.phase1(tokens, t0, t1, tr.new_state() if state is None else state, BEG, 0.01, 0.01, tok_str)


WORKED = [TS(0), T(0), T(1), TS(150)]


def test_voice_length():
    assert tr.voice_length(b" hello") == np.float32(np.float32(0.01) + np.float32(5.0))
    assert float(tr.voice_length(b" world.")) == float(np.float32(np.float32(np.float32(0.01) + np.float32(5.0)) + np.float32(3.0)))
    assert tr.voice_length(b",") == 2 and tr.voice_length(b" 42") == np.float32(np.float32(0.01) + np.float32(6.0))
    assert tr.voice_length(b"x?y") == 5 and tr.voice_length(b"") == 0 and tr.voice_length(b"!") == 3
    assert tr.voice_length("é".encode()) == 2  # bytes, not characters


def test_worked_example():
    st = tr.new_state()
    tok = run(WORKED, 0, 300, st)
    # vlen 5.01 and 8.01, ct = 300 * 5.01 / 13.02 = 115.4
    assert times(tok) == [(0, 0), (0, 115), (115, 300), (300, 300)]
    assert abs(float(tok[1]["vlen"]) - 5.01) < 1e-6 and abs(float(tok[2]["vlen"]) - 8.01) < 1e-6
    assert st == dict(t_beg=0, t_last=300, tid_last=BEG + 150)


def test_small_segments():
    st = tr.new_state()
    assert run([], 10, 20, st) == [] and st == tr.new_state()
    tok = run([T(0, pt=0.9, ptsum=0.9, tid=BEG + 5)], 10, 20, st)
    assert times(tok) == [(10, 20)] and tok[0]["vlen"] == 0 and st == tr.new_state()


def test_segment_without_beg_takes_t_last():
    st = tr.new_state()
    run(WORKED, 0, 300, st)
    tok = run([T(0), T(1), TS(250)], 300, 500, st)
    # t_beg stays 0: tt = 2 * 250 = 500; ct = 300 + 200 * 5.01 / 13.02 = 376.96
    assert times(tok) == [(300, 376), (376, 500), (500, 500)]
    assert st == dict(t_beg=0, t_last=500, tid_last=BEG + 250)


def test_tid_not_after_tid_last_is_ignored():
    tok = run([TS(0), T(5, BEG, 0.9, 0.9), T(0, BEG + 50, 0.9, 0.9), T(1, BEG + 50, 0.9, 0.9), TS(150)], 0, 300)
    # " hello" at tt = 100 is taken, " world." with the same tid is not; ct = 100 + 200 * 5.01 / 13.02 = 176.96
    assert times(tok) == [(0, 0), (0, 100), (100, 176), (176, 300), (300, 300)]


def test_low_probability_is_ignored():
    a = run([TS(0), T(5), T(0, BEG + 50, 0.9, 0.005), T(1), TS(150)], 0, 300)
    b = run([TS(0), T(5), T(0, BEG + 50, 0.005, 0.9), T(1), TS(150)], 0, 300)
    c = run([TS(0), T(5), T(0), T(1), TS(150)], 0, 300)
    assert times(a) == times(b) == times(c)


def test_time_past_segment_end_is_ignored():
    st = tr.new_state()
    tok = run([TS(0), T(0, BEG + 150, 0.9, 0.9), T(1), TS(100)], 0, 200, st)
    # tt = 300 > t1 = 200 is dropped; ct = 200 * 5.01 / 13.02 = 76.96
    assert times(tok) == [(0, 0), (0, 76), (76, 200), (200, 200)]
    assert st["tid_last"] == BEG + 100


def wrapped(tokens, t0s, t0, t1, max_len, sow):
    toks = [dict(t, t0=a) for t, a in zip(tokens, t0s)]
    return [(p["text"], p["t0"], p["t1"], [t["id"] for t in p["tokens"]]) for p in tr.wrap(toks, t0, t1, max_len, sow, EOT, tok_str)]


def test_wrap_max_len_1():
    # the leading timestamp token is token 0 of the segment: the first text token splits after it (an empty piece)
    got = wrapped(WORKED, [0, 0, 115, 300], 0, 300, 1, False)
    assert got == [(b"", 0, 0, [BEG]), (b" hello", 0, 115, [0]), (b" world.", 115, 300, [1, BEG + 150])]


def test_wrap_max_len_8():
    toks = [TS(0), T(0), T(4), T(1), TS(150)]
    t0s = [0, 0, 60, 115, 300]
    assert wrapped(toks, t0s, 0, 300, 8, False) == [(b" hello", 0, 60, [BEG, 0]), (b"ing", 60, 115, [4]),
                                                    (b" world.", 115, 300, [1, BEG + 150])]
    assert wrapped(toks, t0s, 0, 300, 8, True) == [(b" helloing", 0, 115, [BEG, 0, 4]), (b" world.", 115, 300, [1, BEG + 150])]
    # nothing to cut: one piece, its text rebuilt from the tokens < eot
    assert wrapped(toks, t0s, 0, 300, 100, False) == [(b" helloing world.", 0, 300, [BEG, 0, 4, 1, BEG + 150])]


def test_wrap_no_token_starts_with_space():
    toks = [T(4), T(4), T(2), T(4)]
    assert wrapped(toks, [0, 10, 20, 30], 0, 40, 1, True) == [(b"inging,ing", 0, 40, [4, 4, 2, 4])]
    assert [p[0] for p in wrapped(toks, [0, 10, 20, 30], 0, 40, 1, False)] == [b"ing", b"ing", b",", b"ing"]


def test_energy_small():
    x = np.array([1.0, -2.0, 0.5], np.float32)
    e = tr.energy(x)
    s = np.float32(np.float32(np.float32(1.0) + np.float32(2.0)) + np.float32(0.5))
    assert e.dtype == np.float32 and all(e == s / np.float32(65.0))
    x = np.zeros(100, np.float32)
    x[0] = 65.0
    e = tr.energy(x)
    assert all(e[:33] == 1.0) and all(e[33:] == 0.0)
    assert len(tr.energy(np.zeros(0, np.float32))) == 0


def box():
    e = np.zeros(1600, np.float32)  # 10 time units; mean 0.4, threshold 0.2
    e[320:960] = 1.0
    return e


def test_vad_clamps():
    e = box()
    # token 0: start walks up to 320 (t = 2); end walks up to 960 (t = 6), past the next token's t0 = 5: clamped.
    # token 1: start walks down to 319 (t = 1), before token 0's t1 = 5: clamped; end walks down to 959 (t = 5).
    assert tr.vad(e, [(0, 5, 1), (5, 10, 1)]) == [(2, 5), (5, 5)]
    # no neighbour to clamp against: the last token's end runs free
    assert tr.vad(e, [(0, 1, 1), (3, 5, 1)]) == [(1, 1), (1, 6)]


def test_vad_first_token_on_loud_start():
    e = box()
    # j = 0 on a loud sample takes the else branch: e < thold fails at once, t0 stays; its end walks up to 960 (t = 6)
    assert tr.vad(e, [(4, 5, 1), (7, 8, 1)])[0] == (4, 6)


def test_vad_special_tokens_and_silence():
    e = box()
    got = tr.vad(e, [(0, 5, 1), (5, 5, 0), (5, 10, 1), (10, 10, 0)])
    assert got[1] == (5, 5) and got[3] == (10, 10) and got[0] == (2, 5) and got[2] == (5, 5)
    z = np.zeros(1600, np.float32)
    spans = [(0, 3, 1), (3, 3, 1), (3, 9, 1)]
    assert tr.vad(z, spans) == [(a, b) for a, b, _ in spans]


def test_vad_times_outside_the_clip():
    e = box()
    # 99 -> sample 1599 (t = 9), -1 -> sample 0
    assert tr.vad(e, [(-1, 99, 1), (99, 120, 1)]) == [(2, 5), (9, 9)]
    assert tr.vad(np.ones(1, np.float32), [(0, 0, 1), (0, 7, 1)]) == [(0, 0), (0, 0)]
