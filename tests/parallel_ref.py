"""The split, snap and merge rules of whisper_full_parallel in plain Python integers.

split: upstream's whisper_full_parallel. offset_samples = 16000 * offset_ms / 1000, n_per = (n_samples - offset_samples) /
  n_processors; piece 0 is [0, offset_samples + n_per) with the caller's params, piece k >= 1 starts at cut_k =
  offset_samples + k * n_per with offset_ms = 0, the last piece runs to n_samples.
snap: each interior cut moves to the quietest 320-sample window near it (the rule of the app's take_forced_chunk,
  audio.rs:161-225, around a given place): lowest RMS, then nearest, then first.
merge: in piece order; a segment of piece k >= 1 gains shift_k on t0 and t1, then t0 = max(t0, the previous t1). Token
  t0 / t1 / t_dtw that are not -1 gain shift_k too (upstream leaves them; they are not clamped).

Segments are dicts with t0, t1 and (optionally) tokens, a list of dicts that may hold t0, t1, t_dtw; every other key is
carried along untouched.
"""
import copy

RATE = 16000
WINDOW = 320
MAX_PIECES = 128


def offset_samples(offset_ms: int) -> int:
    return RATE * offset_ms // 1000


def n_per(n_samples: int, offset_ms: int, n_processors: int) -> int:
    return (n_samples - offset_samples(offset_ms)) // n_processors


def cuts(n_samples: int, offset_ms: int, n_processors: int) -> list:
    """The piece starts; cuts[0] = 0."""
    per = n_per(n_samples, offset_ms, n_processors)
    assert per > 0
    return [0] + [offset_samples(offset_ms) + k * per for k in range(1, n_processors)]


def pieces(n_samples: int, the_cuts) -> list:
    """[(start, end)] of every piece: the last one takes the remainder."""
    ends = list(the_cuts[1:]) + [n_samples]
    return list(zip(the_cuts, ends))


def snap_bound(snap_ms: int, per: int) -> int:
    """min(snap_ms, 1000 * (n_per / 2 - 320) / 16000); not positive: nothing moves. Keeps moved cuts strictly increasing:
    a cut moves by at most 16 * snap + 160 < n_per / 2."""
    room = per // 2 - WINDOW
    if room <= 0:
        return 0
    return min(snap_ms, 1000 * room // RATE)


def snap_candidates(n_samples: int, cut: int, snap: int) -> list:
    """The windows w wholly inside the clip with |320 w - cut| <= 16 snap."""
    if snap <= 0:
        return []
    return [w for w in range(n_samples // WINDOW) if abs(WINDOW * w - cut) <= 16 * snap]


def snap_cut(rms, n_samples: int, cut: int, snap: int) -> int:
    """rms[w] = the RMS of window w of the whole clip."""
    cand = snap_candidates(n_samples, cut, snap)
    if not cand:
        return cut
    w = min(cand, key=lambda w: (float(rms[w]), abs(WINDOW * w - cut), w))
    return WINDOW * w + WINDOW // 2


def snapped_cuts(rms, n_samples: int, offset_ms: int, n_processors: int, snap_ms: int) -> list:
    c = cuts(n_samples, offset_ms, n_processors)
    snap = snap_bound(snap_ms, n_per(n_samples, offset_ms, n_processors))
    return [0] + [snap_cut(rms, n_samples, x, snap) for x in c[1:]]


def window_rms(pcm) -> list:
    """oracle_py.rms_f32 (audio.rs calculate_rms) of every whole 320-sample window."""
    from oracle_py import rms_f32
    return [rms_f32(pcm[WINDOW * w:WINDOW * (w + 1)]) for w in range(len(pcm) // WINDOW)]


def shift(cut: int, offset_ms: int) -> int:
    return 100 * (cut - offset_samples(offset_ms)) // RATE + offset_ms // 10


def merge(piece_segments, the_cuts, offset_ms: int = 0) -> list:
    """piece_segments[k] = the segments of piece k as its own whisper_full call returns them."""
    out = [copy.deepcopy(s) for s in piece_segments[0]]
    for k in range(1, len(piece_segments)):
        d = shift(the_cuts[k], offset_ms)
        for s in piece_segments[k]:
            s = copy.deepcopy(s)
            s["t0"] += d
            s["t1"] += d
            if out:
                s["t0"] = max(s["t0"], out[-1]["t1"])
            for t in s.get("tokens", []):
                if isinstance(t, dict):
                    for key in ("t0", "t1", "t_dtw"):
                        if key in t and t[key] != -1:
                            t[key] += d
            out.append(s)
    return out


def merge_decisions(piece_decisions, the_cuts, offset_ms: int = 0) -> list:
    out = [dict(d) for d in piece_decisions[0]]
    for k in range(1, len(piece_decisions)):
        for d in piece_decisions[k]:
            out.append(dict(d, seek=d["seek"] + shift(the_cuts[k], offset_ms)))
    return out
