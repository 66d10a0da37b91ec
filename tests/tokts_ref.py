"""Reference for token_timestamps / max_len / split_on_word, in numpy and plain Python, written from
the specification and sharing no code with the engine. Four steps, one function each:

  energy(x)    the smoothed |x| signal of a clip (f32, the same bits as the sequential loop)
  phase1(...)  token t0 / t1 / vlen of one segment from its timestamp tokens, the rest spread by voice length
  vad(...)     the voice-activity adjust of one segment's tokens on the energy signal
  wrap(...)    a segment cut into pieces of at most max_len bytes of text

Times are 10 ms units, absolute within the clip. A token is a dict {id, tid, pt, ptsum} (phase1 adds t0, t1, vlen)."""
import numpy as np

HW = 2000          # half window of the threshold, samples
RATE = 16000


def voice_length(s: bytes) -> np.float32:
    r = np.float32(0.0)
    for ch in s:
        c = chr(ch)
        if c == " ":
            r = np.float32(r + np.float32(0.01))
        elif c == ",":
            r = np.float32(r + np.float32(2.0))
        elif c in ".!?" or "0" <= c <= "9":
            r = np.float32(r + np.float32(3.0))
        else:
            r = np.float32(r + np.float32(1.0))
    return r


def energy(x) -> np.ndarray:
    """e[i] = (sum_{j=-32..32, inside the clip} |x[i+j]|) / 65.0f, the sum in f32 from 0.0f in ascending j.
    Vectorised over i, sequential over j. A tap outside the clip adds +0.0f here where the loop skips it: the sum is
    never negative, so s + 0.0f has the bits of s."""
    a = np.abs(np.asarray(x, dtype=np.float32))
    n = len(a)
    pad = np.zeros(n + 64, np.float32)
    pad[32:32 + n] = a
    s = np.zeros(n, np.float32)
    for j in range(65):
        s = (s + pad[j:j + n]).astype(np.float32)
    return (s / np.float32(65.0)).astype(np.float32)


def new_state() -> dict:
    return dict(t_beg=0, t_last=0, tid_last=0)


def trunc(x: float) -> int:
    if x != x:
        return 0
    if x >= 9223372036854775807.0:
        return 2 ** 63 - 1
    if x <= -9223372036854775808.0:
        return -2 ** 63
    return int(x)


def phase1(tokens, t0, t1, state, beg, thold_pt, thold_ptsum, tok_str):
    """tokens: list of dicts {id, tid, pt, ptsum}; tok_str(id) -> bytes. Returns the tokens as new dicts with
    t0, t1, vlen; `state` (new_state()) is carried from segment to segment of a clip."""
    tok = [dict(t, t0=-1, t1=-1, vlen=np.float32(0.0)) for t in tokens]
    n = len(tok)
    if n == 0:
        return tok
    if n == 1:
        tok[0]["t0"], tok[0]["t1"] = t0, t1
        return tok
    thold_pt, thold_ptsum = np.float32(thold_pt), np.float32(thold_ptsum)
    if tok[0]["id"] == beg:
        tok[0]["t0"] = tok[0]["t1"] = t0
        tok[1]["t0"] = t0
        state["t_beg"] = state["t_last"] = t0
        state["tid_last"] = beg
    else:
        tok[0]["t0"] = state["t_last"]
    for j, t in enumerate(tok):
        t["vlen"] = voice_length(tok_str(t["id"]))
        tt = state["t_beg"] + 2 * (t["tid"] - beg)
        if np.float32(t["pt"]) > thold_pt and np.float32(t["ptsum"]) > thold_ptsum and t["tid"] > state["tid_last"] and tt <= t1:
            if j > 0:
                tok[j - 1]["t1"] = tt
            t["t0"] = tt
            state["tid_last"] = t["tid"]
    tok[n - 2]["t1"] = t1
    tok[n - 1]["t0"] = tok[n - 1]["t1"] = t1
    state["t_last"] = t1
    # fill the unknown intervals
    p0 = p1 = 0
    while True:
        while p1 < n and tok[p1]["t1"] < 0:
            p1 += 1
        if p1 >= n:
            p1 -= 1
        if p1 > p0:
            psum = 0.0
            for j in range(p0, p1 + 1):
                psum += float(tok[j]["vlen"])
            dt = float(tok[p1]["t1"] - tok[p0]["t0"])
            for j in range(p0 + 1, p1 + 1):
                with np.errstate(all="ignore"):
                    ct = float(np.float64(tok[j - 1]["t0"]) + np.float64(dt) * np.float64(tok[j - 1]["vlen"]) / np.float64(psum))
                tok[j - 1]["t1"] = tok[j]["t0"] = trunc(ct)
        p1 += 1
        p0 = p1
        if p1 >= n:
            break
    # fix-up
    for j in range(n - 1):
        if tok[j]["t1"] < 0:
            tok[j + 1]["t0"] = tok[j]["t1"]
        if j > 0 and tok[j - 1]["t1"] > tok[j]["t0"]:
            tok[j]["t0"] = tok[j - 1]["t1"]
            tok[j]["t1"] = max(tok[j]["t0"], tok[j]["t1"])
    return tok


def to_sample(t: int, N: int) -> int:
    q = t * RATE
    k = abs(q) // 100
    k = -k if q < 0 else k  # C division truncates toward zero
    return max(0, min(N - 1, k))


def to_ts(k: int) -> int:
    return (100 * k) // RATE


def vad(e, spans):
    """e: the clip's energy (f32 array, N >= 1 samples); spans: one segment's tokens in order as (t0, t1, is_text),
    is_text false for ids >= eot. Returns the adjusted [(t0, t1)]; a segment of fewer than 2 tokens is not adjusted by
    the engine (the caller leaves it out)."""
    e = np.asarray(e, dtype=np.float32)
    N = len(e)
    tok = [[int(a), int(b)] for a, b, _ in spans]
    n = len(tok)
    for j in range(n):
        if not spans[j][2]:
            continue
        t0, t1 = tok[j]
        s0, s1 = to_sample(t0, N), to_sample(t1, N)
        ss0, ss1 = max(s0 - HW, 0), min(s1 + HW, N)
        ns = ss1 - ss0
        S = np.sum(e[ss0:ss1], dtype=np.float64) if ns > 0 else np.float64(0.0)
        with np.errstate(all="ignore"):
            thold = np.float32(np.float64(0.5) * S / np.float64(ns))
        k = s0
        if e[k] > thold and j > 0:
            while k > 0 and e[k] > thold:
                k -= 1
            t0 = to_ts(k)
            if t0 < tok[j - 1][1]:
                t0 = tok[j - 1][1]
            else:
                s0 = k
        else:
            while e[k] < thold and k < s1:
                k += 1
            s0 = k
            t0 = to_ts(k)
        k = s1
        if e[k] > thold:
            while k < N - 1 and e[k] > thold:
                k += 1
            t1 = to_ts(k)
            if j < n - 1 and t1 > tok[j + 1][0]:
                t1 = tok[j + 1][0]
            else:
                s1 = k
        else:
            while e[k] < thold and k > s0:
                k -= 1
            s1 = k
            t1 = to_ts(k)
        tok[j] = [t0, t1]
    return [tuple(t) for t in tok]


def wrap(tokens, t0, t1, max_len, split_on_word, eot, tok_str):
    """tokens: dicts with id and t0 (after vad). Returns the pieces, in order, as dicts {t0, t1, text, tokens}
    (tokens = the piece's slice of the list)."""
    pieces = []
    cur = dict(t0=t0, t1=t1, text=b"", tokens=list(tokens))
    while True:
        acc, text, split = 0, b"", False
        for i, t in enumerate(cur["tokens"]):
            if t["id"] >= eot:
                continue
            s = tok_str(t["id"])
            if acc + len(s) > max_len and i > 0 and (not split_on_word or s[:1] == b" "):
                rest = dict(t0=t["t0"], t1=cur["t1"], text=b"", tokens=cur["tokens"][i:])
                cur["text"], cur["t1"], cur["tokens"] = text, t["t0"], cur["tokens"][:i]
                pieces.append(cur)
                cur, split = rest, True
                break
            acc += len(s)
            text += s
        if not split:
            cur["text"] = text
            pieces.append(cur)
            return pieces
