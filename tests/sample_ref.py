"""The sampled-draw contract of DESIGN.md §12 in numpy: the Philox4x32-10 uniform word, the draw (float64 prefix
sums over the row's float32 probs, ascending id), and the best_of candidate loop of a t > 0 attempt, built on
beam_ref's rules (the row divided by the float32 temperature), process_step and score_seq.

Every draw records its margin min(target - C_{id-1}, C_id - target) / S: the distance of the uniform target to the
nearest boundary of the drawn token's CDF interval, as a fraction of the row's mass. A test asserts that its inputs
are decided by more than the arithmetic's error.
"""
import math
from dataclasses import dataclass

import numpy as np

import beam_ref as br

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(key, counter):
    """Philox4x32-10 (Random123). key = (k0, k1), counter = (c0, c1, c2, c3); every entry an int or an array of one
    shape. Returns the 4 output words as uint32 arrays [4, ...]."""
    k0, k1 = (np.asarray(k, np.uint64) & MASK for k in key)
    c = [np.asarray(x, np.uint64) & MASK for x in counter]
    shape = np.broadcast(k0, k1, *c).shape
    k0, k1 = np.broadcast_to(k0, shape).copy(), np.broadcast_to(k1, shape).copy()
    c0, c1, c2, c3 = (np.broadcast_to(x, shape).copy() for x in c)
    for _ in range(10):
        p0 = np.uint64(M0) * c0   # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        h0, l0 = p0 >> np.uint64(32), p0 & MASK
        h1, l1 = p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def counter(seek: int, temp_idx: int, cand: int, i):
    """The draw's counter: (0, seek in 10 ms frames, 16 * temp_idx + candidate, token index)."""
    return (0, seek, 16 * temp_idx + cand, i)


def word(seed: int, seek: int, temp_idx: int, cand: int, i):
    """x0 of the draw: output word 0 under key = the 64-bit seed (lo, hi)."""
    return philox((seed & MASK, (seed >> 32) & MASK), counter(seek, temp_idx, cand, i))[0]


def draw(probs, x0: int):
    """The token of one row: (id, margin). probs: the row's float32 probs. id = -1 (margin inf) when the row sums to 0:
    the record then stays as the logits kernel wrote it."""
    p = np.asarray(probs, np.float32).astype(np.float64)
    C = np.cumsum(p)  # sequential, ascending id
    S = float(C[-1])
    if not S > 0.0:
        return -1, math.inf
    u = (float(int(x0)) + 0.5) * 2.0 ** -32
    target = u * S
    i = int(np.searchsorted(C, target, side="right"))  # the smallest i with C_i > target
    if i >= len(p):
        i = int(np.nonzero(p > 0)[0][-1])
        return i, 0.0
    assert p[i] > 0.0
    lo = float(C[i - 1]) if i > 0 else 0.0
    return i, min(target - lo, float(C[i]) - target) / S


@dataclass
class Result:
    cands: list      # per candidate: dict(tokens, sum_logprobs_all, completed, failed, winner, score)
    winner: int      # -1: the attempt failed
    tokens: list     # the winner's tokens cut at result_len (ids)
    result_len: int
    avg_logprobs: float
    margins: list    # every draw's margin
    score_gap: float  # winner's score minus the best other candidate's with different tokens (inf: none)

    def min_margin(self):
        return min(self.margins, default=math.inf)


def sample_candidates(logits_fn, P: br.Params, v: dict, N: int, temperature, seed: int = 0, temp_idx: int = 1,
                      pick=None) -> Result:
    """The N candidates of one sampled attempt of the window at P.seek. logits_fn(prefix) -> raw logits row of the
    step after the generated tokens `prefix` (() = the prompt's last row). pick(probs32, cand, i) -> id replaces the
    draw (tests)."""
    t = np.float32(temperature)
    beg = v["beg"]
    beams = [br.Beam() for _ in range(N)]
    margins = []

    def step(b, cand):
        i = len(b.tokens)
        raw = np.asarray(logits_fn(tuple(b.ids())), np.float32)
        with np.errstate(over="ignore"):
            lp, _ = br.rules(raw / t, b, P, v)
        greedy = br.candidates(lp, 1, v)
        p32 = np.exp(lp).astype(np.float32)
        if pick is not None:
            tok, m = pick(p32, cand, i), math.inf
        else:
            tok, m = draw(p32, int(word(seed, P.seek, temp_idx, cand, i)))
        if tok < 0:  # an empty row: the record of the logits kernel (id 0, p 0)
            c = greedy[0] if greedy else dict(id=0, tid=0, p=0.0, plog=-math.inf, pt=0.0, ptsum=0.0)
        else:
            if pick is None:
                margins.append(m)
            g = greedy[0]
            c = dict(id=tok, tid=g["tid"], p=float(p32[tok]), plog=float(np.float32(lp[tok])), pt=g["pt"], ptsum=g["ptsum"])
            if tok >= beg:
                c["tid"], c["pt"] = tok, c["p"]
        b.ended = not br.process_step(b, c, P, v)

    for cand, b in enumerate(beams):
        step(b, cand)
    while any(b.live() for b in beams):
        if hasattr(logits_fn, "prefetch"):
            logits_fn.prefetch([tuple(b.ids()) for b in beams if b.live()])
        for cand, b in enumerate(beams):
            if b.live():
                b.step += 1
                step(b, cand)
    full_ids = [b.ids() for b in beams]
    for b in beams:
        if not b.failed:
            b.tokens = b.tokens[:b.result_len]
            br.score_seq(b, P)
            if b.result_len > 32 and b.entropy < P.entropy_thold:
                b.failed = True
    win = -1
    for i, b in enumerate(beams):  # beam_winner: the highest score among the non-failed, the lowest index on ties
        if not b.failed and (win < 0 or b.score > beams[win].score):
            win = i
    gap = math.inf
    for i, b in enumerate(beams):
        if win >= 0 and i != win and not b.failed and full_ids[i] != full_ids[win]:
            gap = min(gap, beams[win].score - b.score)
    out = [dict(tokens=full_ids[i], sum_logprobs_all=b.sum_logprobs_all, completed=b.completed, failed=b.failed,
                winner=i == win, score=b.score) for i, b in enumerate(beams)]
    if win < 0:
        return Result(out, -1, [], 0, -math.inf, margins, gap)
    w = beams[win]
    return Result(out, win, w.ids(), w.result_len, w.avg_logprobs, margins, gap)
