"""The beam-search contract of DESIGN.md §11 in numpy: the logits rules (restated from the oracle's
process_logits; decisions in float32 inputs, sums in float64), the candidates of a row, the per-token rules of
whisper_full (process_step), and the bookkeeping (pooling, ordering, re-parenting, scoring, the winner).

Driven by logits_fn(prefix) -> raw logits row [n_vocab] of the step that follows the generated tokens `prefix`
(() = the prompt's last row). Every decision that a small numeric difference could flip records its gap in
Result.gaps, so a test can assert that its inputs are decided by more than the arithmetic's error.
"""
import math
from dataclasses import dataclass, field

import numpy as np

CHUNK = 30


def vocab_ids(n_vocab: int, space: int) -> dict:
    """The special ids the rules use (whisper.cpp's whisper_vocab: multilingual files shift them)."""
    multi = n_vocab >= 51865
    eot = 50256 + (1 if multi else 0)
    sot = eot + 1
    n_lang = n_vocab - 51765 - (1 if multi else 0)
    translate = sot + 1 + n_lang if multi else 50357
    return dict(n_vocab=n_vocab, eot=eot, sot=sot, translate=translate, transcribe=translate + 1, solm=translate + 2,
                prev=translate + 3, nosp=translate + 4, not_=translate + 5, beg=translate + 6, space=space, n_lang=100)


@dataclass
class Params:
    K: int = 5
    max_tokens: int = 0
    single_segment: bool = False
    no_timestamps: bool = False
    suppress_blank: bool = True
    max_initial_ts: float = 1.0
    length_penalty: float = -1.0
    entropy_thold: float = 2.4
    logprob_thold: float = -1.0
    n_max: int = 220          # n_text_ctx / 2 - 4
    seek: int = 0
    seek_end: int = 3000
    n_audio_ctx: int = 1500


@dataclass
class Beam:
    tokens: list = field(default_factory=list)   # dicts {id, tid, p, plog, pt, ptsum}
    result_len: int = 0
    sum_logprobs_all: float = 0.0
    sum_logprobs: float = -math.inf
    avg_logprobs: float = -math.inf
    entropy: float = 0.0
    score: float = -math.inf
    seek_delta: int = 100 * CHUNK
    has_ts: bool = False
    failed: bool = False
    completed: bool = False
    step: int = 0
    ended: bool = False

    def live(self):
        return not (self.ended or self.failed or self.completed)

    def copy(self):
        b = Beam(**{k: getattr(self, k) for k in self.__dataclass_fields__})
        b.tokens = list(self.tokens)
        return b

    def ids(self):
        return [t["id"] for t in self.tokens]


def rules(raw, beam: Beam, P: Params, v: dict):
    """whisper_process_logits at t = 0 for the row that follows `beam`'s tokens. Returns (logprobs [V] float64 with
    -inf for suppressed tokens, text tokens included when the timestamp rule fired; the rule's gap in nats)."""
    x = np.asarray(raw, np.float32).astype(np.float64).copy()
    V, beg, eot = v["n_vocab"], v["beg"], v["eot"]
    ids = beam.ids()
    initial = len(ids) == 0
    if P.suppress_blank and initial:
        x[eot] = -np.inf
        if v["space"] >= 0:
            x[v["space"]] = -np.inf
    x[v["not_"]] = -np.inf
    if P.no_timestamps:
        x[beg:] = -np.inf
    for k in ("sot", "nosp", "solm", "translate", "transcribe", "prev"):
        x[v[k]] = -np.inf
    x[v["sot"] + 1: v["sot"] + 1 + v["n_lang"]] = -np.inf
    last_ts = len(ids) > 0 and ids[-1] >= beg
    penult_ts = len(ids) < 2 or ids[-2] >= beg
    if last_ts:
        if penult_ts:
            x[beg:] = -np.inf
        else:
            x[:eot] = -np.inf
    if initial and P.max_initial_ts > 0.0:
        precision = np.float32(CHUNK) / np.float32(P.n_audio_ctx)
        tid0 = int(round(float(np.float32(P.max_initial_ts) / precision)))
        x[beg + tid0 + 1:] = -np.inf
    if beam.has_ts:
        x[beg: beg + beam.seek_delta // 2] = -np.inf
    fin = np.isfinite(x)
    if not fin.any():
        return np.full(V, -np.inf), math.inf
    mx = x[fin].max()
    lse = math.log(np.exp(x[fin] - mx).sum()) + mx
    lp = np.where(fin, x - lse, -np.inf)
    ts = lp[beg:]
    ts_fin = ts[np.isfinite(ts)]
    ts_logprob = -math.inf
    if ts_fin.size:
        m = ts_fin.max()
        ts_logprob = math.log(np.exp(ts_fin - m).sum()) + m
    max_text = lp[:beg].max()
    gap = abs(ts_logprob - max_text) if math.isfinite(ts_logprob) and math.isfinite(max_text) else math.inf
    if ts_logprob > max_text:
        lp[:beg] = -np.inf
    return lp, gap


def candidates(lp, K: int, v: dict):
    """Contract point 3: the K most probable tokens with p > 0 (float32 p), (p descending, id ascending)."""
    beg = v["beg"]
    p = np.exp(lp)
    p32 = p.astype(np.float32)
    ok = np.nonzero(p32 > 0)[0]
    order = ok[np.lexsort((ok, -p32[ok]))][:K]  # the contract's key: (float32 p descending, id ascending)
    ts = p[beg:]
    sum_ts = float(ts.sum())
    tid_row = beg + int(np.argmax(ts)) if ts.size and ts.max() > 0 else 0
    pt_row = float(ts.max() / (sum_ts + 1e-10)) if ts.size else 0.0
    out = []
    for i in order:
        i = int(i)
        c = dict(id=i, tid=tid_row, p=float(p[i]), plog=float(lp[i]), pt=pt_row, ptsum=sum_ts)
        if i >= beg:
            c["tid"], c["pt"] = i, c["p"]
        out.append(c)
    return out


def process_step(b: Beam, c: dict, P: Params, v: dict) -> bool:
    """whisper_full's per-token code for token index b.step (engine.cpp process_step); True: decoding goes on."""
    i = b.step
    b.tokens.append(c)
    b.sum_logprobs_all += float(np.float32(c["plog"]))  # the engine adds the float plog to a double
    beg, delta_min = v["beg"], 10
    if c["id"] > beg:
        sd_new = 2 * (c["id"] - beg)
        if b.has_ts and b.seek_delta > sd_new and b.result_len < i:
            b.failed = True
            return False
        b.seek_delta = sd_new
        b.result_len = i + 1
        b.has_ts = True
    if c["id"] == v["eot"] or (P.max_tokens > 0 and i >= P.max_tokens) or \
            (b.has_ts and P.seek + b.seek_delta + delta_min >= P.seek_end):
        if b.result_len == 0 and not P.no_timestamps:
            if P.seek + b.seek_delta + delta_min >= P.seek_end:
                b.result_len = i + 1
            else:
                b.failed = True
                return False
        if P.single_segment or P.no_timestamps:
            b.result_len = i + 1
            b.seek_delta = 100 * CHUNK
        b.completed = True
        return False
    if i == P.n_max - 1 and (b.result_len == 0 or b.seek_delta < 100 * CHUNK // 2):
        b.failed = True
        return False
    return i + 1 < P.n_max


def score_seq(b: Beam, P: Params):
    if b.result_len == 0:
        return
    s = 0.0
    for t in b.tokens[:b.result_len]:
        s += float(np.float32(t["plog"]))
    b.sum_logprobs = s
    b.avg_logprobs = s / b.result_len
    pen = float(b.result_len)
    if P.length_penalty > 0.0:
        pen = ((5.0 + pen) / 6.0) ** float(np.float32(P.length_penalty))
    b.score = s / pen
    ids = [t["id"] for t in b.tokens[max(0, b.result_len - 32): b.result_len]]
    ent = 0.0
    for tok in sorted(set(ids)):
        q = ids.count(tok) / len(ids)
        ent -= q * math.log(q)
    b.entropy = ent


@dataclass
class Result:
    beams: list            # per beam: dict(tokens, sum_logprobs_all, completed, failed, winner)
    winner: int            # -1: the attempt failed
    tokens: list           # the winner's tokens cut at result_len (ids)
    result_len: int
    avg_logprobs: float
    entropy: float
    failed0: bool
    gaps: list             # (what, gap in nats or score units)
    picks: list            # per step: [(beam, parent, rank)]
    copies: list           # per step: [(dst beam, src beam, row0, row1)], rows counted from the prompt's first token

    def min_gap(self):
        return min((g for _, g in self.gaps), default=math.inf)


def select(rows, sums, cands, positions, gaps=None):
    """Contract point 5: pool, order, assign. rows: parent beam indices; cands[r]: that row's candidates."""
    pool = []
    for r, par in enumerate(rows):
        for rank, c in enumerate(cands[r]):
            pool.append((sums[r] + float(np.float32(c["plog"])), par, rank, r))
    pool.sort(key=lambda e: (-e[0], e[1], e[2]))
    n = len(positions)
    if gaps is not None:
        for a, b in zip(pool[:n], pool[1:n + 1]):
            gaps.append(("pool order", a[0] - b[0]))
    picks = []
    for i, pos in enumerate(positions):
        picks.append((pos, pool[i][1], pool[i][2], pool[i][3]) if i < len(pool) else (pos, -1, -1, -1))
    return picks


def beam_search(logits_fn, P: Params, v: dict, n_prompt: int = 0) -> Result:
    K = max(1, P.K)
    gaps, all_picks, all_copies = [], [], []
    beams = [Beam() for _ in range(K)]
    held = [None] * K      # generated-token sequences whose K/V rows a beam's self slot holds (None: not even the prompt)
    held[0] = []

    def reparent(rows, cands, positions, first):
        sums = [0.0 if first else beams[r].sum_logprobs_all for r in rows]
        picks = select(rows, sums, cands, positions, gaps)
        all_picks.append([(a, b, c) for a, b, c, _ in picks])
        old = [b.copy() for b in beams]
        old_held = list(held)
        copies = []
        for pos, par, rank, r in picks:
            if par < 0:
                beams[pos].failed = True
                continue
            if par != pos:
                src, dst = old_held[par], old_held[pos]
                if dst is None:
                    m = 0
                else:
                    g = 0
                    while g < len(src) and g < len(dst) and src[g] == dst[g]:
                        g += 1
                    m = n_prompt + g
                if m < n_prompt + len(src):
                    copies.append((pos, par, m, n_prompt + len(src)))
                held[pos] = list(src)
            nb = old[par].copy()
            if not first:
                nb.step += 1
            nb.ended = not process_step(nb, cands[r][rank], P, v)
            beams[pos] = nb
        all_copies.append(copies)

    lp, g = rules(logits_fn(()), Beam(), P, v)
    gaps.append(("timestamp rule", g))
    reparent([0], [candidates(lp, K, v)], list(range(K)), True)
    while any(b.live() for b in beams):
        live = [i for i, b in enumerate(beams) if b.live()]
        cands = []
        if hasattr(logits_fn, "prefetch"):  # (a logits source that is cheaper per step than per prefix)
            logits_fn.prefetch([tuple(beams[i].ids()) for i in live])
        for i in live:
            held[i] = held[i] + [beams[i].tokens[-1]["id"]]
            lp, g = rules(logits_fn(tuple(beams[i].ids())), beams[i], P, v)
            gaps.append(("timestamp rule", g))
            cands.append(candidates(lp, K, v))
        reparent(live, cands, live, False)
    full_ids = [b.ids() for b in beams]
    for b in beams:
        if not b.failed:
            b.tokens = b.tokens[:b.result_len]
            score_seq(b, P)
            if b.result_len > 32:
                gaps.append(("entropy threshold", abs(b.entropy - P.entropy_thold)))
                if b.entropy < P.entropy_thold:
                    b.failed = True
    ok = [i for i, b in enumerate(beams) if not b.failed]
    win = -1
    for i in ok:
        if win < 0 or beams[i].score > beams[win].score:
            win = i
    for i in ok:
        if i != win and math.isfinite(beams[win].score):
            gaps.append(("winner score", beams[win].score - beams[i].score))
    out = [dict(tokens=full_ids[i], sum_logprobs_all=b.sum_logprobs_all, completed=b.completed, failed=b.failed, winner=i == win)
           for i, b in enumerate(beams)]
    if win >= 0:
        w = beams[win]
        if math.isfinite(w.avg_logprobs):
            gaps.append(("logprob threshold", abs(w.avg_logprobs - P.logprob_thold)))
        return Result(out, win, w.ids(), w.result_len, w.avg_logprobs, w.entropy, False, gaps, all_picks, all_copies)
    return Result(out, -1, [], 0, -math.inf, 0.0, True, gaps, all_picks, all_copies)
