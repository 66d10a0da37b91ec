"""kernels/logits.hip's contract in numpy: process_logits + sample_token(best) of oracle/oracle_whisper.cpp for an
arbitrary SeqCtl (the per-row rule inputs of the kernels), and the SeqCtl / ints transition of one decode step
(engine.cpp: process_step appends the token, fill_ctl rebuilds the rule inputs; the pipelined engine does both on
the device in decode_advance_kernel).

The temperature divide is float32 (the oracle and the kernels divide the float row); everything after it is float64.
The log-softmax uses beam_ref.rules' expressions, so at temperature 0 the two references agree bit for bit
(tests/test_logits_ref.py holds them to that, and this file to the oracle).
"""
import math

import numpy as np

CTL_FIELDS = ("is_initial", "last_ts", "penult_ts", "has_ts", "seek_delta", "temperature", "suppress_blank",
              "no_timestamps", "suppress_eot", "tid0_initial", "want_probs", "want_nosp")
# fields decode_advance_kernel owns; the rest of a SeqCtl passes through a step unchanged
CTL_ADVANCED = ("is_initial", "last_ts", "penult_ts", "has_ts", "seek_delta", "want_nosp")


def ctl(**kw) -> dict:
    """A SeqCtl as fill_ctl builds it mid-sequence after two text tokens at t = 0 with the default parameters."""
    c = dict(is_initial=0, last_ts=0, penult_ts=0, has_ts=0, seek_delta=3000, temperature=0.0, suppress_blank=1,
             no_timestamps=0, suppress_eot=0, tid0_initial=50, want_probs=0, want_nosp=0)
    for k in kw:
        assert k in c, k
    c.update(kw)
    return c


def masked(raw, c: dict, v: dict):
    """The filtered logits (float64, -inf = suppressed) in process_logits' order."""
    x32 = np.asarray(raw, np.float32)
    t = np.float32(c["temperature"])
    if t > 0.0:
        with np.errstate(over="ignore"):
            x32 = x32 / t
    x = x32.astype(np.float64)
    beg, eot, sot = v["beg"], v["eot"], v["sot"]
    if c["suppress_blank"] and c["is_initial"]:
        x[eot] = -np.inf
        x[v["space"]] = -np.inf
    x[v["not_"]] = -np.inf
    if c["no_timestamps"]:
        x[beg:] = -np.inf
    for k in ("sot", "nosp", "solm", "translate", "transcribe", "prev"):
        x[v[k]] = -np.inf
    x[sot + 1: sot + 1 + v["n_lang"]] = -np.inf
    if c["suppress_eot"]:
        x[eot] = -np.inf
    if c["last_ts"]:
        if c["penult_ts"]:
            x[beg:] = -np.inf
        else:
            x[:eot] = -np.inf
    if c["is_initial"] and c["tid0_initial"] >= 0:
        x[beg + c["tid0_initial"] + 1:] = -np.inf
    if c["has_ts"]:
        x[beg: beg + c["seek_delta"] // 2] = -np.inf
    return x


def process(raw, c: dict, v: dict) -> dict:
    """One row through the rules and the greedy choice.

    logprobs [V] float64 (-inf: suppressed, text tokens included when the timestamp rule fired), probs = exp(logprobs),
    suppressed (bool [V]), id / tid / p / plog / pt / ptsum as sample_token(best) returns them (id = tid = 0, p = 0,
    plog = -inf, ptsum = 0 for a row without a token: kernels.h), nosp_prob from the raw undivided row, top2_gap (the
    two largest logprobs) and ts_gap (timestamp mass against the best text token), in nats; tid_lp = the logprob that
    decides whether a text token's tid is a timestamp id or 0 (float p > 0), tid_gap = the gap between the two most
    probable timestamps."""
    V, beg = v["n_vocab"], v["beg"]
    raw = np.asarray(raw, np.float32)
    x = masked(raw, c, v)
    fin = np.isfinite(x)
    out = dict(ts_fired=False)
    r64 = raw.astype(np.float64)
    rf = np.isfinite(r64)
    rm = r64[rf].max()
    out["nosp_prob"] = float(np.exp(r64[v["nosp"]] - (math.log(np.exp(r64[rf] - rm).sum()) + rm)))
    if not fin.any():
        out.update(logprobs=np.full(V, -np.inf), probs=np.zeros(V), suppressed=~fin, id=0, tid=0, p=0.0, plog=-math.inf,
                   pt=0.0, ptsum=0.0, top2_gap=math.inf, ts_gap=math.inf, tid_lp=-math.inf, tid_gap=math.inf)
        return out
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
    out["ts_gap"] = abs(ts_logprob - max_text) if math.isfinite(ts_logprob) and math.isfinite(max_text) else math.inf
    if ts_logprob > max_text:
        lp[:beg] = -np.inf
        out["ts_fired"] = True
    p = np.exp(lp)
    top = np.sort(lp[np.isfinite(lp)])[::-1]
    out["top2_gap"] = float(top[0] - top[1]) if top.size > 1 else math.inf
    i = int(np.argmax(lp))  # first index on ties, as the oracle's scan over the probs
    pts = p[beg:]
    sum_ts = float(pts.sum())
    tid_lp = float(lp[beg:].max())
    tst = np.sort(lp[beg:][np.isfinite(lp[beg:])])[::-1]
    out["tid_gap"] = float(tst[0] - tst[1]) if tst.size > 1 else math.inf
    tid = beg + int(np.argmax(pts)) if np.float32(pts.max()) > 0 else 0
    pt = float(pts.max() / (sum_ts + 1e-10))
    if i >= beg:
        tid, pt = i, float(p[i])
    out.update(logprobs=lp, probs=p, suppressed=~np.isfinite(lp), id=i, tid=tid, p=float(p[i]), plog=float(lp[i]), pt=pt,
               ptsum=sum_ts, tid_lp=tid_lp)
    return out


def lp_err(got, ref) -> float:
    """Worst error of a float logprobs row against the reference's, over the tokens the reference keeps: absolute for
    |logprob| <= 1 (the candidates a decision is made among), relative beyond (a float logprob of -1300 is a multiple
    of 1.2e-4; what it can carry is its relative precision)."""
    ref = np.asarray(ref, np.float64)
    keep = np.isfinite(ref)
    if not keep.any():
        return 0.0
    d = np.abs(np.asarray(got, np.float64)[keep] - ref[keep]) / np.maximum(1.0, np.abs(ref[keep]))
    return float(d.max())


def advance(c: dict, ints: np.ndarray, ct: int, r: int, tok: int, beg: int) -> dict:
    """One decode step of row r: process_step appended `tok`, then fill_ctl rebuilt the row's SeqCtl and the decoder's
    inputs moved on (tok | pos | slot | nkv_self | nkv_cross, ct entries each, edited in place)."""
    n = dict(c)
    # fill_ctl over the token list with `tok` appended
    n["is_initial"] = 0
    n["last_ts"] = int(tok >= beg)
    n["penult_ts"] = 1 if c["is_initial"] else int(c["last_ts"])  # fewer than 2 tokens, or tokens[-2] >= beg
    if tok > beg:                                                # process_step
        n["has_ts"] = 1
        n["seek_delta"] = 2 * (tok - beg)
    n["want_nosp"] = 0  # only a window's first step asks for the no-speech probability
    ints[r] = tok
    ints[ct + r] += 1
    ints[3 * ct + r] = ints[ct + r] + 1
    return n
