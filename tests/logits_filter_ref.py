"""The two halves of kernels/logits.hip's rules around whisper_full_params.logits_filter_callback, in numpy
(DESIGN.md §20): pre() is the row the callback gets, post() what the rest of the rules and the greedy choice make of the
row it leaves. tests/logits_ref.py is imported and left alone: post() runs logits_ref.process itself, over a private
second instance of that module whose `masked` is replaced by the post-callback rules over the filtered row, so the
log-softmax, the timestamp rule and the record are logits_ref's own expressions and post(pre(raw)) is
logits_ref.process(raw) in every bit (tests/test_logits_filter_ref.py holds it to that).

Order (include/whisper.h): before the callback the temperature divide (float32), suppress_blank on the initial step,
<|notimestamps|>, no_timestamps, sot / nosp / solm / translate / transcribe / prev and the language tokens; after it
suppress_eot, timestamp pairing, max_initial_ts and the monotonic timestamps. With tdrz (tdrz_enable) solm is kept.
"""
import importlib.util

import numpy as np

import logits_ref as lr

_spec = importlib.util.spec_from_file_location("_logits_ref_for_filter", lr.__file__)
_priv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_priv)


def pre(raw, c: dict, v: dict, tdrz: bool = False):
    """The row a logits_filter_callback gets: float32 [V], -inf = suppressed by a rule that precedes it."""
    x = np.array(raw, np.float32)
    t = np.float32(c["temperature"])
    if t > 0.0:
        with np.errstate(over="ignore"):
            x = x / t
    beg, eot, sot = v["beg"], v["eot"], v["sot"]
    if c["suppress_blank"] and c["is_initial"]:
        x[eot] = -np.inf
        x[v["space"]] = -np.inf
    x[v["not_"]] = -np.inf
    if c["no_timestamps"]:
        x[beg:] = -np.inf
    for k in ("sot", "nosp", "solm", "translate", "transcribe", "prev"):
        if k == "solm" and tdrz:
            continue
        x[v[k]] = -np.inf
    x[sot + 1: sot + 1 + v["n_lang"]] = -np.inf
    assert x.dtype == np.float32
    return x


def post_masked(filtered, c: dict, v: dict):
    """The rules that follow the callback over the row it left (float64, -inf = suppressed): logits_ref.masked's tail."""
    x = np.asarray(filtered, np.float32).astype(np.float64)
    beg, eot = v["beg"], v["eot"]
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


def post(filtered, raw, c: dict, v: dict) -> dict:
    """logits_ref.process's record and rows for the filtered row; nosp_prob is the raw, undivided row's."""
    _priv.masked = lambda _raw, c_, v_: post_masked(filtered, c_, v_)
    try:
        return _priv.process(raw, c, v)
    finally:
        _priv.masked = None
