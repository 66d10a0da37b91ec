"""suppress_nst / suppress_regex in numpy: the deny mask of a vocabulary, and kernels/logits.hip's
contract with a mask, as a wrapper of tests/logits_ref.py.

mask(): whisper.cpp's non-speech list [ext], written out here, and re.fullmatch over the tokens' byte strings. The
engine compiles the pattern with std::regex in its ECMAScript flavour, where `.` excludes "\\r" as well as "\\n"
(Python's excludes "\\n" only), so an unescaped `.` outside a character class is matched as [^\\n\\r] here.
process(): a denied id is a raw logit of -inf to every rule (the rules only ever add -inf, so where the mask is applied
among them does not matter); nosp_prob is the undenied row's.
"""
import math
import re

import numpy as np

import logits_ref as lr

NON_SPEECH = ['"', "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
              "「", "」", "『", "』", "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", '("', "((", "))", "(((", ")))",
              "[[", "]]", "{{", "}}", "♪♪", "♪♪♪", "♩", "♪", "♫", "♬", "♭", "♮", "♯"]
assert len(NON_SPEECH) == 54 and len(set(NON_SPEECH)) == 54


def ecma_bytes(pattern: str) -> bytes:
    """The pattern as bytes for Python's re, with ECMAScript's `.` (no "\\n", no "\\r")."""
    src, out, i, in_class = pattern.encode(), bytearray(), 0, False
    while i < len(src):
        ch = src[i:i + 1]
        if ch == b"\\" and i + 1 < len(src):
            out += src[i:i + 2]
            i += 2
            continue
        if in_class:
            in_class = ch != b"]"
        elif ch == b"[":
            in_class = True
        elif ch == b".":
            out += b"[^\\n\\r]"
            i += 1
            continue
        out += ch
        i += 1
    return bytes(out)


def mask(tokens, suppress_nst: bool, regex) -> np.ndarray:
    """bool [V]: the denied ids of a vocabulary given as the list of its tokens' byte strings (id = index). A string that
    several ids carry belongs to the last of them, as in the engine's token_to_id map. regex: str or None (off)."""
    to_id = {bytes(t): i for i, t in enumerate(tokens)}
    deny = np.zeros(len(tokens), bool)
    if suppress_nst:
        for s in NON_SPEECH:
            for t in (s.encode(), b" " + s.encode()):
                if t in to_id:
                    deny[to_id[t]] = True
        for t in (b" -", b" '"):
            if t in to_id:
                deny[to_id[t]] = True
    if regex is not None:
        rx = re.compile(ecma_bytes(regex))
        for t, i in to_id.items():
            if rx.fullmatch(t):
                deny[i] = True
    return deny


def words(deny: np.ndarray) -> np.ndarray:
    """The mask as the engine packs it: uint32 [(V + 31) // 32], token i = bit i & 31 of word i >> 5, tail bits 0."""
    V = len(deny)
    bits = np.zeros((V + 31) // 32 * 32, np.uint8)
    bits[:V] = deny
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).copy()


def process(raw, c: dict, v: dict, deny) -> dict:
    """logits_ref.process of the row with its denied ids at -inf; nosp_prob from the row as it came."""
    raw = np.asarray(raw, np.float32)
    deny = np.asarray(deny, bool)
    assert deny.shape == raw.shape
    cut = raw.copy()
    cut[deny] = -np.inf
    r64 = raw.astype(np.float64)
    rf = np.isfinite(r64)
    if not np.isfinite(cut).any():  # logits_ref.process takes its no-speech sum over the finite raw logits: none left
        rm = r64[rf].max()
        nosp = float(np.exp(r64[v["nosp"]] - (math.log(np.exp(r64[rf] - rm).sum()) + rm)))
        V = len(raw)
        return dict(ts_fired=False, nosp_prob=nosp, logprobs=np.full(V, -np.inf), probs=np.zeros(V), suppressed=np.ones(V, bool),
                    id=0, tid=0, p=0.0, plog=-math.inf, pt=0.0, ptsum=0.0, top2_gap=math.inf, ts_gap=math.inf,
                    tid_lp=-math.inf, tid_gap=math.inf)
    out = lr.process(cut, c, v)
    if deny.any():
        out["nosp_prob"] = lr.process(raw, c, v)["nosp_prob"]
    return out
