"""The recordings of tests/test_gpu_parallel.py and what the CPU oracle says about their pieces, computed once per session.

The recordings are synthetic_pcm utterances joined by 1.2 s of low noise, as tests/test_gpu_streaming.py's recording().
The seeds were picked with the oracle so that every window of every piece used by the tests is decided at t = 0 and no
greedy step is closer than the f16 near-tie rule's 0.05 nats (check_oracle asserts it; tests/margin_gate.py is the rule).
"""
import numpy as np

import parallel_ref as pr
from make_model import synthetic_pcm
from oracle_py import Oracle, reference_params

SHAPE = "tiny+conf"
SR = 16000
GAP = 0.05  # nats
# whisper_full_params.max_tokens of every call here. The synthetic model never chooses EOT, so a window with 30 s of audio
# behind it decodes to the step limit and fails the entropy rule at t = 0; with max_tokens it completes after 17 tokens at
# its last timestamp (seek_delta < 3000), and the next window starts there: a seek loop whose windows are all decided at t = 0.
MAX_TOKENS = 16

# name -> (utterances (synthetic_pcm seed, seconds), the noise's seed)
RECORDINGS = {
    # 36 s: with n_processors = 3 every piece is one window of 12 s (and with 8, for the beam groups, of 4.5 s). Not longer:
    # this model decides a lone window of 13 s and more at avg_logprob < -1 (its 3 tokens), so it would fall back.
    "rec40": (((40, 9.0), (41, 12.4), (42, 11.0)), 11),
    # ~70 s: with n_processors = 2 each piece runs its own seek loop over more than one window
    "rec70": (((25, 9.0), (26, 27.0), (27, 6.0), (28, 14.0), (29, 8.5)), 7),
}
_REC = {}
_ORACLE = {}


def recording(name: str) -> np.ndarray:
    if name not in _REC:
        utt, noise_seed = RECORDINGS[name]
        rng = np.random.default_rng(noise_seed)
        parts = []
        for seed, sec in utt:
            parts.append(synthetic_pcm(seed, seconds=sec))
            parts.append((rng.standard_normal(int(1.2 * SR)) * 0.002).astype(np.float32))
        _REC[name] = np.concatenate(parts).astype(np.float32)
        _REC[name].setflags(write=False)
    return _REC[name]


def piece_pcm(rec, cuts):
    return [rec[a:b] for a, b in pr.pieces(len(rec), cuts)]


def oracle_pieces(path: str, name: str, cuts, offset_ms: int = 0):
    """The oracle's whisper_full of every piece of the recording cut at `cuts` (piece 0 with offset_ms, the others with
    0), each on a fresh state: a list of oracle_py results. Cached by (recording, cuts, offset)."""
    key = (path, name, tuple(cuts), offset_ms)
    if key not in _ORACLE:
        o = Oracle(path, mode=1, n_threads=16)
        out = []
        for k, x in enumerate(piece_pcm(recording(name), cuts)):
            o.new_state()
            rp = reference_params("en")
            rp.offset_ms = offset_ms if k == 0 else 0
            rp.max_tokens = MAX_TOKENS
            out.append(o.full(x, rp))
        o.close()
        _ORACLE[key] = out
    return _ORACLE[key]


def check_oracle(results):
    """The condition on the inputs: every window decided at t = 0, no greedy step within GAP nats of a tie."""
    for k, r in enumerate(results):
        assert r["rc"] == 0, (k, r["rc"])
        assert r["decisions"] and all(d["temp_idx"] == 0 for d in r["decisions"]), (k, r["decisions"])
        assert len(r["margins"]) > 0 and float(min(r["margins"])) > GAP, (k, float(min(r["margins"])))


def oracle_segments(results):
    """Per piece, the segments as parallel_ref.merge takes them (tokens as plain ids)."""
    return [[dict(t0=s["t0"], t1=s["t1"], text=s["text"], tokens=list(s["tokens"])) for s in r["segments"]] for r in results]
