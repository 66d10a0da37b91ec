"""tests/audio_ctx_ref.py (the reference for whisper_full_params.audio_ctx): the file rewriter changes the header
word and the one tensor and nothing else, and the oracle on a truncated file gives other results than at the full
context (so a library that ignores audio_ctx fails the GPU cases)."""
import struct

from audio_ctx_ref import POS_EMB, _walk, oracle_full_at, truncated_model
from conftest import model_path
from make_model import read_tensors, synthetic_pcm
from margin_gate import kept_token_margins
from oracle_py import cached_full, reference_params


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def test_full_context_is_identity():
    p = model_path("micro")
    assert _bytes(truncated_model(p, 1500)) == _bytes(p)


def test_only_header_and_positional_embedding_change():
    p = model_path("micro")
    a, b = _bytes(p), _bytes(truncated_model(p, 512))
    ha, hb = struct.unpack_from("<12i", a, 0), struct.unpack_from("<12i", b, 0)
    assert ha[2] == 1500 and hb[2] == 512
    assert ha[:2] + ha[3:] == hb[:2] + hb[3:]
    ra, rb = _walk(a), _walk(b)
    assert a[48:ra[0][0]] == b[48:rb[0][0]]  # mel filters and vocabulary
    ta, tb = read_tensors(p), read_tensors(truncated_model(p, 512))
    assert list(ta) == list(tb)
    for name in ta:
        if name == POS_EMB:
            d = ta[name][1][0]
            assert ta[name][0] == tb[name][0] == 0
            assert tuple(ta[name][1]) == (d, 1500) and tuple(tb[name][1]) == (d, 512)
            assert tb[name][2] == ta[name][2][:512 * d * 4] and len(tb[name][2]) == 512 * d * 4
        else:
            assert ta[name] == tb[name], name
    assert len(a) - len(b) == (1500 - 512) * ta[POS_EMB][1][0] * 4


def test_oracle_result_depends_on_the_context():
    ref = oracle_full_at("tiny.en+conf", 512, 2)
    toks, margins = kept_token_margins(ref)
    assert len(toks) == 42, len(toks)
    rp = reference_params("en")
    rp.temperature_inc = 0.0
    full = cached_full(model_path("tiny.en+conf"), ("clip", 2), lambda: synthetic_pcm(2), rp)
    assert toks != kept_token_margins(full)[0]
