"""The beam-search surface of the C ABI and the binding, without a device."""
import ctypes as C


def test_default_params_beam(wrs):
    p = wrs.lib().whisper_full_default_params(wrs.BEAM_SEARCH)
    assert p.strategy == wrs.BEAM_SEARCH
    assert p.beam_search.beam_size == 5
    assert p.beam_search.patience == -1.0
    g = wrs.lib().whisper_full_default_params(wrs.GREEDY)
    assert g.strategy == wrs.GREEDY and g.beam_search.beam_size == -1


def test_beam_symbols_resolve(wrs):
    L = wrs.lib()
    for name in ("whisper_mi355x_beam_info", "whisper_mi355x_debug_logits_topk", "whisper_mi355x_debug_kv_gather"):
        assert getattr(L, name) is not None
    assert C.sizeof(wrs.Cand) == 32
    # no state: no beams
    assert L.whisper_mi355x_beam_info(None, 0, 0, None, 0, None, None) == -1
    # the hooks refuse bad arguments before touching a device
    assert L.whisper_mi355x_debug_logits_topk(None, None, 0, None, None, 1, 0, None, None) == -1
    assert L.whisper_mi355x_debug_kv_gather(None, None, 0, 0, 0, 0, None, 0, None) == -1


def test_beam_full_params(wrs):
    p = wrs.beam_full_params(beam_size=3, language="en")
    r = wrs.reference_full_params("en")
    assert p.strategy == wrs.BEAM_SEARCH and p.beam_search.beam_size == 3
    for f in ("language", "suppress_blank", "no_speech_thold", "entropy_thold", "logprob_thold", "temperature_inc",
              "no_context", "single_segment"):
        assert getattr(p, f) == getattr(r, f), f
    assert wrs.beam_full_params().beam_search.beam_size == 5
