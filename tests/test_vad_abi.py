"""whisper.h's VAD block at the C-ABI boundary, without a GPU (tests/test_abi.py checks that every declared symbol is
exported): the default VAD params and context params, and the argument checks that return before the device is touched."""
import ctypes as C


def test_default_vad_params(wrs):
    p = wrs.lib().whisper_vad_default_params()
    assert abs(p.threshold - 0.5) < 1e-7 and p.min_speech_duration_ms == 250 and p.min_silence_duration_ms == 100
    assert p.max_speech_duration_s == C.c_float(3.4028234663852886e38).value and p.speech_pad_ms == 30
    assert abs(p.samples_overlap - 0.1) < 1e-7
    fp = wrs.lib().whisper_full_default_params(wrs.GREEDY)
    assert fp.vad is False and fp.vad_model_path is None
    q = fp.vad_params   # the same values, with an unbounded max_speech_duration_s
    assert (q.threshold, q.min_speech_duration_ms, q.min_silence_duration_ms, q.speech_pad_ms, q.samples_overlap) == \
        (p.threshold, p.min_speech_duration_ms, p.min_silence_duration_ms, p.speech_pad_ms, p.samples_overlap)
    assert q.max_speech_duration_s > 100000.0


def test_default_vad_context_params(wrs):
    cp = wrs.lib().whisper_vad_default_context_params()
    assert cp.n_threads == 4 and cp.use_gpu is True and cp.gpu_device == 0


def test_null_arguments_return_before_the_device(wrs, tmp_path, capfd):
    L = wrs.lib()
    assert not L.whisper_vad_init_from_file_with_params(str(tmp_path / "missing.bin").encode(), L.whisper_vad_default_context_params())
    assert "refused" in capfd.readouterr().err
    assert L.whisper_vad_detect_speech(None, None, 0) is False
    assert L.whisper_vad_n_probs(None) == 0 and not L.whisper_vad_probs(None)
    assert not L.whisper_vad_segments_from_probs(None, L.whisper_vad_default_params())
    assert L.whisper_vad_segments_n_segments(None) == 0
    L.whisper_vad_free_segments(None)
    L.whisper_vad_free(None)
    assert L.whisper_mi355x_vad_ms(None) == 0.0
    assert L.whisper_mi355x_vad_map(None, 0, None, 0) == -1
    assert L.whisper_mi355x_vad_probs_batch(None, None, None, 1, False, None, None) == -1
    assert L.whisper_mi355x_debug_vad_frontend(None, None, 0, None) == -1
    assert L.whisper_mi355x_debug_vad_gather(None, None, None, 1, None, None, None) == -1
