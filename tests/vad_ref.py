"""The Silero-VAD v5 forward pass, get_speech_timestamps, the filtered audio and the time map, as DESIGN.md §18 defines
them: the reference of the VAD tests (numpy; f64 and f32 forms of the forward pass, integers everywhere else).

A model is the dict of tools/make_vad_model.py: tensor name -> f32 array in torch shape."""
import numpy as np

SR = 16000
N_WINDOW = 512
PAD = 64
N_FFT = 256
HOP = 128
STRIDES = (1, 2, 2, 1)
GAP = 1600  # zero samples between two pieces of the filtered audio (0.1 s)
MIN_SILENCE_AT_MAX_SPEECH_MS = 98


def n_windows(n_samples: int) -> int:
    return (n_samples + N_WINDOW - 1) // N_WINDOW


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def frontend(model: dict, pcm, dtype=np.float64):
    """[n_windows, 512]: the LSTM inputs xg[t] = W_ih x_t + b_ih + b_hh of every window (steps 1-4 and the input half of
    step 5); every window is independent up to here"""
    W = {k: np.asarray(v, dtype=dtype) for k, v in model.items()}
    pcm = np.asarray(pcm, dtype=dtype)
    nw = n_windows(len(pcm))
    if nw == 0:
        return np.zeros((0, 512), dtype=dtype)
    x = np.zeros(nw * N_WINDOW, dtype=dtype)
    x[:len(pcm)] = pcm
    x = np.pad(x.reshape(nw, N_WINDOW), ((0, 0), (PAD, PAD)), mode="reflect")           # [nw, 640]
    fr = np.stack([x[:, f * HOP:f * HOP + N_FFT] for f in range(4)], axis=1)              # [nw, 4, 256]
    basis = W["_model.stft.forward_basis_buffer"][:, 0, :]                                # [258, 256]
    spec = fr @ basis.T                                                                   # [nw, 4, 258]
    nb = N_FFT // 2 + 1
    a = np.sqrt(spec[..., :nb] * spec[..., :nb] + spec[..., nb:] * spec[..., nb:])        # [nw, frames, 129]
    for l, s in enumerate(STRIDES):
        w = W[f"_model.encoder.{l}.reparam_conv.weight"]                                  # [out, in, 3]
        b = W[f"_model.encoder.{l}.reparam_conv.bias"]
        ap = np.pad(a, ((0, 0), (1, 1), (0, 0)))
        n_out = (a.shape[1] + 2 - 3) // s + 1
        cols = np.stack([ap[:, p * s:p * s + 3, :] for p in range(n_out)], axis=1)        # [nw, n_out, 3, in]
        a = np.maximum(np.einsum("npti,oit->npo", cols, w) + b, 0)
    assert a.shape[1] == 1
    xg = a[:, 0, :] @ W["_model.decoder.rnn.weight_ih"].T + W["_model.decoder.rnn.bias_ih"] + W["_model.decoder.rnn.bias_hh"]
    return xg.astype(dtype)


def probs(model: dict, pcm, dtype=np.float64):
    """speech probability of every 512-sample window; h and c start at zero and carry across the windows"""
    xg = frontend(model, pcm, dtype)
    whh = np.asarray(model["_model.decoder.rnn.weight_hh"], dtype=dtype)
    hw = np.asarray(model["_model.decoder.decoder.2.weight"], dtype=dtype).reshape(-1)
    hb = np.asarray(model["_model.decoder.decoder.2.bias"], dtype=dtype)[0]
    H = whh.shape[1]
    h = np.zeros(H, dtype=dtype)
    c = np.zeros(H, dtype=dtype)
    out = np.zeros(len(xg), dtype=dtype)
    for t in range(len(xg)):
        g = xg[t] + whh @ h
        i, f, gg, o = _sigmoid(g[:H]), _sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sigmoid(g[3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        out[t] = _sigmoid(np.dot(hw, np.maximum(h, 0)) + hb)
    return out


def default_params() -> dict:
    return dict(threshold=0.5, min_speech_duration_ms=250, min_silence_duration_ms=100, max_speech_duration_s=float("inf"),
                speech_pad_ms=30, samples_overlap=0.1)


def segments_from_probs(p, prm: dict) -> list:
    """Silero's get_speech_timestamps over window probabilities: [(start, end)] in samples of the original audio, whose
    length counts as len(p) * 512"""
    f32 = np.float32
    thr = f32(prm["threshold"])
    neg = f32(max(f32(thr - f32(0.15)), f32(0.01)))
    big = 2 ** 30  # "unbounded"; durations are clamped to +-big samples

    def ms(v):
        s = SR * abs(int(v)) // 1000 * (1 if int(v) >= 0 else -1)  # (C division truncates toward zero)
        return max(-big, min(big, s))
    min_speech, min_silence, pad = ms(prm["min_speech_duration_ms"]), ms(prm["min_silence_duration_ms"]), ms(prm["speech_pad_ms"])
    max_s = float(prm["max_speech_duration_s"])
    if not np.isfinite(max_s) or abs(max_s) > 100000.0:
        max_speech = big
    else:
        max_speech = int(float(SR) * float(f32(max_s))) - N_WINDOW - 2 * pad
        if max_speech < 0 or max_speech > big:
            max_speech = big
    min_silence_max = SR * MIN_SILENCE_AT_MAX_SPEECH_MS // 1000
    audio_len = len(p) * N_WINDOW

    sp = []
    triggered = False
    temp_end = prev_end = next_start = start = 0
    for i, prob in enumerate(p):
        prob = f32(prob)
        cur = N_WINDOW * i
        if prob >= thr and temp_end:
            temp_end = 0
            if next_start < prev_end:
                next_start = cur
        if prob >= thr and not triggered:
            triggered = True
            start = cur
            continue
        if triggered and cur - start > max_speech:
            if prev_end:
                sp.append([start, prev_end])
                if next_start < prev_end:
                    triggered = False
                else:
                    start = next_start
                prev_end = next_start = temp_end = 0
            else:
                sp.append([start, cur])
                prev_end = next_start = temp_end = 0
                triggered = False
                continue
        if prob < neg and triggered:
            if not temp_end:
                temp_end = cur
            if cur - temp_end > min_silence_max:
                prev_end = temp_end
            if cur - temp_end < min_silence:
                continue
            if temp_end - start > min_speech:
                sp.append([start, temp_end])
            prev_end = next_start = temp_end = 0
            triggered = False
            continue
    if triggered and audio_len - start > min_speech:
        sp.append([start, audio_len])

    for k in range(len(sp)):
        if k == 0:
            sp[k][0] = max(0, sp[k][0] - pad)
        if k + 1 < len(sp):
            silence = sp[k + 1][0] - sp[k][1]
            if silence < 2 * pad:
                sp[k][1] += silence // 2
                sp[k + 1][0] = max(0, sp[k + 1][0] - silence // 2)
            else:
                sp[k][1] = min(audio_len, sp[k][1] + pad)
                sp[k + 1][0] = max(0, sp[k + 1][0] - pad)
        else:
            sp[k][1] = min(audio_len, sp[k][1] + pad)
    return [(a, b) for a, b in sp]


def segment_times(segs) -> list:
    """the ABI's t0 / t1 of the segments: 10 ms units as f32"""
    return [(np.float32(np.float32(a) / np.float32(160.0)), np.float32(np.float32(b) / np.float32(160.0))) for a, b in segs]


def piece_table(segs, n_samples: int, samples_overlap: float) -> list:
    """[(orig_start, orig_end, vad_start, vad_end)] in samples: segment k is copied as [s_k, min(e_k + overlap, s_{k+1})),
    the last as [s_k, e_k), every end clamped to the audio; pieces lie end to end with GAP zeros between them"""
    with np.errstate(over="ignore", invalid="ignore"):
        ov = np.float32(samples_overlap) * np.float32(SR)   # negative or not finite: none; huge: 2^30 samples
    overlap = 0 if not np.isfinite(ov) or ov <= 0 else 2 ** 30 if ov >= 2 ** 30 else int(ov)
    out = []
    pos = 0
    for k, (s, e) in enumerate(segs):
        s = min(s, n_samples)
        e = min(e, n_samples)
        if k + 1 < len(segs):
            e = min(e + overlap, min(segs[k + 1][0], n_samples))
        if e <= s:
            continue
        if out:
            pos += GAP
        out.append((s, e, pos, pos + (e - s)))
        pos += e - s
    return out


def filtered_len(table) -> int:
    return table[-1][3] if table else 0


def filtered_pcm(pcm, table):
    out = np.zeros(filtered_len(table), dtype=np.float32)
    for s, e, vs, ve in table:
        out[vs:ve] = pcm[s:e]
    return out


def map_time(table, t: int) -> int:
    """a time on the filtered axis (10 ms units) back to the original axis"""
    if not table:
        return t
    x = t * 160
    orig = table[0][0]
    for s, e, vs, ve in table:
        if x < vs:
            break            # in the gap before this piece: the end of the piece before (set below)
        orig = s + (x - vs) if x < ve else e
    return orig // 160
