#!/usr/bin/env python3
"""What whisper_full_params.audio_ctx buys on the app's call pattern: one 25.2 s chunk per call on a
fresh whisper_state (the context's state pool on), f16, language "auto", initial prompt = the default vocabulary + the
previous chunk's text (bench.py app_pattern's calls, made through whisper_full_with_state so that audio_ctx can be
set). Per audio_ctx: the median host wall time per call after the first, and the call's phase times.

    python tools/audio_ctx_bench.py [--shape base+conf] [--model-dir DIR] [--calls 6] [--ctx 0,1260,750,375] [--lang auto]

--lang auto is the app's setting: whisper_full detects the language at the full context before it applies audio_ctx, so a
call with audio_ctx < n_audio_ctx encodes window 0 twice. --lang en shows the encoder pass at audio_ctx alone.

The values are interleaved call by call (chunk k at every audio_ctx before chunk k + 1), each with its own chain of
previous texts. Prints one JSON line per audio_ctx."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from conftest import MODEL_DIR, load_whisper_rs  # noqa: E402
from make_model import synthetic_pcm, write_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="base+conf")
    ap.add_argument("--model-dir", default=MODEL_DIR)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--ctx", default="0,1260,750,375")
    ap.add_argument("--lang", default="auto")
    a = ap.parse_args()
    wrs = load_whisper_rs()
    L = wrs.lib()
    os.makedirs(a.model_dir, exist_ok=True)
    path = os.path.join(a.model_dir, f"{a.shape}_s0.bin")
    if not os.path.exists(path):
        write_model(path, a.shape, 0)
    ctxs = [int(x) for x in a.ctx.split(",")]
    chunks = [synthetic_pcm(100 + k, seconds=25.2) for k in range(a.calls)]
    ctx = wrs.WhisperContext(path, dtype=wrs.F16)
    last = {A: None for A in ctxs}
    rows = {A: [] for A in ctxs}
    for x in chunks:
        for A in ctxs:
            p = wrs.reference_full_params(None if a.lang == "auto" else a.lang, wrs.build_initial_prompt(wrs.DEFAULT_VOCABULARY, last[A]))
            p.audio_ctx = A
            k0 = L.whisper_mi355x_decoded_tokens_total()
            t = time.perf_counter()
            st = ctx.create_state()
            rc = st.full(p, x)
            text = b"".join(s.text for s in st.segments()).decode("utf-8", "replace").strip()
            wall = (time.perf_counter() - t) * 1e3
            ph = st.phase_ms()
            st.close()
            assert rc == 0, rc
            last[A] = wrs.filter_hallucinations(text) or None
            rows[A].append(dict(wall_ms=wall, tokens=L.whisper_mi355x_decoded_tokens_total() - k0, **ph))
    ctx.close()
    for A in ctxs:
        steady = rows[A][1:] or rows[A]
        med = {k: round(statistics.median(r[k] for r in steady), 2) for k in ("wall_ms", "mel", "encode", "prefill", "decode", "logits")}
        print(json.dumps(dict(shape=a.shape, lang=a.lang, audio_ctx=A, calls=a.calls, first_call_ms=round(rows[A][0]["wall_ms"], 1), median=med,
                              encode_share=round(med["encode"] / med["wall_ms"], 3),
                              tokens_per_call=[r["tokens"] for r in rows[A]],
                              wall_ms_per_call=[round(r["wall_ms"], 1) for r in rows[A]])))


if __name__ == "__main__":
    main()
