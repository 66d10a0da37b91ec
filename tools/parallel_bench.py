#!/usr/bin/env python3
"""What whisper_full_parallel gains on one long recording: audio-s/s of whisper_full and of
whisper_full_parallel(n) on one synthetic clip (--minutes of 30 s synthetic chunks laid end to end) on the benchmark's
model. One greedy attempt per window (temperature_inc = 0) of at most --tokens tokens (max_tokens; the benchmark's
fixed-work mode decodes 128 per window), so that every call decodes the same kind of work.

    python tools/parallel_bench.py [--model PATH | --shape large-v3+conf] [--dtype bf16|f16] [--minutes 10] [--n 4,20,64]
                                   [--tokens 128] [--snap-ms 0] [--repeats 2]

Before whisper_full_parallel was implemented it was whisper_full: the first line is that yardstick. Prints one JSON line
per call kind."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=None)
    ap.add_argument("--shape", default=None, help="a tools/make_model.py shape (default: bench.py's default model file)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--n", default="4,20,64")
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--snap-ms", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    from conftest import load_whisper_rs, model_path
    from make_model import synthetic_pcm
    wrs = load_whisper_rs()
    if a.model:
        path = a.model
    elif a.shape:
        path = model_path(a.shape)
    else:
        import bench
        path = bench.prepare_default_model()
    n_chunks = max(1, int(round(a.minutes * 2)))
    pcm = np.concatenate([synthetic_pcm(k) for k in range(n_chunks)]).astype(np.float32)
    seconds = len(pcm) / 16000.0
    ctx = wrs.WhisperContext(path, dtype=wrs.BF16 if a.dtype == "bf16" else wrs.F16)
    st = ctx.create_state()

    def params():
        p = wrs.reference_full_params("en")
        p.temperature_inc = 0.0
        p.no_context = True           # every call starts as the first one did
        p.max_tokens = a.tokens - 1
        return p

    def timed(call):
        call()                        # warm-up: graphs, code objects, the buffers
        walls = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            rc = call()
            walls.append(time.perf_counter() - t)
            assert rc == 0, rc
        return statistics.median(walls)

    def line(kind, n, wall):
        dec = st.decisions()
        print(json.dumps(dict(call=kind, n_processors=n, model=os.path.basename(path), dtype=a.dtype, audio_s=round(seconds, 1),
                              wall_s=round(wall, 3), audio_s_per_s=round(seconds / wall, 1), windows=len(dec),
                              segments=st.full_n_segments(), decoded_tokens=int(wrs.lib().whisper_mi355x_batch_decoded_tokens(st.ptr)),
                              phases_ms={k: round(v, 1) for k, v in st.phase_ms().items()}, snap_ms=a.snap_ms if n > 1 else 0)), flush=True)

    line("whisper_full", 1, timed(lambda: st.full(params(), pcm)))
    for n in [int(x) for x in a.n.split(",") if x]:
        line("whisper_full_parallel", n, timed(lambda: st.mi355x_full_parallel(params(), pcm, n, a.snap_ms)))
    st.close()
    ctx.close()


if __name__ == "__main__":
    main()
