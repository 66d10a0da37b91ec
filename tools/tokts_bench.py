#!/usr/bin/env python3
"""What token_timestamps costs: a batch of 30 s clips through whisper_mi355x_full_batch with the switch
off and on, interleaved in one process after warm-up calls of both; per call the host wall time (the call ends in a
stream synchronise), whisper_mi355x_token_times_ms, and from further event-timed calls the class-15 kernel time: of an
ordinary call, and of a call that stops after language detection, whose only class-15 launch is the energy kernel.

    python tools/tokts_bench.py [--shape tiny+conf] [--clips 32] [--repeats 5] [--energy-clips 128] [--max-len 0]

Prints one JSON line per leg and a summary line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from conftest import load_whisper_rs, model_path  # noqa: E402
from make_model import synthetic_pcm              # noqa: E402

K_TOKTS = 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tiny+conf")
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--energy-clips", type=int, default=128)
    ap.add_argument("--max-len", type=int, default=0)
    a = ap.parse_args()
    wrs = load_whisper_rs()
    L = wrs.lib()
    base = [synthetic_pcm(k) for k in range(20)]
    clips = [base[k % 20] for k in range(a.clips)]
    ctx = wrs.WhisperContext(model_path(a.shape))
    st = ctx.create_state()

    def call(on, pcm=clips, mask=0, detect=False):
        p = wrs.reference_full_params("en")
        p.token_timestamps = on
        p.max_len = a.max_len
        p.detect_language = detect
        L.whisper_mi355x_kernel_timing(st.ptr, mask)
        t = time.perf_counter()
        rc = st.full_batch(p, pcm)
        wall = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        out = (C.c_double * 3)()
        L.whisper_mi355x_kernel_stats(st.ptr, K_TOKTS, out)
        return dict(on=on, wall_ms=wall, token_times_ms=st.token_times_ms(), k15_ms=out[0], k15_launches=int(out[1]), k15_bytes=out[2],
                    segments=sum(L.whisper_mi355x_batch_n_segments(st.ptr, j) for j in range(len(pcm))))

    for on in (False, True, False, True):  # warm-up: graphs, code objects, the energy buffers
        call(on)
    legs = {False: [], True: []}
    for _ in range(a.repeats):
        for on in (False, True):
            r = call(on)
            legs[on].append(r)
            print(json.dumps(r))
    timed = call(True, mask=1 << K_TOKTS)
    print(json.dumps(dict(timed, leg="event-timed call")))
    big = [base[k % 20] for k in range(a.energy_clips)]
    call(True, pcm=big, detect=True)
    e = call(True, pcm=big, mask=1 << K_TOKTS, detect=True)
    print(json.dumps(dict(e, leg="energy kernel alone", clips=a.energy_clips)))
    off = statistics.median(r["wall_ms"] for r in legs[False])
    on_ = statistics.median(r["wall_ms"] for r in legs[True])
    print(json.dumps(dict(shape=a.shape, clips=a.clips, repeats=a.repeats, wall_off_ms=off, wall_on_ms=on_, ratio=on_ / off,
                          wall_off_all=[round(r["wall_ms"], 2) for r in legs[False]],
                          wall_on_all=[round(r["wall_ms"], 2) for r in legs[True]],
                          token_times_ms=statistics.median(r["token_times_ms"] for r in legs[True]),
                          k15_ms=timed["k15_ms"], k15_launches=timed["k15_launches"],
                          energy_ms=e["k15_ms"], energy_launches=e["k15_launches"],
                          energy_GBps=e["k15_bytes"] / max(e["k15_ms"], 1e-9) / 1e6)))
    st.close()
    ctx.close()


if __name__ == "__main__":
    main()
