#!/usr/bin/env python3
"""What whisper_full_params.vad costs. Two legs, each in a child process under its own time limit:

  batch: --clips 30 s clips through whisper_mi355x_full_batch with vad on (the "gate" model of tools/make_vad_model.py):
         whisper_mi355x_vad_ms, class 17 by kernel (frontend, lstm, gather) from further event-timed calls, and the same
         clips' encode time with vad off (whisper_mi355x_phase_ms), of which the filter step is reported as a share
  long:  one --seconds clip through whisper_full with vad on and nothing to decode: whisper_mi355x_vad_ms, the split,
         and the lstm kernel's time per step

    python tools/vad_bench.py [--shape tiny+conf | --model PATH] [--dtype f16|bf16] [--clips 128] [--seconds 3600] [--repeats 3]

Prints one JSON line per leg."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

K_VAD = 17


def vad_params(wrs, vad_path, **kw):
    p = wrs.reference_full_params("en")
    p.temperature_inc = 0.0
    if vad_path:
        p.vad, p.vad_model_path = True, vad_path.encode()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def split_ms(st):
    return {k: v[0] for k, v in st.vad_kernel_stats().items()}


def leg_batch(a, wrs, vad_path):
    from conftest import model_path
    from make_model import synthetic_pcm
    L = wrs.lib()
    base = [synthetic_pcm(k) for k in range(20)]
    clips = [base[k % 20] for k in range(a.clips)]
    ctx = wrs.WhisperContext(a.model or model_path(a.shape), dtype=wrs.BF16 if a.dtype == "bf16" else wrs.F16)
    st = ctx.create_state()

    def call(vad, mask=0):
        L.whisper_mi355x_kernel_timing(st.ptr, mask)
        t = time.perf_counter()
        rc = st.full_batch(vad_params(wrs, vad_path if vad else None), clips)
        wall = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        kept = sum(t[-1][3] if t else 0 for t in (st.vad_map(j) for j in range(len(clips)))) if vad else None
        return dict(vad=vad, wall_ms=wall, vad_ms=st.vad_ms(), split_ms=split_ms(st), phases_ms=st.phase_ms(), kept_samples=kept)

    call(False), call(True)   # warm-up: graphs, code objects, the buffers
    on = [call(True) for _ in range(a.repeats)]
    off = [call(False) for _ in range(a.repeats)]
    timed = [call(True, mask=1 << K_VAD) for _ in range(a.repeats)]   # class 17 alone: the split by kernel
    med = lambda rows, f: statistics.median(f(r) for r in rows)
    enc_off = med(off, lambda r: r["phases_ms"]["encode"])
    vad_ms = med(on, lambda r: r["vad_ms"])
    total = sum(len(c) for c in clips)
    print(json.dumps(dict(leg="batch", clips=a.clips, model=a.model or a.shape, dtype=a.dtype, vad_ms=round(vad_ms, 3),
                          split_ms={k: round(med(timed, lambda r: r["split_ms"][k]), 3) for k in ("frontend", "lstm", "gather")},
                          lstm_us_per_step=round(1e3 * med(timed, lambda r: r["split_ms"]["lstm"]) / max(1, max((len(c) + 511) // 512 for c in clips)), 4),
                          encode_ms_vad_off=round(enc_off, 2), encode_ms_vad_on=round(med(on, lambda r: r["phases_ms"]["encode"]), 2),
                          vad_share_of_encode_off=round(vad_ms / max(enc_off, 1e-9), 4),
                          wall_ms_vad_off=round(med(off, lambda r: r["wall_ms"]), 1), wall_ms_vad_on=round(med(on, lambda r: r["wall_ms"]), 1),
                          kept_fraction=round(on[0]["kept_samples"] / total, 4))))
    st.close()
    ctx.close()


def leg_long(a, wrs, vad_path):
    """one long clip through whisper_full with vad on and an offset_ms beyond its end: the filter step runs (and the mel
    of the filtered audio), nothing is encoded or decoded"""
    import numpy as np
    from conftest import model_path
    from make_model import synthetic_pcm
    L = wrs.lib()
    x = np.tile(synthetic_pcm(0), int(a.seconds // 30) + 1)[:int(a.seconds * 16000)]
    ctx = wrs.WhisperContext(model_path("tiny+conf"))
    st = ctx.create_state()
    rows = []
    for _ in range(a.repeats + 1):
        L.whisper_mi355x_kernel_timing(st.ptr, 1 << K_VAD)
        assert st.full(vad_params(wrs, vad_path, offset_ms=int(a.seconds * 1000) + 60000), x) == 0
        rows.append(dict(vad_ms=st.vad_ms(), **split_ms(st)))
    rows = rows[1:]
    steps = (len(x) + 511) // 512
    med = lambda k: statistics.median(r[k] for r in rows)
    print(json.dumps(dict(leg="long", seconds=a.seconds, steps=steps, vad_ms=round(med("vad_ms"), 2), frontend_ms=round(med("frontend"), 3),
                          lstm_ms=round(med("lstm"), 3), gather_ms=round(med("gather"), 3), lstm_us_per_step=round(1e3 * med("lstm") / steps, 4))))
    st.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tiny+conf")
    ap.add_argument("--model", default=None, help="a Whisper model file instead of a synthetic shape")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg", default=None, choices=["batch", "long"])
    ap.add_argument("--vad-model", default=None)
    ap.add_argument("--leg-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.leg is None:
        from make_vad_model import write_vad_model
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "gate.bin")
            write_vad_model(path, "gate", 0)
            for leg in ("batch", "long"):  # a fresh process per leg, each under its own limit; a leg that fails ends the run
                argv = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--vad-model", path] + \
                    [x for x in sys.argv[1:]]
                r = subprocess.run(["timeout", "-k", "10", str(a.leg_timeout)] + argv)
                if r.returncode != 0:
                    sys.exit(r.returncode)
        return
    from conftest import load_whisper_rs
    wrs = load_whisper_rs()
    (leg_batch if a.leg == "batch" else leg_long)(a, wrs, a.vad_model)


if __name__ == "__main__":
    main()
