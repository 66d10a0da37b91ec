"""The price of whisper_full_params.logits_filter_callback: ms per decode step without a callback and with
a callback that does nothing, and the stage kernel's time against its 8 bytes-per-logit roofline.

    python tools/filter_bench.py [--clips 1,16] [--tokens 64] [--out profiles/filter_bench_<tag>.jsonl]

The benchmark's large-v3 bf16 model (bench.py's default file), synthetic 30 s clips, greedy, one window per clip
(single_segment), max_tokens = 64, t = 0 only. The callback is a ctypes no-op: a Python function behind a CFUNCTYPE
trampoline that returns at once, so the callback column is an upper bound on what a compiled callback would pay. Its own
cost is measured apart (the trampoline called from C in a tight loop is not
possible without a compiled caller, so the figure is the interpreter's: the function called through ctypes from Python)
and printed beside the step times, so that a reader can subtract it. Per configuration: one warm-up call, then 3 calls;
the median call's decode time over its steps. Kernel times come from a fourth, event-timed call (timing changes the
wall time, so it is not one of the three). One JSON line per configuration.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_TBS = 6.29  # measured float4 copy rate of an MI355X (the roofline's denominator)
K_LOGITS, K_STAGE = 5, 18


def main():
    import bench
    from make_model import synthetic_pcm
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="1,16")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    wrs = bench.load_wrs()
    L = wrs.lib()
    ctx = wrs.WhisperContext(bench.prepare_default_model(), dtype=wrs.BF16)
    V = L.whisper_n_vocab(ctx.ptr)
    noop = wrs.LOGITS_FILTER_CALLBACK(lambda *a: None)
    loops = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(20000):
            noop(None, None, None, 0, None, None)
        loops.append((time.perf_counter() - t0) / 20000 * 1e6)
    tramp_us = statistics.median(loops)
    lines = []
    for n in [int(x) for x in args.clips.split(",")]:
        pcm = [synthetic_pcm(k) for k in range(n)]
        res = dict(clips=n, max_tokens=args.tokens, n_vocab=V, trampoline_us_per_call=round(tramp_us, 2))
        for name, cb in (("plain", None), ("noop_callback", noop)):
            p = wrs.reference_full_params("en")
            p.max_tokens = args.tokens
            p.temperature_inc = 0.0
            p.single_segment = True
            if cb is not None:
                p.logits_filter_callback = C.cast(cb, C.c_void_p)
            st = ctx.create_state()
            per_step = []
            for call in range(4):
                assert st.full_batch(p, pcm) == 0
                ph = (C.c_double * 5)()
                L.whisper_mi355x_phase_ms(st.ptr, ph)
                steps = L.whisper_mi355x_batch_decoded_tokens(st.ptr) / n - 1  # (the prefill decides the first token)
                if call:
                    per_step.append(ph[3] / steps)
            res[name + "_ms_per_step"] = round(statistics.median(per_step), 4)
            res[name + "_steps"] = steps
            L.whisper_mi355x_kernel_timing(st.ptr, (1 << K_LOGITS) | (1 << K_STAGE))
            assert st.full_batch(p, pcm) == 0
            out = (C.c_double * 3)()
            for cls, key in ((K_LOGITS, "logits"), (K_STAGE, "stage")):
                L.whisper_mi355x_kernel_stats(st.ptr, cls, out)
                if out[1]:
                    res[f"{name}_{key}_us"] = round(out[0] / out[1] * 1e3, 2)
                    res[f"{name}_{key}_launches"] = int(out[1])
            st.close()
        res["stage_roofline_us"] = round(n * V * 8 / (HBM_TBS * 1e12) * 1e6, 3)
        print(json.dumps(res), flush=True)
        lines.append(res)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
