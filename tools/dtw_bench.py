#!/usr/bin/env python3
"""Cost of token-level DTW timestamps on the flagship batch: large-v3 bf16, 128 x 30 s clips resident in HBM,
fixed work (fixed_tokens = 128), alignment heads preset LARGE_V3. Runs the batch with DTW off and on (one
context each, same clips, same process) and prints one JSON line: the phase clocks of both, align_ms and its
per-kernel split (score / cost / DTW kernels, event-timed in a step of their own), the share of the step.

    python tools/dtw_bench.py [--clips 128] [--tokens 128] [--steps 2] [--warmup 1] [--preset LARGE_V3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the flagship benchmark's model file, clip synthesis and binding loader)

K_ALIGN = {"scores": 9, "cost": 10, "dtw": 11}  # whisper_mi355x_kernel_timing classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--preset", default="LARGE_V3")
    args = ap.parse_args()

    wrs = bench.load_wrs()
    L = wrs.lib()
    shape = bench.model_shape(args.model)
    path = os.path.join(bench.MODEL_DIR, f"{shape}_s0.bin")
    os.makedirs(bench.MODEL_DIR, exist_ok=True)
    chunks = bench.start_chunks(list(range(args.clips)))
    bench.ensure_model(path, shape)
    host = [f.result() for f in chunks]
    n = 16000 * 30
    params = wrs.reference_full_params("en")
    out = dict(model=shape, dtype=args.dtype, clips=args.clips, fixed_tokens=args.tokens, preset=args.preset)
    for mode in ("off", "on"):
        kw = dict(dtw_preset=args.preset) if mode == "on" else {}
        ctx = wrs.WhisperContext(path, dtype=wrs.BF16 if args.dtype == "bf16" else wrs.F16, **kw)
        st = ctx.create_state()
        buf = L.whisper_mi355x_dev_alloc(ctx.ptr, args.clips * n * 4)
        assert buf
        for i, h in enumerate(host):
            assert len(h) == n
            L.whisper_mi355x_memcpy(ctx.ptr, C.c_void_p(buf + i * n * 4), h.ctypes.data, n * 4, 1)
        jobs = [(buf + i * n * 4, n) for i in range(args.clips)]

        def step():
            rc = st.full_batch(params, jobs, on_device=True, fixed_tokens=args.tokens)
            assert rc == 0, rc

        for _ in range(args.warmup):
            step()
        ph = {k: 0.0 for k in ("mel", "encode", "prefill", "decode", "logits")}
        align = 0.0
        t0 = time.time()
        for _ in range(args.steps):
            step()
            for k, v in st.phase_ms().items():
                ph[k] += v / args.steps
            align += st.align_ms() / args.steps
        wall = (time.time() - t0) / args.steps * 1e3
        rec = dict(step_ms=round(wall, 1), phases_ms={k: round(v, 1) for k, v in ph.items()}, align_ms=round(align, 1),
                   audio_s_per_s=round(args.clips * 30.0 / (wall / 1e3), 1))
        if mode == "on":
            # the three alignment kernels, event-timed in one more step (the events serialise nothing: one stream)
            L.whisper_mi355x_kernel_timing(st.ptr, sum(1 << k for k in K_ALIGN.values()))
            step()
            split = {}
            for name, k in K_ALIGN.items():
                o = (C.c_double * 3)()
                L.whisper_mi355x_kernel_stats(st.ptr, k, o)
                split[name] = dict(ms=round(o[0], 3), launches=int(o[1]))
            L.whisper_mi355x_kernel_timing(st.ptr, 0)
            rec["align_kernels"] = split
            rec["align_ms_timed_step"] = round(st.align_ms(), 1)
            n_tok = sum(1 for seg in st.token_times(0) for _, t in seg if t >= 0)
            rec["aligned_tokens_clip0"] = n_tok
        out[mode] = rec
        L.whisper_mi355x_dev_free(ctx.ptr, C.c_void_p(buf))
        st.close()
        ctx.close()
    out["align_share_of_step"] = round(out["on"]["align_ms"] / max(1e-9, out["on"]["step_ms"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
