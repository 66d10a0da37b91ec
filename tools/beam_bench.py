"""Beam-search step time on the flagship model, beside the greedy step over as many rows.

large-v3 (synthetic +conf weights, the file bench.py's default run uses), one 30 s clip, beam_size K (default 5),
max_tokens 64, one window: ms per decode step, the per-class kernel times of a timed run (classes 2 cross attention,
3 self attention, 4 decoder GEMMs, 5 greedy logits, 12 top-k logits, 13 self-cache gather), and the bytes the gather
moved with the common-prefix rule and what whole-sequence copies would have moved. Next to it the greedy strategy
over K clips (the same layer kernels over K rows), with and without the pipelined decoding, since beam steps wait for
the host's re-parenting after every step.

  python tools/beam_bench.py [--beams 5] [--dtype bf16] [--reps 3]
Prints one JSON line per leg.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLASSES = {2: "cross_attn", 3: "self_attn", 4: "dec_gemm", 5: "logits", 12: "topk", 13: "kv_gather"}
KSTAT_BEAM_GATHER = 101


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=64)
    ap.add_argument("--greedy-only", action="store_true", help="only the greedy legs (a tree without the beam strategy)")
    args = ap.parse_args()
    import ctypes as C
    import bench
    from make_model import synthetic_pcm
    wrs = bench.load_wrs()
    path = bench.prepare_default_model()
    ctx = wrs.WhisperContext(path, dtype=wrs.BF16 if args.dtype == "bf16" else wrs.F16)
    L = wrs.lib()
    K = args.beams
    pcm = [synthetic_pcm(i) for i in range(K)]

    def params(beam):
        p = wrs.beam_full_params(K, "en") if beam else wrs.reference_full_params("en")
        p.temperature_inc = 0.0
        p.single_segment = True
        p.max_tokens = args.max_tokens
        return p

    def leg(name, beam, clips, env=None):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            st = ctx.create_state()
            run = (lambda: st.full_batch(params(beam), clips)) if len(clips) > 1 else (lambda: st.full(params(beam), clips[0]))
            assert run() == 0  # warm-up: workspace, graphs
            ms = []
            for _ in range(args.reps):
                t = time.perf_counter()
                assert run() == 0
                wall = (time.perf_counter() - t) * 1e3
                ms.append((st.phase_ms()["decode"], wall))
            if beam:
                steps = max(len(b["tokens"]) for b in st.beam_info(0)) - 1
                rows = sum(len(b["tokens"]) - 1 for b in st.beam_info(0))
            else:
                n_tok = [sum(len(s.tokens) for s in st.batch_segments(j)) for j in range(len(clips))] if len(clips) > 1 else \
                    [sum(len(s.tokens) for s in st.segments())]
                steps, rows = max(n_tok) - 1, sum(n_tok) - len(n_tok)
            g0 = (C.c_double * 3)()
            if beam:
                L.whisper_mi355x_kernel_stats(st.ptr, KSTAT_BEAM_GATHER, g0)
            mask = sum(1 << c for c in CLASSES)
            L.whisper_mi355x_kernel_timing(st.ptr, mask)
            assert run() == 0
            kern = {}
            for c, nm in CLASSES.items():
                out = (C.c_double * 3)()
                L.whisper_mi355x_kernel_stats(st.ptr, c, out)
                kern[nm] = dict(ms=round(out[0], 3), launches=int(out[1]), work=out[2])
            L.whisper_mi355x_kernel_timing(st.ptr, 0)
            g1 = (C.c_double * 3)()
            if beam:
                L.whisper_mi355x_kernel_stats(st.ptr, KSTAT_BEAM_GATHER, g1)
            st.close()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        dec = sorted(m[0] for m in ms)[len(ms) // 2]
        rec = dict(leg=name, dtype=args.dtype, clips=len(clips), beams=K if beam else 0, decode_steps=steps, row_steps=rows,
                   decode_ms=[round(m[0], 2) for m in ms], wall_ms=[round(m[1], 2) for m in ms],
                   ms_per_step=round(dec / max(1, steps), 4), kernels_timed_run=kern)
        if beam:
            rec["gather_bytes_per_call"] = g1[0] - g0[0]
            rec["gather_bytes_whole_sequences"] = g1[1] - g0[1]
            rec["gather_bytes_per_step"] = round((g1[0] - g0[0]) / max(1, steps))
            rec["gather_bytes_per_step_whole_sequences"] = round((g1[1] - g0[1]) / max(1, steps))
        print(json.dumps(rec), flush=True)

    if not args.greedy_only:
        leg(f"beam K={K}, 1 clip", True, pcm[:1])
    leg(f"greedy, {K} clips", False, pcm)
    leg(f"greedy, {K} clips, per-step (no pipelining)", False, pcm, {"WHISPER_MI355X_PIPE": "0"})
    leg("greedy, 1 clip", False, pcm[:1])
    ctx.close()


if __name__ == "__main__":
    main()
