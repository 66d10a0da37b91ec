"""Sampled-step time on the flagship model: the host-sampled fallback attempt (best_of = 1) beside the
device-drawn candidates (best_of = N).

large-v3 (synthetic +conf weights, the file bench.py's default run uses), one 30 s clip, a forced fallback
(logprob_thold = 0, temperature_inc = 0.6: attempts at t = 0 and t = 0.6), max_tokens 64, one window. Per leg: the wall
time of the call, the decode phase's ms, the sampled attempt's steps (from the candidates / the segment), ms per sampled
step = (decode ms of the call - decode ms of the same call without fallback) / steps, and the per-class kernel times of a
timed run (5 logits, 14 the sampled draw: us per row = ms / rows).

  python tools/bestof_bench.py [--best-of 5] [--dtype bf16] [--reps 3]
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

CLASSES = {2: "cross_attn", 3: "self_attn", 4: "dec_gemm", 5: "logits", 14: "sample"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--best-of", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=64)
    args = ap.parse_args()
    import ctypes as C
    import bench
    from make_model import synthetic_pcm
    wrs = bench.load_wrs()
    path = bench.prepare_default_model()
    ctx = wrs.WhisperContext(path, dtype=wrs.BF16 if args.dtype == "bf16" else wrs.F16)
    L = wrs.lib()
    pcm = synthetic_pcm(0)

    def params(best_of, fallback):
        p = wrs.reference_full_params("en")
        p.greedy.best_of = best_of
        p.single_segment = True
        p.max_tokens = args.max_tokens
        p.no_speech_thold = 1.0
        if fallback:
            p.temperature_inc = 0.6
            p.logprob_thold = 0.0
        else:
            p.temperature_inc = 0.0
        return p

    def timed(st, p):
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            assert st.full(p, pcm) == 0
            ms.append(((time.perf_counter() - t) * 1e3, st.phase_ms()["decode"]))
        return sorted(ms, key=lambda m: m[1])[len(ms) // 2]

    def leg(name, best_of):
        st = ctx.create_state()
        assert st.full(params(best_of, True), pcm) == 0   # warm-up: workspace, graphs
        assert st.full(params(best_of, False), pcm) == 0
        wall0, dec0 = timed(st, params(best_of, False))
        wall1, dec1 = timed(st, params(best_of, True))
        cands = st.cand_info(0)
        if cands:
            steps = max(len(c["tokens"]) for c in cands) - 1
            rows = sum(len(c["tokens"]) - 1 for c in cands)
        else:
            steps = rows = sum(len(s.tokens) for s in st.segments()) - 1
        L.whisper_mi355x_kernel_timing(st.ptr, sum(1 << c for c in CLASSES))
        assert st.full(params(best_of, True), pcm) == 0
        kern = {}
        for c, nm in CLASSES.items():
            out = (C.c_double * 3)()
            L.whisper_mi355x_kernel_stats(st.ptr, c, out)
            kern[nm] = dict(ms=round(out[0], 4), launches=int(out[1]), work=out[2])
        L.whisper_mi355x_kernel_timing(st.ptr, 0)
        st.close()
        rec = dict(leg=name, dtype=args.dtype, best_of=best_of, candidates=len(cands), sampled_steps=steps, sampled_row_steps=rows,
                   wall_ms=round(wall1, 2), decode_ms=round(dec1, 2), decode_ms_without_fallback=round(dec0, 2),
                   ms_per_sampled_step=round((dec1 - dec0) / max(1, steps), 4), kernels_timed_run=kern)
        if cands and kern["sample"]["launches"]:
            # the first draw of every candidate comes from the prefill row: one launch of len(cands) rows more
            rec["sample_us_per_row"] = round(kern["sample"]["ms"] * 1e3 / (rows + len(cands)), 3)
        print(json.dumps(rec), flush=True)

    leg("best_of 1 (host sampling)", 1)
    leg(f"best_of {args.best_of} (device draws)", args.best_of)
    ctx.close()


if __name__ == "__main__":
    main()
