"""On-path cost of the deny mask: the logits kernels' time per launch with and without a mask, read
through whisper_mi355x_kernel_timing (K_LOGITS, K_TOPK) over whole calls.

Greedy fixed-work runs of 1, 16 and 128 clips (the split form up to 16 rows, one workgroup per row above) and beam
search with 2 beams over 1, 8 and 16 clips (2, 16 and 32 rows: the engine's beam steps stop at 32 rows), each with no
mask, with a mask of about 1 % of the vocabulary in LDS, and with the same mask read through the cache
(WHISPER_MI355X_DENY_GLOBAL=1). A context per configuration, so no captured step is reused. One JSON line per
configuration: us per launch (median of --reps runs) and the launches counted.

  python tools/suppress_bench.py --shape tiny+conf --tokens 32 --reps 5
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

K_LOGITS, K_TOPK = 5, 12
PATTERN = " [a-z][a-z]"  # 676 of the synthetic vocabulary's tokens: 1.3 %


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tiny+conf")
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from conftest import load_whisper_rs, model_path
    from make_model import synthetic_pcm

    wrs = load_whisper_rs()
    L = wrs.lib()
    path = model_path(args.shape)
    pcms = [synthetic_pcm(k) for k in range(8)]

    def measure(mode, n_clips, beams):
        os.environ.pop("WHISPER_MI355X_DENY_GLOBAL", None)
        if mode == "cache":
            os.environ["WHISPER_MI355X_DENY_GLOBAL"] = "1"
        ctx = wrs.WhisperContext(path, dtype=wrs.F16)
        st = ctx.create_state()
        cls = K_TOPK if beams else K_LOGITS
        if beams:
            p = wrs.beam_full_params(beams, "en")
            p.temperature_inc = 0.0
            p.single_segment = True
            p.max_tokens = args.tokens
        else:
            p = wrs.reference_full_params("en")
        p.suppress_regex = None if mode == "none" else PATTERN.encode()
        clips = [pcms[k % len(pcms)] for k in range(n_clips)]
        us, count = [], 0
        for rep in range(args.reps + 1):  # (the first run captures the step graphs)
            L.whisper_mi355x_kernel_timing(st.ptr, 0)
            L.whisper_mi355x_kernel_timing(st.ptr, 1 << cls)
            assert st.full_batch(p, clips, fixed_tokens=0 if beams else args.tokens) == 0
            out = (C.c_double * 3)()
            L.whisper_mi355x_kernel_stats(st.ptr, cls, out)
            if rep and out[1] > 0:
                us.append(1e3 * out[0] / out[1])
                count = int(out[1])
        if mode != "none":
            assert ctx.suppress_mask(False, PATTERN).sum() == 676
        st.close()
        ctx.close()
        print(json.dumps(dict(kernel="topk" if beams else "logits", rows=n_clips * max(1, beams), mask=mode,
                              us_per_launch=round(statistics.median(us), 3), us_min=round(min(us), 3), launches=count)), flush=True)

    for beams, sizes in ((0, (1, 16, 128)), (2, (1, 8, 16))):
        for n in sizes:
            for mode in ("none", "lds", "cache"):
                measure(mode, n, beams)


if __name__ == "__main__":
    main()
