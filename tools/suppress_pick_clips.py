"""Pick synthetic_pcm clips for the exact suppress test (tests/test_gpu_suppress.py test_banned_run_is_the_reference), on
the CPU.

Over the CPU oracle's logits: the plain fixed-work greedy run of every clip, the 8 most frequent text tokens of those
runs as the ban, then the banned greedy run step by step through tests/suppress_ref.py. Prints per clip the steps whose
reference decision has a gap under logits_cases.MIN_GAP; the GPU test takes clips with at most 2 such steps of 24 (the
engine's f16 logits stay within 0.015 of the oracle's) and asserts the cap over the engine's own logits.

  python tools/suppress_pick_clips.py --shape tiny+conf --tokens 24 --clips 0 5
"""
import argparse
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def scan(shape: str, n_tok: int, clips, model_dir: str):
    import numpy as np

    import logits_cases as lc
    import logits_ref as lr
    import suppress_cases as sc
    import suppress_ref as sr
    from make_model import synthetic_pcm, write_model
    from oracle_py import Oracle

    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, f"{shape}_s0.bin")
    if not os.path.exists(path):
        write_model(path, shape, 0)
    o = Oracle(path, mode=1, n_threads=16)
    v = lc.vocab(o.n_vocab)
    sot = o.token("sot")
    prompt = [sot, sot + 1, o.token("transcribe")]

    def run(clip, deny):
        o.new_state()
        o.mel(synthetic_pcm(clip))
        o.encode(0)
        o.kv_clear()
        row = o.decode(prompt, 0)[-1]
        c = lr.ctl(is_initial=1, penult_ts=1, suppress_blank=1, tid0_initial=50, suppress_eot=1)
        ints = np.zeros(5, np.int64)
        toks, low = [], []
        for i in range(n_tok):
            ref = sr.process(row, c, v, deny)
            if not sc.decided(ref):
                low.append(i)
            toks.append(ref["id"])
            c = lr.advance(c, ints, 1, 0, ref["id"], v["beg"])
            if i + 1 < n_tok:
                row = o.decode([ref["id"]], len(prompt) + i)[-1]
        return toks, low

    none = np.zeros(o.n_vocab, bool)
    plain = {clip: run(clip, none)[0] for clip in clips}
    cnt = Counter(t for toks in plain.values() for t in toks if t < v["eot"])
    ids = [i for i, _ in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))[:8]]
    deny = none.copy()
    deny[ids] = True
    print(f"{shape}: ban {ids} = {[o.token_str(i) for i in ids]}")
    for clip in clips:
        toks, low = run(clip, deny)
        diff = sum(a != b for a, b in zip(toks, plain[clip]))
        print(f"{shape} clip {clip}: steps under the gap {low}, {diff} of {n_tok} tokens differ from the plain run", flush=True)
    o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tiny+conf")
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--clips", type=int, nargs=2, default=[0, 5], metavar=("FIRST", "END"))
    ap.add_argument("--model-dir", default=os.environ.get("NW_MODEL_DIR", "/tmp/nw_models"))
    args = ap.parse_args()
    scan(args.shape, args.tokens, range(*args.clips), args.model_dir)


if __name__ == "__main__":
    main()
