"""Pick synthetic_pcm clips for the exact grammar test (tests/test_gpu_grammar.py test_grammar_run_is_the_reference), on
the CPU.

Over the CPU oracle's logits: the fixed-work greedy run of every clip under the grammars G2 and G4 of
tests/grammar_cases.py with penalty 100, step by step through tests/grammar_logits_ref.py over the grammar state that
tests/grammar_ref.py reaches from the chosen tokens. Prints per clip and grammar the steps whose reference decision has a
gap under logits_cases.MIN_GAP, and how many tokens differ from the plain run; the GPU test takes clips with no such
step (the engine's f16 logits stay within 0.015 of the oracle's) and asserts a cap of 2 of 24 over the
engine's own logits.

  python tools/grammar_pick_clips.py --shape tiny+conf --tokens 24 --clips 0 8
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def scan(shape: str, n_tok: int, clips, model_dir: str, penalty: float):
    import numpy as np

    import grammar_cases as gc
    import grammar_logits_ref as glr
    import grammar_ref as gr
    import logits_cases as lc
    import logits_ref as lr
    import suppress_cases as sc
    from make_model import synthetic_pcm, write_model
    from oracle_py import Oracle

    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, f"{shape}_s0.bin")
    if not os.path.exists(path):
        write_model(path, shape, 0)
    o = Oracle(path, mode=1, n_threads=16)
    v = lc.vocab(o.n_vocab)
    eot = v["eot"]
    toks = [o.token_str(i) for i in range(o.n_vocab)]
    toks = [t if isinstance(t, bytes) else t.encode() for t in toks]
    sot = o.token("sot")
    prompt = [sot, sot + 1, o.token("transcribe")]
    masks = {}

    def run(clip, grammar):
        o.new_state()
        o.mel(synthetic_pcm(clip))
        o.encode(0)
        o.kv_clear()
        row = o.decode(prompt, 0)[-1]
        c = lr.ctl(is_initial=1, penult_ts=1, suppress_blank=1, tid0_initial=50, suppress_eot=1)
        ints = np.zeros(5, np.int64)
        st = gr.State(*gc.GRAMMARS[grammar]) if grammar else None
        out, low = [], []
        for i in range(n_tok):
            gram = None
            if st is not None and st.stacks:
                key = (grammar, tuple(st.stacks), st.partial)
                if key not in masks:
                    masks[key] = np.array(st.reject(toks, eot))
                gram = masks[key]
            ref = glr.process(row, c, v, None, gram, penalty)
            if not sc.decided(ref):
                low.append(i)
            out.append(ref["id"])
            if st is not None:
                st.accept_token(toks[ref["id"]])
            c = lr.advance(c, ints, 1, 0, ref["id"], v["beg"])
            if i + 1 < n_tok:
                row = o.decode([ref["id"]], len(prompt) + i)[-1]
        return out, low, bool(st is None or st.stacks)

    for clip in clips:
        plain = run(clip, None)[0]
        for g in ("G2", "G4"):
            out, low, alive = run(clip, g)
            diff = sum(a != b for a, b in zip(out, plain))
            print(f"{shape} clip {clip} {g}: steps under the gap {low}, {diff} of {n_tok} tokens differ from the plain run, "
                  f"grammar {'followed' if alive else 'violated'}", flush=True)
    o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tiny+conf")
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--clips", type=int, nargs=2, default=[0, 8], metavar=("FIRST", "END"))
    ap.add_argument("--penalty", type=float, default=100.0)
    ap.add_argument("--model-dir", default=os.environ.get("NW_MODEL_DIR", "/tmp/nw_models"))
    args = ap.parse_args()
    scan(args.shape, args.tokens, range(*args.clips), args.model_dir, args.penalty)


if __name__ == "__main__":
    main()
