"""Pick synthetic_pcm clips for the exact beam-search tests (tests/test_gpu_beam.py), on the CPU.

Runs the numpy reference of the beam-search contract (tests/beam_ref.py) over the CPU oracle's logits for a range of
clips and prints, per clip, the smallest gap that decided anything (pool order, timestamp rule, winner score,
thresholds), the winner and the beams' lengths. The GPU tests use clips whose smallest gap is widest (the engine's f16
logits stay within 0.015 of the oracle's) and assert that the gap over the engine's own logits exceeds
1e-3 nats.

  python tools/beam_pick_clips.py --shape tiny+conf --beams 5 --max-tokens 12 --clips 0 96
  python tools/beam_pick_clips.py --shape tiny+conf+eot23 --beams 5 --max-tokens 24 --no-timestamps --clips 0 18
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def scan(shape: str, beams: int, no_timestamps: bool, max_tokens: int, clips, model_dir: str):
    import beam_ref as br
    from make_model import synthetic_pcm, synthetic_vocab, write_model
    from oracle_py import Oracle

    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, f"{shape}_s0.bin")
    if not os.path.exists(path):
        write_model(path, shape, 0)
    o = Oracle(path, mode=1, n_threads=16)
    vid = br.vocab_ids(o.n_vocab, synthetic_vocab().index(b" "))
    sot = o.token("sot")
    prompt = [sot, sot + 1, o.token("transcribe")] + ([o.token("not")] if no_timestamps else [])
    for clip in clips:
        t0 = time.time()
        o.new_state()
        _, n_org = o.mel(synthetic_pcm(clip))
        o.encode(0)
        cache = {}

        def logits_fn(prefix):
            if prefix not in cache:
                o.kv_clear()
                cache[prefix] = o.decode(prompt + list(prefix), 0)[-1].copy()
            return cache[prefix]

        params = br.Params(K=beams, max_tokens=max_tokens, single_segment=True, no_timestamps=no_timestamps,
                           seek_end=n_org, n_max=o.n_text_ctx // 2 - 4, n_audio_ctx=o.n_audio_ctx)
        r = br.beam_search(logits_fn, params, vid, n_prompt=len(prompt))
        what, gap = min(r.gaps, key=lambda g: g[1])
        print(f"{shape} K{beams} clip {clip}: min gap {gap:.4f} ({what}), winner {r.winner}, "
              f"lengths {[len(b['tokens']) for b in r.beams]}, copies {sum(len(c) for c in r.copies)}, "
              f"{time.time() - t0:.1f}s", flush=True)
    o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tiny+conf")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--max-tokens", type=int, default=12)
    ap.add_argument("--no-timestamps", action="store_true")
    ap.add_argument("--clips", type=int, nargs=2, default=[0, 16], metavar=("FIRST", "END"))
    ap.add_argument("--model-dir", default=os.environ.get("NW_MODEL_DIR", "/tmp/nw_models"))
    args = ap.parse_args()
    scan(args.shape, args.beams, args.no_timestamps, args.max_tokens, range(*args.clips), args.model_dir)


if __name__ == "__main__":
    main()
