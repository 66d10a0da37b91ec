"""Pick synthetic_pcm clips for the exact best_of tests (tests/test_gpu_bestof.py), on the CPU.

Runs the numpy reference of the sampled-draw contract (tests/sample_ref.py) over the CPU oracle's logits
for a range of clips and prints, per clip, the smallest margin of any draw (the distance of a uniform target to the
nearest CDF boundary of the drawn token, as a fraction of the row's mass), the winner, its score's lead over the other
candidates and the candidates' lengths. The GPU tests use clips whose smallest margin is widest and assert that the
margin over the engine's own logits is at least 1.12e-4.

  python tools/bestof_pick_clips.py --shape tiny+conf --best-of 5 --temperature 0.6 --max-tokens 12 --clips 0 16
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def scan(shape: str, best_of: int, temperature: float, temp_idx: int, seed: int, max_tokens: int, clips, model_dir: str):
    import beam_ref as br
    import sample_ref as sr
    from make_model import synthetic_pcm, synthetic_vocab, write_model
    from oracle_py import Oracle

    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, f"{shape}_s0.bin")
    if not os.path.exists(path):
        write_model(path, shape, 0)
    o = Oracle(path, mode=1, n_threads=16)
    vid = br.vocab_ids(o.n_vocab, synthetic_vocab().index(b" "))
    sot = o.token("sot")
    prompt = [sot, sot + 1, o.token("transcribe")]
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

        params = br.Params(K=1, max_tokens=max_tokens, single_segment=True, seek_end=n_org, n_max=o.n_text_ctx // 2 - 4,
                           n_audio_ctx=o.n_audio_ctx)
        r = sr.sample_candidates(logits_fn, params, vid, best_of, temperature, seed=seed, temp_idx=temp_idx)
        print(f"{shape} best_of {best_of} t {temperature} clip {clip}: min margin {r.min_margin():.3e} over {len(r.margins)} draws, "
              f"winner {r.winner}, score gap {r.score_gap:.4f}, lengths {[len(c['tokens']) for c in r.cands]}, "
              f"distinct {len({tuple(c['tokens']) for c in r.cands})}, {time.time() - t0:.1f}s", flush=True)
    o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tiny+conf")
    ap.add_argument("--best-of", type=int, default=5)
    ap.add_argument("--temperature", type=float, default=0.6)
    ap.add_argument("--temp-idx", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-tokens", type=int, default=12)
    ap.add_argument("--clips", type=int, nargs=2, default=[0, 16], metavar=("FIRST", "END"))
    ap.add_argument("--model-dir", default=os.environ.get("NW_MODEL_DIR", "/tmp/nw_models"))
    args = ap.parse_args()
    scan(args.shape, args.best_of, args.temperature, args.temp_idx, args.seed, args.max_tokens, range(*args.clips), args.model_dir)


if __name__ == "__main__":
    main()
