"""bench.py's command line without a GPU: a plain run keeps every leg beside the headline off, --full
switches them on, a leg's own option wins over both; and the arrays that --dump-outputs writes."""
import importlib.util
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def legs(bench, args):
    return {k: getattr(args, k) for k in bench.FULL_LEGS}


def test_plain_run_has_no_extra_legs(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert legs(bench, a) == dict.fromkeys(bench.FULL_LEGS, 0)
    assert a.fallback_line == 0


def test_full_run_has_every_leg(bench):
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    assert legs(bench, a) == bench.FULL_LEGS
    assert set(bench.FULL_LEGS) == {"variants", "inflight_line", "f16_line", "frontend", "app_pattern", "cpu_baseline"}
    assert all(v == 1 for v in bench.FULL_LEGS.values())


def test_a_legs_own_option_wins(bench):
    a = bench.parse_args(["--full", "--variants", "0", "--cpu-baseline", "0"])
    assert (a.variants, a.cpu_baseline, a.frontend, a.app_pattern) == (0, 0, 1, 1)
    a = bench.parse_args(["--cpu-baseline", "1"])
    assert (a.variants, a.cpu_baseline, a.frontend) == (0, 1, 0)


def test_steps_must_be_positive(bench):
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_collect_outputs_rows(bench):
    """Two chunks (global indices 5 and 9) with 2 and 1 segments of 2, 0 and 3 tokens."""
    ntok = {(0, 0): 2, (0, 1): 0, (1, 0): 3}
    tok = lambda j, s, t: types.SimpleNamespace(id=100 * j + 10 * s + t, tid=7, p=0.5, plog=-0.25, pt=0.125, ptsum=0.75)  # noqa: E731
    L = types.SimpleNamespace(
        whisper_mi355x_batch_n_segments=lambda p, j: (2, 1)[j],
        whisper_mi355x_batch_segment_n_tokens=lambda p, j, s: ntok[j, s],
        whisper_mi355x_batch_segment_t0=lambda p, j, s: 1000 * j + s,
        whisper_mi355x_batch_segment_t1=lambda p, j, s: 1000 * j + s + 50,
        whisper_mi355x_batch_token_data=lambda p, j, s, t: tok(j, s, t))
    out = bench.collect_outputs(types.SimpleNamespace(L=L, ptr=1), [5, 9])
    assert sorted(out) == ["segments", "tokens"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["segments"].tolist() == [[5, 0, 0, 50, 2], [5, 1, 1, 51, 0], [9, 0, 1000, 1050, 3]]
    assert out["tokens"].shape == (5, 9)
    assert out["tokens"][:, :4].tolist() == [[5, 0, 0, 0], [5, 0, 1, 1], [9, 0, 0, 100], [9, 0, 1, 101], [9, 0, 2, 102]]
    assert out["tokens"][0, 4:].tolist() == [7, 0.5, -0.25, 0.125, 0.75]
    empty = bench.collect_outputs(types.SimpleNamespace(L=L, ptr=1), [])
    assert empty["tokens"].shape == (0, 9) and empty["segments"].shape == (0, 5)
