"""The numpy restatement of the sampled-draw contract (tests/sample_ref.py), checked on the CPU: the
Philox known answers, the draw's frequencies, and the candidate loop against beam_ref at K = 1."""
import math
import zlib

import numpy as np
import pytest

import beam_ref as br
import sample_ref as sr
from make_model import synthetic_vocab

V = 51865
VID = br.vocab_ids(V, synthetic_vocab().index(b" "))

# Random123's known answers for philox4x32-10: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(x) for x in sr.philox(key, ctr)) == want


def test_philox_vectorized_equals_scalar():
    i = np.arange(50)
    many = sr.word(0x1234567890abcdef, 300, 1, 4, i)
    for k in (0, 7, 49):
        assert int(many[k]) == int(sr.word(0x1234567890abcdef, 300, 1, 4, k))
    assert len(set(int(x) for x in many)) == 50
    # the seed's halves are the key (lo, hi); the counter is (0, seek, 16 * temp_idx + cand, i)
    assert int(sr.word(0x299f31d0a4093822, 0x85a308d3, 0, 0, 5)) == int(sr.philox((0xa4093822, 0x299f31d0), (0, 0x85a308d3, 0, 5))[0])
    assert sr.counter(300, 2, 3, 9) == (0, 300, 35, 9)


def test_draw_edges():
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25, 0.0], np.float32)
    assert sr.draw(p, 0)[0] == 1                      # the first positive token, never id 0 (p = 0)
    assert sr.draw(p, 2 ** 32 - 1)[0] == 4            # the last positive token, never id 5
    assert sr.draw(p, 2 ** 30 - 1)[0] == 1 and sr.draw(p, 2 ** 30)[0] == 3   # u just below / above 0.25
    i, m = sr.draw(p, 2 ** 31)                        # u = 0.5 + 2^-33 inside [0.25, 0.75)
    assert i == 3 and m == pytest.approx(0.25, abs=1e-9)
    assert sr.draw(np.zeros(6, np.float32), 12345) == (-1, math.inf)


def test_draw_frequencies():
    """20 000 counters over a 6-token row: every token's count within 5 sigma of n p; p = 0 is never drawn."""
    p = np.array([0.05, 0.30, 0.0, 0.15, 0.40, 0.10], np.float32)
    n = 20000
    words = sr.word(0, 0, 1, 0, np.arange(n))
    ids = np.array([sr.draw(p, int(x))[0] for x in words])
    q = p.astype(np.float64) / p.astype(np.float64).sum()
    for tok in range(6):
        cnt = int((ids == tok).sum())
        sigma = math.sqrt(n * q[tok] * (1 - q[tok]))
        assert abs(cnt - n * q[tok]) <= 5 * sigma, (tok, cnt, n * q[tok], sigma)
    assert (ids == 2).sum() == 0


def random_logits(seed):
    """logits_fn: a reproducible random row per prefix (a few tokens well above the rest, timestamps included)."""
    def fn(prefix):
        h = zlib.crc32(np.asarray((seed,) + tuple(prefix), np.int64).tobytes())
        g = np.random.default_rng(h)
        row = g.normal(0.0, 1.0, V).astype(np.float32)
        hot = g.integers(0, VID["eot"], 6)
        row[hot] += g.uniform(6.0, 9.0, 6).astype(np.float32)
        row[VID["beg"] + g.integers(0, 200, 3)] += np.float32(7.0)
        return row
    return fn


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("temperature", [0.6, 1.0])
def test_argmax_pick_is_beam_k1(seed, temperature):
    """Every draw replaced by the row's argmax: each candidate is beam_ref's K = 1 beam over the divided rows."""
    fn = random_logits(seed)
    t = np.float32(temperature)
    P = br.Params(K=1, max_tokens=8, single_segment=True, seek_end=2000)
    want = br.beam_search(lambda prefix: fn(prefix) / t, P, VID)
    got = sr.sample_candidates(fn, P, VID, 3, temperature, pick=lambda p32, cand, i: int(np.argmax(p32)))
    assert got.margins == []
    assert len(got.cands) == 3 and got.winner == (0 if want.winner >= 0 else -1)
    for c in got.cands:
        assert c["tokens"] == want.beams[0]["tokens"] and len(c["tokens"]) > 1
        assert (c["completed"], c["failed"]) == (want.beams[0]["completed"], want.beams[0]["failed"])
        assert c["sum_logprobs_all"] == want.beams[0]["sum_logprobs_all"]
    assert got.tokens == want.tokens and got.result_len == want.result_len
    assert got.avg_logprobs == want.avg_logprobs
    assert got.score_gap == math.inf   # identical candidates: the tie goes to the lowest index


def test_candidates_differ_and_replay():
    """Sampled candidates: distinct counters give distinct draws, the same seed replays, another seed does not."""
    fn = random_logits(3)
    P = br.Params(K=1, max_tokens=8, single_segment=True, seek_end=2000, seek=100)
    a = sr.sample_candidates(fn, P, VID, 5, 1.0, seed=0)
    b = sr.sample_candidates(fn, P, VID, 5, 1.0, seed=0)
    c = sr.sample_candidates(fn, P, VID, 5, 1.0, seed=1)
    assert [x["tokens"] for x in a.cands] == [x["tokens"] for x in b.cands] and a.winner == b.winner
    assert [x["tokens"] for x in a.cands] != [x["tokens"] for x in c.cands]
    assert len({tuple(x["tokens"]) for x in a.cands}) > 1
    assert len(a.margins) == sum(len(x["tokens"]) for x in a.cands) and a.min_margin() >= 0
    assert sum(x["winner"] for x in a.cands) == (1 if a.winner >= 0 else 0)
