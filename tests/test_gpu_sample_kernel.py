"""kernels/sample.hip through whisper_mi355x_debug_sample against tests/sample_ref.py.

Ids are exact, p / plog are the bits of the input row's entries, tid / pt follow process_step's sampled branch, ptsum and
the no-speech probability pass through. The kernel may associate its two double sums (the total and the prefix) differently
from numpy's sequential cumsum: each is off by at most V * 2^-53 = 5.8e-12 relative, so a draw whose reference margin is
below 1e-10 could differ legitimately. The seeds below leave no such draw (test_reference_margins, on the CPU), and a
GPU test fails rather than exclude one.

The kernel's layout (sample.hip): chunks of 64 ids, summed by wavefront (chunk % 16); in the scan lane l owns
ceil(chunks / 64) = 13 consecutive chunks, i.e. ids [832 l, 832 l + 832). The single-token rows sit on those boundaries.
"""
import ctypes as C

import numpy as np
import pytest

import sample_ref as sr
from conftest import model_path

VS = (51864, 51865, 51866)
NS = (1, 5, 17, 32)
MARGIN = 1e-10
REC0 = dict(id=7, tid=3, p=0.25, plog=-1.5, pt=0.5, ptsum=0.75, no_speech_prob=0.125, pad=0.0)


def make_rows(V, n, beg, seed):
    """n rows [n][2][V] float32: softmax rows, and every third row with only timestamp tokens (a run of `beg` zeros)."""
    g = np.random.default_rng(seed)
    x = g.normal(0.0, 2.0, (n, V))  # (every token's share of the mass stays above 2^-32: words 0 and 2^32 - 1 land inside)
    for r in range(n):
        if r % 3 == 1:
            x[r, :beg] = -np.inf
    x -= x.max(axis=1, keepdims=True)
    lp = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    out = np.empty((n, 2, V), np.float32)
    out[:, 0] = np.exp(lp).astype(np.float32)
    out[:, 1] = lp.astype(np.float32)
    return out


def single_rows(V, ids):
    """one positive token per row (p = 0.75: the row need not sum to 1)"""
    out = np.zeros((len(ids), 2, V), np.float32)
    out[:, 1] = -np.inf
    for r, i in enumerate(ids):
        out[r, 0, i] = 0.75
        out[r, 1, i] = np.log(np.float32(0.75))
    return out


def single_ids(V):
    return [0, V - 1, 63, 64, 831, 832, 833, 1023, 1024, 64 * ((V - 1) // 64), 832 * 62, 832 * 62 - 1]


def mid_words(row):
    """words whose target falls mid-interval of the first / the last positive token (0 / 2^32 - 1 if the token is too thin)"""
    p = row[0].astype(np.float64)
    S = p.sum()
    pos = np.nonzero(p > 0)[0]
    first = int(min(2 ** 32 - 1, p[pos[0]] / 2 / S * 2 ** 32))
    last = int(min(2 ** 32 - 1, (1.0 - p[pos[-1]] / 2 / S) * 2 ** 32))
    return first, last


def reference(rows, words):
    """(ids, margins) of sample_ref.draw per row"""
    res = [sr.draw(rows[r, 0], int(words[r])) for r in range(len(rows))]
    return [i for i, _ in res], [m for _, m in res]


def counters_for(n, base):
    c = np.zeros((n, 3), np.int32)
    c[:, 0] = 100 * base + np.arange(n) * 7     # seek
    c[:, 1] = 16 * (1 + np.arange(n) % 4) + np.arange(n) % 8
    c[:, 2] = (np.arange(n) * 13 + base) % 220  # token index
    return c


def philox_words(seed, ctr):
    return sr.philox((seed & 0xFFFFFFFF, seed >> 32), (0, ctr[:, 0], ctr[:, 1], ctr[:, 2]))[0]


SEED = 0x5eed0123456789ab
BEG_REF = 50364  # the multilingual vocabulary's first timestamp id (the zero runs of make_rows; any id would do)


def row_seed(V, n):
    """(chosen so that no draw below is decided by less than MARGIN: test_reference_margins)"""
    return 4000 * n + V


def explicit_cases(V, n):
    """[(rows, words)] of the explicit-word launches of one (V, n)"""
    rows = make_rows(V, n, BEG_REF, row_seed(V, n))
    mids = [mid_words(rows[r]) for r in range(n)]
    return [(rows, np.zeros(n, np.uint32)), (rows, np.full(n, 2 ** 32 - 1, np.uint32)),
            (rows, np.array([m[0] for m in mids], np.uint32)), (rows, np.array([m[1] for m in mids], np.uint32))]


def test_reference_margins():
    """CPU: no draw of the GPU tests below is decided by less than MARGIN."""
    worst = np.inf
    for V in VS:
        for n in NS:
            for rows, words in explicit_cases(V, n):
                worst = min(worst, min(reference(rows, words)[1]))
            ctr = counters_for(n, n)
            worst = min(worst, min(reference(make_rows(V, n, BEG_REF, row_seed(V, n)), philox_words(SEED, ctr))[1]))
    rows = make_rows(51865, 32, BEG_REF, 77)
    for k in range(0, 128, 16):  # (a sample of the 4096-draw test's launches; that test asserts all of them)
        worst = min(worst, min(reference(rows, philox_words(SEED, counters_for(32, k)))[1]))
    assert worst >= MARGIN, worst


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(wrs):
    c = wrs.WhisperContext(model_path("tiny+conf"), dtype=wrs.F16)
    yield c
    c.close()


def run(wrs, ctx, rows, seed, ctr, words=None, rec=REC0):
    L = wrs.lib()
    n, _, V = rows.shape
    rows = np.ascontiguousarray(rows, np.float32)
    ctr = np.ascontiguousarray(ctr, np.int32)
    rin = (wrs.Cand * n)(*[wrs.Cand(**rec) for _ in range(n)])
    rout = (wrs.Cand * n)()
    wp = None
    if words is not None:
        words = np.ascontiguousarray(words, np.uint32)
        wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = L.whisper_mi355x_debug_sample(ctx.ptr, rows.ctypes.data_as(C.POINTER(C.c_float)), rin, n, V, seed,
                                       ctr.ctypes.data_as(C.POINTER(C.c_int)), wp, rout)
    assert rc == 0, rc
    return list(rout)


def bits(x):
    return np.float32(x).view(np.uint32)


def check(out, rows, ids, beg, rec=REC0):
    for r, (o, want) in enumerate(zip(out, ids)):
        if want < 0:  # nothing to draw: the record as it was
            assert (o.id, o.tid, bits(o.p), bits(o.plog), bits(o.pt)) == \
                (rec["id"], rec["tid"], bits(rec["p"]), bits(rec["plog"]), bits(rec["pt"])), r
        else:
            assert o.id == want, (r, o.id, want)
            assert bits(o.p) == bits(rows[r, 0, want]) and bits(o.plog) == bits(rows[r, 1, want]), r
            assert rows[r, 0, want] > 0
            if want >= beg:
                assert o.tid == want and bits(o.pt) == bits(o.p), r
            else:
                assert o.tid == rec["tid"] and bits(o.pt) == bits(rec["pt"]), r
        assert bits(o.ptsum) == bits(rec["ptsum"]) and bits(o.no_speech_prob) == bits(rec["no_speech_prob"]), r


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("n", NS)
def test_explicit_words_and_philox(wrs, ctx, V, n):
    beg = wrs.lib().whisper_token_beg(ctx.ptr)
    ctr = counters_for(n, n)
    for rows, words in explicit_cases(V, n):
        ids, margins = reference(rows, words)
        assert min(margins) >= MARGIN
        check(run(wrs, ctx, rows, SEED, ctr, words), rows, ids, beg)
    rows = make_rows(V, n, BEG_REF, row_seed(V, n))
    words = philox_words(SEED, ctr)
    ids, margins = reference(rows, words)
    assert min(margins) >= MARGIN
    got = run(wrs, ctx, rows, SEED, ctr)                      # the kernel's own Philox word
    check(got, rows, ids, beg)
    assert [o.id for o in got] == [o.id for o in run(wrs, ctx, rows, SEED, ctr, words)]
    # first / last positive token at the extreme words
    first = [int(np.nonzero(rows[r, 0] > 0)[0][0]) for r in range(n)]
    last = [int(np.nonzero(rows[r, 0] > 0)[0][-1]) for r in range(n)]
    assert [o.id for o in run(wrs, ctx, rows, SEED, ctr, np.zeros(n, np.uint32))] == first
    assert [o.id for o in run(wrs, ctx, rows, SEED, ctr, np.full(n, 2 ** 32 - 1, np.uint32))] == last


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
def test_single_token_and_empty_rows(wrs, ctx, V):
    beg = wrs.lib().whisper_token_beg(ctx.ptr)
    ids = single_ids(V) + [beg - 1, beg, beg + 1]
    rows = np.concatenate([single_rows(V, ids), np.zeros((1, 2, V), np.float32)])
    rows[-1, 1] = -np.inf
    n = len(rows)
    want = ids + [-1]
    ctr = counters_for(n, 3)
    for words in (None, np.zeros(n, np.uint32), np.full(n, 2 ** 32 - 1, np.uint32), np.full(n, 2 ** 31, np.uint32)):
        check(run(wrs, ctx, rows, SEED, ctr, words), rows, want, beg)
    # a record whose tid / pt are the logits kernel's timestamp guess is kept for text tokens only
    rec = dict(REC0, id=0, tid=beg + 9, p=0.0, plog=-np.inf)
    check(run(wrs, ctx, rows, 1, ctr, None, rec), rows, want, beg, rec)


@pytest.mark.gpu
def test_4096_philox_draws(wrs, ctx):
    """4096 draws by counter over 32 rows (128 launches): the kernel's Philox word and CDF inversion against numpy."""
    V, n = 51865, 32
    beg = wrs.lib().whisper_token_beg(ctx.ptr)
    rows = make_rows(V, n, BEG_REF, 77)
    cums = [np.cumsum(rows[r, 0].astype(np.float64)) for r in range(n)]
    seen = set()
    for k in range(128):
        ctr = counters_for(n, k)
        words = philox_words(SEED + k % 3, ctr)
        ids = []
        for r in range(n):  # sample_ref.draw over the precomputed prefix sums
            C_, S = cums[r], float(cums[r][-1])
            target = (float(int(words[r])) + 0.5) * 2.0 ** -32 * S
            i = int(np.searchsorted(C_, target, side="right"))
            assert i < V
            lo = float(C_[i - 1]) if i > 0 else 0.0
            assert min(target - lo, float(C_[i]) - target) / S >= MARGIN, (k, r)
            ids.append(i)
        if k % 32 == 0:
            assert ids == reference(rows, words)[0]
        check(run(wrs, ctx, rows, SEED + k % 3, ctr), rows, ids, beg)
        seen.update(ids)
    assert len(seen) > 100


@pytest.mark.gpu
def test_bad_arguments(wrs, ctx):
    L = wrs.lib()
    assert L.whisper_mi355x_debug_sample(None, None, None, 1, 51865, 0, None, None, None) == -1
    rows = make_rows(51865, 1, BEG_REF, 5)
    rin, rout = (wrs.Cand * 33)(), (wrs.Cand * 33)()
    ctr = np.zeros((33, 3), np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    assert L.whisper_mi355x_debug_sample(ctx.ptr, rows.ctypes.data_as(fp), rin, 33, 51865, 0, ctr.ctypes.data_as(ip), None, rout) == -1
    assert L.whisper_mi355x_debug_sample(ctx.ptr, rows.ctypes.data_as(fp), rin, 1, 65537, 0, ctr.ctypes.data_as(ip), None, rout) == -1
