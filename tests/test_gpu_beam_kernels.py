"""Beam search's two kernels through their hooks.

Top-k after the rules (kernels/logits.hip, whisper_mi355x_debug_logits_topk), both forms (one workgroup per row, and
the split form the engine takes for up to 16 rows), 4 rows of the tiny model's vocabulary at once, k in {1, 5, 8}:
ids exact against tests/beam_ref.py's rules, candidate 0 bit-equal to the greedy record of the same row, p and plog
within a bar against float64.

The bar is 4 x the worst difference measured on an MI355X over these rows (both forms, k = 8):
    |plog - ref| <= 1.70e-6 measured -> PLOG_BAR 6.8e-6;  |p / ref - 1| <= 1.67e-6 measured -> P_REL_BAR 6.7e-6
(f32 log-sum-exp of 51865 terms against float64; __expf's few ulp). The smallest gap between the k-th and the
(k + 1)-th plog of the random rows (and their timestamp-rule gap) must be at least 10 bars, so the bar discriminates.

Self-cache gather (kernels/beam.hip, whisper_mi355x_debug_kv_gather): exact against numpy's parallel assignment.
"""
import ctypes as C

import numpy as np
import pytest

import beam_ref as br
from conftest import model_path
from make_model import synthetic_vocab

pytestmark = pytest.mark.gpu

PLOG_BAR = 6.8e-6
P_REL_BAR = 6.7e-6


@pytest.fixture(scope="module")
def ctx(wrs):
    c = wrs.WhisperContext(model_path("tiny"), dtype=wrs.F16)
    yield c
    c.close()


class Dev:
    def __init__(self, wrs, ctx):
        self.L, self.ctx, self.ptrs = wrs.lib(), ctx.ptr, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.L.whisper_mi355x_dev_alloc(self.ctx, a.nbytes)
        assert p
        self.ptrs.append(p)
        assert self.L.whisper_mi355x_memcpy(self.ctx, p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def down(self, p, like):
        out = np.empty_like(like)
        assert self.L.whisper_mi355x_memcpy(self.ctx, out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.L.whisper_mi355x_dev_free(self.ctx, p)
        self.ptrs = []


# ---- top-k ------------------------------------------------------------------------------------------------------
_ROWS = {}


def topk_rows(V):
    """The 4 rows, their rule inputs for the hook, and beam_ref's log-probabilities (computed once)."""
    if V in _ROWS:
        return _ROWS[V]
    vid = br.vocab_ids(V, synthetic_vocab().index(b" "))
    beg = vid["beg"]
    rng = np.random.default_rng(20240611)
    raw = np.empty((4, V), np.float32)
    raw[0] = rng.normal(0.0, 6.0, V)
    raw[1] = rng.normal(0.0, 6.0, V)
    raw[1, [300, 7000]] = np.float32(31.5)           # two exactly equal maxima: the lower id comes first
    raw[2] = rng.normal(0.0, 6.0, V)
    raw[3] = -np.inf
    raw[3, [11, 4242, 40000]] = [0.5, 2.0, -1.0]     # 3 finite logits: 3 candidates
    text = [dict(id=100), dict(id=101)]
    states = [br.Beam(tokens=list(text)), br.Beam(tokens=list(text)),
              br.Beam(tokens=[dict(id=100), dict(id=beg + 10)], has_ts=True, seek_delta=20),  # an unpaired timestamp
              br.Beam(tokens=list(text))]
    P = br.Params()
    rules = np.zeros((4, 10), np.int32)
    for r, b in enumerate(states):
        ids = b.ids()
        rules[r] = [0, ids[-1] >= beg, ids[-2] >= beg, b.has_ts, b.seek_delta, 1, 0, 0, 50, 0]
    lps = [br.rules(raw[r], states[r], P, vid) for r in range(4)]
    _ROWS[V] = (vid, raw, rules, lps)
    return _ROWS[V]


@pytest.mark.parametrize("split", [0, 1], ids=["one-wg", "split"])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_topk(wrs, ctx, k, split):
    L = wrs.lib()
    V = L.whisper_n_vocab(ctx.ptr)
    vid, raw, rules, lps = topk_rows(V)
    d = Dev(wrs, ctx)
    try:
        cand = (wrs.Cand * (4 * k))()
        greedy = (wrs.Cand * 4)()
        rc = L.whisper_mi355x_debug_logits_topk(ctx.ptr, d.up(raw), 4, rules.ctypes.data_as(C.POINTER(C.c_int)), None, k, split,
                                                cand, greedy)
        assert rc == 0
    finally:
        d.free()
    worst_plog = worst_p = 0.0
    min_gap = np.inf
    for r in range(4):
        lp, ts_gap = lps[r]
        want = br.candidates(lp, k, vid)
        got = [cand[r * k + j] for j in range(k)]
        assert [g.id for g in got] == [c["id"] for c in want] + [-1] * (k - len(want)), f"row {r}"
        assert bytes(got[0]) == bytes(greedy[r]), f"row {r}: candidate 0 is not the greedy record"
        for g, c in zip(got, want):
            worst_plog = max(worst_plog, abs(g.plog - c["plog"]))
            worst_p = max(worst_p, abs(g.p / c["p"] - 1.0))
            assert g.tid == c["tid"], f"row {r}"
            assert g.pt == pytest.approx(c["pt"], rel=1e-4, abs=1e-9) and g.ptsum == pytest.approx(c["ptsum"], rel=1e-4, abs=1e-9)
        if r in (0, 2):  # the random rows: what decides which tokens are the k candidates, and the timestamp rule
            top = np.sort(lp[np.isfinite(lp)])[::-1][:k + 1]
            min_gap = min(min_gap, float(top[k - 1] - top[k]), ts_gap)
    print(f"k {k} split {split}: worst |dplog| {worst_plog:.3e}, worst |dp/p| {worst_p:.3e}, smallest deciding gap {min_gap:.3e}")
    assert PLOG_BAR * 10 <= min_gap
    assert worst_plog <= PLOG_BAR and worst_p <= P_REL_BAR
    if k >= 3:
        row1 = [cand[k + j].id for j in range(2)]
        assert row1 == [300, 7000]
        assert [cand[3 * k + j].id for j in range(3)] == [4242, 11, 40000]


# ---- gather -----------------------------------------------------------------------------------------------------
SLOTS, LAYERS, HEADS, NCTX = 6, 2, 2, 448
RANGES = [(0, 1), (37, 38), (17, 224), (0, 448)]


def _lists():
    out = {}
    for r0, r1 in RANGES:
        tag = f"{r0}-{r1}"
        out[f"identity-{tag}"] = ([(s, s, r0, r1) for s in range(SLOTS)], None)
        out[f"fanout-{tag}"] = ([(s, 0, r0, r1) for s in range(1, SLOTS)], 0)
        out[f"swap-{tag}"] = ([(0, 1, r0, r1), (1, 0, r0, r1)], 2)
        out[f"cycle+fanout-{tag}"] = ([(0, 1, r0, r1), (1, 2, r0, r1), (2, 0, r0, r1), (3, 0, r0, r1), (4, 0, r0, r1)], 3)
    # every copy its own range, a chain (2 <- 1 <- 0) beside a swap (4 <-> 5)
    out["mixed"] = ([(1, 0, 0, 1), (2, 1, 37, 38), (4, 5, 17, 224), (5, 4, 0, 448)], 3)
    return out


LISTS = _lists()
_CACHE = {}


def _cache():
    if "c" not in _CACHE:
        rng = np.random.default_rng(7)
        _CACHE["c"] = rng.integers(0, 65536, (SLOTS, LAYERS, 2, HEADS, NCTX, 64), dtype=np.uint16)
    return _CACHE["c"]


@pytest.mark.parametrize("name", list(LISTS))
def test_kv_gather(wrs, ctx, name):
    L = wrs.lib()
    copies, staged = LISTS[name]
    old = _cache()
    want = old.copy()
    for dst, src, r0, r1 in copies:  # parallel assignment: every copy reads the cache as it was
        want[dst, :, :, :, r0:r1, :] = old[src, :, :, :, r0:r1, :]
    if name.startswith("identity"):
        assert (want == old).all()
    d = Dev(wrs, ctx)
    try:
        p = d.up(old)
        cp = np.asarray(copies, np.int32)
        n_staged = C.c_int(-1)
        rc = L.whisper_mi355x_debug_kv_gather(ctx.ptr, p, SLOTS, LAYERS, HEADS, NCTX, cp.ctypes.data_as(C.POINTER(C.c_int)),
                                              len(copies), C.byref(n_staged))
        assert rc == 0
        got = d.down(p, old)
    finally:
        d.free()
    assert (got == want).all(), f"{name}: {int((got != want).sum())} elements differ"
    if staged is not None:
        assert n_staged.value == staged


def test_kv_gather_refuses_bad_lists(wrs, ctx):
    L = wrs.lib()
    d = Dev(wrs, ctx)
    try:
        old = _cache()
        p = d.up(old)
        for bad in ([(6, 0, 0, 1)], [(0, -1, 0, 1)], [(0, 1, 0, 449)], [(0, 1, 5, 5)], [(2, 0, 0, 4), (2, 1, 0, 4)]):
            cp = np.asarray(bad, np.int32)
            rc = L.whisper_mi355x_debug_kv_gather(ctx.ptr, p, SLOTS, LAYERS, HEADS, NCTX, cp.ctypes.data_as(C.POINTER(C.c_int)),
                                                  len(bad), None)
            assert rc != 0, bad
        assert (d.down(p, old) == old).all()
    finally:
        d.free()
