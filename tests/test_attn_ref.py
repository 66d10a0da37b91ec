"""The yardstick of the decoder attention tests (tests/attn_ref.py) checks itself, without a GPU, on
exactly the cases tests/test_gpu_attn_dec.py runs:

reachable  the kernels' rounding restated in float32 (P and the output rounded to T) stays within HALF the
           GPU tests' bound of the float64 reference, so a correct kernel has room for its summation order;
not blind  every deliberately wrong reading of the inputs (attn_ref.MUTATIONS) leaves the bound in at least
           one element of every case it can apply to.
"""
import numpy as np
import pytest

import attn_ref as R

CASES = {dt: list(R.all_cases(dt)) for dt in ("f16", "bf16")}
N_CASES = len(CASES["f16"])


@pytest.fixture(scope="module", params=[(dt, j) for dt in ("f16", "bf16") for j in range(N_CASES)],
                ids=lambda p: f"{p[0]}-{p[1]}")
def case(request):
    dt, j = request.param
    c = CASES[dt][j]()
    ref, mag, applied = c.expected()
    assert applied.all()
    return c, ref, R.bound(ref, mag, dt)


def test_case_lists_cover_the_edges():
    pos = {}
    for n, H, splits, p in R.SELF_CASES:
        c = R.self_case("f16", n, H, splits, p)
        assert len(set(c.slot.tolist())) == n and (c.slot != np.arange(n)).any()
        pos.setdefault((n, H), set()).update((c.n_kv - 1).tolist())
        if n == 33:
            assert set(R.EDGE_POS) <= set((c.n_kv - 1).tolist())
    assert sorted(pos) == [(2, 20), (3, 6), (33, 6), (33, 8)]
    assert all({0, 64, 447} <= s for s in pos.values())
    assert {s for _, _, s, _ in R.SELF_CASES} == {1, 5, 16}
    want = {1, 7, 8, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1030, 1500, 1536}
    for n in (3, 9):
        rows = [c for c in R.CROSS_CASES if c[0] == n]
        assert all(1500 in c[3] and max(c[3]) <= c[1] for c in rows)
        assert set(sum((c[3] for c in rows), [])) == want
        assert {c[2] for c in rows} == {1, 16} and {c[1] for c in rows} == {1500, 1536}
    assert any(c[0] == 9 and set(c[3]) == {1500} for c in R.CROSS_CASES)
    slot, pos = R.prefill_tokens()
    tiles = R.prefill_tiles(slot, pos)
    assert tiles[:, 1].tolist() == [64, 64, 42, 11, 1, 15, 16, 17, 64]
    assert {1, 15, 16, 17, 64} <= set(tiles[:, 1].tolist())
    assert pos[tiles[3, 0]] == 60 and pos[tiles[3, 0] + 10] + 1 == 71 and pos[tiles[4, 0]] == 447


def test_reference_is_the_twenty_lines(case):
    """Case.expected() batches the tokens of a slot; reference() on the rows of single (token, head) pairs is the
    plain statement of the same thing"""
    c, ref, _ = case
    rng = np.random.default_rng(0)
    for i in sorted({0, c.n - 1, *rng.integers(0, c.n, 3).tolist()}):
        h = int(rng.integers(0, c.H))
        o, m = R.reference(*c.rows(i, h))
        assert np.abs(o - ref[i, h * 64:(h + 1) * 64]).max() <= 1e-12 * (1 + m.max())


def test_bound_is_reachable(case):
    c, ref, bound = case
    emu, _, _ = c.expected(emu=True)
    ratio = np.abs(emu - ref) / bound
    assert ratio.max() <= 0.5, f"{c.name}: the emulated kernel is at {ratio.max():.2f} of the bound"
    i, h = c.n - 1, c.H - 1
    one = R.emulate(*c.rows(i, h), c.dtype)
    assert (np.abs(one - ref[i, h * 64:(h + 1) * 64]) <= 0.5 * bound[i, h * 64:(h + 1) * 64]).all()


def test_bound_is_not_blind(case):
    c, ref, bound = case
    skipped = []
    for mut in R.MUTATIONS:
        if mut in ("no_fresh", "fresh_twice") and c.kind != "self":
            continue  # (there is no fresh key: not a mutation of this launcher)
        wrong, _, applied = c.expected(mut)
        if not applied.any():
            skipped.append(mut)
            continue
        ratio = (np.abs(wrong - ref) / bound)[applied]
        assert ratio.max() > 1.0, f"{c.name}: '{mut}' stays within the bound (worst {ratio.max():.2f})"
    assert len(skipped) <= 1, f"{c.name}: {skipped} cannot apply"


def test_from_slabs_is_exact_in_any_order():
    rng = np.random.default_rng(5)
    slabs, bias = R.draw_slabs(rng, 16, 4, 192, np.full(192, 3.0))
    assert (slabs * 256 == np.round(slabs * 256)).all() and np.abs(slabs).max() <= 4 and np.abs(bias).max() <= 4
    exact = (slabs.astype(np.float64).sum(0) + bias).astype(np.float32)
    assert (exact == slabs.astype(np.float64).sum(0) + bias).all()
    for dt in ("f16", "bf16"):
        want = R.to_t(exact * R.K_SCALE, dt)[0]
        assert (R.from_slabs(slabs, bias, R.K_SCALE, dt)[0] == want).all()
        assert (R.from_slabs(slabs[rng.permutation(16)], bias, R.K_SCALE, dt)[0] == want).all()
