"""The numpy yardstick of the token-timestamp alignment (tests/dtw_ref.py) checks itself, without a GPU:
the float32 DTW against brute-force enumeration of every monotone path, the tie rule on integer costs, and
the reflected width-7 median against an explicit loop."""
import itertools

import numpy as np
import pytest

from dtw_ref import cost_matrix, dtw_f32, first_frames, median_filter


def all_paths(N, F):
    """every path (0, 0) -> (N-1, F-1) with steps (1, 1), (1, 0), (0, 1)"""
    def go(i, j):
        if (i, j) == (N - 1, F - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < N and j + dj < F:
                for rest in go(i + di, j + dj):
                    yield [(i, j)] + rest
    return go(0, 0)


def check_path(path, N, F):
    fwd = path[::-1]
    assert fwd[0] == (0, 0) and fwd[-1] == (N - 1, F - 1)
    for (a, b), (c, d) in zip(fwd, fwd[1:]):
        assert (c - a, d - b) in ((1, 1), (1, 0), (0, 1))


@pytest.mark.parametrize("N,F", [(1, 1), (2, 1), (1, 4), (2, 5), (3, 3), (4, 5), (4, 2), (4, 1)])
def test_dtw_is_a_cheapest_path(N, F):
    rng = np.random.default_rng(N * 10 + F)
    for trial in range(6):
        cost = rng.standard_normal((N, F)).astype(np.float32)
        fr, path, _ = dtw_f32(cost)
        check_path(path, N, F)
        c64 = cost.astype(np.float64)
        best = min(sum(c64[p] for p in pth) for pth in all_paths(N, F))
        got = sum(c64[p] for p in path)
        assert abs(got - best) <= 1e-5, (trial, got, best)
        np.testing.assert_array_equal(fr, first_frames(path, N))
        assert (np.diff(fr) >= 0).all() and fr[0] == 0


def test_dtw_integer_ties():
    """integer costs: every sum is exact, so the path is decided by the tie rule alone (trace 0 only if c0 is
    strictly below both, else 1 only if c1 is strictly below both, else 2)"""
    fr, path, trace = dtw_f32(np.zeros((3, 3), np.float32))
    # row 1: only the diagonal at (1, 1), then left moves; column 1 below: only up moves; elsewhere all equal -> 2
    assert path == [(2, 2), (2, 1), (2, 0), (1, 0), (0, 0)]
    assert fr.tolist() == [0, 0, 0]
    assert trace[1, 1] == 0 and trace[1, 2] == 2 and trace[2, 1] == 1 and trace[2, 2] == 2
    rng = np.random.default_rng(3)
    for N, F in ((4, 5), (3, 4), (4, 4)):
        cost = rng.integers(-1, 2, (N, F)).astype(np.float32)
        fr, path, _ = dtw_f32(cost)
        check_path(path, N, F)
        np.testing.assert_array_equal(fr, first_frames(path, N))
    # at (2, 2): c0 = 0 == c2 = 0 < c1 = 5 -> not strictly the smallest -> trace 2 (left)
    _, path, trace = dtw_f32(np.array([[0, 5], [0, 0]], np.float32))
    assert trace[2, 2] == 2 and path == [(1, 1), (1, 0), (0, 0)]
    # at (2, 2): c0 = 0 == c1 = 0 < c2 = 5: a tie between diagonal and up is neither, the walk goes left
    # (through the dearer cell: with ties the traced path need not be a cheapest one; C itself is the minimum)
    _, path, trace = dtw_f32(np.array([[0, 0], [5, 0]], np.float32))
    assert trace[2, 2] == 2 and trace[2, 1] == 1 and path == [(1, 1), (1, 0), (0, 0)]


def test_dtw_more_rows_than_frames():
    rng = np.random.default_rng(11)
    cost = rng.standard_normal((9, 3)).astype(np.float32)
    fr, path, _ = dtw_f32(cost)
    check_path(path, 9, 3)
    assert (np.diff(fr) >= 0).all() and fr.max() <= 2 and len(set(fr.tolist())) <= 3  # vertical runs: rows share frames


@pytest.mark.parametrize("F", [1, 2, 3, 4, 7, 9])
def test_median_filter_matches_loop(F):
    rng = np.random.default_rng(F)
    x = rng.standard_normal((3, F))
    want = np.empty_like(x)
    for r in range(3):
        for t in range(F):
            win = []
            for k in range(-3, 4):
                i = t + k
                if i < 0:
                    i = -i
                if i >= F:
                    i = 2 * (F - 1) - i
                i = min(max(i, 0), F - 1)
                win.append(x[r, i])
            want[r, t] = sorted(win)[3]
    np.testing.assert_array_equal(median_filter(x), want)


def test_cost_matrix_shape_and_stats():
    rng = np.random.default_rng(5)
    P = rng.random((3, 10, 12))
    c = cost_matrix(P, n_sot=2)
    assert c.shape == (7, 12)
    # without the median the head mean of z-scores has zero mean over ALL rows of every frame
    full = cost_matrix(np.concatenate([P, P[:, :1]], 1), n_sot=0, median=False)  # (drops the appended last row)
    Z = (P - P.mean(1, keepdims=True)) / np.sqrt(P.var(1, keepdims=True) + 1e-9)
    np.testing.assert_allclose(cost_matrix(P, 0, median=False), -Z.mean(0)[:9], rtol=0, atol=1e-12)
    assert full.shape == (10, 12)
    assert len(list(itertools.islice(all_paths(3, 3), 100))) == 13  # Delannoy number D(2, 2)
