"""Kernel-level GPU parity of the decoder attention launchers (nobs-whisper_amd/csrc/kernels/attn.hip), one
launch each through whisper_mi355x_debug_attn_self_step / _cross_step / _prefill, against the float64
reference of tests/attn_ref.py (softmax(q . K^T) . V on the exact T-typed inputs, P never rounded).

Bound per output element: TOL * (sum_t p_t |v_t| + |o|) + 1e-5, TOL = 4e-3 (f16) / 1.6e-2 (bf16): the
constants of tests/test_gpu_xattn.py for "P and the output rounded to the MFMA type, every sum f32".
tests/test_attn_ref.py shows on the CPU, for these very cases, that the kernels' rounding stays within half
of it and that a dropped, doubled or misplaced key does not.

Beyond the bound: q, k, v reduced from the split-K slabs are known bit for bit (slab values are multiples of
2^-8, attn_ref.from_slabs), so the rows appended to the self cache are compared exactly, every other byte
of the caches must be unchanged, and the rows around `out` must be untouched.
"""
import ctypes as C
import os

import numpy as np
import pytest

import attn_ref as R
from conftest import model_path

pytestmark = pytest.mark.gpu

SENTINEL = 0x7E5A  # (a NaN in neither format: 2.2e4 in f16, 4.5e37 in bf16)
I, F, P = C.c_int, C.c_float, C.c_void_p
SCALE = float(R.K_SCALE)


@pytest.fixture(scope="module")
def ctxs(wrs):
    c16 = wrs.WhisperContext(model_path("micro"), dtype=wrs.F16)
    cbf = wrs.WhisperContext(model_path("micro"), dtype=wrs.BF16)
    L = wrs.lib()
    L.whisper_mi355x_debug_attn_self_step.argtypes = [P, P, I, P, F, P, P, P, I, I, I, I, I, P]
    L.whisper_mi355x_debug_attn_cross_step.argtypes = [P, P, I, P, F, P, P, P, I, I, I, I, I, P]
    L.whisper_mi355x_debug_attn_prefill.argtypes = [P, P, I, P, P, P, P, I, I, I, I, I, P]
    yield {"f16": c16, "bf16": cbf}
    c16.close()
    cbf.close()


class Dev:
    """device copies of numpy arrays, freed together"""

    def __init__(self, wrs, ctx):
        self.L, self.ctx, self.ptrs = wrs.lib(), ctx.ptr, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= 64 << 20
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


def _check_out(c, got_bits, ref, bound, what):
    """rows [0, n) of the (n + 1)-row output against the reference, the row after them untouched"""
    n = len(ref)
    assert (got_bits[n:] == SENTINEL).all(), f"{c.name} {what}: the row after out[n] was written"
    got = R.from_t(got_bits[:n], c.dtype).astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    print(f"{c.name} {c.dtype} {what}: max err {err.max():.3e}, worst ratio {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"{c.name} {what}: max err {err.max():.3e}, worst ratio {(err / bound).max():.2f}"
    return got


def _blank(n, d):
    return np.full((n + 1, d), SENTINEL, np.uint16)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("n,H,splits,pos", R.SELF_CASES, ids=[f"n{a[0]}-H{a[1]}-s{a[2]}" for a in R.SELF_CASES])
def test_self_step(wrs, ctxs, dtype, n, H, splits, pos):
    c = R.self_case(dtype, n, H, splits, pos)
    ref, mag, _ = c.expected()
    pos = (c.n_kv - 1).astype(np.int32)
    dv = Dev(wrs, ctxs[dtype])
    try:
        p_cache, p_out = dv.up(c.cache_bits), dv.up(_blank(n, c.d))
        rc = dv.L.whisper_mi355x_debug_attn_self_step(ctxs[dtype].ptr, dv.up(c.slabs), splits, dv.up(c.bias), SCALE,
                                                      p_cache, dv.up(c.slot), dv.up(pos), n, R.LAYERS, R.LAYER, H, 448,
                                                      p_out)
        assert rc == 0
        out_bits, cache_after = dv.down(p_out, _blank(n, c.d)), dv.down(p_cache, c.cache_bits)
    finally:
        dv.free()
    _check_out(c, out_bits, ref, R.bound(ref, mag, dtype), "self step")
    # K[pos], V[pos] of every head are the prologue's bits; every other byte of the cache is as it was
    want = c.cache_bits.copy()
    for i in range(n):
        assert (cache_after[c.slot[i], R.LAYER, 0, :, pos[i]] == c.k_new_bits[i]).all(), f"K[{pos[i]}] of token {i}"
        assert (cache_after[c.slot[i], R.LAYER, 1, :, pos[i]] == c.v_new_bits[i]).all(), f"V[{pos[i]}] of token {i}"
        want[c.slot[i], R.LAYER, 0, :, pos[i]] = c.k_new_bits[i]
        want[c.slot[i], R.LAYER, 1, :, pos[i]] = c.v_new_bits[i]
    assert np.array_equal(cache_after, want), "a cache byte outside K[pos], V[pos] changed"
    first = np.flatnonzero(pos == 0)  # a single key: P = 1, out is the fresh v bit for bit
    assert (out_bits[first] == c.v_new_bits[first].reshape(len(first), c.d)).all()


def _cross_launch(dv, ctx, c, rows):
    n = len(rows)
    p_out = dv.up(_blank(n, c.d))
    rc = dv.L.whisper_mi355x_debug_attn_cross_step(ctx.ptr, dv.up(c.slabs[:, rows]), c.splits, dv.up(c.bias), SCALE,
                                                   c.p_cache, dv.up(c.slot[rows]), dv.up(c.n_kv[rows]), n, R.LAYERS,
                                                   R.LAYER, c.H, c.n_ctx, p_out)
    assert rc == 0
    return dv.down(p_out, _blank(n, c.d))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("n,n_ctx,splits,n_kv", R.CROSS_CASES,
                         ids=[f"n{a[0]}-ctx{a[1]}-s{a[2]}-{'_'.join(map(str, a[3][:3]))}" for a in R.CROSS_CASES])
def test_cross_step(wrs, ctxs, dtype, n, n_ctx, splits, n_kv):
    """n = 3: the 1024-thread kernel, n = 9: the 256-thread one (attn_cross_wide_max() = 8 by default), and the
    first three rows of every n = 9 launch again on their own, so that both widths see the same inputs"""
    if "WHISPER_MI355X_XWIDE_MAX" in os.environ:
        pytest.skip("WHISPER_MI355X_XWIDE_MAX is set: the launcher's choice of width is not the default's")
    c = R.cross_case(dtype, n, n_ctx, splits, n_kv)
    ref, mag, _ = c.expected()
    bound = R.bound(ref, mag, dtype)
    dv = Dev(wrs, ctxs[dtype])
    try:
        c.p_cache = dv.up(c.cache_bits)
        out_bits = _cross_launch(dv, ctxs[dtype], c, np.arange(n))
        wide_bits = _cross_launch(dv, ctxs[dtype], c, np.arange(3)) if n == 9 else None
        cache_after = dv.down(c.p_cache, c.cache_bits)
    finally:
        dv.free()
    got = _check_out(c, out_bits, ref, bound, "cross step")
    if wide_bits is not None:
        wide = _check_out(c, wide_bits, ref[:3], bound[:3], "cross step, rows 0-2 at 1024 threads")
        assert (np.abs(wide - got[:3]) <= 2 * bound[:3]).all(), "the two widths disagree"
    assert np.array_equal(cache_after, c.cache_bits), "the cross cache changed"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind,H", R.PREFILL_CASES, ids=[f"{k}-H{h}" for k, h in R.PREFILL_CASES])
def test_prefill(wrs, ctxs, dtype, kind, H):
    c = R.prefill_case(dtype, kind, H)
    ref, mag, _ = c.expected()
    n = c.n
    some = c.tiles[::2]  # a second launch with every other tile: the rows of the others stay untouched
    covered = np.zeros(n, bool)
    for i0, cnt in some:
        covered[i0:i0 + cnt] = True
    dv = Dev(wrs, ctxs[dtype])
    try:
        p_cache, p_q, p_slot, p_nkv = dv.up(c.cache_bits), dv.up(c.q_bits), dv.up(c.slot), dv.up(c.n_kv)
        outs = []
        for tiles in (c.tiles, some):
            p_out = dv.up(_blank(n, c.d))
            rc = dv.L.whisper_mi355x_debug_attn_prefill(ctxs[dtype].ptr, p_q, c.d, p_cache, p_slot, p_nkv, dv.up(tiles),
                                                        len(tiles), R.LAYERS, R.LAYER, H, c.n_ctx, p_out)
            assert rc == 0
            outs.append(dv.down(p_out, _blank(n, c.d)))
        cache_after = dv.down(p_cache, c.cache_bits)
    finally:
        dv.free()
    _check_out(c, outs[0], ref, R.bound(ref, mag, dtype), "prefill")
    assert (outs[1][:n][covered] == outs[0][:n][covered]).all()
    assert (outs[1][:n][~covered] == SENTINEL).all() and (outs[1][n:] == SENTINEL).all(), "a row of no tile was written"
    assert np.array_equal(cache_after, c.cache_bits), "the cache changed"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_error_returns(wrs, ctxs, dtype):
    """host-side refusals: a null context, a self cache of more than 448 rows, a cross cache of more than 1536;
    nothing is launched (every pointer but out is null here) and out stays as it was"""
    L, ctx = wrs.lib(), ctxs[dtype]
    assert L.whisper_mi355x_debug_attn_self_step(None, None, 1, None, 1.0, None, None, None, 1, 2, 1, 6, 448, None) != 0
    assert L.whisper_mi355x_debug_attn_cross_step(None, None, 1, None, 1.0, None, None, None, 1, 2, 1, 6, 1500, None) != 0
    assert L.whisper_mi355x_debug_attn_prefill(None, None, 384, None, None, None, None, 1, 2, 1, 6, 448, None) != 0
    dv = Dev(wrs, ctx)
    try:
        blank = _blank(1, 384)
        p_out = dv.up(blank)
        for splits, n in ((0, 1), (17, 1), (1, 0)):
            assert L.whisper_mi355x_debug_attn_self_step(ctx.ptr, None, splits, None, 1.0, None, None, None, n, 2, 1, 6,
                                                         448, p_out) == -1
            assert L.whisper_mi355x_debug_attn_cross_step(ctx.ptr, None, splits, None, 1.0, None, None, None, n, 2, 1, 6,
                                                          1500, p_out) == -1
        assert L.whisper_mi355x_debug_attn_self_step(ctx.ptr, None, 1, None, 1.0, None, None, None, 1, 2, 1, 6, 449,
                                                     p_out) != 0
        assert L.whisper_mi355x_debug_attn_cross_step(ctx.ptr, None, 1, None, 1.0, None, None, None, 1, 2, 1, 6, 1537,
                                                      p_out) != 0
        assert np.array_equal(dv.down(p_out, blank), blank)
    finally:
        dv.free()
