"""Kernel-level GPU parity of the GGML block-quantized weight path (kernels/gemm.hip: qraw_load / qraw_deq in
dequant_kernel, dequant_multi_kernel and the block-reading instantiations of gemm_small_kernel), one launch each
through whisper_mi355x_debug_dequant / _dequant_multi / _gemm_small_q, against tests/quant_ref.py.

The contract is "w = d * (q - offset) or d * q + m in f32, rounded once to the compute type", so the dequantizers
are compared bit for bit, and the block-reading GEMM bit for bit with the plain GEMM on the reference's rounded
matrix (the same kernel and MFMA order, only the source of B differs). The inputs are random blocks
(quant_ref.case_blocks): every quant byte and high bit random, scales of both signs down to f16 subnormals and
zero; tests/test_quant_ref.py shows on the CPU that they put hundreds of values on exact f16 / bf16 rounding ties
and tens into the f16 subnormal range. A swapped nibble half, a high bit taken from a neighbouring weight, an m
read from the wrong half of dm or a value rounded twice changes at least one output bit here.
"""
import ctypes as C

import numpy as np
import pytest

import quant_ref as qr
from conftest import model_path
from test_gpu_attn_dec import Dev
from test_gpu_kernels import _gelu_ggml

pytestmark = pytest.mark.gpu

CANARY = 0xA5
EPI_STORE, EPI_GELU, EPI_RESID, EPI_F32 = 0, 1, 2, 4
P = C.c_void_p


@pytest.fixture(scope="module")
def ctxs(wrs):
    c = {"f16": wrs.WhisperContext(model_path("micro"), dtype=wrs.F16),
         "bf16": wrs.WhisperContext(model_path("micro"), dtype=wrs.BF16)}
    yield c
    for x in c.values():
        x.close()


def _round(dtype, x):
    return qr.round_f16(x) if dtype == "f16" else qr.round_bf16(x)


def _value(dtype, bits):
    return qr.f16_value(bits) if dtype == "f16" else qr.bf16_value(bits)


class QDev:
    """a quantized matrix on the device, by field, and its reference"""

    def __init__(self, dv, qtype, rows, K, dmax, salt=0):
        self.qtype, self.type, self.rows, self.K = qtype, qr.GGML_TYPE[qtype], rows, K
        qs, qh, dm = qr.regroup(qr.case_blocks(qtype, rows, K, dmax, salt), qtype, rows, K)
        self.f32 = qr.dequant_fields(qtype, qs, qh, dm, rows, K)
        self.qs, self.dm = dv.up(qs), dv.up(dm)
        self.qh = dv.up(qh) if qh is not None else None


def _out(dv, shape, dtype=np.uint16, init=None):
    """device output of `shape` followed by 64 canary bytes; returns (pointer, host image)"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    img = np.full(n + 64, CANARY, np.uint8)
    if init is not None:
        img[:n] = np.ascontiguousarray(init, dtype=dtype).view(np.uint8).reshape(-1)
    return dv.up(img), img


def _down(dv, p, img, shape, dtype=np.uint16):
    got = dv.down(p, img)
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert (got[n:] == CANARY).all(), "bytes after the output were written"
    return got[:n].view(dtype).reshape(shape)


def _same_bits(got, want, what):
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"got {got[bad][:4]} want {want[bad][:4]}"


# ---- dequant_kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K", [(1, 32), (37, 352), (5, 1280), (3, 5120)])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_dequant_bit_exact(wrs, ctxs, qtype, dtype, rows, K):
    """one thread per 8 weights; rows * K / 8 is no multiple of the 256-thread workgroup in three of the shapes
    (4, 1628, 800, 1920 threads), (1, 32) is a single block"""
    L, ctx = wrs.lib(), ctxs[dtype]
    dv = Dev(wrs, ctx)
    try:
        q = QDev(dv, qtype, rows, K, 64.0)
        po, img = _out(dv, (rows, K))
        assert L.whisper_mi355x_debug_dequant(ctx.ptr, q.type, q.qs, q.qh, q.dm, rows, K, po) == 0
        got = _down(dv, po, img, (rows, K))
        _same_bits(got, _round(dtype, q.f32), f"{qtype} {dtype} {rows}x{K}")
    finally:
        dv.free()


# ---- dequant_multi_kernel -------------------------------------------------------------------------------------
# a decoder layer's six projections at d = 384 (QKV, out, cross Q, cross out, FC1: K = d; FC2: K = 4 d) with an
# eighth of the rows, nudged so that no job starts on a multiple of 256 threads
MULTI_JOBS = [(143, 384), (47, 384), (49, 384), (45, 384), (191, 384), (47, 1536)]


def _multi(L, ctx, types, mats, outs, K=None):
    n = len(mats)
    ty = (C.c_int * n)(*types)
    qs = (P * n)(*[m.qs for m in mats])
    qh = (P * n)(*[m.qh if m.qh is not None else m.dm for m in mats])  # never read for the types without high bits
    dm = (P * n)(*[m.dm for m in mats])
    rows = (C.c_long * n)(*[m.rows for m in mats])
    Ks = (C.c_int * n)(*(K if K is not None else [m.K for m in mats]))
    po = (P * n)(*outs)
    return L.whisper_mi355x_debug_dequant_multi(ctx.ptr, ty, n, qs, qh, dm, rows, Ks, po)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_dequant_multi_bit_exact(wrs, ctxs, qtype, dtype):
    L, ctx = wrs.lib(), ctxs[dtype]
    starts = np.cumsum([r * k // 8 for r, k in MULTI_JOBS])
    assert (starts[:-1] % 256 != 0).all() and starts[-1] % 256 != 0, starts
    dv = Dev(wrs, ctx)
    try:
        for jobs in (MULTI_JOBS, MULTI_JOBS[:1], MULTI_JOBS[:2] + [(1, 384)] + MULTI_JOBS[3:]):
            mats = [QDev(dv, qtype, r, k, 64.0, salt=j) for j, (r, k) in enumerate(jobs)]
            outs = [_out(dv, (m.rows, m.K)) for m in mats]
            assert _multi(L, ctx, [mats[0].type] * len(mats), mats, [o[0] for o in outs]) == 0
            for j, (m, (po, img)) in enumerate(zip(mats, outs)):
                got = _down(dv, po, img, (m.rows, m.K))
                _same_bits(got, _round(dtype, m.f32), f"{qtype} {dtype} job {j} of {len(jobs)} ({m.rows}x{m.K})")
                p1, img1 = _out(dv, (m.rows, m.K))
                assert L.whisper_mi355x_debug_dequant(ctx.ptr, m.type, m.qs, m.qh, m.dm, m.rows, m.K, p1) == 0
                _same_bits(got, _down(dv, p1, img1, (m.rows, m.K)), f"{qtype} {dtype} job {j}: multi vs single launch")
            dv.free()
    finally:
        dv.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_dequant_multi_refusals(wrs, ctxs, qtype, dtype):
    """mixed types and K % 32 != 0 are refused on the host (nonzero, nothing written); the context then still
    runs a correct call"""
    L, ctx = wrs.lib(), ctxs[dtype]
    other = qr.GGML_TYPE[qr.QTYPES[(qr.QTYPES.index(qtype) + 1) % len(qr.QTYPES)]]
    dv = Dev(wrs, ctx)
    try:
        mats = [QDev(dv, qtype, r, k, 64.0, salt=j) for j, (r, k) in enumerate([(3, 64), (2, 96), (5, 32)])]
        outs = [_out(dv, (m.rows, m.K)) for m in mats]
        po = [o[0] for o in outs]
        ty = [m.type for m in mats]
        assert _multi(L, ctx, [ty[0], other, ty[2]], mats, po) != 0
        assert _multi(L, ctx, [ty[0], ty[1], other], mats, po) != 0
        assert _multi(L, ctx, ty, mats, po, K=[64, 96, 40]) != 0
        assert _multi(L, ctx, ty, mats, po, K=[48, 96, 32]) != 0
        assert _multi(L, ctx, [ty[0], 1, ty[2]], mats, po) != 0  # f16 is no block type
        assert L.whisper_mi355x_debug_dequant(ctx.ptr, mats[0].type, mats[0].qs, mats[0].qh, mats[0].dm, 3, 48, po[0]) != 0
        for m, (p, img) in zip(mats, outs):
            assert (dv.down(p, img) == CANARY).all(), "a refused call wrote its output"
        assert _multi(L, ctx, ty, mats, po) == 0
        for j, (m, (p, img)) in enumerate(zip(mats, outs)):
            _same_bits(_down(dv, p, img, (m.rows, m.K)), _round(dtype, m.f32), f"{qtype} {dtype} job {j} after refusals")
    finally:
        dv.free()


# ---- gemm_small_kernel reading blocks ---------------------------------------------------------------------------
_GELU = {}


def _gelu_t(dtype, pre):
    """the GELU epilogue on f32 pre-activations: ggml's f16 table (|x| >= 10 shortcuts), then the compute type"""
    pre = np.ascontiguousarray(pre, dtype=np.float32)
    tab = _gelu_ggml(pre).astype(np.float32)
    g = np.where(pre <= -10, np.float32(0), np.where(pre >= 10, pre, tab)).astype(np.float32)
    return _round(dtype, g)


def _ulp(dtype, ref):
    """one unit in the last place of the compute type at |ref| (the subnormal spacing below the normal range)"""
    mant, emin = (10, -14) if dtype == "f16" else (7, -126)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** emin)))
    return 2.0 ** (e - mant)


GEMM_CASES = [
    # M, N, K, epi, scale, lna
    (1, 48, 96, EPI_F32, 1.0, False),        # K / 32 = 3: waves 3-7 have no K-step
    (16, 40, 352, EPI_F32, 1.0, False),      # N % 16 != 0: the row clamp min(n0 + lane, N - 1); 11 K-steps
    (17, 64, 1312, EPI_RESID, 1.0, False),   # the two-row-tile form; wave 0 has 6 steps: a second chunk of 5
    (32, 32, 5120, EPI_RESID, 1.0, False),   # the largest K: four chunks
    (33, 48, 384, EPI_STORE, 0.125, False),  # rows beyond 32: the 32-row chunk loop, a 1-row tail chunk
    (70, 32, 1536, EPI_GELU, 1.0, False),
    (3, 64, 128, EPI_F32, 1.0, True), (16, 48, 384, EPI_STORE, 1.0, True), (7, 32, 1280, EPI_F32, 1.0, True),
]


@pytest.mark.parametrize("M,N,K,epi,scale,lna", GEMM_CASES)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_gemm_small_quant(wrs, ctxs, qtype, dtype, M, N, K, epi, scale, lna):
    """(a) bit-identical to whisper_mi355x_debug_gemm_small on B = round(dequant_fields) uploaded as a plain
    matrix: the same kernel, the same MFMA order, only the source of B differs. The plain hook passes no column
    scale, so the scaled STORE case is compared against (b) only.
    (b) against the float64 product of the same rounded operands, within test_gemm_small_matches_numpy's bounds
    (1e-4 |A||B|^T + 1e-5 + 1e-6 |ref|; 2e-3 |A||B|^T with the LayerNorm prologue, whose operand may round one
    ulp differently from numpy's), plus one output ulp of the compute type for the STORE and GELU epilogues. The
    GELU output is also ggml's f16 table applied to the same launch's own f32 result, bit for bit
    (test_gemm_gelu_epilogue's comparison)."""
    L, ctx = wrs.lib(), ctxs[dtype]
    L.whisper_mi355x_debug_gemm_small.argtypes = [P, C.c_int, P, C.c_int, C.c_int, P, C.c_int, P, P, P, P, C.c_int,
                                                  C.POINTER(C.c_float)]
    rng = np.random.default_rng(1000 * M + N + K + qr.GGML_TYPE[qtype])
    dv = Dev(wrs, ctx)
    try:
        q = QDev(dv, qtype, N, K, 1.0 / 16)
        Bbits = _round(dtype, q.f32)
        B64 = _value(dtype, Bbits).astype(np.float64)
        bias = rng.standard_normal(N).astype(np.float32)
        w = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        b = (0.1 * rng.standard_normal(K)).astype(np.float32)
        if lna:
            A = (3.0 * rng.standard_normal((M, K)) + 0.5).astype(np.float32)
            mu = A.astype(np.float64).mean(1, keepdims=True)
            var = ((A.astype(np.float64) - mu) ** 2).mean(1, keepdims=True)
            ln = ((A - mu) / np.sqrt(var + 1e-5) * w + b).astype(np.float32)
            A64 = _value(dtype, _round(dtype, ln)).astype(np.float64)
        else:
            A = _round(dtype, rng.standard_normal((M, K)).astype(np.float32))
            A64 = _value(dtype, A).astype(np.float64)
        x0 = rng.standard_normal((M, N)).astype(np.float32)
        f32_out = epi in (EPI_RESID, EPI_F32)
        odt = np.float32 if f32_out else np.uint16
        init = x0 if epi == EPI_RESID else None
        pA, pB, pbias, pw, pb = dv.up(A), dv.up(Bbits), dv.up(bias), dv.up(w), dv.up(b)
        lw, lb = (pw, pb) if lna else (None, None)

        def run_q(e, sc):
            po, img = _out(dv, (M, N), np.float32 if e in (EPI_RESID, EPI_F32) else np.uint16, x0 if e == EPI_RESID else None)
            assert L.whisper_mi355x_debug_gemm_small_q(ctx.ptr, e, pA, M, K, q.type, q.qs, q.qh, q.dm, N, pbias, sc, po,
                                                       lw, lb) == 0
            return _down(dv, po, img, (M, N), np.float32 if e in (EPI_RESID, EPI_F32) else np.uint16)

        got = run_q(epi, scale)
        # (a)
        if scale == 1.0:
            po, img = _out(dv, (M, N), odt, init)
            ms = C.c_float()
            assert L.whisper_mi355x_debug_gemm_small(ctx.ptr, epi, pA, M, K, pB, N, pbias, po, lw, lb, 0, C.byref(ms)) == 0
            plain = _down(dv, po, img, (M, N), odt)
            _same_bits(got.view(np.uint32 if f32_out else np.uint16), plain.view(np.uint32 if f32_out else np.uint16),
                       f"{qtype} {dtype} {(M, N, K, epi)} blocks vs plain B")
        # (b)
        pre = A64 @ B64.T + bias
        mag = np.abs(A64) @ np.abs(B64).T
        if epi == EPI_RESID:
            pre = pre + x0
        bound = (2e-3 if lna else 1e-4) * mag + 1e-5 + 1e-6 * np.abs(pre)
        if epi == EPI_STORE:
            ref = pre * np.float64(np.float32(scale))
            assert np.isfinite(qr.f16_value(qr.round_f16(ref))).all()  # dmax = 1/16 keeps f16 outputs finite
            bound = bound * abs(scale) + _ulp(dtype, ref)
            val = _value(dtype, got).astype(np.float64)
        elif epi == EPI_GELU:
            assert np.isfinite(qr.f16_value(qr.round_f16(pre))).all()
            ref = _value(dtype, _gelu_t(dtype, pre.astype(np.float32))).astype(np.float64)
            bound = bound + _ulp(dtype, ref)
            val = _value(dtype, got).astype(np.float64)
            own = run_q(EPI_F32, 1.0)
            _same_bits(got, _gelu_t(dtype, own), f"{qtype} {dtype} GELU of the launch's own f32 result")
        else:
            ref, val = pre, got.astype(np.float64)
        assert np.isfinite(val).all()
        err = np.abs(val - ref)
        print(f"{qtype} {dtype} {(M, N, K, epi, lna)}: max err {err.max():.3e}, worst ratio {(err / bound).max():.3f}, "
              f"max |ref| {np.abs(ref).max():.3g}")
        assert (err <= bound).all(), f"max err {err.max()}, worst ratio {(err / bound).max()}"
    finally:
        dv.free()
