"""The block-quantization reference of the GPU kernel tests (tests/quant_ref.py), without a GPU:
 - regroup + dequant_fields (the QMat field layout, the kernels' input) == tools/make_model.py's
   dequantize_rows (the file layout, block by block; test_quant.py holds the oracle's loader to the same
   function), exactly, on random blocks and on a quantizer's blocks;
 - the random inputs of tests/test_gpu_quant_kernels.py reach what a kernel can get wrong: values on exact
   f16 / bf16 rounding ties, values in the f16 subnormal range, every quant byte value, and nothing overflows.
"""
import numpy as np
import pytest

import quant_ref as qr
from make_model import dequantize_rows, quantize_rows

SHAPES = [(1, 32), (37, 352), (5, 1280)]


@pytest.mark.parametrize("rows,K", SHAPES)
@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_fields_equal_file_dequant_random(qtype, rows, K):
    raw = qr.case_blocks(qtype, rows, K, 64.0)
    assert len(raw) == rows * K // 32 * qr.BLOCK_BYTES[qtype]
    got = qr.dequant_fields(qtype, *qr.regroup(raw, qtype, rows, K), rows, K)
    want = dequantize_rows(raw, qtype, rows * K).reshape(rows, K)
    assert got.dtype == np.float32 and want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_fields_equal_file_dequant_quantized(qtype):
    rows, K = 37, 352
    rng = np.random.default_rng(qr.GGML_TYPE[qtype])
    x = (rng.standard_normal((rows, K)) * np.exp(rng.uniform(-6, 2, (rows, 1)))).astype(np.float32)
    x[3] = 0.0  # all-zero blocks: d = 0
    raw = quantize_rows(x, qtype)
    got = qr.dequant_fields(qtype, *qr.regroup(raw, qtype, rows, K), rows, K)
    want = dequantize_rows(raw, qtype, rows * K).reshape(rows, K)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # and it is a quantization of x: within one step of every weight
    step = np.abs(x).reshape(rows, K // 32, 32).max(2, keepdims=True) / {"q4_0": 8, "q4_1": 7.5, "q5_0": 16, "q5_1": 15.5,
                                                                            "q8_0": 127}[qtype]
    assert (np.abs(got - x).reshape(rows, K // 32, 32) <= 1.01 * step + 1e-30).all()


def test_regroup_layout():
    """the field layout spelled out on one hand-made q5_1 matrix of 2 rows x 64"""
    rows, K = 2, 64
    blk = np.zeros((4, 24), np.uint8)
    for i in range(4):
        blk[i, 0:2] = np.array([np.float16(i + 1)]).view(np.uint8)       # d
        blk[i, 2:4] = np.array([np.float16(-(i + 1))]).view(np.uint8)    # m
        blk[i, 4:8] = np.array([1 << (i + 16)], np.uint32).view(np.uint8)  # fifth bit on weight 16 + i only
        blk[i, 8:24] = np.arange(16) | (i << 4)                           # weights 0..15 = j, weights 16..31 = i
    qs, qh, dm = qr.regroup(blk.tobytes(), "q5_1", rows, K)
    assert qs.shape == (2, 32) and qh.shape == (2, 2) and dm.shape == (2, 2, 2)
    assert qh.tolist() == [[1 << 16, 1 << 17], [1 << 18, 1 << 19]]
    assert dm.view(np.float16).tolist() == [[[1, -1], [2, -2]], [[3, -3], [4, -4]]]
    y = qr.dequant_fields("q5_1", qs, qh, dm, rows, K).reshape(4, 32)
    for i in range(4):
        q = np.concatenate([np.arange(16), np.full(16, i)])
        q[16 + i] += 16
        np.testing.assert_array_equal(y[i], q * (i + 1.0) - (i + 1.0))


def test_rounding_helpers():
    f = np.float32
    # f16: 1 + 2^-11 is a tie -> even (1.0); 1 + 3 * 2^-11 -> 1 + 2^-9; subnormals kept; 2^-25 tie -> 0
    x = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, -2.0 ** -15], f)
    assert qr.round_f16(x).tolist() == [0x3C00, 0x3C02, 0x0001, 0x0002, 0x0000, 0x8200]
    assert qr.count_f16_ties(x) == 4 and qr.count_f16_subnormal(x) == 3
    # bf16: 1 + 2^-8 tie -> even (1.0); 1 + 3 * 2^-8 -> 1 + 2^-6
    y = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -3.0], f)
    assert qr.round_bf16(y).tolist() == [0x3F80, 0x3F82, 0x3F81, 0xC040]
    assert qr.count_bf16_ties(y) == 2
    np.testing.assert_array_equal(qr.bf16_value(qr.round_bf16(y)), np.array([1, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -3], f))


@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_wrong_kernels_would_differ(qtype):
    """What the bit-exact GPU comparisons catch, counted on the reference at their (37, 352) input: the share of
    output bit patterns a wrong dequantizer changes."""
    rows, K = 37, 352
    qs, qh, dm = qr.regroup(qr.case_blocks(qtype, rows, K, 64.0), qtype, rows, K)
    y = qr.dequant_fields(qtype, qs, qh, dm, rows, K)
    want16, wantbf = qr.round_f16(y), qr.round_bf16(y)

    def changed(qs2, qh2, dm2):
        y2 = qr.dequant_fields(qtype, qs2, qh2, dm2, rows, K)
        return (qr.round_f16(y2) != want16).mean(), (qr.round_bf16(y2) != wantbf).mean()

    if qtype != "q8_0":  # nibble halves swapped: every weight whose two nibbles differ (15 / 16), d != 0
        assert min(changed((qs >> 4) | (qs << 4), qh, dm)) > 0.8
    else:  # bytes read as unsigned: every negative weight
        y2 = qs.reshape(rows, K // 32, 32).astype(np.float32) * dm.view(np.float16).astype(np.float32)[:, :, None]
        assert (qr.round_f16(y2.reshape(rows, K)) != want16).mean() > 0.4
    if qh is not None:  # high-bit index off by one: every weight whose neighbour's bit differs (1 / 2)
        assert min(changed(qs, (qh >> 1) | (qh << 31), dm)) > 0.4
        assert min(changed(qs, np.zeros_like(qh), dm)) > 0.4  # high bits dropped
    if dm.ndim == 3:  # m read from the other half of dm
        assert min(changed(qs, qh, dm[:, :, ::-1])) > 0.8
    # a neighbouring block's scale
    assert min(changed(qs, qh, np.roll(dm, 1, axis=1))) > 0.8
    # rounded twice (f32 -> f16 -> bf16) instead of once
    twice = qr.round_bf16(qr.f16_value(want16))
    assert (twice != wantbf).sum() >= 20, (twice != wantbf).sum()
    # round half away from zero / truncation instead of nearest-even: every tie, or about every second value
    u = y.view(np.uint32)
    assert ((((u + 0x8000) >> 16).astype(np.uint16)) != wantbf).sum() >= 50
    # f16 subnormal results flushed to zero
    assert qr.count_f16_subnormal(y) >= 10


@pytest.mark.parametrize("qtype", qr.QTYPES)
def test_gpu_inputs_reach_the_edges(qtype):
    rows, K = 37, 352
    raw = qr.case_blocks(qtype, rows, K, 64.0)
    qs, qh, dm = qr.regroup(raw, qtype, rows, K)
    y = qr.dequant_fields(qtype, qs, qh, dm, rows, K)
    assert np.isfinite(qr.f16_value(qr.round_f16(y))).all()
    ties16, ties_bf, sub = qr.count_f16_ties(y), qr.count_bf16_ties(y), qr.count_f16_subnormal(y)
    print(f"{qtype}: {ties16} f16 ties, {ties_bf} bf16 ties, {sub} f16 subnormal results of {y.size}")
    assert ties16 >= 100 and ties_bf >= 100 and sub >= 10, (ties16, ties_bf, sub)
    # the d (and m) fields hold +-0, subnormals and both signs; every quant byte value occurs (q8_0: -128 too)
    d = dm.reshape(rows * (K // 32), -1)
    for col in range(d.shape[1]):
        mag = d[:, col] & 0x7FFF
        assert (mag == 0).any() and ((mag > 0) & (mag < 0x0400)).any() and (mag == 0x5400).any()
        assert (d[:, col] >> 15).any() and not (d[:, col] >> 15).all()
        assert (mag <= 0x5400).all()
    assert len(np.unique(qs)) == 256
    if qh is not None:
        assert 0.45 < np.unpackbits(qh.view(np.uint8)).mean() < 0.55
