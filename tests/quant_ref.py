"""Plain numpy reference of the GGML block-quantized weight path (imports nothing from the engine).

A quantized matrix [rows][K] (K % 32 == 0) is rows * K / 32 blocks of 32 weights, row-major, each block in ggml's
file format (ggml-common.h block_q4_0 / q4_1 / q5_0 / q5_1 / q8_0):
    q4_0: d f16 | qs[16]              q4_1: d f16 | m f16 | qs[16]
    q5_0: d f16 | qh u32 | qs[16]     q5_1: d f16 | m f16 | qh u32 | qs[16]
    q8_0: d f16 | qs[32] (int8)
q4 / q5: byte j of qs holds weight j in its low nibble and weight j + 16 in its high nibble; bit j of qh is the
fifth bit of weight j. The value is (q - 8) * d (q4_0), (q - 16) * d (q5_0), q * d (q8_0) or q * d + m (q4_1,
q5_1), every operation in f32 (ggml's dequantize_row_*): q * d is exact there, q * d + m is rounded once.

The engine keeps a matrix as those blocks regrouped by field (struct QMat, kernels.h), which `regroup` restates:
    qs  uint8  [rows][K/2]  (q8_0: [rows][K])   the blocks' quant bytes, in block order
    qh  uint32 [rows][K/32]                     q5 types only, else None
    dm  uint16 [rows][K/32] (d) or [rows][K/32][2] (d, m) for the *_1 types
and a kernel's output is `round_f16` / `round_bf16` of `dequant_fields`: one rounding, to nearest even, f16
subnormals kept.
"""
import numpy as np

QTYPES = ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0")
GGML_TYPE = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8}
BLOCK_BYTES = {"q4_0": 18, "q4_1": 20, "q5_0": 22, "q5_1": 24, "q8_0": 34}
HAS_M = ("q4_1", "q5_1")
HAS_H = ("q5_0", "q5_1")


def _random_f16_bits(rng, n, dmax):
    """n f16 bit patterns, finite, |value| <= dmax, both signs: the magnitude bits are uniform over
    [0, bits(dmax)], so every exponent is as likely as any other, subnormals (magnitude bits < 0x0400) and zero
    included. The first entries are pinned to +0, -0, the smallest and the largest subnormal, the smallest normal
    and +-dmax, so these are present whatever the seed."""
    top = int(np.float16(dmax).view(np.uint16))
    assert float(np.float16(dmax)) == dmax and 0x0400 < top < 0x7C00, dmax
    mag = rng.integers(0, top + 1, size=n, dtype=np.uint16)
    sign = rng.integers(0, 2, size=n, dtype=np.uint16) << 15
    bits = (mag | sign).astype(np.uint16)
    pinned = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x0400, top, 0x8000 | top], np.uint16)
    k = min(n, len(pinned))
    bits[:k] = pinned[:k]
    return bits


def random_blocks(rng, qtype, rows, K, dmax):
    """Raw file-format bytes of a random [rows][K] matrix of `qtype`: every quant byte and every qh bit uniformly
    random (patterns a quantizer never emits too: q8_0's -128, high bits set on every weight), d (and m) random
    finite f16 bit patterns of both signs with |.| <= dmax, zeros and subnormals included."""
    assert K % 32 == 0 and rows >= 1
    nb = rows * (K // 32)
    blk = np.zeros((nb, BLOCK_BYTES[qtype]), np.uint8)
    blk[:, 0:2] = _random_f16_bits(rng, nb, dmax).view(np.uint8).reshape(nb, 2)
    off = 2
    if qtype in HAS_M:
        # the pinned values of m sit on other blocks than those of d
        blk[:, 2:4] = _random_f16_bits(rng, nb, dmax)[::-1].copy().view(np.uint8).reshape(nb, 2)
        off = 4
    blk[:, off:] = rng.integers(0, 256, size=(nb, BLOCK_BYTES[qtype] - off), dtype=np.uint8)  # qh (q5) and qs
    return blk.tobytes()


def case_blocks(qtype, rows, K, dmax, salt=0):
    """random_blocks of a fixed seed per (type, shape, salt): the CPU test checks the quality of the very inputs
    the GPU tests use."""
    rng = np.random.default_rng(100003 * GGML_TYPE[qtype] + 1009 * rows + K + 7919 * salt)
    return random_blocks(rng, qtype, rows, K, dmax)


def regroup(raw, qtype, rows, K):
    """File blocks -> the QMat fields (qs, qh, dm), row-major and by field: the same bits, the same bytes."""
    nbk = K // 32
    blk = np.frombuffer(raw, np.uint8).reshape(rows, nbk, BLOCK_BYTES[qtype])
    off = 2
    if qtype in HAS_M:
        dm = np.ascontiguousarray(blk[:, :, 0:4]).view(np.uint16).reshape(rows, nbk, 2)
        off = 4
    else:
        dm = np.ascontiguousarray(blk[:, :, 0:2]).view(np.uint16).reshape(rows, nbk)
    qh = None
    if qtype in HAS_H:
        qh = np.ascontiguousarray(blk[:, :, off:off + 4]).view(np.uint32).reshape(rows, nbk)
        off += 4
    per = 32 if qtype == "q8_0" else 16
    qs = np.ascontiguousarray(blk[:, :, off:off + per]).reshape(rows, nbk * per)
    return qs, qh, dm


def dequant_fields(qtype, qs, qh, dm, rows, K):
    """The QMat fields -> f32 [rows][K], ggml's dequantize_row_* arithmetic in f32."""
    nbk = K // 32
    f32 = np.float32
    dmv = dm.reshape(rows, nbk, -1)
    d = dmv[:, :, 0].copy().view(np.float16).astype(f32)[:, :, None]
    if qtype == "q8_0":
        q = qs.reshape(rows, nbk, 32).view(np.int8).astype(np.int32)
        return (q.astype(f32) * d).reshape(rows, K)
    b = qs.reshape(rows, nbk, 16).astype(np.int32)
    q = np.empty((rows, nbk, 32), np.int32)
    q[:, :, :16] = b & 15   # weight j: low nibble of byte j
    q[:, :, 16:] = b >> 4   # weight j + 16: high nibble of byte j
    if qtype in HAS_H:
        bit = (qh.reshape(rows, nbk, 1).astype(np.int64) >> np.arange(32, dtype=np.int64)) & 1  # bit j = weight j
        q |= bit.astype(np.int32) << 4
    if qtype in HAS_M:
        m = dmv[:, :, 1].copy().view(np.float16).astype(f32)[:, :, None]
        y = q.astype(f32) * d  # exact: <= 5 bits times 11 bits
        y = y + m              # one f32 rounding
    else:
        y = (q - (16 if qtype == "q5_0" else 8)).astype(f32) * d
    assert y.dtype == f32
    return y.reshape(rows, K)


def round_f16(x):
    """f32 -> f16 bit patterns (uint16), round to nearest even, subnormals kept (IEEE convert, as numpy's)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def round_bf16(x):
    """f32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def f16_value(bits):
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(np.float32)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def count_f16_ties(x):
    """f32 values exactly half way between two neighbouring f16 values (normal or subnormal f16 range)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.abs(x.astype(np.float64))
    normal = (a >= 2.0 ** -14) & (a < 65520.0)
    tie_n = normal & ((x.view(np.uint32) & 0x1FFF) == 0x1000)  # the 13 bits f16 drops are 1000...0
    tie_s = (a < 2.0 ** -14) & ((a * 2.0 ** 24) % 1.0 == 0.5)  # subnormal range: spacing 2^-24
    return int((tie_n | tie_s).sum())


def count_bf16_ties(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return int(((u & 0xFFFF) == 0x8000).sum())


def count_f16_subnormal(x):
    """values that round to a nonzero f16 subnormal"""
    b = round_f16(x) & 0x7FFF
    return int(((b > 0) & (b < 0x0400)).sum())
