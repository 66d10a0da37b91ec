"""numpy reference of the decoder attention launchers (nobs-whisper_amd/csrc/kernels/attn.hip:
launch_attn_self_step, launch_attn_cross_step, launch_attn_prefill) — TEST INFRASTRUCTURE ONLY.

One (token, head) of every launcher computes softmax(q . K[0:n_kv]^T) . V[0:n_kv] over rows of a cache
[slot][L][2][H][n_ctx][64]; there is no extra scale (q and the cached K carry d_head^-0.25 each). The
decode steps form q (and the self step its fresh k, v) from split-K slabs first.

reference()   float64, exact T-typed inputs, P never rounded: the yardstick of tests/test_gpu_attn_dec.py.
emulate()     the kernels' rounding restated in float32 (P and the output rounded to T) without their
              summation order: only tests/test_attn_ref.py uses it, to show the bound is reachable.
from_slabs()  the prologue (sum of the slabs, + bias, * scale for q and k, round to T), bit for bit.

The case lists below are shared by the GPU test and the CPU self-check, so that the bound is shown
reachable and not blind (MUTATIONS) for exactly the inputs the kernels are run on.
"""
from __future__ import annotations

import numpy as np

# "P and the output rounded to the MFMA type, every sum f32": the project's constants of
# tests/test_gpu_xattn.py (2^-11 / 2^-8 relative per rounding), restated here so that the CPU self-check
# imports no GPU test module.
TOL = {"f16": 4e-3, "bf16": 1.6e-2}
ABS = 1e-5
K_SCALE = np.float32(64 ** -0.25)
LAYERS, LAYER = 2, 1  # every case: two layers, the second one used, so that the cache offsets matter


# ---- number formats ---------------------------------------------------------------------------------
def to_t(x, dtype):
    """float32 -> (bit patterns uint16, their float32 values) of f16 (numpy's astype) or bf16 (round to
    nearest even on the bits, as _to_bf16_bits of tests/test_gpu_kernels.py)"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "bf16":
        u = x.view(np.uint32)
        b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        return b, (b.astype(np.uint32) << 16).view(np.float32)
    h = x.astype(np.float16)
    return h.view(np.uint16), h.astype(np.float32)


def from_t(bits, dtype):
    bits = np.ascontiguousarray(bits, np.uint16)
    if dtype == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


# ---- the three restatements --------------------------------------------------------------------------
def reference(q, K, V):
    """q [..., 64], K and V [..., n_kv, 64] (exact values of the T-typed inputs) -> (out [..., 64],
    magnitude sum_t p_t |v_t| [..., 64]), float64."""
    q, K, V = (np.asarray(a, np.float64) for a in (q, K, V))
    s = np.einsum("...e,...te->...t", q, K)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("...t,...te->...e", p, V), np.einsum("...t,...te->...e", p, np.abs(V))


def emulate(q, K, V, dtype):
    """the kernels' arithmetic in float32: scores f32, p = T(exp(s - max) / sum), out = T(sum p v)"""
    q, K, V = (np.asarray(a, np.float32) for a in (q, K, V))
    s = np.einsum("...e,...te->...t", q, K)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = to_t(e / e.sum(-1, keepdims=True, dtype=np.float32), dtype)[1]
    return to_t(np.einsum("...t,...te->...e", p, V), dtype)[1]


def from_slabs(slabs, bias, scale, dtype):
    """slabs [splits][n][cols] f32, bias [cols] f32 or None -> (bits, values) of T((sum_z slab_z + bias) *
    scale); scale may be an array over the columns (1 for the v columns). Exact for slab and bias values
    that are multiples of 2^-8 in [-4, 4]: every f32 sum of <= 16 of them plus a bias is exact in any
    order, which leaves one f32 multiply and one rounding."""
    v = np.zeros(slabs.shape[1:], np.float32)
    for z in range(slabs.shape[0]):
        v = v + slabs[z]
    if bias is not None:
        v = v + bias
    return to_t(v * np.asarray(scale, np.float32), dtype)


def bound(ref, mag, dtype):
    return TOL[dtype] * (mag + np.abs(ref)) + ABS


# ---- inputs --------------------------------------------------------------------------------------------
_POOL = None


def _normal(rng, shape):
    """N(0, 1) float32 of a shape, cut from one pool at a random offset (the caches are tens of MB: drawing
    them afresh for every case would dominate the tests' time)"""
    global _POOL
    if _POOL is None:
        _POOL = np.random.default_rng(1234).standard_normal(1 << 25, dtype=np.float32)
    n = int(np.prod(shape))
    assert n < _POOL.size
    o = int(rng.integers(0, _POOL.size - n))
    return _POOL[o:o + n].reshape(shape)


def _quant(x):
    return (np.clip(np.round(x * 256.0), -1024, 1024) / 256.0).astype(np.float32)


def draw_slabs(rng, splits, n, cols, sigma):
    """slabs [splits][n][cols] and a bias [cols], multiples of 2^-8 in [-4, 4], whose sum is about
    N(0, sigma) per column (sigma [cols])"""
    s = (np.asarray(sigma, np.float32) / np.sqrt(splits + 1.0)).astype(np.float32)
    return _quant(rng.standard_normal((splits, n, cols), dtype=np.float32) * s), \
        _quant(rng.standard_normal(cols, dtype=np.float32) * s)


class Case:
    """One launch. Token i, head h attends rows [0, n_kv[i]) of K, V = cache[slot[i]][LAYER][0 / 1][h]; in a
    self step the last of them (row pos[i] = n_kv[i] - 1) is the fresh k, v of the slabs and the cache row
    holds unrelated random values before the launch."""

    def __init__(self, kind, dtype, name, n_ctx, H, slot, n_kv, n_slots, splits=0, spike=None, seed=0):
        self.kind, self.dtype, self.name = kind, dtype, name
        self.n_ctx, self.H, self.d, self.splits, self.n_slots = n_ctx, H, 64 * H, splits, n_slots
        self.slot = np.asarray(slot, np.int32)
        self.n_kv = np.asarray(n_kv, np.int32)
        self.n = n = len(self.slot)
        assert self.n_kv.min() >= 1 and self.n_kv.max() <= n_ctx and self.slot.max() < n_slots
        rng = np.random.default_rng(seed)
        d = self.d
        # q: N(0, 1) * 3 before k_scale; fresh k: N(0, 1) after it; fresh v: N(0, 1)
        if kind == "self":
            sigma = np.concatenate([np.full(d, 3.0), np.full(d, 1.0 / K_SCALE), np.full(d, 1.0)])
            self.slabs, self.bias = draw_slabs(rng, splits, n, 3 * d, sigma)
            # the last head has no late key in the cache: its cached keys are a quarter of the others' and its
            # fresh key is the strong one (no bias, the slabs' sign turned so that q . k > 0), or no input would
            # notice a fresh key left out
            kc = slice(d + (H - 1) * 64, d + H * 64)
            self.bias[kc] = 0.0
            q_last = from_slabs(self.slabs[:, :, (H - 1) * 64:H * 64], self.bias[(H - 1) * 64:H * 64], K_SCALE, dtype)[1]
            turn = np.einsum("ie,ie->i", q_last.astype(np.float64), self.slabs[:, :, kc].sum(0, dtype=np.float64)) < 0
            self.slabs[:, turn, kc] *= -1.0
            scale = np.concatenate([np.full(2 * d, K_SCALE), np.ones(d, np.float32)]).astype(np.float32)
            bits, val = from_slabs(self.slabs, self.bias, scale, dtype)
            self.q = val[:, :d].reshape(n, H, 64)
            self.k_new, self.v_new = val[:, d:2 * d].reshape(n, H, 64), val[:, 2 * d:].reshape(n, H, 64)
            self.k_new_bits, self.v_new_bits = bits[:, d:2 * d].reshape(n, H, 64), bits[:, 2 * d:].reshape(n, H, 64)
        elif kind == "cross":
            self.slabs, self.bias = draw_slabs(rng, splits, n, d, np.full(d, 3.0))
            self.q = from_slabs(self.slabs, self.bias, K_SCALE, dtype)[1].reshape(n, H, 64)
        else:
            self.q_bits, q = to_t(3.0 * K_SCALE * rng.standard_normal((n, d), dtype=np.float32), dtype)
            self.q = q.reshape(n, H, 64)
        self.cache_bits = to_t(_normal(rng, (n_slots, LAYERS, 2, H, n_ctx, 64)), dtype)[0]
        if kind == "self":
            self.cache_bits[:, :, 0, H - 1] = to_t(0.25 * from_t(self.cache_bits[:, :, 0, H - 1], dtype), dtype)[0]
        # one late key per (slot, head), times 4 and turned towards the q of the slot's first token, so that
        # the maximum is late and the keys next to an edge carry weight: the last cached key on even heads,
        # the row one past the end on odd heads (or wherever `spike` puts it)
        cached = self.n_kv - 1 if kind == "self" else self.n_kv  # rows read from the cache
        seen = set()
        for i in range(n):
            s = int(self.slot[i])
            if s in seen:
                continue
            seen.add(s)
            for h in range(H - 1 if kind == "self" else H):
                if spike is not None:
                    if s not in spike:
                        continue
                    r, i_q = spike[s]
                else:
                    last, past = int(cached[i]) - 1, int(self.n_kv[i])
                    r = last if (h % 2 == 0 and last >= 0) or past >= n_ctx else past
                    i_q = i
                    if r < 0:
                        continue
                row = 4.0 * from_t(self.cache_bits[s, LAYER, 0, h, r], dtype)
                if float(row.astype(np.float64) @ self.q[i_q, h].astype(np.float64)) < 0:
                    row = -row
                self.cache_bits[s, LAYER, 0, h, r] = to_t(row, dtype)[0]
        self._planes = {}

    def plane(self, s, layer):
        """float32 values of cache[s][layer] as rows [2 * H * n_ctx + 1][64] (a zero row closes it)"""
        key = (int(s), layer)
        if key not in self._planes:
            v = from_t(self.cache_bits[key[0], layer], self.dtype).reshape(-1, 64)
            self._planes[key] = np.concatenate([v, np.zeros((1, 64), np.float32)])
        return self._planes[key]

    def rows(self, i, h):
        """(q [64], K [n_kv][64], V [n_kv][64]) of token i, head h, as the kernel must read them"""
        ctx, n_c = self.n_ctx, int(self.n_kv[i]) - (self.kind == "self")
        P = self.plane(self.slot[i], LAYER)
        K, V = P[h * ctx:h * ctx + n_c], P[(self.H + h) * ctx:(self.H + h) * ctx + n_c]
        if self.kind == "self":
            K, V = np.concatenate([K, self.k_new[i, h][None]]), np.concatenate([V, self.v_new[i, h][None]])
        return self.q[i, h], K, V

    def expected(self, mut=None, emu=False):
        """reference() of every (token, head) -> out [n][d], mag [n][d], applied [n] (all True for mut None).
        emu: emulate() instead (mag is zero). mut: one of MUTATIONS, the deliberately wrong reading; tokens it
        cannot apply to keep applied[i] = False and zero rows.
        Tokens of one slot share their K and V rows, so their scores are one matrix product per head; the
        key range of every token is a mask over the columns, and a self step's fresh key one more column."""
        n, H, ctx = self.n, self.H, self.n_ctx
        fresh = self.kind == "self"
        ft = np.float32 if emu else np.float64
        out, mag, applied = np.zeros((n, self.d)), np.zeros((n, self.d)), np.zeros(n, bool)
        if mut in ("no_fresh", "fresh_twice") and not fresh:
            return out, mag, applied
        nk = self.n_kv.astype(np.int64)
        n_c = nk - 1 if fresh else nk  # rows read from the cache
        take, ok = n_c.copy(), np.ones(n, bool)
        n_fresh = np.full(n, 1.0 if fresh else 0.0)
        if mut == "drop_last":  # the last cached key (a chunk tail); a self step's fresh key stays
            ok = n_c >= (1 if fresh else 2)
            take = n_c - 1
        elif mut == "one_past":  # one more cache row (in a self step: the row after the fresh key's)
            ok = nk < ctx
        elif mut == "no_fresh":
            ok, n_fresh = n_c >= 1, n_fresh * 0.0
        elif mut == "fresh_twice":
            n_fresh = n_fresh * 2.0
        first = (nk - 1) // CHUNK[self.kind] * CHUNK[self.kind]  # first key of the last chunk
        if mut == "no_norm_tail":
            ok = first > 0
        cols = np.arange(ctx + 1)
        for s in np.unique(self.slot):
            idx = np.flatnonzero((self.slot == s) & ok)
            if len(idx) == 0:
                continue
            s_eff = (int(s) + 1) % self.n_slots if mut == "slot+1" else int(s)
            P = self.plane(s_eff, 0 if mut == "layer0" else LAYER)
            mask = cols[None, :] < take[idx, None]
            if mut == "one_past":
                mask |= cols[None, :] == nk[idx, None]
            for h in range(H):
                hv = (h + 1) % H if mut == "v_head+1" else h
                Kc = P[h * ctx:h * ctx + ctx + 1].astype(ft)
                Vc = P[(H + hv) * ctx:(H + hv) * ctx + ctx + 1].astype(ft)
                q = self.q[idx, h].astype(ft)
                sc = np.where(mask, q @ Kc.T, -np.inf)
                sf = np.full(len(idx), -np.inf, ft)
                vf = np.zeros((len(idx), 64), ft)
                if fresh:
                    sf = np.where(n_fresh[idx] > 0, np.einsum("ie,ie->i", q, self.k_new[idx, h].astype(ft)), -np.inf)
                    vf = self.v_new[idx, hv].astype(ft)
                mx = np.maximum(sc.max(1), sf)
                e = np.exp(sc - mx[:, None])
                ef = (n_fresh[idx] * np.exp(sf - mx)).astype(ft)
                if mut == "no_norm_tail":  # the last chunk's partial sum lost (the fresh key is in that chunk)
                    den = np.where(cols[None, :] < first[idx, None], e, 0).sum(1, dtype=ft)
                else:
                    den = e.sum(1, dtype=ft) + ef
                p, pf = e / den[:, None], ef / den
                if emu:
                    p, pf = to_t(p, self.dtype)[1], to_t(pf, self.dtype)[1]
                o = p @ Vc + pf[:, None] * vf
                if emu:
                    o = to_t(o, self.dtype)[1]
                else:
                    mag[idx, h * 64:(h + 1) * 64] = p @ np.abs(Vc) + pf[:, None] * np.abs(vf)
                out[idx, h * 64:(h + 1) * 64] = o
            applied[idx] = True
        return out, mag, applied


# Keys per pass of a workgroup over the cache: 8 lane groups x 8 rows in the self step, 32 x 8 in the
# 256-thread cross step (128 x 4 = 512 in the 1024-thread one: the smaller chunk is the harder mutation), the
# 64-key tiles of the prefill.
CHUNK = {"self": 64, "cross": 256, "prefill_self": 64, "prefill_cross": 64}

# Deliberately wrong readings that the bound must notice (tests/test_attn_ref.py); the two about the
# fresh key apply to the self step only.
MUTATIONS = ["drop_last", "one_past", "no_fresh", "fresh_twice", "v_head+1", "slot+1", "layer0", "no_norm_tail"]


# ---- the case lists ------------------------------------------------------------------------------------
EDGE_POS = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 446, 447]
# (n, H, splits, positions or None = EDGE_POS and random ones over the 33 rows): HPB 1 (n <= 32), HPB 2
# (H % 4 != 0), HPB 4, and 20 heads; every shape sees 0, 64 and 447
SELF_CASES = [
    (3, 6, 1, [0, 64, 447]), (3, 6, 5, [1, 65, 446]), (3, 6, 16, [447, 0, 64]),
    (33, 6, 5, None), (33, 8, 16, None), (33, 8, 1, None),
    (2, 20, 1, [0, 447]), (2, 20, 5, [64, 127]), (2, 20, 16, [447, 64]),
]
# (n, n_ctx, splits, n_kv): n = 3 takes the 1024-thread kernel, n = 9 the 256-thread one; 1500 in every
# launch, the chunk edges of both widths (32 lane groups x 8 rows, 128 x 4) mixed over the rows; 1536 is
# the LDS limit
_W = [[1500, 1, 7], [8, 1500, 31], [32, 33, 1500], [1500, 255, 256], [257, 1500, 511], [512, 513, 1500],
      [1500, 1023, 1024], [1025, 1500, 1030], [1500, 1500, 1500]]
_W36 = [[1536, 1500, 1025], [1500, 1536, 513], [33, 1500, 1536]]
CROSS_CASES = [(3, 1500, (1, 16)[j % 2], w) for j, w in enumerate(_W)] + \
    [(3, 1536, (16, 1)[j % 2], w) for j, w in enumerate(_W36)] + \
    [(9, 1500, 16, _W[0] + _W[1] + _W[2]), (9, 1500, 1, _W[3] + _W[4] + _W[5]),
     (9, 1500, 16, _W[6] + _W[7] + _W[8]), (9, 1500, 1, [1500] * 9), (9, 1536, 1, _W36[0] + _W36[1] + _W36[2])]
# Prefill: runs of (slot, first position, tokens) over two clips of a three-slot cache. Tiles by the rule
# of decoder_upload: 64, 64, 42 | 11 (kv_end 71 crosses a key tile inside the query tile) | 1 (position
# 447) | 15 | 16 | 17 | 64 (ends at 447).
PREFILL_RUNS = [(1, 0, 170), (0, 60, 11), (1, 447, 1), (0, 100, 15), (1, 200, 16), (0, 300, 17), (1, 384, 64)]
PREFILL_SPIKE = {1: 100, 0: 65}  # slot -> the late key's row (inside a run: its token's last key, the one
#                                  before's one-past key)
PREFILL_CASES = [("prefill_self", 6), ("prefill_self", 20), ("prefill_cross", 6), ("prefill_cross", 20)]


def self_case(dtype, n, H, splits, pos):
    rng = np.random.default_rng(n * 1000 + H * 10 + splits)
    if pos is None:
        pos = np.concatenate([EDGE_POS, rng.integers(0, 448, n - len(EDGE_POS))])
        pos = pos[rng.permutation(n)]
    pos = np.asarray(pos)
    n_slots = n + 1
    slot = (n_slots - 1 - rng.permutation(n_slots))[:n]  # distinct
    if (slot == np.arange(n)).all():
        slot = slot[::-1].copy()
    return Case("self", dtype, f"self n={n} H={H} splits={splits}", 448, H, slot, pos + 1, n_slots, splits,
                seed=n * 77 + H + splits)


def cross_case(dtype, n, n_ctx, splits, n_kv):
    rng = np.random.default_rng(n * 1000 + n_ctx + splits + n_kv[1])
    n_slots = 4 if n == 3 else 6
    slot = rng.permutation(n_slots)[::-1][:n] if n == 3 else \
        np.concatenate([rng.permutation(n_slots), rng.integers(0, n_slots, n - n_slots)])  # slots repeat
    return Case("cross", dtype, f"cross n={n} n_ctx={n_ctx} splits={splits} n_kv={n_kv}", n_ctx, 6, slot, n_kv,
                n_slots, splits, seed=n * 31 + n_ctx + splits + n_kv[1] + n_kv[2])


def prefill_tokens():
    slot = np.concatenate([np.full(c, s) for s, p, c in PREFILL_RUNS]).astype(np.int32)
    pos = np.concatenate([np.arange(p, p + c) for s, p, c in PREFILL_RUNS]).astype(np.int32)
    return slot, pos


def prefill_tiles(slot, pos):
    """decoder_upload's rule: a tile is a run of consecutive tokens of one slot with increasing positions,
    at most 64 of them -> [first token, count] pairs"""
    tiles = []
    for i in range(len(slot)):
        if i > 0 and slot[i] == slot[i - 1] and pos[i] > pos[i - 1] and tiles[-1][1] < 64:
            tiles[-1][1] += 1
        else:
            tiles.append([i, 1])
    return np.asarray(tiles, np.int32)


def prefill_case(dtype, kind, H):
    slot, pos = prefill_tokens()
    if kind == "prefill_self":
        n_ctx, n_kv = 448, pos + 1
        spike = {s: (r, int(np.flatnonzero((slot == s) & (pos == r))[0])) for s, r in PREFILL_SPIKE.items()}
    else:
        n_ctx, n_kv = 1500, np.full(len(pos), 1500)
        spike = {s: (1499, int(np.flatnonzero(slot == s)[0])) for s in PREFILL_SPIKE}
    c = Case(kind, dtype, f"{kind} H={H}", n_ctx, H, slot, n_kv, 3, spike=spike, seed=H + n_ctx)
    c.pos, c.tiles = pos, prefill_tiles(slot, pos)
    return c


def all_cases(dtype):
    """every case of the GPU tests, as a function that builds it (the caches are large: one at a time)"""
    for a in SELF_CASES:
        yield (lambda a=a: self_case(dtype, *a))
    for a in CROSS_CASES:
        yield (lambda a=a: cross_case(dtype, *a))
    for a in PREFILL_CASES:
        yield (lambda a=a: prefill_case(dtype, *a))
