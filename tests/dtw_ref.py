"""numpy reference of the token-timestamp alignment (DESIGN.md "Token timestamps (DTW)") — TEST
INFRASTRUCTURE ONLY. The contract pipeline: softmaxed cross-attention rows of the alignment heads ->
per-(head, frame) z-score over the token rows -> width-7 median along the frames -> head mean, negated,
rows n_sot .. n-2 -> OpenAI's dtw_cpu in float32 -> first frame of every row.

Arithmetic that must be accurate is float64; the DTW, whose bits are compared, is a sequential float32
loop. DecoderRef is a float64 decoder forward from the oracle's tensors, independent of the engine's
decoder and of the oracle's own cross K/V.
"""
from __future__ import annotations

import numpy as np

MEDIAN_WIDTH = 7


def reflect_indices(F: int, width: int = MEDIAN_WIDTH) -> np.ndarray:
    """[F][width] source frames of a median window: reflected without repeating the edge (i < 0 -> -i,
    i >= F -> 2(F-1) - i), then clamped to [0, F-1] (the clamp matters only for F < 4)."""
    half = width // 2
    idx = np.arange(F)[:, None] + np.arange(-half, half + 1)[None, :]
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= F, 2 * (F - 1) - idx, idx)
    return np.clip(idx, 0, F - 1)


def median_filter(x: np.ndarray, width: int = MEDIAN_WIDTH) -> np.ndarray:
    """median of `width` along the last axis with the reflected borders above"""
    idx = reflect_indices(x.shape[-1], width)
    return np.median(x[..., idx], axis=-1)


def cost_matrix(P: np.ndarray, n_sot: int, median: bool = True) -> np.ndarray:
    """P [A][n][F] (softmaxed rows, frames >= F already dropped) -> cost [n - n_sot - 1][F], float64.
    median=False omits the filter (the discrimination checks of the tests)."""
    P = np.asarray(P, np.float64)
    mu = P.mean(axis=1, keepdims=True)
    var = P.var(axis=1, keepdims=True)  # population variance
    Z = (P - mu) / np.sqrt(var + 1e-9)
    if median:
        Z = median_filter(Z)
    cost = -Z.mean(axis=0)
    return cost[n_sot:P.shape[1] - 1]


def dtw_f32(cost: np.ndarray):
    """OpenAI's dtw_cpu as a sequential float32 loop. C[i][j] = cost[i-1][j-1] + min(c0, c1, c2); trace 0 if c0
    is strictly the smallest, else 1 if c1 is, else 2. Returns (fr [N] first frame of every row, path
    [(row, frame)] from the last cell back to (0, 0), trace [N+1][F+1])."""
    cost = np.ascontiguousarray(cost, np.float32)
    N, F = cost.shape
    inf = np.float32(np.inf)
    prev = [np.float32(0.0)] + [inf] * F
    trace = np.full((N + 1, F + 1), -1, np.int8)
    trace[0, :] = 2
    trace[:, 0] = 1
    for i in range(1, N + 1):
        ci = list(cost[i - 1])
        cur = [inf] * (F + 1)
        tr = [1] * (F + 1)
        left = inf
        for j in range(1, F + 1):
            c0, c1, c2 = prev[j - 1], prev[j], left
            if c0 < c1 and c0 < c2:
                t = 0
            elif c1 < c0 and c1 < c2:
                t = 1
            else:
                t = 2
            left = ci[j - 1] + min(c0, c1, c2)  # one float32 add
            cur[j] = left
            tr[j] = t
        trace[i, :] = tr
        prev = cur
    i, j = N, F
    path = []
    fr = np.full(N, -1, np.int64)
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        if i > 0 and j > 0:
            fr[i - 1] = j - 1  # walking backwards: the last one seen in a row is its first frame
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return fr, path, trace


def first_frames(path, N: int) -> np.ndarray:
    fr = np.full(N, -1, np.int64)
    for r, f in reversed(path):  # forward order
        if r >= 0 and f >= 0 and fr[r] < 0:
            fr[r] = f
    return fr


# ---- float64 decoder forward from the oracle's tensors -------------------------------------------------
def _ln(x, w, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * w + b


def _gelu(x):  # ggml's tanh form
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * x * (1.0 + 0.044715 * x * x)))


def _softmax(s):
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


class DecoderRef:
    """Teacher-forced decoder forward in float64 over an encoder output; returns the softmaxed cross-attention
    rows of the requested heads."""

    def __init__(self, oracle):
        self.o = oracle
        self.d, self.H, self.L = oracle.d, oracle.n_head, oracle.n_dec
        self._t = {}

    def t(self, name, shape=None, lookup=False):
        key = (name, lookup)
        if key not in self._t:
            a = self.o.tensor(name, lookup=lookup).astype(np.float64)
            self._t[key] = a.reshape(shape) if shape else a
        return self._t[key]

    def cross_probs(self, tokens, enc, heads) -> np.ndarray:
        """tokens at positions 0.., enc [T][d] -> P [len(heads)][n][T]"""
        d, H = self.d, self.H
        dh = d // H
        n = len(tokens)
        enc = np.asarray(enc, np.float64)
        te = self.t("decoder.token_embedding.weight", (-1, d), lookup=True)
        pe = self.t("decoder.positional_embedding", (-1, d))
        x = te[np.asarray(tokens)] + pe[:n]
        out = [None] * len(heads)
        last = max(l for l, _ in heads)
        causal = np.triu(np.full((n, n), -np.inf), 1)
        for l in range(last + 1):
            p = f"decoder.blocks.{l}."
            W = lambda nm: self.t(p + nm + ".weight", (-1, d) if "mlp.2" not in nm else (d, -1))  # noqa: E731
            B = lambda nm: self.t(p + nm + ".bias")  # noqa: E731
            h = _ln(x, self.t(p + "attn_ln.weight"), self.t(p + "attn_ln.bias"))
            q = (h @ W("attn.query").T + B("attn.query")).reshape(n, H, dh)
            k = (h @ W("attn.key").T).reshape(n, H, dh)
            v = (h @ W("attn.value").T + B("attn.value")).reshape(n, H, dh)
            s = np.einsum("ihc,jhc->hij", q, k) / np.sqrt(dh) + causal[None]
            att = np.einsum("hij,jhc->ihc", _softmax(s), v).reshape(n, d)
            x = x + att @ W("attn.out").T + B("attn.out")
            h = _ln(x, self.t(p + "cross_attn_ln.weight"), self.t(p + "cross_attn_ln.bias"))
            q = (h @ W("cross_attn.query").T + B("cross_attn.query")).reshape(n, H, dh)
            K = (enc @ W("cross_attn.key").T).reshape(-1, H, dh)
            V = (enc @ W("cross_attn.value").T + B("cross_attn.value")).reshape(-1, H, dh)
            Pc = _softmax(np.einsum("ihc,thc->hit", q, K) / np.sqrt(dh))
            for a, (hl, hh) in enumerate(heads):
                if hl == l:
                    out[a] = Pc[hh]
            if l == last:
                break
            x = x + np.einsum("hit,thc->ihc", Pc, V).reshape(n, d) @ W("cross_attn.out").T + B("cross_attn.out")
            h = _ln(x, self.t(p + "mlp_ln.weight"), self.t(p + "mlp_ln.bias"))
            ff = _gelu(h @ self.t(p + "mlp.0.weight", (-1, d)).T + self.t(p + "mlp.0.bias"))
            x = x + ff @ self.t(p + "mlp.2.weight", (d, -1)).T + self.t(p + "mlp.2.bias")
        return np.stack(out)

    def cost(self, tokens, enc, heads, n_sot: int, F: int, median: bool = True) -> np.ndarray:
        return cost_matrix(self.cross_probs(tokens, enc, heads)[:, :, :F], n_sot, median)
