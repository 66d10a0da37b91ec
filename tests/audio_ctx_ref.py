"""The reference for whisper_full_params.audio_ctx -- TEST INFRASTRUCTURE ONLY.

The CPU oracle has no audio_ctx parameter and needs none: a model file rewritten with n_audio_ctx = A in its
header and encoder.positional_embedding cut to its first A rows, every other byte as it was, IS whisper.cpp at
audio_ctx = A when the oracle loads it (the mel window of a seek is 2A frames, the conv stem yields A positions,
every layer and every cross attention sees A positions).

One difference: the oracle takes the timestamp precision 30 / n_audio_ctx from the file, the library (as upstream)
keeps the model's. `oracle_params_at` therefore scales max_initial_ts by 1500 / A, so that both sides cut the
initial timestamp at tid0 = 50.
"""
from __future__ import annotations

import os
import struct

import numpy as np

POS_EMB = "encoder.positional_embedding"
BLOCK_BYTES = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34}  # tools/make_model.py


def _walk(buf: bytes):
    """Offsets of a GGML whisper file (tools/make_model.py:read_tensors documents the layout): the end of the part
    before the tensors, then per tensor (record offset, n_dims, type, ne, name, data offset, data bytes)."""
    o = 4 + 11 * 4
    n_mel, n_fft = struct.unpack_from("<2i", buf, o)
    o += 8 + 4 * n_mel * n_fft
    (n_tok,) = struct.unpack_from("<i", buf, o)
    o += 4
    for _ in range(n_tok):
        (ln,) = struct.unpack_from("<I", buf, o)
        o += 4 + ln
    recs = []
    while o < len(buf):
        r0 = o
        nd, nl, tt = struct.unpack_from("<3i", buf, o)
        o += 12
        ne = struct.unpack_from(f"<{nd}i", buf, o)
        o += 4 * nd
        name = buf[o:o + nl].decode()
        o += nl
        nel = int(np.prod(ne))
        nbytes = nel * 4 if tt == 0 else nel * 2 if tt == 1 else nel // 32 * BLOCK_BYTES[tt]
        recs.append((r0, nd, tt, ne, name, o, nbytes))
        o += nbytes
    assert o == len(buf), "trailing bytes after the last tensor"
    return recs


def truncate_bytes(buf: bytes, A: int) -> bytes:
    n_ctx = struct.unpack_from("<i", buf, 8)[0]
    assert 1 <= A <= n_ctx, (A, n_ctx)
    out = bytearray(buf[:8]) + struct.pack("<i", A)
    pos = 12
    done = False
    for r0, nd, tt, ne, name, d0, nbytes in _walk(buf):
        if name != POS_EMB:
            continue
        assert not done and nd == 2 and tt == 0 and ne[1] == n_ctx, (nd, tt, ne)
        d = ne[0]
        ne_off = r0 + 12  # ne[0], ne[1] (innermost first: [d, n_audio_ctx])
        out += buf[pos:ne_off + 4] + struct.pack("<i", A) + buf[ne_off + 8:d0] + buf[d0:d0 + A * d * 4]
        pos = d0 + nbytes
        done = True
    assert done, f"no {POS_EMB} in the file"
    out += buf[pos:]
    return bytes(out)


def truncated_model(path: str, A: int) -> str:
    """`path` with n_audio_ctx = A and the encoder positional embedding cut to A rows, written once under conftest's
    MODEL_DIR (A = the file's own n_audio_ctx: a byte-identical copy)."""
    from conftest import MODEL_DIR
    os.makedirs(MODEL_DIR, exist_ok=True)
    base = os.path.basename(path)
    stem = base[:-4] if base.endswith(".bin") else base
    out = os.path.join(MODEL_DIR, f"{stem}_actx{A}.bin")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(path):
        with open(path, "rb") as f:
            buf = f.read()
        tmp = f"{out}.{os.getpid()}.tmp"
        with open(tmp, "wb") as f:
            f.write(truncate_bytes(buf, A))
        os.replace(tmp, out)
    return out


def oracle_params_at(A: int, lang: str | None = "en", t_inc: float = 0.0, n_audio_ctx: int = 1500, best_of: int = 1):
    """reference_params for an oracle run on a file truncated to A: max_initial_ts scaled so that tid0 = 50."""
    from oracle_py import reference_params
    rp = reference_params(lang)
    rp.temperature_inc = t_inc
    rp.max_initial_ts = 1.0 * n_audio_ctx / A
    rp.best_of = best_of
    return rp


def oracle_full_at(shape: str, A: int, clip: int, lang: str | None = "en", t_inc: float = 0.0, best_of: int = 1) -> dict:
    """The oracle's whisper_full of synthetic_pcm(clip) (30 s) at audio_ctx = A, once per session."""
    from conftest import model_path
    from make_model import synthetic_pcm
    from oracle_py import cached_full
    return cached_full(truncated_model(model_path(shape), A), ("clip", clip), lambda: synthetic_pcm(clip),
                       oracle_params_at(A, lang, t_inc, best_of=best_of))
