"""Block-quantized files under the teacher-forced logits bound (f16).

tests/test_quant.py and test_gpu_pdec.py hold whisper_full on quantized files to the oracle's tokens, on clips
without a close call; a wrong weight that moves logits without flipping one of those tokens passes there. Here
the raw logits of every step of a fixed-work run (128 steps, teacher-forced along the oracle's own sequence:
the mechanism of test_gpu_fulldepth.test_largev3_few_clips_teacher_forced) are held to the f16 bar of the
plain files, F16_REL_TOL = 1e-3 of the step's largest |logit| with no argmax flip above F16_FLIP_GAP: oracle
mode 1 feeds its matmuls the same f16-rounded dequantized operands, so the bound's argument carries over.

Shape small-4L+conf (d = 768, the smallest width with a block-reading persistent kernel), every decode step
one persistent launch (kernel class 7 counts them):
  - whisper_mi355x_set_pdec_blocks(1), 1 clip, all five types: deq8 and the block layout of the persistent
    kernel (kernels/pdec_body.h), q4_0 included (its whisper_full file, tiny.en, has no persistent kernel);
  - q5_0 at 3 clips: the persistent kernel's form for more than 2 rows;
  - q5_0 with blocks 0: the persistent kernel on the context's expanded copy (dequant_multi_kernel's output).
And tiny.en+conf+q4_0 at 1 clip, also with set_pdec_blocks(1): d = 384 has no block-reading persistent kernel, so
the step runs as the small-M GEMMs reading the blocks (gemm_small_kernel; zero persistent launches asserted).
With blocks 0 the plain persistent kernel would run on the expanded copy, as in the case above.
"""
import ctypes as C

import numpy as np
import pytest

from make_model import synthetic_pcm
from test_gpu_fulldepth import N_TOK, _check, _oracle_logits, _oracle_seq

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

K_PDEC = 7

CASES = [("small-4L+conf+" + q, 1, 1, True) for q in ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0")] + [
    ("small-4L+conf+q5_0", 3, 1, True), ("small-4L+conf+q5_0", 1, 0, True), ("tiny.en+conf+q4_0", 1, 1, False)]


@pytest.mark.parametrize("shape,n_clips,blocks,persistent", CASES)
def test_quant_teacher_forced_logits(wrs, monkeypatch, shape, n_clips, blocks, persistent):
    from conftest import model_path
    monkeypatch.delenv("WHISPER_MI355X_CROSS", raising=False)
    clips = list(range(n_clips))
    seqs = np.array([_oracle_seq(c, shape) for c in clips], np.int32)
    L = wrs.lib()
    L.whisper_mi355x_set_pdec_blocks(blocks)
    try:
        ctx = wrs.WhisperContext(model_path(shape), dtype=wrs.F16)
        st = ctx.create_state()
        L.whisper_mi355x_kernel_timing(st.ptr, 1 << K_PDEC)
        V = L.whisper_n_vocab(ctx.ptr)
        rc, lg = st.full_batch_forced(wrs.reference_full_params("en"), [synthetic_pcm(c) for c in clips], N_TOK, seqs,
                                      clips, V)
        assert rc == 0, rc
        out = (C.c_double * 3)()
        assert L.whisper_mi355x_kernel_stats(st.ptr, K_PDEC, out) == 0
        info, launches, gave_up = st.info(), int(out[1]), st.pdec_give_ups()
        st.close()
        ctx.close()
    finally:
        L.whisper_mi355x_set_pdec_blocks(0)
    assert not info["direct"], info
    assert gave_up == 0
    if persistent:
        assert launches >= N_TOK - 1, launches  # every step after the prompt's
    else:
        assert launches == 0, launches
    for k, c in enumerate(clips):
        _check("F16", c, lg[:, k, :], _oracle_logits(c, shape), f"b{n_clips} blocks {blocks}", shape)
