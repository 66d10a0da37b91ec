"""The GEMM launch plan (nobs-whisper_amd/csrc/gemm_plan.cpp, free of HIP: which kernel, tile, split and reduce a call
gets) against tests/gemm_plan_ref.py, the launcher's decision before the plan existed, on the CPU:
tools/gemm_plan_check.cpp is built with plain g++ and fed every shape of the grid below; every field of every plan
must equal the reference. A second build with -fsanitize=address,undefined runs the same input (a program with its
own main).

Grid, for d in 384..1280 and n_vocab in 51864..51866: the encoder and cross-K/V shapes (M = B * A), prefills, and
every decode / logits step of 1..260 rows; each without a workspace, with exactly the slabs the decode split needs,
one element less, and the engine's size; fused LayerNorm and e4m3 weights on and off; the knobs at their defaults and
one moved at a time. At the defaults every (workspace, fused_ln, w8) combination runs; with a knob moved, every
workspace runs plain and the engine's workspace runs the other three (fused_ln, w8) pairs.
"""
import os
import shutil
import subprocess

import pytest

import gemm_plan_ref as ref
from conftest import ROOT

DS = (384, 512, 768, 1024, 1280)
VOCABS = (51864, 51865, 51866)
DEFAULT = dict(variant=-1, dec_splits=0, dec_bm=32, gm_env=-1)
KNOBS = [DEFAULT] + [dict(DEFAULT, **{k: v}) for k, vs in (("variant", (0, 1, 2, 3)), ("dec_splits", (1, 5, 16)),
                                                         ("dec_bm", (64, 128)), ("gm_env", (0, 8))) for v in vs]


def engine_ws(n_jobs, d):
    """Workspace::splitk_elems of a state sized for n_jobs clips (engine.cpp; n_text_ctx = 448)."""
    n_tok = n_jobs * (448 // 2 + 8)
    return max(16 * min(n_tok, 256) * 4 * d, min(16384 * n_tok, 12 << 22))


PART_N = set(DS) | {3 * d for d in DS}  # the projections whose slabs the attention prologues reduce (launch_gemm_partials)


def shapes():
    """(M, N, K, the engine's workspace for the call), each once."""
    out = set()
    for d in DS:
        for B in (1, 2, 32, 128):
            for A in (1500, 750, 100):
                for N in (d, 3 * d, 4 * d, 2 * 4 * d, 2 * 32 * d):
                    for K in (d, 4 * d, 3 * 80, 3 * 128, 3 * d):
                        out.add((B * A, N, K, engine_ws(B, d)))
        for V in VOCABS:
            nk = ((d, d), (d, 4 * d), (3 * d, d), (4 * d, d), (V, d))
            for M in (1, 3, 8, 229, 1024, 5000):
                out.update((M, N, K, engine_ws(ref.cdiv(M, 232), d)) for N, K in nk)
            for M in range(1, 261):
                out.update((M, N, K, engine_ws(M, d)) for N, K in nk)
    return sorted(out)


def cases():
    """(input line of the program, the reference's output line)."""
    rows = []
    for M, N, K, ws_engine in shapes():
        # the slabs of the decode split (dec_plan with room to spare), to the element
        exact = (ref.dec_plan(N, K, M, 1 << 62, 0)[0] if K % 64 == 0 else 2) * M * N
        wss = ((0, 0), (1, exact), (1, exact - 1), (1, ws_engine))
        for kn in KNOBS:
            for wi, (has_ws, ws) in enumerate(wss):
                for ln, w8 in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    if kn is not DEFAULT and (ln or w8) and wi != 3:
                        continue
                    # logits are EPI_F32, a fused LayerNorm is EPI_RESID's, the d-wide projections are residual adds
                    epis = (ref.EPI_RESID,) if ln else (ref.EPI_F32,) if N in VOCABS else \
                        (ref.EPI_STORE, ref.EPI_RESID) if N in DS else (ref.EPI_STORE,)
                    for epi in epis:
                        rows.append(("%d %d %d %d %d %d %d %d %d %d %d %d" % (epi, M, N, K, has_ws, ws, ln, w8, kn["variant"],
                                                                            kn["dec_splits"], kn["dec_bm"], kn["gm_env"]),
                                     ref.line(ref.plan(epi, M, N, K, has_ws, ws, ln, w8, **kn))))
                if M <= 260 and N in PART_N and kn["variant"] == -1 and kn["gm_env"] == -1:
                    rows.append(("0 %d %d %d %d %d 0 0 -1 %d %d -1 1" % (M, N, K, has_ws, ws, kn["dec_splits"], kn["dec_bm"]),
                                 ref.line(ref.partials(M, N, K, has_ws, ws, kn["dec_splits"], kn["dec_bm"]))))
    return rows


def build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp / name)
    csrc = os.path.join(ROOT, "nobs-whisper_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I", csrc, os.path.join(ROOT, "tools", "gemm_plan_check.cpp"),
                    os.path.join(csrc, "gemm_plan.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gemm_plan")
    return {"plain": build(tmp, "gemm_plan_check", []),
            "san": build(tmp, "gemm_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


@pytest.fixture(scope="module")
def grid():
    return cases()


def run(prog, lines):
    r = subprocess.run([prog], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("which", ["plain", "san"])
def test_plan_matches_reference(progs, grid, which):
    got = run(progs[which], [c[0] for c in grid])
    bad = [(c[0], g, c[1]) for c, g in zip(grid, got) if g != c[1]]
    assert not bad, "%d of %d plans differ; first (input, plan, reference): %s" % (len(bad), len(grid), bad[:3])


def test_grid_reaches_every_arm(grid):
    """The grid is only a check if it visits every kernel, tile, reduce and failure of the launcher."""
    seen = set()
    for _, want in grid:
        f = want.split()
        seen.add(" ".join(f[:4]) if f[0] in ("error", "none") else (f[0], f[1], f[2], f[8], f[12]))
    for k in [("8p", "256", "256", "0", "none"), ("glds", "128", "128", "0", "none"), ("reg", "128", "128", "0", "none"),
              ("reg", "64", "64", "0", "none"), ("reg", "128", "64", "0", "none"), ("reg", "64", "64", "1", "plain"),
              ("reg", "128", "64", "1", "plain"), ("reg", "64", "64", "1", "ln"), ("reg", "128", "64", "1", "ln"),
              ("dec", "32", "64", "1", "plain"), ("dec", "64", "64", "1", "ln4"), ("dec", "128", "64", "1", "none"),
              ("dec", "128", "64", "0", "none"), ("dec", "128", "64", "1", "ln4"), "none",
              "error e4m3 weights need", "error e4m3 decode GEMM:", "error fused LN width", "error fused LN requires"]:
        assert k in seen, k


def logits_plan(prog, d, V, rows):
    lines = ["%d %d %d %d 1 %d 0 0 -1 0 32 -1" % (ref.EPI_F32, n, V, d, engine_ws(n, d)) for n in rows]
    return [l.split() for l in run(prog, lines)]


def test_step_variant_key_is_n_le_64(progs):
    """engine.cpp step_variant's logits-GEMM bit, "the plan is gemm_kernel at the 64-row tile", is n <= 64 for every
    model shape the engine loads: the key's classes are what they were."""
    for d in DS:
        for V in VOCABS:
            for n, f in zip(range(1, 129), logits_plan(progs["plain"], d, V, range(1, 129))):
                assert (f[0] == "reg" and f[1] == "64") == (n <= 64), (d, V, n, f)


def test_logits_kernel_changes_at_81_rows(progs):
    """Rows 65..80 of a logits GEMM take gemm_dec_kernel unsplit, 81..128 gemm_glds_kernel (M * N reaches 2^22); that
    the two give a row the same bits is tests/test_gpu_kernels.py test_logits_gemm_rows_80_81_bitwise."""
    for d in DS:
        for V in VOCABS:
            p = logits_plan(progs["plain"], d, V, (65, 80, 81, 128))
            assert [f[0] for f in p] == ["dec", "dec", "glds", "glds"], (d, V, p)
            assert all(f[8] == "0" and f[12] == "none" for f in p), (d, V, p)
