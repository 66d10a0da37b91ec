"""whisper_full_parallel's host code that needs no HIP (nobs-whisper_amd/csrc/parallel.{h,cpp}: the cuts, the snap choice, the
merge loop the engine runs) against tests/parallel_ref.py, on the CPU: tools/parallel_check.cpp is built with plain g++ and
fed the hand cases of test_parallel_ref.py and seeded random ones; every integer must equal the reference's. A second build
with -fsanitize=address,undefined runs the same script. Also the two new symbols at the C ABI, without a device."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import parallel_ref as pr
import test_parallel_ref as tp


def build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp / name)
    csrc = os.path.join(ROOT, "nobs-whisper_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I", csrc, os.path.join(ROOT, "tools", "parallel_check.cpp"),
                    os.path.join(csrc, "parallel.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parallel_check")
    return {"plain": build(tmp, "parallel_check", []),
            "san": build(tmp, "parallel_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def split_cases():
    out = [(n, off, np_) for _, n, off, np_, _, _ in tp.SPLIT]
    rng = random.Random(20251021)
    for _ in range(200):
        np_ = rng.choice([2, 3, 4, 5, 7, 8, 20, 64, 128])
        off = rng.choice([0, 0, 10, 999, 1234, 30000])
        n = pr.offset_samples(off) + rng.randint(np_, 40 * 16000)
        out.append((n, off, np_))
    return out


def snap_cases():
    rng = random.Random(7)
    nrng = np.random.default_rng(7)
    out = []
    for _ in range(200):
        np_ = rng.choice([2, 3, 4, 9])
        off = rng.choice([0, 0, 500])
        n = pr.offset_samples(off) + rng.choice([rng.randint(np_, 4000), rng.randint(4000, 200000)])
        # few distinct levels, so that ties in RMS are common
        rms = nrng.choice(np.asarray([0.0, 0.001, 0.25, 0.5], np.float32), size=n // 320).astype(np.float32)
        out.append((n, off, np_, rng.choice([0, 1, 20, 30, 200, 500, 100000]), rms))
    return out


def merge_cases():
    rng = random.Random(11)
    out = []
    for _ in range(100):
        np_ = rng.randint(2, 6)
        off = rng.choice([0, 0, 1500])
        n = pr.offset_samples(off) + rng.randint(np_ * 16000, np_ * 16000 * 40)
        cuts = pr.cuts(n, off, np_)
        pieces = []
        for _k in range(np_):
            segs, t = [], rng.choice([0, 0, 3])
            for _s in range(rng.randint(0, 4)):
                t1 = t + rng.randint(0, 400)
                toks = [dict(t0=rng.choice([-1, rng.randint(0, 3000)]), t1=rng.choice([-1, rng.randint(0, 3000)]),
                             t_dtw=rng.choice([-1, -1, rng.randint(0, 3000)])) for _t in range(rng.randint(0, 3))]
                segs.append(dict(t0=t, t1=t1, tokens=toks))
                t = t1
            pieces.append(segs)
        out.append((off, cuts, pieces))
    return out


def script_and_expected():
    lines, exp = [], []
    for n, off, np_ in split_cases():
        lines.append(f"cuts {n} {off} {np_}")
        exp.append(" ".join(map(str, pr.cuts(n, off, np_))))
    for n, off, np_, snap_ms, rms in snap_cases():
        lines.append(f"snap {n} {off} {np_} {snap_ms} {len(rms)} " + " ".join(f"{float(r):.9g}" for r in rms))
        exp.append(" ".join(map(str, pr.snapped_cuts(rms, n, off, np_, snap_ms))))
    for off, cuts, pieces in merge_cases():
        words = ["merge", off, len(cuts), *cuts]
        for segs in pieces:
            words.append(len(segs))
            for s in segs:
                words += [s["t0"], s["t1"], len(s["tokens"])]
                for t in s["tokens"]:
                    words += [t["t0"], t["t1"], t["t_dtw"]]
        lines.append(" ".join(map(str, words)))
        merged = pr.merge(pieces, cuts, off)
        exp.append(" | ".join(" ".join(map(str, [s["t0"], s["t1"], len(s["tokens"])] +
                                           [t[k] for t in s["tokens"] for k in ("t0", "t1", "t_dtw")])) for s in merged))
    return "\n".join(lines) + "\n", exp


@pytest.mark.parametrize("which", ["plain", "san"])
def test_host_code_equals_the_reference(progs, which):
    script, exp = script_and_expected()
    r = subprocess.run([progs[which]], input=script, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (i, script.split("\n")[i][:200], g, e)


def test_snapped_cuts_stay_increasing():
    for n, off, np_, snap_ms, rms in snap_cases():
        c = pr.snapped_cuts(rms, n, off, np_, snap_ms)
        assert all(b > a for a, b in zip(c, c[1:])) and c[-1] < n, (n, off, np_, snap_ms, c)


def test_abi_symbols_and_piece_limit(wrs, capfd):
    L = wrs.lib()
    p = L.whisper_full_default_params(wrs.GREEDY)
    # asked before anything else: no context, no device
    assert L.whisper_mi355x_full_parallel(None, None, p, None, 0, 129, 0, False) == -1
    assert "n_processors 129 > 128" in capfd.readouterr().err
    assert L.whisper_full_parallel(None, p, None, 0, 1000) == -1
    assert "n_processors 1000 > 128" in capfd.readouterr().err
    assert L.whisper_full_parallel(None, p, None, 0, 4) == -1          # no context
    assert capfd.readouterr().err == ""
    assert L.whisper_mi355x_parallel_cuts(None, None, 0) == 0
