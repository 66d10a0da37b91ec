"""The VAD host code that needs no HIP (nobs-whisper_amd/csrc/vad_segments.cpp and vad_file.cpp) against tests/vad_ref.py,
on the CPU: tools/vad_check.cpp is built with plain g++ and fed the hand cases of test_vad_ref.py and 200 seeded random
probability sequences and parameter sets; segments, piece tables and mapped times must equal the reference's exactly
(integers in, integers out). A second build with -fsanitize=address,undefined runs the same script, and the loader's
refusals (a file truncated at every record boundary and inside records, another magic, another geometry, an unknown
and a duplicate tensor) must end clean under it."""
import os
import random
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_vad_model as mk  # noqa: E402
import test_vad_ref as tv  # noqa: E402
import vad_ref as vr  # noqa: E402


def build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp / name)
    csrc = os.path.join(ROOT, "nobs-whisper_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I", csrc, os.path.join(ROOT, "tools", "vad_check.cpp"),
                    os.path.join(csrc, "vad_segments.cpp"), os.path.join(csrc, "vad_file.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vad_check")
    return {"plain": build(tmp, "vad_check", []),
            "san": build(tmp, "vad_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def hand_cases():
    out = []
    for _, p, params, _ in tv.HAND:
        n = len(p) * 512
        out.append((np.asarray(p, dtype=np.float32), params, max(0, n - 100), list(range(0, n // 160 + 30, 7))))
    return out


def random_cases(seed=20250917, count=200):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        p = []
        for _ in range(rng.randint(0, 12)):
            v = rng.choice([0.02, 0.2, 0.34, 0.36, 0.4, 0.49, 0.51, 0.6, 0.9, rng.random()])
            p += [v if rng.random() < 0.8 else rng.random() for _ in range(rng.randint(1, 20))]
        params = dict(threshold=rng.choice([0.5, 0.5, 0.3, 0.1, 0.7]), min_speech_duration_ms=rng.choice([0, 64, 250, 250]),
                      min_silence_duration_ms=rng.choice([0, 32, 100, 100, 300]),
                      max_speech_duration_s=rng.choice([float("inf"), float("inf"), 3.4e38, 0.05, 0.5, 1.0, 2.0]),
                      speech_pad_ms=rng.choice([0, 30, 30, 40, 100]), samples_overlap=rng.choice([0.0, 0.1, 0.1, 0.5]))
        n = len(p) * 512
        n_samples = rng.choice([n, max(0, n - rng.randint(0, 511)), max(0, n - rng.randint(0, 511)), n // 2])
        times = sorted(rng.randint(0, n // 160 + 40) for _ in range(30))
        out.append((np.asarray(p, dtype=np.float32), params, n_samples, times))
    return out


def hostile_cases():
    """parameters at and beyond the ranges of int and float: 64-bit arithmetic with clamps, non-finite values as unbounded / none"""
    p = np.asarray(tv.runs((5, tv.LO), (10, tv.HI), (5, tv.LO), (10, tv.HI), (10, tv.LO)), dtype=np.float32)
    out = []
    for kw in [dict(min_speech_duration_ms=2 ** 31 - 1), dict(min_silence_duration_ms=2 ** 31 - 1), dict(speech_pad_ms=2 ** 31 - 1),
               dict(speech_pad_ms=200000), dict(min_speech_duration_ms=-(2 ** 31)), dict(speech_pad_ms=-50),
               dict(max_speech_duration_s=float("nan")), dict(max_speech_duration_s=-float("inf")), dict(max_speech_duration_s=-3.0e38),
               dict(max_speech_duration_s=99999.0), dict(samples_overlap=float("nan")), dict(samples_overlap=float("inf")),
               dict(samples_overlap=3.0e38), dict(samples_overlap=-1.0), dict(samples_overlap=1.0e6)]:
        out.append((p, tv.prm(**kw), len(p) * 512 - 7, list(range(0, 80, 3))))
    return out


def hx(v):
    return float(np.float32(v)).hex()


def script(cases):
    lines = []
    for p, q, n_samples, times in cases:
        lines.append(f"case {hx(q['threshold'])} {q['min_speech_duration_ms']} {q['min_silence_duration_ms']} "
                     f"{hx(q['max_speech_duration_s'])} {q['speech_pad_ms']} {hx(q['samples_overlap'])} {n_samples} {len(p)} {len(times)}")
        lines.append(" ".join(hx(v) for v in p))
        lines.append(" ".join(str(t) for t in times))
    return "\n".join(lines) + "\n"


def reference(cases):
    out = []
    for p, q, n_samples, times in cases:
        segs = vr.segments_from_probs(p, q)
        tab = vr.piece_table(segs, n_samples, q["samples_overlap"])
        out.append((segs, tab, [vr.map_time(tab, t) for t in times]))
    return out


def parse(stdout):
    out, it = [], iter(stdout.split("\n"))
    for ln in it:
        if not ln:
            continue
        w = ln.split()
        assert w[0] == "segs", ln
        segs = [tuple(int(v) for v in next(it).split()) for _ in range(int(w[1]))]
        w = next(it).split()
        assert w[0] == "pieces"
        tab = [tuple(int(v) for v in next(it).split()) for _ in range(int(w[1]))]
        w = next(it).split()
        assert w[0] == "map"
        out.append((segs, tab, [int(v) for v in w[1:]]))
    return out


@pytest.mark.parametrize("which", ["plain", "san"])
@pytest.mark.parametrize("cases", [hand_cases, random_cases, hostile_cases], ids=["hand", "random", "hostile"])
def test_host_matches_reference(progs, which, cases):
    cs = cases()
    if cases is random_cases:
        assert len(cs) == 200
    out = subprocess.run([progs[which]], input=script(cs), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    got, ref = parse(out.stdout), reference(cs)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (k, cs[k][1], g, r)


def test_random_cases_cover_the_rules():
    ref = reference(random_cases())
    n_segs = [len(r[0]) for r in ref]
    assert sum(n == 0 for n in n_segs) > 10 and sum(n == 1 for n in n_segs) > 10 and sum(n >= 3 for n in n_segs) > 30
    assert sum(any(b[0] == a[1] for a, b in zip(r[0], r[0][1:])) for r in ref) > 10   # the half-gap padding branch
    assert sum(any(b[2] - a[3] == vr.GAP and b[0] == a[1] for a, b in zip(r[1], r[1][1:])) for r in ref) > 10  # a clamped overlap


def loader_files(tmp):
    """(path, accepted) of every file the loader test reads"""
    t = mk.make_tensors("rand", 1)
    good, ends = mk.model_bytes(t)
    f16, _ = mk.model_bytes(t, mk.f16_default_names())
    files = [("good", good, True), ("f16", f16, True)]
    cuts = {0, 3, 4, 7, 12, ends[0] - 4}
    for e in ends[:-1]:
        cuts |= {e, e + 4, e + 11, e + 40}          # at a record boundary, inside the next record's header, name and data
    cuts |= {len(good) - 1, len(good) - 4}
    files += [(f"cut{c}", good[:c], False) for c in sorted(cuts)]
    files.append(("magic", struct.pack("<I", 0x67676A74) + good[4:], False))
    files.append(("type", mk.header_bytes(model_type=b"silero-8k") + good[ends[0]:], False))
    files.append(("geometry", mk.header_bytes(layers=[(129, 128, 3), (128, 64, 3), (64, 64, 3), (64, 64, 3)]) + good[ends[0]:], False))
    files.append(("layers", mk.header_bytes(layers=mk.LAYERS[:3]) + good[ends[0]:], False))
    files.append(("hidden", mk.header_bytes(tail=(128, 64, 128, 1)) + good[ends[0]:], False))
    files.append(("unknown", good + mk.tensor_record("_model.decoder.rnn.bias_xx", np.zeros(512, dtype=np.float32)), False))
    first = good[ends[0]:ends[1]]
    files.append(("duplicate", good + first, False))
    files.append(("shape", good[:ends[0]] + mk.tensor_record("_model.stft.forward_basis_buffer", np.zeros((256, 1, 258), dtype=np.float32)) + good[ends[1]:], False))
    bad_type = bytearray(good)
    bad_type[ends[0] + 8:ends[0] + 12] = struct.pack("<i", 2)
    files.append(("ftype", bytes(bad_type), False))
    huge = bytearray(good)
    huge[ends[0] + 4:ends[0] + 8] = struct.pack("<i", 0x7FFFFFF0)   # a name length far past the file
    files.append(("namelen", bytes(huge), False))
    out = []
    for name, b, ok in files:
        path = str(tmp / f"{name}.bin")
        with open(path, "wb") as f:
            f.write(b)
        out.append((path, ok))
    return out


@pytest.mark.parametrize("which", ["plain", "san"])
def test_loader_refusals_end_clean(progs, which, tmp_path):
    files = loader_files(tmp_path)
    assert sum(not ok for _, ok in files) > 60
    out = subprocess.run([progs[which]], input="".join(f"load {p}\n" for p, _ in files), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(files)
    n_elems = sum(int(np.prod(s)) for _, s in mk.tensor_specs())
    for (path, ok), ln in zip(files, lines):
        assert ln == f"ok {n_elems}" if ok else ln.startswith("refused: "), (path, ln)
