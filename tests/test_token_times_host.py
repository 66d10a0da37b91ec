"""The engine's token-time host code (nobs-whisper_amd/csrc/token_times.cpp, free of HIP: phase 1, the wrap and
voice_length) against tests/tokts_ref.py, on the CPU: tools/token_times_check.cpp is built with plain g++ and fed the
hand cases of test_tokts_ref.py and 200 seeded random segments (five per clip, the clip state carried over); its
output must be the reference's. A second build with -fsanitize=address,undefined runs the same scripts (a program
with its own main)."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import tokts_ref as tr
import test_tokts_ref as tt
from conftest import ROOT

N_VOCAB = tt.BEG + 1501
CONFIGS = [(0, False), (1, False), (8, False), (8, True), (20, True)]


def build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp / name)
    csrc = os.path.join(ROOT, "nobs-whisper_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I", csrc, os.path.join(ROOT, "tools", "token_times_check.cpp"),
                    os.path.join(csrc, "token_times.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("token_times")
    return {"plain": build(tmp, "token_times_check", []),
            "san": build(tmp, "token_times_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def hand_clips():
    """Clips = lists of (t0, t1, tokens): the cases of test_tokts_ref.py."""
    T, TS, BEG = tt.T, tt.TS, tt.BEG
    return [
        [(0, 300, tt.WORKED), (300, 500, [T(0), T(1), TS(250)])],
        [(10, 20, []), (10, 20, [T(0, BEG + 5, 0.9, 0.9)])],
        [(0, 300, [TS(0), T(5, BEG, 0.9, 0.9), T(0, BEG + 50, 0.9, 0.9), T(1, BEG + 50, 0.9, 0.9), TS(150)])],
        [(0, 300, [TS(0), T(5), T(0, BEG + 50, 0.9, 0.005), T(1), TS(150)])],
        [(0, 200, [TS(0), T(0, BEG + 150, 0.9, 0.9), T(1), TS(100)])],
        [(0, 300, [TS(0), T(0), T(4), T(1), TS(150)])],
        [(0, 40, [T(4), T(4), T(2), T(4)])],
    ]


def random_clips(seed=20240611, n_clips=40, per_clip=5):
    rng = random.Random(seed)
    text_ids = sorted(tt.TEXT)
    clips = []
    for _ in range(n_clips):
        segs, t = [], rng.choice([0, 0, 3000, 12000])
        for _ in range(per_clip):
            t1 = t + rng.randint(0, 600)
            n = rng.randint(1, 40)
            toks = []
            for i in range(n):
                r = rng.random()
                if i == 0 and r < 0.7:
                    k = rng.randint(0, 1500)
                    toks.append(dict(id=tt.BEG + k, tid=tt.BEG + k, pt=rng.random(), ptsum=rng.random()))
                    continue
                if r < 0.08:    # a special in the middle
                    i_d = rng.choice([tt.EOT, tt.EOT + 1, tt.EOT + 5, tt.BEG + rng.randint(0, 1500)])
                elif r < 0.12:  # any other plain id
                    i_d = rng.randint(9, tt.EOT - 1)
                else:
                    i_d = rng.choice(text_ids)
                tid = i_d if i_d >= tt.BEG else tt.BEG + rng.randint(-2, 1500)
                pt = float(np.float32(rng.choice([0.0, 0.01, 0.0100001, 0.005, rng.random(), rng.random() ** 4])))
                ps = float(np.float32(rng.choice([0.0, 0.01, 0.02, rng.random(), 1.0])))
                toks.append(dict(id=i_d, tid=tid, pt=pt, ptsum=ps))
            segs.append((t, t1, toks))
            t = t1 if rng.random() < 0.8 else t1 + rng.randint(0, 200)
        clips.append(segs)
    return clips


def script(clips, max_len, sow):
    lines = [f"{tt.BEG} {tt.EOT} 0.01 0.01 {max_len} {int(sow)} {N_VOCAB}"]
    lines += [tt.tok_str(i).hex() or "-" for i in range(N_VOCAB)]
    for segs in clips:
        lines.append("clip")
        for t0, t1, toks in segs:
            lines.append(f"seg {t0} {t1} {len(toks)}")
            lines += [f"{t['id']} {t['tid']} {t['pt']!r} {t['ptsum']!r}" for t in toks]
    return "\n".join(lines) + "\n"


def reference(clips, max_len, sow):
    out = []
    for segs in clips:
        st = tr.new_state()
        for t0, t1, toks in segs:
            tok = tr.phase1(toks, t0, t1, st, tt.BEG, 0.01, 0.01, tt.tok_str)
            rec = dict(tok=[(t["t0"], t["t1"], float(t["vlen"])) for t in tok], pieces=None)
            if max_len > 0:
                i, rec["pieces"] = 0, []
                for p in tr.wrap(tok, t0, t1, max_len, sow, tt.EOT, tt.tok_str):
                    rec["pieces"].append((i, i + len(p["tokens"]), p["t0"], p["t1"], p["text"]))
                    i += len(p["tokens"])
            out.append(rec)
    return out


def parse(stdout, max_len):
    out = []
    for ln in stdout.splitlines():
        w = ln.split()
        if w[0] == "seg":
            out.append(dict(tok=[], pieces=[] if max_len > 0 else None))
        elif w[0] == "tok":
            out[-1]["tok"].append((int(w[1]), int(w[2]), float.fromhex(w[3])))
        elif w[0] == "piece":
            out[-1]["pieces"].append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), b"" if w[5] == "-" else bytes.fromhex(w[5])))
    return out


@pytest.mark.parametrize("which", ["plain", "san"])
@pytest.mark.parametrize("clips", [hand_clips, random_clips], ids=["hand", "random"])
def test_host_matches_reference(progs, which, clips):
    cl = clips()
    if clips is random_clips:
        assert sum(len(s) for s in cl) == 200
    for max_len, sow in CONFIGS:
        out = subprocess.run([progs[which]], input=script(cl, max_len, sow), capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert out.stderr == "", out.stderr[-4000:]
        got, ref = parse(out.stdout, max_len), reference(cl, max_len, sow)
        assert len(got) == len(ref)
        for k, (g, r) in enumerate(zip(got, ref)):
            assert g == r, (max_len, sow, k)


def test_random_segments_cover_the_rules():
    """The random script is worth its name: timestamp hits, ignored tids, ignored late times, segments with and without
    a leading timestamp token, and pieces cut by the wrap all occur."""
    cl = random_clips()
    first_ts = sum(1 for segs in cl for _, _, toks in segs if toks[0]["id"] >= tt.BEG)
    assert 0 < first_ts < 200
    assert any(len(toks) == 1 for segs in cl for _, _, toks in segs)
    ref = reference(cl, 8, True)
    assert sum(len(r["pieces"]) > 1 for r in ref) > 50
    known = sum(1 for r in ref for a, b, _ in r["tok"] if a >= 0 and b >= 0)
    assert known > 1000
