"""The engine's deny-mask host code (nobs-whisper_amd/csrc/suppress.cpp, free of HIP) against tests/suppress_ref.py, on
the CPU: tools/suppress_check.cpp is built with plain g++ and fed three vocabularies (tools/make_model.py's synthetic
one with special-token names behind it, n_vocab = 51866: no multiple of 32; a hand vocabulary with every string of the
non-speech list, with and without the leading space, " -" and " '"; one with none of them) and the patterns of the
issue, each with and without suppress_nst. Its words must be the reference's, the bits at and above n_vocab 0, and the
pattern that does not compile must report -8. A second build with -fsanitize=address,undefined runs the same scripts
(a program with its own main)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import suppress_ref as sr
from conftest import ROOT
from make_model import synthetic_vocab, token_beg

PATTERNS = ["[0-9]+", " ?[A-Z][a-z]*", r"\[_TT_.*\]", "", "(?!)", ".*"]
BAD = "("


def build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp / name)
    csrc = os.path.join(ROOT, "nobs-whisper_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I", csrc, os.path.join(ROOT, "tools", "suppress_check.cpp"),
                    os.path.join(csrc, "suppress.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("suppress")
    return {"plain": build(tmp, "suppress_check", []),
            "san": build(tmp, "suppress_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def synthetic(V=51866):
    toks = synthetic_vocab()
    beg = token_beg(V)
    toks += [f"[_TT_{i - beg}]".encode() if i > beg else f"[_S_{i}]".encode() for i in range(len(toks), V)]
    return V, toks


def hand():
    toks = [b"a", b" b", b"7", b"42", b"Word", b" Word", b"WORD", b"'", b"-", b" -", b" '", b"", b"\n", b"x\ry", b"\xff\xfe"]
    for s in sr.NON_SPEECH:
        toks += [s.encode(), b" " + s.encode()]
    toks += [b"[_TT_12]", b"[_TT_]", b"[_BEG_]"]
    return len(toks) + 5, toks  # (n_vocab beyond the strings: ids no string carries)


def plain():
    toks = [b"a", b" b", b"ab", b"-", b"'", b" a-b", b"seven", b" Eight", b"\xe2\x99", b"9", b"[_TT_3]", b"[_TT_3]", b"zz"]
    return 11, toks  # (n_vocab below the strings: the ids at and above it are never set; a repeated string)


VOCABS = {"synthetic": synthetic, "hand": hand, "plain": plain}
QUERIES = [(nst, p) for nst in (0, 1) for p in [None] + PATTERNS + [BAD]]


def script(V, toks):
    lines = [f"{V} {len(toks)}"] + [t.hex() or "-" for t in toks]
    for nst, p in QUERIES:
        lines.append(f"q {nst} " + ("null" if p is None else (p.encode().hex() or "-")))
    return "\n".join(lines) + "\n"


def reference(V, toks, nst, p):
    m = sr.mask(toks, bool(nst), p)
    m = np.concatenate([m, np.zeros(max(0, V - len(m)), bool)])[:V]
    return sr.words(m)


@pytest.mark.parametrize("which", ["plain", "san"])
@pytest.mark.parametrize("vocab", list(VOCABS))
def test_host_matches_reference(progs, which, vocab):
    V, toks = VOCABS[vocab]()
    out = subprocess.run([progs[which]], input=script(V, toks), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    lines = out.stdout.splitlines()
    k = 0
    for nst, p in QUERIES:
        rc = int(lines[k].split()[1])
        k += 1
        if p == BAD:
            assert rc == -8, (vocab, nst)
            continue
        assert rc == 0, (vocab, nst, p)
        w = lines[k].split()
        k += 1
        assert w[0] == "words"
        got = np.array([int(x, 16) for x in w[1:]], np.uint32)
        ref = reference(V, toks, nst, p)
        assert got.shape == ref.shape == ((V + 31) // 32,), (vocab, nst, p)
        assert (got == ref).all(), (vocab, nst, p, np.nonzero(got != ref)[0][:8])
        if V % 32:
            assert int(got[-1]) >> (V % 32) == 0, "bits at and above n_vocab"
    assert k == len(lines)


def test_the_cases_bite():
    """The vocabularies are worth their names: the hand one has all 110 list entries, the plain one none; `.*` bans
    everything but the strings with a line terminator, (?!) nothing, the empty pattern the empty string alone."""
    V, toks = hand()
    m = sr.mask(toks, True, None)
    assert int(m.sum()) == 2 * 54 + 2
    assert not m[[toks.index(b"'"), toks.index(b"-"), toks.index(b"a")]].any()
    assert not sr.mask(plain()[1], True, None).any()
    assert not sr.mask(toks, False, "(?!)").any()
    assert np.nonzero(sr.mask(toks, False, ""))[0].tolist() == [toks.index(b"")]
    every = sr.mask(toks, False, ".*")
    assert np.nonzero(~every)[0].tolist() == [toks.index(b"\n"), toks.index(b"x\ry")]
    Vs, ts = synthetic()
    m = sr.mask(ts, True, None)
    assert int(m.sum()) == 24 and m[ts.index(b" -")]  # its 23 single-byte list tokens and " -"
    assert int(sr.mask(ts, False, r"\[_TT_.*\]").sum()) == Vs - 1 - token_beg(Vs)
    assert int(sr.mask(ts, False, "[0-9]+").sum()) == 10
