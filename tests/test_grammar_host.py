"""The engine's grammar host code (nobs-whisper_amd/csrc/grammar.cpp, free of HIP) against tests/grammar_ref.py, on the
CPU: tools/grammar_check.cpp is built with plain g++, once with -O2 and once with -fsanitize=address,undefined (programs
with their own main), and fed three vocabularies (the toy one; tools/make_model.py's synthetic one; its first 2 000
entries plus 20 multi-byte strings) and the grammars G1-G5 of tests/grammar_cases.py, each in the states after 0, 1, 3
and all tokens of a valid sentence and after one violating token. The masks must be the reference's bit for bit, the
state's stack count, allow_eot and pending partial too, and every invalid grammar must report -9."""
import os
import shutil
import subprocess

import pytest

import grammar_cases as gc
import grammar_ref as gr
from conftest import ROOT


def build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp / name)
    csrc = os.path.join(ROOT, "nobs-whisper_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-g", "-Wall", *extra, "-I", csrc, os.path.join(ROOT, "tools", "grammar_check.cpp"),
                    os.path.join(csrc, "grammar.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("grammar")
    return {"plain": build(tmp, "grammar_check", ["-O2"]),
            "san": build(tmp, "grammar_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def grammar_lines(rules, start):
    out = [f"g {len(rules)} {start}"]
    for r in rules:
        out.append("-1" if r is None else " ".join([str(len(r))] + [f"{t} {v}" for t, v in r]))
    return out


def header(toks, eot):
    return [f"{len(toks)} {eot} {len(toks)}"] + [t.hex() or "-" for t in toks]


def run(prog, lines):
    out = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]
    return out.stdout.splitlines()


@pytest.mark.parametrize("which", ["plain", "san"])
@pytest.mark.parametrize("vname", gc.VOCABS)
def test_host_matches_reference(progs, which, vname):
    toks, eot = gc.vocab(vname)
    lines, asked = header(toks, eot), []
    for gname, (rules, start) in gc.GRAMMARS.items():
        lines += grammar_lines(rules, start)
        for p in gc.prefixes(vname, gname):
            lines.append(" ".join(["s", str(len(p))] + [str(i) for i in p]))
            asked.append((gname, tuple(p)))
    got = run(progs[which], lines)
    k, last, n_set = 0, None, 0
    for gname, p in asked:
        if gname != last:
            assert got[k] == "rc 0", (gname, got[k])
            k, last = k + 1, gname
        words, st = gc.ref_words(vname, gname, p)
        f = got[k].split()
        assert f[0] == "state"
        assert (int(f[1]), int(f[2])) == (len(st.stacks), int(gr.allow_eot(st.stacks))), (vname, gname, p)
        assert (int(f[3]), int(f[4])) == st.partial, (vname, gname, p)
        w = got[k + 1].split()
        assert w[0] == "words" and tuple(int(x, 16) for x in w[1:]) == words, (vname, gname, p)
        n_set += sum(bin(x).count("1") for x in words)
        k += 2
    assert k == len(got) and n_set > 0


def test_the_cases_bite():
    """Every grammar's sentence is spelled by the synthetic vocabulary in more than three tokens (G1's in two); each
    grammar has a state that allows EOT, a state without stacks and a mask that neither rejects nor accepts everything; G5 on the
    single-byte tokens leaves a pending partial whose mask accepts a continuation byte alone."""
    toks, eot = gc.vocab("synthetic")
    for gname in gc.GRAMMARS:
        ps = gc.prefixes("synthetic", gname)
        assert len(ps) == (4 if gname == "G1" else 5) and (gname == "G1" or len(ps[3]) > 3), (gname, ps)
        states = [gc.ref_words("synthetic", gname, tuple(p))[1] for p in ps]
        assert gr.allow_eot(states[-2].stacks) and not states[-1].stacks
        init = states[0].reject(toks, eot)
        assert 0 < sum(init[:eot]) < eot - 1, gname
    rules, start = gc.GRAMMARS["G5"]
    st = gr.State(rules, start)
    st.accept_token(toks[0xC3])
    assert st.partial == (3, 1)
    m = st.reject(toks, eot)
    # (id 0 is a zero byte: no bytes are decoded, the pending partial stays and still matches)
    assert [i for i in range(eot) if toks[i] and not m[i]] == [0, 0xA9]
    # the multi vocabulary spells G5's sentence with multi-byte tokens
    mt, me = gc.vocab("multi")
    assert gc.tokenize(mt, me, gc.SENTENCES["G5"].encode()) == [mt.index("é♪à".encode()), mt.index("ÿ".encode()),
                                                                mt.index("é".encode())]


@pytest.mark.parametrize("which", ["plain", "san"])
def test_invalid_grammars(progs, which):
    toks, eot = gc.vocab("toy")
    lines = header(toks, eot)
    for rules, start in gc.INVALID.values():
        lines += grammar_lines(rules, start) + ["s 0"]
    got = run(progs[which], lines)
    assert len(got) == 3 * len(gc.INVALID)
    for k, name in enumerate(gc.INVALID):
        assert got[3 * k] == "rc -9", name
        # a refused grammar leaves no rules: the state has no stacks and the mask is empty
        assert got[3 * k + 1].split()[1:3] == ["0", "0"], name
        assert set(got[3 * k + 2].split()[1:]) == {"0"}, name


def test_accept_all_and_timing(progs):
    """The accept-everything grammar rejects only invalid UTF-8 (and allows EOT); `t` times the mask."""
    toks, eot = gc.vocab("synthetic")
    rules, start = gc.ACCEPT_ALL
    got = run(progs["plain"], header(toks, eot) + grammar_lines(rules, start) + ["s 0", "t 3"])
    assert got[0] == "rc 0" and got[3].startswith("time ")
    words = [int(x, 16) for x in got[2].split()[1:]]
    st = gr.State(rules, start)
    assert tuple(words) == tuple(gr.pack(st.reject(toks, eot)))
    bad = [i for i in range(len(toks)) if words[i >> 5] >> (i & 31) & 1]
    # continuation bytes as leads; 0xC0 / 0xC1 (overlong: value < 2); leads of code points above U+10FFFF
    assert bad == list(range(0x80, 0xC2)) + list(range(0xF5, 0x100))
    print("grammar_reject over", eot, "tokens:", got[3].split()[1], "ms")
