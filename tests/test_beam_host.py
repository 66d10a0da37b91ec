"""The engine's beam-search bookkeeping (nobs-whisper_amd/csrc/beam_host.cpp, free of HIP) against tests/beam_ref.py,
on the CPU: tools/beam_host_check.cpp is built with plain g++ and fed the hand-made tables of test_beam_ref.py as
scripted candidate lists; its picks, self-cache copy lists and final beams must be the reference's."""
import os
import shutil
import subprocess

import pytest

import beam_ref as br
import test_beam_ref as tb
from conftest import ROOT

N_PROMPT = 3


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("beam_host") / "beam_host_check")
    csrc = os.path.join(ROOT, "nobs-whisper_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", csrc, os.path.join(ROOT, "tools", "beam_host_check.cpp"),
                    os.path.join(csrc, "beam_host.cpp"), "-o", out], check=True)
    return out


def common_prefix_case():
    t = {(): {tb.A: 0.0, tb.B: -3.0}, (tb.A,): {tb.C_: 0.0, tb.D: -0.1}, (tb.B,): {tb.C_: 0.0},
         (tb.A, tb.C_): {tb.E: 0.0, tb.F: -0.05}, (tb.A, tb.D): {tb.E: 0.0, tb.F: 0.0, tb.X: 0.0, tb.Y: 0.0},
         (tb.A, tb.C_, tb.E): {tb.EOT: 0.0}, (tb.A, tb.C_, tb.F): {tb.EOT: 0.0}}
    return t, None, br.Params(K=2, no_timestamps=True), None, 0


CASES = dict(tb.CASES, common_prefix=common_prefix_case)


def run_case(prog, name, monkeypatch):
    table, default, P, _, _ = CASES[name]()
    rec, last = {}, {}
    base = tb.table_fn(table, default)
    orig = br.candidates

    def fn(prefix):
        last["p"] = prefix
        return base(prefix)

    def cand(lp, K, v):
        c = orig(lp, K, v)
        rec[last["p"]] = c
        return c

    monkeypatch.setattr(br, "candidates", cand)
    ref = br.beam_search(fn, P, tb.VID, n_prompt=N_PROMPT)
    lines = [f"{P.K} {N_PROMPT} {int(P.no_timestamps)} {int(P.single_segment)} {P.max_tokens} {P.n_max} {P.seek_end} "
             f"{P.length_penalty} {P.entropy_thold} {tb.VID['eot']} {tb.VID['beg']}", str(len(rec))]
    for prefix, cs in rec.items():
        lines.append(" ".join(map(str, [len(prefix), *prefix, len(cs)] + [x for c in cs for x in (c["id"], repr(c["plog"]))])))
    out = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    picks, copies, beams, winner = [], [], {}, None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "step":
            v = list(map(int, w[3:]))
            picks.append([tuple(v[i:i + 3]) for i in range(0, len(v), 3)])
            copies.append([])
        elif w[0] == "copy":
            copies[-1].append(tuple(map(int, w[1:6])))
        elif w[0] == "beam":
            beams[int(w[1])] = dict(flags=int(w[3]), sum=float(w[5]), tokens=list(map(int, w[7:])))
        elif w[0] == "winner":
            winner = int(w[1])
    return ref, picks, copies, beams, winner


@pytest.mark.parametrize("name", list(CASES))
def test_host_matches_reference(prog, name, monkeypatch):
    ref, picks, copies, beams, winner = run_case(prog, name, monkeypatch)
    assert picks == ref.picks
    assert [sorted(c[:4] for c in step) for step in copies] == [sorted(step) for step in ref.copies]
    assert winner == ref.winner
    for i, b in enumerate(ref.beams):
        assert beams[i]["tokens"] == b["tokens"]
        assert beams[i]["flags"] == (1 if b["completed"] else 0) | (2 if b["failed"] else 0)
        assert beams[i]["sum"] == pytest.approx(b["sum_logprobs_all"], abs=1e-5)


def test_copy_lists(prog, monkeypatch):
    """A swap goes through the staging buffer, a fan-out from a slot nobody overwrites goes straight, and row0 is the
    length of the common prefix (prompt included)."""
    _, _, copies, _, _ = run_case(prog, "overtaken", monkeypatch)
    assert copies[0] == [(1, 0, 0, N_PROMPT, 0)]                       # step 0: the prompt's rows fan out
    assert sorted(copies[1]) == [(0, 1, 3, 4, 1), (1, 0, 3, 4, 1)]     # the swap, both staged
    _, _, copies, _, _ = run_case(prog, "eot_shrinks", monkeypatch)
    assert sorted(copies[0]) == [(1, 0, 0, 3, 0), (2, 0, 0, 3, 0)]     # fan-out to two beams, straight
    assert copies[2] == [(2, 1, 3, 5, 0)]
    _, _, copies, _, _ = run_case(prog, "common_prefix", monkeypatch)
    assert copies[2] == [(1, 0, 4, 5, 0)]                              # the prompt and the shared first token stay
