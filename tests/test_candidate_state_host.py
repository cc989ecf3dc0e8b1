"""CPU test of the candidate cache's decision state (mincostflow_amd/csrc/candidate_state.h): tools/candidate_state_check.cpp is built with g++
-- under the address and undefined-behaviour sanitizers when the compiler has them -- and run as a child process.  It replays the cache's rules
against a brute-force scan on random graphs: every decision is the scan's argmin, every refusal is one where list and heap cannot tell, and
the heap never holds an entry that violates its invariant.  No device involved."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "candidate_state_check.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# the runtimes linked into the program where the compiler ships them as archives (then nothing depends on the order libraries are loaded in)
FLAG_SETS = [SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []]


def _compiles(cxx, flags, tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    exe = tmp_path / "probe"
    r = subprocess.run([cxx, *flags, str(probe), "-o", str(exe)], capture_output=True)
    return r.returncode == 0 and subprocess.run([str(exe)], capture_output=True).returncode == 0


def test_candidate_state_checker(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler to build the checker with"
    flags = next(f for f in FLAG_SETS if _compiles(cxx, f, tmp_path))          # a set counts when a program built with it also starts
    exe = tmp_path / "candidate_state_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SOURCE, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "candidate_state_check: ok" in r.stdout
