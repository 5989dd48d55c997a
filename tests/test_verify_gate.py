"""The rendezvous of SNARK::verify_many (spartan_amd/host/batch_gate.hpp) on the CPU: tests/csrc/gate_check.cc — a stand-alone program that
includes nothing but that header — built once with the thread sanitizer and once with the address and undefined-behaviour sanitizers, and run
under a time limit. The program drives K in {1, 2, 7, 64} members through randomised step counts against a stub "device", members leaving by
return and by exception at every step position, mixed keys, the stub throwing on a chosen rendezvous; it checks that every request gets the
answer of its own payload, that the stub runs once per group and rendezvous, that every waiter sees a leader's failure, and it ends: a
deadlock shows as the timeout. Nothing is loaded into Python; the sanitizer runtimes are linked statically and the environment is left as it is."""
import os, subprocess
import pytest
from tests.helpers import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "gate_check.cc")
HDR = os.path.join(ROOT, "spartan_amd", "host", "batch_gate.hpp")
# the sanitizer runtimes are linked INTO the program: it needs nothing preloaded and does not care what its environment preloads
BUILDS = {"thread": "-fsanitize=thread -static-libtsan",
          "address_undefined": "-fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan"}


def test_the_check_program_includes_the_gate_header_and_nothing_else_of_the_project():
    inc = [l.split('"')[1] for l in open(SRC) if l.startswith('#include "')]
    assert inc == ["../../spartan_amd/host/batch_gate.hpp"]
    assert '#include "' not in open(HDR).read()      # the gate itself includes the standard library only: no device, no C ABI


@pytest.mark.parametrize("name", sorted(BUILDS))
def test_gate_under_sanitizer(tmp_path, name):
    exe = str(tmp_path / ("gate_check_" + name))
    subprocess.check_call("g++ -O1 -g -std=c++17 -pthread %s %s -o %s" % (BUILDS[name], SRC, exe), cwd=ROOT, shell=True)
    env = dict(os.environ)
    env.update(TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert "0 failures" in out and "scenarios" in out, out[-2000:]
