"""CPU: the owners of the engine's device resources (drb_res.hpp) under
AddressSanitizer and UBSan, with leak detection.

Buf and Handle take their allocator and destroy call as template parameters;
tests/native/res_owner.cpp runs them on a counting fake (malloc underneath, a
live count, a "fail the N-th allocation" switch): grow-only reserve, the
{nullptr, 0} state after any failure, moves, exactly-once destruction, and a
struct of several of them abandoned at every step of its construction -- the
failure paths of the engine's lazily built states, which no GPU test
provokes.  A stand-alone program: nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("res_owner") / "res_owner")
    subprocess.check_call([
        gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
        "-Wno-self-move", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
        "-o", out, os.path.join(HERE, "native", "res_owner.cpp")])
    return out


def test_owning_types(prog):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([prog], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-3000:])
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "ERROR: " not in r.stderr, r.stderr[-3000:]
    word, checks = r.stdout.split()
    assert word == "ok" and int(checks) > 300
