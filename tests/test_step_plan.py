"""CPU: the step round's kinds table, its plan and the build's unit list.

drb_kinds.hpp holds the one table of step-kernel kinds and plan_step, the
choice of the kinds a round launches.  tests/native/step_plan.cpp pins each
row's flags with static_asserts and checks the plan of named engine
configurations -- the EXT triggers, forwarded proposals and member kinds,
placement, elections, the split and lean conditions -- and the stand-in of
every kind at every R against hand-written expectations, under ASan and
UBSan.  The program is stand-alone and host-compiled; it is never loaded
into Python.  build.py reads the same table: its unit list is checked here
against the list of objects written out.
"""
import os
import re
import shutil
import subprocess

import pytest

from dragonboat_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def step_plan(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not available"
    out = str(tmp_path_factory.mktemp("plan") / "step_plan")
    subprocess.check_call([
        gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
        "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC,
        "-o", out, os.path.join(HERE, "native", "step_plan.cpp")])
    return out


def test_step_plan_and_stand_ins(step_plan):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([step_plan], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-3000:])
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    w = r.stdout.split()
    assert w[0] == "ok" and int(w[1]) == 267, r.stdout[-500:]


def _includes(path, seen):
    """The project files `path` includes, transitively."""
    with open(path) as f:
        for inc in re.findall(r'^\s*#include "([^"]+)"', f.read(), re.M):
            p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            if p not in seen:
                seen.add(p)
                _includes(p, seen)
    return seen


def test_build_units_follow_the_kinds_table():
    units = build._units(())
    names = [u[0] for u in units]
    want = ["drb_engine.o", "recover.o", "tan_write.o", "tan_select.o"] + \
        ["step_r%d_k%d.o" % (r, k) for r in range(1, 9) for k in range(9)] + \
        ["step_r%d_k%d.o" % (r, k) for r in (3, 5) for k in (9, 10, 11, 12)]
    assert len(names) == 84 and len(set(names)) == 84
    assert sorted(names) == sorted(want)
    for name, src, defs, deps in units:
        have = {os.path.normpath(d) for d in deps}
        path = os.path.join(build.CSRC, src)
        missing = _includes(path, {path}) - have
        assert not missing, (name, sorted(missing))
        if name.startswith("step_"):
            r, k = re.fullmatch(r"step_r(\d)_k(\d+)\.o", name).groups()
            assert src == "drb_step_inst.hip"
            assert defs == ["DRB_INST_R=" + r, "DRB_INST_KIND=" + k]
