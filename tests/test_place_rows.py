"""CPU: the placement rule and the row codec under ASan and UBSan.

drb_place.hpp is MessageQueue.Add of the GPU inbox -- how one delivered
message enters a (group, sender, receiver) mailbox plane -- behind both
drb_ingest_ex and drb_ingest_wire; drb_rows.hpp packs and unpacks the entry
and proposal rows.  tests/native/place_rows.cpp drives both with a host View
(MB=4, W=8, E=4, C16=2, max_props=2, fwd_props=1): header reset, record
positions, every capacity, elo and max-append, the term rule, the tag byte,
every record decoded again by msg_decode; rows round-tripped at Cmd lengths
0, 1, 15, 16, 17, 32 and the capacity marker at 33.  The program is
stand-alone and host-compiled; it is never loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def place_rows(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("place") / "place_rows")
    subprocess.check_call([
        gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
        "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC,
        "-o", out, os.path.join(HERE, "native", "place_rows.cpp")])
    return out


def test_placement_rule_and_row_codec(place_rows):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([place_rows], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-3000:])
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    w = r.stdout.split()
    assert w[0] == "ok" and int(w[1]) == 686, r.stdout[-500:]
