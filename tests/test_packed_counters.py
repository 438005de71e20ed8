"""CPU: tick_count / kv_count in the packed record under ASan and UBSan.

The two counters are their u64 field plus a 16-bit delta in word 15 of the
64 B record (drb_layout.hpp): the step kernels count in the record and fold
a delta into its field only when it would pass 0xffff.
tests/native/pk_counters.cpp checks, for deltas 0, 1, 0xfffe and 0xffff in
either half and field values 0, 1, 2^32 and 2^63, that pk_decode returns
field + delta with the other half and every other field untouched, that
pk_encode followed by pk_decode is the identity with word 15 = 0, and the
fold rule of pk_count_add.  The program is stand-alone and host-compiled;
it is never loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def counters(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("pkc") / "pk_counters")
    subprocess.check_call([
        gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
        "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC,
        "-o", out, os.path.join(HERE, "native", "pk_counters.cpp")])
    return out


def test_packed_record_counters(counters):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([counters], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-3000:])
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    w = r.stdout.split()
    # 256 decode cases, 256 round trips, 160 + 1 fold cases
    assert w[0] == "ok" and int(w[1]) == 673, r.stdout[-500:]
