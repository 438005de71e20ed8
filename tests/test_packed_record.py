"""CPU: the packed 64 B replica record's codec under ASan and UBSan.

drb_layout.hpp keeps a replica's state in one 64 B record: index fields as
signed 16-bit offsets from `last`, terms as 16-bit distances from `term`,
16-bit ticks and 8-bit ids, each with an escape code that sends the value
to the u64 overflow array.  tests/native/pk_roundtrip.cpp walks the cross
product of every field's range boundary (offsets -40000 .. 32768 around
last = 4 .. 2^63+7, the ring guard's +inf against offsets 32766 / 32767,
term distances 0 .. 65536 and a value above term at term = 2 .. 2^64-2,
ticks and ids around their escape codes), checks each stored code against
a literal expectation (escape or not), that an in-range field neither
writes nor reads its junk-filled overflow slot, and that pk_decode returns
what pk_encode was given.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def roundtrip(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("pk") / "pk_roundtrip")
    subprocess.check_call([
        gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
        "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC,
        "-o", out, os.path.join(HERE, "native", "pk_roundtrip.cpp")])
    return out


def test_packed_record_boundaries_roundtrip(roundtrip):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([roundtrip], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-3000:])
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    w = r.stdout.split()
    assert w[0] == "ok" and int(w[1]) > 300000, r.stdout[-500:]
