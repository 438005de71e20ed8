"""CPU: the session part of the C-ABI boundary (include/drb_engine.h): the
configuration's checks answer before a device is touched, and the new
records' layout matches the ctypes mirror (tests/test_abi.py's gcc method).
"""
import ctypes as C
import os
import re
import subprocess

import pytest

from dragonboat_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drb_engine.h")


@pytest.mark.parametrize("kw", [
    dict(session_slots=17, session_history=1),   # S above 16
    dict(session_slots=4, session_history=0),    # S > 0 needs H >= 1
    dict(session_slots=4, session_history=9),    # H above 8
    dict(session_slots=0, session_history=1),    # H without S
    dict(session_slots=2 ** 32 - 1, session_history=8),
])
def test_create_rejects_invalid_session_config(kw):
    with pytest.raises(engine.DrbError) as ei:
        engine.Engine(num_groups=64, num_replicas=3, **kw)
    assert "status %d" % abi.DRB_EINVAL in str(ei.value)


def test_valid_session_config_reaches_the_device():
    """S = 16, H = 8 passes the validation: whatever answers next is the
    device (tests/test_gpu_sessions.py has the engine's byte count)."""
    try:
        engine.Engine(num_groups=64, num_replicas=3, window=32,
                      session_slots=16, session_history=8).close()
    except engine.DrbError as e:
        assert "status %d" % abi.DRB_EINVAL not in str(e)


STRUCTS = {"drb_session_rec": abi.SessionRec,
           "drb_session_resp": abi.SessionResp,
           "drb_config": abi.Config,
           "drb_apply_result": abi.ApplyResult}


def test_session_struct_layout_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>',
             '#include "drb_engine.h"', 'int main(void) {']
    for cname, cls in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));'
                         % (cname, f, cname, f))
    lines.append('printf("bits %u %u\\n", DRB_APPLY_IGNORED, '
                 'DRB_APPLY_REJECTED);')
    lines.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    got = dict(ln.split(None, 1) for ln in out)
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, \
                (cname, f)
    assert got["bits"] == "%d %d" % (abi.APPLY_IGNORED, abi.APPLY_REJECTED)
    # the configuration's last two fields, in the header's order
    assert [f for f, _ in abi.Config._fields_][-2:] == \
        ["session_slots", "session_history"]
    assert C.sizeof(abi.SessionRec) == 24 and C.sizeof(abi.SessionResp) == 16


def test_header_declares_the_session_calls():
    src = open(HEADER).read()
    for name in ("drb_sessions_export", "drb_sessions_import"):
        assert re.search(r"^int %s\(" % name, src, flags=re.M), name
        assert name in engine.SIGNATURES
