"""The restart structs of include/drb_engine.h against their ctypes mirrors
(dragonboat_amd/abi.py), as tests/test_abi.py checks the others; and the
status / outcome / fallback constants."""
import ctypes as C
import os
import re
import subprocess

from dragonboat_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drb_engine.h")

STRUCTS = {
    "drb_tan_scan_rec": abi.TanScanRec,
    "drb_tan_file": abi.TanFile,
    "drb_recover_in": abi.RecoverIn,
    "drb_recover_status": abi.RecoverStatus,
}


def test_restart_struct_layout_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>',
             '#include "drb_engine.h"', 'int main(void) {']
    for cname, cls in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));'
                         % (cname, f, cname, f))
    lines.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(ln.split() for ln in
               subprocess.run([str(exe)], capture_output=True, text=True,
                              check=True).stdout.splitlines())
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, \
                (cname, f)


def test_restart_constants_match_header():
    src = open(HEADER).read()
    rec = dict(re.findall(r"DRB_REC_(\w+) = (\d+)", src))
    assert {k: int(v) for k, v in rec.items()} == \
        {n: i for i, n in enumerate(abi.REC_NAME)}
    tan = dict(re.findall(r"DRB_TAN_(\w+) = (\d+)", src))
    assert {k: int(v) for k, v in tan.items()} == \
        {n: i for i, n in enumerate(abi.TAN_OUTCOME_NAME)}
    assert re.search(r"DRB_FB_RECOVERY = %d\b" % abi.FB["RECOVERY"], src)
