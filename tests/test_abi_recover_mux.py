"""The structs of drb_recover_tan_mux (include/drb_engine.h) against their
ctypes mirrors, as tests/test_abi_recover.py checks drb_recover_tan's; and
the binding's signature."""
import ctypes as C
import os
import subprocess

from dragonboat_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "drb_tan_mux_file": abi.TanMuxFile,
    "drb_recover_mux_in": abi.RecoverMuxIn,
    "drb_recover_log_status": abi.RecoverLogStatus,
}


def test_mux_struct_layout_matches_header(tmp_path):
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


def test_mux_binding_is_declared():
    res, args = engine.SIGNATURES["drb_recover_tan_mux"]
    assert res is C.c_int and len(args) == 4
    src = open(os.path.join(ROOT, "include", "drb_engine.h")).read()
    assert "int drb_recover_tan_mux(drb_engine *e" in src
    assert hasattr(engine.Engine, "recover_tan_mux")
