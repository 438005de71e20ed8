"""CPU: the session table (dragonboat_amd/csrc/drb_session.hpp) against the
plain-Python model of the reference's session code (tests/session_model.py).

The header is compiled as plain C++ into a stand-alone program
(tests/session_host_main.cc) with -fsanitize=address,undefined; it runs
seeded scripts through the flat accessor and through rows whose chunks are a
stride apart (the device layout), on buffers of exactly the table's bytes.
A sanitizer report makes the program exit non-zero, which fails the test.

The model is unbounded (4096 sessions, any history); the table holds S
sessions of H responses.  Where the model would outgrow the table -- a
register of an S+1-th client, an update that needs an H+1-th response after
its own clearTo -- the table must answer `full` and stay byte-identical (the
program compares), and the model skips the entry, so the comparison goes on
to the script's end, past its first `full`.
"""
import copy
import os
import random
import shutil
import subprocess

import pytest

from tests import session_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "session_host_main.cc")
OPS = 2000
CLIENTS = [11, 22, 33, 2 ** 63 + 5, 2 ** 64 - 1, 66]
SHAPES = [(S, H) for S in (1, 2, 4, 16) for H in (1, 2, 8)]
CLASSES = {"registered", "register-duplicate", "unregistered",
           "unregister-unknown", "unknown-client", "responded", "cached",
           "update", "full", "update-failed"}


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("session") / "session_host_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", out, SRC]
    # the runtimes linked into the program where the compiler can (gcc links
    # them dynamically by default, and the dynamic one insists on being the
    # first library of the process)
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.call(cmd + static, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    return out


def _run(prog, tmp_path, lines):
    path = str(tmp_path / "script.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([prog, path], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    out = r.stdout.decode().splitlines()
    bad = [ln for ln in out if ln.startswith("MISMATCH")]
    assert not bad, bad[:3]
    return out


def _cmd(n):
    """A PBKV of n bytes in all (n >= 5)."""
    return b"\x0a\x01k\x12" + bytes([n - 5]) + b"v" * (n - 5)


def would_fill(m, S, H, client, series, responded_to, cmd):
    """Whether the entry would take the model beyond S sessions or beyond H
    responses in its session."""
    s = m.lru.sessions.get(client)
    if not cmd and series == sm.SERIES_REGISTER:
        return s is None and len(m.lru.sessions) == S
    if (not cmd and series == sm.SERIES_UNREGISTER) or s is None:
        return False
    upto = max(s.responded_up_to, responded_to)
    if series <= upto:
        return False
    hist = [k for k in s.history if k > responded_to]
    return series not in hist and len(hist) == H


def script(seed, S, H):
    """[(client, series, responded_to, cmd, fail)]: series drawn near each
    client's current one, so that duplicates, responded series and gaps
    occur; responded_to mostly close behind."""
    rnd = random.Random(seed)
    cur = {c: 0 for c in CLIENTS}
    ops = []
    for _ in range(OPS):
        c = rnd.choice(CLIENTS[:max(2, min(len(CLIENTS), S + 2))])
        x = rnd.random()
        if x < 0.08:
            ops.append((c, sm.SERIES_REGISTER, 0, b"", 0))
            continue
        if x < 0.12:
            ops.append((c, sm.SERIES_UNREGISTER, 0, b"", 0))
            cur[c] = 0 if rnd.random() < 0.5 else cur[c]
            continue
        if x < 0.13:  # a register series with a Cmd is an update
            ops.append((c, sm.SERIES_REGISTER, 0, _cmd(7), 0))
            continue
        series = max(1, cur[c] + rnd.choice([-2, -1, 0, 0, 1, 1, 1, 2, 3]))
        cur[c] = max(cur[c], series)
        lag = rnd.choice([0, 1, 1, 1, 2, H, H + 1, 2 * H + 2])
        responded = max(0, series - 1 - lag) if rnd.random() < 0.9 else \
            series + rnd.randrange(0, 2)
        ops.append((c, series, responded, _cmd(5 + rnd.randrange(20)),
                    int(rnd.random() < 0.05)))
    return ops


def _fmt_sessions(sessions):
    return "X " + "".join(
        "%d:%d:%s;" % (c, u, ",".join("%d=%d" % kv for kv in sorted(h.items())))
        for c, u, h in sessions)


@pytest.mark.parametrize("rows", [0, 1], ids=["flat", "rows"])
def test_scripts_equal_the_model(prog, tmp_path, rows):
    lines, want, seen = [], [], {}
    for i, (S, H) in enumerate(SHAPES):
        m = sm.Model()
        lines.append("T %d %d %d" % (S, H, rows))
        for n, (c, series, resp, cmd, fail) in enumerate(
                script(0x5E55 + i, S, H)):
            value = len(cmd)
            lines.append("A %d %d %d %d %d %d" % (c, series, resp, len(cmd),
                                                  value, fail))
            if would_fill(m, S, H, c, series, resp, cmd):
                want.append("full 0")
                cls = "full"
            else:
                # an update whose state machine call fails leaves no trace
                snap = None
                if fail:
                    snap = copy.deepcopy(m)
                (v, rej, ign), cls = m.apply(c, series, resp,
                                             sm.ENTRY_APPLICATION, cmd)
                if fail and cls == "update":
                    m = snap
                    cls, v = "update-failed", 0
                want.append("%s %d" % (cls, v))
            seen.setdefault(cls, set()).add((S, H))
            if n % 10 == 9 or n == OPS - 1:
                lines.append("X")
                want.append(_fmt_sessions(m.sessions()))
    got = _run(prog, tmp_path, lines)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    # every outcome class occurs in the script set
    assert set(seen) == CLASSES, CLASSES - set(seen)
    assert len(seen["full"]) > 6 and len(seen["cached"]) == len(SHAPES)


def test_import_export(prog, tmp_path):
    """sess_import takes sess_export's order; what it refuses leaves the
    table unchanged (the program compares the bytes)."""
    for rows in (0, 1):
        lines = ["T 2 2 %d" % rows,
                 "I 2 7 3 2 5 50 4 40 9 0 0", "X",
                 # then entries: a duplicate served from the imported history,
                 # and a use of client 7 that makes it the most recent
                 "A 7 5 3 9 9 0", "X", "A 9 1 0 9 9 0", "X",
                 "I 3 1 0 0 2 0 0 3 0 0",          # more than S sessions
                 "I 1 1 0 3 1 1 2 2 3 3",          # more than H responses
                 "I 1 1 0 1 1 %d" % 2 ** 62,       # a value >= 2^62
                 "I 1 0 0 0",                      # a zero client_id
                 "I 2 4 0 0 4 0 0",                # a repeated client_id
                 "I 1 4 0 2 6 1 6 2",              # a repeated series
                 "I 1 4 5 1 5 1",                  # a series <= responded_up_to
                 "X", "I 0", "X"]
        got = _run(prog, tmp_path, lines)
        assert got == [
            "OK", "X 7:3:4=40,5=50;9:0:;",
            "cached 50", "X 9:0:;7:3:4=40,5=50;",
            "update 9", "X 7:3:4=40,5=50;9:0:1=9;",
            "ERANGE", "ERANGE", "ERANGE", "ERANGE", "ERANGE", "ERANGE",
            "ERANGE", "X 7:3:4=40,5=50;9:0:1=9;", "OK", "X "], got
