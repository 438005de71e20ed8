"""CPU: the Snappy block decoder (dragonboat_amd/csrc/drb_snappy.hpp) against
the oracle's GetPayload (oracle/node_oracle.c, golang/snappy v0.0.4 Decode
and getDecodedPayload restated).

The header is compiled as plain C++ into a stand-alone program
(tests/snappy_host_main.cc) with -fsanitize=address,undefined; it decodes
every vector through the flat accessors and through the strided 16 B-chunk
rows the device uses, with buffers of exactly the bytes the decoder may
touch.  A sanitizer report makes the program exit non-zero, which fails the
test.
"""
import os
import random
import shutil
import subprocess

import pytest

from dragonboat_amd import abi
from oracle import pyoracle as po
from tests import snappy_blocks as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "snappy_host_main.cc")
CAP = sb.CAP
# the oracle allocates what a block declares: beyond this the expectation is
# the capacity rule's alone (a declared length above the capacity is ERR)
ORACLE_MAX = 1 << 24


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("snappy") / "snappy_host_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", out, SRC]
    # the runtimes linked into the program where the compiler can (gcc links
    # them dynamically by default, and the dynamic one insists on being the
    # first library of the process)
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.call(cmd + static, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    return out


def _run(prog, tmp_path, cmds, cap=CAP):
    """Decodes each Cmd with the program: [payload bytes or None (ERR)]."""
    path = str(tmp_path / "vectors.txt")
    with open(path, "w") as f:
        for c in cmds:
            f.write("%d %s\n" % (cap, c.hex() or "-"))
    r = subprocess.run([prog, path], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split()
    assert len(lines) == len(cmds)
    assert "MISMATCH" not in lines, lines.index("MISMATCH")
    return [None if x == "ERR" else bytes.fromhex("" if x == "-" else x)
            for x in lines]


def _oracle(cmd, cap=CAP):
    """The oracle's payload, or None where the reference rejects the Cmd or
    the payload is longer than the capacity."""
    d = sb.declared(cmd[1:])
    if d is None or d > ORACLE_MAX:
        return None
    try:
        p = po.get_payload(abi.ENTRY_ENCODED, cmd)
    except po.OracleError:
        return None
    return p if len(p) <= cap else None


def test_valid_vectors_equal_the_oracle(prog, tmp_path):
    vec = sb.valid_vectors()
    names = {n for n, _, _ in vec}
    assert {"literal", "copy1", "copy2", "copy4_small_offset", "run_offset1",
            "literal_60", "literal_61", "literal_257", "literal_len3",
            "literal_len4", "exact_capacity"} <= names
    cmds = [sb.checked(b, p) for _, b, p in vec]
    # decoded from a block shorter than 64 B into more than 1000 B
    small = [(n, b, p) for n, b, p in vec if len(b) < 64 and len(p) > 1000]
    assert len(small) >= 2, [(n, len(b), len(p)) for n, b, p in vec]
    assert any(len(p) == CAP for _, _, p in vec)
    got = _run(prog, tmp_path, cmds)
    for (name, _, p), g in zip(vec, got):
        assert g == p, name


def test_malformed_vectors_are_rejected(prog, tmp_path):
    vec = sb.malformed_vectors()
    for name, b in vec:
        if sb.declared(b) is not None and sb.declared(b) <= ORACLE_MAX:
            with pytest.raises(po.OracleError):
                po.get_payload(abi.ENTRY_ENCODED, sb.cmd(b))
    got = _run(prog, tmp_path, [sb.cmd(b) for _, b in vec])
    for (name, _), g in zip(vec, got):
        assert g is None, (name, g)


def test_capacity_is_a_bound_on_the_declared_length(prog, tmp_path):
    """A sound block of CAP bytes decodes into CAP bytes and is rejected
    with one byte less (rows: one chunk less)."""
    name, b, p = [v for v in sb.valid_vectors() if v[0] == "exact_capacity"][0]
    c = sb.checked(b, p)
    assert _run(prog, tmp_path, [c], cap=CAP) == [p]
    assert _run(prog, tmp_path, [c], cap=CAP - 1) == [None]
    assert _run(prog, tmp_path, [c], cap=CAP - 16) == [None]


def _corpus(n=2000, seed=0xC0DEC):
    """Single-byte mutations and truncations of the valid blocks."""
    rnd = random.Random(seed)
    base = [sb.cmd(b) for _, b, _ in sb.valid_vectors()]
    out = []
    while len(out) < n:
        c = bytearray(rnd.choice(base))
        kind = rnd.randrange(4)
        if kind == 0:  # truncation
            c = c[:rnd.randrange(1, len(c))]
        else:
            # element tags and lengths sit at the front: favour it
            i = rnd.randrange(1, min(len(c), 24)) if kind == 1 else \
                rnd.randrange(1, len(c))
            c[i] = rnd.randrange(256) if kind < 3 else c[i] ^ (1 << rnd.randrange(8))
        out.append(bytes(c))
    return out


def test_mutation_corpus_agrees_with_the_oracle(prog, tmp_path):
    cmds = _corpus()
    want = [_oracle(c) for c in cmds]
    got = _run(prog, tmp_path, cmds)
    bad = [(i, cmds[i].hex()[:80]) for i in range(len(cmds))
           if got[i] != want[i]]
    assert not bad, bad[:3]
    ok = sum(w is not None for w in want)
    # the corpus exercises both outcomes
    assert ok > 100 and len(cmds) - ok > 300, ok


def test_uncompressed_and_unknown_headers(prog, tmp_path):
    """GetPayload's other branches through the same entry point: header
    0x00 is the bytes after it; unknown versions, compression types and the
    session bit are rejected; so is an empty Cmd."""
    cmds = [b"\x00abc", b"\x00", b"", b"\x10abc", b"\x04abc", b"\x01abc",
            b"\x03" + sb.block(3, sb.literal(b"abc"))]
    got = _run(prog, tmp_path, cmds)
    assert got == [b"abc", b"", None, None, None, None, None]


def test_drb_payload_decode_equals_the_oracle():
    """The library's host entry point (no engine, no device) on the same
    vectors."""
    from dragonboat_amd import engine
    try:
        engine.lib()
    except (OSError, RuntimeError) as e:
        pytest.skip("libdrb_engine.so does not load on this machine: %s" % e)
    for name, b, p in sb.valid_vectors():
        assert engine.payload_decode(abi.ENTRY_ENCODED, sb.checked(b, p),
                                     CAP) == p, name
    for name, b in sb.malformed_vectors():
        with pytest.raises(engine.DrbError):
            engine.payload_decode(abi.ENTRY_ENCODED, sb.cmd(b), CAP)
    for c in _corpus(400, seed=7):
        want = _oracle(c)
        try:
            got = engine.payload_decode(abi.ENTRY_ENCODED, c, CAP)
        except engine.DrbError:
            got = None
        assert got == want, c.hex()[:80]
    assert engine.payload_decode(abi.ENTRY_APPLICATION, b"xyz", 8) == b"xyz"
    assert engine.payload_decode(abi.ENTRY_ENCODED, b"\x00xyz", 8) == b"xyz"
    with pytest.raises(engine.DrbError):
        engine.payload_decode(abi.ENTRY_ENCODED, b"\x00" + b"x" * 9, 8)
