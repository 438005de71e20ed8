"""CPU: the per-message wire decoder under AddressSanitizer and UBSan.

drb_msgdec.hpp is the body k_ing_count / k_ing_decode run on every Requests
element of an ingested stream (Message.Unmarshal, raft_optimized.go:659-983,
and the colfer Entry, :308-656).  tests/native/msgdecode.cpp drives it as a
stand-alone program built here with -fsanitize=address,undefined, each
message in a heap allocation of exactly its size, over tests/wire_cases.py:

- the hand-written cases (canonical controls, encodings Go accepts and never
  emits, bytes Go refuses): hand expectation == oracle == decoder, on the
  outcome, every field, every entry and the Cmd bytes at cmd_off;
- 16000 seeded bit flips and byte deletions of two canonical messages:
  oracle == decoder;
- everywhere: no sanitizer report, and the count pass (ents == nullptr) and
  the decode pass agree on outcome and entry count.
"""
import os
import shutil
import struct
import subprocess

import pytest

from oracle import pyoracle as po
from tests import wire_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))
CMD_CAP = 32
OUTCOME = {0: "ok", 1: "bad", 2: "snapshot", 3: "big"}


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("msgdecode") / "msgdecode")
    subprocess.check_call([
        gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
        "-o", out, os.path.join(HERE, "native", "msgdecode.cpp")])
    return out


def run_decoder(decoder, msgs, tmp_path, cmd_cap=CMD_CAP):
    """[(count outcome, count n_ent, decode outcome, msg dict | None)]; the
    msg dict as po.msg(), its Cmds read from the message at cmd_off."""
    p = tmp_path / "msgs.bin"
    p.write_bytes(b"".join(struct.pack("<I", len(m)) + m for m in msgs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([decoder, str(p), str(cmd_cap)], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "msg":
            k, r1, n1, r2, n2 = map(int, w[1:6])
            assert k == len(out)
            t, to, frm, sh, term, lt, li, com, rej, hint, hh = \
                map(int, w[6:17])
            m = po.msg(t, from_=frm, to=to, term=term, log_term=lt,
                       log_index=li, commit=com, reject=bool(rej), hint=hint,
                       hint_high=hh, shard_id=sh)
            out.append([OUTCOME[r1], n1, OUTCOME[r2], n2, m])
        else:
            term, index, typ, key, cid, sid, rto, off, ln = map(int, w[1:])
            data = msgs[len(out) - 1]
            assert off + ln <= len(data)  # the Cmd lies inside the message
            out[-1][4]["entries"].append(po.ent(
                term=term, index=index, type=typ, key=key, client_id=cid,
                series_id=sid, responded_to=rto, cmd=data[off:off + ln]))
    assert len(out) == len(msgs)
    return out


def expected_msg(m):
    """A wire_cases message dict as po.msg() makes it."""
    return po.msg(m["type"], from_=m["from_"], to=m["to"], term=m["term"],
                  log_term=m["log_term"], log_index=m["log_index"],
                  commit=m["commit"], reject=bool(m["reject"]),
                  hint=m["hint"], hint_high=m["hint_high"],
                  entries=[po.ent(**e) for e in m["entries"]],
                  shard_id=m["shard_id"])


def check_passes(name, got):
    r1, n1, r2, n2, m = got
    assert (r1, n1) == (r2, n2), name
    if r2 in ("ok", "big"):
        assert len(m["entries"]) == n2, name


def oracle_outcome(data, cmd_cap=CMD_CAP):
    o, m = po.message_unmarshal(data)
    if o == "ok" and any(len(e["cmd"]) > cmd_cap for e in m["entries"]):
        o = "big"
    return o, m


def test_hand_cases(decoder, tmp_path):
    cases = wc.hand_cases(1, CMD_CAP)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for want in ("ok", "bad", "snapshot", "big"):
        assert any(c.outcome == want for c in cases), want
    got = run_decoder(decoder, [c.data for c in cases], tmp_path)
    for c, g in zip(cases, got):
        check_passes(c.name, g)
        oo, om = oracle_outcome(c.data)
        assert c.outcome == oo == g[2], (c.name, c.go, c.outcome, oo, g[2])
        if c.outcome in ("ok", "big"):
            want = expected_msg(c.msg)
            assert want == om, (c.name, c.go, "oracle", want, om)
            assert want == g[4], (c.name, c.go, "decoder", want, g[4])


def test_named_refusal_is_the_only_one():
    """Wire type 3 is the one input Go accepts that the decoder (and the
    oracle) refuse: the case exists, by name, and expects `bad`."""
    cases = {c.name: c for c in wc.hand_cases(1, CMD_CAP)}
    c = cases["refuse_group_wire_type_3"]
    assert c.outcome == "bad" and "MD_REFUSE_GROUP" in c.go
    hdr = open(os.path.join(HERE, "..", "dragonboat_amd", "csrc",
                            "drb_msgdec.hpp")).read()
    assert "MD_REFUSE_GROUP" in hdr


def test_mutations(decoder, tmp_path):
    """The 16000 mutations, and the 256 the GPU test ingests (one shard
    each), so that every byte string the GPU sees went through here."""
    muts = wc.mutations(1)
    assert len(muts) == 4 * wc.MUT_COUNT
    muts = muts + wc.mutation_sample(256, 1)
    got = run_decoder(decoder, [d for _, d in muts], tmp_path)
    seen = set()
    for (name, data), g in zip(muts, got):
        check_passes(name, g)
        oo, om = oracle_outcome(data)
        assert oo == g[2], (name, oo, g[2])
        if oo in ("ok", "big"):
            assert om == g[4], (name, om, g[4])
        seen.add(oo)
    assert {"ok", "bad"} <= seen, seen  # the mutations reach both sides


def test_mutations_are_deterministic():
    assert wc.mutations(1, count=50) == wc.mutations(1, count=50)
    assert wc.mutation_sample(8, 1) == wc.mutation_sample(8, 1)
