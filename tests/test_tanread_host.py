"""CPU: the tan read path (dragonboat_amd/csrc/drb_tanread.hpp) against the
oracle's record reader (oracle/tan_oracle.c orc_tan_read, record.go:163-311
restated) and the independent Update decoder of tests/test_oracle_tan.py.

The header is compiled as plain C++ into a stand-alone program
(tests/tanread_host_main.cc) with -fsanitize=address,undefined; every log is
handed to it in a heap buffer of exactly the file's length.  A sanitizer
report makes the program exit non-zero, which fails the test.  The logs are
written by the oracle's tan db (tests/tan_images.py).
"""
import os
import shutil
import subprocess

import pytest

from oracle import pyoracle as po
from tests import tan_images as ti
from tests.test_oracle_tan import _decode_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tanread_host_main.cc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("tanread") / "tanread_host_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", out, SRC]
    # (the runtimes linked statically where the compiler can, as
    # tests/test_snappy_host.py)
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.call(cmd + static, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    return out


def _hex(b):
    return b.hex() or "-"


def _run(prog, tmp_path, lines):
    path = str(tmp_path / "commands.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([prog, path], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    out = r.stdout.decode().split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def _scan(prog, tmp_path, files):
    """[(outcome, valid_end, [record dicts])] of the program's scan."""
    res = []
    for line in _run(prog, tmp_path, ["scan " + _hex(f) for f in files]):
        t = line.split()
        recs = []
        for r in t[3:]:
            v = [int(x) for x in r.split(":")]
            recs.append(dict(zip(("offset", "end", "shard_id", "replica_id",
                                  "has_state", "term", "vote", "commit",
                                  "first_index", "last_index", "n_entries"),
                                 v)))
        assert len(recs) == int(t[2])
        res.append((int(t[0]), int(t[1]), recs))
    return res


def _dump(prog, tmp_path, files):
    """[(outcome, [(offset, payload, [entry dicts])])]."""
    res = []
    for line in _run(prog, tmp_path, ["dump " + _hex(f) for f in files]):
        t = line.split()
        recs = []
        for r in t[2:]:
            off, pay, ents = r.split(":")
            es = []
            for e in ([] if ents == "-" else ents.split(",")):
                v = e.split("/")
                d = dict(zip(("term", "index", "type", "key", "client_id",
                              "series_id", "responded_to"),
                             [int(x) for x in v[:7]]))
                d["cmd"] = b"" if v[7] == "-" else bytes.fromhex(v[7])
                es.append(d)
            recs.append((int(off), b"" if pay == "-" else bytes.fromhex(pay),
                         es))
        res.append((int(t[0]), recs))
    return res


def _replica(prog, tmp_path, jobs):
    """jobs: [(shard, replica, base, cmd_cap, W, snappy, files)] ->
    [(plan dict, {index: (term, cmd)}, [(applied index, term)])]."""
    lines = ["replica %d %d %d %d %d %d %s" % (
        j[0], j[1], j[2], j[3], j[4], j[5],
        " ".join(_hex(f) for f in j[6])) for j in jobs]
    res = []
    for line in _run(prog, tmp_path, lines):
        head, log, app = line.split("|")
        plan = dict(zip(("status", "files", "offset", "records", "entries",
                         "term", "vote", "commit", "last_index", "applied"),
                        [int(x) for x in head.split()]))
        lg = {}
        for e in (log.split(",") if log else []):
            i, t, c = e.split("/")
            lg[int(i)] = (int(t), b"" if c == "-" else bytes.fromhex(c))
        ap = [tuple(int(x) for x in a.split("/"))
              for a in (app.split(",") if app else [])]
        res.append((plan, lg, ap))
    return res


# ---------------------------------------------------------------- case 1
def _clean_shapes():
    small = ti.write_logs(ti.steady_updates(40), 3, 1, 1024)
    big = ti.write_logs(ti.steady_updates(70, val=bytes(range(256)) * 4), 3, 1,
                        1 << 16)
    state_only = ti.write_logs([((2, 1, 0), []), ((2, 1, 4), []),
                                ((3, 0, 4), []), (None, []),
                                ((3, 2, 1 << 40), [])], 1 << 33, 3)
    over = ti.write_logs(ti.overwrite_updates(), 9, 1)
    return dict(small=small, big=big, state_only=state_only, over=over)


def test_clean_logs_equal_the_oracle(prog, tmp_path):
    shapes = _clean_shapes()
    assert len(shapes["small"]) >= 3          # several files
    assert len(shapes["big"]) >= 2
    big = shapes["big"][0]
    assert len(big) > 32768
    # records across blocks (a MIDDLE / LAST chunk at a block start) or
    # padding before one
    assert any(big[b + 6] in (3, 4) or big[b - 1] == 0
               for b in range(32768, len(big), 32768))
    for name, files in shapes.items():
        dumps = _dump(prog, tmp_path, files)
        scans = _scan(prog, tmp_path, files)
        for f, (oc, recs), (oc2, vend, srecs) in zip(files, dumps, scans):
            want = po.tan_read(f)
            assert oc == ti.EOF and oc2 == ti.EOF, name
            assert [(o, p) for o, p, _ in recs] == want, name
            assert vend == len(f), name
            assert [r["offset"] for r in srecs] == [o for o, _ in want]
            assert [r["end"] for r in srecs] == \
                [o for o, _ in want[1:]] + [len(f)]
            for (off, pay, ents), sr in zip(recs, srecs):
                shard, replica, state, dents = _decode_update(pay)
                assert (sr["shard_id"], sr["replica_id"]) == (shard, replica)
                assert sr["has_state"] == (state is not None)
                assert (sr["term"], sr["vote"], sr["commit"]) == \
                    (state or (0, 0, 0))
                assert sr["n_entries"] == len(dents)
                assert (sr["first_index"], sr["last_index"]) == \
                    ((dents[0]["index"], dents[-1]["index"]) if dents
                     else (0, 0))
                assert ents == dents, (name, off)


def test_overwrite_and_multi_file_replay(prog, tmp_path):
    shapes = _clean_shapes()
    jobs = [(9, 1, 0, 64, 64, 0, shapes["over"]),
            (3, 1, 0, 64, 64, 0, shapes["small"]),
            (3, 1, 0, 1100, 64, 0, shapes["big"]),
            (3, 1, 7, 64, 64, 0, shapes["small"]),      # a base inside
            (3, 1, 0, 64, 16, 0, shapes["small"]),      # a small window
            # State-only records: the log is all below the base
            (1 << 33, 3, 1 << 40, 64, 64, 0, shapes["state_only"])]
    res = _replica(prog, tmp_path, jobs)
    plan, log, ap = res[0]
    assert plan["status"] == ti.OK
    assert [(i, log[i][0]) for i in sorted(log)] == \
        [(i, 2) for i in range(1, 6)] + [(i, 3) for i in range(6, 9)]
    assert (plan["term"], plan["vote"], plan["commit"],
            plan["last_index"]) == (3, 2, 8, 8)
    # every committed entry applied once, in order, in its final form
    assert ap == [(i, 2) for i in range(1, 6)] + [(i, 3) for i in range(6, 9)]
    for job, (plan, log, ap) in zip(jobs[:5], res[:5]):
        base = job[2]
        state, mlog, _, _ = ti.replay_model(job[6], base)
        assert plan["status"] == ti.OK, plan
        assert (plan["term"], plan["vote"], plan["commit"]) == state
        assert plan["last_index"] == max(mlog)
        assert {i: (e["term"], e["cmd"]) for i, e in mlog.items()} == log
        assert [i for i, _ in ap] == list(range(base + 1, state[2] + 1))
        assert plan["files"] == len(job[6])
        assert plan["offset"] == len(job[6][-1])
    plan, log, ap = res[5]
    assert plan["status"] == ti.OK and not log and not ap
    assert (plan["term"], plan["vote"], plan["commit"],
            plan["last_index"]) == (3, 2, 1 << 40, 1 << 40)


# ---------------------------------------------------------------- case 2
def test_every_truncation_length(prog, tmp_path):
    data = ti.small_log()
    full = po.tan_read(data)
    assert len(full) >= 12 and 500 < len(data) < 1500
    ends = [o for o, _ in full[1:]] + [len(data)]
    cuts = [data[:n] for n in range(len(data) + 1)]
    got = _scan(prog, tmp_path, cuts)
    classes = {}
    for n, (oc, vend, recs) in enumerate(got):
        want, wrecs = ti.oracle_outcome(cuts[n])
        assert oc == want, n
        kept = sum(e <= n for e in ends)
        assert len(recs) == kept, n
        if wrecs is not None:
            assert len(wrecs) == kept, n
        assert vend == ([0] + ends)[kept], n
        classes[oc] = classes.get(oc, 0) + 1
    # a cut at a record boundary reads clean, any other is an invalid chunk
    assert classes == {ti.EOF: len(full) + 1,
                       ti.INVALID: len(data) - len(full)}, classes


# ---------------------------------------------------------------- case 3
def test_mutations_and_zero_tails(prog, tmp_path):
    data = ti.small_log()
    full = po.tan_read(data)
    starts = [o for o, _ in full]
    muts = ti.mutations(data)
    tails = [data + bytes(n) for n in (1, 6, 7, 64)]
    files = [m for _, m in muts] + tails
    got = _scan(prog, tmp_path, files)
    counts = {}
    for k, (f, (oc, vend, recs)) in enumerate(zip(files, got)):
        want, wrecs = ti.oracle_outcome(f)
        # a flipped bit the chunks do not cover cannot be seen by the reader;
        # one the Update decoder refuses is MALFORMED where the oracle's
        # reader, which does not unmarshal, reads clean
        if oc == ti.MALFORMED:
            assert want == ti.EOF, k
        else:
            assert oc == want, (k, oc, want)
        counts[oc] = counts.get(oc, 0) + 1
        # the kept records read clean through the oracle, and are all of them
        assert len(po.tan_read(f[:vend], 4096)) == len(recs), k
        if k < len(muts) and oc == ti.CRC:
            assert len(recs) == sum(s <= muts[k][0] for s in starts) - 1, k
        if wrecs is not None and oc == ti.EOF:
            assert len(wrecs) == len(recs), k
    assert got[len(muts) + 2][0] == ti.EOF        # 7 zero bytes: clean
    assert got[len(muts) + 3][0] == ti.ZEROED     # 64 zero bytes
    assert counts.get(ti.MALFORMED, 0) == 0, counts
    n = len(muts)
    assert counts[ti.CRC] > 0.9 * n, counts
    assert 0 < counts[ti.INVALID] < 0.1 * n, counts
    assert counts[ti.ZEROED] >= 1 and counts[ti.EOF] >= 1, counts
    assert sum(counts.values()) == len(files)


# ---------------------------------------------------------------- case 4
def test_hostile_lengths_are_malformed(prog, tmp_path):
    host = ti.hostile_records()
    assert {"entry_count_max", "entry_len_past_record", "uvarint_11_bytes",
            "state_len_max"} <= set(host)
    good = ti.record(po.update_marshal(5, 2, (2, 1, 1), []))
    files = [good + ti.record(p) for p in host.values()]
    for f in files:  # the chunks check out: the oracle's reader is content
        assert len(po.tan_read(f)) == 2
    got = _scan(prog, tmp_path, files)
    for name, (oc, vend, recs) in zip(host, got):
        assert oc == ti.MALFORMED, name
        assert len(recs) == 1 and vend == len(good), name
    # and as a replica's log: corrupt, not a tail
    res = _replica(prog, tmp_path, [(5, 2, 0, 64, 64, 0, [f]) for f in files])
    for name, (plan, _, _) in zip(host, res):
        assert plan["status"] == ti.CORRUPT, name


def test_recover_cases_statuses(prog, tmp_path):
    """The images of the device test's rejected inputs, through pass 1 and
    pass 2 of the same header under the sanitizers first."""
    cases = ti.recover_cases()
    jobs = [(1 + g, 1, 0, ti.CMD_CAP, ti.W, 0, files)
            for g, (files, _) in enumerate(cases.values())]
    res = _replica(prog, tmp_path, jobs)
    for (name, (files, status)), (plan, log, ap) in zip(cases.items(), res):
        assert plan["status"] == status, (name, plan)
        if status == ti.TAIL_CUT:
            recs = po.tan_read(files[-1][:plan["offset"]])
            assert plan["files"] == len(files)
            # the oracle's boundary: the records before the cut, no more
            with pytest.raises(po.OracleError):
                po.tan_read(files[-1])
            assert len(recs) == 2
            state, mlog, _, _ = ti.replay_model(
                files[:-1] + [files[-1][:plan["offset"]]])
            assert {i: (e["term"], e["cmd"]) for i, e in mlog.items()} == log
            assert (plan["term"], plan["vote"], plan["commit"]) == state
    # a window the pending span does not fit is refused in pass 1
    ups = [((2, 1, 0), [ti.kv_ent(i, 2, b"k", b"v") for i in range(1, 40)]),
           ((2, 1, 39), [])]
    f = ti.write_logs(ups, 1, 1)
    (plan, _, _), (plan2, log2, ap2) = _replica(
        prog, tmp_path, [(1, 1, 0, 64, 32, 0, f), (1, 1, 0, 64, 64, 0, f)])
    assert plan["status"] == ti.CAPACITY
    assert plan2["status"] == ti.OK and len(ap2) == 39


def test_overwritten_tail_and_the_window(prog, tmp_path):
    """A tail that an overwrite cuts off again has still passed through the
    window: index i took slot i mod W.  The program's placer keeps such a
    ring and refuses to apply an entry that is no longer its slot's occupant
    (status 8), and checks the window pass 2 reports (status 100); pass 1
    must say CAPACITY before either can happen.  Entries 1..n uncommitted,
    10..12 rewritten, then commit 12, W = 64: the pending 1..12 are intact
    exactly while n < 64."""
    W = 64
    ns = list(range(13, 140, 3)) + [62, 63, 64, 65, 73, 127, 128, 129]
    jobs = [(1, 1, 0, 64, W, 0,
             ti.write_logs(ti.tail_overwritten_updates(n), 1, 1)) for n in ns]
    for n, (plan, log, ap) in zip(ns, _replica(prog, tmp_path, jobs)):
        assert plan["status"] == (ti.OK if n < W else ti.CAPACITY), (n, plan)
        if n < W:
            assert ap == [(i, 2) for i in range(1, 10)] + \
                [(i, 3) for i in range(10, 13)], n
            assert sorted(log) == list(range(1, 13)), n
            assert plan["last_index"] == 12, n
    # a tail that grows again after the cut: the commit catches up in steps
    ups = ti.tail_overwritten_updates(60)
    ups += [((3, 2, 12 + 8 * k), [ti.kv_ent(i, 3, b"g", b"h%d" % i)
                                  for i in range(13 + 8 * k, 21 + 8 * k)])
            for k in range(12)]
    ups.append(((3, 2, 108), []))
    (plan, log, ap), = _replica(prog, tmp_path,
                                [(1, 1, 0, 64, W, 0,
                                  ti.write_logs(ups, 1, 1))])
    assert plan["status"] == ti.OK, plan
    assert [i for i, _ in ap] == list(range(1, 109))


# ---------------------------------------------------------------- case 5
def test_drb_tan_scan_equals_the_oracle():
    """The library's host entry point (no engine, no device) on the same
    cases."""
    from dragonboat_amd import engine
    try:
        engine.lib()
    except (OSError, RuntimeError) as e:
        pytest.skip("libdrb_engine.so does not load on this machine: %s" % e)
    for name, files in _clean_shapes().items():
        for f in files:
            oc, vend, recs = engine.tan_scan(f)
            want = po.tan_read(f)
            assert (oc, vend) == (ti.EOF, len(f)), name
            assert [r["offset"] for r in recs] == [o for o, _ in want]
            for r, (_, pay) in zip(recs, want):
                shard, replica, state, ents = _decode_update(pay)
                assert (r["shard_id"], r["replica_id"], r["has_state"],
                        r["n_entries"]) == (shard, replica,
                                            int(state is not None), len(ents))
                assert (r["term"], r["vote"], r["commit"]) == \
                    (state or (0, 0, 0))
                assert (r["first_index"], r["last_index"]) == \
                    ((ents[0]["index"], ents[-1]["index"]) if ents else (0, 0))
    data = ti.small_log()
    ends = [o for o, _ in po.tan_read(data)[1:]] + [len(data)]
    for n in range(len(data) + 1):
        oc, vend, recs = engine.tan_scan(data[:n])
        assert oc == ti.oracle_outcome(data[:n])[0], n
        assert len(recs) == sum(e <= n for e in ends), n
    for i, m in ti.mutations(data, n=400, seed=11):
        oc, vend, recs = engine.tan_scan(m)
        assert oc == ti.oracle_outcome(m)[0], i
    assert engine.tan_scan(data + bytes(64))[0] == ti.ZEROED
    assert engine.tan_scan(data + bytes(7))[0] == ti.EOF
    good = ti.record(po.update_marshal(5, 2, (2, 1, 1), []))
    for name, p in ti.hostile_records().items():
        oc, vend, recs = engine.tan_scan(good + ti.record(p))
        assert (oc, vend, len(recs)) == (ti.MALFORMED, len(good), 1), name
    # a cap below the record count: the count is the full one
    oc, vend, recs = engine.tan_scan(data, cap=3)
    assert oc == ti.EOF and len(recs) == 3 and vend == len(data)
