"""CPU: the multiplexed tan read path (dragonboat_amd/csrc/drb_tanmux.hpp)
against the sequential reader of drb_tanread.hpp and the oracle's record
reader.

tests/tanmux_host_main.cc is compiled as plain C++ with
-fsanitize=address,undefined, as tests/test_tanread_host.py builds its
program; it summarizes the blocks of every file in reverse order, composes
them, lists and partitions the records and runs the per-replica passes with
the ring placer of tanread_host_main.cc.  The images are written by the
oracle's shared db (tests/tan_mux_images.py).
"""
import os
import shutil
import subprocess

import pytest

from oracle import pyoracle as po
from tests import tan_images as ti
from tests import tan_mux_images as tm
from tests.test_tanread_host import _hex, _replica, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tanmux_host_main.cc")
B = ti.B


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("tanmux") / "tanmux_host_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", out, SRC]
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.call(cmd + static, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def big():
    files = tm.big_files()
    img = files[0]
    assert len(files) >= 2 and len(img) > 2 * B          # 3 blocks
    # the second block starts inside a record
    assert img[B + 6] in (3, 4), img[B + 6]
    return files


def _line(t):
    v = t.split()
    recs = [tuple(int(x) for x in r.split(":")) for r in v[3:]]
    assert len(recs) == int(v[2])
    return int(v[0]), int(v[1]), recs


def _index_and_seq(prog, tmp_path, files):
    """[(outcome, valid_end, [(off, end, shard, replica)])] by the block
    index, checked equal to the sequential reader's."""
    out = _run(prog, tmp_path, [c + _hex(f) for f in files
                                for c in ("index ", "seq ")])
    res = []
    for k in range(len(files)):
        assert out[2 * k] == out[2 * k + 1], (k, len(files[k]))
        res.append(_line(out[2 * k]))
    return res


def _against_oracle(f, got, where):
    oc, vend, recs = got
    want, wrecs = ti.oracle_outcome(f)
    assert oc == want, (where, oc, want)
    kept = po.tan_read(f[:vend], 4096)
    assert [o for o, _ in kept] == [r[0] for r in recs], where
    if wrecs is not None:
        assert len(wrecs) == len(recs) and vend <= len(f), where
    return oc


# ---------------------------------------------------------------- case 1
def test_index_equals_the_sequential_reader_clean(prog, tmp_path, big):
    from tests.test_oracle_tan import _decode_update
    small = tm.small_shared()
    assert 500 < len(small) < 1500
    files = big + [small]
    for f, got in zip(files, _index_and_seq(prog, tmp_path, files)):
        assert _against_oracle(f, got, len(f)) == ti.EOF
        want = po.tan_read(f)
        assert got[1] == len(f)
        assert [(r[2], r[3]) for r in got[2]] == \
            [_decode_update(p)[:2] for _, p in want]
        assert [r[1] for r in got[2]][:-1] == [o for o, _ in want[1:]]
    assert len({r[2] for r in _line(_run(prog, tmp_path,
                                         ["index " + _hex(big[0])])[0])[2]}) \
        == 3                                          # three shards in one log


def test_index_every_truncation_of_a_small_log(prog, tmp_path):
    data = tm.small_shared()
    ends = [o for o, _ in po.tan_read(data)[1:]] + [len(data)]
    cuts = [data[:n] for n in range(len(data) + 1)]
    classes = {}
    for n, got in enumerate(_index_and_seq(prog, tmp_path, cuts)):
        oc = _against_oracle(cuts[n], got, n)
        kept = sum(e <= n for e in ends)
        assert len(got[2]) == kept and got[1] == ([0] + ends)[kept], n
        classes[oc] = classes.get(oc, 0) + 1
    assert classes == {ti.EOF: len(ends) + 1,
                       ti.INVALID: len(data) - len(ends)}, classes


def test_index_truncations_at_blocks_and_record_ends(prog, tmp_path, big):
    img = big[0]
    ends = [o for o, _ in po.tan_read(img)[1:]] + [len(img)]
    marks = [b for b in range(B, len(img), B)] + ends
    ns = sorted({n for m in marks for n in range(m - 40, m + 41)
                 if 0 <= n <= len(img)})
    seen = set()
    # (one program run per chunk of cuts: the command file stays small)
    for i in range(0, len(ns), 64):
        part = ns[i:i + 64]
        res = _index_and_seq(prog, tmp_path, [img[:n] for n in part])
        for n, got in zip(part, res):
            oc = _against_oracle(img[:n], got, n)
            kept = sum(e <= n for e in ends)
            assert len(got[2]) == kept and got[1] == ([0] + ends)[kept], n
            seen.add(oc)
    # a cut at a block boundary behind a FIRST chunk: the record has no LAST
    assert img[B + 6] in (3, 4)
    (oc, vend, recs), = _index_and_seq(prog, tmp_path, [img[:B]])
    assert oc == ti.UNEXPECTED_EOF and vend == max(e for e in ends if e <= B)
    assert {ti.EOF, ti.INVALID, ti.UNEXPECTED_EOF} <= seen, seen


def test_index_mutations_flips_and_zero_tails(prog, tmp_path, big):
    data = tm.small_shared()
    muts = ti.mutations(data)
    tails = [data + bytes(n) for n in (1, 6, 7, 64)]
    img = big[0]
    flips = []
    for at in (B // 2, B + B // 2, len(img) - 40):    # first, middle, last
        m = bytearray(img)
        m[at] ^= 0x04
        flips.append(bytes(m))
    files = [m for _, m in muts] + tails + flips + \
        [img + bytes(n) for n in (1, 6, 7, 64)]
    got = _index_and_seq(prog, tmp_path, files)
    counts = {}
    for k, (f, g) in enumerate(zip(files, got)):
        oc = _against_oracle(f, g, k)
        counts[oc] = counts.get(oc, 0) + 1
    n = len(muts)
    assert got[n + 2][0] == ti.EOF and got[n + 3][0] == ti.ZEROED
    starts = [o for o, _ in po.tan_read(img)]
    for at, g in zip((B // 2, B + B // 2, len(img) - 40), got[n + 4:n + 7]):
        assert g[0] == ti.CRC, at
        assert len(g[2]) == sum(s <= at for s in starts) - 1, at
    assert counts[ti.CRC] > 0.9 * n and counts[ti.INVALID] > 0, counts
    assert counts.get(ti.MALFORMED, 0) == 0, counts


# ---------------------------------------------------------------- case 2
PLAN_FIELDS = ("status", "term", "vote", "commit", "last_index", "records",
               "entries", "applied")


def _mux(prog, tmp_path, slot, first, groups, logs, base=0, cmd_cap=64,
         W=ti.W):
    line, = _run(prog, tmp_path, [tm.mux_command(slot, first, groups, base,
                                                 cmd_cap, W, 0, logs)])
    return tm.parse_mux(line)


def test_demultiplexing_equivalence(prog, tmp_path):
    lists = tm.equivalence_lists(first_shard=5)
    first, groups = 5, tm.KEYS * len(lists)
    logs = tm.shared_logs(lists, 1, 1024)
    assert list(logs) == [5] and len(logs[5]) >= 4      # one log, many files
    lst, reps = _mux(prog, tmp_path, 0, first, groups, logs)
    assert lst[5][0] == ti.OK
    assert lst[5][1:3] == (len(logs[5]) - 1, len(logs[5][-1]))
    own = _replica(prog, tmp_path,
                   [(shard, 1, 0, 64, ti.W, 0, ti.write_logs(ups, shard, 1))
                    for shard, ups in lists.items()])
    assert sum(r[0]["records"] for r in own) == lst[5][3]
    statuses = set()
    for (shard, ups), (plan, log, ap) in zip(lists.items(), own):
        mplan, mlog, map_ = reps[shard - first]
        assert {f: mplan[f] for f in PLAN_FIELDS} == \
            {f: plan[f] for f in PLAN_FIELDS}, shard
        assert (mlog, map_) == (log, ap), shard
        statuses.add(plan["status"])
    assert statuses == {ti.OK, ti.CAPACITY}


# ---------------------------------------------------------------- case 3
def _three(replica=2):
    lists = {s: ti.steady_updates(12, first=1) for s in (5, 21, 37)}
    return lists, tm.write_shared(tm.interleave(lists), replica, 1024)


def test_log_level_refusals(prog, tmp_path):
    lists, files = _three()
    assert len(files) >= 3
    slot, first, groups = 1, 5, 33
    gs = [s - first for s in lists]
    clean_lst, clean = _mux(prog, tmp_path, slot, first, groups, {5: files})
    assert clean_lst[5][0] == ti.OK
    assert all(clean[g][0]["status"] == ti.OK for g in gs)
    host = ti.hostile_records()

    def with_tail(rec):
        return files[:-1] + [files[-1] + rec]

    flip = bytearray(files[0])
    flip[po.tan_read(files[0])[1][0] + ti.HDR + 12] ^= 0x10
    mid = po.tan_read(files[0])[2][0] + 9
    other_key = ti.record(po.update_marshal(6, 2, (2, 1, 1), []))
    other_rep = ti.record(po.update_marshal(21, 3, (2, 1, 1), []))
    outside = ti.record(po.update_marshal(5 + 16 * 40, 2, (2, 1, 1), []))
    refused = {
        "crc_early": ([bytes(flip)] + files[1:], ti.CORRUPT),
        "invalid_early": ([files[0][:mid]] + files[1:], ti.CORRUPT),
        "crc_last": (files[:-1] + [files[-1][:-3] +
                                   bytes([files[-1][-3] ^ 1]) +
                                   files[-1][-2:]], ti.CORRUPT),
        "ids_11_bytes": (with_tail(ti.record(host["uvarint_11_bytes"])),
                         ti.CORRUPT),
        "ids_overflow": (with_tail(ti.record(host["uvarint_overflow"])),
                         ti.CORRUPT),
        "ids_empty": (with_tail(ti.record(host["empty"])), ti.CORRUPT),
        "other_key": (with_tail(other_key), ti.MISMATCH),
        "other_replica": (with_tail(other_rep), ti.MISMATCH),
        "not_a_group": (with_tail(outside), ti.MISMATCH),
    }
    for name, (fs, want) in refused.items():
        lst, reps = _mux(prog, tmp_path, slot, first, groups, {5: fs})
        assert lst[5][0] == want, name
        for g in gs:
            plan, log, ap = reps[g]
            assert plan["status"] == want and not log and not ap, (name, g)
    # the same cut in the last file ends the log there: every replica keeps
    # its records in front of it
    last = po.tan_read(files[-1])
    assert len(last) >= 3
    cut_at = last[2][0] + 9
    fs = files[:-1] + [files[-1][:cut_at]]
    lst, reps = _mux(prog, tmp_path, slot, first, groups, {5: fs})
    assert lst[5][:3] == (ti.TAIL_CUT, len(files) - 1, last[2][0])
    kept = sum(len(po.tan_read(f)) for f in files[:-1]) + 2
    assert lst[5][3] == kept == sum(reps[g][0]["records"] for g in gs)
    assert len(po.tan_read(fs[-1][:lst[5][2]])) == 2
    with pytest.raises(po.OracleError):
        po.tan_read(fs[-1])
    for g in gs:
        plan, log, ap = reps[g]
        assert plan["status"] == ti.OK, g
        assert plan["last_index"] == max(log), g
        assert [i for i, _ in ap] == list(range(1, plan["commit"] + 1)), g
        assert 0 < plan["records"] <= clean[g][0]["records"]
    assert sum(reps[g][0]["records"] for g in gs) < \
        sum(clean[g][0]["records"] for g in gs)
    # a record whose ids parse and whose Update does not: its replica alone
    for name in ("state_len_max", "entry_len_past_record", "cut_after_ids"):
        lst, reps = _mux(prog, tmp_path, slot, first, groups,
                         {5: with_tail(ti.record(host[name]))})
        assert lst[5][0] == ti.OK, name
        assert [reps[g][0]["status"] for g in gs] == \
            [ti.CORRUPT, ti.OK, ti.OK], name
        assert reps[gs[1]] == clean[gs[1]], name


# ---------------------------------------------------------------- case 4
def test_replica_level_refusals(prog, tmp_path):
    first = 1
    lists, want = tm.replica_case_lists(first)
    logs = tm.shared_logs(lists, 1, 1024)
    assert list(logs) == [1] and len(logs[1]) >= 3
    groups = tm.KEYS * len(lists)
    lst, reps = _mux(prog, tmp_path, 0, first, groups, logs,
                     cmd_cap=ti.CMD_CAP)
    assert lst[1][0] == ti.OK
    cases = ti.recover_cases()
    for shard, (name, status) in want.items():
        plan, log, ap = reps[shard - first]
        assert plan["status"] == status, (name, plan)
        if status == ti.OK:
            state, mlog, _, _ = ti.replay_model(cases[name][0])
            assert (plan["term"], plan["vote"], plan["commit"]) == state
            assert {i: (e["term"], e["cmd"]) for i, e in mlog.items()} == log
            assert [i for i, _ in ap] == list(range(1, state[2] + 1)), name
        else:
            assert not log and not ap, name
    assert {s for _, s in want.values()} == {ti.OK, ti.GAP, ti.ENTRY_TYPE,
                                             ti.CAPACITY, ti.EMPTY}
