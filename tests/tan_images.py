"""Tan log images for the read-path tests (tests/test_tanread_host.py on the
CPU, tests/test_gpu_recover.py on the device): every log is written by the
oracle's tan db (po.TanDB, internal/tan/db.go:97-130 restated), then cut or
mutated here.  The GPU test takes its rejected inputs from recover_cases(),
the same images the sanitized CPU program reads first.
"""
import random
import struct

from oracle import pyoracle as po

B = 32768
HDR = 7

# the reader's outcome classes: drb_tan_scan's outcome, the oracle's message
EOF, ZEROED, INVALID, CRC, UNEXPECTED_EOF, MALFORMED = range(6)
ORACLE_CLASS = {"zeroed chunk": ZEROED, "invalid chunk": INVALID,
                "crc mismatch": CRC, "unexpected EOF": UNEXPECTED_EOF}
# drb_recover_tan's statuses (abi.REC_*)
OK, TAIL_CUT, EMPTY, CORRUPT, MISMATCH, GAP, ENTRY_TYPE, CAPACITY, \
    APPLY_STOPPED, SNAPSHOT = range(10)


def oracle_outcome(data):
    """(class, records or None) of the oracle's record reader on data."""
    try:
        return EOF, po.tan_read(data, 4096)
    except po.OracleError as e:
        msg = str(e).split("tan read: ")[-1]
        return ORACLE_CLASS[msg], None


def kv_cmd(key, val):
    """An application entry's Cmd: the PBKV of key -> val."""
    return po.pbkv_marshal(key, val)


def kv_ent(index, term, key, val, **kw):
    return po.ent(term=term, index=index, type=0, key=1000 + index,
                  client_id=77, cmd=kv_cmd(key, val), **kw)


def write_logs(updates, shard, replica, max_log=0):
    """The files of one replica's tan db after db.write of each
    (state or None, entries): [bytes per log number]."""
    db = po.TanDB(max_log)
    for state, ents in updates:
        db.write(shard, replica, state, ents)
    n = db.last()["log"] + 1
    return [db.file(lg) for lg in range(n)]


def steady_updates(n, term=2, val=b"v" * 16, first=1, commit_lag=1):
    """n Updates of one entry each, the State's commit commit_lag behind."""
    out = []
    for i in range(n):
        idx = first + i
        out.append(((term, 1, max(0, idx - commit_lag)),
                    [kv_ent(idx, term, b"k%03d" % (idx % 7), val)]))
    out.append(((term, 1, first + n - 1), []))
    return out


def overwrite_updates():
    """Entries 1..10 at term 2 (commit 5), then 6..8 at term 3: the final
    log is 1..5 at term 2 followed by 6..8 at term 3."""
    a = [kv_ent(i, 2, b"a%d" % i, b"x%d" % i) for i in range(1, 11)]
    b = [kv_ent(i, 3, b"a%d" % i, b"y%d" % i) for i in range(6, 9)]
    return [((2, 1, 5), a), ((3, 2, 5), b), ((3, 2, 8), [])]


def tail_overwritten_updates(n):
    """Entries 1..n saved uncommitted at term 2 (a cut-off leader's tail),
    10..12 rewritten at term 3, then commit 12."""
    a = [kv_ent(i, 2, b"t%d" % (i % 50), b"a%d" % i) for i in range(1, n + 1)]
    b = [kv_ent(i, 3, b"t%d" % (i % 50), b"b%d" % i) for i in range(10, 13)]
    return [((2, 1, 0), a), ((3, 2, 0), b), ((3, 2, 12), [])]


def small_log(shard=5, replica=2):
    """A multi-record log of about 1 KB: entries, State-only records and a
    record without State."""
    ups = []
    for i in range(1, 13):
        ups.append(((2, 1, i - 1), [kv_ent(i, 2, b"k%d" % i, b"val%02d" % i)]))
        if i % 3 == 0:
            ups.append(((2, 1, i), []))
    ups.append((None, []))
    files = write_logs(ups, shard, replica)
    assert len(files) == 1
    return files[0]


def mutations(data, n=3000, seed=0x7A9):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        i = rnd.randrange(len(data))
        m = bytearray(data)
        m[i] ^= 1 << rnd.randrange(8)
        out.append((i, bytes(m)))
    return out


def record(payload):
    """One FULL chunk with a valid checksum around payload."""
    crc = po.xxh64(b"\x01" + payload) & 0xFFFFFFFF
    return struct.pack("<IHB", crc, len(payload), 1) + payload


def hostile_records():
    """Records whose chunks check out and whose Update lies about a length."""
    good_ent = po.entry_marshal(kv_ent(1, 2, b"k", b"v"))
    le = lambda x: struct.pack("<I", x)
    return {
        "entry_count_max": b"\x05\x02\x00" + le(0xFFFFFFFF) + b"\x00",
        "entry_count_one_short": b"\x05\x02\x00" + le(2) + le(len(good_ent))
        + good_ent + b"\x00",
        "entry_len_past_record": b"\x05\x02\x00" + le(1) + le(len(good_ent)
                                                             + 40)
        + good_ent + b"\x00",
        "entry_len_zero": b"\x05\x02\x00" + le(1) + le(0) + b"\x00",
        "uvarint_11_bytes": b"\x80" * 10 + b"\x01" + b"\x02\x00" + le(0)
        + b"\x00",
        "uvarint_overflow": b"\xff" * 9 + b"\x02" + b"\x02\x00" + le(0)
        + b"\x00",
        "state_len_max": b"\x05\x02\x01" + le(0xFFFFFFFF) + b"\x08\x02",
        "state_value_past_state": b"\x05\x02\x01" + le(2) + b"\x08\x80\x01"
        + le(0) + b"\x00",
        "cmd_len_past_entry": b"\x05\x02\x00" + le(1) + le(6)
        + b"\x01\x01\x07\x7f\x41\x7f" + b"\x00",
        "no_snapshot_flag": b"\x05\x02\x00" + le(0),
        "cut_after_ids": b"\x05\x02",
        "trailing_bytes": b"\x05\x02\x00" + le(0) + b"\x00\x00",
        "empty": b"",
    }


# ---------------------------------------------------------------- recovery
CMD_CAP = 32   # the engine configuration of test_recover_overwritten_and_cut
W = 64


def recover_cases(first_shard=1):
    """{name: (files of replica 1 of its group, expected status)}; the group
    of a case is its position in this dict, its ShardID first_shard + that."""
    cases = {}

    def shard():
        return first_shard + len(cases)

    cases["clean"] = (write_logs(steady_updates(20), shard(), 1, 1024), OK)
    cases["overwrite"] = (write_logs(overwrite_updates(), shard(), 1), OK)
    files = write_logs(steady_updates(20), shard(), 1, 1024)
    assert len(files) >= 2
    recs = po.tan_read(files[-1])
    assert len(recs) >= 3
    cut_at = recs[2][0] + 9  # inside the third record of the last log
    cases["tail_cut"] = (files[:-1] + [files[-1][:cut_at]], TAIL_CUT)
    files = write_logs(steady_updates(20), shard(), 1, 1024)
    recs = po.tan_read(files[0])
    cases["cut_in_earlier_log"] = ([files[0][:recs[2][0] + 9]] + files[1:],
                                   CORRUPT)
    files = write_logs(steady_updates(20), shard(), 1, 1024)
    m = bytearray(files[0])
    m[po.tan_read(files[0])[1][0] + HDR + 12] ^= 0x10
    cases["bit_flip"] = ([bytes(m)] + files[1:], CORRUPT)
    ups = steady_updates(6)
    del ups[3]
    cases["gap"] = (write_logs(ups, shard(), 1), GAP)
    cases["wrong_replica"] = (write_logs(steady_updates(6), shard(), 2),
                              MISMATCH)
    cc = po.ent(term=2, index=3, type=1, cmd=b"\x08\x00\x10\x04")
    ups = steady_updates(2) + [((2, 1, 3), [cc])]
    cases["config_change"] = (write_logs(ups, shard(), 1), ENTRY_TYPE)
    ups = steady_updates(2) + [((2, 1, 3),
                                [kv_ent(3, 2, b"big", b"z" * CMD_CAP)])]
    cases["cmd_above_cap"] = (write_logs(ups, shard(), 1), CAPACITY)
    # A tail of W or more uncommitted entries that an overwrite cuts off
    # again: entries 65.. took the window slots of 1.. on their way, so the
    # commit of 1..12 that follows cannot be applied from the window
    cases["long_tail_overwritten"] = (
        write_logs(tail_overwritten_updates(100), shard(), 1), CAPACITY)
    # the same with a tail the window holds
    cases["short_tail_overwritten"] = (
        write_logs(tail_overwritten_updates(40), shard(), 1), OK)
    cases["no_file"] = ([], EMPTY)
    return cases


def replay_model(files, base=0):
    """The log and the KV a replica's clean files leave: the overwrite rule
    and the committed entries applied in order, in plain Python.  Returns
    (state, {index: entry dict}, kv dict, applied count)."""
    from tests.test_oracle_tan import _decode_update
    log, state = {}, None
    for f in files:
        for _, payload in po.tan_read(f):
            _, _, st, ents = _decode_update(payload)
            if ents:
                for i in [i for i in log if i >= ents[0]["index"]]:
                    del log[i]
                for e in ents:
                    if e["index"] > base:
                        log[e["index"]] = e
            if st is not None:
                state = st
    kv, n = {}, 0
    for i in range(base + 1, state[2] + 1):
        e = log[i]
        if e["cmd"]:
            k, v = po.pbkv_unmarshal(po.get_payload(e["type"], e["cmd"]))
            kv[k] = v
            n += 1
    return state, log, kv, n
