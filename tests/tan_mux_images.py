"""Images of multiplexed tan logs for tests/test_tanmux_host.py (CPU) and
tests/test_gpu_recover_mux.py (device): one oracle db (po.TanDB) written for
several shards in turn is the shared db of CreateLogMultiplexedTan -- the
nodes of a log interleaved record by record, nodeStates kept per node.
"""
from oracle import pyoracle as po
from tests import tan_images as ti

KEYS = 16
VAL_1K = bytes(range(256)) * 4


def interleave(lists):
    """{shard: [(state, entries)]} -> [(shard, state, entries)], one record
    of each shard in turn."""
    out, k = [], 0
    while any(k < len(u) for u in lists.values()):
        for shard, ups in lists.items():
            if k < len(ups):
                out.append((shard,) + tuple(ups[k]))
        k += 1
    return out


def write_shared(items, replica, max_log=0):
    """The files of one shared db after db.write of each (shard, state,
    entries) for `replica`: [bytes per log number]."""
    db = po.TanDB(max_log)
    for shard, state, ents in items:
        db.write(shard, replica, state, ents)
    return [db.file(lg) for lg in range(db.last()["log"] + 1)]


def shared_logs(lists, replica, max_log=0):
    """{key: files} of the shared dbs the shards of `lists` write."""
    keys = {}
    for shard, ups in lists.items():
        keys.setdefault(shard % KEYS, {})[shard] = ups
    return {key: write_shared(interleave(ls), replica, max_log)
            for key, ls in keys.items()}


def big_files(replica=1):
    """Shards 5, 21 and 37 (key 5) with 1 KiB values in 64 KiB logs: files
    above 64 KiB with records across block boundaries."""
    lists = {s: ti.steady_updates(30, val=VAL_1K, first=1) for s in (5, 21, 37)}
    return write_shared(interleave(lists), replica, 1 << 16)


def small_shared(replica=2):
    """One shared log of about 1 KB: three shards, entries, State-only
    records and records without State."""
    lists = {}
    for n, shard in enumerate((5, 21, 37)):
        ups = []
        for i in range(1, 5):
            ups.append(((2, 1, i - 1),
                        [ti.kv_ent(i, 2, b"k%d" % i, b"v%02d" % (i + n))]))
            if i % 2 == 0:
                ups.append(((2, 1, i), []))
        ups.append((None, []))
        lists[shard] = ups
    files = write_shared(interleave(lists), replica)
    assert len(files) == 1
    return files[0]


def equivalence_lists(first_shard=5):
    """The update lists of the demultiplexing tests, each with a shard of
    its own of one key: {shard: updates}."""
    lists = [ti.overwrite_updates(), ti.steady_updates(40)]
    lists += [ti.tail_overwritten_updates(n) for n in (40, ti.W - 1, ti.W,
                                                       100)]
    lists.append([((2, 1, 0), []), ((2, 1, 0), []), ((3, 0, 0), []),
                  (None, [])])          # State only
    return {first_shard + KEYS * i: ups for i, ups in enumerate(lists)}


def mux_command(slot, first_shard, groups, base, cmd_cap, W, snappy, logs):
    """The program's mux command for logs {key: files}."""
    words = ["mux", slot, first_shard, groups, base, cmd_cap, W, snappy]
    for key, files in sorted(logs.items()):
        words += [key, len(files)] + [f.hex() or "-" for f in files]
    return " ".join(str(w) for w in words)


def parse_mux(line):
    """({key: (status, log, offset, records)}, {g: (plan, log, applied)})
    of the program's mux line."""
    head, reps = line.split("@")
    logs = {}
    for t in head.split():
        key, status, lg, off, n = (int(x) for x in t.split(","))
        logs[key] = (status, lg, off, n)
    out = {}
    for r in (reps.split(";") if reps else []):
        g, rest = r.split("~")
        plan, log, app = rest.split("|")
        plan = dict(zip(("status", "files", "offset", "records", "entries",
                         "term", "vote", "commit", "last_index", "applied"),
                        [int(x) for x in plan.split()]))
        lg = {}
        for e in (log.split(",") if log else []):
            i, t, c = e.split("/")
            lg[int(i)] = (int(t), b"" if c == "-" else bytes.fromhex(c))
        ap = [tuple(int(x) for x in a.split("/"))
              for a in (app.split(",") if app else [])]
        out[int(g)] = (plan, lg, ap)
    return logs, out


# cases of ti.recover_cases() that are a replica's own (the others damage
# bytes of a file or its ids: in a shared log they refuse the log)
REPLICA_CASES = ("clean", "overwrite", "gap", "config_change",
                 "cmd_above_cap", "long_tail_overwritten",
                 "short_tail_overwritten", "no_file")


def replica_case_lists(first_shard=1):
    """({shard: updates}, {shard: (name, status)}): the records of each
    replica-level case of ti.recover_cases(), decoded from its files, for a
    shard of its own of key first_shard % 16."""
    from tests.test_oracle_tan import _decode_update
    cases = ti.recover_cases()
    lists, want = {}, {}
    for n, name in enumerate(REPLICA_CASES):
        files, status = cases[name]
        ups = []
        for f in files:
            for _, payload in po.tan_read(f):
                _, _, state, ents = _decode_update(payload)
                ups.append((state, ents))
        shard = first_shard + KEYS * n
        lists[shard] = ups
        want[shard] = (name, status)
    return lists, want
