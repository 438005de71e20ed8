#!/usr/bin/env python3
"""Times drb_recover_tan at C3's and C5's shapes (not a test, not part of
bench.py).

An engine of G groups x 3 replicas writes its own tan logs: --entries rounds
of one seeded KV proposal per group with encode_saves, every round's records
copied out of the device's save buffer (drb_tan_buffers) and appended to
per-replica log images on the host, as a NodeHost's pwrite loop would.  A
fresh engine of the same configuration is then recovered from the images,
--repeats times (a new engine each), with DRB_RECOVER_TIMING=1: the library
reports the device-event times of the upload, of pass 1 (validation,
checksums) and of pass 2 (placement, apply).  One JSON line per shape: log
bytes, entries, the three times of every repeat, their medians and spreads
(max - min), GB/s of each phase and entries applied per second of pass 2.

The upload of the same bytes is the floor.  The CPU side of the comparison
is the library's host reader (drb_tan_scan, one thread) over a sample of the
logs, labelled host_scan: the oracle has no replay entry point to time.

--mux adds the multiplexed format: the same workload written by a
tan_multiplexed engine (one file per log: 16 logs a replica slot, each
round's staged bytes of a log appended to its image), recovered with
drb_recover_tan_mux after the regular recovery of the same shape, so that
both are timed in one call.  Its JSON line (format "mux") has the upload,
the block index (pass A and the composition), the scan with the one D2H of
the record count, the partition (pass B and the sort), pass 1 and pass 2,
the record-table bytes and the device bytes the call held.

  python tools/measure_recover.py [--groups N] [--entries K]
                                  [--shapes c3,c5] [--repeats N] [--mux]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dragonboat_amd import abi  # noqa: E402
from dragonboat_amd import engine as en  # noqa: E402
from dragonboat_amd.engine import Engine  # noqa: E402

SEED = 0x5EEDD8B0
SHAPES = {  # val_len, cmd_cap, kv_val_cap, kv_slots, save_cap
    "c3": dict(val_len=4, cmd_cap=32, kv_val_cap=4, kv_slots=512,
               save_cap=512),
    "c5": dict(val_len=1011, cmd_cap=1040, kv_val_cap=1024, kv_slots=64,
               save_cap=3584),
}


def d2h(hip, dst, src, n):
    rc = hip.hipMemcpy(dst.ctypes.data_as(C.c_void_p), C.c_void_p(src),
                       C.c_size_t(n), 2)  # hipMemcpyDeviceToHost
    if rc:
        raise RuntimeError("hipMemcpy failed: %d" % rc)


def write_logs(G, shape, entries, hip):
    """(cfg, per-replica lengths [3G], bytes of every log back to back in
    replica order slot * G + g)."""
    cfg = dict(num_groups=G, num_replicas=3, window=max(64, entries * 2),
               cmd_cap=shape["cmd_cap"], max_props=1, prop_slots=2,
               ri_slots=1, mailbox=8, kv_slots=shape["kv_slots"],
               kv_val_cap=shape["kv_val_cap"], save_cap=shape["save_cap"],
               save_tan=1)
    w = cfg["window"]
    cfg["window"] = 1 << (w - 1).bit_length()
    eng = Engine(**cfg)
    eng.init_steady(term=2, leader_slot=0, seed=SEED)
    bytes_p, recs_p = C.c_void_p(), C.c_void_p()
    en._ck(en.lib().drb_tan_buffers(eng.h, C.byref(bytes_p), C.byref(recs_p)),
           "drb_tan_buffers")
    N, cap = 3 * G, shape["save_cap"]
    save = np.empty((N, cap), dtype=np.uint8)
    recs = np.empty((N, 4), dtype=np.uint32)
    pieces, lens = [], []
    col = np.arange(cap, dtype=np.uint32)[None, :]
    for r in range(entries + 2):  # two more rounds: the followers catch up
        k = 1 if r < entries else 0
        if k:
            eng.gen_kv_proposals(0, 1, 256, shape["val_len"], SEED, r)
        out = eng.step(tick=(r % 2 == 0), prop_slot=0 if k else abi.DRB_NONE,
                       encode_saves=True)
        if out.fallbacks or out.errors:
            raise RuntimeError("round %d: %s" % (r, out.to_dict()))
        d2h(hip, save, bytes_p.value, N * cap)
        d2h(hip, recs, recs_p.value, N * 16)
        ln = np.where(recs[:, 3] & abi.TAN_WRITTEN, recs[:, 2], 0)
        pieces.append(save[col < ln[:, None]])  # replica-major, in order
        lens.append(ln.astype(np.int64))
    eng.close()
    lens = np.stack(lens)                       # [rounds, N]
    total = lens.sum(axis=0)
    start = np.concatenate(([0], np.cumsum(total)))[:-1]
    blob = np.empty(int(total.sum()), dtype=np.uint8)
    cur = start.copy()
    for ln, pc in zip(lens, pieces):
        first = np.repeat(cur, ln)
        within = np.arange(pc.size) - np.repeat(np.cumsum(ln) - ln, ln)
        blob[first + within] = pc
        cur += ln
    return cfg, start, total, blob


def recover(cfg, G, start, total, blob, base):
    """One recovery into a fresh engine: (times dict, statuses summary)."""
    N = 3 * G
    table = (abi.TanFile * N)()
    for q in range(N):
        table[q] = abi.TanFile(q % G, q // G, 0, int(start[q]), int(total[q]))
    eng = Engine(**cfg)
    rin = abi.RecoverIn(0, G, blob.ctypes.data_as(C.c_void_p), blob.size,
                        table, N, base, 2, SEED)
    st = (abi.RecoverStatus * N)()
    # the library's timing line goes to stderr: read it back from a file
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        try:
            t0 = time.perf_counter()
            en._ck(en.lib().drb_recover_tan(eng.h, C.byref(rin), st),
                   "drb_recover_tan")
            wall = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        text = tf.read().decode()
    m = re.search(r"upload_ms=([\d.]+) check_ms=([\d.]+) place_ms=([\d.]+)",
                  text)
    if not m:
        raise RuntimeError("no timing line: %r" % text[-200:])
    words = np.frombuffer(st, dtype=np.uint64).reshape(N, 9)
    bad = int(((words[:, 0] & 0xffffffff) != abi.REC_OK).sum())
    ents = int(words[:, 3].sum())
    applied = int((words[:, 8] - base).sum())
    eng.close()
    return dict(upload_ms=float(m.group(1)), check_ms=float(m.group(2)),
                place_ms=float(m.group(3)), wall_ms=wall * 1e3), bad, ents, \
        applied


def _timed_call(fn):
    """Runs fn with the library's stderr captured: (text, wall seconds)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        try:
            t0 = time.perf_counter()
            fn()
            wall = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        return tf.read().decode(), wall


def write_mux_logs(G, shape, entries):
    """(cfg, {(slot, key): bytes}) of a multiplexed engine's logs."""
    cfg = dict(num_groups=G, num_replicas=3, window=max(64, entries * 2),
               cmd_cap=shape["cmd_cap"], max_props=1, prop_slots=2,
               ri_slots=1, mailbox=8, kv_slots=shape["kv_slots"],
               kv_val_cap=shape["kv_val_cap"], save_cap=shape["save_cap"],
               save_tan=1, tan_multiplexed=1, tan_max_log=1 << 40)
    w = cfg["window"]
    cfg["window"] = 1 << (w - 1).bit_length()
    eng = Engine(**cfg)
    eng.init_steady(term=2, leader_slot=0, seed=SEED)
    logs = {(s, c): bytearray() for s in range(3) for c in range(16)}
    for r in range(entries + 2):
        k = 1 if r < entries else 0
        if k:
            eng.gen_kv_proposals(0, 1, 256, shape["val_len"], SEED, r)
        out = eng.step(tick=(r % 2 == 0), prop_slot=0 if k else abi.DRB_NONE,
                       encode_saves=True)
        if out.fallbacks or out.errors:
            raise RuntimeError("round %d: %s" % (r, out.to_dict()))
        for key, img in logs.items():
            lg, data = eng.export_tan_log(*key)
            if lg["start_log"] or lg["end_log"] or \
                    lg["start_offset"] != len(img):
                raise RuntimeError("log %s: %s" % (key, lg))
            img += data
    eng.close()
    return cfg, {k: v for k, v in logs.items() if v}


MUX_TIMES = ("upload_ms", "index_ms", "scan_ms", "partition_ms", "check_ms",
             "place_ms")


def recover_mux(cfg, G, blob, table, base):
    """One multiplexed recovery into a fresh engine."""
    N = 3 * G
    eng = Engine(**cfg)
    rin = abi.RecoverMuxIn(blob.ctypes.data_as(C.c_void_p), blob.size, table,
                           len(table), base, 2, SEED)
    st = (abi.RecoverStatus * N)()
    lst = (abi.RecoverLogStatus * 48)()
    text, wall = _timed_call(lambda: en._ck(
        en.lib().drb_recover_tan_mux(eng.h, C.byref(rin), st, lst),
        "drb_recover_tan_mux"))
    t = {}
    for k in MUX_TIMES + ("records", "blocks", "table_bytes", "temp_bytes"):
        m = re.search(r"%s=([\d.]+)" % k, text)
        if not m:
            raise RuntimeError("no timing line: %r" % text[-300:])
        t[k] = float(m.group(1))
    t["wall_ms"] = wall * 1e3
    words = np.frombuffer(st, dtype=np.uint64).reshape(N, 9)
    bad = int(((words[:, 0] & 0xffffffff) != abi.REC_OK).sum())
    bad += sum(l.status != abi.REC_OK for l in lst)
    ents = int(words[:, 3].sum())
    applied = int((words[:, 8] - base).sum())
    eng.close()
    return t, bad, ents, applied


def measure_mux(name, shape, G, entries, repeats):
    cfg, logs = write_mux_logs(G, shape, entries)
    table = (abi.TanMuxFile * len(logs))()
    blob = np.empty(sum(len(v) for v in logs.values()), dtype=np.uint8)
    off = 0
    for i, ((s, c), img) in enumerate(sorted(logs.items())):
        table[i] = abi.TanMuxFile(s, c, 0, 0, off, len(img))
        blob[off:off + len(img)] = np.frombuffer(img, dtype=np.uint8)
        off += len(img)
    del logs
    runs = []
    for _ in range(repeats):
        t, bad, ents, applied = recover_mux(cfg, G, blob, table, 4)
        if bad:
            raise RuntimeError("%s mux: %d not recovered" % (name, bad))
        runs.append(t)
    line = dict(shape=name, format="mux", groups=G, replicas=3, rounds=entries,
                logs=len(table), log_bytes=int(blob.size), entries=ents,
                applied=applied, records=int(runs[0]["records"]),
                blocks=int(runs[0]["blocks"]),
                table_bytes=int(runs[0]["table_bytes"]),
                device_bytes=int(runs[0]["temp_bytes"]))
    for k in MUX_TIMES + ("wall_ms",):
        v = sorted(r[k] for r in runs)
        line[k] = dict(runs=[round(r[k], 3) for r in runs],
                       median=round(v[len(v) // 2], 3),
                       spread=round(v[-1] - v[0], 3))
    line["index_and_partition_over_upload"] = round(
        (line["index_ms"]["median"] + line["scan_ms"]["median"] +
         line["partition_ms"]["median"]) / line["upload_ms"]["median"], 3)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mux", action="store_true")
    ap.add_argument("--groups", type=int, default=262144)
    ap.add_argument("--entries", type=int, default=64)
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    os.environ["DRB_RECOVER_TIMING"] = "1"
    en.lib()
    hip = C.CDLL("libamdhip64.so")
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        # (C5's 1 KB entries: an eighth of the groups keeps the host's copy
        # of the logs within a few GB)
        G = args.groups if name == "c3" else max(256, args.groups // 8)
        cfg, start, total, blob = write_logs(G, shape, args.entries, hip)
        runs = []
        for _ in range(args.repeats):
            t, bad, ents, applied = recover(cfg, G, start, total, blob, 4)
            if bad:
                raise RuntimeError("%s: %d replicas not recovered" % (name,
                                                                      bad))
            runs.append(t)
        # the host reader over a sample of the logs, one thread
        sample = range(0, 3 * G, max(1, 3 * G // 2048))
        t0 = time.perf_counter()
        sb = 0
        for q in sample:
            f = blob[int(start[q]):int(start[q] + total[q])].tobytes()
            oc, vend, recs = en.tan_scan(f, cap=1)
            assert oc == abi.TAN_EOF and vend == len(f)
            sb += len(f)
        scan_s = time.perf_counter() - t0
        line = dict(shape=name, groups=G, replicas=3, rounds=args.entries,
                    log_bytes=int(blob.size), entries=int(ents),
                    applied=int(applied),
                    host_scan_gbps=round(sb / scan_s / 1e9, 3))
        for k in ("upload_ms", "check_ms", "place_ms", "wall_ms"):
            v = sorted(r[k] for r in runs)
            line[k] = dict(runs=[round(r[k], 3) for r in runs],
                           median=round(v[len(v) // 2], 3),
                           spread=round(v[-1] - v[0], 3))
            if k != "wall_ms":
                line[k]["gbps"] = round(
                    blob.size / (v[len(v) // 2] * 1e-3) / 1e9, 2)
        line["applied_per_s"] = round(
            applied / (line["place_ms"]["median"] * 1e-3))
        print(json.dumps(line), flush=True)
        if args.mux:
            del blob
            measure_mux(name, shape, G, args.entries, args.repeats)


if __name__ == "__main__":
    main()
