#!/usr/bin/env python3
"""Times the device-side Snappy apply at C5's shape (not a test, not part
of bench.py).

C5 (bench.py --workload c5): 4M groups x 3 replicas, window 8,
Quiesce, listed rounds, EntryBatch saves, a tick every round, 1 % of the
groups proposing one 128 B / 1 KB entry per round.  Three engines step the
same seeded decoded payloads (PBKV{LE64 key < 256, value = a seeded 8-byte
pattern repeated}: compressible, unlike bench.py's random values):

  a  entry_compression = 0, Cmd = 0x00 || payload, C5's cmd_cap
  b  entry_compression = 1, Cmd = 0x02 || Snappy block, the same cmd_cap
  c  entry_compression = 1, cmd_cap cut to what the blocks need

Per repeat the engines are built, warmed (--warm rounds, past the Quiesce
threshold), timed with device events around each round, and destroyed in
turn -- a, b, c, a, b, c, ... -- so that drift shows in the spread.  One
JSON line per payload: ms/round of each repeat, their median and spread
(max - min), drb_engine_device_bytes, committed entries.

  python tools/measure_snappy.py [--groups N] [--payloads 128,1024]
                                 [--warm W] [--warmup U] [--steps K]
                                 [--repeats N]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dragonboat_amd import abi  # noqa: E402
from dragonboat_amd.engine import Engine  # noqa: E402

C5_VAL = {128: 116, 1024: 1011}  # bench.py
C5_SLOTS, C5_KEYS, C5_OVF_PER = 32, 256, 1 / 64
SEED = 0x5EEDD8B0


def uvarint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7f) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def draw(G, ppm, rnd):
    """The round's proposing groups, their keys and value patterns."""
    rng = np.random.default_rng(SEED + rnd)
    n = int(rng.binomial(G, ppm / 1e6))
    idx = np.unique(rng.integers(0, G, n, dtype=np.int64))
    n = idx.size
    keys = rng.integers(0, C5_KEYS, n, dtype=np.uint64)
    pats = rng.integers(1, 256, (n, 8), dtype=np.uint8)
    return idx, keys, pats


def cmds(keys, pats, vlen, snappy):
    """[n, L] uint8: every entry's Cmd (one length per payload and form)."""
    n = keys.size
    hdr = b"\x0a\x08" + bytes(8) + b"\x12" + uvarint(vlen)
    plen = len(hdr) + vlen
    if not snappy:
        out = np.zeros((n, 1 + plen), dtype=np.uint8)
        out[:, 1:1 + len(hdr)] = np.frombuffer(hdr, dtype=np.uint8)
        out[:, 3:11] = keys.view(np.uint8).reshape(n, 8)
        reps = (vlen + 7) // 8
        out[:, 1 + len(hdr):] = np.tile(pats, (1, reps))[:, :vlen]
        return out
    # 0x02, uvarint(plen), literal(header + the first period), copies of
    # offset 8 and up to 64 bytes each
    lit = len(hdr) + 8
    assert lit <= 60
    head = b"\x02" + uvarint(plen) + bytes([(lit - 1) << 2])
    rest, tail = vlen - 8, bytearray()
    while rest:
        k = min(64, rest)
        tail += bytes([2 | ((k - 1) << 2), 8, 0])
        rest -= k
    out = np.zeros((n, len(head) + lit + len(tail)), dtype=np.uint8)
    out[:, :len(head)] = np.frombuffer(head, dtype=np.uint8)
    o = len(head)
    out[:, o:o + len(hdr)] = np.frombuffer(hdr, dtype=np.uint8)
    out[:, o + 2:o + 10] = keys.view(np.uint8).reshape(n, 8)
    out[:, o + len(hdr):o + lit] = pats
    out[:, o + lit:] = np.frombuffer(bytes(tail), dtype=np.uint8)
    return out


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def stage(eng, slot, G, idx, ekeys, clients, cmd):
    counts = np.zeros(G, dtype=np.uint8)
    counts[idx] = 1
    n = idx.size
    lens = np.full(max(1, n), cmd.shape[1], dtype=np.uint16)
    pool = np.ascontiguousarray(cmd).reshape(-1)
    if n == 0:
        pool = np.zeros(1, dtype=np.uint8)
    eng.stage_proposals_packed(slot, abi.ENTRY_ENCODED, ptr(counts, C.c_uint8),
                               n, ptr(ekeys, C.c_uint64),
                               ptr(clients, C.c_uint64),
                               ptr(lens, C.c_uint16), ptr(pool, C.c_uint8),
                               n * cmd.shape[1])


def run(G, payload, form, rounds, args, torch):
    vlen = C5_VAL[payload]
    plain_cap = ((12 + (1 if vlen < 128 else 2) + vlen) + 15) // 16 * 16
    one = np.zeros(1, dtype=np.uint64)
    snap_len = cmds(one, np.ones((1, 8), np.uint8), vlen, True).shape[1]
    cmd_cap = (snap_len + 15) // 16 * 16 if form == "c" else plain_cap
    bound = 73 + cmd_cap
    total = args.warm + args.warmup + args.steps
    mean = G * 3 * args.active_ppm / 1e6 * total
    eng = Engine(num_groups=G, num_replicas=3, window=8, cmd_cap=cmd_cap,
                 max_props=1, prop_slots=2, ri_slots=1, mailbox=8,
                 kv_slots=C5_SLOTS, kv_val_cap=vlen + 13 & ~15,
                 kv_pool_blocks=int(mean + 8 * mean ** 0.5) + 3 * 65536,
                 kv_overflow_buckets=int(G * 3 * C5_OVF_PER) + 1024,
                 save_cap=(4 * bound + 15) // 16 * 16, quiesce=1,
                 entry_compression=int(form != "a"))
    eng.init_steady(term=2, leader_slot=0, seed=SEED)
    stream = torch.cuda.ExternalStream(eng.stream)
    ev = []
    for i, (idx, keys, pats) in enumerate(rounds):
        ekeys = (idx.astype(np.uint64) * np.uint64(2654435761) +
                 np.uint64(i)) | np.uint64(1)
        clients = idx.astype(np.uint64) * np.uint64(2) + np.uint64(1)
        stage(eng, i % 2, G, idx, ekeys, clients,
              cmds(keys, pats, vlen, form != "a"))
        timed = i >= args.warm + args.warmup
        if timed:
            a, b = (torch.cuda.Event(enable_timing=True),
                    torch.cuda.Event(enable_timing=True))
            a.record(stream)
        eng.step_async(tick=True, prop_slot=i % 2, encode_saves=True,
                       listed=True)
        if timed:
            b.record(stream)
            ev.append((a, b))
        if i % 64 == 63 or i + 1 == args.warm + args.warmup:
            eng.sync()
            if i + 1 == args.warm + args.warmup:
                eng.read_counters(reset=True)
    eng.sync()
    torch.cuda.synchronize()
    out = eng.read_counters(reset=True)
    if out.fallbacks or out.errors:
        raise RuntimeError("%s/%d: fallbacks %d errors %d" % (
            form, payload, out.fallbacks, out.errors))
    res = dict(ms=sum(a.elapsed_time(b) for a, b in ev) / len(ev),
               device_bytes=eng.device_bytes, cmd_cap=cmd_cap,
               cmd_len=snap_len if form != "a" else 13 + len(uvarint(vlen)) +
               vlen, committed=int(out.committed_entries),
               applied=int(out.applied_entries))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4 << 20)
    ap.add_argument("--payloads", default="128,1024")
    ap.add_argument("--active-ppm", type=int, default=10000)
    ap.add_argument("--warm", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    G = args.groups
    for payload in [int(x) for x in args.payloads.split(",")]:
        rounds = [draw(G, args.active_ppm, i)
                  for i in range(args.warm + args.warmup + args.steps)]
        runs = {f: [] for f in "abc"}
        for _ in range(args.repeats):
            for f in "abc":
                runs[f].append(run(G, payload, f, rounds, args, torch))
        line = dict(payload=payload, groups=G, replicas=3,
                    active_ppm=args.active_ppm, steps=args.steps,
                    warm=args.warm + args.warmup)
        for f in "abc":
            ms = sorted(r["ms"] for r in runs[f])
            line[f] = dict(ms_per_round=[round(r["ms"], 4) for r in runs[f]],
                           median_ms=round(ms[len(ms) // 2], 4),
                           spread_ms=round(ms[-1] - ms[0], 4),
                           device_bytes=runs[f][0]["device_bytes"],
                           cmd_cap=runs[f][0]["cmd_cap"],
                           cmd_len=runs[f][0]["cmd_len"],
                           committed=runs[f][0]["committed"],
                           applied=runs[f][0]["applied"])
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
