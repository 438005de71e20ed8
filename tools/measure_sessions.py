#!/usr/bin/env python3
"""Times the device-side session path at C5's shape (not a test, not part of
bench.py).

C5 (bench.py --workload c5) at 128 B: 4M groups x 3 replicas,
window 8, Quiesce, listed rounds, EntryBatch saves, a tick every round, 1 %
of the groups proposing one entry per round.  Three engines step the same
seeded proposals (Cmd = 0x00 || PBKV{LE64 key < 256, a 116 B value}):

  a  session_slots = 0 (the parent's configuration), NoOP-session proposals
  b  session_slots = S, session_history = H, the same NoOP-session proposals:
     what the option costs a client that does not use it
  c  the same engine; every group's client registers in round 0 and proposes
     with an advancing SeriesID and RespondedTo = SeriesID - 1 (the client
     has seen every earlier response): lookup, clearTo, history store

All three stage through drb_stage_proposals (the packed form carries no
SeriesID), outside the timed span.  Per repeat the engines are built, warmed
(--warm rounds, past the Quiesce threshold), timed with device events around
each round, and destroyed in turn -- a, b, c, a, b, c, ... -- so that drift
shows in the spread.  One JSON line: ms/round of each repeat, their median
and spread (max - min), drb_engine_device_bytes, committed entries.

  python tools/measure_sessions.py [--groups N] [--slots S] [--history H]
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

VLEN = 116  # bench.py's C5 value at 128 B
C5_SLOTS, C5_KEYS, C5_OVF_PER = 32, 256, 1 / 64
SEED = 0x5EEDD8B0
ENTRY = np.dtype([("term", "<u8"), ("index", "<u8"), ("key", "<u8"),
                  ("client_id", "<u8"), ("series_id", "<u8"),
                  ("responded_to", "<u8"), ("type", "<u4"), ("cmd_len", "<u4"),
                  ("cmd_off", "<u8")])
assert ENTRY.itemsize == C.sizeof(abi.Entry)
HDR = b"\x00\x0a\x08" + bytes(8) + b"\x12" + bytes([VLEN])
CLEN = len(HDR) + VLEN


def draw(G, ppm, rnd):
    """The round's proposing groups, their keys and value patterns."""
    rng = np.random.default_rng(SEED + rnd)
    n = int(rng.binomial(G, ppm / 1e6))
    idx = np.unique(rng.integers(0, G, n, dtype=np.int64))
    n = idx.size
    keys = rng.integers(0, C5_KEYS, n, dtype=np.uint64)
    pats = rng.integers(1, 256, (n, 8), dtype=np.uint8)
    return idx, keys, pats


def cmds(keys, pats):
    n = keys.size
    out = np.zeros((n, CLEN), dtype=np.uint8)
    out[:, :len(HDR)] = np.frombuffer(HDR, dtype=np.uint8)
    out[:, 3:11] = keys.view(np.uint8).reshape(n, 8)
    out[:, len(HDR):] = np.tile(pats, (1, (VLEN + 7) // 8))[:, :VLEN]
    return out


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def run(G, form, rounds, args, torch):
    cmd_cap = (CLEN + 15) // 16 * 16
    bound = 73 + cmd_cap
    total = args.warm + args.warmup + args.steps
    mean = G * 3 * args.active_ppm / 1e6 * total
    sess = dict(session_slots=args.slots, session_history=args.history) \
        if form != "a" else {}
    eng = Engine(num_groups=G, num_replicas=3, window=8, cmd_cap=cmd_cap,
                 max_props=1, prop_slots=2, ri_slots=1, mailbox=8,
                 kv_slots=C5_SLOTS, kv_val_cap=VLEN + 13 & ~15,
                 kv_pool_blocks=int(mean + 8 * mean ** 0.5) + 3 * 65536,
                 kv_overflow_buckets=int(G * 3 * C5_OVF_PER) + 1024,
                 save_cap=(4 * bound + 15) // 16 * 16, quiesce=1, **sess)
    eng.init_steady(term=2, leader_slot=0, seed=SEED)
    stream = torch.cuda.ExternalStream(eng.stream)
    counts = np.zeros(G, dtype=np.uint32)
    ents = np.zeros(G, dtype=ENTRY)
    clients = np.arange(G, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    series = np.zeros(G, dtype=np.uint64)
    ents["client_id"] = clients
    ents["type"] = abi.ENTRY_ENCODED
    one = np.zeros(1, dtype=np.uint8)
    ev = []
    for i, (idx, keys, pats) in enumerate(rounds):
        counts[:] = 0
        if form == "c" and i == 0:  # every group's client registers
            counts[:] = 1
            ents["key"] = clients
            ents["series_id"] = np.uint64(abi.SERIES_REGISTER)
            ents["type"] = abi.ENTRY_APPLICATION
            ents["cmd_len"] = 0
            pool = one
        else:
            counts[idx] = 1
            ents["key"][idx] = (idx.astype(np.uint64) * np.uint64(2654435761)
                                + np.uint64(i)) | np.uint64(1)
            if form == "c":
                series[idx] += np.uint64(1)
                ents["series_id"][idx] = series[idx]
                ents["responded_to"][idx] = series[idx] - np.uint64(1)
            ents["type"][idx] = abi.ENTRY_ENCODED
            ents["cmd_len"][idx] = CLEN
            ents["cmd_off"][idx] = np.arange(idx.size, dtype=np.uint64) * \
                np.uint64(CLEN)
            pool = np.ascontiguousarray(cmds(keys, pats)).reshape(-1)
            if pool.size == 0:
                pool = one
        eng.stage_proposals(i % 2, ptr(counts, C.c_uint32),
                            ptr(ents, abi.Entry), ptr(pool, C.c_uint8),
                            pool.size)
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
        raise RuntimeError("%s: fallbacks %d errors %d" % (
            form, out.fallbacks, out.errors))
    res = dict(ms=sum(a.elapsed_time(b) for a, b in ev) / len(ev),
               device_bytes=eng.device_bytes,
               committed=int(out.committed_entries),
               applied=int(out.applied_entries))
    if form == "c":  # the sessions did what the timing claims
        g = int(np.argmax(series))
        (cid, upto, hist), = eng.sessions_export(g, 0)
        assert cid == int(clients[g]) and upto >= int(series[g]) - 2, \
            (cid, upto, hist, int(series[g]))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4 << 20)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--history", type=int, default=2)
    ap.add_argument("--active-ppm", type=int, default=10000)
    ap.add_argument("--warm", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    G = args.groups
    rounds = [draw(G, args.active_ppm, i)
              for i in range(args.warm + args.warmup + args.steps)]
    runs = {f: [] for f in "abc"}
    for _ in range(args.repeats):
        for f in "abc":
            runs[f].append(run(G, f, rounds, args, torch))
            print("%s: %.4f ms/round" % (f, runs[f][-1]["ms"]),
                  file=sys.stderr, flush=True)
    line = dict(payload=128, groups=G, replicas=3, slots=args.slots,
                history=args.history, active_ppm=args.active_ppm,
                steps=args.steps, warm=args.warm + args.warmup)
    for f in "abc":
        ms = sorted(r["ms"] for r in runs[f])
        line[f] = dict(ms_per_round=[round(r["ms"], 4) for r in runs[f]],
                       median_ms=round(ms[len(ms) // 2], 4),
                       spread_ms=round(ms[-1] - ms[0], 4),
                       device_bytes=runs[f][0]["device_bytes"],
                       committed=runs[f][0]["committed"],
                       applied=runs[f][0]["applied"])
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
