"""GPU: the engine's grow-only buffers and its teardown (drb_res.hpp).

Every device buffer that grows on demand has one owner; a growth frees the
old allocation and makes a new one.  For each such buffer with a public
path, engine A makes a small call, a large call (the buffer regrows), then
the small call again; engine B, with the same seeded history, makes only
that last call.  The two results must be the same bytes: a regrown buffer
neither keeps a stale pointer or capacity nor changes what a call returns.

Then engines are created, used (every lazily built state once: the wire
encoder, the wire ingest, the step-worker export with its drain thread, the
session clients) and destroyed eight times in a row, and a ninth runs the
ordinary parity check against the oracle: the teardown joins the drain
thread, frees nothing under a running copy and leaves a fresh engine sound.

All at 300 groups x 3 replicas: one full 256-lane block and a ragged one.
No allocation failure is provoked here; tests/test_res_owner.py runs the
failure paths on the host.
"""
import ctypes as C
import random
import zlib

import pytest

from dragonboat_amd import abi, workload
from tests.gpu_harness import Pair
from tests.test_gpu_wire import SRC, TwoNodes

pytestmark = pytest.mark.gpu

G, R = 300, 3
READS, KEYS = 9, 16
SAMPLE = (0, 1, 255, 256, 299)  # both blocks' edges
# 1011-byte values (test_gpu_wire's long payloads): a proposing round's
# plane of 4 entries per group passes the wire output's 1 MiB growth step
LONG = dict(cmd_cap=1040, kv_val_cap=1024, kv_slots=64, max_props=4)
LONG_VAL = 1011
DID = 0xD1D


def _states(eng):
    return [st.to_dict(R) for st in eng.export_replicas(0, G)]


def _fingerprint(eng):
    """Every replica record, and the log tail, KV, outbox and ReadyToReads
    of the sampled groups."""
    sts = eng.export_replicas(0, G)
    out = [[st.to_dict(R) for st in sts]]
    for g in SAMPLE:
        for s in range(R):
            last = sts[g * R + s].last_index
            out.append((eng.export_log(g, s, max(1, last - 8), last),
                        eng.kv_export(g, s), eng.export_outbox(g, s),
                        eng.export_ready(g, s)))
    return out


def _pair(**kw):
    """The same seeded history on every call: writes, ticks, a ReadIndex
    round with served reads."""
    p = Pair(G=G, R=R, max_reads_per_ctx=READS, **kw)
    for r in range(3):
        o, e = p.round(k=1, tick=(r % 2 == 0), read_index=True, reads=READS,
                       read_key_space=KEYS, key_space=KEYS)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict())
    return p


def _both(small_then_large, last):
    """last(p) on engine A after small_then_large(p), and on engine B."""
    a = _pair()
    small_then_large(a)
    got_a = last(a)
    a.eng.close()
    b = _pair()
    got_b = last(b)
    b.eng.close()
    return got_a, got_b


def test_scratch_regrowth_keeps_results():
    """drb_export_replicas over 1 group and over all of them; the scratch
    buffer starts at 1 MiB, so a CRC batch of 1.5 MiB is what regrows it."""
    rnd = random.Random(0x5C7A)
    blobs = [rnd.randbytes(512 << 10) for _ in range(3)]
    assert sum(map(len, blobs)) > 1 << 20  # past the scratch buffer's floor

    def pre(p):
        one = p.eng.export_replicas(0, 1)
        every = p.eng.export_replicas(0, G)
        assert [s.to_dict(R) for s in one] == \
            [s.to_dict(R) for s in every[:R]]
        assert p.eng.crc32_batch(blobs) == [zlib.crc32(x) for x in blobs]
        assert _states(p.eng) == [s.to_dict(R) for s in every]

    def last(p):
        return [s.to_dict(R) for s in p.eng.export_replicas(0, 1)], \
            _states(p.eng)

    got_a, got_b = _both(pre, last)
    assert got_a == got_b


def test_stage_buffer_regrowth_keeps_results():
    """drb_stage_proposals with 1 entry and with max_props entries per
    group, then the round's batch: the round that reads the slot sees only
    the last batch."""
    def pre(p):
        mp = p.eng.cfg["max_props"]
        pools = []
        for k, salt in ((1, 1000), (mp, 1001)):
            counts, ents, pool = workload.build_batch(G, k, p.seed, salt,
                                                      KEYS, 4)
            pools.append(C.sizeof(pool))
            eents = (abi.Entry * (G * mp))()
            for g in range(G):
                for j in range(k):
                    eents[g * mp + j] = ents[g * k + j]
            p.eng.stage_proposals(0, counts, eents, pool)
        # the upload is the fixed entry and count arrays plus the Cmd pool
        # (at least 16 B): only a longer pool regrows the buffer
        assert pools[1] > pools[0] >= 16, pools

    def last(p):
        o, e = p.round(k=1, tick=True, key_space=KEYS)
        assert e.fallbacks == 0 and e.errors == 0, e.to_dict()
        assert e.committed_entries == o.committed_entries
        return e.to_dict(), _fingerprint(p.eng)

    got_a, got_b = _both(pre, last)
    assert got_a == got_b


def _raw(p, fn, typ, first, n):
    arr, cnt = p.eng._batch(fn, typ, 0, first, n, 1 << 16)
    return cnt, C.string_at(arr, cnt * C.sizeof(typ))


def test_batch_export_regrowth_keeps_results():
    """The batch exports' device output: one group, every group, one
    group."""
    from dragonboat_amd.engine import lib

    def exports(p, first, n):
        return (_raw(p, lib().drb_export_ready_to_reads_batch,
                     abi.ReadyToRead, first, n),
                _raw(p, lib().drb_export_read_results, abi.ReadResult,
                     first, n),
                p.eng.export_read_values(0, first, n))

    def pre(p):
        one, every = exports(p, 255, 1), exports(p, 0, G)
        # (the output is sized by the record count: more records regrow it)
        assert every[0][0] > one[0][0] and every[1][0] > one[1][0]
        assert len(every[2]) > len(one[2])

    got_a, got_b = _both(pre, lambda p: exports(p, 255, 1))
    assert got_a == got_b
    assert got_a[0][0] >= 1  # (the compared export is not an empty one)


def test_wire_output_regrowth_keeps_results():
    """drb_encode_wire after an idle round, after a proposing round whose
    plane passes the output's growth step, and after an idle round."""
    def run(encode_all):
        p = Pair(G=G, R=R, **LONG)
        sizes = []
        for k in (0, 4, 0):
            o, e = p.round(k=k, tick=True, val_len=LONG_VAL)
            assert e.fallbacks == 0 and e.errors == 0, e.to_dict()
            if encode_all or len(sizes) == 2:
                res, data = p.eng.encode_wire(0, 1, DID, SRC)
                assert res["n_bytes"] == len(data)
            sizes.append(len(data) if encode_all else None)
        p.eng.close()
        return res, data, sizes

    res_a, data_a, sizes = run(True)
    assert sizes[1] > sizes[0] + (1 << 20) > sizes[2] > 0, sizes
    res_b, data_b, _ = run(False)
    assert res_a == res_b and data_a == data_b


def test_ingest_buffers_regrowth_keeps_results():
    """drb_ingest_wire of a short and then a long stream.  Two NodeHosts
    joined by the wire; before a round's crossing, A's leader host also
    takes the leader plane of an idle round and of a proposing round --
    every message of it is for a replica it does not host, so the streams
    are walked, CRC'd, decoded and sorted in full (every ingest buffer
    grows) and dropped at placement."""
    def run(extra):
        t = TwoNodes(G=G, R=R, did=DID, **LONG)
        planes = []
        for k in (0, 4):
            t.round(k=k, tick=True, val_len=LONG_VAL)
            planes.append(t.lead.encode_wire(0, 1, DID, SRC))
        if extra:
            for res, data in planes:
                got = t.lead.ingest_wire(data, DID)
                assert got["bad"] == 0 and got["consumed"] == len(data), got
                assert got["messages"] == res["n_msgs"] > 0, got
                assert got["accepted"] == 0, got
                assert got["dropped"] == res["n_msgs"], got
        outs = []
        for r in range(2):  # (the second consumes what the first delivered)
            o, a, b = t.round(k=r, tick=True, val_len=LONG_VAL)
            outs.append((a.to_dict(), b.to_dict()))
        fp = _fingerprint(t.lead), _fingerprint(t.foll)
        sizes = [len(d) for _r, d in planes]
        t.lead.close()
        t.foll.close()
        return outs, fp, sizes

    outs_a, fp_a, sizes = run(True)
    assert sizes[1] > (1 << 20) > sizes[0] > 0, sizes
    outs_b, fp_b, _ = run(False)
    assert outs_a == outs_b
    assert fp_a == fp_b


def _worker_export(p, caps):
    b = p.eng.worker_bufs(*caps)
    try:
        p.eng.worker_export(0, b)
        nr, nv, nd = p.eng.worker_wait(b)
        return (nr, nv, nd, C.string_at(b.lanes, 4 * G),
                C.string_at(b.reads, 4 * nr), C.string_at(b.values, 4 * nv),
                C.string_at(b.value_meta, (nv + 3) // 4),
                C.string_at(b.deferred, 8 * nd))
    finally:
        p.eng.free_worker_bufs(b)


def test_worker_staging_regrowth_keeps_results():
    """drb_worker_export with small and then larger capacities."""
    small = (2 * G, 2 * G * READS, 2 * G)
    large = (16 * G, 16 * G * READS, 16 * G)
    # (each staging buffer is sized by its capacity: 4 or 8 B per element)
    assert all(x > y > 0 for x, y in zip(large, small))

    def pre(p):
        assert _worker_export(p, small) == _worker_export(p, large)

    got_a, got_b = _both(pre, lambda p: _worker_export(p, small))
    assert got_a == got_b
    assert got_a[0] > 0 and got_a[1] + got_a[2] > 0, got_a[:3]


def test_create_use_destroy_repeated():
    """Eight engines in a row, each stepped 4 rounds, with every lazy state
    built once, then destroyed; a ninth is bit-exact with the oracle."""
    caps = (2 * G, 2 * G * READS, 2 * G)
    for i in range(8):
        p = Pair(G=G, R=R, max_reads_per_ctx=READS)
        for r in range(4):
            o, e = p.round(k=1, tick=(r % 2 == 0), read_index=True,
                           reads=READS, read_key_space=KEYS, key_space=KEYS)
            assert e.fallbacks == 0 and e.errors == 0, (i, r, e.to_dict())
        res, data = p.eng.encode_wire(0, 1, DID, SRC)
        assert res["n_msgs"] > 0 and len(data) == res["n_bytes"]
        # (co-resident replicas: the plane is walked and decoded, not placed)
        got = p.eng.ingest_wire(data, DID)
        assert got["bad"] == 0 and got["messages"] == res["n_msgs"], got
        out = _worker_export(p, caps)
        assert out[0] > 0, out[:3]
        p.eng.set_session_clients([workload.client_id(p.seed, g)
                                   for g in range(G)])
        p.eng.close()
    p = Pair(G=G, R=R)
    for r in range(8):
        o, e = p.round(k=1 + r % 2, tick=(r % 2 == 0),
                       read_index=(r % 3 == 1))
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), r
    errs = p.check()
    assert not errs, errs[:2]
    p.eng.close()
