"""GPU: Snappy-compressed EncodedEntries (Config.EntryCompressionType =
Snappy, drb_config.entry_compression = 1) applied on the device, against the
oracle, whose GetPayload decompresses them on the CPU.

The host encodes (rsm.GetEncoded): here tests/snappy_blocks.py builds the
blocks, and every Cmd is first asserted against the oracle's decoder.  The
engine carries the Cmd as the opaque bytes it is -- ring, mailboxes, saves --
and only the apply looks inside (drb_snappy.hpp, apply_entry).
"""
import ctypes as C
import struct

import pytest

from dragonboat_amd import abi, workload
from dragonboat_amd.engine import DrbError, Engine
from oracle import pyoracle as po
from tests import snappy_blocks as sb
from tests.gpu_harness import Pair, state_diff
from tests.test_gpu_fallback import (_flagged, _ingest, _stage_engine_only,
                                     _unhost)
from tests.test_gpu_tan import _check_round

pytestmark = pytest.mark.gpu

FB = abi.FB


def key8(i):
    return struct.pack("<Q", i)


def snappy_kv(key, val, blk=None):
    """(type, Cmd) of PBKV{key, val} as a Snappy EncodedEntry; blk: the
    block to use in place of the greedy one."""
    payload = po.pbkv_marshal(key, val)
    return abi.ENTRY_ENCODED, sb.checked(blk or sb.compress(payload), payload)


def plain_kv(key, val):
    return abi.ENTRY_ENCODED, b"\x00" + po.pbkv_marshal(key, val)


def make_batch(G, k, rows, seed=0):
    """rows: {g: [(type, client_id, Cmd)]} in workload.build_batch's layout
    (ents [g][k])."""
    counts = (C.c_uint32 * G)()
    ents = (abi.Entry * (G * k))()
    pool = bytearray()
    for g, es in rows.items():
        assert len(es) <= k
        counts[g] = len(es)
        for j, (typ, cid, cmd) in enumerate(es):
            ekey = workload.mix64(seed * 1000003 + g * 16 + j) | 1
            ents[g * k + j] = abi.Entry(0, 0, ekey, cid, 0, 0, typ, len(cmd),
                                        len(pool))
            pool += cmd
    pbuf = (C.c_uint8 * max(1, len(pool))).from_buffer_copy(bytes(pool) or
                                                           b"\0")
    return counts, ents, pbuf


def cid(g):
    return workload.client_id(0x5EEDD8B0, g)


def _ok(p, o, e, r):
    assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
    assert (e.committed_entries, e.applied_entries, e.messages) == \
        (o.committed_entries, o.applied_entries, o.messages), \
        (r, e.to_dict(), o.to_dict())


def _kv_equal(p, r, cap=32):
    okv = {}
    for g in range(p.G):
        for s in range(p.R):
            okv[g, s] = p.orc.export_kv(g, s, key_cap=16, val_cap=1024,
                                        cap=cap)
            assert p.eng.kv_export(g, s) == okv[g, s], (r, g, s)
    return okv


def _all_applied(p, more_than):
    for g in range(p.G):
        st = p.orc.export(g, 0)
        assert st.sm_index == st.committed > more_than, g


# ------------------------------------------------------------ 1: one wave
def _mixed_entry(g, r, j):
    """Entry j of group g in round r: header 0x00, Snappy literal-only,
    Snappy with a copy inside an 8-byte repeated key, an empty no-op --
    neighbouring lanes take different branches."""
    n = (r * 96 + g) * 3 + j
    kind = (g + j + r + (workload.mix64(g) & 1)) % 4
    val = struct.pack("<I", workload.mix64(n) & 0xffffffff)
    if kind == 0:
        return plain_kv(key8(n % 5), val) + (kind,)
    if kind == 1:
        payload = po.pbkv_marshal(key8(n % 5), val)
        blk = sb.block(len(payload), sb.literal(payload))
        return snappy_kv(key8(n % 5), val, blk) + (kind,)
    if kind == 2:
        b = 1 + n % 250
        key = bytes([b]) * 8
        blk = sb.block(16, sb.literal(b"\x0a\x08" + bytes([b])),
                       sb.copy1(1, 7), sb.literal(b"\x12\x04" + val))
        return snappy_kv(key, val, blk) + (kind,)
    return abi.ENTRY_APPLICATION, b"", kind


def test_mixed_headers_in_one_wave():
    """G = 96 (a full wave and a partial one), k = 3: uncompressed, Snappy
    literal-only, Snappy with a copy, and empty no-op entries interleaved
    across the lanes of a wave and inside one group's batch, with ticks and
    ReadIndex.  No fallback, parity every round.  (Without
    entry_compression every Snappy proposal falls back before the append.)"""
    G = 96
    p = Pair(G=G, R=3, cmd_cap=32, kv_val_cap=4, entry_compression=1)
    kinds = {}
    for r in range(6):
        rows = {}
        for g in range(G):
            rows[g] = []
            for j in range(3):
                typ, cmd, kind = _mixed_entry(g, r, j)
                rows[g].append((typ, cid(g) if kind != 3 else 0, cmd))
                kinds.setdefault(kind, set()).add(g // 64)
        o, e = p.round(batch=make_batch(G, 3, rows, r), tick=(r % 2 == 0),
                       read_index=(r % 3 == 0))
        _ok(p, o, e, r)
        errs = p.check()
        assert not errs, (r, errs[:2])
    assert all(kinds[k] == {0, 1} for k in range(4)), kinds
    _all_applied(p, 12)


# ------------------------------------------------------- 2: inline values
def test_inline_long_values_and_scratch_reuse():
    """kv_val_cap = 64 (inline slots), cmd_cap = 96: values whose blocks
    use copy1 and copy2; in every group and round a 64 B value is followed
    by a 3 B value for the same key, then a 61 B one for another -- the
    decoded row is reused entry after entry, and no byte of the longer
    payload may reach the slot."""
    G = 16
    p = Pair(G=G, R=3, cmd_cap=96, kv_val_cap=64, kv_slots=16,
             entry_compression=1)
    for r in range(5):
        rows = {}
        for g in range(G):
            pat8 = struct.pack("<Q", workload.mix64(r * G + g) |
                               0x0101010101010101)
            k1, k2 = key8((g + r) % 3), key8(3 + (g + r) % 2)
            v64 = pat8 * 8
            pay = po.pbkv_marshal(k1, v64)
            head = len(pay) - 64
            blk64 = sb.block(len(pay), sb.literal(pay[:head + 8]),
                             sb.copy2(8, 56))
            pat5 = pat8[:5]
            v61 = (pat5 * 13)[:61]
            pay = po.pbkv_marshal(k2, v61)
            head = len(pay) - 61
            # 5 literal bytes of the value, 5 x 11 by copy1, the last by copy2
            blk61 = sb.block(len(pay), sb.literal(pay[:head + 5]),
                             *[sb.copy1(5, 11)] * 5, sb.copy2(5, 1))
            rows[g] = [(t, cid(g), c) for (t, c) in (
                snappy_kv(k1, v64, blk64), snappy_kv(k1, pat8[:3]),
                snappy_kv(k2, v61, blk61))]
        o, e = p.round(batch=make_batch(G, 3, rows, r), tick=(r % 2 == 1))
        _ok(p, o, e, r)
        errs = p.check(kv=False)
        assert not errs, (r, errs[:2])
        okv = _kv_equal(p, r)
    assert all(len(okv[g, 0][key8((g + 4) % 3)]) == 3 for g in range(G))
    _all_applied(p, 10)


# ------------------------------------------- 3: decoded longer than cmd_cap
def _long_value(n, kind):
    """1000 B runs; period-7 patterns of 900 B (a 1000 B one does not fit a
    64 B Cmd: tests/snappy_blocks.py valid_vectors)."""
    x = workload.mix64(n)
    if kind == 0:
        return bytes([1 + x % 255]) * 1000
    pat = struct.pack("<Q", x | 0x0101010101010101)[:7]
    return (pat * 129)[:900]


@pytest.mark.parametrize("mode", ["insert", "overwrite"])
@pytest.mark.parametrize("ovf", [0, 1])
def test_decoded_payload_longer_than_cmd_cap(mode, ovf):
    """cmd_cap = 64, kv_val_cap = 1024 (out-of-line values): every Cmd is
    at most 64 B and decodes to a PBKV of 913-1013 B.  insert: every entry
    writes a key of its own; overwrite: two keys per group rewritten every
    round with the other kind of value (another length).  ovf: kv_slots = 4
    with overflow buckets, so that apply_entry's overflow-chain branch reads
    the decoded row too.  ReadIndex with 2 reads per ctx every round: the
    served values come back whole."""
    G, K = 16, 2
    kw = dict(kv_slots=4, kv_overflow_buckets=128) if ovf else \
        dict(kv_slots=16)
    p = Pair(G=G, R=3, cmd_cap=64, kv_val_cap=1024, kv_pool_blocks=1024,
             max_reads_per_ctx=2, entry_compression=1, **kw)
    seen, reads = {}, 0
    for r in range(4):
        rows = {}
        for g in range(G):
            rows[g] = []
            for j in range(K):
                ki = (r * K + j) % 8 if mode == "insert" else j
                val = _long_value((r * G + g) * K + j, (r + j + g) % 2)
                typ, cmd = snappy_kv(key8(ki), val)
                assert len(cmd) <= 64 < len(val)
                seen.setdefault((g, ki), []).append(len(val))
                rows[g].append((typ, cid(g), cmd))
        o, e = p.round(batch=make_batch(G, K, rows, r), tick=(r % 2 == 0),
                       read_index=True, reads=2, read_key_space=8)
        _ok(p, o, e, r)
        errs = p.check(kv=False)
        assert not errs, (r, errs[:2])
        okv = _kv_equal(p, r)
        for (g, index, low, j, key, found, val) in \
                p.eng.export_read_values(0, pool_cap=1 << 16):
            assert val == okv[g, 0].get(key8(key)), (r, g, j, key)
            reads += found
    if mode == "insert":
        assert all(len(v) == 1 for v in seen.values()) and len(seen) == 8 * G
    else:
        assert all(len(v) == 4 and len(set(v)) == 2 for v in seen.values())
    assert reads > 8, reads
    _all_applied(p, 6)


# ------------------------------------------------------- 4: the other ways
def _small_rows(G, r, k=2):
    rows = {}
    for g in range(G):
        rows[g] = []
        for j in range(k):
            n = (r * G + g) * k + j
            val = struct.pack("<I", workload.mix64(n) & 0xffffffff)
            if (g + j + r) % 3 == 0:
                typ, cmd = plain_kv(key8(n % 6), val)
            else:
                b = 1 + n % 200
                typ, cmd = snappy_kv(bytes([b]) * 8, val)
            rows[g].append((typ, cid(g), cmd))
    return rows


def test_forwarded_snappy_proposals():
    """forward_proposals: the entry queue is at replica 2, a follower; its
    Propose carries the Snappy entries by value to the leader."""
    G = 16
    p = Pair(G=G, R=3, forward_proposals=1, max_props=2, mailbox=16,
             entry_compression=1)
    for r in range(8):
        o, e = p.round(batch=make_batch(G, 2, _small_rows(G, r), r),
                       tick=(r % 2 == 0), prop_replica=2)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), (r, e.to_dict(), o.to_dict())
        errs = p.check()
        assert not errs, (r, errs[:2])
    _all_applied(p, 10)


def test_ingested_replicates_carry_snappy_entries():
    """The leader (slot 2) lives on another NodeHost: its Replicates arrive
    through drb_ingest, and the hosted followers apply what that leader's
    host compressed."""
    G = 8
    p = Pair(G=G, R=3, leader_slot=2, entry_compression=1)
    for r in range(3):
        o, e = p.round(k=1, tick=False)
        assert e.fallbacks == 0 and e.errors == 0
    _unhost(p, range(G), 2)
    o, e = p.round(k=0, tick=False)  # what the leader sent last is handled
    assert not p.check()
    want = {}
    for step in range(3):
        msgs = []
        for g in range(G):
            for to in (1, 2):
                st = p.orc.export(g, to - 1)
                ents = []
                if step < 2:
                    b = 1 + (g * 4 + step) % 200
                    val = struct.pack("<I", workload.mix64(g * 8 + step)
                                      & 0xffffffff)
                    typ, cmd = snappy_kv(bytes([b]) * 8, val)
                    want[g, step] = (bytes([b]) * 8, val)
                    ents = [po.ent(term=2, index=st.last_index + 1, type=typ,
                                   key=77 + step, client_id=cid(g), cmd=cmd)]
                msgs.append(po.msg(abi.MSG["Replicate"], from_=3, to=to,
                                   term=2, log_index=st.last_index,
                                   log_term=2, commit=st.last_index,
                                   entries=ents, shard_id=1 + g))
        _ingest(p, msgs)
        o, e = p.round(k=0, tick=False)
        assert e.fallbacks == 0 and e.errors == 0, (step, p.why())
        errs = p.check()
        assert not errs, (step, errs[:2])
    for g in range(G):
        for s in (0, 1):
            st = p.eng.export_replicas(g, 1)[s]
            assert st.sm_index == st.last_index == st.committed, (g, s)
            kv = p.eng.kv_export(g, s)
            for step in range(2):
                k, v = want[g, step]
                assert kv[k] == v, (g, s, step)


def test_raft_launch_applies_snappy_entries():
    """elections: the leaders of some groups stop, their followers elect on
    the GPU (the raft launch), and Snappy proposals keep arriving
    throughout: whichever launch steps a replica applies them."""
    G = 16
    p = Pair(G=G, R=3, elections=1, max_props=2, entry_compression=1)
    slow = 0
    E = [1, 6, 11]
    for r in range(70):
        if r == 3:
            _unhost(p, E, 0)
        o, e = p.round(batch=make_batch(G, 2, _small_rows(G, r), r),
                       tick=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), (r, e.to_dict(), o.to_dict())
        errs = p.check()
        assert not errs, (r, errs[:2])
        slow += e.elections_stepped
        if r > 3 and all(
                abi.LEADER in [x.role for x in
                               p.eng.export_replicas(g, 1)[1:]] for g in E):
            break
    else:
        raise AssertionError("no new leaders")
    assert slow > 0
    before = {g: p.orc.export(g, 1).sm_index for g in E}
    for r in range(70, 76):  # writes under the new leaders
        o, e = p.round(batch=make_batch(G, 2, _small_rows(G, r), r),
                       tick=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
        errs = p.check()
        assert not errs, (r, errs[:2])
    for g in E:
        assert p.eng.export_replicas(g, 1)[1].sm_index > before[g] + 4


def test_apply_results_carry_the_decoded_length():
    """drb_apply_results: KVTest's Result.Value is the length of the
    payload it was handed (kvtest.go:161) -- of a Snappy entry, the decoded
    one."""
    G = 8
    p = Pair(G=G, R=3, cmd_cap=64, kv_val_cap=1024, kv_slots=16,
             kv_pool_blocks=256, max_props=2, entry_compression=1)
    seen = set()
    for r in range(4):
        prev = {(g, s): p.orc.export(g, s).sm_index
                for g in range(G) for s in range(3)}
        rows = _small_rows(G, r)
        for g in range(0, G, 2):
            typ, cmd = snappy_kv(key8(g), _long_value(r * G + g, r % 2))
            rows[g][1] = (typ, cid(g), cmd)
        o, e = p.round(batch=make_batch(G, 2, rows, r), tick=(r % 2 == 0))
        _ok(p, o, e, r)
        for s in range(3):
            exp = []
            for g in range(G):
                now = p.orc.export(g, s).sm_index
                for t in p.orc.export_log(g, s, prev[g, s] + 1, now):
                    term, index, typ, key, c, sid, _, cmd = t
                    val = len(po.get_payload(typ, cmd)) if c else 0
                    exp.append((g, index, key, c, sid, val, int(c == 0)))
                    seen.add(val)
            assert p.eng.apply_results(s) == exp, (r, s)
        assert not p.check(kv=False)
    assert {16, 913, 1013} <= seen, seen


@pytest.mark.parametrize("tan", [0, 1])
def test_saves_hold_the_compressed_cmd(tan):
    """encode_saves: the EntryBatch (or tan record) of the round's
    EntriesToSave equals the oracle's, and the Cmd in it is the compressed
    one."""
    G = 16
    kw = dict(save_tan=1) if tan else {}
    p = Pair(G=G, R=3, cmd_cap=64, kv_val_cap=1024, kv_pool_blocks=512,
             kv_slots=16, save_cap=4096, entry_compression=1, **kw)
    dbs = [[po.TanDB() for _ in range(p.R)] for _ in range(p.G)]
    logs = {}
    for r in range(5):
        rows = {}
        cmds = {}
        for g in range(G):
            typ, cmd = snappy_kv(key8(g % 4), _long_value(r * G + g, r % 2))
            rows[g] = [(typ, cid(g), cmd)]
            cmds[g] = cmd
        o, e = p.round(batch=make_batch(G, 1, rows, r), tick=(r % 2 == 0),
                       encode_saves=True)
        _ok(p, o, e, r)
        errs = p.check(kv=False)
        assert not errs, (r, errs[:2])
        _kv_equal(p, r)
        if tan:
            assert _check_round(p, dbs, logs, r) > 0
            for g in range(G):
                assert cmds[g] in p.eng.export_tan(g, 0)[1], (r, g)
        else:
            assert not p.check_saves(), r
            for g in range(G):
                eb, _ = p.eng.export_saved(g, 0)
                assert cmds[g] in eb and len(eb) < 200, (r, g, len(eb))


# ------------------------------------------------------- 5: corrupt blocks
@pytest.mark.parametrize("which", ["offset_0", "offset_beyond_produced",
                                   "declared_above_capacity",
                                   "literal_past_input"])
def test_corrupt_block_stops_the_apply(which):
    """A block the CPU decoder test rejects (tests/test_snappy_host.py),
    staged on the engine alone -- the oracle would panic: the leader appends
    and replicates it (the Cmd is opaque to raft), the entry commits, and
    every replica's apply stops at it with the KV as it was."""
    blk = dict(sb.malformed_vectors())[which]
    with pytest.raises(po.OracleError):
        po.get_payload(abi.ENTRY_ENCODED, sb.cmd(blk))
    G, bad = 8, 3
    p = Pair(G=G, R=3, prop_slots=2, entry_compression=1)
    for r in range(3):
        o, e = p.round(batch=make_batch(G, 1, _small_rows(G, r, 1), r),
                       tick=False)
        assert e.fallbacks == 0 and e.errors == 0
    for r in range(6):  # until every replica applied what was proposed
        o, e = p.round(k=0, tick=True)
        assert not p.check()
        sts = p.eng.export_replicas(bad, 1)
        if all(st.sm_index == st.last_index for st in sts):
            break
    kv0 = [p.eng.kv_export(bad, s) for s in range(3)]
    assert all(kv0)
    pre = p.eng.export_replicas(bad, 1)
    index = pre[0].last_index + 1
    assert all(st.sm_index == index - 1 for st in pre)
    _stage_engine_only(p, {bad: [po.ent(type=abi.ENTRY_ENCODED, key=99,
                                        client_id=cid(bad),
                                        cmd=sb.cmd(blk))]})
    others = [g for g in range(G) if g != bad]
    stopped = {}
    for r in range(6):
        p.orc.round(tick=True)
        e = p.eng.step(tick=True, prop_slot=1 if r == 0 else abi.DRB_NONE)
        p.rounds += 1
        assert e.errors == 0, (r, p.why())
        for (g, s), (reason, flags) in _flagged(p).items():
            assert g == bad and reason == FB["ENTRY_TYPE"], (g, s, reason)
            assert flags & abi.F_APPLY_STOPPED and flags & abi.F_FALLBACK
            stopped[s] = r
        errs = p.check(groups=others)
        assert not errs, (r, errs[:2])
        if len(stopped) == 3:
            break
    assert sorted(stopped) == [0, 1, 2], stopped
    sts = p.eng.export_replicas(bad, 1)
    for s, st in enumerate(sts):
        assert st.flags & abi.F_APPLY_STOPPED
        assert st.fallback_reason == FB["ENTRY_TYPE"]
        assert st.sm_index == index - 1 and st.last_index == index, (s, index)
        assert st.committed == index
        assert not set(state_diff(st, pre[s], 3)) & {"sm_index", "sm_term",
                                                     "kv_count"}
        assert p.eng.kv_export(bad, s) == kv0[s], s


# ---------------------------------------------------------- 6: default off
def test_default_engine_still_falls_back():
    """entry_compression = 0: the same proposal that applies above makes the
    leader fall back before it appends; values other than 0 and 1 are
    refused at create."""
    p = Pair(G=8, R=3, prop_slots=2)
    for r in range(2):
        p.round(k=1, tick=False)
    typ, cmd = snappy_kv(b"k" * 8, b"vvvv")
    _stage_engine_only(p, {3: [po.ent(type=typ, client_id=77, cmd=cmd)]})
    p.orc.round(tick=False)
    out = p.eng.step(tick=False, prop_slot=1)
    p.rounds += 1
    assert _flagged(p) == {(3, 0): (FB["ENTRY_TYPE"], abi.F_FALLBACK | 1)}
    assert out.fallbacks == 1
    assert not p.check(groups=[g for g in range(8) if g != 3])
    with pytest.raises(DrbError):
        Engine(num_groups=8, num_replicas=3, entry_compression=2)
