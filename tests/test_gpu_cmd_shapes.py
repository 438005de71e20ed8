"""GPU: ragged Cmd shapes through the apply path and the encoders.

The seeded workload's Cmds are all 0x00 || PBKV{8-byte key, value} with one
length per run, so a Cmd's length mod 16 (the ring stores Cmds in 16 B
chunks, ByteOut flushes every 16 B) and the value's offset in the Cmd (the
byte shift of value_chunk / extract16 / mask16) see one or two values.
Here a local builder makes PBKV Cmds of every key length 0..8, values from
empty to kv_val_cap, both field orders, encoded and plain application
entries, with Entry.Key and ClientID at their varint widths, different
lengths inside one round and one group's batch, and 8 keys per group so a
key is rewritten long -> short -> empty -> long (stale tail bytes of a
slot or value block would show).  Everything is compared with the oracle.
"""
import ctypes as C
import struct

import pytest

from dragonboat_amd import abi, workload
from dragonboat_amd.engine import DrbError
from oracle import pyoracle as po
from tests.gpu_harness import Pair, state_diff
from tests.test_gpu_fallback import _flagged, _settle_and_return
from tests.test_gpu_tan import _check_round
from tests.test_gpu_wire import _check_planes

pytestmark = pytest.mark.gpu

G = 16
# Entry.Key: the colfer varint at 1, 2, 3 and 7 bytes, 2^49 - 1 (last
# varint) against 2^49 (first 9-byte form), and a seeded odd 64-bit value
EKEYS = [1, 127, 128, 16383, 16384, (1 << 42) + 5, (1 << 49) - 1, 1 << 49]
CIDS = [1, 127, 128, (1 << 49) - 1, 1 << 49, 0xC0FFEE1234567891]


def kv_cmd(key, val, key_first=True, encoded=True):
    """(entry type, Cmd) of PBKV{key, val}: ENTRY_ENCODED carries the v0
    header byte 0x00, ENTRY_APPLICATION the bare payload."""
    kf = b"\x0a" + workload.varint(len(key)) + key
    vf = b"\x12" + workload.varint(len(val)) + val
    body = kf + vf if key_first else vf + kf
    if encoded:
        return abi.ENTRY_ENCODED, b"\x00" + body
    return abi.ENTRY_APPLICATION, body


def key_bytes(i, klen):
    """Key i of a group's 8: LE64(i) at 8 bytes (what the served reads look
    up), else klen non-zero bytes."""
    return struct.pack("<Q", i) if klen == 8 else bytes([i + 1]) * klen


def value_bytes(n, vlen):
    out, x = b"", workload.mix64(n + 1)
    while len(out) < vlen:
        out += struct.pack("<Q", x | 0x0101010101010101)  # no zero bytes
        x = workload.mix64(x)
    return out[:vlen]


def value_offset(key, val, key_first, encoded):
    hv = 2 if len(val) < 128 else 3
    return int(encoded) + (2 + len(key) if key_first else 0) + hv


def value_first_ok(key, val, encoded):
    """Both headers inside the device's parse window: the Cmd's first 64
    bytes (drb_step.hpp apply_entry reads a header as up to 3 bytes)."""
    start = int(encoded) + (2 if len(val) < 128 else 3) + len(val)
    return start + 3 <= 64 and start + 2 + len(key) <= 64


# name: engine config, value range, key lengths of the 8 keys, (klen, vlen,
# key_first, encoded) shapes every run must contain
CONFIGS = {
    "nonext": dict(kw=dict(cmd_cap=64, kv_val_cap=48), v=(0, 48),
                   klens=[0, 1, 2, 3, 4, 5, 6, 7, 8], enc_saves=False,
                   must=[(8, 48, True, True), (0, 48, False, False),
                         (8, 0, False, True), (0, 0, True, False),
                         (8, 48, False, False)]),
    "inline": dict(kw=dict(cmd_cap=144, kv_val_cap=124), v=(0, 124),
                   klens=[0, 1, 5, 8], enc_saves=True,
                   must=[(8, 123, True, True), (8, 124, True, True),
                         (8, 114, True, True),    # cmd_len 127
                         (8, 115, True, True),    # cmd_len 128
                         (0, 124, True, False), (5, 40, False, True)]),
    "ool": dict(kw=dict(cmd_cap=144, kv_val_cap=256), v=(0, 130),
                klens=[0, 1, 5, 8], enc_saves=True,
                must=[(8, 130, True, True),       # cmd_len == cmd_cap
                      (8, 127, True, True), (8, 128, True, True),
                      (0, 127, True, False), (0, 128, True, False),
                      (1, 129, True, True), (1, 50, False, True)]),
    "1k": dict(kw=dict(cmd_cap=1040, kv_val_cap=1024), v=(1008, 1024),
               klens=[0, 1, 5, 8], enc_saves=True,
               must=[(8, 1024, True, True), (0, 1024, True, False),
                     (8, 1008, True, True)]),
}


def build_round(cfg, r, all_encoded=False):
    """One round's batch in workload.build_batch's layout, k = 3 columns:
    group g proposes 1 + (r + g) % 3 entries.  Returns (counts, ents, pool,
    shapes) with shapes = [(g, key index, klen, vlen, key_first, encoded,
    cmd_len, value offset)]."""
    lo, hi = cfg["v"]
    span = hi - lo + 1
    klens, must = cfg["klens"], cfg["must"]
    counts = (C.c_uint32 * G)()
    ents = (abi.Entry * (G * 3))()
    pool = bytearray()
    shapes = []
    for g in range(G):
        counts[g] = 1 + (r + g) % 3
        for j in range(counts[g]):
            n = (r * G + g) * 3 + j
            ki = (r + 3 * j + g) % 8
            klen = klens[(ki + g) % len(klens)]
            if j == 0:
                vlen = lo + (16 * r + g) % span
            elif j == 1:  # long -> short -> empty -> long on one key
                vlen = (hi, lo + 3, lo, hi - 1, lo + 16, lo, hi - 7,
                        lo + 1)[(r // 4 + g) % 8]
                ki = g % 8
                klen = klens[(ki + g) % len(klens)]
            else:
                vlen = hi - (7 * r + g) % span
            key_first = (r + g + j) % 3 != 0
            encoded = all_encoded or (r + g // 2 + j) % 4 != 0
            i = r * G + g
            if j == 0 and r >= 1 and i - G < len(must):
                klen, vlen, key_first, encoded = must[i - G]
                encoded = encoded or all_encoded
                ki = next(q for q in range(len(klens))
                          if klens[(q + g) % len(klens)] == klen)
            key, val = key_bytes(ki, klen), value_bytes(n, vlen)
            if not key_first and not value_first_ok(key, val, encoded):
                key_first = True
            typ, cmd = kv_cmd(key, val, key_first, encoded)
            assert len(cmd) <= cfg["kw"]["cmd_cap"]
            ekey = EKEYS[n % 9] if n % 9 < 8 else workload.mix64(n) | 1
            ents[g * 3 + j] = abi.Entry(0, 0, ekey, CIDS[(g + r // 4) % 6], 0,
                                        0, typ, len(cmd), len(pool))
            pool += cmd
            shapes.append((g, ki, klen, vlen, key_first, encoded, len(cmd),
                           value_offset(key, val, key_first, encoded)))
    pbuf = (C.c_uint8 * max(1, len(pool))).from_buffer_copy(bytes(pool))
    return counts, ents, pbuf, shapes


def reachable_offsets(cfg, all_encoded=False):
    """Every value offset mod 16 the configuration's shapes can take."""
    lo, hi = cfg["v"]
    out = set()
    for enc in ((1,) if all_encoded else (0, 1)):
        for hv in {2 if lo < 128 else 3, 2 if hi < 128 else 3}:
            for kl in cfg["klens"]:
                out.add((enc + 2 + kl + hv) % 16)
        if lo < 62:  # value first: a short value, then the key's header
            out.add(enc + 2)
    return out


def _long_short_empty_long(hist, long_from):
    """Some key's write history holds long, shorter, empty, long again."""
    for seq in hist.values():
        st = 0
        for v in seq:
            if st == 0 and v >= long_from:
                st = 1
            elif st == 1 and 0 < v < long_from:
                st = 2
            elif st == 2 and v == 0:
                st = 3
            elif st == 3 and v >= long_from:
                return True
    return False


ROUNDS = 18


@pytest.mark.parametrize("name,tan,packed", [
    ("nonext", 0, False), ("inline", 0, False), ("inline", 1, False),
    ("inline", 0, True), ("ool", 0, False), ("ool", 1, False),
    ("1k", 0, False), ("1k", 1, False)])
def test_ragged_lengths(name, tan, packed):
    """G=16, 1-3 proposals a group a round with different lengths, 18
    rounds.  Input conditions (asserted; the oracle applies every entry):
    every cmd_len % 16, every value offset the configuration can reach,
    the listed boundary shapes (value == kv_val_cap, cmd_len == cmd_cap,
    the 127 / 128 Cmd- and value-length varint boundaries), and a key
    rewritten long -> short -> empty -> long.  fallbacks == 0 and full
    parity every round; on the EXT configurations also the EntryBatch saves
    (or tan records), the Replicate plane (0,1) and whole served-read
    values.  packed: staged through drb_stage_proposals_packed (u16
    lengths, one entry type).  GPU time measured: 0.4-0.9 s a case."""
    cfg = CONFIGS[name]
    ext = cfg["enc_saves"]
    kw = dict(cfg["kw"], kv_slots=64, max_props=4)
    if ext:
        kw.update(save_cap=16384, max_reads_per_ctx=9)
    if tan:
        kw.update(save_tan=1)
    p = Pair(G=G, R=3, **kw)
    dbs = [[po.TanDB() for _ in range(p.R)] for _ in range(p.G)]
    logs = {}
    res, offs, lens, hist = set(), set(), set(), {}
    reads = 0
    for r in range(ROUNDS):
        counts, ents, pool, shapes = build_round(cfg, r, all_encoded=packed)
        for (g, ki, klen, vlen, kf, enc, clen, voff) in shapes:
            res.add(clen % 16)
            offs.add(voff % 16)
            lens.add(clen)
            hist.setdefault((g, ki, klen), []).append(vlen - cfg["v"][0])
        tick, ri = r % 2 == 0, ext and r % 2 == 1
        if packed:
            p.orc.stage_proposals(counts, 3, ents, pool)
            p.eng.stage_proposals_packed(
                0, abi.ENTRY_ENCODED,
                *workload.pack_batch(G, 3, counts, ents, pool))
            pin, _ = p.stage(k=0, read_index=ri)
            o = p.orc.round(tick=tick)
            e = p.eng.step(tick=tick, prop_slot=0,
                           ri_slot=0 if ri else abi.DRB_NONE, reads_per_ctx=9,
                           key_space=8, encode_saves=True)
            p.rounds += 1
        else:
            o, e = p.round(batch=(counts, ents, pool), tick=tick,
                           read_index=ri, reads=9 if ext else 0,
                           read_key_space=8, encode_saves=ext)
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        assert (e.committed_entries, e.applied_entries, e.messages) == \
            (o.committed_entries, o.applied_entries, o.messages), \
            (r, e.to_dict(), o.to_dict())
        errs = p.check(kv=False)
        assert not errs, (r, errs[:2])
        okv = {}
        for g in range(G):
            for s in range(3):
                okv[g, s] = p.orc.export_kv(g, s, key_cap=16, val_cap=1024,
                                            cap=16)
                assert p.eng.kv_export(g, s) == okv[g, s], (r, g, s)
        if not ext:
            continue
        if tan:
            _check_round(p, dbs, logs, r)
        else:
            assert not p.check_saves(), r
        _check_planes(p, did=0xD1D, limits=[0], planes=[(0, 1)])
        for (g, index, low, j, key, found, val) in \
                p.eng.export_read_values(0, pool_cap=64):
            want = okv[g, 0].get(struct.pack("<Q", key))
            assert val == want, (r, g, j, key)
            reads += found
    # the inputs covered what they are here for
    assert res == set(range(16)), sorted(res)
    assert offs == reachable_offsets(cfg, packed), (sorted(offs), name)
    for (klen, vlen, kf, enc) in cfg["must"]:
        assert int(enc or packed) + 2 + klen + (2 if vlen < 128 else 3) + \
            vlen in lens, (klen, vlen)
    if name == "inline":
        assert {127, 128} <= lens
    if name == "ool":
        assert 144 in lens
    assert _long_short_empty_long(hist, 16) or cfg["v"][0] > 0
    for g in range(G):  # the oracle applied every entry
        st = p.orc.export(g, 0)
        assert st.sm_index == st.committed > ROUNDS, g
    if ext:
        assert reads > 20, reads


def _bad_cmds(val_cap):
    return {
        "empty": (abi.ENTRY_APPLICATION, b""),
        "key9": kv_cmd(b"k" * 9, b"abcd"),
        "value": kv_cmd(b"kkkkkkkk", b"v" * (val_cap + 1)),
        "field3": (abi.ENTRY_ENCODED, b"\x00" + b"\x0a\x01k\x12\x01v" +
                   b"\x1a\x01z"),
    }


@pytest.mark.parametrize("which", ["empty", "key9", "value", "field3"])
def test_unappliable_cmd_stops_apply_only(which):
    """A Cmd that passes prop_fast (NoOP session, well-formed type) but
    that apply_entry cannot apply on the device -- an empty application Cmd
    with a ClientID, a 9-byte key, a value of kv_val_cap + 1, a third PBKV
    field: the raft round completes, the replicas that reach the entry
    stop applying there (DRB_F_APPLY_STOPPED | DRB_F_FALLBACK,
    DRB_FB_ENTRY_TYPE) with only sm_index / sm_term / kv_count behind the
    oracle, and after the CPU path (the oracle) settled the group and it
    is imported back it is bit-exact again, its KV holding what the oracle
    applied.  The 9-byte key and the long value are the device table's
    documented limits (include/drb_engine.h, drb_kv_import: key_lens <= 8,
    val_lens <= kv_val_cap, DRB_ERANGE otherwise): the oracle's map then
    holds a pair the table cannot, the import is refused with DRB_ERANGE
    and the group stays on the CPU path while the others go on bit-exact.
    GPU time: 1.6 s a case."""
    VC = 16
    p = Pair(G=4, R=3, cmd_cap=64, kv_val_cap=VC, max_props=4)
    for r in range(3):
        o, e = p.round(k=1, tick=(r % 2 == 0))
        assert e.fallbacks == 0 and e.errors == 0
    assert not p.check()
    typ, cmd = _bad_cmds(VC)[which]
    bad = 2
    counts = (C.c_uint32 * p.G)()
    ents = (abi.Entry * p.G)()
    counts[bad] = 1
    ents[bad] = abi.Entry(0, 0, 77, 0xC1, 0, 0, typ, len(cmd), 0)
    pool = (C.c_uint8 * max(1, len(cmd))).from_buffer_copy(cmd or b"\0")
    stopped = {}
    for r in range(8):
        snap = p.snapshot()
        if r == 0:
            o, e = p.round(batch=(counts, ents, pool), tick=False)
        else:
            o, e = p.round(k=0, tick=(r % 2 == 1))
        assert e.errors == 0, (r, p.why())
        for (g, s), (reason, flags) in _flagged(p).items():
            assert g == bad and reason == abi.FB["ENTRY_TYPE"], (g, s, reason)
            assert flags & abi.F_APPLY_STOPPED and flags & abi.F_FALLBACK
            a, b, pre = (p.eng.export_replicas(g, 1)[s], p.orc.export(g, s),
                         snap[(g, s)])
            d = state_diff(a, b, p.R)
            assert set(d) <= {"sm_index", "sm_term", "kv_count"}, d
            assert (a.sm_index, a.kv_count) == (pre.sm_index, pre.kv_count)
            assert a.pushed_index == b.pushed_index > a.sm_index
            stopped[s] = r
        errs = p.check(groups=[g for g in range(p.G) if g != bad])
        assert not errs, (r, errs[:2])
        if stopped:  # (a stopped leader sends nothing more: the others
            break    # may never learn the commit on the device)
    assert stopped, "the entry was never reached"
    # the oracle applied it
    st = p.orc.export(bad, 0)
    assert st.sm_index == st.committed
    p.to_cpu(bad)
    if which in ("key9", "value"):
        with pytest.raises(DrbError, match="drb_kv_import failed with "
                                           "status -5"):
            _settle_and_return(p, [bad])
        assert bad in p.cpu
        for r in range(3):
            o, e = p.round(k=1, tick=True)
            assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
            assert not p.check()
        return
    _settle_and_return(p, [bad])
    errs = p.check()
    assert not errs, errs[:2]
    assert p.eng.kv_export(bad, 0) == p.orc.export_kv(bad, 0)
    for r in range(3):
        o, e = p.round(k=1, tick=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        assert not p.check()
