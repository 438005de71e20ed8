"""GPU: one term that outgrows the narrow forms.

The packed replica record (drb_layout.hpp) keeps its index fields as signed
16-bit offsets from `last`; F_TERM_START -- the first index of the current
term -- escapes to the u64 overflow array once one term holds more than
32767 entries.  The colfer / varint encoders switch widths at 128 and
16384.  The runs here stay in term 2 until last_index passes those points,
against the oracle: counters every round, everything (state, logs, KV,
outboxes, ReadyToReads, persistence, wire planes) around each boundary.
"""
import zlib

import pytest

from dragonboat_amd import abi
from oracle import pyoracle as po
from tests.gpu_harness import Pair, state_diff
from tests.test_gpu_tan import _check_round
from tests.test_gpu_wire import TwoNodes, _check_planes

pytestmark = pytest.mark.gpu

BOUNDS = (128, 16384, 32768, 32768 + 4)
K = 16


def _lasts(p):
    return [p.orc.export(g, s).last_index for g in range(p.G)
            for s in range(p.R)]


def _near(lasts, bounds=BOUNDS, d=40):
    return any(abs(li - b) <= d for li in lasts for b in bounds)


class _Saves:
    """The encoded persistence of one save mode against the oracle."""

    def __init__(self, p, mode):
        self.p, self.mode = p, mode
        if mode == "batched":
            self.db = po.BatchDB()
            self.first = p.eng.cfg["first_shard_id"]
        if mode == "tan":
            self.dbs = [[po.TanDB(1 << 40) for _ in range(p.R)]
                        for _ in range(p.G)]

    def round(self, r, check):
        """After every round (the oracle's stores take every Update);
        check: compare the engine's output of this round."""
        p = self.p
        if self.mode == "crc":
            if not check:
                return
            assert not p.check_saves(), r
            for g in range(p.G):
                for s in range(p.R):
                    b, crc = p.eng.export_saved(g, s)
                    assert crc == (zlib.crc32(b) if b else 0), (r, g, s)
        elif self.mode == "batched":
            for g in range(p.G):
                for s in range(p.R):
                    ob, _ = p.orc.export_saved(g, s)
                    ents = po.entrybatch_unmarshal(ob) if ob else []
                    want = [(b, v, zlib.crc32(v)) for b, v in
                            self.db.record(self.first + g, s + 1, ents)] \
                        if ents else []
                    if check:
                        assert p.eng.export_save_records(g, s) == want, \
                            (r, g, s)
        else:
            if not check:
                for g in range(p.G):
                    for s in range(p.R):
                        p.orc.tan_write(g, s, self.dbs[g][s])
                return
            # the log images as they stood before this round's records
            logs = {}
            for g in range(p.G):
                for s in range(p.R):
                    lg = self.dbs[g][s].last()["log"]
                    logs[(g, s, lg)] = bytearray(self.dbs[g][s].file(lg))
            _check_round(p, self.dbs, logs, r)


MODES = {"crc": {}, "batched": {"save_batched": 1},
         "tan": {"save_tan": 1, "tan_max_log": 1 << 40}}


@pytest.mark.parametrize("mode", ["crc", "batched", "tan"])
def test_term_longer_than_packed_range(mode):
    """G=2, R=3, window 64, a tick every other round, k=16 proposals a
    round for 2110 rounds -- k=4 for 8440 rounds with save_batched, whose
    first record is merged with up to 47 earlier entries of its batch:
    the pre-pass wants them resident below min(committed, saved_to), which
    trails last by up to 3k, so 47 + 3k < 64 allows k <= 5 (k=16 falls
    back with DRB_FB_CAPACITY, test_batched_merge_span_wider_than_window)
    -- so last_index passes
    33 700 in term 2, so term_start leaves the packed record's 16-bit
    offset (escape code, u64 overflow array) while every other index field
    stays in range, and Index / Commit / LogIndex cross the 1 -> 2 -> 3
    byte varint widths in EntryBatch, batched-LogDB and tan records and on
    the wire planes.  Counters every round; full state + persistence +
    planes (0,1), (1,0) every round within +-40 of 128, 16384, 32768 and
    32768+4, state every 64th round.  GPU time measured: 2.1 s (crc), 6.4 s
    (batched, 8440 rounds), 3.2 s (tan)."""
    k = 4 if mode == "batched" else K
    p = Pair(G=2, R=3, window=64, max_props=K, save_cap=8192, **MODES[mode])
    sv = _Saves(p, mode)
    assert not _near([4])  # the start is outside every window
    windows = 0
    for r in range(33760 // k):
        o, e = p.round(k=k, tick=(r % 2 == 0), encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), (r, e.to_dict(), o.to_dict())
        near = _near(_lasts(p))
        sv.round(r, near)
        if near or r % (1024 // k) == 0:
            errs = p.check()
            assert not errs, (r, errs[:2])
        if near:
            windows += 1
            _check_planes(p, did=0xD1D, limits=[0], planes=[(0, 1), (1, 0)])
    errs = p.check()
    assert not errs, errs[:2]
    lasts = _lasts(p)
    assert min(lasts) > 32768 + 44 + 800, lasts
    assert all(p.orc.export(g, s).term == 2 for g in range(p.G)
               for s in range(p.R))
    assert windows >= 4 * 4, windows


def test_batched_merge_span_wider_than_window():
    """save_batched at window 64 with 16 proposals a round and a save buffer
    that would hold them: the round's first record is merged with up to 47
    earlier entries of its batch, which the pre-pass wants resident below
    min(committed, saved_to); at 16 a round the window has moved past them
    within a few rounds.  The replica then leaves the fast path before it
    mutates (DRB_FB_CAPACITY: include/drb_engine.h, save_batched "needs
    window >= 64 and save_cap for a full batch") -- the documented limit,
    not wrong records: until then every record equals the oracle's.  GPU
    time: 0.02 s."""
    p = Pair(G=2, R=3, window=64, max_props=K, save_cap=32768,
             save_batched=1)
    sv = _Saves(p, "batched")
    for r in range(8):
        snap = p.snapshot()
        o, e = p.round(k=K, tick=(r % 2 == 0), encode_saves=True)
        assert e.errors == 0, (r, p.why())
        recs, lost = p.eng.take_flagged()
        if recs:
            assert e.fallbacks == len(recs)
            for (g, s, reason, flags, _rnd, _sid) in recs:
                assert reason == abi.FB["CAPACITY"], recs
                assert flags & abi.F_FALLBACK, recs
                a = p.eng.export_replicas(g, 1)[s]
                assert not state_diff(a, snap[(g, s)], p.R), (r, g, s)
            assert r >= 2
            return
        assert e.fallbacks == 0
        sv.round(r, True)
        errs = p.check()
        assert not errs, (r, errs[:2])
    raise AssertionError("a merge span past the window was never refused")


def test_long_term_quiesce_lean_rounds():
    """The lean kernel's copy of the record store (drb_lean.hpp) with an
    escaped term_start: Quiesce on, listed rounds, k=16 until last_index
    passes 32768 + 40 in term 2, then idle stretches (k=0, ticks only --
    the heartbeat-only rounds the lean kernel takes) long enough to
    quiesce, separated by bursts of proposals that wake the groups.  Full
    check every round after the boundary.  GPU time measured: 1.9 s."""
    ERTT = 4
    p = Pair(G=2, R=3, window=64, max_props=K, save_cap=8192,
             election_rtt=ERTT, quiesce=True)
    r = 0
    while min(_lasts(p)) <= 32768 + 40:
        o, e = p.round(k=K, tick=(r % 2 == 0), encode_saves=True, listed=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), r
        if _near(_lasts(p)) or r % 64 == 63:
            errs = p.check()
            assert not errs, (r, errs[:2])
        r += 1
        assert r < 2200
    lean = 0
    for stretch in (12, 25 * ERTT, 12):
        for i in range(stretch):
            o, e = p.round(k=0, tick=True, encode_saves=True, listed=True)
            assert e.fallbacks == 0 and e.errors == 0, (r, i, p.why())
            assert (e.committed_entries, e.messages) == \
                (o.committed_entries, o.messages), (r, i)
            lean += e.to_dict()["lean_stepped"]
            errs = p.check()
            assert not errs, (r, i, errs[:2])
            assert not p.check_saves(), (r, i)
        for i in range(3):
            o, e = p.round(k=K if i < 2 else 1, tick=(i == 1),
                           encode_saves=True, listed=True)
            assert e.fallbacks == 0 and e.errors == 0, (r, i, p.why())
            errs = p.check()
            assert not errs, (r, i, errs[:2])
            assert not p.check_saves(), (r, i)
    assert lean > 0
    assert all(p.orc.export(g, s).term == 2 for g in range(p.G)
               for s in range(p.R))


def test_two_nodehosts_past_varint_widths():
    """Two engines joined by drb_encode_wire -> drb_ingest_wire, G=2,
    window 64, k=16, 1040 rounds: LogIndex / Commit / Index cross 128 and
    16384 in Replicate, ReplicateResp, Heartbeat(+Resp) and the ReadIndex
    hints, so the device encoder writes and the device decoder parses the
    2- and 3-byte varints.  Counters every round; t.check() every 64th
    round and every round within 64 entries (+-4 rounds) of a crossing.
    GPU time measured: 3.0 s."""
    t = TwoNodes(G=2, window=64, max_props=K)
    checked = 0
    for r in range(1040):
        o, a, b = t.round(k=K, tick=(r % 2 == 0), read_index=(r % 3 == 1))
        for x in (a, b):
            assert x.fallbacks == 0 and x.errors == 0, (r, x.to_dict())
        assert a.committed_entries + b.committed_entries == \
            o.committed_entries, r
        lasts = [t.orc.export(g, s).last_index for g in range(t.G)
                 for s in range(t.R)]
        near = _near(lasts, (128, 16384), 64)
        if near or r % 64 == 63:
            errs = t.check()
            assert not errs, (r, errs[:2])
            checked += near
    errs = t.check()
    assert not errs, errs[:2]
    assert checked >= 12 and min(lasts) > 16384 + 64, (checked, lasts)
