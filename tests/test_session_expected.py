"""CPU: the expected side of the session carrier tests on its own
(tests/test_gpu_session_carriers.py; the helpers of tests/session_harness.py).

Only the oracle is stepped, on the no-op twins of the two scripts.  The
expected EntryBatches, batched LogDB records, tan files and wire streams are
built as the GPU tests build them, and shown to hold what was staged: they
decode back to the staged entries, the tan files read back record by record,
and the decoded entries cover what the GPU tests say they compare (register,
unregister, a non-zero RespondedTo, both colfer forms of both fields).
"""
import pytest

from dragonboat_amd.engine import tan_scan
from oracle import pyoracle as po
from tests import wire_ref as wr
from tests.session_harness import (FIRST_SHARD, SRC, Coverage, OrcPair,
                                   TanTwins, TAN_FILLER, filler_rounds, script_rounds,
                                   wide)
from tests.test_gpu_sessions import lifecycle

G = 12
SCRIPTS = {"lifecycle": lifecycle, "wide": wide}


def staged_of(p, ents):
    """The decoded entries that were staged with a session: each must be
    the staged entry itself."""
    n = 0
    for e in ents:
        r = p.real.get(e["key"])
        if r is not None:
            assert (e["client_id"], e["series_id"], e["responded_to"],
                    e["cmd"]) == r, e
            n += 1
    return n


def all_staged_seen(p, seen):
    """Every staged session entry was met in the carrier, on every replica
    slot in `seen` ({slot: set of Keys})."""
    for s, keys in seen.items():
        assert keys == set(p.real), (s, len(keys), len(p.real))


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_expected_entrybatches_decode_to_the_staged_entries(name):
    p = OrcPair(G)
    cov, seen = Coverage(), {s: set() for s in range(3)}
    for rows, tick, ri in script_rounds(G, SCRIPTS[name]):
        p.sess_round(rows, tick=tick, read_index=ri)
        for g in range(G):
            for s in range(3):
                b, crc = p.expected_saved(g, s)
                twin, _ = p.orc.export_saved(g, s)
                if not b:
                    assert not twin and crc == 0
                    continue
                got = po.entrybatch_unmarshal(b)
                assert got == p.saved_entries(g, s)
                assert [(e["term"], e["index"], e["key"]) for e in got] == \
                    [(e["term"], e["index"], e["key"])
                     for e in po.entrybatch_unmarshal(twin)]
                staged_of(p, got)
                seen[s] |= {e["key"] for e in got if e["key"] in p.real}
                cov.add(got)
    all_staged_seen(p, seen)
    cov.check(wide=(name == "wide"))


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_expected_batched_records_hold_session_entries(name):
    """Filler rounds first, so that the script's entries straddle index 48,
    the first batch boundary: a merged record holds a session entry."""
    p = OrcPair(G)
    db = po.BatchDB()
    merged = 0
    rounds = filler_rounds(G, 14) + list(script_rounds(G, SCRIPTS[name]))
    for rows, tick, ri in rounds:
        p.sess_round(rows, tick=tick, read_index=ri)
        for g in range(G):
            for s in range(3):
                for b, v, crc in p.expected_records(db, g, s):
                    ents = po.entrybatch_unmarshal(v)
                    merged += len(ents) > 1 and \
                        any(e["series_id"] for e in ents)
                    staged_of(p, ents)
    assert merged
    last = p.orc.export(0, 0).last_index
    assert last > 48 and last - len(SCRIPTS[name](0)) < 48


@pytest.mark.parametrize("mux,G", [(False, 12), (True, 12), (True, 20)])
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_expected_tan_files_read_back(name, mux, G):
    """1 KiB logs; TAN_FILLER rounds in front bring every log to 630-760
    bytes, so that each switches inside the script (which writes 520-590
    bytes a replica).  G = 20: shards 1-4 share their logs with 17-20."""
    p = OrcPair(G)
    tt = TanTwins(p, 1024, mux=mux)
    cov, seen = Coverage(), {s: set() for s in range(3)}
    written = {}  # the db's place -> [(log, shard, first, last, n)]
    switched = set()
    rounds = filler_rounds(G, TAN_FILLER) + \
        list(script_rounds(G, SCRIPTS[name]))
    for r, (rows, tick, ri) in enumerate(rounds):
        p.sess_round(rows, tick=tick, read_index=ri)
        for s in range(3):
            for g in range(G):
                want = tt.write(g, s)
                if want is None:
                    continue
                ents = p.saved_entries(g, s)
                place = (s, (FIRST_SHARD + g) % 16) if mux else (g, s)
                written.setdefault(place, []).append(
                    (want["log"], FIRST_SHARD + g,
                     ents[0]["index"] if ents else 0,
                     ents[-1]["index"] if ents else 0, len(ents)))
                cov.add(ents)
                seen[s] |= {e["key"] for e in ents if e["key"] in p.real}
                if want["new_log"] and r >= TAN_FILLER:
                    switched.add(place)
    for (a, b), recs in written.items():
        db = tt.real[a][b]
        got = []
        for lg in range(db.last()["log"] + 1):
            f = db.file(lg)
            assert po.tan_read(f)
            oc, vend, scan = tan_scan(f)
            assert (oc, vend) == (0, len(f)), (a, b, lg, oc)
            got += [(lg, r["shard_id"], r["first_index"] if r["n_entries"]
                     else 0, r["last_index"] if r["n_entries"] else 0,
                     r["n_entries"]) for r in scan]
        assert got == recs, (a, b)
    assert switched == set(written)  # every log switched inside the script
    all_staged_seen(p, seen)
    cov.check(wide=(name == "wide"))


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_expected_wire_streams_decode_to_the_staged_entries(name):
    p = OrcPair(G)
    cov, seen = Coverage(), {1: set(), 2: set()}
    did = 0xD1D
    for rows, tick, ri in script_rounds(G, SCRIPTS[name]):
        p.sess_round(rows, tick=tick, read_index=ri)
        for frm in range(3):
            for to in range(3):
                if frm == to:
                    continue
                msgs = p.wire_messages(frm, to)
                for lim in (0, 1, 500):
                    data = wr.expected_stream(msgs, did, SRC,
                                              lim or wr.MAX_MSG_BATCH)
                    got = []
                    for pl in wr.parse_stream(data):
                        ms, d, src, bv = po.messagebatch_unmarshal(pl)
                        assert (d, src) == (did, SRC)
                        got += ms
                    assert got == msgs, (frm, to, lim)
                for m in msgs:
                    staged_of(p, m["entries"])
                    cov.add(m["entries"])
                    if frm == 0:
                        seen[to] |= {e["key"] for e in m["entries"]
                                     if e["key"] in p.real}
    all_staged_seen(p, seen)
    cov.check(wide=(name == "wide"))
