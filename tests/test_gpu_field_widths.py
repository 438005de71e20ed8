"""GPU: terms and ticks that do not fit the packed record's 16 bits.

The packed replica record (drb_layout.hpp) stores appliedToTerm / prevTerm
/ smTerm as 16-bit distances from `term` and the three tick fields as 16
bits, each with an escape (0xffff) to the u64 overflow array.  Here a term
jump of exactly 65534 (the last in-range distance), 65535 (the first
escape) and to 2^49 -+ (the 7- / 9-byte varint boundary of the wire and
colfer encodings), and election ticks walking through 65534 / 65535 /
65536 (large ElectionRTT), against the oracle every round.
"""
import pytest

from dragonboat_amd import abi
from oracle import pyoracle as po
from tests.gpu_harness import Pair
from tests.test_gpu_tan import _check_round
from tests.test_gpu_truncation import _unhost
from tests.test_gpu_wire import SRC, _check_planes

pytestmark = pytest.mark.gpu

DID = 0xD1D


@pytest.mark.parametrize("tan", [0, 1])
def test_term_jump_past_packed_distance(tan):
    """Slot 2 stops.  A HeartbeatResp from it at term 3 first makes the two
    hosted replicas elect among themselves, so appliedToTerm / smTerm /
    prevTerm move to the new term inside the packed record while their
    overflow slots still hold the initial 2 (a later escape that failed to
    store its value would read that).  Then a HeartbeatResp at term T
    reaches replicas 1 and 2 of group g as a wire frame (drb_ingest_wire
    parses the 3-, 7- and 9-byte Term varints), T = term + 65534, term +
    65535, 2^49 - 2, 2^49 + 5.  Both become followers at T with
    appliedToTerm / smTerm still the old term -- distance 65534 is the
    last that packs, the others escape -- then time out, campaign, and a
    leader above T appends and commits: the entries carry the wide term in
    EntryBatch / tan records and in Replicate.  State, logs, KV, outboxes,
    ReadyToReads, saves and the planes from the hosted slots every round,
    60 ticking rounds after the jump; the planes of the rounds in which a
    term changes carry records sent before the change (their own term,
    rterm).  GPU time measured: 3.6 s."""
    G = 4
    p = Pair(G=G, R=3, elections=1, save_cap=4096, max_props=4,
             **({"save_tan": 1} if tan else {}))
    dbs = [[po.TanDB() for _ in range(p.R)] for _ in range(p.G)]
    logs = {}
    planes = [(0, 1), (1, 0), (0, 2), (1, 2)]
    first = p.eng.cfg["first_shard_id"]

    def one(r, k=1):
        o, e = p.round(k=k, tick=True, encode_saves=True,
                       read_index=(r % 3 == 0))
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), (r, e.to_dict(), o.to_dict())
        errs = p.check()
        assert not errs, (r, errs[:2])
        if tan:
            _check_round(p, dbs, logs, r)
        else:
            assert not p.check_saves(), r
        _check_planes(p, did=DID, limits=[0], planes=planes)

    def jump(terms):
        msgs = [po.msg(abi.MSG["HeartbeatResp"], from_=3, to=to,
                       term=terms[g], shard_id=first + g)
                for g in range(G) for to in (1, 2)]
        p.orc.ingest(msgs)
        got = p.eng.ingest_wire(
            po.wire_frame(po.messagebatch_marshal(msgs, DID, SRC)), DID)
        assert got["bad"] == 0 and got["accepted"] == len(msgs), got

    def pair_of(g):
        return [p.eng.export(g, s) for s in (0, 1)]

    def led(g):
        sts = pair_of(g)
        return sorted(a.role for a in sts) == \
            sorted([abi.FOLLOWER, abi.LEADER]) and \
            all(a.applied_to_term == a.sm_term == a.term for a in sts)

    _unhost(p, range(G), 2)  # (the last import: the overflow slots hold 2)
    r = 0
    for r in range(3):
        one(r)
    jump([3] * G)
    while not all(led(g) and pair_of(g)[0].term > 2 for g in range(G)):
        r += 1
        one(r)
        assert r < 60, [[(a.role, a.term) for a in pair_of(g)]
                        for g in range(G)]
    cur = [pair_of(g)[0].term for g in range(G)]
    assert min(cur) > 2
    T = [cur[0] + 65534, cur[1] + 65535, (1 << 49) - 2, (1 << 49) + 5]
    jump(T)
    r += 1
    one(r)
    for g in range(G):
        for a in pair_of(g):
            assert (a.role, a.term, a.applied_to_term, a.sm_term) == \
                (abi.FOLLOWER, T[g], cur[g], cur[g]), g
    for _ in range(60):
        r += 1
        one(r)
    for g in range(G):
        sts = pair_of(g)
        osts = [p.orc.export(g, s) for s in (0, 1)]
        assert [(a.role, a.term) for a in sts] == \
            [(b.role, b.term) for b in osts], g
        assert led(g), g
        for a in sts:
            assert a.term > T[g] and a.committed > 8, g
        s = 0 if sts[0].role == abi.LEADER else 1
        ent = p.eng.export_log(g, s, sts[s].last_index, sts[s].last_index)[0]
        assert ent[0] == sts[s].term  # the wide term in the resident log


@pytest.mark.parametrize("ertt", [70000, 40000])
def test_ticks_past_16_bits(ertt):
    """ElectionRTT 70000: every randomizedElectionTimeout (ElectionRTT +
    rand % ElectionRTT, raft.go:571-580) exceeds 65535 and lives in the
    overflow array; ElectionRTT 40000: the 48 timeouts fall on both sides
    of 65535 (seed 0x5EEDD8B0), so packed and escaped timeouts sit in one
    wavefront.  (No ElectionRTT puts the timeouts on both sides of 65535
    AND lets a leader's electionTick, which wraps at ElectionRTT, reach
    65535 -- hence two cases.)  With 70000 half the groups are re-imported
    with election_tick = 65530 at the leader, whose tick then walks
    through 65534 / 65535 / 65536 (in range -> escaped), and 65534 / 65535
    at the followers, which tick once more (escaped) before the first
    heartbeat resets them (escaped -> in range).  12 ticking rounds, k=1,
    full check every round.  GPU time measured: 2.2 s."""
    G = 16
    p = Pair(G=G, R=3, election_rtt=ertt)
    ts = [p.orc.export(g, s).randomized_election_timeout
          for g in range(G) for s in range(3)]
    if ertt == 70000:
        assert min(ts) > 65535, min(ts)
    else:
        assert min(ts) < 65535 < max(ts), (min(ts), max(ts))
        assert sum(t < 65535 for t in ts) >= 8 <= sum(t > 65535 for t in ts)
    assert not p.check(), "init"
    moved = range(0, G, 2) if ertt == 70000 else ()
    for g in moved:
        reps = []
        for s in range(3):
            st = p.orc.export(g, s)
            st.election_tick = (65530, 65534, 65535)[s]
            log = [po._etuple_to_dict(t)
                   for t in p.orc.export_log(g, s, 1, st.last_index)]
            reps.append((st, log))
        p.import_group(g, reps)
    errs = p.check()
    assert not errs, ("import", errs[:2])
    seen, foll = set(), {}
    for r in range(12):
        o, e = p.round(k=1, tick=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), r
        errs = p.check()
        assert not errs, (r, errs[:2])
        for g in moved:
            seen.add(p.eng.export(g, 0).election_tick)
            for s in (1, 2):
                foll.setdefault(s, []).append(p.eng.export(g, s).election_tick)
    if ertt == 70000:
        assert {65534, 65535, 65536} <= seen, sorted(seen)
        for s in (1, 2):  # escaped, then reset by the heartbeat
            assert max(foll[s]) >= 65535 and foll[s][-1] < 16, foll[s][:24]
