"""GPU: the two inbound paths place by one rule (csrc/drb_place.hpp).

Twin engines of one configuration (4 groups x 3 replicas, mailbox 4, window
8, cmd_cap 32, max_props 2, forward proposals, replica 1 on another
NodeHost) take the same messages, one through drb_ingest_ex (decoded
pb.Message arrays; the host places them) and one through drb_ingest_wire
(the TCP bytes; a kernel places them).  Each case drives one capacity of the
GPU inbox (include/drb_engine.h, above enum drb_ingest_fate) and asserts the
promised outcome -- the counts, every message's fate, each receiver's inbox
and the flagged receivers -- and that both paths give it.  Within a case a
receiver is sent to over one sender plane, so the paths' documented
difference of scope stays out; the last case is about that difference.
"""
import pytest

from dragonboat_amd import abi
from dragonboat_amd.engine import Engine
from oracle import pyoracle as po
from tests import wire_ref as wr
from tests.gpu_harness import DistPair

pytestmark = pytest.mark.gpu

MSG = abi.MSG
DID = 0xD1D
PLACED, DIVERTED = abi.ING_PLACED, abi.ING_DIVERTED
CFG = dict(num_groups=4, num_replicas=3, mailbox=4, window=8, cmd_cap=32,
           max_props=2, forward_proposals=1)
LAST = 4  # every log's last index after init_steady (R config changes + 1)


def _twins(unhost=(0,), **kw):
    """Two engines alike: steady at term 2, the replicas of `unhost` on
    another NodeHost, one quiet round behind them (the inbox planes carry
    the previous round's tag)."""
    engs = []
    for _ in range(2):
        e = Engine(**dict(CFG, **kw))
        e.init_steady(term=2, leader_slot=0)
        for s in unhost:
            e.host_slot(s, False)
        e.step()
        assert e.take_flagged() == ([], 0)
        engs.append(e)
    return engs


def _feed_ex(e, msgs):
    got = e.ingest_ex(*po.build_messages(msgs))
    return (got["accepted"], got["dropped"], got["diverted"]), got["status"]


def _feed_wire(e, msgs):
    """The fates by what drb_ingest_wire_cpu hands back: the messages of a
    case are all different, so a tuple names its message."""
    tuples = [po.msg_tuple(m) for m in msgs]
    assert all(tuples.count(t) == 1 for t in tuples)
    data = wr.expected_stream(msgs, DID, b"cpu:1")
    got = e.ingest_wire(data, DID)
    assert (got["bad"], got["messages"]) == (0, len(msgs)), got
    cpu = e.ingest_wire_cpu()
    assert all(f == DIVERTED for _, _, f in cpu), cpu
    div = [wr.message_tuple(data[o:o + n]) for o, n, _ in cpu]
    assert all(t in tuples for t in div) and len(div) == got["diverted"]
    # (stream order, as the header promises)
    assert div == [t for t in tuples if t in div]
    return (got["accepted"], got["dropped"], got["diverted"]), \
        [DIVERTED if t in div else PLACED for t in tuples]


def _inboxes(e, G, slots):
    return {(g, s): e.export_inbox(g, s) for g in range(G) for s in slots}


def _flagged(e):
    recs, lost = e.take_flagged()
    assert lost == 0
    return sorted(recs)


def _both(engs, msgs, fates, flagged, G=4, slots=(1, 2)):
    """Feeds msgs to both engines.  fates: each message's promised fate; a
    receiver's inbox is then its PLACED messages, a Quiesce ahead of the
    others; flagged: the (group, slot) that leave with DRB_FB_CAPACITY."""
    counts = (fates.count(PLACED), 0, fates.count(DIVERTED))
    inbox = {(g, s): [] for g in range(G) for s in slots}
    for m, f in zip(msgs, fates):
        if f == PLACED:
            box = inbox[(m["shard_id"] - 1, m["to"] - 1)]
            box.insert(0 if m["type"] == MSG["Quiesce"] else len(box),
                       po.msg_tuple(m))
    seen = []
    for e, feed in zip(engs, (_feed_ex, _feed_wire)):
        got_counts, got_fates = feed(e, msgs)
        assert got_counts == counts, (feed.__name__, got_counts, counts)
        assert list(got_fates) == fates, (feed.__name__, got_fates)
        assert _inboxes(e, G, slots) == inbox, feed.__name__
        fl = _flagged(e)
        assert {(g, s, r) for (g, s, r, *_x) in fl} == \
            {(g, s, abi.FB["CAPACITY"]) for (g, s) in flagged}, fl
        seen.append(fl)
    assert seen[0] == seen[1]  # flags, round and shard alike
    for e in engs:
        e.close()


def _hb(g, commit, term=2, frm=1, to=2):
    return po.msg(MSG["Heartbeat"], from_=frm, to=to, term=term,
                  commit=commit, shard_id=g + 1)


def _ents(first, n, cmd=b"0123456789abcdef"):
    return [po.ent(term=2, index=first + x, key=100 + x, client_id=7,
                   cmd=cmd[:len(cmd) - x] if x else cmd) for x in range(n)]


def _rep(g, log_index, n, to=2, commit=LAST, cmd=b"0123456789abcdef"):
    return po.msg(MSG["Replicate"], from_=1, to=to, term=2, log_term=2,
                  log_index=log_index, commit=commit, shard_id=g + 1,
                  entries=_ents(log_index + 1, n, cmd))


def _prop(g, n, cmd=b"\x00twelve bytes"):
    es = [po.ent(key=5 + x, client_id=9, type=abi.ENTRY_ENCODED, cmd=cmd)
          for x in range(n)]
    return po.msg(MSG["Propose"], from_=1, to=2, shard_id=g + 1, entries=es)


def test_five_messages_on_a_four_record_plane():
    msgs = [_hb(0, c) for c in range(1, 6)] + [_hb(1, 1), _hb(1, 2)] + \
        [_hb(2, c, to=3) for c in range(1, 5)]
    _both(_twins(), msgs, [PLACED] * 4 + [DIVERTED] + [PLACED] * 6, {(0, 1)})


def test_one_propose_per_plane_and_max_props():
    second = _prop(0, 1, cmd=b"\x00another")
    msgs = [_prop(0, 1), second, _prop(1, 3), _prop(2, 2, cmd=b""),
            _prop(3, 2)]
    _both(_twins(), msgs, [PLACED, DIVERTED, DIVERTED, PLACED, PLACED],
          {(0, 1), (1, 1)})


def test_replicate_beyond_the_window():
    msgs = [_rep(0, LAST, 9), _rep(1, LAST, 8), _rep(2, LAST, 0, commit=3)]
    _both(_twins(), msgs, [DIVERTED, PLACED, PLACED], {(0, 1)})


def test_cmd_over_cmd_cap():
    long, full = bytes(range(1, 34)), bytes(range(1, 33))
    msgs = [_rep(0, LAST, 1, cmd=long), _rep(1, LAST, 2, cmd=full),
            _prop(2, 1, cmd=b"\x00" + long[1:]), _prop(3, 1, cmd=b"\x00" +
                                                       full[1:]),
            _hb(0, 1, to=3)]
    _both(_twins(), msgs, [DIVERTED, PLACED, DIVERTED, PLACED, PLACED],
          {(0, 1), (2, 1)})


def test_two_terms_after_a_prevote():
    """Every record comes back with the term it was sent with: the pre-vote
    never lends the plane its term, and the second Heartbeat's differs from
    the first's (elections on: the records' own terms are kept)."""
    pv = po.msg(MSG["RequestPreVote"], from_=1, to=2, term=3, log_term=2,
                log_index=LAST, shard_id=1)
    msgs = [pv, _hb(0, 1, term=2), _hb(0, 2, term=3),
            _hb(1, 1, term=2), _hb(1, 2, term=5), _hb(1, 3, term=2)]
    _both(_twins(elections=1, pre_vote=1), msgs, [PLACED] * 6, set())


def test_quiesce_on_a_full_plane():
    q = po.msg(MSG["Quiesce"], from_=1, to=2, shard_id=1)
    msgs = [_hb(0, c) for c in range(1, 5)] + [q, _hb(0, 5)]
    _both(_twins(), msgs, [PLACED] * 5 + [DIVERTED], {(0, 1)})


def test_remote_plane_entry_rows():
    """Replicas spread over two ranks, two entry rows a remote plane: group
    0's third Replicate runs past the rows, group 2's last one lies below
    their first index; a commit-only Replicate needs no row."""
    pairs = []
    for _ in range(2):
        # (forward rows are a co-resident plane's: not with placement)
        p = DistPair(G=4, R=3, N=2, E=2, window=8, mailbox=4, cmd_cap=32,
                     max_props=2)
        for e in p.engs:
            e.host_slot(0, False)
        p.round(k=0)
        pairs.append(p)
    # replica 2 (slot 1) of groups 0 and 2 lives on rank 1, lanes 0 and 1,
    # and its plane from slot 0 is a remote one
    engs = [p.engs[1] for p in pairs]
    assert all(p.where(g, 1) == (1, g // 2) for p in pairs for g in (0, 2))
    msgs = [_rep(0, LAST, 1), _rep(0, LAST + 1, 1), _rep(0, LAST + 2, 1),
            _rep(2, LAST, 0, commit=3), _rep(2, LAST, 2),
            _rep(2, LAST - 1, 1)]
    fates = [PLACED, PLACED, DIVERTED, PLACED, PLACED, DIVERTED]
    want = {0: [po.msg_tuple(m) for m in msgs[:2]],
            1: [po.msg_tuple(m) for m in msgs[3:5]]}
    seen = []
    for e, feed in zip(engs, (_feed_ex, _feed_wire)):
        counts, got = feed(e, msgs)
        assert counts == (4, 0, 2) and list(got) == fates, (counts, got)
        for lane in (0, 1):
            assert e.export_inbox(lane, 1) == want[lane], (feed.__name__, lane)
        fl = _flagged(e)
        assert [(j, s, r) for (j, s, r, *_x) in fl] == \
            [(0, 1, abi.FB["CAPACITY"]), (1, 1, abi.FB["CAPACITY"])], fl
        seen.append(fl)
    assert seen[0] == seen[1]
    for p in pairs:
        for e in p.engs:
            e.close()


def test_scope_of_a_divert_differs_as_documented():
    """Two senders to one receiver, the first plane overflows: the host path
    diverts the rest of the call for that receiver, the wire path only the
    overflowing plane's (include/drb_engine.h, above enum drb_ingest_fate).
    Either way the receiver is flagged and every sender's order is kept."""
    ex, wire = _twins(unhost=(0, 1))
    msgs = [_hb(0, c, to=3) for c in range(1, 6)] + \
        [_hb(0, c, frm=2, to=3) for c in (6, 7)]
    t = [po.msg_tuple(m) for m in msgs]
    counts, fates = _feed_ex(ex, msgs)
    assert counts == (4, 0, 3) and fates == [PLACED] * 4 + [DIVERTED] * 3
    assert ex.export_inbox(0, 2) == t[:4]
    counts, fates = _feed_wire(wire, msgs)
    assert counts == (6, 0, 1)
    assert fates == [PLACED] * 4 + [DIVERTED] + [PLACED] * 2
    assert wire.export_inbox(0, 2) == t[:4] + t[5:]
    fl = [_flagged(e) for e in (ex, wire)]
    assert fl[0] == fl[1] and \
        [(g, s, r) for (g, s, r, *_x) in fl[0]] == [(0, 2, abi.FB["CAPACITY"])]
    for e in (ex, wire):
        e.close()
