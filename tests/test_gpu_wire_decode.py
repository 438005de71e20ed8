"""GPU: drb_ingest_wire on hostile and non-canonical message bytes.

tests/wire_cases.py through the whole receive path: every case's message M
travels in a stream of three frames of the right deployment with sound
CRCs -- a one-message frame, MessageBatch{[good, M, good]}, a one-message
frame -- so only the per-message decoder (drb_msgdec.hpp in k_ing_count /
k_ing_decode) can object.  The expected drb_wire_in counters, the inbox
contents and the CPU path's list come from the corpus' hand-written outcome,
never from the engine.  The same bytes go through the decoder on the CPU
under AddressSanitizer / UBSan in tests/test_msgdecode_host.py.

Replica 3 (slot 2) leads every group from another NodeHost: it is unhosted
on both sides.  Case k's M goes from it to replica 1 of shard first + k;
the good messages (Heartbeats) go to replica 2 of the same shard, a plane
of their own, so no plane fills and a diverted M takes nothing with it.
"""
import pytest

from dragonboat_amd import abi
from dragonboat_amd.engine import Engine
from oracle import pyoracle as po
from tests import wire_cases as wc
from tests.gpu_harness import Pair
from tests.test_gpu_truncation import _unhost
from tests.test_msgdecode_host import expected_msg

pytestmark = pytest.mark.gpu

DID = 0xD1D
FIRST = 1      # the default first_shard_id
CMD_CAP = 32   # the default cmd_cap
CASES = wc.hand_cases(FIRST, CMD_CAP)
COUNTERS = ("frames", "messages", "accepted", "dropped", "bad", "consumed",
            "snapshots", "diverted")


def stream_of(shard, data, elem_tag=b"\x0a", elem_len_pad=0):
    """(stream, length of its first frame, offset of M in the stream, the
    good message)."""
    good = wc.cmsg(wc.heartbeat(shard, to=2))
    f1 = wc.frame(wc.batch([good], DID))
    payload = wc.batch([good, data, good], DID, elem_tag=elem_tag,
                       elem_len_pad=elem_len_pad)
    # frame 2: a 20-byte header, the first element, M's tag and length
    off = len(f1) + 20
    for n in (len(good), len(data)):
        off += len(elem_tag) + len(wc.vi(n)) + elem_len_pad
    off += len(good)
    stream = f1 + wc.frame(payload) + f1
    assert stream[off:off + len(data)] == data
    return stream, len(f1), off, good


def expected_counters(outcome, placed, stream_len, first_len):
    """drb_wire_in of the three-frame stream, from the outcome alone."""
    want = dict(frames=3, messages=5, accepted=4, dropped=0, bad=0,
                consumed=stream_len, snapshots=0, diverted=0)
    if outcome == "bad":  # ErrBadMessage: the stream stops at frame 2
        want.update(frames=1, messages=1, accepted=1, bad=1,
                    consumed=first_len)
    elif outcome == "snapshot":
        want.update(messages=4, snapshots=1)
    elif outcome == "big":
        want.update(diverted=1)
    elif placed:
        want.update(accepted=5)
    else:
        want.update(dropped=1)
    return want


def inbox_tuple(m):
    """What drb_export_inbox returns for an expected message: an entry's
    Index is not stored (it is LogIndex + 1 + its position, as in every
    Replicate a leader sends)."""
    m = expected_msg(m)
    for x, e in enumerate(m["entries"]):
        e["index"] = m["log_index"] + 1 + x
    return po.msg_tuple(m)


def test_hand_cases():
    """Every hand-written case, one call each (under 2 KB), then one ticking
    round of all groups against the oracle: counters, inboxes and the CPU
    path's list per case; a refused frame leaves no trace.  GPU time
    measured: 3.2 s (260 calls)."""
    G = len(CASES)
    p = Pair(G=G, R=3, leader_slot=2)
    assert (p.eng.cfg["first_shard_id"], p.eng.cfg["cmd_cap"]) == \
        (FIRST, CMD_CAP)
    _unhost(p, range(G), 2)
    o, e = p.round(k=0, tick=False)
    assert e.fallbacks == 0 and e.errors == 0
    assert not p.check(groups=range(0, G, 16))
    fed, big, errs = [], [], []
    for k, c in enumerate(CASES):
        shard = FIRST + k
        stream, first_len, off, good = stream_of(shard, c.data, c.elem_tag,
                                                 c.elem_len_pad)
        assert len(stream) < 2048, c.name
        got = p.eng.ingest_wire(stream, DID)
        got = {f: got[f] for f in COUNTERS}
        want = expected_counters(c.outcome, c.placed, len(stream), first_len)
        cpu = p.eng.ingest_wire_cpu()
        good_m = expected_msg(wc.heartbeat(shard, to=2))
        n_good = 1 if c.outcome == "bad" else 4
        inbox = [inbox_tuple(c.msg)] if c.outcome == "ok" and c.placed else []
        want_cpu = []  # refused, or decoded and dropped: nothing for the CPU
        if c.outcome == "snapshot":
            want_cpu = [(off, len(c.data), abi.ING_SNAPSHOT)]
        elif c.outcome == "big":
            want_cpu = [(off, len(c.data), abi.ING_DIVERTED)]
            big.append(k)
        for what, a, b in (
                ("counters", got, want), ("cpu", cpu, want_cpu),
                ("goods", p.eng.export_inbox(k, 1),
                 [po.msg_tuple(good_m)] * n_good),
                ("inbox", p.eng.export_inbox(k, 0), inbox)):
            if a != b:
                errs.append((c.name, c.go, what, a, b))
        fed += [good_m] * n_good
        if inbox:
            fed.append(expected_msg(c.msg))
    assert not errs, (len(errs), errs[:4])
    assert len(big) == 3
    # the oracle takes the canonical equivalents of what was placed.  Not
    # compared from here on: the receivers of the diverted messages and of
    # the answer types a follower's fast path does not take (Case.steps),
    # which the engine handed to the CPU raft.Peer
    off_path = set(big) | {k for k, c in enumerate(CASES) if not c.steps}
    live = [g for g in range(G) if g not in off_path]
    p.orc.ingest(fed)
    o, e = p.round(k=0, tick=True)
    assert e.errors == 0, (e.to_dict(), p.why())
    errs = [(CASES[x[0]].name,) + tuple(x[1:4]) for x in p.check(groups=live)]
    assert not errs, (len(errs), errs)


def test_mutation_sample():
    """256 seeded bit flips and byte deletions (wire_cases.mutation_sample),
    one call each, on the counters: what the oracle's Message.Unmarshal
    makes of the bytes (equal to the decoder's on the CPU, tests/
    test_msgdecode_host.py) decides refused / snapshot / diverted /
    accepted / dropped.  GPU time measured: 0.2 s."""
    N = 256
    eng = Engine(num_groups=N, num_replicas=3)
    eng.init_steady(term=2, leader_slot=2, seed=0x5EEDD8B0)
    eng.host_slot(2, False)
    seen = set()
    for j, (name, data) in enumerate(wc.mutation_sample(N, FIRST)):
        stream, first_len, off, good = stream_of(FIRST + j, data)
        outcome, m = po.message_unmarshal(data)
        placed = False
        if outcome == "ok":
            if any(len(x["cmd"]) > CMD_CAP for x in m["entries"]):
                outcome = "big"
            placed = FIRST <= m["shard_id"] < FIRST + N and \
                m["from_"] == 3 and m["to"] in (1, 2)
            if not placed:
                outcome = "ok"  # dropped before a Cmd's size matters
        got = eng.ingest_wire(stream, DID)
        want = expected_counters(outcome, placed, len(stream), first_len)
        assert {f: got[f] for f in COUNTERS} == want, (name, outcome, got)
        seen.add((outcome, placed))
    assert {("ok", True), ("bad", False)} <= seen, seen
