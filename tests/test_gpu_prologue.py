"""GPU: the step kernels' one-trip prologue against the oracle.

The step kernels issue every load whose address follows from (slot, group)
and the round parameters before their first wait -- the state record, the
remotes, every sender's inbox header, the staged inputs, the readIndex
queue's first row -- for every lane of the launch, the ones without a
round included; the dispatch loop takes the senders' record counts from
the pre-pass.  These tests step the shapes where that can go wrong:
lanes at the edges of a wave and of a workgroup, planes that still hold
older rounds' records, replicas that load but have no round, inboxes with
many senders, and rounds that release several ReadyToReads at once.
Every round is compared with the oracle.
"""
import struct

import pytest

from dragonboat_amd import abi, workload
from tests.gpu_harness import Pair, state_diff

pytestmark = pytest.mark.gpu

READS = 9
KEYS = 16


def _counts(o, e):
    return ((e.committed_entries, e.applied_entries, e.messages,
             e.ready_to_reads, e.dropped_read_indexes),
            (o.committed_entries, o.applied_entries, o.messages,
             o.ready_to_reads, o.dropped_read_indexes))


def _same_counts(o, e, what):
    a, b = _counts(o, e)
    assert a == b, (what, e.to_dict(), o.to_dict())
    assert e.fallbacks == 0 and e.errors == 0, (what, e.to_dict())


def _sample(G):
    """The groups at the edges of the waves and workgroups, and every
    16th: what the rounds between two full comparisons look at."""
    edge = {0, 1, 62, 63, 64, 65, 127, 128, 255, 256, G - 2, G - 1}
    return sorted(g for g in edge | set(range(0, G, 16)) if 0 <= g < G)


def _check(p, what, full=True):
    """Every live replica against the oracle (state, log, KV, messages,
    ReadyToReads); between full comparisons a sample of the groups -- the
    round's counters (_same_counts) cover all of them every round.  (A
    full comparison exports every replica through the C ABI one by one:
    2-3 s a round at G = 257-300 or R = 8, 20-34 s a test.)"""
    groups = [g for g in (range(p.G) if full else _sample(p.G))
              if g not in p.cpu]
    errs = p.check(groups=groups)
    assert not errs, (what, errs[:3])


def _set_hosted(p, groups, slot, hosted):
    for g in groups:
        p.orc.set_hosted(g, slot, hosted)
        sts = p.eng.export_replicas(g, 1)
        if hosted:
            sts[slot].flags |= abi.F_HOSTED
        else:
            sts[slot].flags &= ~abi.F_HOSTED
        p.eng.import_replicas(g, sts)


def _check_reads(p, e, key_space, what):
    """The round's served reads against the oracle's: counts and sums."""
    sums, served, deferred = p.orc.serve_reads(READS, key_space)
    assert (e.reads_served, e.reads_deferred) == (served, deferred), what
    esums = p.eng.export_read_sums(0, p.G)
    for i, x in enumerate(sums):
        if x is not None:
            assert esums[i] == x, (what, i)
    return served, deferred


@pytest.mark.parametrize("G", [1, 65, 257])
def test_edge_lanes(G):
    """A lone lane, a partial second wave, one lane in a second workgroup:
    the lanes past the last group load a valid group's words and use none
    of them."""
    p = Pair(G=G, R=3)
    for r in range(8):
        o, e = p.round(k=1, tick=(r % 2 == 0), read_index=True, reads=READS)
        _same_counts(o, e, r)
        _check_reads(p, e, 256, r)
        _check(p, r, full=(G <= 65 or r == 7))
    p.eng.sync()  # no device error


def test_stale_planes_quiet_rounds():
    """Rounds without input read planes that still hold the records and
    headers of older rounds (stale round tags): nothing comes of them."""
    p = Pair(G=300, R=3)

    def busy(n, base):
        for r in range(n):
            o, e = p.round(k=1, tick=True, read_index=True, reads=READS)
            _same_counts(o, e, (base, r))
            _check(p, (base, r), full=(r == n - 1))

    busy(4, "busy")
    # three rounds with no proposal, tick or ReadIndex: what is still in
    # flight drains exactly as the oracle's does
    for r in range(3):
        o, e = p.round(k=0, tick=False, read_index=False, reads=READS)
        _same_counts(o, e, ("quiet", r))
        _check(p, ("quiet", r), full=False)
    # ... until the cluster is at rest; then three more, whose planes
    # hold nothing but stale records: no message, no ReadyToRead, no
    # state change
    for r in range(8):
        o, e = p.round(k=0, tick=False, read_index=False, reads=READS)
        _same_counts(o, e, ("drain", r))
        _check(p, ("drain", r), full=False)
        if o.messages == 0 and o.ready_to_reads == 0:
            break
    else:
        raise AssertionError("the cluster did not come to rest")
    before = p.eng.export_replicas(0, p.G)
    for r in range(3):
        o, e = p.round(k=0, tick=False, read_index=False, reads=READS)
        assert (e.messages, e.ready_to_reads, e.committed_entries,
                e.applied_entries, e.reads_served) == (0, 0, 0, 0, 0), \
            (r, e.to_dict())
        _same_counts(o, e, ("rest", r))
        _check(p, ("rest", r), full=False)
    after = p.eng.export_replicas(0, p.G)
    for i, (a, b) in enumerate(zip(after, before)):
        assert not state_diff(a, b, p.R), (i // p.R, i % p.R)
    _check(p, "rest")
    busy(4, "again")


def test_replicas_with_no_round():
    """A stopped follower and a group in fallback: their lanes load with
    the others and keep their state, an empty ReadyToRead list and an
    empty save record."""
    p = Pair(G=70, R=3, save_cap=4096)
    kw = dict(k=1, read_index=True, reads=READS, encode_saves=True)
    for r in range(3):
        o, e = p.round(tick=False, **kw)
        _same_counts(o, e, r)
        _check(p, r)
    assert not p.check_saves()
    stopped = [5, 33, 64, 69]
    _set_hosted(p, stopped, 2, False)
    fb = 40
    p.to_cpu(fb)  # every replica of the group marked FALLBACK
    pre_fb = p.eng.export_replicas(fb, 1)
    pre_st = {g: p.eng.export_replicas(g, 1)[2] for g in stopped}
    for r in range(3):
        o, e = p.round(tick=False, **kw)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict())
        errs = p.check()
        assert not errs, (r, errs[:3])
        assert not p.check_saves([g for g in p.live_groups()
                                  if g not in stopped])
        for s, (a, b) in enumerate(zip(p.eng.export_replicas(fb, 1), pre_fb)):
            assert not state_diff(a, b, p.R), (r, fb, s)
            assert a.flags == b.flags
            assert p.eng.export_ready(fb, s) == []
            assert p.eng.export_saved(fb, s)[0] == b""
        for g in stopped:
            a = p.eng.export_replicas(g, 1)[2]
            assert not state_diff(a, pre_st[g], p.R), (r, g)
            assert a.flags == pre_st[g].flags
            assert p.eng.export_ready(g, 2) == []
            assert p.eng.export_saved(g, 2)[0] == b""
    _set_hosted(p, stopped, 2, True)
    for r in range(8):  # reject, retry, catch up
        o, e = p.round(tick=False, **kw)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict())
        errs = p.check()
        assert not errs, (r, errs[:3])
    assert not p.check_saves(p.live_groups())


@pytest.mark.parametrize("R", [5, 8])
def test_wide_inboxes(R):
    """Several senders at the leader, batches of four entries, a tick and a
    ReadIndex every round: the per-sender record counts of R = 8 take both
    packed words."""
    p = Pair(G=70, R=R, max_props=4)
    for r in range(10):
        o, e = p.round(k=4, tick=True, read_index=True, reads=READS)
        _same_counts(o, e, r)
        _check_reads(p, e, 256, r)
        _check(p, r, full=(r == 9))
    p.eng.sync()


def test_wide_inboxes_through_the_raft_launch():
    """The same mix on an elections engine whose leaders stop in some
    groups: their followers time out and campaign, so the raft launch
    steps replicas whose senders' header terms differ (votes at term 3
    beside records of term 2) and then runs the mix under the new leaders
    with one member silent."""
    G, R = 70, 5
    p = Pair(G=G, R=R, max_props=4, elections=1)
    E = [1, 6, 20, 63, 64, 69]
    near = sorted(set(E) | {0, 2, 62, 65})
    st = {"slow": 0, "roles": 0}

    def rounds(n, full_last=True):
        for i in range(n):
            o, e = p.round(k=4, tick=True, read_index=True, reads=READS)
            _same_counts(o, e, p.rounds)
            _check_reads(p, e, 256, p.rounds)
            if full_last and i == n - 1:
                _check(p, p.rounds)
            else:  # the groups with an election, and their neighbours
                errs = p.check(groups=near)
                assert not errs, (p.rounds, errs[:2])
            st["slow"] += e.elections_stepped
            st["roles"] += e.role_changes

    def leaders(g):
        return [s for s, x in enumerate(p.eng.export_replicas(g, 1))
                if x.role == abi.LEADER]

    rounds(3)
    assert st["slow"] == 0
    _set_hosted(p, E, 0, False)
    for _ in range(60):
        rounds(1, full_last=False)
        if all(len(leaders(g)) == 2 for g in E):  # the stopped one, a new one
            break
    else:
        raise AssertionError("no new leaders")
    assert st["slow"] > 0 and st["roles"] >= len(E), st
    rounds(6)
    for g in E:
        assert len(leaders(g)) == 2 and 0 in leaders(g), (g, leaders(g))
    p.eng.sync()


def _expected_results(p, slot, key_space):
    exp = []
    for g in range(p.G):
        st = p.orc.export(g, slot)
        kv = p.orc.export_kv(g, slot)
        for (index, low, high) in p.orc.export_ready(g, slot):
            if index > st.sm_index:
                continue  # deferred: no result yet
            for j in range(READS):
                x = workload.mix64(
                    low ^ (((j + 1) * workload.GOLDEN) & workload.MASK))
                key = x % key_space
                v = kv.get(struct.pack("<Q", key))
                exp.append((g, index, low, j, key, int(v is not None),
                            len(v) if v is not None else 0,
                            int.from_bytes((v or b"")[:4], "little")))
    return exp


class _Reads:
    """Rounds with served reads (16 keys, 9 reads per ctx) compared with
    the oracle: counts, read sums and the ReadyToRead lists every round;
    the read results and every group's full state where `full`."""

    def __init__(self, G):
        self.p = Pair(G=G, R=3, max_reads_per_ctx=READS)
        self.most = self.served = self.deferred = 0

    def one(self, what, at, tick=False, full=False, **kw):
        p = self.p
        o, e = p.round(tick=tick, ri_replica=at, reads=READS,
                       read_key_space=KEYS, key_space=KEYS, **kw)
        _same_counts(o, e, what)
        _check(p, what, full)
        for slot in sorted({0, at - 1 if at else 0}):
            ready = {g: p.orc.export_ready(g, slot) for g in range(p.G)}
            assert p.eng.export_ready_batch(slot) == \
                {g: x for g, x in ready.items() if x}, (what, slot)
            self.most = max([self.most] + [len(x) for x in ready.values()])
            if full:
                assert p.eng.export_read_results(slot) == \
                    _expected_results(p, slot, KEYS), (what, slot)
        s, d = _check_reads(p, e, KEYS, what)
        self.served += s
        self.deferred += d
        return e


@pytest.mark.parametrize("ri_replica", [0, 2])
def test_ready_to_reads_beyond_the_register_cache(ri_replica):
    """A leader whose followers are stopped queues a ReadIndex ctx in each
    of three rounds; once they answer again, the next confirmed ctx
    releases the whole queue in one round: four ReadyToReads, which the
    served reads take from the round output in order.  Before and after,
    the requests are issued at ri_replica (0: the leader, 2: a follower)."""
    G = 70
    t = _Reads(G)
    p = t.p
    for r in range(2):
        t.one(("steady", r), ri_replica, k=1, read_index=True)
    # let the requests in flight finish (a follower's take four rounds)
    for r in range(5 if ri_replica else 2):
        t.one(("drain", r), ri_replica, k=1, read_index=False)
    for s in (1, 2):
        _set_hosted(p, range(G), s, False)
    for r in range(3):  # queued at the leader: no quorum to confirm them
        e = t.one(("stopped", r), 0, k=1, read_index=True)
        assert e.ready_to_reads == 0
    for s in (1, 2):
        _set_hosted(p, range(G), s, True)
    t.one("restart", 0, k=1, read_index=True)  # the fourth ctx, heard again
    for r in range(3):  # its confirmation releases all four
        t.one(("release", r), 0, full=True, k=1, read_index=False)
    assert t.most >= 3, t.most
    for r in range(6):
        t.one(("after", r), ri_replica, full=(r == 5), k=1, read_index=True)
    assert t.served > 5 * G * READS


def test_deferred_ctx_at_a_lagging_reader():
    """A released ctx whose index is above the applied index is deferred:
    the reading follower falls behind (stopped while the others commit),
    asks on its return, and misses the rounds in which the leader's
    catch-up Replicate arrives; the ReadIndexResp it then hears carries
    the leader's commit index, above what it has applied.  (A few groups
    keep their reader throughout.)"""
    G, at = 70, 2
    t = _Reads(G)
    p = t.p
    reader = at - 1
    lag = [g for g in range(G) if g % 8 != 5]
    for r in range(2):
        t.one(("steady", r), at, k=1, read_index=False)
    _set_hosted(p, lag, reader, False)
    for r in range(4):
        t.one(("behind", r), 0, k=1, read_index=False)
    _set_hosted(p, lag, reader, True)
    t.one("ask", at, k=1, read_index=True)
    _set_hosted(p, lag, reader, False)
    for r in range(2):
        t.one(("missed", r), 0, k=1, read_index=False)
    _set_hosted(p, lag, reader, True)
    assert t.deferred == 0
    for r in range(2):
        t.one(("answer", r), at, full=True, k=1, read_index=False)
    assert t.deferred >= len(lag) * READS, t.deferred
    for r in range(4):  # heartbeats unpause the leader's remote: caught up
        t.one(("recover", r), at, tick=True, full=(r == 3), k=1,
              read_index=False)
