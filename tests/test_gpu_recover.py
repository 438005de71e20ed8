"""GPU: replicas restart from their tan logs on the device (drb_recover_tan,
drb_recover.hpp / drb_tanread.hpp): node.replayLog (node.go:666-692), newRaft
(internal/raft/raft.go:241-297) and the step loop's first apply.

An engine writes its replicas' tan logs (checked byte for byte against the
oracle's tan db, as tests/test_gpu_tan.py); a second engine of the same
configuration is recovered from those images alone and must hold what the
oracle cluster holds -- State, log, KV, writer position -- and then go on in
lock-step with it through an election and further rounds.  Logs built on the
CPU (tests/tan_images.py, the images the sanitized CPU program has read)
cover the overwrite rule, the tail rule and every refusal.
"""
import pytest

from dragonboat_amd import abi
from dragonboat_amd.engine import DrbError, Engine
from oracle import pyoracle as po
from tests import tan_images as ti
from tests.gpu_harness import Pair
from tests.test_gpu_tan import _check_round, _read_back

pytestmark = pytest.mark.gpu

SEED = 0x5EEDD8B0


def _write_phase(rounds, k_of, tan_max_log, **kw):
    """An engine / oracle pair that wrote `rounds` rounds of tan records:
    (pair, dbs, log images)."""
    p = Pair(save_tan=1, tan_max_log=tan_max_log, **kw)
    dbs = [[po.TanDB(tan_max_log) for _ in range(p.R)] for _ in range(p.G)]
    logs = {}
    for r in range(rounds):
        rkw = k_of(r)
        o, e = p.round(tick=(r % 2 == 0), encode_saves=True, **rkw)
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
        _check_round(p, dbs, logs, r)
    return p, dbs, logs


def _files(logs, G, R):
    """{(g, s): [(log number, bytes)]} of the collected images."""
    out = {(g, s): [] for g in range(G) for s in range(R)}
    for (g, s, lg) in sorted(logs):
        out[g, s].append((lg, bytes(logs[g, s, lg])))
    return out


def _model_kv(orc, g, s, base, commit):
    """The oracle's log entries (base, commit] applied in order, in Python."""
    kv = {}
    for t in orc.export_log(g, s, base + 1, commit):
        e = po._etuple_to_dict(t)
        if e["cmd"]:
            k, v = po.pbkv_unmarshal(po.get_payload(e["type"], e["cmd"]))
            kv[k] = v
    return kv


def _compare(p, e2, sts, base):
    """The recovered engine e2 against the pair's oracle and first engine."""
    for g in range(p.G):
        got = e2.export_replicas(g, 1)
        for s in range(p.R):
            st, o, a = sts[g, s], p.orc.export(g, s), got[s]
            where = (g, s, st.to_dict())
            assert st.status == abi.REC_OK, where
            assert (st.term, st.vote, st.commit) == \
                (o.prev_term, o.prev_vote, o.prev_commit), where
            assert st.last_index == o.saved_to, where
            assert st.applied == st.commit, where
            assert (a.term, a.vote, a.committed, a.last_index) == \
                (o.prev_term, o.prev_vote, o.prev_commit, o.saved_to), where
            assert (a.prev_term, a.prev_vote, a.prev_commit) == \
                (a.term, a.vote, a.committed), where
            assert (a.role, a.leader_id, a.flags, a.election_tick,
                    a.heartbeat_tick, a.tick_count, a.ri_count, a.votes) == \
                (abi.FOLLOWER, 0, abi.F_HOSTED, 0, 0, 0, 0, 0), where
            assert (a.marker_index, a.saved_to, a.applied_to_index,
                    a.applied_to_term) == (a.last_index + 1, a.last_index,
                                           0, 0), where
            assert (a.processed, a.applied, a.applied_index, a.pushed_index,
                    a.confirmed_index, a.sm_index) == (a.committed,) * 6, where
            rtt = p.eng.cfg["election_rtt"]
            assert rtt <= a.randomized_election_timeout < 2 * rtt, where
            for r in a.remotes[:p.R]:
                assert (r.match, r.next, r.state, r.active) == \
                    (0, a.last_index + 1, abi.REMOTE_RETRY, 0), where
            lo = max(base + 1, a.last_index - 7)
            assert e2.export_log(g, s, lo, a.last_index) == \
                p.orc.export_log(g, s, lo, a.last_index), where
            assert a.sm_term == p.orc.export_log(
                g, s, a.committed, a.committed)[0][0], where
            assert e2.kv_export(g, s) == \
                _model_kv(p.orc, g, s, base, a.committed), where
            assert e2.tan_get(g, s) == p.eng.tan_get(g, s), where
    assert all(row[abi.LEADER] == 0 for row in e2.role_census())
    assert sum(row[abi.FOLLOWER] for row in e2.role_census()) == p.G * p.R


def _recover(p, logs, **cfg_over):
    cfg = dict(p.eng.cfg)
    cfg.update(cfg_over)
    e2 = Engine(**cfg)
    sts = e2.recover_tan(_files(logs, p.G, p.R), base_index=p.R + 1,
                         base_term=2, seed=SEED)
    return e2, sts


def test_recover_matches_the_oracle_and_continues():
    ks = (2, 0, 3, 1, 0, 2, 3, 1, 0, 2, 1, 3, 0, 2)
    p, dbs, logs = _write_phase(
        14, lambda r: dict(k=ks[r], read_index=(r % 3 == 0)), 1024,
        G=12, R=3, elections=1, window=64, max_props=4, save_cap=4096)
    assert any(lg > 0 for (_, _, lg) in logs)  # several files per replica
    # leaders hold a saved tail that is not committed
    assert any(p.orc.export(g, 0).saved_to > p.orc.export(g, 0).prev_commit
               for g in range(p.G))
    e2, sts = _recover(p, logs)
    _compare(p, e2, sts, p.R + 1)
    # the oracle cluster restarts the same way: every replica takes the
    # recovered state, with its own log and KV
    for g in range(p.G):
        got = e2.export_replicas(g, 1)
        for s in range(p.R):
            log = [po._etuple_to_dict(t) for t in
                   p.orc.export_log(g, s, 1, got[s].last_index)]
            p.orc.import_replica(g, s, got[s], log)
    # The entries the logs continue from (1 .. R + 1: no snapshot was taken,
    # the host still has them) are made resident again with drb_import_log.
    # Without them a fresh leader whose follower rejects its first Replicate
    # leaves the fast path (DRB_FB_CAPACITY): the step kernels' pre-pass
    # bounds a rejected remote's next by its match + 1 = 1, below the
    # recovered window's start -- as in any engine whose window has moved
    # past index 1.  Seen here: 4 such leaders in the 14th round after the
    # restart, the replicas that held the unacknowledged tail.
    for g in range(p.G):
        for s in range(p.R):
            pre = [po._etuple_to_dict(t) for t in
                   p.orc.export_log(g, s, 1, p.R + 1)]
            arr, pool, n = po.EntryPool(pre).arrays()
            for i in range(n):
                arr[i].index = i + 1
            e2.import_log(g, s, arr, pool)
    first = p.eng
    p.eng = e2
    # (the oracle's outbox and ReadyToRead exports still show its last round
    # before the restart; both sides start with nothing in flight)
    assert not p.check(msgs=False, ready=False)
    rtt = p.eng.cfg["election_rtt"]
    r0 = p.rounds
    for _ in range(12 * rtt):
        o, e = p.round(k=0, tick=True, encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (p.rounds, e.to_dict(),
                                                     p.why())
        errs = p.check()
        assert not errs, (p.rounds, errs[:2])
        _check_round(p, dbs, logs, p.rounds)
        if all(sum(st.role == abi.LEADER
                   for st in p.eng.export_replicas(g, 1)) == 1
               for g in range(p.G)):
            break
    else:
        raise AssertionError("no leaders after %d rounds" % (p.rounds - r0))
    # (a leader's term-start no-op commits before client writes are taken)
    for r in range(4):
        o, e = p.round(k=0, tick=True, encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (p.rounds, p.why())
        _check_round(p, dbs, logs, p.rounds)
    for r in range(6):
        o, e = p.round(k=(1, 3, 2)[r % 3], tick=(r % 2 == 0),
                       read_index=(r % 3 == 0), encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (p.rounds, e.to_dict(),
                                                     p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), (p.rounds, e.to_dict())
        errs = p.check()
        assert not errs, (p.rounds, errs[:2])
        _check_round(p, dbs, logs, p.rounds)
    _read_back(logs, dbs)
    first.close()


@pytest.mark.parametrize("val_len,cmd_cap,val_cap", [(116, 144, 128),
                                                     (1011, 1040, 1024)])
def test_recover_long_payloads(val_len, cmd_cap, val_cap):
    """C5 payloads: records across 32 KiB blocks, out-of-line values."""
    p, dbs, logs = _write_phase(
        16, lambda r: dict(k=(1, 4, 2)[r % 3], val_len=val_len), 1 << 16,
        G=16, R=3, cmd_cap=cmd_cap, kv_val_cap=val_cap, kv_slots=64,
        max_props=4, save_cap=8192, window=64)
    if val_len > 1000:
        assert any(len(img) > 32768 for img in logs.values())
    e2, sts = _recover(p, logs)
    _compare(p, e2, sts, p.R + 1)


def test_recover_snappy():
    """entry_compression: Snappy entries are decoded by the replay's apply."""
    from tests.test_gpu_snappy import (_long_value, cid, key8, make_batch,
                                       snappy_kv)
    G = 8
    p = Pair(G=G, R=3, cmd_cap=64, kv_val_cap=1024, kv_pool_blocks=512,
             kv_slots=16, save_cap=4096, entry_compression=1, save_tan=1,
             window=64)
    dbs = [[po.TanDB() for _ in range(p.R)] for _ in range(p.G)]
    logs = {}
    for r in range(6):
        rows = {g: [(snappy_kv(key8(g % 4), _long_value(r * G + g, r % 2))[0],
                     cid(g),
                     snappy_kv(key8(g % 4), _long_value(r * G + g, r % 2))[1])]
                for g in range(G)}
        o, e = p.round(batch=make_batch(G, 1, rows, r), tick=(r % 2 == 0),
                       encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        _check_round(p, dbs, logs, r)
    e2, sts = _recover(p, logs)
    _compare(p, e2, sts, p.R + 1)
    assert any(len(v) >= 900 for v in e2.kv_export(0, 0).values())
    # without the option the same logs are refused, before the KV is touched
    e3, sts3 = _recover(p, logs, entry_compression=0)
    assert all(st.status == abi.REC_ENTRY_TYPE for st in sts3.values())
    assert e3.kv_export(0, 0) == {}


def test_recover_overwritten_and_cut_logs():
    cases = ti.recover_cases(first_shard=1)
    G = len(cases)
    cfg = dict(num_groups=G, num_replicas=3, window=ti.W, cmd_cap=ti.CMD_CAP,
               kv_val_cap=16, kv_slots=64, save_cap=4096, save_tan=1,
               tan_max_log=1024, elections=1)
    eng, fresh = Engine(**cfg), Engine(**cfg)
    files = {(g, 0): list(enumerate(fs))
             for g, (fs, _) in enumerate(cases.values()) if fs}
    sts = eng.recover_tan(files, base_index=0, base_term=0, seed=SEED)
    for g, (name, (fs, want)) in enumerate(cases.items()):
        st = sts[g, 0]
        assert st.status == want, (name, st.to_dict())
        a = eng.export_replicas(g, 1)[0]
        never = fresh.export_replicas(g, 1)[0]
        if want in (ti.OK, ti.TAIL_CUT):
            kept = fs if want == ti.OK else fs[:-1] + [fs[-1][:st.offset]]
            if want == ti.TAIL_CUT:
                # the oracle's boundary: the kept prefix reads clean, the
                # whole file does not
                assert len(po.tan_read(kept[-1])) == 2
                with pytest.raises(po.OracleError):
                    po.tan_read(fs[-1])
            state, log, kv, n = ti.replay_model(kept)
            assert (a.term, a.vote, a.committed) == state, name
            assert a.last_index == max(log) == st.last_index, name
            assert (a.flags, a.role) == (abi.F_HOSTED, abi.FOLLOWER), name
            got = eng.export_log(g, 0, 1, a.last_index)
            assert [po._etuple_to_dict(t) for t in got] == \
                [log[i] for i in range(1, a.last_index + 1)], name
            assert eng.kv_export(g, 0) == kv, name
            assert a.kv_count == n and a.sm_index == a.committed, name
            assert a.sm_term == log[a.committed]["term"], name
            assert eng.tan_get(g, 0)[:2] == (st.offset, len(fs) - 1), name
            assert st.log == len(fs) - 1 and st.offset == len(kept[-1]), name
        else:
            if want == ti.EMPTY:
                assert (a.flags, a.fallback_reason) == (0, 0), name
            else:
                assert a.flags == abi.F_FALLBACK, name
                assert a.fallback_reason == abi.FB["RECOVERY"], name
                a.flags, a.fallback_reason = never.flags, never.fallback_reason
            assert bytes(a) == bytes(never), name
            assert eng.kv_export(g, 0) == {}, name
            assert eng.tan_get(g, 0) == fresh.tan_get(g, 0), name
        # the other slots of the group had no file
        assert sts[g, 1].status == sts[g, 2].status == abi.REC_EMPTY
    over = list(cases).index("overwrite")
    assert [t[0] for t in eng.export_log(over, 0, 1, 8)] == [2] * 5 + [3] * 3


def test_recover_in_group_ranges():
    p, dbs, logs = _write_phase(
        8, lambda r: dict(k=(2, 1, 3, 0)[r % 4]), 1024,
        G=10, R=3, window=64, max_props=4, save_cap=4096)
    e1, s1 = _recover(p, logs)
    e2 = Engine(**p.eng.cfg)
    files = _files(logs, p.G, p.R)
    s2 = {}
    for g0, n in ((0, 4), (4, 6)):
        part = {k: v for k, v in files.items() if g0 <= k[0] < g0 + n}
        s2.update(e2.recover_tan(part, p.R + 1, 2, SEED, first_group=g0,
                                 n_groups=n))
    assert {k: v.to_dict() for k, v in s1.items()} == \
        {k: v.to_dict() for k, v in s2.items()}
    for g in range(p.G):
        a, b = e1.export_replicas(g, 1), e2.export_replicas(g, 1)
        for s in range(p.R):
            assert bytes(a[s]) == bytes(b[s]), (g, s)
            assert e1.kv_export(g, s) == e2.kv_export(g, s), (g, s)
            assert e1.export_log(g, s, p.R + 2, a[s].last_index) == \
                e2.export_log(g, s, p.R + 2, a[s].last_index), (g, s)
            assert e1.tan_get(g, s) == e2.tan_get(g, s)
    _compare(p, e2, s2, p.R + 1)


def test_recover_preconditions():
    cfg = dict(num_groups=4, num_replicas=3, window=64, save_cap=4096,
               save_tan=1, kv_val_cap=16)
    files = {(0, 0): [(0, ti.write_logs(ti.steady_updates(3), 1, 1)[0])]}
    eng = Engine(**cfg)
    sts = eng.recover_tan(files, 0, 0, SEED, first_group=0, n_groups=1)
    assert sts[0, 0].status == abi.REC_OK
    # a value the KV does not take stops the apply: the one status reached
    # after the KV was touched
    small = Engine(**dict(cfg, kv_val_cap=4))
    st = small.recover_tan(files, 0, 0, SEED)[0, 0]
    assert (st.status, st.applied) == (abi.REC_APPLY_STOPPED, 0)
    a = small.export_replicas(0, 1)[0]
    assert (a.flags, a.fallback_reason) == (abi.F_FALLBACK,
                                            abi.FB["RECOVERY"])
    eng.recover_tan({}, 0, 0, SEED, first_group=1, n_groups=3)  # repeatable
    # ... over disjoint ranges: a group is recovered once (its log would be
    # applied into the KV again)
    kv, count = eng.kv_export(0, 0), eng.export(0, 0).kv_count
    for g0, n in ((0, 4), (0, 1), (3, 1)):
        with pytest.raises(DrbError, match="status -1"):
            eng.recover_tan(files if g0 == 0 else {}, 0, 0, SEED,
                            first_group=g0, n_groups=n)
    assert (eng.kv_export(0, 0), eng.export(0, 0).kv_count) == (kv, count)
    eng.step(tick=True)
    with pytest.raises(DrbError, match="status -1"):
        eng.recover_tan(files, 0, 0, SEED)
    mux = Engine(tan_multiplexed=1, **cfg)
    with pytest.raises(DrbError, match="status -1"):
        mux.recover_tan(files, 0, 0, SEED)
    # a file table that points outside the bytes, or is out of log order
    e3 = Engine(**cfg)
    with pytest.raises(DrbError, match="status -5"):
        e3.recover_tan({(9, 0): files[0, 0]}, 0, 0, SEED)
    with pytest.raises(DrbError, match="status -1"):
        e3.recover_tan({(0, 0): [(1, b""), (0, b"")]}, 0, 0, SEED)
