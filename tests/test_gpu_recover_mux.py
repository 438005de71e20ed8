"""GPU: replicas of a tan_multiplexed engine restart from their slot's 16
shared logs on the device (drb_recover_tan_mux, drb_recover_mux.hpp /
drb_tanmux.hpp): the logs are indexed by 32 KiB blocks, their records handed
to the replicas that own them, and each replica replayed as drb_recover_tan
replays a log of its own.

An engine writes the multiplexed logs (checked byte for byte against the
oracle's shared dbs, as tests/test_gpu_tan.py); a second engine is recovered
from the dbs' files and must hold what the oracle cluster holds, then go on
in lock-step with it and with the SAME dbs.  Logs built on the CPU
(tests/tan_mux_images.py, the images the sanitized CPU program has read)
cover the equivalence with the regular format and every refusal.
"""
import pytest

from dragonboat_amd import abi
from dragonboat_amd.engine import DrbError, Engine
from oracle import pyoracle as po
from tests import tan_images as ti
from tests import tan_mux_images as tm
from tests.gpu_harness import Pair
from tests.test_gpu_recover import SEED, _compare
from tests.test_gpu_tan import _mux_round

pytestmark = pytest.mark.gpu


def _write_phase(rounds, k_of, max_log, **kw):
    """A multiplexed engine / oracle pair that wrote `rounds` rounds:
    (pair, the oracle's shared dbs [slot][key])."""
    p = Pair(save_tan=1, tan_multiplexed=1, tan_max_log=max_log, **kw)
    dbs = [[po.TanDB(max_log) for _ in range(16)] for _ in range(p.R)]
    for r in range(rounds):
        o, e = p.round(encode_saves=True, **k_of(r))
        assert e.fallbacks == 0 and e.errors == 0, (r, e.to_dict(), p.why())
        _mux_round(p, dbs, r)
    return p, dbs


def _files(dbs):
    """{(slot, key): [(log number, bytes)]} of the dbs that wrote."""
    out = {}
    for s, row in enumerate(dbs):
        for c, db in enumerate(row):
            last = db.last()
            if last["log"] or last["offset"]:
                out[s, c] = [(lg, db.file(lg)) for lg in range(last["log"] + 1)]
    return out


def _recover(p, files, **cfg_over):
    cfg = dict(p.eng.cfg)
    cfg.update(cfg_over)
    e2 = Engine(**cfg)
    sts, lst = e2.recover_tan_mux(files, base_index=p.R + 1, base_term=2,
                                  seed=SEED)
    return e2, sts, lst


def _logs_ok(p, files, lst):
    first = p.eng.cfg["first_shard_id"]
    for (s, c), l in lst.items():
        if (s, c) not in files:
            assert l.status == abi.REC_EMPTY, (s, c, l.to_dict())
            continue
        assert l.status == abi.REC_OK, (s, c, l.to_dict())
        g = next(g for g in range(p.G) if (first + g) % 16 == c)
        assert (l.offset, l.log) == p.eng.tan_get(g, s)[:2], (s, c)
        assert l.records == sum(len(po.tan_read(f)) for _, f in files[s, c])


def test_recover_mux_matches_the_oracle_and_continues():
    ks = (2, 0, 3, 1, 0, 2, 3, 1, 0, 2, 1, 3, 0, 2)
    p, dbs = _write_phase(
        14, lambda r: dict(k=ks[r], read_index=(r % 3 == 0),
                           tick=(r % 2 == 0)), 2048,
        G=40, R=3, elections=1, window=64, max_props=4, save_cap=8192)
    files = _files(dbs)
    assert any(len(fs) > 1 for fs in files.values())   # a log switched files
    assert any(p.orc.export(g, 0).saved_to > p.orc.export(g, 0).prev_commit
               for g in range(p.G))
    e2, sts, lst = _recover(p, files)
    _compare(p, e2, sts, p.R + 1)
    _logs_ok(p, files, lst)
    # the oracle cluster restarts the same way
    # (tests/test_gpu_recover.py::test_recover_matches_the_oracle_and_continues)
    for g in range(p.G):
        got = e2.export_replicas(g, 1)
        for s in range(p.R):
            log = [po._etuple_to_dict(t) for t in
                   p.orc.export_log(g, s, 1, got[s].last_index)]
            p.orc.import_replica(g, s, got[s], log)
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
    assert not p.check(msgs=False, ready=False)
    rtt = p.eng.cfg["election_rtt"]
    r0 = p.rounds
    for _ in range(12 * rtt):
        o, e = p.round(k=0, tick=True, encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (p.rounds, e.to_dict(),
                                                     p.why())
        errs = p.check()
        assert not errs, (p.rounds, errs[:2])
        _mux_round(p, dbs, p.rounds)
        if all(sum(st.role == abi.LEADER
                   for st in p.eng.export_replicas(g, 1)) == 1
               for g in range(p.G)):
            break
    else:
        raise AssertionError("no leaders after %d rounds" % (p.rounds - r0))
    for r in range(4):   # the term-start no-op commits
        o, e = p.round(k=0, tick=True, encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (p.rounds, p.why())
        _mux_round(p, dbs, p.rounds)
    for r in range(6):
        o, e = p.round(k=(1, 3, 2)[r % 3], tick=(r % 2 == 0),
                       read_index=(r % 3 == 0), encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (p.rounds, e.to_dict(),
                                                     p.why())
        assert (e.committed_entries, e.messages) == \
            (o.committed_entries, o.messages), (p.rounds, e.to_dict())
        errs = p.check()
        assert not errs, (p.rounds, errs[:2])
        _mux_round(p, dbs, p.rounds)
    first.close()


def test_recover_mux_long_payloads():
    """1 KB payloads in 64 KiB logs: files of several blocks, records across
    block boundaries."""
    p, dbs = _write_phase(
        24, lambda r: dict(k=(0, 1, 3, 0, 2)[r % 5], tick=(r % 2 == 0),
                           read_index=(r % 3 == 0), val_len=1011), 1 << 16,
        G=40, R=3, cmd_cap=1040, kv_val_cap=1024, kv_slots=64, max_props=4,
        save_cap=8192, window=64)
    files = _files(dbs)
    imgs = [f for fs in files.values() for _, f in fs]
    assert any(len(f) > 32768 for f in imgs)
    assert any(f[b + 6] in (3, 4) for f in imgs
               for b in range(32768, len(f) - 6, 32768))
    e2, sts, lst = _recover(p, files)
    _compare(p, e2, sts, p.R + 1)
    _logs_ok(p, files, lst)


CFG = dict(num_replicas=3, window=ti.W, cmd_cap=ti.CMD_CAP, kv_val_cap=16,
           kv_slots=64, save_cap=4096, save_tan=1, tan_max_log=1024,
           elections=1)


def test_recover_mux_equals_the_regular_recovery():
    lists = tm.equivalence_lists(first_shard=1)
    G = tm.KEYS * len(lists)
    reg = Engine(num_groups=G, **CFG)
    mux = Engine(num_groups=G, tan_multiplexed=1, **CFG)
    own = {(shard - 1, 0): list(enumerate(ti.write_logs(ups, shard, 1, 1024)))
           for shard, ups in lists.items()}
    s1 = reg.recover_tan(own, 0, 0, SEED)
    shared = tm.shared_logs(lists, 1, 1024)
    assert list(shared) == [1] and len(shared[1]) >= 4
    s2, lst = mux.recover_tan_mux({(0, 1): list(enumerate(shared[1]))}, 0, 0,
                                  SEED)
    assert lst[0, 1].status == abi.REC_OK
    assert (lst[0, 1].log, lst[0, 1].offset) == (len(shared[1]) - 1,
                                                 len(shared[1][-1]))
    statuses = set()
    for g in range(G):
        a, b = s1[g, 0], s2[g, 0]
        da, db = a.to_dict(), b.to_dict()
        for f in ("log", "offset"):          # the writer is the log's
            da.pop(f), db.pop(f)
        assert da == db, (g, da, db)
        statuses.add(a.status)
        ra, rb = reg.export_replicas(g, 1)[0], mux.export_replicas(g, 1)[0]
        assert bytes(ra) == bytes(rb), g
        assert reg.kv_export(g, 0) == mux.kv_export(g, 0), g
        if a.status == abi.REC_OK and a.last_index:
            assert reg.export_log(g, 0, 1, a.last_index) == \
                mux.export_log(g, 0, 1, a.last_index), g
        assert reg.tan_get(g, 0)[2] == mux.tan_get(g, 0)[2], g
        if (1 + g) % 16 == 1:
            assert mux.tan_get(g, 0)[:2] == (lst[0, 1].offset, lst[0, 1].log)
    assert statuses == {abi.REC_OK, abi.REC_CAPACITY, abi.REC_EMPTY}


def _untouched(eng, fresh, g, s, flagged, where, writer=None):
    """Replica (g, s) is bytewise a fresh engine's apart from the fallback
    mark, its KV empty; writer: (offset, log) of its log where that stands
    (the log's writer is shared, the replica's stored State stays empty)."""
    a, never = eng.export_replicas(g, 1)[s], fresh.export_replicas(g, 1)[s]
    if flagged:
        assert (a.flags, a.fallback_reason) == \
            (abi.F_FALLBACK, abi.FB["RECOVERY"]), where
        a.flags, a.fallback_reason = never.flags, never.fallback_reason
    assert bytes(a) == bytes(never), where
    assert eng.kv_export(g, s) == {}, where
    assert eng.tan_get(g, s) == (fresh.tan_get(g, s) if writer is None
                                 else writer + (0,)), where


def test_recover_mux_log_refusals():
    """CPU case 3 on the device: slot 1 (ReplicaID 2), shards 5, 21, 37."""
    lists = {s: ti.steady_updates(12, first=1) for s in (5, 21, 37)}
    files = tm.write_shared(tm.interleave(lists), 2, 1024)
    host = ti.hostile_records()
    flip = bytearray(files[0])
    flip[po.tan_read(files[0])[1][0] + ti.HDR + 12] ^= 0x10
    mid = po.tan_read(files[0])[2][0] + 9
    tail = lambda rec: files[:-1] + [files[-1] + rec]
    rec = lambda shard, rep: ti.record(po.update_marshal(shard, rep,
                                                         (2, 1, 1), []))
    last = po.tan_read(files[-1])
    cut = files[:-1] + [files[-1][:last[2][0] + 9]]
    cases = {
        "crc_early": ([bytes(flip)] + files[1:], ti.CORRUPT),
        "invalid_early": ([files[0][:mid]] + files[1:], ti.CORRUPT),
        "ids": (tail(ti.record(host["uvarint_11_bytes"])), ti.CORRUPT),
        "other_key": (tail(rec(6, 2)), ti.MISMATCH),
        "other_replica": (tail(rec(21, 3)), ti.MISMATCH),
        "tail_cut": (cut, ti.TAIL_CUT),
        "body": (tail(ti.record(host["state_len_max"])), ti.OK),
    }
    G = 33
    cfg = dict(CFG, num_groups=G, first_shard_id=5, tan_multiplexed=1)
    fresh = Engine(**cfg)
    gs = [s - 5 for s in lists]
    for name, (fs, want) in cases.items():
        eng = Engine(**cfg)
        sts, lst = eng.recover_tan_mux({(1, 5): list(enumerate(fs))}, 0, 0,
                                       SEED)
        l = lst[1, 5]
        assert l.status == want, (name, l.to_dict())
        if want in (ti.CORRUPT, ti.MISMATCH):
            for g in gs:
                assert sts[g, 1].status == want, (name, g)
                _untouched(eng, fresh, g, 1, True, (name, g))
            continue
        kept = files if name == "body" else fs  # (less the hostile record)
        if want == ti.TAIL_CUT:
            assert (l.log, l.offset) == (len(fs) - 1, last[2][0]), name
            kept = fs[:-1] + [fs[-1][:l.offset]]
            assert len(po.tan_read(kept[-1])) == 2
            with pytest.raises(po.OracleError):
                po.tan_read(fs[-1])
        for g in gs:
            st = sts[g, 1]
            if name == "body" and g == 0:    # the record's replica alone
                assert st.status == ti.CORRUPT, st.to_dict()
                _untouched(eng, fresh, g, 1, True, (name, g),
                           (l.offset, l.log))
                continue
            assert st.status == ti.OK, (name, g, st.to_dict())
            # the replica's own records of the kept files, as a model
            recs = [pay for f in kept for _, pay in po.tan_read(f)]
            state, log, kv = _model(recs, 5 + g)
            a = eng.export_replicas(g, 1)[1]
            assert (a.term, a.vote, a.committed) == state, (name, g)
            assert a.last_index == max(log) == st.last_index, (name, g)
            assert eng.kv_export(g, 1) == kv, (name, g)
            assert eng.tan_get(g, 1)[:2] == (l.offset, l.log), (name, g)
        # every other replica of the engine: no record, untouched
        assert sts[1, 1].status == sts[0, 0].status == abi.REC_EMPTY
        _untouched(eng, fresh, 1, 1, False, name)
        eng.close()


def _model(payloads, shard):
    """(state, {index: entry}, kv) of the Updates of `shard` among the
    payloads, by the overwrite rule (as ti.replay_model)."""
    from tests.test_oracle_tan import _decode_update
    log, state = {}, None
    for pay in payloads:
        sh, _, st, ents = _decode_update(pay)
        if sh != shard:
            continue
        if ents:
            for i in [i for i in log if i >= ents[0]["index"]]:
                del log[i]
            for e in ents:
                log[e["index"]] = e
        if st is not None:
            state = st
    kv = {}
    for i in range(1, state[2] + 1):
        k, v = po.pbkv_unmarshal(po.get_payload(log[i]["type"],
                                                log[i]["cmd"]))
        kv[k] = v
    return state, log, kv


def test_recover_mux_replica_refusals():
    """CPU case 4 on the device: ti.recover_cases(), a shard each, in one
    log."""
    lists, want = tm.replica_case_lists(first_shard=1)
    G = tm.KEYS * len(lists)
    cfg = dict(CFG, num_groups=G, tan_multiplexed=1)
    eng, fresh = Engine(**cfg), Engine(**cfg)
    shared = tm.shared_logs(lists, 1, 1024)
    sts, lst = eng.recover_tan_mux({(0, 1): list(enumerate(shared[1]))}, 0, 0,
                                   SEED)
    assert lst[0, 1].status == abi.REC_OK
    cases = ti.recover_cases()
    for shard, (name, status) in want.items():
        g, st = shard - 1, sts[shard - 1, 0]
        assert st.status == status, (name, st.to_dict())
        if status == ti.OK:
            state, log, kv, n = ti.replay_model(cases[name][0])
            a = eng.export_replicas(g, 1)[0]
            assert (a.term, a.vote, a.committed) == state, name
            assert a.last_index == max(log) == st.last_index, name
            got = eng.export_log(g, 0, 1, a.last_index)
            assert [po._etuple_to_dict(t) for t in got] == \
                [log[i] for i in range(1, a.last_index + 1)], name
            assert eng.kv_export(g, 0) == kv, name
            assert a.kv_count == n and a.sm_index == a.committed, name
        else:
            _untouched(eng, fresh, g, 0, status != ti.EMPTY, name,
                       (lst[0, 1].offset, lst[0, 1].log))


def test_recover_mux_snappy():
    """The rounds of test_recover_snappy on a multiplexed pair."""
    from tests.test_gpu_snappy import (_long_value, cid, key8, make_batch,
                                       snappy_kv)
    G = 16
    p = Pair(G=G, R=3, cmd_cap=64, kv_val_cap=1024, kv_pool_blocks=512,
             kv_slots=16, save_cap=4096, entry_compression=1, save_tan=1,
             tan_multiplexed=1, window=64)
    dbs = [[po.TanDB() for _ in range(16)] for _ in range(p.R)]
    for r in range(6):
        rows = {g: [(snappy_kv(key8(g % 4), _long_value(r * G + g, r % 2))[0],
                     cid(g),
                     snappy_kv(key8(g % 4), _long_value(r * G + g, r % 2))[1])]
                for g in range(G)}
        o, e = p.round(batch=make_batch(G, 1, rows, r), tick=(r % 2 == 0),
                       encode_saves=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        _mux_round(p, dbs, r)
    files = _files(dbs)
    e2, sts, lst = _recover(p, files)
    _compare(p, e2, sts, p.R + 1)
    _logs_ok(p, files, lst)
    assert any(len(v) >= 900 for v in e2.kv_export(0, 0).values())
    e3, sts3, lst3 = _recover(p, files, entry_compression=0)
    assert all(st.status == abi.REC_ENTRY_TYPE for st in sts3.values())
    assert all(l.status == abi.REC_OK for l in lst3.values())
    assert all(e3.kv_export(g, 0) == {} for g in range(G))


def test_recover_mux_preconditions():
    cfg = dict(num_groups=4, num_replicas=3, window=64, save_cap=4096,
               save_tan=1, kv_val_cap=16)
    img = ti.write_logs(ti.steady_updates(3), 1, 1)[0]
    files = {(0, 1): [(0, img)]}

    def state(e):
        return (e.kv_export(0, 0), bytes(e.export_replicas(0, 1)[0]),
                e.tan_get(0, 0))

    def refused(e, status, fs=files):
        before = state(e)
        with pytest.raises(DrbError, match="status %d" % status):
            e.recover_tan_mux(fs, 0, 0, SEED)
        assert state(e) == before

    refused(Engine(**cfg), -1)                       # a regular engine
    stepped = Engine(tan_multiplexed=1, **cfg)
    stepped.step(tick=True)
    refused(stepped, -1)
    eng = Engine(tan_multiplexed=1, **cfg)
    refused(eng, -1, {(0, 1): [(1, img), (0, img)]})  # out of log order
    refused(eng, -5, {(0, 16): [(0, img)]})           # key >= 16
    refused(eng, -5, {(3, 1): [(0, img)]})            # slot >= R
    before = state(eng)
    blob = (abi.TanMuxFile * 1)(abi.TanMuxFile(0, 1, 0, 0, 8, len(img)))
    import ctypes as C
    from dragonboat_amd.engine import _u8, lib
    buf = _u8(bytearray(img))
    rin = abi.RecoverMuxIn(C.cast(buf, C.c_void_p), len(img), blob, 1, 0, 0,
                           SEED)
    st = (abi.RecoverStatus * 12)()
    lst = (abi.RecoverLogStatus * 48)()
    assert lib().drb_recover_tan_mux(eng.h, C.byref(rin), st, lst) == -5
    assert state(eng) == before                       # a file outside bytes
    sts, lsts = eng.recover_tan_mux(files, 0, 0, SEED)
    assert sts[0, 0].status == abi.REC_OK and lsts[0, 1].status == abi.REC_OK
    assert eng.kv_export(0, 0)
    refused(eng, -1)                                  # a second call
    before = state(eng)
    with pytest.raises(DrbError, match="status -1"):
        eng.recover_tan({(0, 0): [(0, img)]}, 0, 0, SEED)
    assert state(eng) == before
