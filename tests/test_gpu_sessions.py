"""GPU: client sessions on the device (drb_config.session_slots /
session_history; dragonboat_amd/csrc/drb_session.hpp): register, unregister
and at-most-once updates applied by the step kernels, the per-entry results
(drb_apply_results), the hand-over (drb_sessions_export / _import) and the
restart from tan logs.

The C oracle panics on session-managed entries, so every round is checked in
two parts (tests/session_harness.py): the oracle stepped on a no-op twin of
the batch for everything raft, and tests/session_model.py -- the reference's
session code in plain Python, pinned by the reference's own tests in
tests/test_session_model.py -- for the state machine.
"""
import pytest

from dragonboat_amd import abi, workload
from dragonboat_amd.engine import DrbError, Engine
from oracle import pyoracle as po
from tests import session_model as sm
from tests import tan_images as ti
from tests import tan_mux_images as tm
from tests.session_harness import (REG, UNREG, SessPair, cl, ent, pbkv,
                                   script_rounds, val)
from tests.test_gpu_elections import _unhost

pytestmark = pytest.mark.gpu

G = 96  # a full wave and a partial one
SEED = 0x5EEDD8B0
ALL = {(w, s) for w in (0, 1) for s in range(3)}


def lifecycle(g):
    """The twelve steps of a group's script."""
    A, B, U = cl(g, 0), cl(g, 1), cl(g, 2)
    k1, k2, k3, v = b"a%d" % (g % 7), b"b", b"c", val(g)
    return [
        ent(A, REG),                      # 1 register
        ent(A, 1, 0, pbkv(k1, v)),        # 2 series 1
        ent(A, 1, 0, pbkv(k1, v)),        # 3 again: cached
        ent(A, 2, 1, pbkv(k2, v)),        # 4 series 2, responded_to 1
        ent(A, 1, 1, pbkv(k1, v)),        # 5 series 1 again: responded
        ent(U, 1, 0, pbkv(k3, v)),        # 6 an unregistered client
        ent(A, REG),                      # 7 a duplicate register
        ent(B, REG),                      # 8 a second client
        ent(A, UNREG),                    # 9 unregister
        ent(A, UNREG),                    # 10 again: rejected
        ent(U, 0, 0, pbkv(k3, v)),        # 11 NoOP session, unregistered
        ent(0, 0),                        # 12 an empty no-op
    ]


def run_script(p, steps, per_round=3, drain=4, **kw):
    """Group g's steps, per_round a round, its phase g % 4 rounds late;
    ticks and ReadIndex rounds mixed in; every round checked."""
    for rows, tick, ri in script_rounds(p.G, steps, per_round, drain):
        p.sess_round(rows, tick=tick, read_index=ri, **kw)
    for g in range(p.G):
        sts = p.eng.export_replicas(g, 1)
        assert all(a.sm_index == a.last_index == sts[0].last_index
                   for a in sts), g


def test_device_bytes_count_the_session_arrays():
    """drb_engine_device_bytes: the tables [R][S][2 + H][G] x 16 B and the
    outcome ring [R][W][G] x 8 B, and nothing without the option."""
    kw = dict(num_groups=64, num_replicas=3, window=32)
    a = Engine(**kw)
    b = Engine(session_slots=16, session_history=8, **kw)
    assert b.device_bytes - a.device_bytes == \
        3 * 16 * 10 * 64 * 16 + 3 * 32 * 64 * 8
    a.close()
    b.close()


# ------------------------------------------------------------ 1: lifecycle
def test_session_lifecycle_in_one_wave():
    p = SessPair(G, R=3, session_slots=4, session_history=2)
    run_script(p, lifecycle)
    want = {"registered", "update", "cached", "responded", "unknown-client",
            "register-duplicate", "unregistered", "unregister-unknown",
            "noop-session", "noop"}
    # every outcome class in both waves and on all three replicas
    assert set(p.classes) == want, set(p.classes) ^ want
    assert all(p.classes[c] == ALL for c in want), p.classes
    # the leader's drb_apply_results were compared for every entry of every
    # group (two registers and two updates in a script), and the engine
    # itself reported each kind of answer: seven values, three rejected, two
    # ignored (the responded one and the empty no-op)
    twice = ("registered", "update")
    assert p.compared == {c: (2 if c in twice else 1) * G for c in want}, \
        p.compared
    assert p.reported == {(True, 0): 7 * G,
                          (False, abi.APPLY_REJECTED): 3 * G,
                          (False, abi.APPLY_IGNORED): 2 * G}, p.reported
    for g in (0, 1, 66, 95):
        res = [p.results[g][i] for i in sorted(p.results[g])
               if i > p.base[g]]
        by = {}
        for (r, cls, _) in res:
            by.setdefault(cls, []).append(r)
        # the cached result is the first one's; one real update per series
        assert by["cached"] == [by["update"][0]], (g, by)
        assert p.snaps[g][max(p.snaps[g])][1] == 3, g  # KVTest.Count
        assert [c for c, _, _ in p.snaps[g][max(p.snaps[g])][2]] == \
            [cl(g, 1)], g


def test_session_entries_fall_back_without_the_option():
    """Contrast: the same first batch on an engine with session_slots = 0
    falls back DRB_FB_ENTRY_TYPE before the append."""
    p = SessPair(8, R=3)
    before = [a.last_index for a in p.eng.export_replicas(0, 8)]
    p.stage_rows({g: lifecycle(g)[:3] for g in range(8)})
    e = p.eng.step(prop_slot=0)
    assert e.fallbacks == 8, e.to_dict()
    recs, _ = p.eng.take_flagged()
    assert sorted((g, s, reason) for (g, s, reason, *_r) in recs) == \
        [(g, 0, abi.FB["ENTRY_TYPE"]) for g in range(8)]
    assert [a.last_index for a in p.eng.export_replicas(0, 8)] == before
    with pytest.raises(DrbError, match="status -1"):
        p.eng.sessions_export(0, 0)


# ------------------------------------------------------------- 2: capacity
def capacity_steps(g):
    """S = 2, H = 1.  Even groups: a third register; odd groups: series 2
    with responded_to = 0 while series 1 is cached.  The entry in front of
    the full one applies in the same round."""
    A, B, Cc = cl(g, 0), cl(g, 1), cl(g, 2)
    v = val(g)
    if g % 2 == 0:
        return [[ent(A, REG), ent(A, 1, 0, pbkv(b"x", v))],
                [ent(B, REG), ent(B, 1, 0, pbkv(b"y", v))],
                [ent(A, 2, 1, pbkv(b"z", v)), ent(Cc, REG)]]
    return [[ent(A, REG), ent(A, 1, 0, pbkv(b"x", v))],
            [ent(B, REG)],
            [ent(B, 1, 0, pbkv(b"y", v)), ent(A, 2, 0, pbkv(b"z", v))]]


def test_session_capacity_stops_the_apply():
    p = SessPair(G, R=3, session_slots=2, session_history=1)
    for r in range(2):
        p.sess_round({g: capacity_steps(g)[r] for g in range(G)},
                     tick=(r == 0))
    for r in range(4):
        p.sess_round(tick=(r % 2 == 1))
    first = p.eng.export_replicas(0, G)
    full = [first[g * 3].last_index + 2 for g in range(G)]  # the full entry
    p.sess_round({g: capacity_steps(g)[2] for g in range(G)})
    stopped, lead_round = {}, None
    for r in range(8):
        o = p.orc.round(tick=False)
        e = p.eng.step(tick=False)
        p.rounds += 1
        assert e.errors == 0, e.to_dict()
        sts = p.eng.export_replicas(0, G)
        p.advance_model(sts)
        for g in range(G):
            for s in range(3):
                a = sts[g * 3 + s]
                if (g, s) in stopped or not a.flags & abi.F_FALLBACK:
                    continue
                stopped[g, s] = r
                w = (r, g, s)
                assert a.flags == abi.F_HOSTED | abi.F_FALLBACK | \
                    abi.F_APPLY_STOPPED, (w, a.flags)
                assert a.fallback_reason == abi.FB["CAPACITY"], w
                assert a.sm_index == full[g] - 1, (w, a.sm_index, full[g])
                # the table and the KV as the model has them just before
                p.check_sm(g, s, a, w)
        lead_now = [g for g in range(G) if stopped.get((g, 0)) == r]
        if lead_now:
            # the entries applied before the stop are reported
            assert len(lead_now) == G and lead_round is None
            lead_round = r
            got = {}
            for (g, idx, key, cid, series, value, ign) in \
                    p.eng.apply_results(0):
                got.setdefault(g, []).append((idx, key, value, ign))
            for g in range(G):
                i = full[g] - 1
                res, cls, key = p.results[g][i]
                assert cls == "update" and got[g] == [(i, key, res[0], 0)], \
                    (g, got[g], p.results[g][i])
        if len(stopped) == 3 * G:
            break
    assert len(stopped) == 3 * G, len(stopped)
    # nothing of the full entry reached the model's replay either
    assert all(max(p.snaps[g]) == full[g] - 1 for g in range(G))


# -------------------------------------------------------- 3: import/export
def test_sessions_import_export_round_trip():
    p = SessPair(G, R=3, session_slots=4, session_history=2)

    def table(g):
        A, B, Cc = cl(g, 0), cl(g, 1), cl(g, 2)
        return [(A, 3, {4: 40 + g, 5: 50}), (B, 0, {}), (Cc, 7, {9: 2 ** 62 - 1})]

    for g in range(G):
        for s in range(3):
            p.eng.sessions_import(g, s, table(g))
            assert p.eng.sessions_export(g, s) == table(g), (g, s)
        # the model takes the same table, in the same order
        for (c, upto, hist) in table(g):
            ses = sm.Session(c)
            ses.responded_up_to, ses.history = upto, dict(hist)
            p.model[g].lru.add(ses)
        p.snaps[g][p.base[g]] = p.model[g].snapshot()
    p.sm_seen.clear()

    def steps(g):
        A, B, Cc = cl(g, 0), cl(g, 1), cl(g, 2)
        v = val(g)
        return [ent(A, 5, 3, pbkv(b"k", v)),   # served from the import
                ent(B, 1, 0, pbkv(b"k", v)),   # B becomes the most recent
                ent(A, 6, 4, pbkv(b"m", v)),   # clearTo drops series 4
                ent(Cc, REG)]                  # a duplicate register: a use
    run_script(p, steps, per_round=2, drain=3)
    for g in (0, 65):
        by = {cls: r for (r, cls, _) in p.results[g].values()}
        assert by["cached"] == (50, False, False), by
        assert [c for c, _, _ in p.eng.sessions_export(g, 1)] == \
            [cl(g, 1), cl(g, 0), cl(g, 2)], g
    assert {"cached", "update", "register-duplicate"} <= set(p.classes)
    # what the import refuses leaves the table unchanged
    A = cl(0, 0)
    bad = [
        [(c, 0, {}) for c in (1, 2, 3, 4, 5)],       # more than S sessions
        [(A, 0, {1: 1, 2: 2, 3: 3})],                # more than H responses
        [(A, 0, {1: 2 ** 62})],                      # a value >= 2^62
        [(0, 0, {})],                                # a zero client_id
        [(A, 0, {}), (A, 0, {})],                    # a repeated client_id
    ]
    for s in range(3):
        have = p.eng.sessions_export(0, s)
        for tbl in bad:
            with pytest.raises(DrbError, match="status -5"):
                p.eng.sessions_import(0, s, tbl)
            assert p.eng.sessions_export(0, s) == have, tbl
    # the state and KV imports do not touch the sessions
    have = p.eng.sessions_export(5, 0)
    p.eng.import_replicas(5, p.eng.export_replicas(5, 1))
    p.eng.kv_import(5, 0, p.eng.kv_export(5, 0))
    assert p.eng.sessions_export(5, 0) == have
    # the step worker's one-word records cannot carry session results
    with pytest.raises(DrbError, match="status -1"):
        p.eng.worker_export(0, abi.WorkerBufs())


# ------------------------------------------------------------- 4: failover
def test_retry_after_failover_is_not_applied_twice():
    p = SessPair(G, R=3, elections=1, session_slots=4, session_history=2)
    E = [g for g in range(G) if g % 4 == 1]  # in both waves
    v = {g: pbkv(b"k", val(g)) for g in range(G)}
    p.sess_round({g: [ent(cl(g, 0), REG), ent(cl(g, 0), 1, 0, v[g])]
                  for g in range(G)}, tick=True)
    for r in range(4):
        p.sess_round(tick=True)
    for g in range(G):
        assert all(a.sm_index == a.last_index
                   for a in p.eng.export_replicas(g, 1)), g
    for r in range(2):  # quiet rounds
        p.sess_round()
    count = {g: p.eng.export(g, 1).kv_count for g in E}
    assert set(count.values()) == {1}
    _unhost(p, E, 0)

    def leaders(g):
        return [s for s, a in enumerate(p.eng.export_replicas(g, 1))
                if s and a.role == abi.LEADER]

    rest = [g for g in range(G) if g not in E]
    for r in range(60):
        # nothing is staged for the stopped leaders' groups
        p.sess_round({g: [ent(cl(g, 0), 0, 0, v[g])] for g in rest}
                     if r % 5 == 0 else None, tick=True)
        if all(len(leaders(g)) == 1 for g in E):
            break
    assert all(len(leaders(g)) == 1 for g in E)
    for r in range(3):  # the new leaders' term-start no-ops commit
        p.sess_round(tick=True)
    # the client resends series 1 to the new leader, then goes on
    p.sess_round({g: [ent(cl(g, 0), 1, 0, v[g])] for g in E}, tick=True)
    for r in range(4):
        p.sess_round(tick=True)
    for g in E:
        res = [x for x in p.results[g].values() if x[1] == "cached"]
        assert [r for r, _, _ in res] == [(len(v[g]), False, False)], (g, res)
        for s in (1, 2):
            a = p.eng.export(g, s)
            assert a.kv_count == count[g] and a.sm_index == a.last_index, \
                (g, s)
    p.sess_round({g: [ent(cl(g, 0), 2, 1, v[g])] for g in E}, tick=True)
    for r in range(4):
        p.sess_round(tick=True)
    for g in E:
        assert all(p.eng.export(g, s).kv_count == count[g] + 1
                   for s in (1, 2)), g
    assert p.classes["cached"] >= {(w, s) for w in (0, 1) for s in (1, 2)}


# ------------------------------------------------------------ 5: forwarded
def test_forwarded_session_proposals():
    p = SessPair(G, R=3, forward_proposals=1, session_slots=4,
                 session_history=2)
    run_script(p, lambda g: lifecycle(g)[:6], drain=6, prop_replica=2)
    want = {"registered", "update", "cached", "responded", "unknown-client"}
    assert set(p.classes) >= want and all(p.classes[c] == ALL for c in want), \
        p.classes
    assert p.compared == {c: (2 if c == "update" else 1) * G for c in want}, \
        p.compared


# -------------------------------------------------------------- 6: restart
def session_updates(g, first=1, term=2):
    """The tan Updates of group g's replicas from a session script: one
    entry a record, the commit one behind, then a State that commits the
    rest.  Returns (updates, entries)."""
    A, B, U = cl(g, 0), cl(g, 1), cl(g, 2)
    v = val(g)
    script = [(A, REG, 0, b""), (A, 1, 0, pbkv(b"k1", v)),
              (A, 1, 0, pbkv(b"k1", v)), (B, REG, 0, b""),
              (A, 2, 1, pbkv(b"k2", v)), (A, 1, 1, pbkv(b"k1", v)),
              (U, 3, 0, pbkv(b"k3", v)), (B, 1, 0, pbkv(b"k3", v)),
              (A, UNREG, 0, b""), (U, 0, 0, pbkv(b"k4", v)), (0, 0, 0, b"")]
    ups, ents = [], []
    for i, (c, series, resp, cmd) in enumerate(script):
        idx = first + i
        e = po.ent(term=term, index=idx, type=0, key=1000 + idx, client_id=c,
                   series_id=series, responded_to=resp, cmd=cmd)
        ents.append(e)
        ups.append(((term, 1, idx - 1), [e]))
    ups.append(((term, 1, first + len(script) - 1), []))
    return ups, ents


def model_of(ents, model=None):
    m = model or sm.Model()
    for e in ents:
        m.apply(e["client_id"], e["series_id"], e["responded_to"], e["type"],
                e["cmd"])
    return m


REC_CFG = dict(num_replicas=3, window=64, cmd_cap=32, kv_val_cap=4,
               kv_slots=64, save_cap=4096, save_tan=1, tan_max_log=1024,
               elections=1, max_props=3)


def _assert_recovered(eng, g, s, st, ents, m, base=0):
    a = eng.export_replicas(g, 1)[s]
    w = (g, s, st.to_dict())
    assert st.status == abi.REC_OK, w
    assert a.last_index == a.committed == a.sm_index == base + len(ents), w
    assert eng.kv_export(g, s) == m.kv and a.kv_count == m.count, w
    assert eng.sessions_export(g, s) == m.sessions(), w
    assert [po._etuple_to_dict(t) for t in
            eng.export_log(g, s, base + 1, a.last_index)] == ents, w


def test_recover_session_logs():
    n = 70  # groups in two waves' worth of lanes (n x 3 replica lanes)
    cfg = dict(REC_CFG, num_groups=n, session_slots=4, session_history=2)
    eng = Engine(**cfg)
    files, want = {}, {}
    for g in range(n):
        ups, ents = session_updates(g)
        for s in range(3):
            files[g, s] = list(enumerate(ti.write_logs(ups, 1 + g, s + 1)))
        want[g] = ents
    sts = eng.recover_tan(files, base_index=0, base_term=0, seed=SEED)
    for g in range(n):
        m = model_of(want[g])
        assert m.count == 4 and len(m.sessions()) == 1
        for s in range(3):
            _assert_recovered(eng, g, s, sts[g, s], want[g], m)
    for r in range(2):  # two live rounds continue
        e = eng.step(tick=True)
        assert e.fallbacks == 0 and e.errors == 0, e.to_dict()
    # S too small: the second register stops the replay's apply
    small = Engine(**dict(cfg, session_slots=1, session_history=2))
    st = small.recover_tan(files, 0, 0, SEED)
    for g in (0, n - 1):
        assert (st[g, 0].status, st[g, 0].applied) == \
            (abi.REC_APPLY_STOPPED, 3), st[g, 0].to_dict()
        a = small.export_replicas(g, 1)[0]
        assert (a.flags, a.fallback_reason) == (abi.F_FALLBACK,
                                                abi.FB["RECOVERY"])
        assert small.sessions_export(g, 0) == model_of(want[g][:3]).sessions()
    # the same images without the option
    off = Engine(**dict(cfg, session_slots=0, session_history=0))
    st = off.recover_tan(files, 0, 0, SEED)
    assert {x.status for x in st.values()} == {abi.REC_ENTRY_TYPE}


def test_recover_session_logs_from_a_snapshot():
    """base_index > 0: drb_sessions_import and drb_kv_import are the
    snapshot; the logs' session entries apply onto them."""
    n, base = 8, 40
    cfg = dict(REC_CFG, num_groups=n, session_slots=4, session_history=2)
    eng = Engine(**cfg)
    files = {}

    def snapshot(g):
        """The state machine at the base: two sessions, one key."""
        m = sm.Model()
        for (c, upto, hist) in [(cl(g, 5), 2, {3: 11}), (cl(g, 0), 0, {1: 11})]:
            ses = sm.Session(c)
            ses.responded_up_to, ses.history = upto, dict(hist)
            m.lru.add(ses)
        m.kv = {b"k0": val(g)}
        return m

    for g in range(n):
        snap = snapshot(g)
        ups, ents = session_updates(g, first=base + 1)
        for s in range(3):
            eng.sessions_import(g, s, snap.sessions())
            eng.kv_import(g, s, snap.kv)
            files[g, s] = list(enumerate(ti.write_logs(ups, 1 + g, s + 1)))
    sts = eng.recover_tan(files, base_index=base, base_term=2, seed=SEED)
    for g in range(n):
        _, ents = session_updates(g, first=base + 1)
        m = model_of(ents, snapshot(g))
        # the register is a duplicate; series 1 is served from the snapshot
        # (11, not the payload's length): three updates, clients 5 and 1 left
        assert m.count == 3 and m.kv[b"k0"] == val(g)
        assert [c for c, _, _ in m.sessions()] == [cl(g, 5), cl(g, 1)]
        for s in range(3):
            _assert_recovered(eng, g, s, sts[g, s], ents, m, base)


def test_recover_session_logs_multiplexed():
    n = 20
    cfg = dict(REC_CFG, num_groups=n, tan_multiplexed=1, first_shard_id=1,
               session_slots=4, session_history=2)
    eng = Engine(**cfg)
    lists, want = {}, {}
    for g in range(n):
        ups, ents = session_updates(g)
        lists[1 + g] = ups
        want[g] = ents
    files = {}
    for s in range(3):
        for key, fs in tm.shared_logs(lists, s + 1).items():
            files[s, key] = list(enumerate(fs))
    sts, lst = eng.recover_tan_mux(files, 0, 0, SEED)
    for g in range(n):
        m = model_of(want[g])
        for s in range(3):
            _assert_recovered(eng, g, s, sts[g, s], want[g], m)
