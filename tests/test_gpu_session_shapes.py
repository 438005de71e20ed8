"""GPU: the session table at its compiled limits and beside the other
options (drb_session.hpp, apply_entry in drb_step.hpp).

G = 66: a full wave of groups and a partial one.  Every test asserts that
each outcome class it targets was seen in both waves on every replica slot
(SessPair.classes).  The checker is tests/session_harness.py: the oracle on
the no-op twin for everything raft, tests/session_model.py for the tables.
"""
import functools

import pytest

from dragonboat_amd import abi
from oracle import pyoracle as po
from tests import snappy_blocks as sb
from tests.session_harness import (REG, UNREG, SessPair, cl, ent, pbkv,
                                   script_rounds, val)
from tests.test_gpu_sessions import lifecycle, run_script

pytestmark = pytest.mark.gpu

G = 66
STOPPED = abi.F_FALLBACK | abi.F_APPLY_STOPPED
LIFECYCLE = {"registered", "update", "cached", "responded", "unknown-client",
             "register-duplicate", "unregistered", "unregister-unknown",
             "noop-session", "noop"}


def slots(R):
    return {(w, s) for w in (0, 1) for s in range(R)}


def seen_everywhere(p, classes, R=3):
    assert set(p.classes) >= set(classes), set(classes) - set(p.classes)
    for c in classes:
        assert p.classes[c] == slots(R), (c, p.classes[c])


def drain(p, n=4, **kw):
    for r in range(n):
        p.sess_round(tick=(r % 2 == 1), **kw)
    for g in range(p.G):
        sts = p.eng.export_replicas(g, 1)
        assert all(a.sm_index == a.last_index == sts[0].last_index
                   for a in sts), g


def stops_at(p, full, reason, groups=None, rounds=8):
    """The entries at full[g] are in the leaders' logs: step until every
    replica of `groups` has stopped its apply in front of its group's, with
    the state machine as the model has it just before; the other groups
    keep the full check."""
    groups = list(range(p.G)) if groups is None else groups
    rest = [g for g in range(p.G) if g not in groups]
    p.sm_seen.clear()  # export every table again
    stopped = {}
    for r in range(rounds):
        o = p.orc.round(tick=False)
        e = p.eng.step(tick=False)
        p.rounds += 1
        assert e.errors == 0, e.to_dict()
        sts = p.eng.export_replicas(0, p.G)
        p.advance_model(sts)
        for g in groups:
            for s in range(p.R):
                a = sts[g * p.R + s]
                if (g, s) in stopped or not a.flags & abi.F_FALLBACK:
                    continue
                stopped[g, s] = r
                w = (r, g, s)
                assert a.flags == abi.F_HOSTED | STOPPED, (w, a.flags)
                assert a.fallback_reason == reason, (w, a.fallback_reason)
                assert a.sm_index == full[g] - 1, (w, a.sm_index, full[g])
                p.sm_seen.pop((g, s), None)
                p.check_sm(g, s, a, w)
        if rest:
            p.check_round(o, e, groups=rest)
        if len(stopped) == p.R * len(groups):
            break
    assert len(stopped) == p.R * len(groups), len(stopped)
    # nothing of the stopping entry reached the model's replay either
    assert all(max(p.snaps[g]) == full[g] - 1 for g in groups)


def next_index(p):
    return [a.last_index + 1 for a in p.eng.export_replicas(0, p.G)[::p.R]]


# --------------------------------------------------- 1: S = 16, H = 8
def full_table(g):
    c7, v = cl(g, 7), val(g)

    def up(series, responded_to):
        return ent(c7, series, responded_to, pbkv(b"h%d" % series, v))

    return [ent(cl(g, n), REG) for n in range(16)] + \
        [up(x, 0) for x in range(1, 9)] + [   # the history full: two trips
        up(3, 0),                             # cached
        up(9, 5),                             # five dropped, lowest slot
        up(7, 5),                             # cached
        up(4, 5),                             # responded
        ent(cl(g, 0), UNREG),
        ent(cl(g, 16), REG),                  # slot 0, exported last but one
        up(10, 5), up(11, 5)]


def test_full_table_and_full_history():
    p = SessPair(G, R=3, session_slots=16, session_history=8)
    run_script(p, full_table)
    seen_everywhere(p, {"registered", "update", "cached", "responded",
                        "unregistered"})
    for g in (0, 1, 64, 65):
        tbl = p.eng.sessions_export(g, 2)
        assert len(tbl) == 16
        # least recently used first: the new client in slot 0 comes last but
        # one, client 7 (used since) last, its history ascending by series
        assert [c for c, _, _ in tbl[-2:]] == [cl(g, 16), cl(g, 7)]
        assert tbl[-1][1] == 5 and list(tbl[-1][2]) == [6, 7, 8, 9, 10, 11]
        assert [c for c, _, _ in tbl[:6]] == [cl(g, n) for n in range(1, 7)]
    drain(p, 2)
    full = next_index(p)
    p.sess_round({g: [ent(cl(g, 17), REG)] for g in range(G)})
    stops_at(p, full, abi.FB["CAPACITY"])


def test_a_ninth_unanswered_series_stops_the_apply():
    p = SessPair(G, R=3, session_slots=16, session_history=8)
    A = [cl(g, 0) for g in range(G)]

    def steps(g):
        return [ent(A[g], REG)] + [ent(A[g], x, 0, pbkv(b"k%d" % x, val(g)))
                                   for x in range(1, 9)]
    run_script(p, steps, drain=3)
    assert all(len(p.eng.sessions_export(g, 1)[0][2]) == 8 for g in (0, 65))
    full = next_index(p)
    p.sess_round({g: [ent(A[g], 9, 0, pbkv(b"k9", val(g)))]
                  for g in range(G)})
    stops_at(p, full, abi.FB["CAPACITY"])


# ------------------------------------------------------- 2: R = 1, R = 5
@pytest.mark.parametrize("R", [1, 5])
def test_session_lifecycle_other_replica_counts(R):
    p = SessPair(G, R=R, session_slots=4, session_history=2)
    run_script(p, lifecycle)
    assert set(p.classes) == LIFECYCLE
    seen_everywhere(p, LIFECYCLE, R)
    twice = ("registered", "update")
    assert p.compared == {c: (2 if c in twice else 1) * G
                          for c in LIFECYCLE}, p.compared


# --------------------------------------------------------------- 3: Snappy
def snappy_cmd(key, value):
    payload = po.pbkv_marshal(key, value)
    return sb.checked(sb.compress(payload), payload)


@functools.lru_cache(maxsize=None)
def snappy_steps(g):
    A, ENC = cl(g, 0), abi.ENTRY_ENCODED
    small = snappy_cmd(bytes([1 + g]) * 8, val(g))
    # a run of 1000 bytes: a Cmd of at most 64 B that decodes to 1013
    big = snappy_cmd((g).to_bytes(8, "little"), bytes([1 + g % 250]) * 1000)
    assert len(big) <= 64 < len(po.get_payload(ENC, big))
    return [ent(A, REG),
            ent(A, 1, 0, small, ENC),
            ent(A, 1, 0, small, ENC),     # cached
            ent(A, 2, 1, big, ENC),
            ent(A, 2, 1, big, ENC),       # cached: the decoded length
            ent(A, 1, 2, small, ENC)]     # responded


SNAPPY = dict(entry_compression=1, cmd_cap=64, kv_val_cap=1024, kv_slots=16,
              kv_pool_blocks=1024, save_cap=4096, session_slots=4,
              session_history=2)


def test_sessions_with_snappy_entries():
    p = SessPair(G, R=3, payload=po.get_payload, **SNAPPY)
    held = 0
    for rows, tick, ri in script_rounds(G, snappy_steps):
        p.sess_round(rows, tick=tick, read_index=ri, encode_saves=True)
        for g in range(G):
            for s in range(3):
                got = p.eng.export_saved(g, s)
                assert got == p.expected_saved(g, s), (p.rounds, g, s)
                held += sum(e["series_id"] not in (0, REG) and e["type"] ==
                            abi.ENTRY_ENCODED and e["cmd"][:1] == b"\x02"
                            for e in po.entrybatch_unmarshal(got[0])) \
                    if got[0] else 0
    assert held == 3 * 5 * G  # the compressed Cmds with their session fields
    seen_everywhere(p, {"registered", "update", "cached", "responded"})
    for g in (0, 65):
        res = [p.results[g][i][0] for i in sorted(p.results[g])]
        # Result.Value is the decoded payload's length, the cached one too
        assert [v for v, _, _ in res[1:]] == [16, 16, 1013, 1013, 0]
    # a corrupt block in a session update: no history entry, no KV change
    blk = dict(sb.malformed_vectors())["offset_0"]
    with pytest.raises(po.OracleError):
        po.get_payload(abi.ENTRY_ENCODED, sb.cmd(blk))
    full = next_index(p)
    p.sess_round({g: [ent(cl(g, 0), 3, 2, sb.cmd(blk), abi.ENTRY_ENCODED)]
                  for g in range(G)})
    stops_at(p, full, abi.FB["ENTRY_TYPE"])
    for g in (0, 65):
        for s in range(3):
            (c, upto, hist), = p.eng.sessions_export(g, s)
            assert (c, upto, hist) == (cl(g, 0), 2, {})


# ------------------------------------------- 4: Quiesce and listed rounds
def test_sessions_reach_quiesced_groups_in_listed_rounds():
    p = SessPair(G, R=3, quiesce=True, election_rtt=4, session_slots=4,
                 session_history=2)
    for rows, tick, ri in script_rounds(G, lambda g: lifecycle(g)[:6]):
        p.sess_round(rows, tick=tick, read_index=ri)
    for r in range(90):  # past 20 x ElectionRTT idle ticks
        p.sess_round(tick=True, listed=True)
    assert all(p.orc.export(g, s).qs_quiesced_since != 0
               for g in range(G) for s in range(3))
    for rows, tick, ri in script_rounds(G, lambda g: lifecycle(g)[6:]):
        p.sess_round(rows, tick=tick, read_index=ri, listed=True)
    drain(p, 2, listed=True)
    assert set(p.classes) == LIFECYCLE
    seen_everywhere(p, LIFECYCLE)


# ------------------------------------- 5: a full KV and a refused payload
def _four_keys(g):
    A, v = cl(g, 0), val(g)
    return [ent(A, REG)] + [ent(A, x, x - 1, pbkv(b"k%d" % x, v))
                            for x in range(1, 5)]


@pytest.mark.parametrize("case", ["kv_full", "value_above_kv_val_cap"])
def test_a_failed_update_leaves_both_tables_as_they_were(case):
    """The failing update carries responded_to = 4: its clearTo and its
    response are decided but must not be stored."""
    p = SessPair(G, R=3, kv_slots=4, kv_overflow_buckets=0, session_slots=4,
                 session_history=2)
    run_script(p, _four_keys, drain=3)
    if case == "kv_full":  # a fifth key
        cmd, reason = pbkv(b"k5", b"vvvv"), abi.FB["CAPACITY"]
    else:  # a known key, a value of 5 bytes
        cmd, reason = pbkv(b"k4", b"vvvvv"), abi.FB["ENTRY_TYPE"]
    full = next_index(p)
    p.sess_round({g: [ent(cl(g, 0), 5, 4, cmd)] for g in range(G)})
    stops_at(p, full, reason)
    for g in (0, 1, 64, 65):
        for s in range(3):
            assert p.eng.sessions_export(g, s) == [(cl(g, 0), 3, {4: 10})]
            assert p.eng.export(g, s).kv_count == 4
            assert sorted(p.eng.kv_export(g, s)) == \
                [b"k1", b"k2", b"k3", b"k4"]


# ---------------------------------------------------------------- 6: gates
def _gate(g, kind):
    """(the entry put in the leader's log, whether it stops the apply)."""
    A, c = cl(g, 0), pbkv(b"g", val(g))
    return {
        "register_with_cmd": (ent(A, REG, 0, c), True),
        "unregister_with_cmd": (ent(A, UNREG, 0, c), True),
        "client_0_with_cmd": (ent(0, 0, 0, c), True),
        "client_0_series_5_empty": (ent(0, 5), False),
        "metadata_type": (ent(A, 2, 1, c, abi.ENTRY_METADATA), True),
    }[kind]


@pytest.mark.parametrize("kind", [
    "register_with_cmd", "unregister_with_cmd", "client_0_with_cmd",
    "client_0_series_5_empty", "metadata_type"])
def test_entries_that_staging_refuses_meet_the_apply_gates(kind):
    """prop_fast refuses these when they are staged, so each goes into the
    leader's log with drb_import_log, in place of an empty no-op appended
    that round and not yet replicated (followers copy a Replicate's entries
    from the leader's window).  The oracle's twin is that no-op, of the same
    type -- a session entry of a type that is neither APPLICATION nor
    ENCODED can be appended this way too, no earlier gate reads the type.
    ClientID 0 with a series and no Cmd is the reference's IsEmpty entry: it
    applies as a no-op, is reported APPLY_IGNORED and leaves the table
    untouched; the others stop the apply (DRB_FB_ENTRY_TYPE)."""
    p = SessPair(G, R=3, session_slots=4, session_history=2)
    run_script(p, lambda g: [ent(cl(g, 0), REG),
                             ent(cl(g, 0), 1, 0, pbkv(b"k", val(g)))],
               drain=3)
    full = next_index(p)
    mp = p.eng.cfg["max_props"]
    counts, real, twin, pbuf = p.build_rows(
        {g: [ent(0, 0)] for g in range(G)}, mp, 1)
    for g in range(G):
        twin[g].type = _gate(g, kind)[0]["type"]
    p.orc.stage_proposals(counts, 1, twin, pbuf, 0)
    p.eng.stage_proposals(0, counts, real, pbuf)
    o = p.orc.round(tick=False)
    e = p.eng.step(tick=False, prop_slot=0)
    p.rounds += 1
    for g in range(G):
        gate = _gate(g, kind)[0]
        log = [po._etuple_to_dict(t)
               for t in p.eng.export_log(g, 0, 1, full[g])]
        assert log[-1]["index"] == full[g] and \
            log[-1]["key"] == real[g * mp].key, g
        log[-1] = dict(log[-1], **gate)
        arr, pool, n = po.EntryPool(log).arrays()
        p.eng.import_log(g, 0, arr, pool)
        p.real[log[-1]["key"]] = (gate["client_id"], gate["series_id"],
                                  gate["responded_to"], gate["cmd"])
    p.check_round(o, e)  # the leaders' logs and Replicates hold the entries
    stop = _gate(0, kind)[1]
    if stop:
        stops_at(p, full, abi.FB["ENTRY_TYPE"])
    else:
        drain(p, 4)
        seen_everywhere(p, {"noop"})
        for g in range(G):
            res, cls, _ = p.results[g][full[g]]
            assert (res, cls) == ((0, False, True), "noop"), g
        assert p.reported.get((False, abi.APPLY_IGNORED), 0) == G
    for g in range(G):
        for s in range(3):
            assert p.eng.export(g, s).sm_index == full[g] - stop, (g, s)
            assert p.eng.sessions_export(g, s) == [(cl(g, 0), 0, {1: 9})], \
                (g, s)
