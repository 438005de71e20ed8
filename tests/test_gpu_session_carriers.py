"""GPU: session entries on every carrier, byte for byte.

What a GPU NodeHost saves and sends for dragonboat's default client mode:
the EntryBatch and batched LogDB records (drb_codec.hpp), the tan records
(drb_tan.hpp) with a restart from the engine's own logs, the wire streams
(drb_wire.hpp: from ring rows and, with forwarded proposals, from staged
rows) and the mailbox planes between ranks -- each with non-zero SeriesID
and RespondedTo, in both colfer forms (varint below 2^49, fixed 8 bytes from
there; a register's SeriesID is MaxUint64 - 1).

The oracle sees the no-op twin; the expected bytes are what it saved or sent
with the staged entries put back by Key, marshalled by the oracle's codecs
(tests/session_harness.py; tests/test_session_expected.py checks that half
alone).  Every round keeps the full check of SessPair.check_round.
"""
import pytest

from dragonboat_amd import abi
from dragonboat_amd.engine import Engine
from oracle import pyoracle as po
from tests.gpu_harness import DistPair, by_dest, state_diff
from tests.session_harness import (FIRST_SHARD, TAN_FILLER, Coverage,
                                   SessPair, TanTwins, Twins,
                                   check_tan_mux_round, check_tan_round,
                                   check_wire_planes, filler_rounds,
                                   script_rounds, wide)
from tests.test_gpu_sessions import REC_CFG, SEED, lifecycle
from tests.test_gpu_wire import TwoNodes
from tests.test_oracle_tan import _decode_update

pytestmark = pytest.mark.gpu

SESS = dict(session_slots=4, session_history=2)
SCRIPTS = {"lifecycle": lifecycle, "wide": wide}
NAMES = sorted(SCRIPTS)


def _replicas(p):
    return [(g, s) for g in range(p.G) for s in range(p.R)]


# ------------------------------------------------ a: EntryBatch, batched
@pytest.mark.parametrize("name", NAMES)
def test_entrybatch_saves_hold_the_session_fields(name):
    p = SessPair(12, R=3, save_cap=4096, **SESS)
    cov = Coverage()
    for rows, tick, ri in script_rounds(p.G, SCRIPTS[name]):
        o, e = p.sess_round(rows, tick=tick, read_index=ri,
                            encode_saves=True)
        total = 0
        for g, s in _replicas(p):
            got = p.eng.export_saved(g, s)
            assert got == p.expected_saved(g, s), (p.rounds, g, s)
            total += len(got[0])
            if got[0]:
                cov.add(po.entrybatch_unmarshal(got[0]))
        assert e.saved_bytes == total, p.rounds
    cov.check(wide=(name == "wide"))


@pytest.mark.parametrize("name", NAMES)
def test_batched_records_hold_the_session_fields(name):
    """Fourteen filler rounds first: the script's entries straddle index 48,
    so a batch's first record merges session entries with earlier saves."""
    p = SessPair(12, R=3, save_cap=8192, save_batched=1, window=64, **SESS)
    db = po.BatchDB()
    cov, merged = Coverage(), 0
    rounds = filler_rounds(p.G, 14) + \
        list(script_rounds(p.G, SCRIPTS[name]))
    for rows, tick, ri in rounds:
        p.sess_round(rows, tick=tick, read_index=ri, encode_saves=True)
        for g, s in _replicas(p):
            want = p.expected_records(db, g, s)
            got = p.eng.export_save_records(g, s)
            assert got == want, (p.rounds, g, s)
            for _, v, _ in got:
                ents = po.entrybatch_unmarshal(v)
                cov.add(ents)
                merged += len(ents) > 1 and any(e["series_id"] for e in ents)
    assert merged
    cov.check(wide=(name == "wide"))


# ------------------------------------------------------------------ b: tan
def _restart(p, files, mux):
    """A fresh engine recovered from the images the first one wrote."""
    base = p.base[0]
    assert set(p.base) == {base}
    cfg = dict(REC_CFG, num_groups=p.G, **SESS)
    if mux:
        cfg.update(tan_multiplexed=1, first_shard_id=FIRST_SHARD)
    e2 = Engine(**cfg)
    if mux:
        sts, _ = e2.recover_tan_mux(files, base, 2, SEED)
    else:
        sts = e2.recover_tan(files, base_index=base, base_term=2, seed=SEED)
    for g, s in _replicas(p):
        a = e2.export_replicas(g, 1)[s]
        last = p.orc.export(g, s).last_index
        w = (g, s, sts[g, s].to_dict())
        assert sts[g, s].status == abi.REC_OK, w
        assert a.last_index == a.committed == a.sm_index == last, w
        kv, count, sessions = p.snaps[g][last]
        assert e2.kv_export(g, s) == kv and a.kv_count == count, w
        assert e2.sessions_export(g, s) == sessions, w
        assert e2.export_log(g, s, base + 1, last) == \
            [p._back(t) for t in p.orc.export_log(g, s, base + 1, last)], w
    for r in range(2):
        e = e2.step(tick=True)
        assert e.fallbacks == 0 and e.errors == 0, e.to_dict()
    e2.close()


@pytest.mark.parametrize("mux,G", [(False, 12), (True, 12), (True, 20)])
@pytest.mark.parametrize("name", NAMES)
def test_tan_records_and_restart_from_the_engines_own_logs(name, mux, G):
    """1 KiB logs; the filler rounds bring every log near 700 bytes, so each
    switches inside the script.  G = 20: shards 1-4 share their multiplexed
    logs with shards 17-20."""
    kw = dict(tan_multiplexed=1) if mux else {}
    p = SessPair(G, R=3, save_cap=4096, save_tan=1, tan_max_log=1024,
                 **kw, **SESS)
    tt = TanTwins(p, 1024, mux=mux)
    logs, at_script = {}, None
    rounds = filler_rounds(G, TAN_FILLER) + \
        list(script_rounds(G, SCRIPTS[name]))
    for r, (rows, tick, ri) in enumerate(rounds):
        if r == TAN_FILLER:
            at_script = {k[:2]: k[2] for k in sorted(logs)}
        o, e = p.sess_round(rows, tick=tick, read_index=ri,
                            encode_saves=True)
        n = (check_tan_mux_round if mux else check_tan_round)(p, tt, logs, r)
        assert e.log_records == n, (r, e.to_dict())
    # every GPU-built log is the expected file; each switched in the script
    cov, files = Coverage(), {}
    for key in sorted(logs):
        a, b, lg = key
        img = bytes(logs[key])
        assert img == tt.real[a][b].file(lg), key
        files.setdefault((a, b), []).append((lg, img))
        for _, payload in po.tan_read(img):
            cov.add(_decode_update(payload)[3])
    end = {k[:2]: k[2] for k in sorted(logs)}
    assert all(end[k] > at_script[k] for k in end) and \
        set(end) == set(at_script), (at_script, end)
    cov.check(wide=(name == "wide"))
    _restart(p, files, mux)


# ----------------------------------------------------------------- c: wire
@pytest.mark.parametrize("name", NAMES)
def test_wire_planes_hold_the_session_fields(name):
    p = SessPair(40, R=3, **SESS)
    cov = Coverage()
    for rows, tick, ri in script_rounds(p.G, SCRIPTS[name]):
        p.sess_round(rows, tick=tick, read_index=ri)
        check_wire_planes(p, p.eng, 0x1234567890 + p.rounds, [0, 1, 500],
                          cov=cov)
    cov.check(wide=(name == "wide"))


def test_wire_propose_plane_from_staged_rows():
    """forward_proposals, the entry queue at replica 2 (slot 1): that
    follower's Propose plane is encoded from the staged rows, drb_wire.hpp's
    second header source."""
    p = SessPair(40, R=3, forward_proposals=1, **SESS)
    cov, proposed = Coverage(), 0
    for rows, tick, ri in script_rounds(p.G, lambda g: lifecycle(g)[:6],
                                        drain=6):
        p.sess_round(rows, tick=tick, read_index=ri, prop_replica=2)
        check_wire_planes(p, p.eng, 0xD1D, [0, 1, 500], cov=cov)
        for m in p.wire_messages(1, 0):
            if m["type"] == abi.MSG["Propose"]:
                proposed += sum(e["series_id"] != 0 for e in m["entries"])
    # all six steps of every group are session entries
    assert proposed == 6 * p.G, proposed
    assert abi.SERIES_REGISTER in cov.series and any(cov.responded - {0})


class SessTwoNodes(Twins, TwoNodes):
    """TwoNodes with the real batch for the leaders' engine, its twin for
    the oracle, and the model for both engines' state machines."""

    def __init__(self, G, **kw):
        TwoNodes.__init__(self, G, cmd_cap=32, kv_val_cap=4, max_props=3,
                          **kw)
        self.init_twins()
        sts = self.lead.export_replicas(0, G)
        self.init_models([sts[g * self.R].sm_index for g in range(G)])

    def eng_of(self, s):
        return self.lead if s == 0 else self.foll

    def sess_round(self, rows, tick, read_index):
        batch = None
        if rows:
            k = max(len(v) for v in rows.values())
            counts, real, twin, pbuf = self.build_rows(
                rows, self.lead.cfg["max_props"], k)
            batch = (counts, k, twin, real, pbuf)
        o, a, b = self.round(k=0, tick=tick, read_index=read_index,
                             batch=batch)
        for x in (a, b):
            assert x.fallbacks == 0 and x.errors == 0, (self.rounds,
                                                        x.to_dict())
        self.check_sess()

    def check_sess(self):
        for g in range(self.G):
            reps = [self.eng_of(s).export_replicas(g, 1)[s]
                    for s in range(self.R)]
            src = max(range(self.R), key=lambda s: reps[s].sm_index)
            self.advance_group(
                g, reps[src].sm_index,
                lambda lo, hi: self.eng_of(src).export_log(g, src, lo, hi))
            for s in range(self.R):
                eng, a, b = self.eng_of(s), reps[s], self.orc.export(g, s)
                w = (self.rounds, g, s)
                d = state_diff(a, b, self.R)
                d.pop("kv_count", None)
                assert not d, (w, d)
                lo = max(1, b.last_index - 8)
                assert eng.export_log(g, s, lo, b.last_index) == \
                    [self._back(t) for t in
                     self.orc.export_log(g, s, lo, b.last_index)], w
                assert by_dest(eng.export_outbox(g, s)) == \
                    self._msgs(self.orc.export_outbox(g, s)), w
                assert eng.export_ready(g, s) == self.orc.export_ready(g, s), w
                self.check_sm_of(eng, g, g, s, a, w)


def test_two_nodehosts_over_the_wire_with_sessions():
    t = SessTwoNodes(32, **SESS)
    for rows, tick, ri in script_rounds(t.G, lifecycle):
        t.sess_round(rows, tick, ri)
    assert t.wire_bytes > 0
    for g in range(t.G):
        sts = [t.eng_of(s).export_replicas(g, 1)[s] for s in range(3)]
        assert all(a.sm_index == a.last_index == sts[0].last_index
                   for a in sts), g
    want = {"registered", "update", "cached", "responded", "unknown-client",
            "register-duplicate", "unregistered", "unregister-unknown",
            "noop-session", "noop"}
    assert set(t.classes) == want
    assert all(t.classes[c] == {(0, s) for s in range(3)} for c in want)


# ----------------------------------------------------- d: spread placement
class SessDist(Twins, DistPair):
    def __init__(self, G, **kw):
        DistPair.__init__(self, G, cmd_cap=32, kv_val_cap=4, max_props=3,
                          **kw)
        self.init_twins()
        self.init_models([self.replica(g, 0).sm_index for g in range(G)])

    def sess_round(self, rows, tick, read_index):
        batch = None
        if rows:
            k = max(len(v) for v in rows.values())
            counts, real, twin, pbuf = self.build_rows(
                rows, self.engs[0].cfg["max_props"], k)
            batch = (counts, k, twin, real, pbuf)
        o, tot = self.round(k=0, tick=tick, read_index=read_index,
                            batch=batch)
        assert tot["fallbacks"] == 0 and tot["errors"] == 0, \
            (self.rounds, tot, self.why())
        assert (tot["applied_entries"], tot["messages"]) == \
            (o.applied_entries, o.messages), (self.rounds, tot, o.to_dict())
        self.check_sess()

    def check_sess(self):
        for g in range(self.G):
            reps = [self.replica(g, s) for s in range(self.R)]
            src = max(range(self.R), key=lambda s: reps[s].sm_index)
            r, j = self.where(g, src)
            self.advance_group(
                g, reps[src].sm_index,
                lambda lo, hi: self.engs[r].export_log(j, src, lo, hi))
            for s in range(self.R):
                r, j = self.where(g, s)
                eng, a, b = self.engs[r], reps[s], self.orc.export(g, s)
                w = (self.rounds, g, s)
                assert not a.flags & (abi.F_FALLBACK | abi.F_ERROR), \
                    (w, a.flags, a.fallback_reason)
                d = state_diff(a, b, self.R)
                d.pop("kv_count", None)
                assert not d and a.shard_id == b.shard_id, (w, d)
                lo = max(1, b.last_index - 8)
                assert eng.export_log(j, s, lo, b.last_index) == \
                    [self._back(t) for t in
                     self.orc.export_log(g, s, lo, b.last_index)], w
                assert by_dest(eng.export_outbox(j, s)) == \
                    self._msgs(self.orc.export_outbox(g, s)), w
                self.check_sm_of(eng, j, g, s, a, w)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("counted", [False, True])
def test_sessions_with_replicas_spread_over_ranks(N, counted):
    d = SessDist(24, R=3, N=N, E=4, counted=counted, **SESS)
    for rows, tick, ri in script_rounds(d.G, lifecycle):
        d.sess_round(rows, tick, ri)
    for g in range(d.G):
        sts = [d.replica(g, s) for s in range(3)]
        assert all(a.sm_index == a.last_index == sts[0].last_index
                   for a in sts), g
    want = {"registered", "update", "cached", "responded", "unknown-client",
            "register-duplicate", "unregistered", "unregister-unknown",
            "noop-session", "noop"}
    assert set(d.classes) == want
    assert all(d.classes[c] == {(0, s) for s in range(3)} for c in want)
