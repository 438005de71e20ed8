"""The checker of the GPU session tests (tests/test_gpu_sessions.py).

The C oracle panics on session-managed entries, so the check has two parts:

  the no-op twin   the engine gets the real batch; the oracle gets the same
                   batch with every SeriesID != 0 entry replaced by an empty
                   no-op of the same Key (ClientID 0, no Cmd) -- raft never
                   reads those fields.  Every round and replica: the state
                   (without kv_count), the log and the outbox after putting
                   the staged entries back by Key, the ReadyToReads, and the
                   round's applied_entries and messages.
  the model        tests/session_model.py replayed over the group's log,
                   with a snapshot per index (followers lag): each replica's
                   KV, kv_count and exported sessions at its own sm_index,
                   and the leader slot's drb_apply_results.
"""
import ctypes as C

from dragonboat_amd import abi, workload
from tests import session_model as sm
from tests.gpu_harness import Pair, by_dest, state_diff

APP = abi.ENTRY_APPLICATION
REG, UNREG = abi.SERIES_REGISTER, abi.SERIES_UNREGISTER


def pbkv(key, val):
    """PBKV{key, val} marshalled (short fields)."""
    return b"\x0a" + bytes([len(key)]) + key + b"\x12" + bytes([len(val)]) + val


def ent(client, series, responded_to=0, cmd=b"", typ=APP):
    return dict(client_id=client, series_id=series, responded_to=responded_to,
                type=typ, cmd=cmd)


def bits(res):
    """drb_apply_result.ignored of a model result (value, rejected,
    ignored)."""
    return (abi.APPLY_IGNORED if res[2] else 0) | \
        (abi.APPLY_REJECTED if res[1] else 0)


class SessPair(Pair):
    def __init__(self, G, **kw):
        kw.setdefault("cmd_cap", 32)
        kw.setdefault("kv_val_cap", 4)
        kw.setdefault("max_props", 3)
        kw.setdefault("window", 64)
        super().__init__(G, **kw)
        self.real = {}    # Key -> the staged entry (tuple fields 4..7)
        self.nkey = 0
        sts = self.eng.export_replicas(0, G)
        # the model of each group, its snapshots and results per index
        self.base = [sts[g * self.R].sm_index for g in range(G)]
        self.model = [sm.Model() for _ in range(G)]
        self.snaps = [{self.base[g]: self.model[g].snapshot()}
                      for g in range(G)]
        self.results = [{} for _ in range(G)]
        self.classes = {}  # outcome class -> {(wave, slot)}
        self.sm_seen = {}
        # the leader slots' drb_apply_results records that were compared:
        # the model's outcome class -> records, and the engine's own
        # (value != 0, ignored bits) -> records
        self.compared = {}
        self.reported = {}

    # -------------------------------------------------------------- staging
    def stage_rows(self, rows, prop_replica=0):
        """rows: {g: [ent(...)]}; the engine gets them, the oracle their
        no-op twins."""
        k = max([len(v) for v in rows.values()] + [1])
        mp = self.eng.cfg["max_props"]
        assert k <= mp
        counts = (C.c_uint32 * self.G)()
        real = (abi.Entry * (self.G * mp))()
        twin = (abi.Entry * (self.G * k))()
        pool = bytearray()
        for g, es in rows.items():
            counts[g] = len(es)
            for j, e in enumerate(es):
                self.nkey += 1
                key = workload.mix64(0x5E55 + self.nkey) | 1
                cmd = e["cmd"]
                real[g * mp + j] = abi.Entry(
                    0, 0, key, e["client_id"], e["series_id"],
                    e["responded_to"], e["type"], len(cmd), len(pool))
                if e["series_id"] != 0:
                    twin[g * k + j] = abi.Entry(0, 0, key, 0, 0, 0, e["type"],
                                                0, 0)
                    self.real[key] = (e["client_id"], e["series_id"],
                                      e["responded_to"], bytes(cmd))
                else:
                    twin[g * k + j] = real[g * mp + j]
                pool += cmd
        pbuf = (C.c_uint8 * max(1, len(pool))).from_buffer_copy(
            bytes(pool) or b"\0")
        self.orc.stage_proposals(counts, k, twin, pbuf, prop_replica)
        self.eng.stage_proposals(0, counts, real, pbuf)

    def sess_round(self, rows=None, tick=False, read_index=False,
                   prop_replica=0, check=True):
        pin = abi.DRB_NONE
        if rows:
            self.stage_rows(rows, prop_replica)
            pin = 0
        _, ri_in = self.stage(k=0, read_index=read_index)
        o = self.orc.round(tick=tick)
        e = self.eng.step(tick=tick, prop_slot=pin, ri_slot=ri_in,
                          prop_replica=prop_replica)
        self.rounds += 1
        if check:
            self.check_round(o, e)
        return o, e

    # ------------------------------------------------------------- the twin
    def _back(self, t):
        """An oracle entry tuple with the staged entry put back by Key."""
        r = self.real.get(t[3])
        return t if r is None else t[:4] + r

    def _msgs(self, msgs):
        return by_dest([m[:11] + (tuple(self._back(t) for t in m[11]),)
                        for m in msgs])

    def advance_model(self, sts):
        """The model of every group up to the highest sm_index of its
        replicas, over the leader's (or any up-to-date replica's) log."""
        for g in range(self.G):
            reps = sts[g * self.R:(g + 1) * self.R]
            done = max(self.snaps[g])
            hi = max(a.sm_index for a in reps)
            if hi <= done:
                continue
            src = max(range(self.R), key=lambda s: reps[s].sm_index)
            for t in self.eng.export_log(g, src, done + 1, hi):
                res, cls = self.model[g].apply(t[4], t[5], t[6], t[2], t[7])
                self.snaps[g][t[1]] = self.model[g].snapshot()
                self.results[g][t[1]] = (res, cls, t[3])

    def check_round(self, o, e, fallbacks=0):
        where = self.rounds
        assert e.errors == 0 and e.fallbacks == fallbacks, \
            (where, e.to_dict(), self.why())
        assert (e.applied_entries, e.messages) == \
            (o.applied_entries, o.messages), (where, e.to_dict(), o.to_dict())
        sts = self.eng.export_replicas(0, self.G)
        self.advance_model(sts)
        lead_res = {}
        for g in range(self.G):
            for s in range(self.R):
                a, b = sts[g * self.R + s], self.orc.export(g, s)
                w = (where, g, s)
                assert not a.flags & (abi.F_FALLBACK | abi.F_ERROR), \
                    (w, a.flags, a.fallback_reason)
                d = state_diff(a, b, self.R)
                d.pop("kv_count", None)
                assert not d, (w, d)
                lo = max(1, b.last_index - 8)
                assert self.eng.export_log(g, s, lo, b.last_index) == \
                    [self._back(t) for t in
                     self.orc.export_log(g, s, lo, b.last_index)], w
                assert by_dest(self.eng.export_outbox(g, s)) == \
                    self._msgs(self.orc.export_outbox(g, s)), w
                assert self.eng.export_ready(g, s) == \
                    self.orc.export_ready(g, s), w
                self.check_sm(g, s, a, w)
                if a.role == abi.LEADER and a.flags & abi.F_HOSTED and \
                        a.sm_index > a.applied_index:
                    lead_res.setdefault(s, {})[g] = (a.applied_index,
                                                     a.sm_index)
        # the leader slots' drb_apply_results: value and both bits
        for s, groups in lead_res.items():
            got = {}
            for (g, idx, key, cid, series, value, ign) in \
                    self.eng.apply_results(s):
                got.setdefault(g, []).append((idx, key, value, ign))
            for g, (lo, hi) in groups.items():
                want = [(i, self.results[g][i][2], self.results[g][i][0][0],
                         bits(self.results[g][i][0]))
                        for i in range(lo + 1, hi + 1)]
                assert got.get(g, []) == want, (where, g, s, got.get(g), want)
                for i, (_, _, value, ign) in zip(range(lo + 1, hi + 1),
                                                 got[g] if want else []):
                    cls = self.results[g][i][1]
                    self.compared[cls] = self.compared.get(cls, 0) + 1
                    k = (value != 0, ign)
                    self.reported[k] = self.reported.get(k, 0) + 1

    def check_sm(self, g, s, a, w):
        """Replica (g, s)'s KV, kv_count and sessions against the model at
        its own sm_index (exported only when that moved)."""
        if self.sm_seen.get((g, s)) == a.sm_index:
            return
        kv, count, sessions = self.snaps[g][a.sm_index]
        assert a.kv_count == count, (w, a.kv_count, count)
        assert self.eng.kv_export(g, s) == kv, w
        assert self.eng.sessions_export(g, s) == sessions, \
            (w, self.eng.sessions_export(g, s), sessions)
        for i in range(self.sm_seen.get((g, s), self.base[g]) + 1,
                       a.sm_index + 1):
            self.classes.setdefault(self.results[g][i][1], set()).add(
                (g // 64, s))
        self.sm_seen[g, s] = a.sm_index
