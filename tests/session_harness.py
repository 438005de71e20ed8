"""The checker of the GPU session tests (tests/test_gpu_sessions.py,
test_gpu_session_carriers.py, test_gpu_session_shapes.py).

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

The expected bytes of a carrier (EntryBatch, batched records, tan records,
wire streams) follow the same rule: what the oracle saved or sent on the
twin, the staged entries put back by Key (Twins.real is the one source),
marshalled by the oracle's codecs -- which are not the code under test.
tests/test_session_expected.py checks that half alone, without a GPU.
"""
import ctypes as C
import struct
import zlib

from dragonboat_amd import abi, workload
from dragonboat_amd.engine import tan_scan
from oracle import pyoracle as po
from tests import session_model as sm
from tests import wire_ref as wr
from tests.gpu_harness import Pair, by_dest, state_diff

APP = abi.ENTRY_APPLICATION
REG, UNREG = abi.SERIES_REGISTER, abi.SERIES_UNREGISTER
FIRST_SHARD = 1  # drb_config.first_shard_id's default, the oracle's too
SRC = b"gpu-node-7.example:26001"
TAN_FILLER = 6  # filler rounds in front of a script in the tan tests


def pbkv(key, val):
    """PBKV{key, val} marshalled (short fields)."""
    return b"\x0a" + bytes([len(key)]) + key + b"\x12" + bytes([len(val)]) + val


def ent(client, series, responded_to=0, cmd=b"", typ=APP):
    return dict(client_id=client, series_id=series, responded_to=responded_to,
                type=typ, cmd=cmd)


def cl(g, n):
    """Client n of group g: ids over the whole 64 bits, never 0."""
    return workload.mix64(0xC11E + 8 * g + n) | 1


def val(g):
    return struct.pack("<I", workload.mix64(g) & 0xffffffff)


def wide(g):
    """One client whose SeriesID and RespondedTo cross 2^49, where colfer
    goes from a varint to the fixed 8-byte form, up to the largest series a
    client can send; each update answers the one before."""
    A, v = cl(g, 0), val(g)
    s = [2 ** 49 - 1, 2 ** 49, 2 ** 56 + g, 2 ** 63 + g, 2 ** 64 - 3]
    steps = [ent(A, REG)]
    steps += [ent(A, x, r, pbkv(b"w%d" % i, v))
              for i, (x, r) in enumerate(zip(s, [0] + s[:-1]))]
    steps += [ent(A, s[-1], s[-1], pbkv(b"w9", v)),  # responded: ignored
              ent(A, UNREG)]
    return steps


def script_rounds(G, steps, per_round=3, drain=4):
    """The rounds of a script: group g's steps, per_round a round, its
    phase g % 4 rounds late; ticks and ReadIndex rounds mixed in.  Yields
    (rows, tick, read_index)."""
    n = max(len(steps(g)) for g in range(G))
    rounds = (n + per_round - 1) // per_round + 3
    for r in range(rounds + drain):
        rows = {}
        for g in range(G):
            q = r - g % 4
            part = steps(g)[per_round * q:per_round * (q + 1)] if q >= 0 \
                else []
            if part:
                rows[g] = part
        yield rows, r % 2 == 0, r % 3 == 0


def filler_rounds(G, n):
    """n rounds of three NoOP-session proposals a group (no session entry
    among them), to move a script along the log."""
    return [({g: [ent(cl(g, 5), 0, 0, pbkv(b"f", b"%d" % (r % 10)))] * 3
              for g in range(G)}, r % 2 == 0, False) for r in range(n)]


def bits(res):
    """drb_apply_result.ignored of a model result (value, rejected,
    ignored)."""
    return (abi.APPLY_IGNORED if res[2] else 0) | \
        (abi.APPLY_REJECTED if res[1] else 0)


class Twins:
    """The staged entries by Key and the expected bytes of every carrier.
    Needs self.orc (a po.Cluster stepped on the twins), self.G, self.R."""

    def init_twins(self):
        self.real = {}    # Key -> the staged entry (tuple fields 4..7)
        self.nkey = 0

    def init_models(self, base, payload=sm.get_payload):
        """The model of each group, its snapshots and results per index;
        base: every group's sm_index at the start."""
        self.base = list(base)
        self.payload = payload  # GetPayload of the model (Model.apply)
        self.model = [sm.Model() for _ in range(self.G)]
        self.snaps = [{self.base[g]: self.model[g].snapshot()}
                      for g in range(self.G)]
        self.results = [{} for _ in range(self.G)]
        self.classes = {}  # outcome class -> {(wave, slot)}
        self.sm_seen = {}

    def advance_group(self, g, hi, log_of):
        """Group g's model up to index hi over log_of(lo, hi), the entry
        tuples of a replica that holds them."""
        done = max(self.snaps[g])
        if hi <= done:
            return
        for t in log_of(done + 1, hi):
            res, cls = self.model[g].apply(t[4], t[5], t[6], t[2], t[7],
                                           self.payload)
            self.snaps[g][t[1]] = self.model[g].snapshot()
            self.results[g][t[1]] = (res, cls, t[3])

    def check_sm_of(self, eng, lane, g, s, a, w):
        """Replica (g, s), held by eng at `lane` with state a: its KV,
        kv_count and sessions against the model at its own sm_index
        (exported only when that moved)."""
        if self.sm_seen.get((g, s)) == a.sm_index:
            return
        kv, count, sessions = self.snaps[g][a.sm_index]
        assert a.kv_count == count, (w, a.kv_count, count)
        assert eng.kv_export(lane, s) == kv, w
        assert eng.sessions_export(lane, s) == sessions, \
            (w, eng.sessions_export(lane, s), sessions)
        for i in range(self.sm_seen.get((g, s), self.base[g]) + 1,
                       a.sm_index + 1):
            self.classes.setdefault(self.results[g][i][1], set()).add(
                (g // 64, s))
        self.sm_seen[g, s] = a.sm_index

    def build_rows(self, rows, mp, k):
        """rows: {g: [ent(...)]} -> (counts, the real batch [g][mp], its
        no-op twin [g][k], the Cmd pool)."""
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
        return counts, real, twin, pbuf

    # ------------------------------------------------------------- the twin
    def _back(self, t):
        """An oracle entry tuple with the staged entry put back by Key."""
        r = self.real.get(t[3])
        return t if r is None else t[:4] + r

    def back_dict(self, e):
        """_back of an entry dict (po.ent's fields)."""
        r = self.real.get(e["key"])
        if r is None:
            return e
        return dict(e, client_id=r[0], series_id=r[1], responded_to=r[2],
                    cmd=r[3])

    def _msgs(self, msgs):
        return by_dest(self.back_outbox(msgs))

    def back_outbox(self, msgs):
        return [m[:11] + (tuple(self._back(t) for t in m[11]),) for m in msgs]

    # ------------------------------------------------------ expected bytes
    def saved_entries(self, g, s):
        """Replica (g, s)'s EntriesToSave of the last round, put back."""
        ob, _ = self.orc.export_saved(g, s)
        return [self.back_dict(e) for e in po.entrybatch_unmarshal(ob)] \
            if ob else []

    def expected_saved(self, g, s):
        """(EntryBatch bytes, crc32) drb_export_saved must give."""
        ents = self.saved_entries(g, s)
        b = po.entrybatch_marshal(ents) if ents else b""
        return b, (zlib.crc32(b) if b else 0)

    def expected_records(self, db, g, s):
        """[(batch id, value, crc32)] drb_export_save_records must give;
        db: the po.BatchDB that has taken every earlier round."""
        ents = self.saved_entries(g, s)
        return [(b, v, zlib.crc32(v)) for b, v in
                db.record(FIRST_SHARD + g, s + 1, ents)] if ents else []

    def wire_messages(self, frm, to):
        """The plane's messages with the entries put back first: the batch
        cut depends on the Cmd lengths."""
        return wr.plane_messages(
            lambda g, s: self.back_outbox(self.orc.export_outbox(g, s)),
            self.G, frm, to)


class OrcPair(Twins):
    """The reference half alone: an oracle cluster stepped on the twins
    (tests/test_session_expected.py)."""

    def __init__(self, G, R=3, seed=0x5EEDD8B0):
        self.G, self.R, self.seed = G, R, seed
        self.orc = po.Cluster(G, R, seed=seed)
        self.orc.setup_steady(0)
        self.init_twins()
        self.rounds = 0

    def sess_round(self, rows=None, tick=False, read_index=False,
                   prop_replica=0):
        if rows:
            k = max(len(v) for v in rows.values())
            counts, _, twin, pbuf = self.build_rows(rows, k, k)
            self.orc.stage_proposals(counts, k, twin, pbuf, prop_replica)
        if read_index:
            lo, hi = workload.build_read_index(self.G, self.seed, self.rounds,
                                               self.rounds + 30, None)
            self.orc.stage_read_index(lo, hi, 0)
        self.rounds += 1
        return self.orc.round(tick=tick)


class TanTwins:
    """Per tan db a twin (what the oracle writes for the no-op twins) and a
    real one (the expected files).  The twin's record tells whether the
    round writes one and with which State; the real db takes that State and
    the put-back EntriesToSave."""

    def __init__(self, t, max_log, mux=False):
        self.t, self.mux = t, mux
        n = (t.R, 16) if mux else (t.G, t.R)
        self.twin = [[po.TanDB(max_log) for _ in range(n[1])]
                     for _ in range(n[0])]
        self.real = [[po.TanDB(max_log) for _ in range(n[1])]
                     for _ in range(n[0])]

    def dbs(self, g, s):
        if self.mux:
            c = (FIRST_SHARD + g) % 16
            return self.twin[s][c], self.real[s][c]
        return self.twin[g][s], self.real[g][s]

    def write(self, g, s):
        """Replica (g, s)'s expected record of the last round (TanDB.last()
        of the real db) or None.  Multiplexed: call in the shared log's
        order, groups ascending per slot."""
        twin, real = self.dbs(g, s)
        w = self.t.orc.tan_write(g, s, twin)
        ents = self.t.saved_entries(g, s)
        if w is None:
            assert not ents, (g, s)
            return None
        _, _, recs = tan_scan(twin.file(w["log"]))
        last = recs[-1]
        assert last["offset"] == w["off"] and \
            last["shard_id"] == FIRST_SHARD + g, (g, s, last, w)
        state = (last["term"], last["vote"], last["commit"]) \
            if last["has_state"] else None
        want = real.write(FIRST_SHARD + g, s + 1, state, ents)
        assert want is not None, (g, s)
        return want


def check_tan_round(p, tt, logs, r):
    """Every replica's tan record of the round against the expected one
    (tests/test_gpu_tan.py::_check_round's comparisons); the engine's bytes
    are appended to its log images {(g, s, log): bytearray}."""
    n = 0
    for g in range(p.G):
        for s in range(p.R):
            want = tt.write(g, s)
            rec, data = p.eng.export_tan(g, s)
            where = (r, g, s, rec, want)
            if want is None:
                assert not rec["flags"] & abi.TAN_WRITTEN, where
                assert rec["len"] == 0, where
                continue
            assert rec["flags"] & abi.TAN_WRITTEN, where
            assert (rec["offset"], rec["len"], rec["log"]) == \
                (want["off"], want["len"], want["log"]), where
            assert bool(rec["flags"] & abi.TAN_SYNC) == want["sync"], where
            assert bool(rec["flags"] & abi.TAN_NEW_LOG) == want["new_log"], \
                where
            f = tt.dbs(g, s)[1].file(want["log"])
            assert data == f[want["off"]:want["off"] + want["len"]], where
            img = logs.setdefault((g, s, rec["log"]), bytearray())
            assert len(img) == rec["offset"], where
            img += data
            n += 1
    return n


def check_tan_mux_round(p, tt, logs, r):
    """The multiplexed round (tests/test_gpu_tan.py::_mux_round's
    comparisons) against the real shared dbs; the staged bytes of every log
    are appended to logs {(s, key, log): bytearray}."""
    n = 0
    for s in range(p.R):
        for c in range(16):
            db = tt.real[s][c]
            before = db.last()["offset"]
            pieces, syncs, fresh = [], False, False
            for g in range(p.G):
                if (FIRST_SHARD + g) % 16 != c:
                    continue
                want = tt.write(g, s)
                rec, data = p.eng.export_tan(g, s)
                where = (r, s, c, g, rec, want)
                if want is None:
                    assert not rec["flags"] & abi.TAN_WRITTEN, where
                    continue
                assert rec["flags"] & abi.TAN_WRITTEN, where
                assert (rec["offset"], rec["len"], rec["log"]) == \
                    (want["off"], want["len"], want["log"]), where
                assert bool(rec["flags"] & abi.TAN_SYNC) == want["sync"], \
                    where
                assert bool(rec["flags"] & abi.TAN_NEW_LOG) == \
                    want["new_log"], where
                f = db.file(want["log"])
                assert data == f[want["off"]:want["off"] + want["len"]], where
                img = logs.setdefault((s, c, rec["log"]), bytearray())
                assert len(img) == rec["offset"], where
                img += data
                pieces.append(data)
                syncs |= want["sync"]
                fresh |= want["new_log"]
                n += 1
            lg, staged = p.eng.export_tan_log(s, c)
            where = (r, s, c, lg)
            assert staged == b"".join(pieces), where
            assert lg["start_offset"] == before, where
            end = db.last()["offset"]
            assert lg["end_offset"] == end, where
            assert bool(lg["flags"] & abi.TAN_SYNC) == syncs, where
            assert bool(lg["flags"] & abi.TAN_NEW_LOG) == fresh, where
            if pieces:
                assert p.eng.tan_get(next(
                    g for g in range(p.G)
                    if (FIRST_SHARD + g) % 16 == c), s)[0] == end, where
    return n


def check_wire_planes(p, eng, did, limits, planes=None, cov=None):
    """tests/test_gpu_wire.py::_check_planes against the put-back stream;
    cov (a Coverage) takes the entries of the compared messages."""
    planes = planes or [(a, b) for a in range(p.R) for b in range(p.R)
                        if a != b]
    n = 0
    for frm, to in planes:
        msgs = p.wire_messages(frm, to)
        for lim in limits:
            res, data = eng.encode_wire(frm, to, did, SRC, max_batch=lim)
            exp = wr.expected_stream(msgs, did, SRC, lim or wr.MAX_MSG_BATCH)
            assert res["n_msgs"] == len(msgs), (frm, to, lim)
            assert res["n_bytes"] == len(exp), (frm, to, lim)
            if data != exp:
                i = next(k for k in range(min(len(data), len(exp)))
                         if data[k] != exp[k])
                raise AssertionError((frm, to, lim, "first diff at", i,
                                      data[max(0, i - 8):i + 8].hex(),
                                      exp[max(0, i - 8):i + 8].hex()))
            assert res["n_frames"] == len(
                wr.split_batches(msgs, lim or wr.MAX_MSG_BATCH))
        n += len(msgs)
        for m in msgs if cov is not None else ():
            cov.add(m["entries"])
    return n


class Coverage:
    """What the compared bytes held: the session fields of every decoded
    entry, for the coverage assertions of the carrier tests."""

    def __init__(self):
        self.series, self.responded = set(), set()

    def add(self, ents):
        for e in ents:
            self.series.add(e["series_id"])
            self.responded.add(e["responded_to"])

    def check(self, wide=False):
        assert REG in self.series, "no register"
        assert UNREG in self.series, "no unregister"
        assert any(self.responded - {0}), "no responded_to"
        if wide:  # both colfer forms (fixed 8 bytes from 2^49) of both
            for f in (self.series, self.responded):
                assert any(0 < x < 2 ** 49 for x in f), f
                assert any(x >= 2 ** 49 for x in f), f


class SessPair(Twins, Pair):
    def __init__(self, G, payload=sm.get_payload, **kw):
        kw.setdefault("cmd_cap", 32)
        kw.setdefault("kv_val_cap", 4)
        kw.setdefault("max_props", 3)
        kw.setdefault("window", 64)
        super().__init__(G, **kw)
        self.init_twins()
        sts = self.eng.export_replicas(0, G)
        self.init_models([sts[g * self.R].sm_index for g in range(G)],
                         payload)
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
        counts, real, twin, pbuf = self.build_rows(rows, mp, k)
        self.orc.stage_proposals(counts, k, twin, pbuf, prop_replica)
        self.eng.stage_proposals(0, counts, real, pbuf)

    def sess_round(self, rows=None, tick=False, read_index=False,
                   prop_replica=0, check=True, encode_saves=False,
                   listed=False):
        pin = abi.DRB_NONE
        if rows:
            self.stage_rows(rows, prop_replica)
            pin = 0
        _, ri_in = self.stage(k=0, read_index=read_index)
        o = self.orc.round(tick=tick)
        e = self.eng.step(tick=tick, prop_slot=pin, ri_slot=ri_in,
                          prop_replica=prop_replica,
                          encode_saves=encode_saves, listed=listed)
        self.rounds += 1
        if check:
            self.check_round(o, e)
        return o, e

    def advance_model(self, sts):
        """The model of every group up to the highest sm_index of its
        replicas, over the leader's (or any up-to-date replica's) log."""
        for g in range(self.G):
            reps = sts[g * self.R:(g + 1) * self.R]
            hi = max(a.sm_index for a in reps)
            src = max(range(self.R), key=lambda s: reps[s].sm_index)
            self.advance_group(
                g, hi, lambda lo, hi: self.eng.export_log(g, src, lo, hi))

    def check_round(self, o, e, fallbacks=0, groups=None):
        """groups: only these (the others have left the fast path: the
        round's counters are then not the oracle's)."""
        where = self.rounds
        assert e.errors == 0, (where, e.to_dict(), self.why())
        if groups is None:
            assert e.fallbacks == fallbacks, (where, e.to_dict(), self.why())
            assert (e.applied_entries, e.messages) == \
                (o.applied_entries, o.messages), \
                (where, e.to_dict(), o.to_dict())
        sts = self.eng.export_replicas(0, self.G)
        self.advance_model(sts)
        lead_res = {}
        for g in (range(self.G) if groups is None else groups):
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
        self.check_sm_of(self.eng, g, g, s, a, w)
