"""A plain-Python model of the reference's rsm session code, the checker of
the device's session path (the C oracle panics on session-managed entries).

Restated from internal/rsm: Session (session.go:49-107), lrusession.go,
SessionManager (sessionmanager.go:44-125), StateMachine.handleEntry / update
(statemachine.go:935-969, 1033-1103) over KVTest (internal/tests/kvtest.go:
145-162, Result.Value = len(payload), Count incremented per Update) and
GetPayload for uncompressed entries (encoded.go:55-65).  Capacity 4096 with
LRU eviction and unbounded histories, as the reference runs it.

tests/test_session_model.py pins it with the reference's own tests.
"""
from collections import OrderedDict

SERIES_REGISTER = 2 ** 64 - 2      # client.SeriesIDForRegister
SERIES_UNREGISTER = 2 ** 64 - 1    # client.SeriesIDForUnregister
NOOP_SERIES = 0                    # client.NoOPSeriesID
LRU_MAX_SESSIONS = 4096            # settings.Hard.LRUMaxSessionCount

ENTRY_APPLICATION, ENTRY_CONFIG_CHANGE, ENTRY_ENCODED = 0, 1, 2


class Session:
    def __init__(self, client_id):
        self.client_id = client_id
        self.responded_up_to = 0
        self.history = {}

    def get_response(self, series):
        return self.history.get(series)

    def add_response(self, series, value):
        assert series not in self.history, "adding a duplicated response"
        self.history[series] = value

    def clear_to(self, to):
        if to <= self.responded_up_to:
            return
        if to == self.responded_up_to + 1:
            self.history.pop(to, None)
            self.responded_up_to = to
            return
        self.responded_up_to = to
        for k in [k for k in self.history if k <= to]:
            del self.history[k]

    def has_responded(self, series):
        return series <= self.responded_up_to

    def snapshot(self):
        return (self.client_id, self.responded_up_to, dict(self.history))


class LRUSessions:
    """lrusession: getSession and addSession move the session to the most
    recently used end; ordered() walks least recently used first."""

    def __init__(self, size=LRU_MAX_SESSIONS):
        self.size = size
        self.sessions = OrderedDict()

    def add(self, s):
        self.sessions[s.client_id] = s
        self.sessions.move_to_end(s.client_id)
        while len(self.sessions) > self.size:
            self.sessions.popitem(last=False)

    def get(self, client_id):
        s = self.sessions.get(client_id)
        if s is not None:
            self.sessions.move_to_end(client_id)
        return s

    def delete(self, client_id):
        self.sessions.pop(client_id, None)

    def ordered(self):
        return list(self.sessions)


def pbkv(cmd):
    """PBKV.Unmarshal (kvpb/kv.go) of the two string fields: (key, val)."""
    key = val = b""
    i = 0
    while i < len(cmd):
        tag = cmd[i]
        i += 1
        n = sh = 0
        while True:
            b = cmd[i]
            i += 1
            n |= (b & 0x7f) << sh
            sh += 7
            if not b & 0x80:
                break
        assert tag in (0x0a, 0x12) and i + n <= len(cmd), cmd.hex()
        if tag == 0x0a:
            key = bytes(cmd[i:i + n])
        else:
            val = bytes(cmd[i:i + n])
        i += n
    return key, val


def get_payload(typ, cmd):
    if typ == ENTRY_ENCODED:
        assert cmd and cmd[0] == 0, "the model takes uncompressed entries"
        return cmd[1:]
    return cmd


class Model:
    """One replica's state machine: sessions, the KV and Count."""

    def __init__(self, size=LRU_MAX_SESSIONS):
        self.lru = LRUSessions(size)
        self.kv = {}
        self.count = 0
        self.applied = 0

    # outcome classes, named as the device names them (drb_session.hpp)
    def apply(self, client_id, series_id, responded_to, typ, cmd,
              payload=get_payload):
        """handleEntry: ((value, rejected, ignored), outcome class).
        payload(typ, cmd) is GetPayload: this module's for uncompressed
        entries, the oracle's (po.get_payload) where Cmds are Snappy blocks;
        Result.Value is the decoded payload's length (kvtest.go:161)."""
        self.applied += 1
        assert typ != ENTRY_CONFIG_CHANGE
        if client_id == 0:  # not session managed
            assert not cmd, "not session managed, not empty"
            return (0, False, True), "noop"
        if not cmd and series_id == SERIES_REGISTER:
            if self.lru.get(client_id) is not None:
                return (0, True, False), "register-duplicate"
            self.lru.add(Session(client_id))
            return (client_id, False, False), "registered"
        if not cmd and series_id == SERIES_UNREGISTER:
            if self.lru.get(client_id) is None:
                return (0, True, False), "unregister-unknown"
            self.lru.delete(client_id)
            return (client_id, False, False), "unregistered"
        s = None
        if series_id != NOOP_SERIES:
            s = self.lru.get(client_id)
            if s is None:
                return (0, True, False), "unknown-client"
            s.clear_to(responded_to)
            if s.has_responded(series_id):
                return (0, False, True), "responded"
            v = s.get_response(series_id)
            if v is not None:
                return (v, False, False), "cached"
        data = payload(typ, cmd)
        key, val = pbkv(data)
        self.kv[key] = val
        self.count += 1
        value = len(data)
        if s is not None:
            s.add_response(series_id, value)
        return (value, False, False), "update" if s else "noop-session"

    def sessions(self):
        """[(client_id, responded_up_to, {series: value})], least recently
        used first (lrusession.save's order)."""
        return [self.lru.sessions[c].snapshot() for c in self.lru.ordered()]

    def snapshot(self):
        return (dict(self.kv), self.count, self.sessions())
