"""CPU: tests/session_model.py pinned by the reference's own tests, restated
as known-answer tests (internal/rsm/statemachine_test.go:1264-1447,
session_test.go:58-117, lrusession_test.go:71-90).
"""
import random

import pytest

from tests import session_model as sm

# genTestKVData("test-key", "test-value") (statemachine_test.go:1028-1047)
DATA = b"\x0a\x08test-key\x12\x0atest-value"
CID = 12345


def register(m, cid=CID):
    return m.apply(cid, sm.SERIES_REGISTER, 0, sm.ENTRY_APPLICATION, b"")[0]


def unregister(m, cid=CID):
    return m.apply(cid, sm.SERIES_UNREGISTER, 0, sm.ENTRY_APPLICATION, b"")[0]


def update(m, series, responded_to=0, cid=CID, data=DATA):
    return m.apply(cid, series, responded_to, sm.ENTRY_APPLICATION, data)[0]


def test_session_can_be_created_and_removed():
    m = sm.Model()
    assert register(m) == (CID, False, False)
    assert m.lru.get(CID) is not None
    assert unregister(m) == (CID, False, False)
    assert m.lru.get(CID) is None


def test_duplicated_session_will_be_reported():
    m = sm.Model()
    assert register(m) == (CID, False, False)
    assert register(m) == (0, True, False)
    assert m.lru.get(CID) is not None


def test_removing_unregistered_session_will_be_reported():
    m = sm.Model()
    assert unregister(m) == (0, True, False)
    assert m.lru.get(CID) is None


def test_update_from_unregistered_client_will_be_reported():
    m = sm.Model()
    assert update(m, 1) == (0, True, False)
    assert m.count == 0 and not m.kv


def test_duplicated_update_will_not_be_applied_twice():
    m = sm.Model()
    register(m)
    assert update(m, 1) == (len(DATA), False, False)
    assert m.kv[b"test-key"] == b"test-value"
    count = m.count
    # the result again (ApplyUpdate is invoked), the SM not updated again
    assert update(m, 1) == (len(DATA), False, False)
    assert m.count == count == 1


def test_responded_update_will_not_be_applied_twice():
    m = sm.Model()
    register(m)
    update(m, 1)
    count = m.count
    update(m, 1, responded_to=1)
    assert m.lru.get(CID).responded_up_to == 1
    # ignored: ApplyUpdate is not invoked
    assert update(m, 1, responded_to=1) == (0, False, True)
    assert m.count == count


def test_noop_session_allows_entry_to_be_applied_twice():
    m = sm.Model()
    register(m)
    update(m, sm.NOOP_SERIES)
    count = m.count
    update(m, sm.NOOP_SERIES)
    assert m.count != count


@pytest.mark.parametrize("series,clear_to,size,probe,found", [
    ([1, 2, 3], 2, 1, 2, False), ([1, 2, 3], 2, 1, 3, True),
    ([1, 2, 3], 3, 0, 3, False), ([1, 2, 3], 4, 0, 3, False),
    ([3, 4, 5], 2, 3, 3, True), ([3, 4, 5], 6, 0, 5, False)])
def test_cached_response_data_can_be_cleared(series, clear_to, size, probe,
                                             found):
    s = sm.Session(0)
    for x, v in zip(series, (100, 200, 300)):
        s.add_response(x, v)
    s.clear_to(clear_to)
    assert len(s.history) == size
    assert (s.get_response(probe) is not None) == found


@pytest.mark.parametrize("series,clear_to,probe,want", [
    ([1, 2, 3], 2, 1, True), ([1, 2, 3], 2, 2, True),
    ([1, 2, 3], 2, 3, False), ([1, 2, 3], 3, 3, True),
    ([3, 4, 5], 2, 1, True), ([3, 4, 5], 2, 2, True),
    ([3, 4, 5], 2, 3, False)])
def test_whether_responded_can_be_returned(series, clear_to, probe, want):
    s = sm.Session(0)
    for x, v in zip(series, (100, 200, 300)):
        s.add_response(x, v)
    s.clear_to(clear_to)
    assert s.has_responded(probe) == want


def test_ordered_do_is_lru_ordered():
    m = sm.LRUSessions(100)
    for i in range(100):
        m.add(sm.Session(i))
    rnd = random.Random(1)
    for _ in range(100):
        idx = rnd.randrange(100)
        m.get(idx)
        ids = m.ordered()
        assert len(ids) == 100 and ids[99] == idx


def test_clear_to_equals_drop_every_key_at_or_below():
    """What the device restates: history keys are always above
    RespondedUpTo, so both of clearTo's branches are "drop every key <= to,
    RespondedUpTo = max"."""
    rnd = random.Random(2)
    for _ in range(300):
        s = sm.Session(1)
        upto = 0
        for _ in range(20):
            if rnd.random() < 0.6:
                x = s.responded_up_to + rnd.randrange(1, 6)
                if x not in s.history:
                    s.add_response(x, x * 10)
            else:
                to = rnd.randrange(0, s.responded_up_to + 7)
                keep = {k: v for k, v in s.history.items() if k > to}
                drop_all = to > upto
                before = dict(s.history)
                s.clear_to(to)
                upto = max(upto, to)
                assert s.responded_up_to == upto
                assert s.history == (keep if drop_all else before)


def test_snappy_update_value_is_the_decoded_length_and_is_cached():
    """Model.apply with the oracle's GetPayload: a Snappy-encoded update's
    Result.Value is the decoded payload's length (kvtest.go:161), not the
    Cmd's, and a retry of the series is served that value from the history
    without a second Update."""
    from oracle import pyoracle as po
    from tests import snappy_blocks as sb
    data = po.pbkv_marshal(b"test-key", b"z" * 200)
    cmd = sb.checked(sb.compress(data), data)
    assert len(cmd) < len(data) // 2
    m = sm.Model()
    register(m)
    first = m.apply(CID, 1, 0, sm.ENTRY_ENCODED, cmd, po.get_payload)
    assert first == ((len(data), False, False), "update")
    assert m.kv[b"test-key"] == b"z" * 200 and m.count == 1
    again = m.apply(CID, 1, 0, sm.ENTRY_ENCODED, cmd, po.get_payload)
    assert again == ((len(data), False, False), "cached")
    assert m.count == 1 and m.sessions() == [(CID, 0, {1: len(data)})]
    # the default payload function still refuses a compressed Cmd
    with pytest.raises(AssertionError):
        sm.Model().apply(0x77, 0, 0, sm.ENTRY_ENCODED, cmd)
