"""GPU parity at every group size: the launcher each kind resolves to.

The LOCAL kinds are built for R = 3 and 5 and run as their stand-ins at the
other R (drb_kinds.hpp); the lean kinds are built for every R.  An engine
without placement asks for the LOCAL kinds, so R = 1..8 walks both halves
of that mapping: plain rounds through kinds 9 / 10 (or 0 / 2), Quiesce
rounds (an EXT trigger) through 11 / 12 (or 1 / 3), and the listed rounds
among them through the lean kinds 7 / 8 first.  State, logs, KV, messages
and counters are compared with the oracle after every round.
"""
import pytest

from tests.gpu_harness import Pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("quiesce", [False, True])
@pytest.mark.parametrize("R", range(1, 9))
def test_every_group_size_steps_its_kinds(R, quiesce):
    p = Pair(G=80, R=R, quiesce=quiesce)  # one ragged wave beyond 64
    for r in range(8):
        o, e = p.round(k=1, tick=True, listed=quiesce and r % 2 == 1)
        assert (e.committed_entries, e.applied_entries, e.messages,
                e.ready_to_reads, e.dropped_read_indexes) == \
            (o.committed_entries, o.applied_entries, o.messages,
             o.ready_to_reads, o.dropped_read_indexes), (r, e.to_dict(),
                                                         o.to_dict())
        assert e.fallbacks == 0 and e.errors == 0, e.to_dict()
        errs = p.check()
        assert not errs, (r, errs[:3])
