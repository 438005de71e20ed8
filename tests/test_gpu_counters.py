"""GPU: tick_count and kv_count counted in the packed record.

The step kernels keep both counters as their u64 field plus a 16-bit delta
in word 15 of the replica's 64 B record (drb_layout.hpp) and fold a delta
into its field only when it would pass 0xffff; the ABI still exports whole
counters.  Checked here:
  - the fold, against closed form: 66,000 ticking rounds with a proposal
    each take both counters across 0xffff (G = 64, and G = 300 with a
    partial last wave);
  - export and re-import in the middle of a run against the oracle: the
    deltas are non-zero at the export and zero after the import, so a delta
    that survived the import would count twice;
  - a mixed workload on a plain engine (the C3 kernels) and on a listed
    Quiesce engine (the EXT and lean kernels): replicas that fall back keep
    their pre-round counters, everyone else equals the oracle;
  - entries applied below term_start take their term from the ring: replicas
    at term 3 apply committed entries of term 2 (the C3 apply reads meta
    chunk 0 only there).
"""
import pytest

from dragonboat_amd import abi, workload
from oracle import pyoracle as po
from tests.gpu_harness import Pair, state_diff

pytestmark = pytest.mark.gpu

FB = abi.FB


def _diff_all(p, groups=None):
    """state_diff of every replica against the oracle, one export call."""
    est = p.eng.export_replicas(0, p.G)
    errs = []
    for g in (range(p.G) if groups is None else groups):
        for s in range(p.R):
            a, b = est[g * p.R + s], p.orc.export(g, s)
            if a.flags & (abi.F_FALLBACK | abi.F_ERROR):
                errs.append((g, s, "flags", a.flags, a.fallback_reason))
                continue
            d = state_diff(a, b, p.R)
            if d:
                errs.append((g, s, d))
    return errs


@pytest.mark.parametrize("G", [64, 300])
def test_counters_fold_past_16_bits(G):
    """66,000 rounds, each a tick and one 16 B KV write per group, 256
    rounds per drb_step_rounds call.  Closed form, no oracle: tick_count
    grows by the ticks given, kv_count by the advance of sm_index (every
    applied entry is a KV write); both cross 0xffff, so every replica folds
    each delta into its u64 field at least once."""
    R, ROUNDS, PER = 3, 66000, 256
    p = Pair(G=G, R=R)
    p.eng.gen_kv_proposals(0, 1, 256, 4, p.seed, 0)
    before = p.eng.export_replicas(0, G)
    chunk = (G + 255) // 256 * 256
    full = p.eng.round_array([dict(tick=True, prop_slot=0)] * PER)
    done = 0
    while done < ROUNDS:
        n = min(PER, ROUNDS - done)
        p.eng.step_rounds(full if n == PER else
                          [dict(tick=True, prop_slot=0)] * n, chunk)
        done += n
    out = p.eng.read_counters(reset=True)
    assert out.fallbacks == 0 and out.errors == 0, (out.to_dict(), p.why())
    after = p.eng.export_replicas(0, G)
    for i, (a, b) in enumerate(zip(before, after)):
        g, s = divmod(i, R)
        assert not b.flags & (abi.F_FALLBACK | abi.F_ERROR), (g, s)
        assert b.tick_count == a.tick_count + ROUNDS, (g, s, a.tick_count,
                                                       b.tick_count)
        assert b.kv_count == a.kv_count + (b.sm_index - a.sm_index), \
            (g, s, a.kv_count, b.kv_count, a.sm_index, b.sm_index)
        assert b.tick_count > 0xffff and b.kv_count > 0xffff, \
            (g, s, b.tick_count, b.kv_count)


def test_export_and_import_between_rounds():
    """40 rounds against the oracle, every replica's state compared every
    round; after round 20 every replica is exported and imported again."""
    G = 128
    p = Pair(G=G, R=3)
    for r in range(40):
        o, e = p.round(k=1, tick=(r % 4 != 3))
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        errs = _diff_all(p)
        assert not errs, (r, errs[:2])
        if r == 19:
            sts = p.eng.export_replicas(0, G)
            assert all(st.tick_count > 1 and st.kv_count > 0 for st in sts)
            p.eng.import_replicas(0, sts)
            errs = _diff_all(p)
            assert not errs, ("import", errs[:2])
    assert not p.check(groups=range(0, G, 8))


def _unhost(p, groups, slot):
    for g in groups:
        p.orc.set_hosted(g, slot, False)
        sts = p.eng.export_replicas(g, 1)
        sts[slot].flags &= ~abi.F_HOSTED
        p.eng.import_replicas(g, sts)


@pytest.mark.parametrize("quiesce", [False, True])
def test_mixed_workload_and_fallbacks_keep_counters(quiesce):
    """1 % of the groups propose per round, every round ticks.  Plain engine:
    the C3 kernels; Quiesce engine with listed rounds: the lean kernel and
    the full EXT one.  The leaders of four groups stop; their followers
    reach the election timeout and fall back before the round changes
    anything: their exported state, counters included, is the oracle's
    before that round.  Every other group equals the oracle throughout."""
    G, R, ERTT = 256, 3, 4
    kw = dict(election_rtt=ERTT)
    rkw = {}
    if quiesce:
        kw.update(quiesce=True, cmd_cap=144, kv_val_cap=128, kv_slots=32,
                  max_props=2, save_cap=8192, prop_slots=2)
        rkw.update(listed=True, encode_saves=True)
    p = Pair(G=G, R=R, **kw)
    E = [5, 70, 131, 255]
    lean = 0
    sample = sorted(set(range(0, G, 7)) | {g + d for g in E for d in (-1, 1)
                                           if 0 <= g + d < G})

    def one(r):
        nonlocal lean
        act = list(workload.active_groups(G, p.seed, r, 10000))
        snap = {(g, s): p.orc.export(g, s) for g in E for s in range(R)}
        o, e = p.round(k=1, tick=True, groups=act, **rkw)
        lean += e.to_dict().get("lean_stepped", 0)
        recs, lost = p.eng.take_flagged()
        assert lost == 0 and e.errors == 0
        for (g, s, reason, flags, _, _) in recs:
            assert g in E and s != 0 and reason == FB["ELECTION"], \
                (r, g, s, abi.FB_NAME.get(reason, reason))
            a = p.eng.export_replicas(g, 1)[s]
            assert a.flags & abi.F_FALLBACK
            d = state_diff(a, snap[(g, s)], R)
            assert not d, (r, g, s, d)
            assert (a.tick_count, a.kv_count) == \
                (snap[(g, s)].tick_count, snap[(g, s)].kv_count)
            if g not in p.cpu:
                p.to_cpu(g)
        return len(recs)

    for r in range(6):
        assert one(r) == 0
    assert not _diff_all(p)
    _unhost(p, E, 0)
    for r in range(6, 6 + 4 * ERTT):
        one(r)
        if len(p.cpu) == len(E):
            break
    assert sorted(p.cpu) == E
    for r in range(30, 40):
        assert one(r) == 0
    errs = _diff_all(p, p.live_groups())
    assert not errs, errs[:2]
    errs = p.check(groups=[g for g in sample if g not in p.cpu])
    assert not errs, errs[:2]
    if quiesce:
        assert lean > 0


def test_apply_below_term_start_reads_the_entry_term():
    """Every replica is imported at term 3 with three committed, unapplied
    KV writes of term 2 at the end of its log.  An import restarts the term
    cache (term_start = last + 1), so the apply takes these entries' term
    from the ring: sm_term must be 2, not the replica's term.  The proposals
    of the following rounds are appended at term 3 and applied from the
    cache.  Full state, logs, KV, messages against the oracle for 10
    rounds."""
    G, R, N = 128, 3, 3
    p = Pair(G=G, R=R)
    for g in range(G):
        reps = []
        for s in range(R):
            st = p.orc.export(g, s)
            base = st.last_index
            log = [po._etuple_to_dict(t)
                   for t in p.orc.export_log(g, s, 1, base)]
            for j in range(N):
                e = workload.proposal(p.seed, g, 1000, j, 256, 4)
                log.append(po.ent(term=2, index=base + 1 + j, type=e["type"],
                                  key=e["key"], client_id=e["client_id"],
                                  cmd=e["cmd"]))
            assert st.term == 2 and st.sm_index == base == st.committed
            st.term = st.prev_term = 3
            st.last_index = st.saved_to = st.committed = base + N
            st.prev_commit = base + N
            st.marker_index = base + N + 1
            if st.role == abi.LEADER:
                for q in range(R):
                    st.remotes[q].match = base + N
                    st.remotes[q].next = base + N + 1
            reps.append((st, log))
        p.import_group(g, reps)
    errs = _diff_all(p)
    assert not errs, ("import", errs[:2])
    for r in range(10):
        o, e = p.round(k=1, tick=True)
        assert e.fallbacks == 0 and e.errors == 0, (r, p.why())
        if r == 0:
            assert e.applied_entries == o.applied_entries == G * R * N
            for st in p.eng.export_replicas(0, G):
                assert (st.term, st.sm_term, st.kv_count) == (3, 2, N)
        errs = _diff_all(p)
        assert not errs, (r, errs[:2])
        errs = p.check(groups=range(0, G, 4))
        assert not errs, (r, errs[:2])
    for st in p.eng.export_replicas(0, G):
        assert st.sm_term == 3 and st.kv_count > N
