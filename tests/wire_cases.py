"""Hostile and non-canonical pb.Message bytes for the wire decoder.

One corpus for tests/test_msgdecode_host.py (drb_msgdec.hpp on the CPU under
AddressSanitizer / UBSan, against the oracle) and for
tests/test_gpu_wire_decode.py (the same bytes through drb_ingest_wire).

hand_cases() returns Case tuples whose expectation was written by hand from
the Go text (raftpb/raft_optimized.go unless another file is named): `go` is
the file:line it was read from.  Nothing here calls the oracle or the
decoder; the bytes are put together from the small encoders below, which
restate Message.MarshalTo (raftpb/message.go:32-124) and the colfer
Entry.marshalTo (raft_optimized.go:166-300).

outcome: "ok" (msg: the decoded fields, a po.msg()-shaped dict), "bad" (Go
refuses the bytes), "snapshot" (a Snapshot that is not the empty one: the
CPU path's) or "big" (decodes, a Cmd over cmd_cap: diverted).

Case k is addressed to shard first_shard + k, from replica 3 (the leader,
on another NodeHost) to replica 1; `placed` says whether an engine hosting
those shards takes it into an inbox (else it is dropped: an unknown shard
or replica).  The messages that are placed are harmless to step: a
Heartbeat with commit 0, or a Replicate whose LogIndex (10) is past the
follower's log and inside its window, which is rejected before its entries
are looked at (raft.go handleFollowerReplicate / handleReplicateMessage).
`steps` is False for the three answer types a follower's fast path does not
take (it hands the replica to the CPU path, DRB_FB_MESSAGE_TYPE): they are
decoded and placed, and not stepped here.

mutations() are seeded single-bit flips and single-byte deletions of two
canonical messages; they carry no expectation (oracle == decoder).
"""
import collections
import random
import struct
import zlib

Case = collections.namedtuple(
    "Case", "name data outcome msg go placed elem_tag elem_len_pad steps")

FROM, TO = 3, 1
HEARTBEAT, REPLICATE, READ_INDEX = 17, 12, 19
EMPTY_SNAPSHOT = bytes([0x12, 0, 0x18, 0, 0x20, 0, 0x28, 0, 0x32, 2, 0x08, 0,
                        0x48, 0, 0x50, 0, 0x58, 0, 0x60, 0, 0x68, 0, 0x70, 0])
SCALARS = ["type", "to", "from_", "shard_id", "term", "log_term", "log_index",
           "commit", "reject", "hint"]  # fields 1-10; hint_high is 13
U64 = (1 << 64) - 1


# ------------------------------------------------------------- encoders
def vi(v, total=0, last=None):
    """Varint of v; total > 0: with redundant continuation bytes (0x80 ...
    0x00) up to `total` bytes, the final byte `last` instead of 0."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    if total > len(out):
        out[-1] |= 0x80
        while len(out) < total - 1:
            out.append(0x80)
        out.append(0 if last is None else last)
    return bytes(out)


def tag(field, wt, total=0, last=None):
    return vi(field << 3 | wt, total, last)


def sc(field, v):
    return tag(field, 0) + vi(v)


def u64f(t, v, form=None):
    """colfer u64 field t (raft_optimized.go:166-190): omitted when 0, a
    varint below 2^49, else 8 bytes big endian behind the flagged header."""
    if form is None:
        form = "omit" if v == 0 else "var" if v < 1 << 49 else "flag"
    if form == "omit":
        return b""
    if form == "flag":
        return bytes([t | 0x80]) + struct.pack(">Q", v)
    return bytes([t]) + vi(v)


def ent(term=0, index=0, type=0, key=0, client_id=0, series_id=0,
        responded_to=0, cmd=b""):
    return dict(term=term, index=index, type=type, key=key,
                client_id=client_id, series_id=series_id,
                responded_to=responded_to, cmd=bytes(cmd))


def centry(e):
    """Entry.marshalTo: what a Go sender emits."""
    out = u64f(0, e["term"]) + u64f(1, e["index"])
    if e["type"]:
        out += b"\x02" + vi(e["type"])
    out += u64f(3, e["key"]) + u64f(4, e["client_id"])
    out += u64f(5, e["series_id"]) + u64f(6, e["responded_to"])
    if e["cmd"]:
        out += b"\x07" + vi(len(e["cmd"])) + e["cmd"]
    return out + b"\x7f"


def elem(body, field=11):
    return tag(field, 2) + vi(len(body)) + body


def msg(type, shard_id, term=2, log_term=0, log_index=0, commit=0, reject=0,
        hint=0, hint_high=0, entries=(), to=TO, from_=FROM):
    return dict(type=type, to=to, from_=from_, shard_id=shard_id, term=term,
                log_term=log_term, log_index=log_index, commit=commit,
                reject=reject, hint=hint, hint_high=hint_high,
                entries=list(entries))


def pieces(m, snapshot=EMPTY_SNAPSHOT):
    """Message.MarshalTo as a list of whole fields, in Go's order."""
    ps = [sc(i + 1, int(m[f])) for i, f in enumerate(SCALARS)]
    ps += [elem(centry(e)) for e in m["entries"]]
    ps.append(elem(snapshot, 12))
    ps.append(sc(13, m["hint_high"]))
    return ps


def cmsg(m, snapshot=EMPTY_SNAPSHOT):
    return b"".join(pieces(m, snapshot))


def heartbeat(shard, **kw):
    return msg(HEARTBEAT, shard, **kw)


def replicate(shard, entries=(), **kw):
    kw.setdefault("log_index", 10)
    kw.setdefault("log_term", 2)
    return msg(REPLICATE, shard, entries=entries, **kw)


def zero_msg():
    return msg(0, 0, term=0, to=0, from_=0)


# --------------------------------------------------- batches and frames
def batch(elems, did, src=b"peer:1", bin_ver=210, elem_tag=b"\x0a",
          elem_len_pad=0):
    """MessageBatch.MarshalTo (raftpb/messagebatch.go:23-70).  elem_tag /
    elem_len_pad re-encode the Requests elements' tag and length."""
    out = b""
    for e in elems:
        out += elem_tag + vi(len(e), len(vi(len(e))) + elem_len_pad
                             if elem_len_pad else 0) + e
    return out + b"\x10" + vi(did) + b"\x1a" + vi(len(src)) + src + \
        b"\x20" + vi(bin_ver)


def frame(payload):
    """writeMessage (internal/transport/tcp.go:142-178), both CRCs sound."""
    h = struct.pack(">HQ", 100, len(payload))
    pcrc = struct.pack(">I", zlib.crc32(payload))
    hcrc = struct.pack(">I", zlib.crc32(h + b"\0\0\0\0" + pcrc))
    return b"\xae\x7d" + h + hcrc + pcrc + payload


# ---------------------------------------------------------- hand cases
def hand_cases(first_shard=1, cmd_cap=32):
    cases = []

    def shard():
        return first_shard + len(cases)

    def add(name, data, outcome, go, m=None, placed=None, elem_tag=b"\x0a",
            elem_len_pad=0, steps=True):
        if placed is None:
            placed = outcome in ("ok", "big")
        assert (m is not None) == (outcome in ("ok", "big")), name
        cases.append(Case(name, bytes(data), outcome, m, go, placed, elem_tag,
                          elem_len_pad, steps))

    def add_rep_entry(name, ebytes, e, go, outcome="ok"):
        """A Replicate whose one Entries element is ebytes, expected e."""
        m = replicate(shard(), [e] if e else [])
        ps = pieces(replicate(shard()))
        data = b"".join(ps[:10]) + elem(ebytes) + b"".join(ps[10:])
        add(name, data, outcome, go, m if outcome in ("ok", "big") else None)

    # ---- canonical controls: what a Go sender emits -------------------
    for name, t in (("Replicate", 12), ("ReplicateResp", 13),
                    ("RequestVoteResp", 15), ("Heartbeat", 17),
                    ("HeartbeatResp", 18), ("ReadIndexResp", 20)):
        m = msg(t, shard(), log_index=10 if t == 12 else 0,
                log_term=2 if t == 12 else 0)
        add("canon_type_" + name, cmsg(m), "ok", "message.go:32-124", m,
            steps=t not in (13, 15, 18))
    for n in (0, 1, 3):
        m = replicate(shard(), [ent(term=2, index=11 + j, key=7 + j,
                                    client_id=9, series_id=1 + j,
                                    cmd=bytes([65 + j]) * (4 + j))
                                for j in range(n)])
        add("canon_replicate_%d_entries" % n, cmsg(m), "ok",
            "message.go:95-107", m)
    for f in ("term", "index", "key", "client_id", "series_id",
              "responded_to"):
        for v in (0, 1, 127, 128, (1 << 49) - 1, 1 << 49, 1 << 56, U64):
            e = ent(term=2, index=11, key=5, client_id=6, series_id=7,
                    responded_to=8, cmd=b"ab")
            e[f] = v
            m = replicate(shard(), [e])
            add("canon_entry_%s_%d" % (f, v), cmsg(m), "ok", ":166-300", m)
    for n in (0, 1, 127, 128, cmd_cap, cmd_cap + 1):
        e = ent(term=2, index=11, key=3, cmd=bytes(range(1, n + 1)))
        m = replicate(shard(), [e])
        add("canon_cmd_len_%d" % n, cmsg(m),
            "big" if n > cmd_cap else "ok", ":280-297", m)
    m = heartbeat(shard())
    add("canon_empty_snapshot", cmsg(m), "ok", "message.go:108-116", m)

    # ---- accepted by Go, never emitted ---------------------------------
    e = ent(term=2, index=11, key=4, cmd=b"xyz")
    for n in (1, 16):
        add_rep_entry("entry_%d_bytes_after_terminator" % n,
                      centry(e) + bytes(range(0x70, 0x70 + n)), e,
                      ":645-650 (called at :910)")
    # redundant continuation bytes: a tag, a scalar value, an Entries length
    for total, last in ((2, None), (5, None), (10, None), (10, 0x7e)):
        sfx = "%d%s" % (total, "_high_bits" if last else "")
        m = heartbeat(shard(), hint=77)
        ps = pieces(m)
        ps[9] = tag(10, 0, total, last) + vi(77)
        add("padded_tag_" + sfx, b"".join(ps), "ok", ":665-678", m)
        m = heartbeat(shard(), hint=77)
        ps = pieces(m)
        ps[9] = tag(10, 0) + vi(77, total, last)
        add("padded_value_" + sfx, b"".join(ps), "ok", ":865-878", m)
        m = replicate(shard(), [e])
        ps = pieces(m)
        ps[10] = tag(11, 2) + vi(len(centry(e)), total, last) + centry(e)
        add("padded_entries_length_" + sfx, b"".join(ps), "ok", ":883-897",
            m)
    # (a 10th byte of 1 is bit 63)
    m = heartbeat(shard(), hint=77 | 1 << 63)
    ps = pieces(m)
    ps[9] = tag(10, 0) + vi(77, 10, 1)
    add("padded_value_10_bit63", b"".join(ps), "ok", ":865-878", m)
    m = heartbeat(shard(), hint=5, hint_high=6)
    add("scalars_out_of_order", b"".join(reversed(pieces(m))), "ok",
        ":687-976 (a switch per tag: no order)", m)
    m = heartbeat(shard(), hint=9)
    ps = pieces(m)
    add("scalar_repeated_last_wins", b"".join(ps[:9]) + sc(10, 7) + sc(10, 9)
        + b"".join(ps[10:]), "ok", ":864", m)
    es = [ent(term=2, index=11 + j, key=j + 1, cmd=b"q" * j)
          for j in range(3)]
    # (Commit and LogTerm: fields a Replicate's mailbox record carries)
    m = replicate(shard(), es, commit=3, log_term=2)
    ps = pieces(replicate(shard(), log_term=1))
    add("scalars_between_entries", b"".join(ps[:10]) + elem(centry(es[0])) +
        sc(8, 3) + elem(centry(es[1])) + sc(6, 2) + elem(centry(es[2]))
        + b"".join(ps[10:]), "ok", ":879-913 (append)", m)
    for name, enc in (("2", b"\x02"), ("0x80_0x01", b"\x80\x01")):
        m = heartbeat(shard(), reject=1)
        ps = pieces(m)
        ps[8] = tag(9, 0) + enc
        add("reject_as_" + name, b"".join(ps), "ok", ":844-859 (v != 0)", m)
    # unknown fields (skipRaft, common.go:36-140)
    bodies = {0: vi(300), 1: bytes(range(8)), 2: vi(3) + b"abc",
              5: bytes(range(4))}
    k = 0
    for fnum in (14, 15, 16, 1 << 28):
        for wt in (0, 1, 2, 5):
            m = heartbeat(shard(), hint=k)
            ps = pieces(m)
            pos = (0, 6, len(ps))[k % 3]
            ps.insert(pos, tag(fnum, wt) + bodies[wt])
            add("unknown_field_%d_wt%d_%s" % (fnum, wt,
                                              ("first", "middle", "last")[k % 3]),
                b"".join(ps), "ok", ":963-975, common.go:56-97,132-134", m)
            k += 1
    m = heartbeat(shard())
    ps = pieces(m)
    ps.insert(3, tag(14, 2) + vi(0))
    add("unknown_bytes_field_length_0", b"".join(ps), "ok", "common.go:74-97",
        m)
    m = heartbeat(shard())
    add("unknown_bytes_field_ends_at_message_end",
        cmsg(m) + tag(15, 2) + vi(5) + b"tail!", "ok",
        ":972 (iNdEx + skippy == l)", m)
    # colfer forms
    e = ent(term=2, index=11, key=4)
    add_rep_entry("colfer_small_value_flagged",
                  u64f(0, 2, "flag") + u64f(1, 11) + u64f(3, 4, "flag") +
                  b"\x7f", e, ":343-352")
    big9 = 0xAB << 56 | 0x1234567
    e = ent(term=2, index=11, key=big9)
    b9 = bytearray()
    v = big9
    for _ in range(8):
        b9.append((v & 0x7f) | 0x80)
        v >>= 7
    b9.append(v)  # the 9th byte whole: 0xAB, its top bit is data
    assert v == 0xAB
    add_rep_entry("colfer_9_byte_varint", u64f(0, 2) + u64f(1, 11) +
                  b"\x03" + bytes(b9) + b"\x7f", e, ":332-335 (shift == 56)")
    e = ent(term=2, index=11, type=(1 << 32) - 5)
    add_rep_entry("colfer_type_negated", u64f(0, 2) + u64f(1, 11) +
                  b"\x82\x05\x7f", e, ":420-444 (^x + 1)")
    e = ent(term=2, index=11, type=0xF0000001)
    add_rep_entry("colfer_type_5_bytes_bits_above_32", u64f(0, 2) +
                  u64f(1, 11) + b"\x02\x81\x80\x80\x80\x7f\x7f", e,
                  ":397-416 (uint32 shift)")
    e = ent(term=2, index=11, type=3)
    add_rep_entry("colfer_type_overlong_7_bytes", u64f(0, 2) + u64f(1, 11) +
                  b"\x02\x83\x80\x80\x80\x80\x80\x01\x7f", e,
                  ":402-414 (no limit: bits shifted out are lost)")
    e = ent(term=2, index=11, cmd=b"hi")
    add_rep_entry("colfer_cmd_length_overlong_11_bytes", u64f(0, 2) +
                  u64f(1, 11) + b"\x07\x82" + b"\x80" * 9 + b"\x01hi\x7f",
                  e, ":608-626 (no limit)")
    m = heartbeat(shard())
    ps = pieces(m)
    ps[0] = tag(1, 0) + vi((1 << 32) + HEARTBEAT)
    add("message_type_above_2_32", b"".join(ps), "ok",
        ":692-706, types.go:6 (MessageType int32)", m)
    m = heartbeat(shard())
    ps = pieces(m)
    ps[0] = sc(1, 13)
    add("field_number_2_32_plus_1_is_field_1", b"".join(ps) +
        tag((1 << 32) + 1, 0) + vi(HEARTBEAT), "ok",
        ":679 (int32(wire >> 3))", m)
    add("field_number_2_31_refused", cmsg(heartbeat(shard())) +
        tag(1 << 31, 0) + vi(1), "bad", ":684 (fieldNum <= 0)")
    add("field_number_2_32_refused", cmsg(heartbeat(shard())) +
        tag(1 << 32, 0) + vi(1), "bad", ":684 (fieldNum <= 0)")
    add("empty_requests_element", b"", "ok", ":662 (no field: defaults)",
        zero_msg(), placed=False)
    m = heartbeat(shard())
    add("snapshot_field_length_0", cmsg(m, b""), "ok",
        ":914-943 (Snapshot.Unmarshal of no bytes)", m)
    snap = EMPTY_SNAPSHOT[:4] + b"\x20\x05" + EMPTY_SNAPSHOT[6:]  # Index 5
    add("snapshot_not_empty", cmsg(heartbeat(shard()), snap), "snapshot",
        ":914-943")
    ps = pieces(heartbeat(shard()), snap)
    add("snapshot_not_empty_then_cut_varint", b"".join(ps[:-1]) + b"\x68\x80",
        "bad", ":949-954 (io.ErrUnexpectedEOF)")

    # ---- refused by Go --------------------------------------------------
    # every prefix of a canonical two-entry Replicate: one that ends between
    # two fields is a message (of the fields before it), any other is
    # refused; they all go to a shard nobody hosts
    away = first_shard + (1 << 40)
    m2 = replicate(away, [ent(term=2, index=11, key=300, client_id=1 << 50,
                              cmd=b"first"),
                          ent(term=2, index=12, type=1, series_id=9,
                              responded_to=8, cmd=b"second!")],
                   commit=3, hint=200, hint_high=1 << 60)
    ps = pieces(m2)
    whole = b"".join(ps)
    ends = {}
    at = 0
    names = SCALARS + ["e0", "e1", "snapshot", "hint_high"]
    for j, p in enumerate(ps):
        at += len(p)
        ends[at] = j + 1
    for cut in range(len(whole)):
        if cut in ends or cut == 0:
            part = zero_msg()
            nf = ends.get(cut, 0)
            for f in SCALARS[:nf]:
                part[f] = m2[f]
            part["entries"] = m2["entries"][:max(0, min(2, nf - 10))]
            add("prefix_%d_after_%s" % (cut, names[nf - 1] if nf else "none"),
                whole[:cut], "ok", ":662 (iNdEx == l ends the loop)", part,
                placed=False)
        else:
            add("prefix_%d" % cut, whole[:cut], "bad",
                ":669,697,902 / :318-328,634 (EOF inside a field)")
    body = centry(ent(term=2, index=11, cmd=b"abc"))
    ps = pieces(replicate(shard()))
    add("entry_length_past_message_end", b"".join(ps[:10]) + tag(11, 2) +
        vi(len(body) + 5) + body, "bad", ":901-904")
    head = u64f(0, 2) + u64f(1, 11) + b"\x07"
    for name, n in (("equal_to", 4), ("one_more_than", 5)):
        # four bytes are left in the entry after the length: "abc", 0x7f
        add_rep_entry("cmd_length_%s_bytes_left" % name,
                      head + vi(n) + b"abc\x7f", None, ":632-636", "bad")
    add_rep_entry("cmd_length_above_16_MiB", head + vi((16 << 20) + 1) +
                  b"abc\x7f", None, ":632-636 (ColferSizeMax is 8 TiB, :33)",
                  "bad")
    add_rep_entry("cmd_length_above_ColferSizeMax", head + vi((8 << 40) + 1) +
                  b"abc\x7f", None, ":628-630", "bad")
    add_rep_entry("entry_without_terminator", head + vi(3) + b"abc\x00", None,
                  ":645-647", "bad")
    add_rep_entry("entry_ends_before_terminator", u64f(0, 2) + u64f(1, 11),
                  None, ":367-369", "bad")
    add_rep_entry("entry_length_0", b"", None, ":309-311", "bad")
    add_rep_entry("entry_headers_out_of_order", u64f(1, 11) + u64f(0, 2) +
                  b"\x7f", None, ":645-647 (header 0 after Index)", "bad")
    ps = pieces(heartbeat(shard()))
    add("varint_11_bytes_tag", b"".join(ps[:9]) + b"\x80" * 10 + b"\x00" +
        vi(1) + b"".join(ps[9:]), "bad", ":666-668")
    ps = pieces(heartbeat(shard()))
    add("varint_11_bytes_value", b"".join(ps[:9]) + tag(10, 0) + b"\x80" * 10
        + b"\x00" + b"".join(ps[10:]), "bad", ":866-868")
    ps = pieces(replicate(shard()))
    add("varint_11_bytes_entries_length", b"".join(ps[:10]) + tag(11, 2) +
        b"\x83" + b"\x80" * 9 + b"\x00" + b"\x00\x02\x7f" + b"".join(ps[10:]),
        "bad", ":885-887")
    for fnum in range(1, 14):
        ps = pieces(heartbeat(shard()))
        wrong = tag(fnum, 0) + vi(0) if fnum in (11, 12) else \
            tag(fnum, 2) + vi(0)
        ps.insert(fnum - 1 if fnum < 11 else 10, wrong)
        add("field_%d_wrong_wire_type" % fnum, b"".join(ps), "bad",
            ":689,708,727,746,765,784,803,822,841,861,880,915,945")
    add("field_number_0", cmsg(heartbeat(shard())) + b"\x00\x00", "bad",
        ":684-686")
    for wt, go in ((4, ":681-683"), (6, "common.go:135-136"),
                   (7, "common.go:135-136")):
        ps = pieces(heartbeat(shard()))
        ps.insert(5, tag(14, wt) + b"\x00")
        add("wire_type_%d" % wt, b"".join(ps), "bad", go)
    add("unknown_fixed64_cut_at_7", cmsg(heartbeat(shard())) + tag(14, 1) +
        bytes(7), "bad", "common.go:71-73, :972-974")
    add("unknown_fixed32_cut_at_3", cmsg(heartbeat(shard())) + tag(14, 5) +
        bytes(3), "bad", "common.go:132-134, :972-974")
    # the one deliberate refusal (drb_msgdec.hpp MD_REFUSE_GROUP): Go skips
    # a group (common.go:98-129); raft.proto has none, the decoder and the
    # oracle refuse it
    ps = pieces(heartbeat(shard()))
    ps.insert(4, tag(14, 3) + sc(1, 5) + tag(14, 4))
    add("refuse_group_wire_type_3", b"".join(ps), "bad",
        "common.go:98-129 accepts; MD_REFUSE_GROUP")

    # ---- batch level: the device's re-parse of the element's tag and
    # length (k_ing_elems) ----------------------------------------------
    m = heartbeat(shard(), hint=31)
    add("requests_tag_2_byte_varint", cmsg(m), "ok", ":1075-1090", m,
        elem_tag=b"\x8a\x00")
    m = heartbeat(shard(), hint=32)
    add("requests_length_redundant_continuation", cmsg(m), "ok",
        ":1095-1110", m, elem_len_pad=1)
    return cases


# ----------------------------------------------------------- mutations
MUT_SEED = 0x5EEDD8B0
MUT_COUNT = 4000


def mutation_bases(shard):
    es = [ent(term=2, index=11 + j, key=100 + j, client_id=1 << 50,
              series_id=3 + j, responded_to=2 + j, type=j & 1,
              cmd=bytes([97 + j]) * (5 + 7 * j)) for j in range(3)]
    return [("replicate3", cmsg(replicate(shard, es, commit=2))),
            ("readindex", cmsg(msg(READ_INDEX, shard, hint=0x1234567,
                                   hint_high=(1 << 63) + 99)))]


def mutations(shard=1, count=MUT_COUNT, seed=MUT_SEED):
    """[(name, message bytes)]: count single-bit flips and count single-byte
    deletions of each base, seeded.  (The Requests element's length is the
    message's own length wherever the bytes are framed: fixed up.)"""
    rng = random.Random(seed)
    out = []
    for bname, base in mutation_bases(shard):
        for k in range(count):
            at, bit = rng.randrange(len(base)), rng.randrange(8)
            b = bytearray(base)
            b[at] ^= 1 << bit
            out.append(("%s_flip_%d_%d_%d" % (bname, k, at, bit), bytes(b)))
        for k in range(count):
            at = rng.randrange(len(base))
            out.append(("%s_del_%d_%d" % (bname, k, at),
                        base[:at] + base[at + 1:]))
    return out


def mutation_sample(n=256, first_shard=1, seed=MUT_SEED + 1):
    """n of the mutations, sample j made from the bases of shard first_shard
    + j (a shard, hence a mailbox plane, of its own): the same picks of
    base, form and position as mutations() makes, drawn with their own
    seed."""
    rng = random.Random(seed)
    out = []
    for j in range(n):
        bname, base = mutation_bases(first_shard + j)[rng.randrange(2)]
        at, bit = rng.randrange(len(base)), rng.randrange(8)
        if rng.randrange(2):
            b = bytearray(base)
            b[at] ^= 1 << bit
            out.append(("%s_flip_s%d_%d_%d" % (bname, j, at, bit), bytes(b)))
        else:
            out.append(("%s_del_s%d_%d" % (bname, j, at),
                        base[:at] + base[at + 1:]))
    return out
