"""uvhttp_ws_echo_messages (the host twin of the device echo of data messages) against the
frames the product's process_data makes of a recording on_message (tests/_echo_ref.py): message
lengths at the header steps, fragmented messages with empty fragments and a PING in between, a
message completing after a CLOSE, a connection that fails part-way, enable = 0, client
connections with keys by echo slot and without keys, SERVER_SEND, messages carried in and still
open, a missing carry, the capacity failures and a seeded mix."""
import random

import pytest

import _echo_ref as ER

LENGTHS = [0, 1, 125, 126, 127, 65535, 65536, 65537]


@pytest.fixture(scope="module")
def U():
    import uvhttp_amd as U
    return U


def _decode(conns, is_server=None, pending=None):
    wire, st = ER.streams_of(conns, is_server, pending)
    w, desc, first, nd, out = ER.FR.oracle_decode(wire, st)
    return w, desc, first, nd, out


def _check(U, conns, is_server=None, enable=None, keys=None, flags=0, pending=None, delivered=None,
           silent=(), carries=None):
    """host twin == on_message reference for every connection of `conns`"""
    w, desc, first, nd, out = _decode(conns, is_server, pending)
    if delivered is not None:
        assert nd == delivered
    want = ER.expected_batch(conns, is_server, enable, keys, flags, None, pending, silent)
    got = ER.host_batch(U, w, desc, first, nd, is_server, enable, keys, flags, pending, carries)
    assert got == want
    for s, c in enumerate(got["conn"]):  # the open message is the decoder's pending message
        if c["status"] == ER.OK and (enable is None or enable[s]):
            assert c["open_len"] == int(out["frag_size"][s])
            assert c["open_len"] == 0 or c["open_opcode"] == int(out["frag_opcode"][s])
    return got


def _payload(n, salt=0):
    return bytes((salt + 31 * i + (i >> 8)) & 0xFF for i in range(n))


@pytest.mark.parametrize("op", [1, 2])
@pytest.mark.parametrize("n", LENGTHS)
def test_unfragmented_lengths(U, n, op):
    p = _payload(n, op)
    got = _check(U, [[ER.Fr(op, 1, p)]])
    hdr = 2 if n <= 125 else 4 if n <= 65535 else 10
    assert got["conn"][0] == dict(ER.ZERO, n_echoes=1, out_len=hdr + n)
    assert got["out"][0] == 0x80 | op and got["out"][hdr:] == p


def test_fragmented_messages(U):
    P = ER.ping(b"\xff\xfe")
    conns = [
        [ER.text(b"ab", 0), ER.cont(b"cd")],
        [ER.binary(b"abc", 0), ER.cont(b"", 0), ER.cont(b"defg")],
        [ER.text(b"x" * 100, 0), P, ER.cont(b"y" * 30, 0), P, P, ER.cont(b"")],
        [ER.text(b"", 0), ER.text(b"fresh")],  # an empty first fragment opens nothing
        [ER.text(b"one"), ER.binary(b"q" * 70000, 0), ER.cont(b"r" * 3), ER.text(b"")],
    ]
    got = _check(U, conns, delivered=[2, 3, 6, 2, 4])
    assert [c["n_echoes"] for c in got["conn"]] == [1, 1, 1, 1, 3]
    assert got["out"][:6] == b"\x81\x04abcd"
    assert got["out"][6:15] == b"\x82\x07abcdefg"


def test_message_completing_after_a_close(U):
    conns = [[ER.text(b"before"), ER.text(b"open", 0), ER.close(b"\x03\xe8"), ER.cont(b"ed"), ER.text(b"after")],
             [ER.close(b""), ER.binary(b"late", 0)]]
    got = _check(U, conns, delivered=[5, 2])
    assert got["out"] == b"\x81\x06before"
    assert got["conn"][1] == dict(ER.ZERO, first_echo=1, open_len=4, open_opcode=2) and got["open"] == b"late"


def test_failure_at_frame_k(U):
    frames = [ER.text(b"ok"), ER.binary(b"part", 0), ER.Fr(0, 1, b"bad", rsv=True), ER.text(b"never")]
    got = _check(U, [frames], delivered=[2])
    assert got["out"] == b"\x81\x02ok" and got["open"] == b"part" and got["conn"][0]["open_opcode"] == 2


def test_enable_zero(U):
    conns = [[ER.text(b"a")], [ER.text(b"quiet"), ER.text(b"op", 0)], [], [ER.binary(b"b")]]
    got = _check(U, conns, enable=[1, 0, 1, 1])
    assert got["conn"][1] == dict(ER.ZERO, first_echo=1) and got["conn"][3]["first_echo"] == 1
    assert got["out"] == b"\x81\x01a\x82\x01b"


def test_client_connections_mask_by_echo_slot(U):
    rng = random.Random(11)
    conns = [[ER.text(b"abcde"), ER.ping(b"p"), ER.binary(b"fr", 0), ER.cont(b"agment")], [ER.text(_payload(300))]]
    keys = ER.keys_for(rng, 8)
    got = _check(U, conns, is_server=[0, 0], keys=keys)
    k0 = ER.key_bytes(keys[0])
    assert got["out"][:6] == b"\x81\x85" + k0
    assert got["out"][6:11] == bytes(a ^ b for a, b in zip(b"abcde", k0 * 2))
    assert got["conn"][1]["first_echo"] == 2 and got["conn"][1]["out_len"] == 8 + 300
    # no key table: a client connection gets nothing and says why; a server one needs none
    got = _check(U, conns + [[ER.text(b"srv")]], is_server=[0, 0, 1], keys=None)
    assert [c["status"] for c in got["conn"]] == [ER.NO_KEYS, ER.NO_KEYS, ER.OK]
    assert got["out"] == b"\x81\x03srv"


def test_server_send_flag(U):
    conns = [[ER.binary(b"bin"), ER.text(b""), ER.binary(b"l", 0), ER.cont(b"ate"), ER.binary(b"")]]
    got = _check(U, conns, flags=ER.SERVER_SEND)
    assert got["out"] == b"\x81\x03bin\x81\x04late"
    assert _check(U, conns)["conn"][0]["n_echoes"] == 4


def test_carried_in_and_completed(U):
    conns = [[ER.cont(b" world")], [ER.ping(b""), ER.cont(b"", 0), ER.cont(b"!"), ER.text(b"next")],
             [ER.text(b"none")]]
    pending = [(1, b"hello"), (2, _payload(200)), None]
    got = _check(U, conns, pending=pending)
    assert got["out"][:13] == b"\x81\x0bhello world"
    assert got["out"][13:17] == b"\x82\x7e\x00\xc9" and got["out"][17:217] == _payload(200)
    assert got["open"] == b""


def test_carried_in_and_still_open(U):
    conns = [[ER.cont(b"more", 0), ER.ping(b"x")], [], [ER.ping(b"only")], [ER.cont(b"fin"), ER.text(b"again", 0)]]
    pending = [(1, b"so far "), (2, b"idle"), (1, b"kept"), (2, b"x")]
    got = _check(U, conns, pending=pending)
    assert got["open"] == b"so far more" + b"idle" + b"kept" + b"again"
    assert got["open_off"] == [0, 11, 15, 19, 24]
    assert [c["open_opcode"] for c in got["conn"]] == [1, 2, 1, 1]
    assert got["out"] == b"\x82\x04xfin"


def test_carry_missing(U):
    conns = [[ER.cont(b" world")], [ER.text(b"fine")]]
    pending = [(1, b"hello"), None]
    got = _check(U, conns, pending=pending, silent={0: ER.NO_CARRY}, carries=[b"hell", b""])
    assert got["conn"][0] == dict(ER.ZERO, status=ER.NO_CARRY) and got["out"] == b"\x81\x04fine"


def test_bad_payload_range(U):
    conns = [[ER.text(b"abc"), ER.binary(b"defgh")]]
    w, desc, first, nd, _ = _decode(conns)
    out, off, opn, r = U.echo_messages(w, desc, 0, 2, wire_len=w.size - 1)
    assert out == b"" and opn == b"" and r == dict(ER.ZERO, status=ER.BAD_RANGE) and set(off) == {0}


def test_capacity_one_short_then_the_reported_sizes(U):
    conns = [[ER.text(b"abc"), ER.binary(_payload(130), 0), ER.cont(b"z"), ER.text(b"still", 0), ER.cont(b" open", 0)]]
    w, desc, first, nd, _ = _decode(conns)
    full, off, opn, res = U.echo_messages(w, desc, 0, nd[0])
    assert res == dict(ER.ZERO, n_echoes=2, out_len=5 + 4 + 131, open_len=10, open_opcode=1) and opn == b"still open"
    for kw in ({"max_echoes": 1}, {"out_cap": len(full) - 1}, {"open_cap": 9}):
        out, o, op_, r = U.echo_messages(w, desc, 0, nd[0], **kw)
        assert out == b"" and op_ == b"" and set(o) == {0}
        assert r == dict(res, status=ER.ERR_CAPACITY, open_opcode=0)
    # without an open buffer open_cap is not tested
    assert U.echo_messages(w, desc, 0, nd[0], open_cap=0, want_open=False)[3] == res
    out, o, op_, r = U.echo_messages(w, desc, 0, nd[0], max_echoes=4, out_cap=len(full), open_cap=10)
    assert out == full and op_ == opn and r == res and o == off[:2] + [len(full)] * 3


def test_arguments(U):
    import ctypes as C
    L = U.lib()
    off = (C.c_uint64 * 2)()
    r = U.EchoConn()
    a = [None, 0, None, 0, 0, 1, 1, None, 0, 0, 0, None, 0, None, 0, off, 1, None, 0, C.byref(r)]
    assert L.uvhttp_ws_echo_messages(*a) == 0 and r.n_echoes == 0 and list(off) == [0, 0]
    for k, v in ((4, 1), (15, None), (19, None), (1, 9), (14, 9), (12, 3)):
        b = list(a)
        b[k] = v
        assert L.uvhttp_ws_echo_messages(*b) == -1, k


@pytest.mark.parametrize("seed", range(40))
def test_seeded_mix(U, seed):
    """random connections: messages cut into 1-5 fragments with PINGs between, sometimes a CLOSE
    or a failing frame part-way, a carried-in message, servers and clients, both flags"""
    rng = random.Random(9100 + seed)
    conns, srv, pending = [], [], []
    for _ in range(rng.randint(1, 8)):
        rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 5, 125, 126, 300, 2000])))
                for _ in range(rng.randint(0, 6))]
        fr = ER.FR.fragment_randomly(rng, rows)
        pend = None
        if rng.random() < 0.4:
            pend = (rng.choice([1, 2]), rng.randbytes(rng.choice([1, 3, 16, 200])))
            pre = [ER.cont(rng.randbytes(rng.choice([0, 2, 40])), 0) for _ in range(rng.randint(0, 2))]
            # the carried message completes and others follow, or it stays open
            fr = pre + [ER.cont(rng.randbytes(rng.choice([0, 7])))] + fr if rng.random() < 0.7 else pre
        if rng.random() < 0.3 and fr:
            fr.insert(rng.randrange(len(fr) + 1), ER.close(b"\x03\xe8"))
        if rng.random() < 0.2 and fr:
            fr.insert(rng.randrange(len(fr) + 1), ER.Fr(2, 1, b"bad", rsv=True))
        if rng.random() < 0.3:
            fr = fr[:max(0, len(fr) - 1)]  # may leave a message open
        conns.append(fr)
        srv.append(rng.choice([1, 1, 0]))
        pending.append(pend)
    keys = ER.keys_for(rng, 200) if rng.random() < 0.8 else None
    enable = [rng.choice([1, 1, 1, 0]) for _ in conns] if rng.random() < 0.5 else None
    _check(U, conns, srv, enable, keys, rng.choice([0, ER.SERVER_SEND]), pending)
