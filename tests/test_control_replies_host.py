"""uvhttp_ws_control_replies (the host twin of the device control replies) against the frames
the existing host path hands the control sink (tests/_replies_ref.py): PING and CLOSE lengths at
the edges, PONG and data frames in between, frames after a CLOSE under both flags, a connection
that fails part-way, enable = 0, a client connection with keys by reply slot, the capacity
failure, a bad payload range, the reference's known answers and the ABI."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import _replies_ref as RR

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_known_answers.json")


@pytest.fixture(scope="module")
def U():
    import uvhttp_amd as U
    return U


def _decode(conns, is_server=None):
    wire, st = RR.streams_of(conns, is_server)
    w, desc, first, nd, _ = RR.FR.oracle_decode(wire, st)
    return w, desc, first, nd


def _check(U, conns, is_server=None, enable=None, keys=None, flags=0, delivered=None):
    """host twin == sink reference for every connection of `conns`"""
    w, desc, first, nd = _decode(conns, is_server)
    if delivered is not None:
        assert nd == delivered
    want = RR.expected_batch(conns, is_server, enable, keys, flags)
    got = RR.host_batch(U, w, desc, first, nd, is_server, enable, keys, flags)
    assert got == want
    return got


MIX = [RR.data(b"hello", 1), RR.ping(b""), RR.pong(b"xyz"), RR.ping(b"a"), RR.data(b"", 2),
       RR.ping(bytes(range(124))), RR.data(b"frag", 1, 0), RR.ping(bytes(range(125))), RR.data(b"ment", 0, 1),
       RR.pong(b""), RR.data(b"z" * 300)]


def test_ping_lengths_between_data_and_pongs(U):
    got = _check(U, [MIX], delivered=[len(MIX)])
    assert got["summary"]["n_replies"] == 4 and got["conn"][0]["closed"] == 0
    assert got["out"][:2] == b"\x8a\x00" and got["out"][2:5] == b"\x8a\x01a"


@pytest.mark.parametrize("n", [0, 1, 2, 3, 125])
def test_close_lengths(U, n):
    payload = (b"\x03\xe8" + b"r" * 123)[:n]
    got = _check(U, [[RR.data(b"x"), RR.close(payload), RR.data(b"y")]])
    want = b"\x88" + (bytes([n]) + payload if n >= 2 else b"\x00")
    assert got["out"] == want and got["conn"][0] == {
        "first_reply": 0, "n_replies": 1, "out_len": len(want), "status": RR.OK, "closed": 1}


@pytest.mark.parametrize("flags", [0, RR.AFTER_CLOSE])
def test_after_close(U, flags):
    frames = [RR.ping(b"1"), RR.close(b"\x03\xe9bye"), RR.ping(b"2"), RR.data(b"d"), RR.ping(b""),
              RR.close(b"\x03\xea"), RR.ping(b"3")]
    got = _check(U, [frames], flags=flags, delivered=[len(frames)])
    assert got["conn"][0]["n_replies"] == (6 if flags else 2)


def test_failure_at_frame_k(U):
    frames = [RR.ping(b"before"), RR.data(b"ok"), RR.Fr(2, 1, b"bad", rsv=True), RR.ping(b"after"), RR.close(b"")]
    got = _check(U, [frames], delivered=[2])
    assert got["out"] == b"\x8a\x06before"


def test_enable_zero_and_mixed_connections(U):
    conns = [MIX, [RR.ping(b"quiet"), RR.close(b"\x03\xe8")], [], [RR.close(b"")], [RR.data(b"only data")]]
    got = _check(U, conns, enable=[1, 0, 1, 1, 1])
    assert got["conn"][1] == {"first_reply": 4, "n_replies": 0, "out_len": 0, "status": RR.OK, "closed": 1}
    assert got["conn"][3]["first_reply"] == 4 and got["conn"][4]["first_reply"] == 5


def test_client_connection_masks_by_reply_slot(U):
    rng = random.Random(7)
    conns = [[RR.ping(b"abcde"), RR.data(b"x"), RR.close(b"\x03\xe8done"), RR.ping(b"no")],
             [RR.ping(bytes(range(125))), RR.ping(b"")]]
    keys = RR.keys_for(rng, 8)
    got = _check(U, conns, is_server=[0, 0], keys=keys)
    k0 = RR.key_bytes(keys[0])
    assert got["out"][:6] == b"\x8a\x85" + k0
    assert got["out"][6:11] == bytes(a ^ b for a, b in zip(b"abcde", (k0 * 2)))
    assert got["conn"][1]["first_reply"] == 2
    # no key table: a client connection gets no replies and says why; a server one needs none
    got = _check(U, conns + [[RR.ping(b"srv")]], is_server=[0, 0, 1], keys=None)
    assert [c["status"] for c in got["conn"]] == [RR.NO_KEYS, RR.NO_KEYS, RR.OK]
    assert got["out"] == b"\x8a\x03srv" and got["conn"][0]["closed"] == 1


def test_capacity_failure_reports_the_totals(U):
    w, desc, first, nd = _decode([MIX])
    full, off, res = U.control_replies(w, desc, 0, nd[0])
    assert res["n_replies"] == 4 and res["out_len"] == len(full) == 4 * 2 + 0 + 1 + 124 + 125
    for kw in ({"max_replies": 3}, {"out_cap": len(full) - 1}):
        out, o, r = U.control_replies(w, desc, 0, nd[0], **kw)
        assert out == b"" and set(o) == {0}
        assert r == dict(res, status=RR.ERR_CAPACITY)
    # the reported sizes are enough, and the offsets past the replies hold the total
    out, o, r = U.control_replies(w, desc, 0, nd[0], max_replies=6, out_cap=len(full))
    assert out == full and r == res and o == off[:4] + [len(full)] * 3


def test_capacity_failure_writes_nothing(U):
    w, desc, first, nd = _decode([MIX])
    L = U.lib()
    wb = (C.c_uint8 * w.size).from_buffer_copy(w.tobytes())
    db = (C.c_uint8 * desc.nbytes).from_buffer_copy(desc.tobytes())
    out = (C.c_uint8 * 300)(*([0xEE] * 300))
    off = (C.c_uint64 * 5)()
    r = U.ReplyConn()
    assert L.uvhttp_ws_control_replies(wb, w.size, db, 0, nd[0], 1, 1, None, 0, out, 257, off, 4, C.byref(r)) == 0
    assert r.status == RR.ERR_CAPACITY and bytes(out) == b"\xee" * 300


def test_bad_payload_range(U):
    frames = [RR.ping(b"first"), RR.data(b"d"), RR.ping(b"second"), RR.close(b"")]
    w, desc, first, nd = _decode([frames])
    bad = desc.copy()
    bad["payload_off"][2] = w.size - 3  # six bytes from there leave the wire
    out, off, r = U.control_replies(w, bad, 0, nd[0])
    assert out == b"" and set(off) == {0}
    assert r == {"first_reply": 0, "n_replies": 0, "out_len": 0, "status": RR.BAD_RANGE, "closed": 1}
    # a shorter wire_len does the same to the intact table; an empty payload has no range
    assert U.control_replies(w, desc, 0, nd[0], wire_len=int(desc["payload_off"][2]) + 5)[2]["status"] == RR.BAD_RANGE
    bad = desc.copy()
    bad["payload_off"][3] = 1 << 40
    assert U.control_replies(w, bad, 0, nd[0])[2]["status"] == RR.OK
    # enable = 0 judges nothing
    bad["payload_off"][0] = 1 << 40
    assert U.control_replies(w, bad, 0, nd[0], enable=0)[2] == {
        "first_reply": 0, "n_replies": 0, "out_len": 0, "status": RR.OK, "closed": 1}


def test_reference_known_answers_echoed_masked_close(U):
    """test/unit/test_websocket_boost_coverage2.cpp:613-710: the masked CLOSE 1000 "OK" and the
    masked CLOSE 1002.  A server echoes code and reason unmasked; a client that echoes with the
    key the frame came with sends back the very bytes it received."""
    cases = {"masked_close_1000_ok": ("888437fa213d34126e76", b"\x88\x04\x03\xe8OK"),
             "masked_close_1002": ("8882aabbccdda951", b"\x88\x02\x03\xea")}
    with open(GOLDEN) as f:  # the frames fed are the golden file's
        known = {c["id"]: c for group in json.load(f).values() if isinstance(group, list)
                 for c in group if isinstance(c, dict) and "id" in c}
    for cid, (hx, _) in cases.items():
        assert known[cid]["feeds"][0]["hex"] == hx
    for hx, echo in cases.values():
        raw = bytes.fromhex(hx)
        for srv in (1, 0):
            wire = np.frombuffer(raw, np.uint8).copy()
            st = np.zeros(1, RR.O.STREAM_DT)
            st[0] = (0, len(raw), 65536, 0, 0, RR.MF, RR.MM, srv, 0, 0, 0)
            w, desc, first, nd, _ = RR.FR.oracle_decode(wire, st)
            assert nd == [1]
            key = int.from_bytes(raw[2:6], "little")
            out, _, r = U.control_replies(w, desc, 0, 1, is_server=srv, mask_keys=[key])
            assert out == (echo if srv else raw) and r["closed"] == 1
            want = RR.expected_batch([raw], [srv], None, [key])
            assert out == want["out"]


def test_seeded_mixes_against_the_sink(U):
    for seed in range(40):
        rng = random.Random(9000 + seed)
        conns, srv = [], []
        for _ in range(rng.randint(1, 6)):
            fr = RR.D.mixed(rng, rng.randint(0, 14), sizes=(0, 1, 7, 100, 300), p_ctrl=0.5, p_res=0.0,
                            bad_at=rng.choice([None, None, 3]))
            conns.append(b"".join(f.bytes for f in fr))
            srv.append(rng.choice([1, 1, 0]))
        total = sum(len(c) for c in conns)
        keys = RR.keys_for(rng, total // 6 + 1)
        flags = rng.choice([0, RR.AFTER_CLOSE])
        enable = [rng.choice([1, 1, 0]) for _ in conns]
        wire = np.frombuffer(b"".join(conns) or b"\0", np.uint8).copy()
        st = np.zeros(len(conns), RR.O.STREAM_DT)
        pos = 0
        for s, c in enumerate(conns):
            st[s] = (pos, len(c), 65536, 0, 0, RR.MF, RR.MM, srv[s], 0, 0, 0)
            pos += len(c)
        w, desc, first, nd, _ = RR.FR.oracle_decode(wire, st)
        want = RR.expected_batch(conns, srv, enable, keys, flags)
        got = RR.host_batch(U, w, desc, first, nd, srv, enable, keys, flags)
        assert got == want, seed


def test_abi_and_null_arguments(U):
    assert C.sizeof(U.ReplyConn) == 16 and C.sizeof(U.ReplySummary) == 32
    L = U.lib()
    r, off = U.ReplyConn(), (C.c_uint64 * 2)(7, 7)
    assert L.uvhttp_ws_control_replies(None, 0, None, 0, 0, 1, 1, None, 0, None, 0, off, 1, C.byref(r)) == 0
    assert list(off) == [0, 0] and r.n_replies == 0 and r.status == RR.OK
    assert L.uvhttp_ws_control_replies(None, 0, None, 0, 1, 1, 1, None, 0, None, 0, off, 1, C.byref(r)) == -1
    assert L.uvhttp_ws_control_replies(None, 0, None, 0, 0, 1, 1, None, 0, None, 0, None, 1, C.byref(r)) == -1
    assert L.uvhttp_ws_control_replies(None, 0, None, 0, 0, 1, 1, None, 0, None, 0, off, 1, None) == -1
    assert L.uvhttp_ws_control_replies(None, 0, None, 0, 0, 1, 1, None, 0, None, 9, off, 1, C.byref(r)) == -1
