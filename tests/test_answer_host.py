"""uvhttp_ws_answer_messages (the host twin of the device's answers: echoes and control replies
as one run in frame order) against the transcript of the product's process_data with the
on_message hook and the control sink recording into one list (tests/_answer_ref.py): PINGs before,
between and after messages, between the fragments of a message and of a carried-in one, CLOSE
payloads of 0, 1, 2 and 125 bytes, frames after the CLOSE with and without REPLY_AFTER_CLOSE,
SERVER_SEND, clients with and without keys, NO_CARRY, BAD_RANGE from a data frame and from a PING,
the header steps, the capacity failures, a decode failure mid-stream and a seeded mix."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

import _answer_ref as AR
import _echo_ref as ER
import _replies_ref as RR

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def U():
    import uvhttp_amd as U
    return U


def _decode(conns, is_server=None, pending=None):
    wire, st = AR.streams_of(conns, is_server, pending)
    return ER.FR.oracle_decode(wire, st)


def _check(U, conns, is_server=None, enable=None, keys=None, flags=0, pending=None, delivered=None,
           silent=(), carries=None):
    """host twin == transcript for every connection of `conns`"""
    w, desc, first, nd, out = _decode(conns, is_server, pending)
    if delivered is not None:
        assert nd == delivered
    want = AR.expected_batch(conns, is_server, enable, keys, flags, None, pending, silent)
    got = AR.host_batch(U, w, desc, first, nd, is_server, enable, keys, flags, pending, carries)
    assert got == want
    for s, c in enumerate(got["conn"]):  # the open message is the decoder's pending message
        if c["status"] == AR.OK and (enable is None or enable[s]):
            assert c["open_len"] == int(out["frag_size"][s])
    return got


def _payload(n, salt=0):
    return bytes((salt + 31 * i + (i >> 8)) & 0xFF for i in range(n))


def test_pings_before_between_and_after_messages(U):
    conns = [[AR.ping(b"first"), AR.text(b"one"), AR.ping(b""), AR.binary(b"two"), AR.ping(b"last")]]
    got = _check(U, conns, delivered=[5])
    assert got["out"] == b"\x8a\x05first" b"\x81\x03one" b"\x8a\x00" b"\x82\x03two" b"\x8a\x04last"
    assert got["conn"][0] == dict(AR.ZERO, n_answers=5, n_replies=3, out_len=len(got["out"]))
    assert got["reply"][0] == dict(AR.RZERO, n_replies=3, out_len=7 + 2 + 6)


def test_ping_between_fragments_precedes_the_echo(U):
    conns = [[AR.text(b"frag", 0), AR.ping(b"mid"), AR.cont(b"ment", 0), AR.ping(b"dle"), AR.cont(b"s")]]
    got = _check(U, conns)
    assert got["out"] == b"\x8a\x03mid" b"\x8a\x03dle" b"\x81\x09fragments"


def test_ping_between_a_carried_messages_continuations(U):
    conns = [[AR.cont(b" wor", 0), AR.ping(b"p"), AR.cont(b"ld"), AR.ping(b"q")],
             [AR.ping(b"only")], [AR.ping(b"x"), AR.cont(b"more", 0)]]
    pending = [(1, b"hello"), (2, b"kept"), (1, b"so far ")]
    got = _check(U, conns, pending=pending)
    assert got["out"] == b"\x8a\x01p" b"\x81\x0bhello world" b"\x8a\x01q" b"\x8a\x04only" b"\x8a\x01x"
    assert got["open"] == b"kept" + b"so far more" and got["open_off"] == [0, 0, 4, 15]


@pytest.mark.parametrize("n", [0, 1, 2, 125])
def test_close_payloads(U, n):
    p = (b"\x03\xe8" + _payload(123))[:n]
    got = _check(U, [[AR.text(b"bye"), AR.close(p)]], delivered=[2])
    echo = b"" if n < 2 else p
    assert got["out"] == b"\x81\x03bye" + bytes([0x88, len(echo)]) + echo
    assert got["conn"][0]["closed"] == 1 and got["reply"][0]["closed"] == 1


@pytest.mark.parametrize("flags", [0, AR.REPLY_AFTER_CLOSE])
def test_frames_after_the_close(U, flags):
    conns = [[AR.text(b"open", 0), AR.close(b"\x03\xe8"), AR.ping(b"late"), AR.cont(b"ed"), AR.text(b"after"),
              AR.close(b"\x03\xe9again")]]
    got = _check(U, conns, flags=flags, delivered=[6])
    first = b"\x88\x02\x03\xe8"
    assert got["out"] == (first + b"\x8a\x04late" b"\x88\x07\x03\xe9again" if flags else first)
    assert got["conn"][0]["n_answers"] == got["conn"][0]["n_replies"] == (3 if flags else 1)


def test_server_send_with_an_empty_message_next_to_a_ping(U):
    conns = [[AR.binary(b"bin"), AR.text(b""), AR.ping(b"p"), AR.binary(b""), AR.binary(b"l", 0), AR.cont(b"ate")]]
    got = _check(U, conns, flags=AR.SERVER_SEND)
    assert got["out"] == b"\x81\x03bin" b"\x8a\x01p" b"\x81\x04late"
    assert _check(U, conns)["conn"][0]["n_answers"] == 5


def test_client_connections_mask_by_answer_slot(U):
    rng = random.Random(12)
    conns = [[AR.text(b"abcde"), AR.ping(b"pingpong"), AR.binary(b"fr", 0), AR.cont(b"agment")],
             [AR.ping(b""), AR.text(_payload(300)), AR.close(b"\x03\xe8bye")]]
    keys = AR.keys_for(rng, 16)
    got = _check(U, conns, is_server=[0, 0], keys=keys)
    k0, k1 = AR.key_bytes(keys[0]), AR.key_bytes(keys[1])
    assert got["out"][:6] == b"\x81\x85" + k0
    assert got["out"][11:17] == b"\x8a\x88" + k1
    assert got["out"][17:25] == bytes(a ^ b for a, b in zip(b"pingpong", k1 * 2))
    assert got["conn"][1]["first_answer"] == 3 and got["reply"][1]["out_len"] == 6 + 6 + 5
    # no key table: a client connection gets nothing and says why; a server one needs none
    got = _check(U, conns + [[AR.ping(b"srv")]], is_server=[0, 0, 1], keys=None)
    assert [c["status"] for c in got["conn"]] == [AR.NO_KEYS, AR.NO_KEYS, AR.OK]
    assert [q["status"] for q in got["reply"]] == [3, 3, 0] and got["conn"][1]["closed"] == 1
    assert got["out"] == b"\x8a\x03srv"


def test_enable_zero(U):
    conns = [[AR.ping(b"a")], [AR.text(b"quiet"), AR.ping(b"z"), AR.close(b"")], [AR.binary(b"b")]]
    got = _check(U, conns, enable=[1, 0, 1])
    assert got["conn"][1] == dict(AR.ZERO, first_answer=1, closed=1)
    assert got["out"] == b"\x8a\x01a\x82\x01b"


def test_carry_missing(U):
    conns = [[AR.cont(b" world"), AR.ping(b"unanswered"), AR.close(b"")], [AR.ping(b"fine")]]
    pending = [(1, b"hello"), None]
    got = _check(U, conns, pending=pending, silent={0: AR.NO_CARRY}, carries=[b"hell", b""])
    assert got["conn"][0] == dict(AR.ZERO, status=AR.NO_CARRY, closed=1)
    assert got["reply"][0] == dict(AR.RZERO, closed=1) and got["out"] == b"\x8a\x04fine"


@pytest.mark.parametrize("bad", ["data", "ping"])
def test_bad_payload_range(U, bad):
    last = AR.binary(b"defgh") if bad == "data" else AR.ping(b"defgh")
    conns = [[AR.ping(b"p"), AR.text(b"abc"), AR.close(b""), last]]
    w, desc, first, nd, _ = _decode(conns)
    assert nd == [4]
    out, off, opn, r, q = U.answer_messages(w, desc, 0, 4, wire_len=w.size - 1)
    assert out == b"" and opn == b"" and set(off) == {0}
    assert r == dict(AR.ZERO, status=AR.BAD_RANGE, closed=1) and q == dict(AR.RZERO, status=2, closed=1)


@pytest.mark.parametrize("n", [0, 125, 126, 65535, 65536])
def test_message_lengths_at_the_header_steps(U, n):
    p = _payload(n, 7)
    cut = (n + 1) // 2  # (an empty first fragment opens nothing: the empty message is one frame)
    msg = [AR.ping(b"b"), AR.binary(p)] if n == 0 else [AR.binary(p[:cut], 0), AR.ping(b"b"), AR.cont(p[cut:])]
    got = _check(U, [[AR.ping(b"a")] + msg + [AR.ping(b"c")]])
    hdr = 2 if n <= 125 else 4 if n <= 65535 else 10
    assert got["out"][:6] == b"\x8a\x01a\x8a\x01b" and got["out"][6] == 0x82
    assert got["out"][6 + hdr:6 + hdr + n] == p and got["out"][-3:] == b"\x8a\x01c"


def test_capacity_one_short_then_the_reported_sizes(U):
    conns = [[AR.text(b"abc"), AR.ping(b"pp"), AR.binary(_payload(130), 0), AR.cont(b"z"), AR.text(b"still", 0),
              AR.ping(b""), AR.cont(b" open", 0)]]
    w, desc, first, nd, _ = _decode(conns)
    full, off, opn, res, rep = U.answer_messages(w, desc, 0, nd[0])
    assert res == dict(AR.ZERO, n_answers=4, n_replies=2, out_len=5 + 4 + 4 + 131 + 2, open_len=10, open_opcode=1)
    assert opn == b"still open" and rep == dict(AR.RZERO, n_replies=2, out_len=6)
    for kw in ({"max_answers": 3}, {"out_cap": len(full) - 1}, {"open_cap": 9}):
        out, o, op_, r, q = U.answer_messages(w, desc, 0, nd[0], **kw)
        assert out == b"" and op_ == b"" and set(o) == {0}
        assert r == dict(res, status=AR.ERR_CAPACITY, open_opcode=0) and q == dict(AR.RZERO, status=1)
    # without an open buffer open_cap is not tested
    assert U.answer_messages(w, desc, 0, nd[0], open_cap=0, want_open=False)[3] == res
    out, o, op_, r, q = U.answer_messages(w, desc, 0, nd[0], max_answers=res["n_answers"] + 2,
                                          out_cap=res["out_len"], open_cap=res["open_len"])
    assert out == full and op_ == opn and r == res and q == rep and o == off[:4] + [len(full)] * 3


def test_decode_failure_mid_stream(U):
    frames = [AR.ping(b"1"), AR.text(b"ok"), AR.binary(b"part", 0), AR.ping(b"2"), AR.Fr(0, 1, b"bad", rsv=True),
              AR.ping(b"never"), AR.text(b"never")]
    got = _check(U, [frames], delivered=[4])
    assert got["out"] == b"\x8a\x011\x81\x02ok\x8a\x012" and got["open"] == b"part"


def test_transcript_is_the_merge_of_the_two_references():
    """the cross-check: the transcript's echoes are _echo_ref's calls and its replies are
    _replies_ref's sink calls, each in its own order"""
    rng = random.Random(5)
    rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 3, 200]))) for _ in range(6)]
    fr = ER.FR.fragment_randomly(rng, rows, p_ping=0.8)
    fr.insert(len(fr) - 3, AR.close(b"\x03\xe8"))
    for flags in (0, AR.REPLY_AFTER_CLOSE):
        events, still, closed = AR.transcript([AR.raw(fr)], 1, flags)
        assert [e for e in events if e[0] < 8] == ER.on_messages([AR.raw(fr)])[0]
        assert [e for e in events if e[0] >= 8] == RR.sink_calls([AR.raw(fr)], 1, 1, 1 if flags else 0)[0]
        assert closed and any(a[0] >= 8 and b[0] < 8 for a, b in zip(events, events[1:]))


def test_arguments(U):
    L = U.lib()
    off = (C.c_uint64 * 2)()
    r, q = U.AnswerConn(), U.ReplyConn()
    a = [None, 0, None, 0, 0, 1, 1, None, 0, 0, 0, None, 0, None, 0, off, 1, None, 0, C.byref(r), C.byref(q)]
    assert L.uvhttp_ws_answer_messages(*a) == 0 and r.n_answers == 0 and list(off) == [0, 0]
    a[20] = None  # the reply table is optional
    assert L.uvhttp_ws_answer_messages(*a) == 0
    for k, v in ((4, 1), (15, None), (19, None), (1, 9), (14, 9), (12, 3), (8, 4), (8, 0x80000000)):
        b = list(a)
        b[k] = v
        assert L.uvhttp_ws_answer_messages(*b) == -1, k


def test_sanitized_program_runs_clean():
    """tests/c/answer_check.c: the twin over a few of these cases, built with ASan / UBSan as a
    program of its own (by the Makefile's rule for the three *_check programs, as the close and
    fail tests get theirs: nothing to do after a full build)"""
    exe = ROOT / "tests" / "c" / "_build" / "answer_check"
    subprocess.run(["make", "-C", str(ROOT), "tests/c/_build/answer_check"], check=True, stdout=subprocess.DEVNULL)
    assert exe.exists()
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "answer_check: ok" in p.stdout


@pytest.mark.parametrize("seed", range(40))
def test_seeded_mix(U, seed):
    """random connections: messages cut into 1-5 fragments with PINGs between, PINGs and PONGs
    around them, sometimes one or two CLOSEs or a failing frame part-way, a carried-in message,
    servers and clients, every flag combination"""
    rng = random.Random(9300 + seed)
    conns, srv, pending = [], [], []
    for _ in range(rng.randint(1, 8)):
        rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 5, 125, 126, 300, 2000])))
                for _ in range(rng.randint(0, 6))]
        fr = ER.FR.fragment_randomly(rng, rows, p_ping=0.5)
        pend = None
        if rng.random() < 0.4:
            pend = (rng.choice([1, 2]), rng.randbytes(rng.choice([1, 3, 16, 200])))
            pre = [AR.cont(rng.randbytes(rng.choice([0, 2, 40])), 0) for _ in range(rng.randint(0, 2))]
            fr = pre + [AR.cont(rng.randbytes(rng.choice([0, 7])))] + fr if rng.random() < 0.7 else pre
        for _ in range(rng.randint(0, 4)):
            fr.insert(rng.randrange(len(fr) + 1),
                      rng.choice([AR.ping(rng.randbytes(rng.choice([0, 1, 16, 125]))), AR.Fr(10, 1, b"pong")]))
        for _ in range(rng.choice([0, 0, 1, 2])):
            fr.insert(rng.randrange(len(fr) + 1), AR.close(rng.choice([b"", b"\x03", b"\x03\xe8", b"\x03\xe8why"])))
        if rng.random() < 0.2 and fr:
            fr.insert(rng.randrange(len(fr) + 1), AR.Fr(2, 1, b"bad", rsv=True))
        if rng.random() < 0.3:
            fr = fr[:max(0, len(fr) - 1)]  # may leave a message open
        conns.append(fr)
        srv.append(rng.choice([1, 1, 0]))
        pending.append(pend)
    keys = AR.keys_for(rng, 400) if rng.random() < 0.8 else None
    enable = [rng.choice([1, 1, 1, 0]) for _ in conns] if rng.random() < 0.5 else None
    _check(U, conns, srv, enable, keys, rng.choice([0, 1, 2, 3]), pending)
