"""uvhttp_ws_utf8_judge_frames (the host twin of the frame-level UTF-8 validation) against the
Python walk of tests/_utf8_frames_ref.py over the descriptors of the oracle's stream decode:
the known answers as one frame and cut into fragments at every byte, empty fragments and PINGs
in between, carried-in states, any stream split into two calls with the state handed over,
CLOSE reasons, bad ranges and the ABI."""
import ctypes as C
import random

import pytest

import _utf8_frames_ref as FR
import _utf8_ref as R

KNOWN = ([bytes.fromhex(h) for h in R.KNOWN_VALID] + [bytes.fromhex(h) for h in R.KNOWN_INVALID] +
         [bytes.fromhex(h) for h, _ in R.KNOWN_TRUNCATED])


@pytest.fixture(scope="module")
def U():
    import uvhttp_amd as U
    return U


def _state(U, pend):
    st = U.Utf8State()
    st.n = len(pend)
    for k, b in enumerate(pend):
        st.pend[k] = b
    return st


class Decoded:
    """connections' frames decoded by the oracle, as ctypes buffers for the host twin"""

    def __init__(self, conns, pending=None):
        self.conns = conns
        wire, st = FR.streams_of(conns, pending)
        self.wire, self.desc, self.first, self.nd, _ = FR.oracle_decode(wire, st)
        self.wbuf = (C.c_uint8 * max(1, self.wire.size)).from_buffer_copy(self.wire.tobytes() or b"\0")
        self.dbuf = (C.c_uint8 * max(32, self.desc.nbytes)).from_buffer_copy(self.desc.tobytes().ljust(32, b"\0"))

    def host(self, U, s, lo=0, hi=None, open_opcode=0, state=None, flags=0, wire_len=None):
        """the host twin over frames [lo, hi) of connection s"""
        hi = self.nd[s] if hi is None else hi
        out = U.Utf8ConnVerdict()
        rc = U.lib().uvhttp_ws_utf8_judge_frames(
            self.wbuf, self.wire.size if wire_len is None else wire_len, self.dbuf, self.first[s] + lo,
            hi - lo, open_opcode, C.byref(state) if state is not None else None, flags, C.byref(out))
        assert rc == 0
        return out.as_dict()


def _check_one(U, frames, all_delivered=True, **kw):
    d = Decoded([frames])
    if all_delivered:
        assert d.nd[0] == len(frames)
    got = d.host(U, 0, flags=kw.get("flags", 0))
    want = FR.judge(frames[:d.nd[0]], **kw)
    assert got == want, (got, want)
    return got


def test_known_answers_one_frame(U):
    for b in KNOWN:
        got = _check_one(U, [FR.Fr(1, 1, b)])
        assert got["status"] == (R.VALID if R.is_valid(b) else R.INVALID)
        got = _check_one(U, [FR.Fr(1, 0, b)])  # left open: a prefix
        assert got["status"] == R.prefix_verdict(b)[0]
        assert got["state"][1] == R.prefix_verdict(b)[1]
        assert _check_one(U, [FR.Fr(2, 1, b)])["status"] == R.VALID  # BINARY: anything goes


def test_cut_at_every_byte(U):
    for b in KNOWN:
        for cut in range(1, len(b) + 1):
            for fin in (1, 0):
                frames = FR.fragments(b, [cut])
                frames[-1] = FR.Fr(0, fin, frames[-1].payload)
                _check_one(U, frames)


def test_cut_at_every_pair_with_empty_fragments_and_pings(U):
    for b in KNOWN:
        for a in range(1, len(b) + 1):
            for z in range(a, len(b) + 1):
                _check_one(U, FR.fragments(b, [a, a, z, z], between=(FR.PING(),)))


def test_one_byte_fragments(U):
    for b in KNOWN + ["héllo wörld €uro 😀!".encode()]:
        if len(b) >= 2:
            _check_one(U, FR.fragments(b, list(range(1, len(b)))))


def test_euro_split_with_binary_between_text(U):
    frames = [FR.Fr(1, 0, b"\xe2\x82"), FR.Fr(0, 1, b"\xac"), FR.Fr(2, 1, b"\xff\xfe"),
              FR.Fr(1, 0, b"a\xe2"), FR.PING(), FR.Fr(0, 1, b"\x82\xac")]
    got = _check_one(U, frames)
    assert got["status"] == R.VALID and got["n_text_frames"] == 4
    # the same bytes with the BINARY message's opcode TEXT: FF is invalid at frame 2
    frames[2] = FR.Fr(1, 1, b"\xff\xfe")
    got = _check_one(U, frames)
    assert got["status"] == R.INVALID and got["first_invalid"] == 2 and got["n_text_frames"] == 5


def test_zero_length_fin_continuation_inside_a_sequence(U):
    got = _check_one(U, [FR.Fr(1, 0, b"ab\xe2"), FR.PING(), FR.Fr(0, 0, b""), FR.Fr(0, 1, b"")])
    assert got["status"] == R.INVALID and got["first_invalid"] == 3
    got = _check_one(U, [FR.Fr(1, 0, b"ab\xe2"), FR.Fr(0, 0, b"")])
    assert got["status"] == R.PREFIX and got["state"] == (b"\xe2", 1)


@pytest.mark.parametrize("pend", [b"\xc2", b"\xe2\x82", b"\xf0\x9f\x98", b""])
def test_carried_in_state(U, pend):
    for rest in (b"\x80", b"\xac", b"a", b"", b"\x80\x80\x80", b"\x80\xe2"):
        for fin in (1, 0):
            frames = [FR.Fr(0, fin, rest), FR.PING()] + ([FR.Fr(1, 1, b"ok")] if fin else [])
            d = Decoded([frames], pending=[(1, 7)])
            assert d.nd[0] == len(frames)
            got = d.host(U, 0, open_opcode=1, state=_state(U, pend))
            assert got == FR.judge(frames, open_opcode=1, pend=pend), (rest, fin)
            # the carried-in message BINARY: the state is ignored, nothing of it is text
            d = Decoded([frames], pending=[(2, 7)])
            got = d.host(U, 0, open_opcode=2, state=_state(U, pend))
            assert got == FR.judge(frames, open_opcode=2, pend=pend)
            assert got["status"] == R.VALID and got["n_text_frames"] == fin
    if pend:
        d = Decoded([[FR.Fr(0, 1, b"\x80")]], pending=[(1, 7)])
        got = d.host(U, 0, open_opcode=1, state=_state(U, pend))
        assert got["status"] == R.VALID  # C2 80, E2 82 80, F0 9F 98 80
        got = d.host(U, 0, open_opcode=1)  # the state dropped: a stray continuation byte
        assert got["status"] == R.INVALID and got["first_invalid"] == 0


def _combine(a, b):
    """what two successive calls say about the connection as a whole"""
    bad = a["status"] in (R.INVALID, R.BAD_RANGE)
    return {"first_invalid": a["first_invalid"] if bad else b["first_invalid"],
            "n_text_frames": a["n_text_frames"] + b["n_text_frames"],
            "state": (b"", 0) if bad else b["state"], "status": a["status"] if bad else b["status"]}


def _open_after(frames):
    op = 0
    for f in frames:
        if f.op in (1, 2):
            op = f.op
        if f.op < 8 and f.fin:
            op = 0
    return op


@pytest.mark.parametrize("seed", range(4))
def test_any_split_into_two_calls(U, seed):
    """every connection (two fuzz messages, fragmented, PINGs sprinkled in) judged in one call
    and, for every frame k, as frames [0, k) then [k, n) with the state handed over"""
    rng = random.Random(seed)
    rows = R.fuzz_messages(seed)
    conns = [FR.fragment_randomly(rng, rows[k:k + 2]) for k in range(0, len(rows), 2)]
    d = Decoded(conns)
    n_split = n_prefix = 0
    for s, frames in enumerate(conns):
        assert d.nd[s] == len(frames)
        whole = d.host(U, s)
        assert whole == FR.judge(frames, first_frame=d.first[s]), s
        for k in range(len(frames) + 1):
            a = d.host(U, s, 0, k)
            st = _state(U, a["state"][0])
            b = d.host(U, s, k, None, open_opcode=_open_after(frames[:k]), state=st)
            assert _combine(a, b) == whole, (s, k, a, b, whole)
            n_split += 1
            n_prefix += a["status"] == R.PREFIX and a["state"][1] > 0
    assert n_split > 5000 and n_prefix > 50


def _close(reason):
    return FR.Fr(8, 1, (1000).to_bytes(2, "big") + reason)


@pytest.mark.parametrize("reason,bad", [(b"bye \xe2\x82\xac", False), (b"\xc0\x80", True), (b"bye \xe2\x82", True),
                                         (b"", False)])
def test_close_reasons(U, reason, bad):
    frames = [FR.Fr(1, 1, b"hi"), FR.PING(), _close(reason)]
    got = _check_one(U, frames, flags=FR.CHECK_CLOSE)
    assert got["status"] == (R.INVALID if bad else R.VALID)
    assert got["first_invalid"] == (2 if bad else FR.NONE)
    got = _check_one(U, frames)  # without the flag CLOSE frames are ignored
    assert got["status"] == R.VALID and got["first_invalid"] == FR.NONE


def test_bad_range(U):
    frames = [FR.Fr(1, 1, b"one"), FR.Fr(2, 1, b"\xff" * 40), FR.Fr(1, 0, b"two \xe2"), FR.Fr(0, 1, b"\x82\xac")]
    d = Decoded([frames])
    assert d.host(U, 0)["status"] == R.VALID
    # the wire cut inside frame 3's payload, inside frame 2's, and inside the BINARY frame's
    end3 = int(d.desc["payload_off"][3] + d.desc["payload_len"][3])
    for wire_len, bad in ((end3 - 1, {3}), (int(d.desc["payload_off"][2]) + 1, {2, 3}),
                          (int(d.desc["payload_off"][1]) + 5, {2, 3})):
        got = d.host(U, 0, wire_len=wire_len)
        assert got == FR.judge(frames, bad_range=bad)
        assert got["status"] == R.BAD_RANGE and got["first_invalid"] == min(bad)
    # an INVALID frame before the bad range wins
    frames[0] = FR.Fr(1, 1, b"\x80ne")
    d = Decoded([frames])
    got = d.host(U, 0, wire_len=end3 - 1)
    assert got == FR.judge(frames, bad_range={3}) and got["status"] == R.INVALID and got["first_invalid"] == 0


def test_failing_connection_judges_only_the_delivered_frames(U):
    frames = [FR.Fr(1, 0, b"ok \xf0\x9f"), FR.Fr(0, 0, b"\x98", rsv=True), FR.Fr(0, 1, b"\xff\xff")]
    d = Decoded([frames])
    assert d.nd[0] == 1
    got = d.host(U, 0)
    assert got == FR.judge(frames[:1]) and got["status"] == R.PREFIX and got["state"] == (b"\xf0\x9f", 2)


def test_abi(U):
    assert C.sizeof(U.Utf8ConnVerdict) == 16 and C.sizeof(U.Utf8FramesSummary) == 16
    assert U.Utf8ConnVerdict.state.offset == 8 and U.Utf8ConnVerdict.status.offset == 12
    assert U.UTF8_CHECK_CLOSE == 1
    out = U.Utf8ConnVerdict()
    assert U.lib().uvhttp_ws_utf8_judge_frames(None, 0, None, 0, 0, 0, None, 0, C.byref(out)) == 0
    assert out.as_dict() == {"first_invalid": FR.NONE, "n_text_frames": 0, "state": (b"", 0), "status": R.VALID}
    assert U.lib().uvhttp_ws_utf8_judge_frames(None, 0, None, 0, 1, 0, None, 0, C.byref(out)) == -1
    assert U.lib().uvhttp_ws_utf8_judge_frames(None, 0, None, 0, 0, 0, None, 0, None) == -1
    # the module-level wrapper
    d = Decoded([[FR.Fr(1, 0, b"\xe2\x82")]])
    assert U.utf8_judge_frames(d.wire, d.desc, 0, 1) == FR.judge(d.conns[0])
