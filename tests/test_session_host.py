"""Whole server sessions over many calls on the host (tests/_session_ref.py): the per-call loop of
INTEGRATION.md with every pass on — TLS open, stream decode, UTF-8 verdicts, control replies,
echoes, seal, uvhttp_ws_deliver_stream — through the oracle's decoders, the host twins
uvhttp_ws_utf8_judge_frames / uvhttp_ws_control_replies / uvhttp_ws_echo_messages and the seal
reference, with all six pieces of carried state handed from call to call.  Pins the session model
itself, and the cut invariance of the host twins and of deliver_stream: after every call the
decoder's pending_bytes, the echo's open_len / open_opcode / open bytes, the verdict's state and
the product connection's fragment state and recv buffer agree; at the end every connection's
events, return code, calls, buffers, echo frames, reply frames, first invalid frame and sealed
record stream are those of the references fed the same reads in one go.  The same sessions run
on the device in test_gpu_sessions.py; the conditions that prove they reach the hard cases are
asserted in both files."""
import functools

import pytest

import _session_ref as SR

SEEDS = range(4)


def _run(conns, scheds, **kw):
    lives, log = SR.run_session(SR.HostBackend(), conns, scheds, **kw)
    return lives, log, SR.check_session(conns, scheds, lives)


@functools.lru_cache(maxsize=None)
def _expects(seed, transport):
    conns, scheds = SR.random_session(seed, transport)
    return conns, scheds, [SR.expect(c, cuts) for c, cuts in zip(conns, scheds)]


def check_every_cut_conditions(conns, scheds, log):
    """one connection per byte offset, none skipped; the two calls' frames sum to the one-shot's"""
    n = len(conns[0].wire)
    assert [s[0] for s in scheds] == list(range(1, n)) and len(log) == 2
    total = len(conns[0].frames)
    for s in range(len(conns)):
        assert log[0][1]["results"][s].n_delivered + log[1][1]["results"][s].n_delivered == total, s


def check_random_conditions(transport):
    """the conditions of the random sessions, from the scripts and the references only"""
    counts = {}
    for seed in SEEDS:
        conns, scheds, expects = _expects(seed, transport)
        lived = [e.n_calls if e.leave_call is None else e.leave_call + 1 for e in expects]
        last = [e.leave_call is None or e.leave_call == e.n_calls - 1 for e in expects]
        assert len(conns) == 32 and 3 <= max(c.join + e.n_calls for c, e in zip(conns, expects)) <= 6
        assert 4 * sum(n >= 2 for n in lived) >= 3 * len(conns), (seed, lived)
        assert 2 * sum(last) >= len(conns), (seed, last)
        assert any(c.join for c in conns) and not all(last)          # late joiners, early leavers
        assert any(len(f.payload) > 65536 for c in conns for f in c.frames)
        assert transport == "tls" or {c.is_server for c in conns} == {0, 1}
        for k, v in SR.coverage(conns, scheds, expects).items():
            counts[k] = counts.get(k, 0) + v
    kinds = SR.KINDS_WS + (SR.KINDS_TLS if transport == "tls" else ())
    assert all(counts.get(k, 0) >= 1 for k in kinds), counts
    assert counts["msg_open"] >= 10 and counts["utf8_char"] >= 5 and counts["invalid_straddle"] >= 3, counts
    return counts


@pytest.mark.parametrize("transport", ["plain", "tls"])
def test_every_cut_two_calls(transport):
    conns, scheds = SR.every_cut_session(transport)
    lives, log, expects = _run(conns, scheds)
    check_every_cut_conditions(conns, scheds, log)
    assert all(e.why == "closed" and e.leave_call == 1 for e in expects)
    kinds = set().union(*(SR.classify(c, s[0]) for c, s in zip(conns, scheds)))
    want = {"ws_hdr2", "ws_hdr4", "ws_key", "ws_payload", "frame_edge", "utf8_char", "msg_open", "ctrl_after_open"}
    assert want | (set(SR.KINDS_TLS) if transport == "tls" else set()) <= kinds, kinds


@pytest.mark.parametrize("transport", ["plain", "tls"])
def test_random_session_conditions(transport):
    print(transport, sorted(check_random_conditions(transport).items()))


@pytest.mark.parametrize("transport", ["plain", "tls"])
@pytest.mark.parametrize("seed", SEEDS)
def test_random_sessions(seed, transport):
    conns, scheds, expects = _expects(seed, transport)
    lives, _ = SR.run_session(SR.HostBackend(), conns, scheds)
    SR.check_session(conns, scheds, lives, expects=expects)


def test_long_open_message_many_calls():
    conns, scheds = SR.long_open_session()
    lives, log, expects = _run(conns, scheds)
    SR.check_long_open_conditions(conns, scheds, log, expects)


def test_shapes_shrink_and_grow():
    conns, scheds = SR.shapes_session()
    lives, log, _ = _run(conns, scheds)
    assert [x["S"] for x, _ in log] == [300, 3, 600, 1]


@pytest.mark.parametrize("mistake", [
    "zero_state_in",     # the verdict history misses the sequence that straddles two calls
    "drop_carry",        # the echo pass refuses a connection whose carry is missing
    "reuse_write_seq"])  # the sealed record stream repeats a sequence number
def test_a_broken_driver_is_caught(mistake):
    """the checks are not vacuous: each deliberate mistake of the per-call loop fails them"""
    conns, scheds, expects = _expects(0, "tls")
    with pytest.raises(AssertionError):
        lives, _ = SR.run_session(SR.HostBackend(), conns, scheds, break_driver=mistake)
        SR.check_session(conns, scheds, lives, expects=expects)


def test_the_call_comparison_sees_every_output():
    """assert_same_call, which test_gpu_sessions.py puts between the device and the host after every
    call, fails for one changed byte or field in each kind of output"""
    import copy
    conns, scheds, _ = _expects(1, "plain")
    _, log = SR.run_session(SR.HostBackend(), conns, scheds)
    x, o = next((x, o) for x, o in log[1:] if o["echo"]["summary"]["open_bytes"] and o["reply"]["summary"]["n_replies"])
    SR.assert_same_call(o, copy.deepcopy(o), x, "same")

    def flip(b, at=0):
        return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]

    s = next(s for s, r in enumerate(o["results"]) if r.n_delivered and o["desc"][r.first_frame]["payload_len"])
    at = int(o["desc"][o["results"][s].first_frame]["payload_off"])  # a delivered payload byte
    changes = {
        "wire": lambda c: c["wire"].__setitem__(at, 0x5A ^ c["wire"][at]),
        "result": lambda c: setattr(c["results"][s], "pending_bytes", c["results"][s].pending_bytes + 1),
        "desc": lambda c: c["desc"]["flags"].__setitem__(c["results"][s].first_frame, 0x3F),
        "stream": lambda c: setattr(c["streams"][s], "pending_opcode", 7),
        "verdict": lambda c: c["verdicts"][s].__setitem__("n_text_frames", 99),
        "utf8 summary": lambda c: c["usum"].__setitem__("n_open_conns", 99),
        "echo out": lambda c: c["echo"].__setitem__("out", flip(c["echo"]["out"])),
        "echo out_off": lambda c: c["echo"]["out_off"].__setitem__(1, c["echo"]["out_off"][1] + 1),
        "echo open": lambda c: c["echo"].__setitem__("open", flip(c["echo"]["open"], len(c["echo"]["open"]) - 1)),
        "echo open_off": lambda c: c["echo"]["open_off"].__setitem__(-1, 0),
        "echo conn": lambda c: c["echo"]["conn"][s].__setitem__("open_opcode", 9),
        "reply out": lambda c: c["reply"].__setitem__("out", flip(c["reply"]["out"])),
        "reply conn": lambda c: c["reply"]["conn"][s].__setitem__("closed", 1 - c["reply"]["conn"][s]["closed"]),
        "reply summary": lambda c: c["reply"]["summary"].__setitem__("n_replies", 0),
    }
    for name, change in changes.items():
        c = copy.deepcopy(o)
        change(c)
        with pytest.raises(AssertionError):
            SR.assert_same_call(c, o, x, name)
            pytest.fail("unseen: " + name, pytrace=False)
