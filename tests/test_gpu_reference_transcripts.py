"""The device calls against tests/golden/reference_transcripts.json: sessions the reference's own
uvhttp_ws_process_data ran (tests/golden/make_reference_transcripts.py).  Only the committed file
is read; the reference itself is not needed.

All sessions of one side are the connections of ONE device call (a few hundred connections of a
few hundred bytes, and the few with 65 535 / 65 536 / 70 000-byte payloads), each at a 16-byte
aligned start with random bytes between that no kernel may touch; descriptor and result tables
have guard entries behind them.  UTF-8 validation and fail points, which the reference does not
have, stay off.

  decode_reads with the sessions' read boundaries (and decode_streams on the one-read sessions),
    then uvhttp_ws_deliver_stream into a recording connection: the events (messages, close codes,
    and the frames sent: the control sink's and the echo hook's, under send_frame's rule), the
    return code, the calls made, the bytes left buffered, the buffer size and the open-message
    state are the reference's.  Run on the default engine (speculative stream decode on) and on
    one with it off (the walk).
  decode_inplace and decode_compact with an offset table, then uvhttp_ws_deliver_batch /
    uvhttp_ws_deliver_messages, on the server sessions cut one read per frame: there the batch
    contract (every frame is fed alone, in order, to one connection whose receive
    buffer is empty) is the session itself, because every read is one whole frame that the call
    consumes or fails on, which the committed results show (recv_buffer_pos 0 after every
    successful call).  The receive buffer's size is not compared: a batch has none.
  control_replies_streams on the sessions wired to a server context without the echo hook,
    echo_messages_streams on those with the hook and no context, answer_messages_streams on those
    with both: every connection's output is the concatenation of the frames the reference sent, in
    its order; clients take the session's keys by position."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _reference as RF
from test_gpu_echo import FAILED, FILL, _dev

pytestmark = pytest.mark.gpu

DOC, ENTRIES = RF.load_transcripts()
GAP = 16          # random bytes between connections
ERR_BUFFER = -6     # UVHTTP_WS_FRAME_ERR_BUFFER
MAX_PER_CONN = 256  # descriptors allowed for per connection (no session has 30 frames)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def engines(torch):
    """the default engine (speculative stream decode on) and one that always walks, selected as
    tests/test_gpu_stream_spec.py does"""
    import os
    import uvhttp_amd as U
    spec = U.GpuEngine(0)
    os.environ["UVHTTP_WS_STREAM_SPEC"] = "0"
    try:
        walk = U.GpuEngine(0)
    finally:
        del os.environ["UVHTTP_WS_STREAM_SPEC"]
    yield {"spec": spec, "walk": walk}
    spec.close()
    walk.close()


@pytest.fixture(scope="module")
def host_hooks():
    RF.install_host_hooks()
    yield
    RF.remove_host_hooks()


def _limits(e):
    return (RF.DEFAULT_MF if e.mfs is None else e.mfs, RF.DEFAULT_MM if e.mms is None else e.mms)


class Decoded:
    """one decode_reads / decode_streams call over `entries`, its outputs on the host, guards
    checked"""

    def __init__(self, torch, eng, entries, use_reads):
        import uvhttp_amd as U
        self.entries, S = entries, len(entries)
        rng = np.random.default_rng(0xD0C0 + S + int(use_reads))
        st = np.zeros(S, O.STREAM_DT)
        read_end, pos, spans = [], 0, []
        for s, e in enumerate(entries):
            pos = (pos + 15) & ~15
            pos += GAP
            mf, mm = _limits(e)
            nr = len(e.read_lens) if use_reads else 0
            assert use_reads or len(e.read_lens) == 1
            st[s] = (pos, len(e.wire), 65536, 0, 0, mf, mm, e.is_server, len(read_end), nr, 0)
            if use_reads:
                read_end += [int(x) for x in np.cumsum(e.read_lens)]
            spans.append((pos, len(e.wire)))
            pos += len(e.wire)
        self.wire_len = pos
        wire = rng.integers(0, 256, pos + 64, dtype=np.uint8)
        outside = np.ones(pos + 64, bool)
        for (p, n), e in zip(spans, entries):
            wire[p:p + n] = np.frombuffer(e.wire, np.uint8)
            outside[p:p + n] = False
        self.max_frames = MAX_PER_CONN * S
        self.st, self.S = st, S
        self.dw = torch.from_numpy(wire.copy()).to("cuda")
        self.dst = _dev(torch, st, 0)
        re_dev = torch.tensor(read_end or [0], dtype=torch.int64, device="cuda") if use_reads else None
        desc_t = torch.full(((self.max_frames + 2) * 32,), FILL, dtype=torch.uint8, device="cuda")
        res_t = torch.full(((S + 1) * U.STREAM_RESULT_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
        self.desc, self.res = eng.decode_streams(self.dw, self.dst, S, self.max_frames, wire_len=pos, desc=desc_t,
                                                 results=res_t, read_end=re_dev, n_reads=len(read_end))
        torch.cuda.synchronize()
        eng.sync()
        self.results = eng.read_stream_results(self.res, S)
        self.host_wire = self.dw.cpu().numpy()
        self.host_desc = self.desc.cpu().numpy()
        assert np.array_equal(self.host_wire[outside], wire[outside]), "bytes outside the connections were written"
        assert (self.host_desc[self.max_frames * 32:] == FILL).all(), "descriptors written past max_frames"
        assert (self.res.cpu().numpy()[S * U.STREAM_RESULT_BYTES:] == 0x5A).all(), "results written past n_streams"
        for r in self.results:
            assert r.first_status not in FAILED, r.as_dict()


def _deliver_streams(dec, what):
    import uvhttp_amd as U
    hw = (C.c_uint8 * dec.host_wire.size).from_buffer(dec.host_wire)
    hd = (C.c_uint8 * dec.host_desc.size).from_buffer(dec.host_desc)
    for k, e in enumerate(dec.entries):
        stream = U.Stream.from_buffer_copy(dec.st[k].tobytes())
        r = dec.results[k]
        h = RF.HostConn(e)
        try:
            with h:
                rc = U.lib().uvhttp_ws_deliver_stream(h.conn.ptr, hw, hd, C.byref(stream), C.byref(r))
            RF.check_delivery(e, h, rc, r.calls, what)
            end = e.transcript["end"]
            info = (e.seed, e.mode, r.as_dict())
            # the result record itself (include/uvhttp_ws_amd.h): stream bytes [consumed_bytes,
            # buffered_end) are what recv_buffer holds afterwards; both are 0 when the first call failed
            # its growth check, which returns before it touches the buffer (:836-857)
            if r.first_status == ERR_BUFFER and r.calls <= 1:
                assert (r.consumed_bytes, r.buffered_end, end[1]) == (0, 0, 0), info
            else:
                assert r.buffered_end - r.consumed_bytes == end[1], info
            assert r.recv_buffer_size == end[2], info
            # pending_bytes: the open message after the calls.  After a failing call the record is
            # held to the reference only through the connection (check_delivery above compares the
            # fragment state deliver_stream leaves): the neighbours (tests/test_gpu_streams.py) pin the
            # field for successful calls only, and so does this test
            if rc == 0:
                assert r.pending_bytes == (0 if end[5] else end[3]), info
        finally:
            h.close()


@pytest.mark.parametrize("side", ["server", "client"])
@pytest.mark.parametrize("engine", ["spec", "walk"])
def test_decode_reads_and_deliver_stream(torch, engines, host_hooks, engine, side):
    entries = [e for e in ENTRIES if e.side == side]
    assert len(entries) >= 100
    dec = Decoded(torch, engines[engine], entries, use_reads=True)
    _deliver_streams(dec, "decode_reads (%s)" % engine)


@pytest.mark.parametrize("side", ["server", "client"])
@pytest.mark.parametrize("engine", ["spec", "walk"])
def test_decode_streams_on_the_one_read_sessions(torch, engines, host_hooks, engine, side):
    entries = [e for e in ENTRIES if e.side == side and e.mode == "one"]
    assert len(entries) >= 20
    dec = Decoded(torch, engines[engine], entries, use_reads=False)
    _deliver_streams(dec, "decode_streams (%s)" % engine)


# ---- the batch forms on one-read-per-frame server sessions ---------------------------------------

def _batch_inputs(torch, e):
    offs = np.cumsum([0] + e.read_lens[:-1]).astype(np.uint64)
    n = len(e.wire)
    host = np.full(n + 64 + (-n) % 16, FILL, np.uint8)
    host[:n] = np.frombuffer(e.wire, np.uint8)
    return torch.from_numpy(host).to("cuda"), torch.from_numpy(offs.view(np.int64)).to("cuda"), host


@pytest.mark.parametrize("compact", [False, True], ids=["inplace", "compact"])
def test_batch_decodes_on_the_per_frame_server_sessions(torch, engines, host_hooks, compact):
    import uvhttp_amd as U
    eng = engines["spec"]
    for e in RF.batch_sessions(ENTRIES):
        nf, n = len(e.read_lens), len(e.wire)
        mf, mm = _limits(e)
        d, o, host = _batch_inputs(torch, e)
        desc_t = torch.full(((nf + 1) * 32,), FILL, dtype=torch.uint8, device="cuda")
        kw = dict(offsets=o, wire_len=n, max_frame_size=mf, max_message_size=mm, is_server=1, desc=desc_t)
        if compact:
            arena = torch.full((n + 64,), FILL, dtype=torch.uint8, device="cuda")
            msgs_t = torch.full(((nf + 2) * 32,), FILL, dtype=torch.uint8, device="cuda")
            desc, msgs, summ = eng.decode_compact(d, nf, arena[:n + 32], msgs=msgs_t, **kw)
        else:
            desc, summ = eng.decode_inplace(d, nf, **kw)
        torch.cuda.synchronize()
        s = eng.read_summary(summ)
        tr = e.transcript
        failed = tr["reads"][-1][0] != 0
        info = (e.seed, s)
        assert s["n_delivered"] == len(tr["reads"]) - (1 if failed else 0), info
        assert s["status"] == tr["reads"][-1][0], info
        hw = d.cpu().numpy()
        assert (hw[n:] == FILL).all(), "bytes past the wire were written"
        hd = desc.cpu().numpy()
        assert (hd[nf * 32:] == FILL).all(), "descriptors written past n_frames"
        h = RF.HostConn(e)
        try:
            with h:
                if compact:
                    ha = arena.cpu().numpy()
                    assert (ha[n + 32:] == FILL).all(), "the arena was written past its capacity"
                    hm = msgs_t.cpu().numpy()
                    assert (hm[(nf + 1) * 32:] == FILL).all(), "messages written past n_frames + 1"
                    rc = U.deliver_messages(h.conn, ha[: max(1, s["arena_bytes"])], hm[: (s["n_messages"] + 1) * 32],
                                            s, wire=hw[:n], desc=hd[: nf * 32])
                else:
                    cw = (C.c_uint8 * n).from_buffer_copy(hw[:n].tobytes())
                    cd = (C.c_uint8 * (32 * nf)).from_buffer_copy(hd[: nf * 32].tobytes())
                    cs = (C.c_uint8 * C.sizeof(U.BatchSummary)).from_buffer_copy(summ.cpu().numpy().tobytes())
                    rc = U.lib().uvhttp_ws_deliver_batch(h.conn.ptr, C.cast(cw, C.c_void_p), C.cast(cd, C.c_void_p),
                                                         C.cast(cs, C.c_void_p))
            RF.check_delivery(e, h, rc, None, "decode_compact" if compact else "decode_inplace", sizes=False)
        finally:
            h.close()


# ---- the frames sent ------------------------------------------------------------------------------

def _sender_batch(torch, eng, kind):
    """decode_reads over every session whose sender is `kind`, both sides -> (Decoded, slot keys:
    connection s's answer slots take its own key words, a server's slots zeros)"""
    entries = [e for e in ENTRIES if RF.sender_kind(e) == kind]
    assert len(entries) >= 30 and {e.is_server for e in entries} == {0, 1}
    assert sum(len(RF.sent_frames(e)) for e in entries) >= 30
    dec = Decoded(torch, eng, entries, use_reads=True)
    keys = []
    for e in entries:
        keys += [int(k) for k in e.keys] if not e.is_server else [0] * len(RF.sent_frames(e))
    return dec, np.array(keys + [0] * 8, np.uint32)


def _check_runs(dec, got, first_key, n_key):
    for s, e in enumerate(dec.entries):
        c = got["conn"][s]
        assert c["status"] == 0, (e.seed, c)
        off = got["out_off"]
        frames = [got["out"][off[j]:off[j + 1]] for j in range(c[first_key], c[first_key] + c[n_key])]
        RF.check_sent(e, frames, "the device's frames")
    assert got["summary"]["out_bytes"] == sum(
        f["n"] if isinstance(f, dict) else len(f) for e in dec.entries for f in RF.sent_frames(e))


def test_control_replies_streams_are_the_frames_the_reference_sent(torch, engines):
    from test_gpu_control_replies import Out
    eng = engines["spec"]
    dec, keys = _sender_batch(torch, eng, "replies")
    max_replies = len(keys)
    out_cap = 131 * max_replies
    o = Out(torch, dec.S, max_replies, out_cap)
    eng.control_replies_streams(dec.dw, dec.desc, dec.max_frames, dec.dst, dec.res, dec.S, max_replies, out_cap,
                                mask_keys=_dev(torch, keys, 0), out=o.out, out_off=o.off, runs=o.runs, conn=o.conn,
                                summary=o.summ, wire_len=dec.wire_len)
    torch.cuda.synchronize()
    _check_runs(dec, o.read(eng), "first_reply", "n_replies")


def test_echo_messages_streams_are_the_frames_the_reference_sent(torch, engines):
    from test_gpu_echo import Out
    eng = engines["spec"]
    dec, keys = _sender_batch(torch, eng, "echoes")
    max_echoes = len(keys)
    out_cap = 14 * max_echoes + dec.wire_len
    o = Out(torch, dec.S, max_echoes, out_cap, dec.wire_len)
    eng.echo_messages_streams(dec.dw, dec.desc, dec.max_frames, dec.dst, dec.res, dec.S, max_echoes, out_cap,
                              mask_keys=_dev(torch, keys, 0), wire_len=dec.wire_len, **o.kw())
    torch.cuda.synchronize()
    _check_runs(dec, o.read(eng), "first_echo", "n_echoes")


def test_answer_messages_streams_are_the_frames_the_reference_sent(torch, engines):
    """the frame order README claims for the answers, against frames the reference sent"""
    from test_gpu_answer import Out
    eng = engines["spec"]
    dec, keys = _sender_batch(torch, eng, "answers")
    max_answers = len(keys)
    out_cap = 14 * max_answers + dec.wire_len
    o = Out(torch, dec.S, max_answers, out_cap, dec.wire_len)
    eng.answer_messages_streams(dec.dw, dec.desc, dec.max_frames, dec.dst, dec.res, dec.S, max_answers, out_cap,
                                mask_keys=_dev(torch, keys, 0), wire_len=dec.wire_len, **o.kw())
    torch.cuda.synchronize()
    got = o.read(eng)
    _check_runs(dec, got, "first_answer", "n_answers")
    for s, e in enumerate(dec.entries):  # closed: a CLOSE was delivered <-> on_close ran
        assert got["conn"][s]["closed"] == int(any(ev[0] == "c" for ev in e.transcript["events"])), e.seed
