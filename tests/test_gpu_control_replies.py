"""uvhttp_ws_gpu_control_replies_streams / _inplace after decode_streams / decode_reads /
decode_inplace / decode_compact: device == the host twin uvhttp_ws_control_replies, byte for byte,
in d_out, d_out_off, the runs, the per-connection results and the summary — and == the frames the
existing host path hands the control sink (tests/_replies_ref.py) — for mixed batches, every scan
block boundary, every output alignment, read tables, the in-place form, the capacity failure, the
no-sync chain into uvhttp_tls_gpu_seal_frames, a captured graph and a seeded fuzz."""
import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
import _replies_ref as RR
import _tls_send_ref as TS

pytestmark = pytest.mark.gpu
SCAN_BLOCK = 256  # descriptors per workgroup of the scans (ws_replies_gpu.hip: kBlock)
GUARD, FILL = 64, 0xA5
FAILED = (-9, -10, -11)  # ERR_LAYOUT, ERR_CAPACITY, ERR_DEVICE: the connection considers nothing


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def eng(torch):
    import uvhttp_amd as U
    e = U.GpuEngine(0)
    yield e
    e.close()


def _dev(torch, a, pad=64):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.zeros(max(16, a.size + pad), dtype=torch.uint8, device="cuda")
    if a.size:
        d[: a.size] = torch.from_numpy(a.copy()).to("cuda")
    return d


def _raw(c):
    return bytes(c) if isinstance(c, (bytes, bytearray)) else b"".join(f.bytes for f in c)


def _streams(conns, is_server=None, reads=None, gap=0):
    """wire, stream table and read table of `conns` (raw bytes each) back to back"""
    wire, st, read_end = bytearray(), np.zeros(len(conns), O.STREAM_DT), []
    for s, b in enumerate(conns):
        srv = 1 if is_server is None else int(is_server[s])
        fr, nr = 0, 0
        if reads is not None and reads[s] is not None:
            fr, nr = len(read_end), len(reads[s])
            read_end += list(np.cumsum([len(r) for r in reads[s]]))
        st[s] = (len(wire), len(b), 65536, 0, 0, RR.MF, RR.MM, srv, fr, nr, 0)
        wire += b + b"\xff" * gap
    return np.frombuffer(bytes(wire) or b"\0", np.uint8).copy(), st, read_end


class Out:
    """guarded device outputs of one replies call, and their host copies"""

    def __init__(self, torch, S, max_replies, out_cap):
        t = torch
        self.S, self.max_replies, self.out_cap = S, max_replies, out_cap
        self.buf = t.full((GUARD + out_cap + GUARD,), FILL, dtype=t.uint8, device="cuda")
        self.out = self.buf[GUARD:GUARD + out_cap] if out_cap else self.buf[GUARD:GUARD + 1]
        self.off = t.full((max_replies + 2,), -7, dtype=t.int64, device="cuda")
        self.runs = t.full((2 * S + 2,), 0x5A5A5A5A, dtype=t.int32, device="cuda")
        self.conn = t.full((16 * S + 16,), FILL, dtype=t.uint8, device="cuda")
        self.summ = t.full((32,), FILL, dtype=t.uint8, device="cuda")

    def read(self, eng):
        summ = eng.read_reply_summary(self.summ)
        ok = summ["status"] == RR.OK
        buf = self.buf.cpu().numpy()
        n = summ["out_bytes"] if ok else 0
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), "d_out written outside the replies"
        off = self.off.cpu().numpy()
        assert off[-1] == -7, "d_out_off written past max_replies"
        runs = self.runs.cpu().numpy().view(np.uint32)
        assert (runs[2 * self.S:] == 0x5A5A5A5A).all()
        assert (self.conn.cpu().numpy()[16 * self.S:] == FILL).all()
        conn = eng.read_reply_conns(self.conn, self.S)
        assert [(int(runs[2 * s]), int(runs[2 * s + 1])) for s in range(self.S)] == \
            [(c["first_reply"], c["n_replies"]) for c in conn]
        return {"out": buf[GUARD:GUARD + n].tobytes(), "out_off": [int(x) for x in off[:-1]], "conn": conn,
                "summary": summ}


def _want(host, max_replies, out_cap):
    if host["summary"]["n_replies"] > max_replies or host["summary"]["out_bytes"] > out_cap:
        return RR.capacity_failure(host, max_replies)
    return host


def run_streams(torch, eng, conns, is_server=None, enable=None, keys=None, flags=0, reads=None, gap=0,
                max_frames=None, max_replies=None, out_cap=None, sink=True, silent=None):
    """decode_streams (decode_reads with `reads`) then control_replies_streams, no host sync
    between; everything the call writes against the host twin over the device's own decode, and
    (sink) against the control sink's frames -> (got, stream results)"""
    import uvhttp_amd as U
    conns = [_raw(c) for c in conns]
    S = len(conns)
    wire, st, read_end = _streams(conns, is_server, reads, gap)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    re_dev = torch.tensor(read_end or [0], dtype=torch.int64, device="cuda") if reads is not None else None
    if max_frames is None:
        max_frames = len(wire) // 2 + 1
    max_replies = max_frames if max_replies is None else max_replies
    out_cap = 131 * max_replies if out_cap is None else out_cap
    d_en = _dev(torch, np.array(enable, np.uint8), 0) if enable is not None else None
    d_keys = _dev(torch, np.asarray(keys, np.uint32), 0) if keys is not None else None
    o = Out(torch, S, max_replies, out_cap)
    desc, res = eng.decode_streams(dw, dst, S, max_frames, wire_len=wire.size, read_end=re_dev,
                                   n_reads=len(read_end))
    eng.control_replies_streams(dw, desc, max_frames, dst, res, S, max_replies, out_cap, enable=d_en,
                                mask_keys=d_keys, flags=flags, out=o.out, out_off=o.off, runs=o.runs,
                                conn=o.conn, summary=o.summ, wire_len=wire.size)
    torch.cuda.synchronize()
    got = o.read(eng)
    results = eng.read_stream_results(res, S)
    first = [r.first_frame for r in results]
    nd = [0 if r.first_status in FAILED else r.n_delivered for r in results]
    hw, hd = dw[: wire.size].cpu().numpy(), eng.read_desc(desc, max_frames)
    host = RR.host_batch(U, hw, hd, first, nd, is_server, enable, keys, flags, max_replies)
    assert got == _want(host, max_replies, out_cap)
    if sink:
        ref = RR.expected_batch(conns, is_server, enable, keys, flags, reads, silent or {}, max_replies)
        assert host == ref
    return got, results


# ---- the CPU cases in one batch of mixed connections --------------------------------------------

def _mixed_conns():
    P = RR.ping
    conns = [
        [RR.data(b"hello", 1), P(b""), RR.pong(b"xyz"), P(b"a"), RR.data(b"", 2), P(bytes(range(124))),
         RR.data(b"frag", 1, 0), P(bytes(range(125))), RR.data(b"ment", 0, 1), RR.pong(b""), RR.data(b"z" * 300)],
        [],
        [RR.data(b"x"), RR.close(b""), RR.data(b"y")],
        [RR.close(b"\x03")],
        [RR.close(b"\x03\xe8")],
        [RR.close(b"\x03\xe8!")],
        [RR.close(b"\x03\xe8" + b"r" * 123)],
        [P(b"1"), RR.close(b"\x03\xe9bye"), P(b"2"), RR.data(b"d"), P(b""), RR.close(b"\x03\xea"), P(b"3")],
        [P(b"before"), RR.data(b"ok"), RR.Fr(2, 1, b"bad", rsv=True), P(b"after"), RR.close(b"")],
        [P(b"quiet"), RR.close(b"\x03\xe8")],
        [],
        [P(b"abcde"), RR.data(b"x"), RR.close(b"\x03\xe8done"), P(b"no")],
        [P(bytes(range(125))), P(b"")],
        [RR.data(b"only data")],
    ]
    srv = [1] * len(conns)
    srv[11] = srv[12] = 0
    en = [1] * len(conns)
    en[9] = 0
    return conns, srv, en


@pytest.mark.parametrize("flags", [0, RR.AFTER_CLOSE])
def test_mixed_connections(torch, eng, flags):
    conns, srv, en = _mixed_conns()
    keys = RR.keys_for(random.Random(3), 64)
    got, res = run_streams(torch, eng, conns, srv, en, keys, flags, gap=3)
    assert [r.n_delivered for r in res][8] == 2
    assert got["conn"][7]["n_replies"] == (6 if flags else 2)
    assert got["conn"][9] == {"first_reply": got["conn"][8]["first_reply"] + 1, "n_replies": 0, "out_len": 0,
                              "status": RR.OK, "closed": 1}
    assert got["summary"]["n_closed_conns"] == 8


def test_client_connections_without_keys(torch, eng):
    conns, srv, en = _mixed_conns()
    got, _ = run_streams(torch, eng, conns, srv, en, None)
    assert [c["status"] for c in got["conn"]] == [RR.NO_KEYS if s in (11, 12) else RR.OK for s in range(len(conns))]
    assert got["conn"][11]["closed"] == 1 and got["conn"][11]["n_replies"] == 0


def test_failed_decode_results(torch, eng):
    """ERR_CAPACITY (max_frames too small: every connection) and ERR_LAYOUT (a read table whose
    last entry is not the length): nothing is considered"""
    conns, srv, en = _mixed_conns()
    conns = [_raw(c) for c in conns]
    got, res = run_streams(torch, eng, conns, srv, en, RR.keys_for(random.Random(4), 64), max_frames=10,
                           sink=False)
    assert {r.first_status for r, c in zip(res, conns) if c} == {-10}
    assert got["summary"] == {"out_bytes": 0, "n_replies": 0, "n_closed_conns": 0, "status": RR.OK}
    assert got["out_off"] == [0] * 11
    reads = [None] * len(conns)
    reads[0] = [conns[0][:5], conns[0][5:-1]]  # one byte short of the length
    reads[7] = [conns[7][:4], conns[7][4:]]
    got, res = run_streams(torch, eng, conns, srv, en, RR.keys_for(random.Random(5), 64), reads=reads,
                           silent={0: RR.OK})
    assert res[0].first_status == -9 and got["conn"][0]["n_replies"] == 0 and got["conn"][7]["n_replies"] == 2


def test_bad_payload_range(torch, eng):
    """wire_len cut short of a connection's last PING payload: BAD_RANGE, no replies for it, the
    others as before"""
    import uvhttp_amd as U
    conns = [_raw(c) for c in ([RR.ping(b"a"), RR.data(b"b")], [RR.ping(b"first"), RR.close(b""), RR.ping(b"second")])]
    wire, st, _ = _streams(conns)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 2, 8, wire_len=wire.size)
    short = wire.size - 2
    for flags in (0, RR.AFTER_CLOSE):
        o = Out(torch, 2, 8, 256)
        eng.control_replies_streams(dw, desc, 8, dst, res, 2, 8, 256, flags=flags, out=o.out, out_off=o.off,
                                    runs=o.runs, conn=o.conn, summary=o.summ, wire_len=short)
        torch.cuda.synchronize()
        got = o.read(eng)
        results = eng.read_stream_results(res, 2)
        host = RR.host_batch(U, dw[: wire.size].cpu().numpy(), eng.read_desc(desc, 8), [r.first_frame for r in results],
                             [r.n_delivered for r in results], flags=flags, max_replies=8, wire_len=short)
        assert got == host
        assert got["conn"][1] == {"first_reply": 1, "n_replies": 0, "out_len": 0, "status": RR.BAD_RANGE, "closed": 1}
        assert got["out"] == b"\x8a\x01a"


# ---- scan boundaries ---------------------------------------------------------------------------

# (the last two: more than 64 and more than 256 block aggregates, so the top scan of the head marks
# carries across a wave boundary, and every lane of it folds a run of more than one aggregate)
@pytest.mark.parametrize("n", [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1,
                               64 * SCAN_BLOCK + 1, 256 * SCAN_BLOCK + 1])
@pytest.mark.parametrize("mode", ["none", "one", "ends", "all"])
def test_scan_boundaries(torch, eng, n, mode):
    """n descriptors exactly (max_frames = n) over three connections, the middle one straddling
    the block boundaries; replies: none, one in the middle, the very first and the very last
    descriptor, every frame"""
    def frame(i):
        hit = {"none": False, "one": i == SCAN_BLOCK - 3, "ends": i in (0, n - 1), "all": True}[mode]
        return RR.ping(bytes([i & 0xFF]) * (i % 7)) if hit else RR.data(bytes([i & 0xFF]))
    cuts = [0, 100, n - 7, n]
    conns = [[frame(i) for i in range(cuts[k], cuts[k + 1])] for k in range(3)]
    got, res = run_streams(torch, eng, conns, max_frames=n, sink=(n == SCAN_BLOCK + 1))
    assert sum(r.n_delivered for r in res) == n
    assert got["summary"]["n_replies"] == {"none": 0, "one": 1, "ends": 2, "all": n}[mode]
    assert sum(c["n_replies"] for c in got["conn"]) == got["summary"]["n_replies"]


# ---- alignment ---------------------------------------------------------------------------------

@pytest.mark.parametrize("client", [0, 1])
def test_every_alignment_and_length(torch, eng, client):
    """PING lengths 0..125 in sequence: every frame length, and reply starts at every residue
    mod 16; guard bytes around d_out stay as they were (Out.read)"""
    conns = [[RR.ping(bytes((7 * i + k) & 0xFF for k in range(i))) for i in range(126)], [RR.close(b"\x03\xe8end")]]
    keys = RR.keys_for(random.Random(6), 200)
    got, _ = run_streams(torch, eng, conns, [1 - client] * 2, None, keys, out_cap=127 * 131 - 5)
    assert {x % 16 for x in got["out_off"][:127]} == set(range(16))
    assert got["summary"]["n_replies"] == 127


# ---- read tables -------------------------------------------------------------------------------

def test_reads_split_a_ping_and_complete_a_close(torch, eng):
    a = [RR.data(b"lead"), RR.ping(b"split across two reads"), RR.data(b"tail")]
    b = [RR.ping(b"whole"), RR.close(b"\x03\xe8completed by the last read")]
    ra, rb = _raw(a), _raw(b)
    cut_a = len(a[0].bytes) + 9           # inside the PING's payload
    cut_b = len(rb) - 4                   # the CLOSE lacks its last four bytes until the last read
    reads = [[ra[:cut_a], ra[cut_a:]], [rb[:3], rb[3:cut_b], rb[cut_b:]]]
    got, res = run_streams(torch, eng, [ra, rb], reads=reads)
    assert [r.calls for r in res] == [2, 3]
    assert [c["n_replies"] for c in got["conn"]] == [1, 2] and got["conn"][1]["closed"] == 1
    # the CLOSE is still incomplete when the reads stop short: no echo yet
    got, res = run_streams(torch, eng, [ra, rb[:cut_b]], reads=[reads[0], reads[1][:2]])
    assert [c["n_replies"] for c in got["conn"]] == [1, 1] and got["conn"][1]["closed"] == 0


# ---- the in-place form -------------------------------------------------------------------------

@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("client", [0, 1])
def test_inplace_form(torch, eng, compact, client):
    import uvhttp_amd as U
    rng = random.Random(40 + client)
    frames = RR.D.mixed(rng, 300, sizes=(0, 1, 7, 100, 300), p_ctrl=0.3, p_res=0.0, bad_at=280)
    raw = b"".join(f.bytes for f in frames)
    n = len(frames)
    wire = np.frombuffer(raw, np.uint8).copy()
    offs = np.cumsum([0] + [len(f.bytes) for f in frames[:-1]]).astype(np.uint64)
    dw = _dev(torch, wire)
    kw = dict(offsets=torch.from_numpy(offs.view(np.int64)).to("cuda"), wire_len=wire.size, max_frame_size=RR.MF,
              max_message_size=RR.MM, is_server=1 - client)
    keys = RR.keys_for(rng, n)
    flags = RR.AFTER_CLOSE if compact else 0  # (the mix holds a CLOSE early on)
    o = Out(torch, 1, n, 131 * n)
    if compact:
        arena = torch.zeros(wire.size + 64, dtype=torch.uint8, device="cuda")
        desc, _, summ = eng.decode_compact(dw, n, arena, **kw)
    else:
        desc, summ = eng.decode_inplace(dw, n, **kw)
    eng.control_replies_inplace(dw, desc, n, summ, n, 131 * n, is_server=1 - client, mask_keys=_dev(torch, keys, 0),
                                flags=flags, out=o.out, out_off=o.off, runs=o.runs, conn=o.conn, summary=o.summ, wire_len=wire.size)
    torch.cuda.synchronize()
    got = o.read(eng)
    nd = eng.read_summary(summ)["n_delivered"]
    assert nd == 280
    host = RR.host_batch(U, dw[: wire.size].cpu().numpy(), eng.read_desc(desc, n), [0], [nd], [1 - client], None, keys,
                         flags, n)
    assert got == host
    # the sink's frames for the delivered part of the batch
    assert host == RR.expected_batch([b"".join(f.bytes for f in frames[:nd])], [1 - client], None, keys, flags, None, {}, n)
    assert got["summary"]["n_replies"] > 20 if flags else got["conn"][0]["closed"] == 1


# ---- capacity ----------------------------------------------------------------------------------

def test_capacity_one_short(torch, eng):
    conns, srv, en = _mixed_conns()
    keys = RR.keys_for(random.Random(8), 64)
    full, _ = run_streams(torch, eng, conns, srv, en, keys)
    n, nbytes = full["summary"]["n_replies"], full["summary"]["out_bytes"]
    for kw in (dict(max_replies=n - 1, out_cap=nbytes), dict(max_replies=n, out_cap=nbytes - 1)):
        got, _ = run_streams(torch, eng, conns, srv, en, keys, sink=False, **kw)
        assert got["summary"] == dict(full["summary"], status=RR.ERR_CAPACITY)
        assert got["out"] == b"" and set(got["out_off"]) == {0}
        assert {c["status"] for c in got["conn"]} == {RR.ERR_CAPACITY}
    # a second call with the reported sizes succeeds
    got, _ = run_streams(torch, eng, conns, srv, en, keys, sink=False, max_replies=n, out_cap=nbytes)
    assert got["out"] == full["out"] and got["conn"] == full["conn"] and got["out_off"] == full["out_off"][:n + 1]


# ---- the no-sync chain -------------------------------------------------------------------------

def test_chain_records_in_sealed_replies_out(torch):
    """seal_records (the clients' PINGs / CLOSEs) -> open_records -> ws_streams -> decode_reads ->
    control_replies_streams -> seal_frames with n_sends = n_streams and a pre-filled sends table:
    no host read before the end.  The sealed replies, opened by the oracle, are the control
    sink's frames of every connection."""
    import uvhttp_amd as U
    t = torch
    rng = random.Random(77)
    S = 24
    kinds = [TS.KEY_KINDS[rng.randrange(6)] for _ in range(S)]
    keys = np.concatenate([TS.make_key(rng, k) for k in kinds] + [TS.make_key(rng, k) for k in kinds])
    plains, recs_rows, tls_st, reads = [], [], np.zeros(S, O.TLS_STREAM_DT), []
    src_pos, out_pos = 0, 0
    for c in range(S):
        fr = []
        for _ in range(rng.randint(0, 10)):
            r = rng.random()
            if r < 0.45:
                fr.append(RR.ping(rng.randbytes(rng.choice([0, 1, 5, 60, 125])), rng.randbytes(4)))
            elif r < 0.55:
                fr.append(RR.close(rng.choice([b"", b"\x03\xe8", b"\x03\xe9going away"])))
            elif r < 0.65:
                fr.append(RR.pong(rng.randbytes(3)))
            else:
                fr.append(RR.data(rng.randbytes(rng.choice([1, 20, 200, 3000]))))
        plain = _raw(fr)
        seq0, begin, pos, j, rd = rng.randrange(1 << 40), out_pos, 0, 0, []
        while pos < len(plain):
            n = min(len(plain) - pos, rng.choice([1, 7, 40, 500, 16384]))
            recs_rows.append((src_pos + pos, out_pos, seq0 + j, n, c, 23, 0))
            rd.append(plain[pos:pos + n])
            out_pos += n + TS.overhead(keys[c])
            pos += n
            j += 1
        tls_st[c] = (begin, out_pos - begin, seq0, c, 0)
        plains.append(plain)
        reads.append(rd or None)
        src_pos += len(plain)
    seal = np.array(recs_rows, O.TLS_SEAL_DT)
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")  # noqa: E731
    eng_t, eng_w = U.TlsEngine(0), U.GpuEngine(0)
    d_keys, d_src = dev(keys), dev(np.frombuffer(b"".join(plains), np.uint8))
    cipher = t.zeros(out_pos + 64, dtype=t.uint8, device="cuda")
    max_records = len(seal) + 1
    plain_cap = max(16, out_pos)  # the opened content lies where its records lay: the ciphertext's size
    plain_out = t.zeros(plain_cap + 64, dtype=t.uint8, device="cuda")
    ws = []
    for c in range(S):
        s = U.Stream()
        conn = U.WsConnection(1, RR.MF, RR.MM)
        U.lib().uvhttp_ws_stream_init(conn.ptr, 0, 0, C.byref(s))
        ws.append(bytes(s))
    ws_dev = dev(np.frombuffer(b"".join(ws), np.uint8))
    read_end = t.zeros(max_records, dtype=t.int64, device="cuda")
    max_frames = max_replies = 512
    out_cap = 131 * max_replies
    sends = np.zeros(S, TS.TLS_SEND_DT)
    seq_s = [rng.randrange(1 << 40) for _ in range(S)]
    for c in range(S):
        sends[c] = (seq_s[c], 0xDEAD, 0xBEEF, S + c, 23, 0, 0)  # first_frame / n_frames: the call's
    d_sends = dev(sends)
    sealed = t.zeros(max_replies * 170, dtype=t.uint8, device="cuda")

    eng_t.seal_records(d_src, dev(seal), len(seal), d_keys, len(keys), cipher[:out_pos])
    tls_dev = dev(tls_st)
    recs, res = eng_t.open_records(cipher, d_keys, len(keys), tls_dev, S, max_records, plain_out[:plain_cap],
                                   wire_len=out_pos)
    eng_t.ws_streams(res, recs, S, tls_dev, plain_out, ws_dev, read_end)
    desc, wres = eng_w.decode_streams(plain_out, ws_dev, S, max_frames, wire_len=plain_cap, read_end=read_end,
                                      n_reads=max_records)
    out, off, rconn, rsum = eng_w.control_replies_streams(plain_out, desc, max_frames, ws_dev, wres, S, max_replies,
                                                          out_cap, runs=d_sends[8:], run_stride=32,
                                                          wire_len=plain_cap)
    _, sres, ssum = eng_t.seal_frames(out, off, max_replies, d_sends, S, d_keys, len(keys), max_replies, sealed,
                                      frames_len=out_cap)
    t.cuda.synchronize()  # the first host read

    want = RR.expected_batch(plains, reads=reads)
    assert eng_w.read_reply_summary(rsum) == want["summary"] and want["summary"]["n_replies"] > 20
    assert eng_w.read_reply_conns(rconn, S) == want["conn"]
    sr = sres.cpu().numpy()[:S * 48].view(TS.TLS_SEND_RESULT_DT)
    assert (sr["status"] == 0).all()
    assert [int(x) for x in sr["n_records"]] == [c["n_replies"] for c in want["conn"]]
    # open every connection's sealed run with the oracle: the plaintext is its reply frames
    host_sealed = sealed.cpu().numpy()
    open_st = np.zeros(S, O.TLS_STREAM_DT)
    for c in range(S):
        open_st[c] = (int(sr[c]["out_off"]), int(sr[c]["out_len"]), seq_s[c], S + c, 0)
    total = int(ssum.cpu().numpy().view(TS.TLS_SEND_SUMMARY_DT)[0]["out_bytes"])
    o_recs, o_res, o_out = O.tls_open_batch(host_sealed[:max(1, total)], keys, open_st, out_cap=total + 16)
    for c in range(S):
        r, w = o_res[c], want["conn"][c]
        assert r["n_delivered"] == w["n_replies"]
        got = b"".join(o_out[rec["out_off"]:rec["out_off"] + rec["content_len"]].tobytes()
                       for rec in o_recs[r["first_record"]:r["first_record"] + r["n_delivered"]])
        lo = want["out_off"][w["first_reply"]]
        assert got == want["out"][lo:lo + w["out_len"]], c
    eng_w.close()
    eng_t.close()


# ---- a captured graph --------------------------------------------------------------------------

def test_graph_replay(torch, eng):
    """decode_streams + control_replies_streams captured on a side stream after one uncaptured
    call of the shape, replayed over two wires of the same layout: the replies follow the bytes"""
    import uvhttp_amd as U
    rng = random.Random(9)
    a = [[RR.data(rng.randbytes(20)), RR.ping(rng.randbytes(9)), RR.pong(b"12345"), RR.close(b"\x03\xe8")] for _ in range(8)]
    b = [[RR.data(rng.randbytes(20)), RR.ping(rng.randbytes(9)), RR.ping(b"54321"), RR.pong(b"\x03\xe8")] for _ in range(8)]
    (w0, st, _), (w1, st1, _) = _streams([_raw(c) for c in a]), _streams([_raw(c) for c in b])
    assert w0.size == w1.size and (st == st1).all()
    S, mf = 8, 40
    dw, dst = _dev(torch, w0), _dev(torch, st, 0)
    desc = torch.zeros(mf * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
    o = Out(torch, S, mf, 131 * mf)

    def both(stream=None):
        eng.decode_streams(dw, dst, S, mf, desc=desc, results=res, wire_len=w0.size, stream=stream)
        eng.control_replies_streams(dw, desc, mf, dst, res, S, mf, 131 * mf, out=o.out, out_off=o.off, runs=o.runs,
                                    conn=o.conn, summary=o.summ, wire_len=w0.size, stream=stream)

    both()
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        both(cs)
    for w, conns in ((w0, a), (w1, b), (w0, a)):
        dw[: w.size] = torch.from_numpy(w).to("cuda")
        o.buf.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = o.read(eng)
        want = RR.expected_batch([_raw(c) for c in conns], max_replies=mf)
        assert got == want
        assert got["summary"]["n_closed_conns"] == (8 if conns is a else 0)


# ---- a seeded fuzz -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_fuzz_small_batches(torch, eng, seed):
    """60 small batches per seed: random connections of mixed frames (half of them control
    frames, some failing part-way), servers and clients, enable bits, both flags, sometimes a
    capacity one short: device == host twin"""
    rng = random.Random(7000 + seed)
    seen = 0
    for _ in range(60):
        conns, srv = [], []
        for _ in range(rng.randint(1, 12)):
            fr = RR.D.mixed(rng, rng.randint(0, 20), sizes=(0, 1, 7, 100, 300), p_ctrl=0.5, p_res=0.0,
                            bad_at=rng.choice([None, None, 5]))
            conns.append(b"".join(f.bytes for f in fr))
            srv.append(rng.choice([1, 1, 0]))
        keys = RR.keys_for(rng, 300) if rng.random() < 0.8 else None
        enable = [rng.choice([1, 1, 1, 0]) for _ in conns] if rng.random() < 0.5 else None
        kw = {}
        if rng.random() < 0.2:
            kw = dict(max_replies=rng.randint(0, 8), out_cap=rng.randint(0, 300))
        got, _ = run_streams(torch, eng, conns, srv, enable, keys, rng.choice([0, RR.AFTER_CLOSE]),
                             gap=rng.choice([0, 1, 5]), sink=False, **kw)
        seen += got["summary"]["n_replies"]
    assert seen > 500


# ---- arguments ---------------------------------------------------------------------------------

def test_arguments(torch, eng):
    import uvhttp_amd as U
    wire, st, _ = _streams([_raw([RR.ping(b"ok")])])
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 1, 4, wire_len=wire.size)
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    o = Out(torch, 1, 4, 64)
    torch.cuda.synchronize()

    class Null:
        def data_ptr(self):
            return None

    base = dict(wire=dw, desc=desc, streams_dev=dst, results=res, out=o.out, out_off=o.off, conn=o.conn,
                summary=o.summ, batch_summary=summ, mask_keys=None, runs=None)

    def streams(max_frames=4, max_replies=4, run_stride=8, n_streams=1, **kw):
        a = dict(base, **kw)
        eng.control_replies_streams(a["wire"], a["desc"], max_frames, a["streams_dev"], a["results"], n_streams,
                                    max_replies, 64, mask_keys=a["mask_keys"], out=a["out"], out_off=a["out_off"],
                                    runs=a["runs"], run_stride=run_stride, conn=a["conn"], summary=a["summary"],
                                    wire_len=wire.size)

    def inplace(max_replies=4, run_stride=8, **kw):
        a = dict(base, **kw)
        eng.control_replies_inplace(a["wire"], a["desc"], 1, a["batch_summary"], max_replies, 64,
                                    mask_keys=a["mask_keys"], out=a["out"], out_off=a["out_off"], runs=a["runs"],
                                    run_stride=run_stride, conn=a["conn"], summary=a["summary"], wire_len=wire.size)

    streams()
    inplace()
    for call, names in ((streams, ["wire", "desc", "streams_dev", "results", "out", "out_off", "conn", "summary"]),
                        (inplace, ["wire", "desc", "batch_summary", "out", "out_off", "conn", "summary"])):
        for name in names:
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**{name: Null()})
            if name != "out":  # d_out may start at any byte
                view = base[name].view(torch.uint8) if name == "out_off" else base[name]
                with pytest.raises(U.GpuError, match="rc=-1"):
                    call(**{name: view[1:]})
        for bad in (dict(mask_keys=dw[1:]), dict(runs=dw[2:]), dict(runs=o.runs, run_stride=4),
                    dict(runs=o.runs, run_stride=10), dict(max_replies=(1 << 28) + 1)):
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**bad)
    with pytest.raises(U.GpuError, match="rc=-1"):
        streams(max_frames=(1 << 28) + 1)
    with pytest.raises(U.GpuError, match="rc=-1"):
        streams(n_streams=(1 << 31) + 1)
    torch.cuda.synchronize()
