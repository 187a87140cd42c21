"""uvhttp_ws_gpu_echo_messages_streams / _inplace after decode_streams / decode_reads /
decode_inplace / decode_compact: device == the host twin uvhttp_ws_echo_messages, byte for byte,
in d_out, d_out_off, the runs, d_open, d_open_off, the per-connection results and the summary —
and == the frames process_data's on_message makes (tests/_echo_ref.py) — for mixed batches, every
source and destination alignment, the header steps, every scan block boundary, read tables, two
calls chained through d_open -> d_carry, build_frames over the same messages, the in-place form,
the capacity failures, the no-sync chain into uvhttp_tls_gpu_seal_frames, a captured graph, the
emit in several pieces and a seeded fuzz."""
import ctypes as C
import random

import numpy as np
import pytest

import _echo_ref as ER
import _oracle as O
import _tls_send_ref as TS
from test_gpu_build import BUILD_DT
from test_gpu_epoch_wrap import _engine

pytestmark = pytest.mark.gpu
SCAN_BLOCK = 256   # descriptors per workgroup of the scans (ws_echo_gpu.hip: kBlock)
TILE = 65536       # output bytes per workgroup of the emit (kTile)
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


def _streams(conns, is_server=None, reads=None, pending=None, gap=0):
    """wire, stream table and read table of `conns` (raw bytes each) back to back"""
    wire, st = ER.streams_of(conns, is_server, pending, gap)
    read_end = []
    for s in range(len(conns)):
        if reads is not None and reads[s] is not None:
            st[s]["first_read"], st[s]["n_reads"] = len(read_end), len(reads[s])
            read_end += list(np.cumsum([len(r) for r in reads[s]]))
    return wire, st, read_end


class Out:
    """guarded device outputs of one echo call, and their host copies"""

    def __init__(self, torch, S, max_echoes, out_cap, open_cap, with_open=True):
        t = torch
        self.S, self.max_echoes, self.out_cap, self.open_cap = S, max_echoes, out_cap, open_cap
        self.buf = t.full((GUARD + out_cap + GUARD,), FILL, dtype=t.uint8, device="cuda")
        self.out = self.buf[GUARD:GUARD + out_cap] if out_cap else self.buf[GUARD:GUARD + 1]
        self.obuf = t.full((GUARD + open_cap + GUARD,), FILL, dtype=t.uint8, device="cuda")
        self.open = (self.obuf[GUARD:GUARD + open_cap] if open_cap else self.obuf[GUARD:GUARD + 1]) if with_open else None
        self.off = t.full((max_echoes + 2,), -7, dtype=t.int64, device="cuda")
        self.ooff = t.full((S + 2,), -7, dtype=t.int64, device="cuda")
        self.runs = t.full((2 * S + 2,), 0x5A5A5A5A, dtype=t.int32, device="cuda")
        self.conn = t.full((32 * S + 32,), FILL, dtype=t.uint8, device="cuda")
        self.summ = t.full((32,), FILL, dtype=t.uint8, device="cuda")

    def kw(self):
        return dict(out=self.out, out_off=self.off, runs=self.runs, open=self.open, open_cap=self.open_cap,
                    open_off=self.ooff, conn=self.conn, summary=self.summ)

    def read(self, eng):
        summ = eng.read_echo_summary(self.summ)
        ok = summ["status"] == ER.OK
        buf, obuf = self.buf.cpu().numpy(), self.obuf.cpu().numpy()
        n = summ["out_bytes"] if ok else 0
        m = summ["open_bytes"] if ok and self.open is not None else 0
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), "d_out written outside the echoes"
        assert (obuf[:GUARD] == FILL).all() and (obuf[GUARD + m:] == FILL).all(), "d_open written outside the messages"
        off, ooff = self.off.cpu().numpy(), self.ooff.cpu().numpy()
        assert off[-1] == -7 and ooff[-1] == -7, "an offset table written past its end"
        runs = self.runs.cpu().numpy().view(np.uint32)
        assert (runs[2 * self.S:] == 0x5A5A5A5A).all()
        assert (self.conn.cpu().numpy()[32 * self.S:] == FILL).all()
        conn = eng.read_echo_conns(self.conn, self.S)
        assert [(int(runs[2 * s]), int(runs[2 * s + 1])) for s in range(self.S)] == \
            [(c["first_echo"], c["n_echoes"]) for c in conn]
        return {"out": buf[GUARD:GUARD + n].tobytes(), "out_off": [int(x) for x in off[:-1]],
                "open": obuf[GUARD:GUARD + m].tobytes(), "open_off": [int(x) for x in ooff[:-1]], "conn": conn,
                "summary": summ}


def _want(host, max_echoes, out_cap, open_cap, with_open=True):
    s = host["summary"]
    if s["n_echoes"] > max_echoes or s["out_bytes"] > out_cap or (with_open and s["open_bytes"] > open_cap):
        return ER.capacity_failure(host, max_echoes)
    return host if with_open else dict(host, open=b"")


def run_streams(torch, eng, conns, is_server=None, enable=None, keys=None, flags=0, reads=None, pending=None,
                carries=None, gap=0, max_frames=None, max_echoes=None, out_cap=None, open_cap=None, with_open=True,
                ref=True, silent=None, ref_eng=None):
    """decode_streams (decode_reads with `reads`) then echo_messages_streams, no host sync between;
    everything the call writes against the host twin over the device's own decode, and (ref)
    against the on_message reference -> (got, stream results)"""
    import uvhttp_amd as U
    conns = [ER.raw(c) for c in conns]
    S = len(conns)
    wire, st, read_end = _streams(conns, is_server, reads, pending, gap)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    re_dev = torch.tensor(read_end or [0], dtype=torch.int64, device="cuda") if reads is not None else None
    if max_frames is None:
        max_frames = len(wire) // 2 + 1
    carry, coff = ER.carry_tables(pending, S)
    if carries is not None:
        carry, coff = ER.carry_tables([(0, c) for c in carries], S)
    max_echoes = max_frames if max_echoes is None else max_echoes
    out_cap = 14 * max_echoes + len(wire) + len(carry) if out_cap is None else out_cap
    open_cap = len(wire) + len(carry) if open_cap is None else open_cap
    d_en = _dev(torch, np.array(enable, np.uint8), 0) if enable is not None else None
    d_keys = _dev(torch, np.asarray(keys, np.uint32), 0) if keys is not None else None
    d_carry = _dev(torch, np.frombuffer(carry, np.uint8)) if pending is not None or carries is not None else None
    d_coff = torch.tensor(coff, dtype=torch.int64, device="cuda") if d_carry is not None else None
    o = Out(torch, S, max_echoes, out_cap, open_cap, with_open)
    desc, res = eng.decode_streams(dw, dst, S, max_frames, wire_len=wire.size, read_end=re_dev,
                                   n_reads=len(read_end))
    eng.echo_messages_streams(dw, desc, max_frames, dst, res, S, max_echoes, out_cap, enable=d_en,
                              mask_keys=d_keys, flags=flags, carry=d_carry, carry_len=len(carry),
                              carry_off=d_coff, wire_len=wire.size, **o.kw())
    torch.cuda.synchronize()
    got = o.read(eng)
    results = eng.read_stream_results(res, S)
    first = [r.first_frame for r in results]
    nd = [0 if r.first_status in FAILED else r.n_delivered for r in results]
    hw, hd = dw[: wire.size].cpu().numpy(), eng.read_desc(desc, max_frames)
    host = ER.host_batch(U, hw, hd, first, nd, is_server, enable, keys, flags, pending, carries, max_echoes)
    assert got == _want(host, max_echoes, out_cap, open_cap, with_open)
    if got["summary"]["status"] == ER.OK:
        for s, c in enumerate(got["conn"]):  # the open message is the decoder's
            if c["status"] == ER.OK and (enable is None or enable[s]) and results[s].first_status not in FAILED:
                assert c["open_len"] == results[s].pending_bytes, s
    if ref:
        want = ER.expected_batch(conns, is_server, enable, keys, flags, reads, pending, silent or {}, max_echoes)
        assert host == want
    if ref_eng is not None:  # the same call on an unsplit engine: byte for byte
        o2 = Out(torch, S, max_echoes, out_cap, open_cap, with_open)
        ref_eng.echo_messages_streams(dw, desc, max_frames, dst, res, S, max_echoes, out_cap, enable=d_en,
                                      mask_keys=d_keys, flags=flags, carry=d_carry, carry_len=len(carry),
                                      carry_off=d_coff, wire_len=wire.size, **o2.kw())
        torch.cuda.synchronize()
        assert o2.read(ref_eng) == got
    return got, results


def _payload(n, salt=0):
    return bytes((salt + 31 * i + (i >> 8)) & 0xFF for i in range(n))


# ---- the CPU cases in one batch of mixed connections --------------------------------------------

def _mixed_conns():
    P = ER.ping(b"\xff\xfe")
    T, B, K = ER.text, ER.binary, ER.cont
    conns = [
        [T(b""), B(b"a"), T(_payload(125)), B(_payload(126, 1)), T(_payload(127, 2))],
        [],
        [T(b"ab", 0), K(b"cd")],
        [B(b"abc", 0), K(b"", 0), K(b"defg")],
        [T(b"x" * 100, 0), P, K(b"y" * 30, 0), P, P, K(b"")],
        [T(b"", 0), T(b"fresh")],
        [T(b"before"), T(b"open", 0), ER.close(b"\x03\xe8"), K(b"ed"), T(b"after")],
        [T(b"ok"), B(b"part", 0), ER.Fr(0, 1, b"bad", rsv=True), T(b"never")],
        [T(b"quiet"), T(b"op", 0)],
        [],
        [T(b"abcde"), P, B(b"fr", 0), K(b"agment")],
        [T(_payload(300, 3))],
        [K(b" world"), T(b"next", 0)],
        [K(b"more", 0), P],
        [],
        [B(_payload(65535, 4)), T(_payload(65536, 5)), B(_payload(65537, 6))],
    ]
    S = len(conns)
    srv = [1] * S
    srv[10] = srv[11] = 0
    en = [1] * S
    en[8] = 0
    pending = [None] * S
    pending[12], pending[13], pending[14] = (1, b"hello"), (2, _payload(200, 7)), (1, b"idle")
    return conns, srv, en, pending


@pytest.mark.parametrize("flags", [0, ER.SERVER_SEND])
def test_mixed_connections(torch, eng, flags):
    conns, srv, en, pending = _mixed_conns()
    keys = ER.keys_for(random.Random(3), 64)
    got, res = run_streams(torch, eng, conns, srv, en, keys, flags, pending=pending, gap=3)
    assert [r.n_delivered for r in res][7] == 2
    assert got["conn"][6]["n_echoes"] == 1 and got["conn"][8] == dict(ER.ZERO, first_echo=got["conn"][7]["first_echo"] + 1)
    assert got["conn"][14]["open_len"] == 4 and got["conn"][13]["open_len"] == 204
    assert got["conn"][0]["n_echoes"] == (4 if flags else 5)


def test_client_connections_without_keys(torch, eng):
    conns, srv, en, pending = _mixed_conns()
    got, _ = run_streams(torch, eng, conns, srv, en, None, pending=pending)
    assert [c["status"] for c in got["conn"]] == [ER.NO_KEYS if s in (10, 11) else ER.OK for s in range(len(conns))]


def test_carry_missing_or_short(torch, eng):
    conns, srv, en, pending = _mixed_conns()
    carries = [p[1] if p else b"" for p in pending]
    carries[12] = b"hell"
    got, _ = run_streams(torch, eng, conns, srv, en, ER.keys_for(random.Random(3), 64), pending=pending,
                         carries=carries, silent={12: ER.NO_CARRY})
    assert got["conn"][12] == dict(ER.ZERO, first_echo=got["conn"][12]["first_echo"], status=ER.NO_CARRY)
    # no carry buffer at all: every carrying connection says so, and no open bytes are asked for
    wire, st, _ = _streams([ER.raw(c) for c in conns], srv, None, pending)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    mf = wire.size // 2 + 1
    desc, res = eng.decode_streams(dw, dst, len(conns), mf, wire_len=wire.size)
    _, _, _, conn, summ = eng.echo_messages_streams(dw, desc, mf, dst, res, len(conns), mf, wire.size + 14 * mf,
                                                    wire_len=wire.size, mask_keys=_dev(torch, ER.keys_for(random.Random(1), mf), 0))
    torch.cuda.synchronize()
    st_ = [c["status"] for c in eng.read_echo_conns(conn, len(conns))]
    assert [s for s, x in enumerate(st_) if x == ER.NO_CARRY] == [12, 13, 14]


def test_failed_decode_results(torch, eng):
    """ERR_CAPACITY (max_frames too small: every connection) and ERR_LAYOUT (a read table whose
    last entry is not the length): nothing is considered, a carry passes through"""
    conns, srv, en, pending = _mixed_conns()
    conns = [ER.raw(c) for c in conns]
    keys = ER.keys_for(random.Random(4), 64)
    got, res = run_streams(torch, eng, conns, srv, en, keys, pending=pending, max_frames=10, ref=False)
    assert {r.first_status for r, c in zip(res, conns) if c} == {-10}
    assert got["summary"] == {"out_bytes": 0, "open_bytes": 209, "n_echoes": 0, "status": ER.OK}
    assert got["out_off"] == [0] * 11 and got["open"] == b"hello" + _payload(200, 7) + b"idle"
    reads = [None] * len(conns)
    reads[0] = [conns[0][:5], conns[0][5:-1]]  # one byte short of the length
    reads[2] = [conns[2][:3], conns[2][3:]]
    got, res = run_streams(torch, eng, conns, srv, en, keys, reads=reads, pending=pending, silent={0: ER.OK})
    assert res[0].first_status == -9 and got["conn"][0]["n_echoes"] == 0 and got["conn"][2]["n_echoes"] == 1


def test_bad_payload_range(torch, eng):
    """wire_len cut short of a connection's last payload: BAD_RANGE, nothing for it, the others
    as before"""
    import uvhttp_amd as U
    conns = [ER.raw(c) for c in ([ER.text(b"a"), ER.binary(b"bc", 0)], [ER.text(b"first"), ER.text(b"second")])]
    wire, st, _ = _streams(conns)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 2, 8, wire_len=wire.size)
    short = wire.size - 2
    o = Out(torch, 2, 8, 256, 64)
    eng.echo_messages_streams(dw, desc, 8, dst, res, 2, 8, 256, wire_len=short, **o.kw())
    torch.cuda.synchronize()
    got = o.read(eng)
    results = eng.read_stream_results(res, 2)
    host = ER.host_batch(U, dw[: wire.size].cpu().numpy(), eng.read_desc(desc, 8), [r.first_frame for r in results],
                         [r.n_delivered for r in results], max_echoes=8, wire_len=short)
    assert got == host
    assert got["conn"][1] == dict(ER.ZERO, first_echo=1, status=ER.BAD_RANGE)
    assert got["out"] == b"\x81\x01a" and got["open"] == b"bc"


# ---- alignment ---------------------------------------------------------------------------------

@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("many", [0, 1])
def test_every_alignment_and_length(torch, eng, client, many):
    """message lengths 0..300 in sequence, as one connection and as 301: every source and
    destination residue mod 16 and the 125 / 126 header step; guard bytes stay (Out.read)"""
    msgs = [ER.Fr(1 + (i & 1), 1, _payload(i, i)) for i in range(301)]
    conns = [[m] for m in msgs] if many else [msgs]
    keys = ER.keys_for(random.Random(6), 400)
    got, _ = run_streams(torch, eng, conns, [1 - client] * len(conns), None, keys, gap=many)
    assert {x % 16 for x in got["out_off"][:301]} == set(range(16))
    assert got["summary"]["n_echoes"] == 301


@pytest.mark.parametrize("client", [0, 1])
def test_large_messages_split_at_their_ends(torch, eng, client):
    """65 535 / 65 536 / 65 537 bytes, split 1 + rest and rest + 1: the 4 / 10 byte header step,
    several emit tiles per message, a join one byte from either end"""
    conns = []
    for n in (65535, 65536, 65537):
        p = _payload(n, n)
        conns += [[ER.binary(p[:1], 0), ER.cont(p[1:])], [ER.text(p[:-1], 0), ER.ping(b"mid"), ER.cont(p[-1:])]]
    keys = ER.keys_for(random.Random(16), 16)
    got, _ = run_streams(torch, eng, conns, [1 - client] * 6, None, keys)
    assert got["summary"]["n_echoes"] == 6 and got["summary"]["out_bytes"] > 5 * TILE


@pytest.mark.parametrize("client", [0, 1])
def test_whole_tiles(torch, eng, client):
    """messages that cover whole emit tiles: from one fragment, from the carry, and from three
    fragments (no tile of it has one source record-wide); a short one after each so that the next
    starts at an odd offset"""
    conns = [[ER.binary(_payload(200000, 1)), ER.text(b"abc")],
             [ER.cont(b"0123456789"), ER.text(_payload(140001, 2))],
             [ER.text(_payload(70000, 3), 0), ER.cont(_payload(70001, 4), 0), ER.cont(_payload(70002, 5))],
             [ER.cont(_payload(150000, 6), 0)]]
    pending = [None, (2, _payload(150000, 7)), None, (1, _payload(70000, 8))]
    keys = ER.keys_for(random.Random(17), 16)
    got, _ = run_streams(torch, eng, conns, [1 - client] * 4, None, keys, pending=pending)
    assert got["summary"]["n_echoes"] == 5 and got["summary"]["open_bytes"] == 220000


# ---- scan boundaries ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1])
@pytest.mark.parametrize("mode", ["none", "one", "ends", "all"])
def test_scan_boundaries(torch, eng, n, mode):
    """n descriptors exactly (max_frames = n) over three connections, the middle one straddling
    the block boundaries; data messages: none, one in the middle, the very first and the very
    last descriptor, every frame"""
    def frame(i):
        hit = {"none": False, "one": i == SCAN_BLOCK - 3, "ends": i in (0, n - 1), "all": True}[mode]
        return ER.binary(bytes([i & 0xFF]) * (i % 7)) if hit else ER.ping(bytes([i & 0xFF]))
    cuts = [0, 100, n - 7, n]
    conns = [[frame(i) for i in range(cuts[k], cuts[k + 1])] for k in range(3)]
    got, res = run_streams(torch, eng, conns, max_frames=n, ref=(n == SCAN_BLOCK + 1))
    assert sum(r.n_delivered for r in res) == n
    assert got["summary"]["n_echoes"] == {"none": 0, "one": 1, "ends": 2, "all": n}[mode]


def test_fragments_across_scan_blocks(torch, eng):
    """one message of 600 one-byte fragments with PINGs between (its frames span three scan
    blocks), then a second connection: the message length and the frame search cross blocks"""
    p = _payload(600, 9)
    a = []
    for i in range(600):
        a += [ER.Fr(2 if i == 0 else 0, i == 599, p[i:i + 1])] + ([ER.ping(b"")] if i % 5 == 0 else [])
    got, _ = run_streams(torch, eng, [a, [ER.text(b"tail")]])
    assert got["out"][:4] == b"\x82\x7e\x02\x58" and got["out"][4:604] == p


# ---- read tables -------------------------------------------------------------------------------

def test_message_split_across_reads(torch, eng):
    a = [ER.text(b"lead"), ER.binary(b"split across ", 0), ER.cont(b"two reads"), ER.text(b"tail", 0)]
    ra = ER.raw(a)
    cut = len(a[0].bytes) + len(a[1].bytes) + 9  # inside the CONTINUATION
    got, res = run_streams(torch, eng, [ra, ER.raw([ER.text(b"whole")])], reads=[[ra[:cut], ra[cut:]], None])
    assert res[0].calls == 2 and got["conn"][0]["n_echoes"] == 2 and got["open"] == b"tail"
    # the reads stop short of the CONTINUATION's end: its message stays open
    got, res = run_streams(torch, eng, [ra[:cut]], reads=[[ra[:10], ra[10:cut]]])
    assert got["conn"][0]["n_echoes"] == 1 and got["open"] == b"split across "


# ---- build_frames over the same messages -------------------------------------------------------

def test_equals_build_frames(torch, eng):
    """unfragmented server batches: d_out and d_out_off are what build_frames makes of a
    host-made descriptor table of the same messages"""
    rng = random.Random(21)
    conns = [[ER.Fr(rng.choice([1, 2]), 1, rng.randbytes(rng.choice([0, 1, 125, 126, 999, 70000])))
              for _ in range(rng.randint(0, 6))] for _ in range(12)]
    wire, st, _ = _streams([ER.raw(c) for c in conns])
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    n = sum(map(len, conns))
    desc, res = eng.decode_streams(dw, dst, len(conns), n, wire_len=wire.size)
    cap = wire.size + 16
    out, off, _, _, summ = eng.echo_messages_streams(dw, desc, n, dst, res, len(conns), n, cap, wire_len=wire.size)
    torch.cuda.synchronize()
    hd = eng.read_desc(desc, n)
    table = np.zeros(n, BUILD_DT)
    table["payload_off"], table["payload_len"], table["opcode"], table["fin"] = hd["payload_off"], hd["payload_len"], hd["opcode"], 1
    out2 = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    off2 = eng.build_frames(dw[: wire.size], _dev(torch, table, 0), n, out2)
    torch.cuda.synchronize()
    total = eng.read_echo_summary(summ)["out_bytes"]
    assert eng.read_echo_summary(summ)["n_echoes"] == n and total == int(off2[n])
    assert (off.cpu().numpy() == off2.cpu().numpy()).all()
    assert out[:total].cpu().numpy().tobytes() == out2[:total].cpu().numpy().tobytes()


# ---- two calls chained through d_open -> d_carry ------------------------------------------------

@pytest.mark.parametrize("client", [0, 1])
def test_chained_calls_at_every_frame_boundary(torch, eng, client):
    """a 3-message, 7-fragment connection cut at every frame boundary: connection k of call 1
    gets frames [0, k), of call 2 the rest with call 1's (d_open, d_open_off, open_bytes) as its
    (d_carry, d_carry_off, carry_len) as they lie.  The echoes of both calls together are those
    of one call over the whole wire"""
    frames = [ER.text(b"first ", 0), ER.cont(b"message", 0), ER.cont(b" done"), ER.binary(_payload(130, 1), 0),
              ER.cont(_payload(70, 2)), ER.text(b"x", 0), ER.cont(b"yz")]
    cuts = list(range(1, 7))
    S = len(cuts)
    srv = [1 - client] * S
    keys = ER.keys_for(random.Random(31), 64)
    whole, _ = run_streams(torch, eng, [frames], [1 - client], None, keys)
    msgs = [whole["out"][whole["out_off"][j]:whole["out_off"][j + 1]] for j in range(3)]

    w1, st1, _ = _streams([ER.raw(frames[:k]) for k in cuts], srv)
    dw1, dst1 = _dev(torch, w1), _dev(torch, st1, 0)
    desc1, res1 = eng.decode_streams(dw1, dst1, S, 64, wire_len=w1.size)
    o1 = Out(torch, S, 64, 4096, 4096)
    d_keys = _dev(torch, keys, 0)
    eng.echo_messages_streams(dw1, desc1, 64, dst1, res1, S, 64, 4096, mask_keys=d_keys, wire_len=w1.size, **o1.kw())
    torch.cuda.synchronize()
    got1 = o1.read(eng)
    r1 = eng.read_stream_results(res1, S)
    # call 2's stream table: the decoder's pending bytes and the echo call's open opcode
    pend2 = [(c["open_opcode"], b"\0" * r.pending_bytes) for c, r in zip(got1["conn"], r1)]
    w2, st2, _ = _streams([ER.raw(frames[k:]) for k in cuts], srv, None, pend2)
    dw2, dst2 = _dev(torch, w2), _dev(torch, st2, 0)
    desc2, res2 = eng.decode_streams(dw2, dst2, S, 64, wire_len=w2.size)
    o2 = Out(torch, S, 64, 4096, 4096)
    keys2 = keys[got1["summary"]["n_echoes"]:]  # so that the slots of both calls differ
    eng.echo_messages_streams(dw2, desc2, 64, dst2, res2, S, 64, 4096, mask_keys=_dev(torch, keys2, 0),
                              carry=o1.open, carry_len=got1["summary"]["open_bytes"], carry_off=o1.ooff,
                              wire_len=w2.size, **o2.kw())
    torch.cuda.synchronize()
    got2 = o2.read(eng)
    assert all(c["status"] == ER.OK for c in got2["conn"]) and got2["open"] == b""

    def unmask(b):  # a client echo with its key taken off, so that echoes of different slots compare
        if not client:
            return b
        h = 2 if b[1] & 0x7F < 126 else 4 if b[1] & 0x7F == 126 else 10
        k = b[h:h + 4]
        return b[:h] + bytes(x ^ k[i & 3] for i, x in enumerate(b[h + 4:]))

    for s in range(S):
        both = []
        for g in (got1, got2):
            c = g["conn"][s]
            both += [g["out"][g["out_off"][j]:g["out_off"][j + 1]] for j in range(c["first_echo"], c["first_echo"] + c["n_echoes"])]
        assert [unmask(b) for b in both] == [unmask(m) for m in msgs], cuts[s]


# ---- the in-place form -------------------------------------------------------------------------

@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("client", [0, 1])
def test_inplace_form(torch, eng, compact, client):
    """after decode_inplace with the wire, after decode_compact with the arena as d_wire"""
    import uvhttp_amd as U
    rng = random.Random(40 + client)
    rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 7, 100, 300, 5000]))) for _ in range(60)]
    frames = ER.FR.fragment_randomly(rng, rows) + [ER.text(b"left open", 0), ER.ping(b"p")]
    raw = ER.raw(frames)
    n = len(frames)
    wire = np.frombuffer(raw, np.uint8).copy()
    offs = np.cumsum([0] + [len(f.bytes) for f in frames[:-1]]).astype(np.uint64)
    dw = _dev(torch, wire)
    kw = dict(offsets=torch.from_numpy(offs.view(np.int64)).to("cuda"), wire_len=wire.size, max_frame_size=ER.MF,
              max_message_size=ER.MM, is_server=1 - client)
    keys = ER.keys_for(rng, n)
    o = Out(torch, 1, n, wire.size + 14 * n, wire.size)
    if compact:
        arena = torch.zeros(wire.size + 64, dtype=torch.uint8, device="cuda")
        desc, _, summ = eng.decode_compact(dw, n, arena, **kw)
        src, src_len = arena, wire.size
    else:
        desc, summ = eng.decode_inplace(dw, n, **kw)
        src, src_len = dw, wire.size
    eng.echo_messages_inplace(src, desc, n, summ, n, wire.size + 14 * n, is_server=1 - client,
                              mask_keys=_dev(torch, keys, 0), wire_len=src_len, **o.kw())
    torch.cuda.synchronize()
    got = o.read(eng)
    bs = eng.read_summary(summ)
    assert bs["n_delivered"] == n
    host = ER.host_batch(U, src[:src_len].cpu().numpy(), eng.read_desc(desc, n), [0], [n], [1 - client], None, keys,
                         max_echoes=n)
    assert got == host
    assert host == ER.expected_batch([raw], [1 - client], None, keys, max_echoes=n)
    assert got["open"] == b"left open" and got["conn"][0]["open_len"] == bs["pending_bytes"]
    assert got["summary"]["n_echoes"] == 60


# ---- capacity ----------------------------------------------------------------------------------

def test_capacity_one_short(torch, eng):
    conns, srv, en, pending = _mixed_conns()
    keys = ER.keys_for(random.Random(8), 64)
    full, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending)
    n, nbytes, nopen = (full["summary"][k] for k in ("n_echoes", "out_bytes", "open_bytes"))
    assert nopen > 0
    for kw in (dict(max_echoes=n - 1, out_cap=nbytes, open_cap=nopen), dict(max_echoes=n, out_cap=nbytes - 1, open_cap=nopen),
               dict(max_echoes=n, out_cap=nbytes, open_cap=nopen - 1)):
        got, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending, ref=False, **kw)
        assert got["summary"] == dict(full["summary"], status=ER.ERR_CAPACITY)
        assert got["out"] == b"" and got["open"] == b"" and set(got["out_off"]) == {0} and set(got["open_off"]) == {0}
        assert {c["status"] for c in got["conn"]} == {ER.ERR_CAPACITY}
    # a second call with the reported sizes succeeds; without d_open, open_cap is not tested
    got, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending, ref=False, max_echoes=n, out_cap=nbytes,
                         open_cap=nopen)
    assert got["out"] == full["out"] and got["open"] == full["open"] and got["conn"] == full["conn"]
    got, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending, ref=False, max_echoes=n, out_cap=nbytes,
                         open_cap=0, with_open=False)
    assert got["out"] == full["out"] and got["open_off"] == full["open_off"]


# ---- the no-sync chain -------------------------------------------------------------------------

def _parse_unmasked(b):
    """[(opcode, payload)] of unmasked frames back to back"""
    out, i = [], 0
    while i < len(b):
        n, h = b[i + 1] & 0x7F, 2
        if n == 126:
            n, h = int.from_bytes(b[i + 2:i + 4], "big"), 4
        elif n == 127:
            n, h = int.from_bytes(b[i + 2:i + 10], "big"), 10
        assert b[i] & 0x80 and not b[i + 1] & 0x80
        out.append((b[i] & 0x0F, bytes(b[i + h:i + h + n])))
        i += h + n
    return out


def test_chain_records_in_sealed_echoes_out(torch):
    """seal_records (the clients' messages) -> open_records -> ws_streams -> decode_reads ->
    echo_messages_streams -> seal_frames with n_sends = n_streams and a pre-filled sends table:
    no host read before the end.  The sealed echoes, opened by the oracle and decoded, are the
    messages every connection sent."""
    import uvhttp_amd as U
    t = torch
    rng = random.Random(78)
    S = 24
    kinds = [TS.KEY_KINDS[rng.randrange(6)] for _ in range(S)]
    keys = np.concatenate([TS.make_key(rng, k) for k in kinds] + [TS.make_key(rng, k) for k in kinds])
    plains, sent, recs_rows, tls_st, reads = [], [], [], np.zeros(S, O.TLS_STREAM_DT), []
    src_pos, out_pos = 0, 0
    for c in range(S):
        rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 20, 200, 3000, 20000]))) for _ in range(rng.randint(0, 6))]
        plain = ER.raw(ER.FR.fragment_randomly(rng, rows))
        sent.append(rows)
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
    plain_cap = max(16, out_pos)
    plain_out = t.zeros(plain_cap + 64, dtype=t.uint8, device="cuda")
    ws = []
    for c in range(S):
        s = U.Stream()
        conn = U.WsConnection(1, ER.MF, ER.MM)
        U.lib().uvhttp_ws_stream_init(conn.ptr, 0, 0, C.byref(s))
        ws.append(bytes(s))
    ws_dev = dev(np.frombuffer(b"".join(ws), np.uint8))
    read_end = t.zeros(max_records, dtype=t.int64, device="cuda")
    max_frames = max_echoes = 2048
    out_cap = src_pos + 14 * max_echoes
    sends = np.zeros(S, TS.TLS_SEND_DT)
    seq_s = [rng.randrange(1 << 40) for _ in range(S)]
    for c in range(S):
        sends[c] = (seq_s[c], 0xDEAD, 0xBEEF, S + c, 23, 0, 0)  # first_frame / n_frames: the call's
    d_sends = dev(sends)
    max_out_records = max_echoes + out_cap // 16384 + 1
    sealed = t.zeros(out_cap + max_out_records * 64, dtype=t.uint8, device="cuda")

    eng_t.seal_records(d_src, dev(seal), len(seal), d_keys, len(keys), cipher[:out_pos])
    tls_dev = dev(tls_st)
    recs, res = eng_t.open_records(cipher, d_keys, len(keys), tls_dev, S, max_records, plain_out[:plain_cap],
                                   wire_len=out_pos)
    eng_t.ws_streams(res, recs, S, tls_dev, plain_out, ws_dev, read_end)
    desc, wres = eng_w.decode_streams(plain_out, ws_dev, S, max_frames, wire_len=plain_cap, read_end=read_end,
                                      n_reads=max_records)
    out, off, _, econn, esum = eng_w.echo_messages_streams(plain_out, desc, max_frames, ws_dev, wres, S, max_echoes,
                                                           out_cap, runs=d_sends[8:], run_stride=32,
                                                           wire_len=plain_cap)
    _, sres, ssum = eng_t.seal_frames(out, off, max_echoes, d_sends, S, d_keys, len(keys), max_out_records, sealed,
                                      frames_len=out_cap)
    t.cuda.synchronize()  # the first host read

    want = ER.expected_batch(plains, reads=reads)
    assert eng_w.read_echo_summary(esum) == want["summary"] and want["summary"]["n_echoes"] > 30
    assert eng_w.read_echo_conns(econn, S) == want["conn"]
    sr = sres.cpu().numpy()[:S * 48].view(TS.TLS_SEND_RESULT_DT)
    assert (sr["status"] == 0).all()
    host_sealed = sealed.cpu().numpy()
    open_st = np.zeros(S, O.TLS_STREAM_DT)
    for c in range(S):
        open_st[c] = (int(sr[c]["out_off"]), int(sr[c]["out_len"]), seq_s[c], S + c, 0)
    total = int(ssum.cpu().numpy().view(TS.TLS_SEND_SUMMARY_DT)[0]["out_bytes"])
    o_recs, o_res, o_out = O.tls_open_batch(host_sealed[:max(1, total)], keys, open_st, out_cap=total + 16)
    for c in range(S):
        r, w = o_res[c], want["conn"][c]
        got = b"".join(o_out[rec["out_off"]:rec["out_off"] + rec["content_len"]].tobytes()
                       for rec in o_recs[r["first_record"]:r["first_record"] + r["n_delivered"]])
        lo = want["out_off"][w["first_echo"]]
        assert got == want["out"][lo:lo + w["out_len"]], c
        assert _parse_unmasked(got) == sent[c], c
    eng_w.close()
    eng_t.close()


# ---- a captured graph --------------------------------------------------------------------------

def test_graph_replay(torch, eng):
    """decode_streams + echo_messages_streams captured on a side stream after one uncaptured call
    of the shape, replayed over two wires of the same layout: the echoes follow the bytes"""
    rng = random.Random(9)

    def conns_of(second_fin):
        return [[ER.text(rng.randbytes(20)), ER.binary(rng.randbytes(300), 0), ER.cont(rng.randbytes(9), second_fin),
                 ER.ping(b"12345")] for _ in range(8)]
    a, b = conns_of(1), conns_of(0)
    (w0, st, _), (w1, st1, _) = _streams([ER.raw(c) for c in a]), _streams([ER.raw(c) for c in b])
    assert w0.size == w1.size and (st == st1).all()
    S, mf, cap = 8, 40, 4096
    dw, dst = _dev(torch, w0), _dev(torch, st, 0)
    desc = torch.zeros(mf * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
    o = Out(torch, S, mf, cap, cap)

    def both(stream=None):
        eng.decode_streams(dw, dst, S, mf, desc=desc, results=res, wire_len=w0.size, stream=stream)
        eng.echo_messages_streams(dw, desc, mf, dst, res, S, mf, cap, wire_len=w0.size, stream=stream, **o.kw())

    both()
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        both(cs)
    for w, conns in ((w0, a), (w1, b), (w0, a)):
        dw[: w.size] = torch.from_numpy(w).to("cuda")
        o.buf.fill_(FILL)
        o.obuf.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = o.read(eng)
        assert got == ER.expected_batch([ER.raw(c) for c in conns], max_echoes=mf)
        assert got["summary"]["n_echoes"] == (16 if conns is a else 8)
        assert got["summary"]["open_bytes"] == (0 if conns is a else 8 * 309)


# ---- the emit in several pieces -----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_grid_pieces(torch, monkeypatch, n):
    """the main cases with the emit's tiles going out in launches of n workgroups
    (UVHTTP_WS_GRID_PIECE, the experiment build), against the references and, byte for byte,
    against an unsplit engine"""
    split = _engine(monkeypatch, {"UVHTTP_WS_GRID_PIECE": n})
    whole = _engine(monkeypatch, {})
    try:
        conns, srv, en, pending = _mixed_conns()
        keys = ER.keys_for(random.Random(3), 64)
        split.grid_pieces()
        got, _ = run_streams(torch, split, conns, srv, en, keys, pending=pending, gap=3, ref_eng=whole)
        passes, pieces, tiles = split.grid_pieces()
        assert tiles >= 5 and pieces >= -(-tiles // n) and pieces > passes
        big = [[ER.binary(_payload(65537, 1)[:1], 0), ER.cont(_payload(65537, 1)[1:]), ER.text(_payload(40000, 2), 0)],
               [ER.text(_payload(65535, 3))]]
        got, _ = run_streams(torch, split, big, [0, 1], None, keys, ref_eng=whole)
        assert got["summary"]["out_bytes"] > 2 * TILE and got["summary"]["open_bytes"] == 40000
    finally:
        whole.close()
        split.close()


# ---- a seeded fuzz -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_fuzz_small_batches(torch, eng, seed):
    """50 batches per seed of at most 64 connections and 2 000 frames: random messages cut into
    fragments with PINGs between, a CLOSE or a failing frame part-way, carried-in messages,
    servers and clients, enable bits, both flags, sometimes a capacity too small: device == host
    twin"""
    rng = random.Random(7100 + seed)
    seen = 0
    for _ in range(50):
        conns, srv, pending = [], [], []
        budget = 2000
        for _ in range(rng.randint(1, 64)):
            rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 5, 15, 16, 17, 125, 126, 300, 2000])))
                    for _ in range(rng.randint(0, 5))]
            fr = ER.FR.fragment_randomly(rng, rows)
            pend = None
            if rng.random() < 0.3:
                pend = (rng.choice([1, 2]), rng.randbytes(rng.choice([1, 3, 16, 200])))
                pre = [ER.cont(rng.randbytes(rng.choice([0, 2, 40])), 0) for _ in range(rng.randint(0, 2))]
                fr = pre + [ER.cont(rng.randbytes(rng.choice([0, 7])))] + fr if rng.random() < 0.7 else pre
            if rng.random() < 0.2 and fr:
                fr.insert(rng.randrange(len(fr) + 1), ER.close(b"\x03\xe8"))
            if rng.random() < 0.15 and fr:
                fr.insert(rng.randrange(len(fr) + 1), ER.Fr(2, 1, b"bad", rsv=True))
            if rng.random() < 0.3:
                fr = fr[:max(0, len(fr) - 1)]
            fr = fr[:budget]
            budget -= len(fr)
            conns.append(ER.raw(fr))
            srv.append(rng.choice([1, 1, 0]))
            pending.append(pend)
        keys = ER.keys_for(rng, 400) if rng.random() < 0.8 else None
        enable = [rng.choice([1, 1, 1, 0]) for _ in conns] if rng.random() < 0.5 else None
        kw = {}
        if rng.random() < 0.2:
            kw = dict(max_echoes=rng.randint(0, 40), out_cap=rng.randint(0, 20000), open_cap=rng.randint(0, 300))
        got, _ = run_streams(torch, eng, conns, srv, enable, keys, rng.choice([0, ER.SERVER_SEND]), pending=pending,
                             gap=rng.choice([0, 1, 5]), ref=False, with_open=rng.random() < 0.9, **kw)
        seen += got["summary"]["n_echoes"]
    assert seen > 1000


# ---- arguments ---------------------------------------------------------------------------------

def test_arguments(torch, eng):
    import uvhttp_amd as U
    wire, st, _ = _streams([ER.raw([ER.text(b"ok")])])
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 1, 4, wire_len=wire.size)
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    o = Out(torch, 1, 4, 64, 64)
    torch.cuda.synchronize()

    class Null:
        def data_ptr(self):
            return None

    base = dict(wire=dw, desc=desc, streams_dev=dst, results=res, batch_summary=summ, mask_keys=None, carry=None,
                carry_off=None, **o.kw())
    del base["open_cap"]

    def streams(max_frames=4, max_echoes=4, run_stride=8, n_streams=1, **kw):
        a = dict(base, **kw)
        eng.echo_messages_streams(a["wire"], a["desc"], max_frames, a["streams_dev"], a["results"], n_streams,
                                  max_echoes, 64, mask_keys=a["mask_keys"], carry=a["carry"], carry_off=a["carry_off"],
                                  out=a["out"], out_off=a["out_off"], runs=a["runs"], run_stride=run_stride,
                                  open=a["open"], open_cap=64, open_off=a["open_off"], conn=a["conn"],
                                  summary=a["summary"], wire_len=wire.size)

    def inplace(max_echoes=4, run_stride=8, **kw):
        a = dict(base, **kw)
        eng.echo_messages_inplace(a["wire"], a["desc"], 1, a["batch_summary"], max_echoes, 64,
                                  mask_keys=a["mask_keys"], out=a["out"], out_off=a["out_off"], runs=a["runs"],
                                  run_stride=run_stride, open=a["open"], open_cap=64, open_off=a["open_off"],
                                  conn=a["conn"], summary=a["summary"], wire_len=wire.size)

    streams()
    inplace()
    for call, names in ((streams, ["wire", "desc", "streams_dev", "results", "out", "out_off", "open_off", "conn", "summary"]),
                        (inplace, ["wire", "desc", "batch_summary", "out", "out_off", "open_off", "conn", "summary"])):
        for name in names:
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**{name: Null()})
            view = base[name].view(torch.uint8) if name in ("out_off", "open_off") else base[name]
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**{name: view[1:]})
        for bad in (dict(mask_keys=dw[1:]), dict(runs=dw[2:]), dict(runs=o.runs, run_stride=4), dict(open=o.obuf[1:]),
                    dict(runs=o.runs, run_stride=10), dict(max_echoes=(1 << 28) + 1)):
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**bad)
    for bad in (dict(carry=dw[1:]), dict(carry_off=o.ooff.view(torch.uint8)[1:]), dict(max_frames=(1 << 28) + 1),
                dict(n_streams=(1 << 31) + 1)):
        with pytest.raises(U.GpuError, match="rc=-1"):
            streams(**bad)
    torch.cuda.synchronize()
