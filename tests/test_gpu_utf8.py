"""uvhttp_ws_gpu_validate_utf8 on the device against CPython's strict decoder
(tests/_utf8_ref.py): the known answers at every alignment within a vector, a 4-byte character
across every power-of-two offset (whatever vector, wave and workgroup sizes the kernel uses),
the cases a kernel that ignores message boundaries gets wrong, the message table of a real
compact decode (fragmented messages, the open message's PREFIX / tail, a batch that fails
part-way), a fuzz corpus, a captured graph and two streams."""
import random

import numpy as np
import pytest

import _deliver as D
import _utf8_ref as R

pytestmark = pytest.mark.gpu
MF = 16 * 1024 * 1024
SENT = 0xEE  # verdict entries the call must not touch


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


def _dev(torch, b):
    """host bytes -> device uint8 tensor (padded to a non-empty allocation)"""
    a = np.frombuffer(bytes(b), np.uint8)
    d = torch.zeros(max(16, a.size), dtype=torch.uint8, device="cuda")
    if a.size:
        d[: a.size] = torch.from_numpy(a.copy()).to("cuda")
    return d


def _table(torch, table):
    m = np.zeros(max(1, len(table)), D.MSG_DT)
    for i, (off, ln, op) in enumerate(table):
        m[i] = (off, ln, i, i, op, 0)
    return torch.from_numpy(m.view(np.uint8).copy()).to("cuda")


def _generic(torch, eng, data, table, data_len=None, extra=3):
    """the generic form over `table` = [(arena_off, len, opcode)] -> ([(status, tail)], summary);
    the verdict array has `extra` entries past max_msgs, which must stay untouched"""
    n = len(table)
    dl = len(data) if data_len is None else data_len
    d = _dev(torch, data)
    verdict = torch.full(((n + extra) * 4,), SENT, dtype=torch.uint8, device="cuda")
    v, s = eng.validate_utf8(d[:dl], _table(torch, table), n, n_msgs=n, verdict=verdict)
    torch.cuda.synchronize()
    got = eng.read_utf8(v, n + extra)
    assert (v[n * 4:].cpu().numpy() == SENT).all()
    return [(int(x["status"]), int(x["tail"])) for x in got[:n]], eng.read_utf8_summary(s)


def _check_generic(torch, eng, data, table, data_len=None):
    got, summ = _generic(torch, eng, data, table, data_len)
    ref, rsumm = R.judge(bytes(data), table, data_len)
    bad = [(i, table[i], g, r) for i, (g, r) in enumerate(zip(got, ref)) if g != r]
    assert not bad, bad[:5]
    assert summ == rsumm
    return got, summ


def _pack(rows, start=0, fill=b"a"):
    """messages back to back from offset `start` (an ASCII TEXT message before them when
    start > 0) -> (data, table)"""
    data, table = bytearray(), []
    if start:
        data += fill * start
        table.append((0, start, 1))
    for op, b in rows:
        table.append((len(data), len(b), op))
        data += b
    return bytes(data), table


KNOWN = ([bytes.fromhex(h) for h in R.KNOWN_VALID] + [bytes.fromhex(h) for h in R.KNOWN_INVALID] +
         [bytes.fromhex(h) for h, _ in R.KNOWN_TRUNCATED])


@pytest.mark.parametrize("start", range(16))
def test_known_answers_every_alignment(torch, eng, start):
    """each known answer its own TEXT message, packed back to back, the first at `start`"""
    data, table = _pack([(1, b) for b in KNOWN], start)
    got, summ = _check_generic(torch, eng, data, table)
    k = 1 if start else 0
    nv = len(R.KNOWN_VALID)
    assert [s for s, _ in got[k:k + nv]] == [R.VALID] * nv
    assert [s for s, _ in got[k + nv:]] == [R.INVALID] * (len(KNOWN) - nv)  # truncated: complete messages
    assert summ["n_invalid"] == len(KNOWN) - nv and summ["first_invalid"] == k + nv


BOUNDS = [1 << k for k in range(4, 17)]


@pytest.mark.parametrize("mode", ["valid", "invalid", "alternate"])
@pytest.mark.parametrize("split", [1, 2, 3])
def test_every_power_of_two_boundary(torch, eng, split, mode):
    """F0 9F 98 80 across every offset B = 16 .. 65536 with `split` bytes before B, one message
    per B (message B covers [3B/4, 3B/2)); the invalid twin ends in 41 instead of 80"""
    data = bytearray(b"a" * (128 * 1024))
    table, want = [], []
    for k, B in enumerate(BOUNDS):
        bad = mode == "invalid" or (mode == "alternate" and k % 2 == 0)
        data[B - split:B - split + 4] = b"\xf0\x9f\x98\x41" if bad else b"\xf0\x9f\x98\x80"
        table.append((B - B // 4, B // 4 + B // 2, 1))
        want.append(R.INVALID if bad else R.VALID)
    got, _ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got] == want


def test_whole_arena_one_message(torch, eng):
    """one 128 KiB message with a character across every boundary: VALID; then one bad byte
    deep inside it (the packed-word path): INVALID"""
    data = bytearray(b"a" * (128 * 1024))
    for k, B in enumerate(BOUNDS):
        at = B - (1 + k % 3)
        data[at:at + 4] = b"\xf0\x9f\x98\x80"
    got, _ = _check_generic(torch, eng, data, [(0, len(data), 1)])
    assert got == [(R.VALID, 0)]
    for at, bad in ((70001, 0x80), (4096, 0xC0), (8191, 0xE2), (len(data) - 1, 0xC2)):
        d2 = bytearray(data)
        d2[at] = bad
        got, _ = _check_generic(torch, eng, d2, [(0, len(d2), 1)])
        assert got == [(R.INVALID, 0)], at


@pytest.mark.parametrize("at", [5, 15, 16, 17, 1023, 1024, 1025, 4096, 16384])
def test_boundary_confusion(torch, eng, at):
    """message boundaries at offset `at` (inside a vector, at and around offsets 16 and 1024, at
    a wave's and a workgroup's first byte): what a kernel that ignores them gets wrong"""
    V, I, N = R.VALID, R.INVALID, R.NOT_TEXT
    # E2 82 | AC: concatenated they are the euro sign
    data, table = _pack([(1, b"\xe2\x82"), (1, b"\xac")], at - 2)
    got, _ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got[-2:]] == [I, I]
    data, table = _pack([(1, b"ok\xf0\x9f"), (1, b"\x98\x80ok")], at - 4)
    got, _ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got[-2:]] == [I, I]
    # a BINARY message's bytes are not examined and do not leak into its neighbours
    data, table = _pack([(1, b"abc"), (2, b"\xff\xfe\x80"), (1, "déf".encode())], at - 3)
    got, _ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got[-3:]] == [V, N, V]
    data, table = _pack([(1, b"ab\xc3"), (2, b"\xa9\xfe\x80"), (1, b"\x80f")], at - 3)
    got, _ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got[-3:]] == [I, N, I]
    # zero-length TEXT messages between two others
    for first, last, want in ((b"a", "é".encode(), [V] * 5), (b"\xe2\x82", b"\xac", [I, V, V, V, I])):
        data, table = _pack([(1, first), (1, b""), (1, b""), (1, b""), (1, last)], at - len(first))
        got, _ = _check_generic(torch, eng, data, table)
        assert [s for s, _ in got[-5:]] == want
    # a gap of garbage between two ranges of a generic table
    data = b"a" * (at - 2) + "é".encode() + b"\x80\x80\x80" + "ü".encode() + b"zz"
    table = [(0, at, 1), (at + 3, 4, 1)]
    got, _ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got] == [V, V]
    # ... and with the sequence cut by the gap
    table = [(0, at - 1, 1), (at + 3, 4, 1)]
    got, _ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got] == [I, V]


def test_bad_range_and_arguments(torch, eng):
    import uvhttp_amd as U
    data = b"hello w\xc3\xb6rld!!"
    n = len(data)
    table = [(0, 5, 1), (5, 6, 1), (n - 2, 10, 2), (n - 2, 10, 1), (1 << 62, 1 << 63, 1)]
    got, summ = _check_generic(torch, eng, data, table)
    assert [s for s, _ in got] == [R.VALID, R.VALID, R.NOT_TEXT, R.BAD_RANGE, R.BAD_RANGE]
    assert summ == {"n_text": 4, "n_invalid": 2, "first_invalid": 3, "open_verdict": 0}
    # data_len cuts the data short of the allocation: nothing past it is judged as in range
    got, summ = _check_generic(torch, eng, data, [(0, 5, 1), (5, 6, 1)], data_len=9)
    assert [s for s, _ in got] == [R.VALID, R.BAD_RANGE]
    # an empty table
    got, summ = _generic(torch, eng, data, [])
    assert got == [] and summ == {"n_text": 0, "n_invalid": 0, "first_invalid": 0xFFFFFFFF, "open_verdict": 0}
    d, m = _dev(torch, data), _table(torch, table)
    with pytest.raises(U.GpuError):
        eng.validate_utf8(d, m, 2, n_msgs=3)       # n_msgs > max_msgs
    with pytest.raises(U.GpuError):
        eng.validate_utf8(d[1:], m, 3, n_msgs=3)   # data not 16-byte aligned
    with pytest.raises(U.GpuError):
        eng.validate_utf8(d, m[4:], 3, n_msgs=3)   # table not 8-byte aligned


# ---- after a real compact decode ----------------------------------------------------------

CH = {1: b"x", 2: "é".encode(), 3: "€".encode(), 4: "\U0001F600".encode()}
P = 200           # payload bytes of every data frame: a fixed stride of 208
STRIDE = P + 8
TAILS = [(b"", (R.PREFIX, 0)), (b"\xc3", (R.PREFIX, 1)), (b"\xe2\x82", (R.PREFIX, 2)),
         (b"\xf0\x9f\x98", (R.PREFIX, 3)), (b"\xed\xa0", (R.INVALID, 0))]


def _fill(rng, b, upto):
    while len(b) < upto:
        b += CH[min(upto - len(b), rng.choice((1, 1, 2, 3, 4)))]


def _fragmented(rng, cuts):
    """3 * P bytes of valid text; a 4-byte character straddles offset P with cuts[0] bytes
    before it and offset 2 P with cuts[1] bytes before it -> the three fragments' payloads"""
    b = bytearray()
    _fill(rng, b, P - cuts[0])
    b += CH[4]
    _fill(rng, b, 2 * P - cuts[1])
    b += CH[4]
    _fill(rng, b, 3 * P)
    return [bytes(b[i * P:(i + 1) * P]) for i in range(3)]


def _frames_of(rng, parts, op=1, corrupt=None, ping=False):
    out = []
    for i, p in enumerate(parts):
        if corrupt == i:
            p = b"A" + p[1:]  # the fragment began inside a character
        out.append(D.Frame(op if i == 0 else 0, i == len(parts) - 1, p, key=rng.randbytes(4)))
        if ping and i == 0:
            out.append(D.Frame(9, 1, b"\xff\xfe", key=rng.randbytes(4)))
    return out


def _scenario(rng, tail, pings):
    """frames and the verdicts expected of their messages, the open one last"""
    frames, want = [], []
    for cuts in ((1, 2), (3, 1), (2, 3)):
        frames += _frames_of(rng, _fragmented(rng, cuts), ping=pings)
        want.append((R.VALID, 0))
        frames.append(D.Frame(2, 1, rng.randbytes(P), key=rng.randbytes(4)))
        want.append((R.NOT_TEXT, 0))
        frames += _frames_of(rng, _fragmented(rng, cuts), corrupt=1 + (cuts[0] & 1), ping=pings)
        want.append((R.INVALID, 0))
    one = bytearray()
    _fill(rng, one, P)
    frames.append(D.Frame(1, 1, bytes(one), key=rng.randbytes(4)))
    want.append((R.VALID, 0))
    if tail is not None:
        b = bytearray()
        _fill(rng, b, P - len(tail[0]))
        frames.append(D.Frame(1, 0, bytes(b) + tail[0], key=rng.randbytes(4)))
        want.append(tail[1])
    return frames, want


def _upload(torch, frames):
    wire = np.frombuffer(b"".join(f.bytes for f in frames), np.uint8).copy()
    d = torch.zeros(wire.size + 64, dtype=torch.uint8, device="cuda")
    d[: wire.size] = torch.from_numpy(wire).to("cuda")
    return wire, d


def _decode_kw(torch, frames, stride):
    if stride:
        assert all(len(f.bytes) == STRIDE for f in frames)
        return dict(stride=STRIDE, no_desc=True)
    offs = np.cumsum([0] + [len(f.bytes) for f in frames[:-1]]).astype(np.uint64)
    return dict(offsets=torch.from_numpy(offs.view(np.int64)).to("cuda"))


def _decode_validate(torch, eng, frames, stride):
    """decode_compact + validate_utf8 with no host sync between -> (verdicts of the judged
    entries, utf8 summary, batch summary); checked against the reference on the host copy of
    the arena and table; entries past the judged ones must be untouched"""
    n = len(frames)
    wire, d = _upload(torch, frames)
    arena = torch.zeros(wire.size + 64, dtype=torch.uint8, device="cuda")
    verdict = torch.full((n * 4,), SENT, dtype=torch.uint8, device="cuda")
    _, msgs, summ = eng.decode_compact(d, n, arena, wire_len=wire.size, max_frame_size=MF,
                                       max_message_size=0, **_decode_kw(torch, frames, stride))
    v, us = eng.validate_utf8(arena, msgs, n, batch_summary=summ, n_msgs=12345, verdict=verdict)
    torch.cuda.synchronize()
    s = eng.read_summary(summ)
    nm = s["n_messages"]
    judged = nm + (1 if s["pending_bytes"] else 0)
    m = eng.read_msgs(msgs, judged)
    table = [(int(x["arena_off"]), int(x["len"]), int(x["opcode"])) for x in m]
    ref, rsumm = R.judge(arena.cpu().numpy().tobytes(), table, open_index=nm if s["pending_bytes"] else None)
    got = [(int(x["status"]), int(x["tail"])) for x in eng.read_utf8(v, judged)]
    assert got == ref
    assert eng.read_utf8_summary(us) == rsumm
    assert (v[judged * 4:].cpu().numpy() == SENT).all()
    return got, rsumm, s


@pytest.mark.parametrize("stride", [False, True], ids=["offsets", "stride"])
@pytest.mark.parametrize("tail", [None] + TAILS, ids=["closed", "t0", "t1", "t2", "t3", "eda0"])
def test_after_compact_decode(torch, eng, tail, stride):
    """fragmented TEXT messages whose fragment boundaries cut 4-byte characters (valid only as
    one arena range), twins with a corrupted fragment, BINARY messages and PINGs in between,
    and the last message left open"""
    rng = random.Random(repr((tail, stride)))
    frames, want = _scenario(rng, tail, pings=not stride)
    got, summ, s = _decode_validate(torch, eng, frames, stride)
    assert s["n_delivered"] == len(frames) and s["status"] == 0
    assert got == want
    ov = 0 if tail is None else tail[1][0] | (tail[1][1] << 8)
    assert summ["open_verdict"] == ov
    assert summ["n_text"] == sum(1 for w in want if w[0] != R.NOT_TEXT)
    assert summ["first_invalid"] == 2


@pytest.mark.parametrize("stride", [False, True], ids=["offsets", "stride"])
@pytest.mark.parametrize("open_msg", [False, True])
def test_batch_that_fails_part_way(torch, eng, open_msg, stride):
    """an unmasked frame in the middle: exactly the messages the summary counts are judged (and
    the message open at the failure, as a prefix)"""
    rng = random.Random(repr((open_msg, stride)))
    frames, want = _scenario(rng, TAILS[2] if open_msg else None, pings=not stride)
    n_ok = len(frames)
    frames.append(D.Frame(0 if open_msg else 1, 1, b"y" * (P + 4), masked=False))
    more, _ = _scenario(rng, None, pings=not stride)
    frames += more
    got, summ, s = _decode_validate(torch, eng, frames, stride)
    assert s["n_delivered"] == n_ok and s["status"] == -1
    assert got == want
    assert summ["open_verdict"] == ((R.PREFIX | 2 << 8) if open_msg else 0)
    assert summ["n_invalid"] == 3 and summ["first_invalid"] == 2


# ---- fuzz ----------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_fuzz(torch, eng, seed):
    """2 000 messages back to back (from an odd offset): every verdict and the summary"""
    rows = R.fuzz_messages(seed)
    data, table = _pack(rows, start=1 + 5 * seed)
    assert len(data) < 4 * 1024 * 1024
    got, summ = _check_generic(torch, eng, data, table)
    text = [b for op, b in rows if op == 1]
    share = sum(not R.is_valid(b) for b in text) / len(text)
    assert 0.2 <= share <= 0.6
    assert summ["n_text"] == len(text) + 1
    assert summ["n_invalid"] == sum(not R.is_valid(b) for b in text)


# ---- graphs and streams --------------------------------------------------------------------

def _two_wires(rng):
    """two batches of the same shape: all valid, and one with a single invalid message"""
    frames, _ = _scenario(rng, TAILS[1], pings=False)
    good = [f for f in frames]
    keep, k = [], 0
    # drop the corrupted twins (3 frames each, after every BINARY frame) from the valid wire
    while k < len(good):
        if good[k].op == 2:
            keep.append(good[k])
            k += 4
        else:
            keep.append(good[k])
            k += 1
    valid = keep
    invalid = list(valid)
    victim = next(i for i, f in enumerate(invalid) if f.op == 0)
    invalid[victim] = D.Frame(0, invalid[victim].fin, b"\x80" + invalid[victim].payload[1:],
                              key=b"\x05\x06\x07\x08")
    return valid, invalid


def test_graph_replay(torch, eng):
    """decode_compact + validate_utf8 captured on a side stream, replayed over two wires: the
    verdicts follow the wire"""
    rng = random.Random(77)
    valid, invalid = _two_wires(rng)
    n = len(valid)
    wires = [np.frombuffer(b"".join(f.bytes for f in fr), np.uint8).copy() for fr in (valid, invalid)]
    assert wires[0].size == wires[1].size == n * STRIDE
    d = torch.zeros(wires[0].size + 64, dtype=torch.uint8, device="cuda")
    arena = torch.zeros(wires[0].size + 64, dtype=torch.uint8, device="cuda")
    msgs = torch.zeros(n * eng.MSG_BYTES, dtype=torch.uint8, device="cuda")
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    verdict = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    us = torch.zeros(16, dtype=torch.uint8, device="cuda")
    kw = dict(stride=STRIDE, max_frame_size=MF, max_message_size=0, wire_len=wires[0].size,
              msgs=msgs, summary=summ, no_desc=True)
    eng.reserve(n, wires[0].size + 64, wires[0].size + 64)
    d[: wires[0].size] = torch.from_numpy(wires[0]).to("cuda")
    eng.decode_compact(d, n, arena, **kw)  # one uncaptured call of the shape
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        eng.decode_compact(d, n, arena, stream=cs, **kw)
        eng.validate_utf8(arena, msgs, n, batch_summary=summ, verdict=verdict, summary=us, stream=cs)
    seen = []
    for w in (wires[0], wires[1], wires[0], wires[1]):
        d[: w.size] = torch.from_numpy(w).to("cuda")
        verdict.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        s = eng.read_summary(summ)
        nm = s["n_messages"]
        assert s["n_delivered"] == n and s["pending_bytes"]
        m = eng.read_msgs(msgs, nm + 1)
        table = [(int(x["arena_off"]), int(x["len"]), int(x["opcode"])) for x in m]
        ref, rsumm = R.judge(arena.cpu().numpy().tobytes(), table, open_index=nm)
        got = [(int(x["status"]), int(x["tail"])) for x in eng.read_utf8(verdict, nm + 1)]
        assert got == ref and eng.read_utf8_summary(us) == rsumm
        seen.append(rsumm["n_invalid"])
    assert seen == [0, 1, 0, 1]


def test_decode_and_validate_on_two_streams(torch, eng):
    """decode on stream A, validate on stream B, no explicit sync between: the engine's stream
    hand-over orders them"""
    rng = random.Random(5)
    # large enough that the decode is still running when the validate call is made
    frames = []
    for _ in range(60):
        fr, _ = _scenario(rng, None, pings=False)
        frames += fr
    tail_frames, _ = _scenario(rng, TAILS[3], pings=False)
    frames += tail_frames
    n = len(frames)
    wire, d = _upload(torch, frames)
    arena = torch.zeros(wire.size + 64, dtype=torch.uint8, device="cuda")
    msgs = torch.zeros(n * eng.MSG_BYTES, dtype=torch.uint8, device="cuda")
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    verdict = torch.full((n * 4,), SENT, dtype=torch.uint8, device="cuda")
    us = torch.zeros(16, dtype=torch.uint8, device="cuda")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        eng.decode_compact(d, n, arena, stride=STRIDE, wire_len=wire.size, max_frame_size=MF,
                           max_message_size=0, msgs=msgs, summary=summ, no_desc=True, stream=sa)
        eng.validate_utf8(arena, msgs, n, batch_summary=summ, verdict=verdict, summary=us, stream=sb)
        sb.synchronize()
        s = eng.read_summary(summ)
        nm = s["n_messages"]
        assert s["n_delivered"] == n and s["pending_bytes"]
        m = eng.read_msgs(msgs, nm + 1)
        table = [(int(x["arena_off"]), int(x["len"]), int(x["opcode"])) for x in m]
        ref, rsumm = R.judge(arena.cpu().numpy().tobytes(), table, open_index=nm)
        got = [(int(x["status"]), int(x["tail"])) for x in eng.read_utf8(verdict, nm + 1)]
        assert got == ref and eng.read_utf8_summary(us) == rsumm
        assert rsumm["open_verdict"] == (R.PREFIX | 3 << 8) and rsumm["n_invalid"] == 183
        arena.zero_()
        verdict.fill_(SENT)
        torch.cuda.synchronize()
