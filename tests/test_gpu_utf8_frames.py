"""uvhttp_ws_gpu_validate_utf8_streams / _inplace on the device after a real decode_streams /
decode_reads / decode_inplace: device == the Python walk of tests/_utf8_frames_ref.py (CPython's
strict decoder) == the host twin uvhttp_ws_utf8_judge_frames, for every connection of every
case."""
import random

import numpy as np
import pytest

import _oracle as O
import _utf8_frames_ref as FR
import _utf8_ref as R

pytestmark = pytest.mark.gpu
SCAN_BLOCK = 256  # descriptors per workgroup of the carry scan (utf8_frames_gpu.hip: kBlock)
KNOWN = ([bytes.fromhex(h) for h in R.KNOWN_VALID] + [bytes.fromhex(h) for h in R.KNOWN_INVALID] +
         [bytes.fromhex(h) for h, _ in R.KNOWN_TRUNCATED])


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


def _states(pends):
    st = np.zeros((len(pends), 4), np.uint8)
    for s, p in enumerate(pends):
        st[s, :len(p)] = list(p)
        st[s, 3] = len(p)
    return st


def _state_struct(pend):
    import uvhttp_amd as U
    st = U.Utf8State()
    st.n = len(pend)
    for k, b in enumerate(pend):
        st.pend[k] = b
    return st


def run_streams(torch, eng, conns, pending=None, pends=None, flags=0, gap=0, lead=0, read_end=None,
                spare=3, expect_nd=None):
    """decode_streams (decode_reads with read_end) then validate_utf8_streams, no host sync
    between; every connection's verdict and the summary against the reference and the host
    twin -> (verdicts, summary, stream results)"""
    import uvhttp_amd as U
    S = len(conns)
    wire, st = FR.streams_of(conns, pending, gap, lead)
    re_dev = None
    if read_end is not None:
        re_dev = torch.tensor(list(read_end[1]), dtype=torch.int64, device="cuda")
        for s, (fr, nr) in enumerate(read_end[0]):
            st[s]["first_read"], st[s]["n_reads"] = fr, nr
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    max_frames = sum(len(c) for c in conns) + spare
    state_in = _dev(torch, _states(pends), 0) if pends is not None else None
    desc, res = eng.decode_streams(dw, dst, S, max_frames, wire_len=wire.size, read_end=re_dev)
    v, sm = eng.validate_utf8_streams(dw, desc, max_frames, dst, res, S, state_in=state_in, flags=flags,
                                      wire_len=wire.size)
    torch.cuda.synchronize()
    results = eng.read_stream_results(res, S)
    _, _, _, nd, _ = FR.oracle_decode(wire, st, None if read_end is None else np.array(read_end[1], np.uint64))
    assert [r.n_delivered for r in results] == nd
    if expect_nd is not None:
        assert nd == expect_nd
    got = eng.read_utf8_conn_verdicts(v, S)
    hw, hd = dw[: wire.size].cpu().numpy(), eng.read_desc(desc, max_frames)
    want, host = [], []
    for s in range(S):
        pop = pending[s][0] if pending and pending[s] and pending[s][1] else 0
        pend = bytes(pends[s]) if pends is not None else b""
        ff = results[s].first_frame
        want.append(FR.judge(conns[s][:nd[s]], first_frame=ff if nd[s] else 0, open_opcode=pop, pend=pend,
                             flags=flags))
        host.append(U.utf8_judge_frames(hw, hd, ff, nd[s], pop, _state_struct(pend), flags))
    bad = [(s, got[s], want[s], host[s]) for s in range(S) if not (got[s] == want[s] == host[s])]
    assert not bad, bad[:4]
    summ = eng.read_utf8_frames_summary(sm)
    assert summ == FR.summary(want)
    return got, summ, results


def _cut_cases():
    conns = []
    for b in KNOWN:
        for cut in range(1, len(b) + 1):
            conns.append(FR.fragments(b, [cut]))
            conns.append(FR.fragments(b, [cut])[:-1] + [FR.Fr(0, 0, b[cut:])])  # left open
        for a in range(1, len(b) + 1):
            for z in range(a, len(b) + 1):
                conns.append(FR.fragments(b, [a, a, z, z], between=(FR.PING(),)))
        if len(b) >= 2:
            conns.append(FR.fragments(b, list(range(1, len(b)))))
    conns.append([FR.Fr(1, 0, b"\xe2\x82"), FR.Fr(0, 1, b"\xac"), FR.Fr(2, 1, b"\xff\xfe"),
                  FR.Fr(1, 0, b"a\xe2"), FR.PING(), FR.Fr(0, 1, b"\x82\xac")])
    conns.append([FR.Fr(1, 0, b"ab\xe2"), FR.PING(), FR.Fr(0, 0, b""), FR.Fr(0, 1, b"")])
    return conns


@pytest.mark.parametrize("phase", range(16))
def test_fragment_cuts_every_phase(torch, eng, phase):
    """the known answers cut at every byte, at every pair of bytes with empty fragments and
    PINGs between, and into one-byte fragments: one connection each, the first payload at
    byte phase `phase` of a 16-byte vector"""
    conns = _cut_cases()
    got, summ, _ = run_streams(torch, eng, conns, lead=(phase - 6) % 16)
    assert got[-1]["status"] == R.INVALID
    assert got[-2]["status"] == R.VALID and summ["n_invalid_conns"] > 50 and summ["n_open_conns"] > 10


@pytest.mark.parametrize("edge", [16, 4096, 16384])
def test_character_cut_on_tile_edges(torch, eng, edge):
    """F0 9F 98 80 cut by a fragment boundary after 1, 2 and 3 bytes, with the first fragment's
    payload ending on the edge and with the second fragment's payload starting on it; the
    invalid twin ends in 41"""
    for split in (1, 2, 3):
        for on_edge in ("end", "start"):
            for last in (b"\x80", b"\x41"):
                ch = b"\xf0\x9f\x98" + last
                fill = b"a" * (edge + 40)
                a, b = FR.Fr(1, 0, fill + ch[:split]), FR.Fr(0, 1, ch[split:] + fill)
                rel = len(a.bytes) if on_edge == "end" else len(a.bytes) + len(b.bytes) - len(b.payload)
                lead = (edge - rel) % 16384
                assert (lead + rel) % edge == 0
                got, _, _ = run_streams(torch, eng, [[a, b]], lead=lead)
                assert got[0]["status"] == (R.VALID if last == b"\x80" else R.INVALID)
                assert got[0]["first_invalid"] == (FR.NONE if last == b"\x80" else 1)


def test_connection_boundaries(torch, eng):
    """A ends with an open F0 9F 98; B, directly behind it in the wire, starts with 80"""
    a = [FR.Fr(1, 0, b"tail \xf0\x9f\x98")]
    got, _, _ = run_streams(torch, eng, [a, [FR.Fr(1, 1, b"\x80 head")], a, [FR.Fr(2, 1, b"\x80 head")]])
    assert [g["status"] for g in got] == [R.PREFIX, R.INVALID, R.PREFIX, R.VALID]
    assert got[0]["state"] == (b"\xf0\x9f\x98", 3) and got[1]["first_invalid"] == 1


@pytest.mark.parametrize("corrupt", [False, True])
def test_carry_across_scan_blocks(torch, eng, corrupt):
    """2 x (scan block) + 1 one-byte TEXT fragments spelling 4-byte characters"""
    n = 2 * SCAN_BLOCK + 1
    text = bytearray(b"!" + ("\U0001F600" * (n // 4)).encode())
    assert len(text) == n
    if corrupt:
        text[n - 1] = 0x41  # the one frame of the last block: judged against three carried bytes
    got, _, _ = run_streams(torch, eng, [FR.fragments(bytes(text), list(range(1, n)))])
    assert got[0]["n_text_frames"] == n
    assert got[0]["status"] == (R.INVALID if corrupt else R.VALID)
    assert got[0]["first_invalid"] == (n - 1 if corrupt else FR.NONE)


def test_segment_heads_everywhere_in_a_block(torch, eng):
    rng = random.Random(3)
    conns = []
    for s in range(300):
        ch = rng.choice(["é", "€", "\U0001F600"]).encode()
        k = rng.randint(1, len(ch))
        bad = s % 7 == 3
        conns.append([FR.Fr(1, 0, b"x" * (s % 5) + ch[:k]), FR.PING(),
                      FR.Fr(0, s % 2, (ch[k:] if not bad else b"\xc0") + b"y" * (s % 3))])
    got, summ, _ = run_streams(torch, eng, conns)
    assert summ["n_text_frames"] == 600 and summ["first_invalid_conn"] == 3


def test_long_run_of_empty_fragments_and_pings(torch, eng):
    mid = []
    for k in range(200):
        mid.append(FR.Fr(0, 0, b"") if k % 2 else FR.PING())
    got, _, _ = run_streams(torch, eng, [[FR.Fr(1, 0, b"\xe2\x82")] + mid + [FR.Fr(0, 1, b"\xac")],
                                         [FR.Fr(1, 0, b"\xe2\x82")] + mid + [FR.Fr(0, 1, b"\x2c")]])
    assert got[0]["status"] == R.VALID and got[0]["n_text_frames"] == 102
    assert got[1]["status"] == R.INVALID and got[1]["first_invalid"] == 202 + 201


def test_connection_that_fails_part_way(torch, eng):
    ok = [FR.Fr(1, 0, b"fine \xf0\x9f"), FR.Fr(0, 1, b"\x98\x80")]
    failing = [FR.Fr(1, 0, b"so far \xe2\x82"), FR.Fr(0, 0, b"\xac", rsv=True), FR.Fr(0, 1, b"\xff\xff\xff\xff"),
               FR.Fr(1, 1, b"\x80\x80\x80\x80\x80\x80")]
    got, summ, res = run_streams(torch, eng, [ok, failing, ok], expect_nd=[2, 1, 2])
    assert res[1].status != 0
    assert [g["status"] for g in got] == [R.VALID, R.PREFIX, R.VALID]
    assert got[1]["state"] == (b"\xe2\x82", 2) and summ["n_text_frames"] == 5


def test_capacity_overflow_judges_nothing(torch, eng):
    conns = [[FR.Fr(1, 1, b"\xff")] * 4, [FR.Fr(1, 1, b"\x80")] * 4]
    wire, st = FR.streams_of(conns)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 2, 5, wire_len=wire.size)
    v, sm = eng.validate_utf8_streams(dw, desc, 5, dst, res, 2, wire_len=wire.size)
    torch.cuda.synchronize()
    assert all(r.first_status == -10 for r in eng.read_stream_results(res, 2))
    none = {"first_invalid": FR.NONE, "n_text_frames": 0, "state": (b"", 0), "status": R.VALID}
    assert eng.read_utf8_conn_verdicts(v, 2) == [none, none]
    assert eng.read_utf8_frames_summary(sm) == FR.summary([none, none])


TAILS = [b"", b"\xc2", b"\xe2\x82", b"\xf0\x9f\x98", b"\xed\xa0"]


def test_message_open_across_two_decode_calls(torch, eng):
    """call 1 leaves a TEXT (or BINARY) message open with each tail; call 2 gets the first
    result's pending_bytes, the opcode and the first verdict's state, and must say what one
    call over all the frames says"""
    rest = [b"\x80", b"\xac", b"\x98\x80", b"\x80\x80", b"a"]
    first, second, ops = [], [], []
    for op in (1, 2):
        for t in TAILS:
            for r in rest:
                first.append([FR.Fr(1, 1, b"one"), FR.Fr(op, 0, b"open " + t), FR.PING()])
                second.append([FR.PING(), FR.Fr(0, 0, r[:1]), FR.Fr(0, 1, r[1:] + b" end"), FR.Fr(1, 1, b"\xc3\xa9")])
                ops.append(op)
    S = len(first)
    got1, _, res1 = run_streams(torch, eng, first)
    assert all(r.pending_bytes == 5 + len(TAILS[(s // len(rest)) % len(TAILS)]) for s, r in enumerate(res1))
    pending = [(ops[s], int(res1[s].pending_bytes)) for s in range(S)]
    pends = [g["state"][0] for g in got1]
    got2, _, _ = run_streams(torch, eng, second, pending=pending, pends=pends)
    whole, _, resw = run_streams(torch, eng, [a + b for a, b in zip(first, second)])
    n_inv = 0
    for s in range(S):
        if got1[s]["status"] == R.INVALID:  # ED A0: the server closes after call 1
            assert whole[s]["status"] == R.INVALID
            assert whole[s]["first_invalid"] - resw[s].first_frame == got1[s]["first_invalid"] - res1[s].first_frame == 1
            assert ops[s] == 1 and TAILS[(s // len(rest)) % len(TAILS)] == b"\xed\xa0"
            continue
        assert got2[s]["status"] == whole[s]["status"], s
        assert got2[s]["n_text_frames"] + got1[s]["n_text_frames"] == whole[s]["n_text_frames"]
        assert (got2[s]["first_invalid"] == FR.NONE) == (whole[s]["first_invalid"] == FR.NONE)
        n_inv += whole[s]["status"] == R.INVALID
    assert 5 < n_inv < S - 5


def test_decode_reads_with_boundaries_inside_characters(torch, eng):
    text = "grüße, 世界 \U0001F600\U0001F601 end".encode()
    conns = [FR.fragments(text, [9, 15, 21]), FR.fragments(text[:-6] + b"\xff" + text[-5:], [9, 15, 21])]
    lens = [sum(len(f.bytes) for f in c) for c in conns]
    table, reads = [], []
    for s, ln in enumerate(lens):
        ends = sorted({e for e in (7, 12, 19, 23, 31, 40, ln - 3, ln) if 0 < e <= ln})
        table.append((len(reads), len(ends)))
        reads += ends
    got, _, _ = run_streams(torch, eng, conns, read_end=(table, reads), expect_nd=[4, 4])
    assert got[0]["status"] == R.VALID and got[1]["status"] == R.INVALID and got[1]["first_invalid"] == 4 + 3


@pytest.mark.parametrize("corrupt", [False, True])
def test_more_than_64_segments_in_a_wave_share(torch, eng, corrupt):
    """600 eight-byte TEXT frames: about 290 segments per 4 KiB, the payload pass's per-lane
    search; the error sits past the frame's third byte, where only that pass looks"""
    frames = [FR.Fr(1, 1, "ab€é1".encode()) for _ in range(600)]
    if corrupt:
        frames[417] = FR.Fr(1, 1, b"abc\xe2\x28\xa1zz")
        frames[599] = FR.Fr(1, 1, b"abcdefg\xc3")
    got, _, _ = run_streams(torch, eng, [frames[:300], frames[300:]])
    assert got[0]["status"] == R.VALID
    assert got[1]["first_invalid"] == (417 if corrupt else FR.NONE)


def test_bad_range(torch, eng):
    """the validation's wire_len cut short of the decode's: TEXT frames past it are BAD_RANGE
    (an INVALID frame before them wins), BINARY frames past it are nobody's business"""
    import uvhttp_amd as U
    conns = [[FR.Fr(1, 1, b"one"), FR.Fr(1, 0, b"two \xe2"), FR.Fr(0, 1, b"\x82\xac")],
             [FR.Fr(1, 1, b"\x80ne"), FR.Fr(1, 1, b"fine")],
             [FR.Fr(1, 1, b"ok"), FR.Fr(2, 1, b"\xff" * 40)],
             [FR.Fr(1, 1, b"last one, cut"), FR.Fr(8, 1, b"\x03\xe8bye")]]
    wire, st = FR.streams_of(conns)
    S, mf = len(conns), sum(len(c) for c in conns)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, S, mf, wire_len=wire.size)
    torch.cuda.synchronize()
    hd = eng.read_desc(desc, mf)
    ends = [int(x["payload_off"] + x["payload_len"]) for x in hd]
    hw = dw[: wire.size].cpu().numpy()
    seen = set()
    for wl in (wire.size, ends[-1] - 1, ends[-2] - 1, ends[6] - 1, ends[4] + 3, ends[3] - 1, ends[2] - 1, ends[1] - 2, 1, 0):
        v, sm = eng.validate_utf8_streams(dw, desc, mf, dst, res, S, flags=FR.CHECK_CLOSE, wire_len=wl)
        torch.cuda.synchronize()
        got = eng.read_utf8_conn_verdicts(v, S)
        results = eng.read_stream_results(res, S)
        for s, r in enumerate(results):
            bad = {i for i in range(r.n_delivered) if ends[r.first_frame + i] > wl}
            want = FR.judge(conns[s], first_frame=r.first_frame, flags=FR.CHECK_CLOSE, bad_range=bad)
            host = U.utf8_judge_frames(hw, hd, r.first_frame, r.n_delivered, 0, None, FR.CHECK_CLOSE, wire_len=wl)
            assert got[s] == want == host, (wl, s, got[s], want, host)
            seen.add((s, got[s]["status"]))
    assert {(0, R.VALID), (0, R.BAD_RANGE), (1, R.INVALID), (2, R.VALID), (2, R.BAD_RANGE), (3, R.BAD_RANGE)} <= seen


# ---- in place ------------------------------------------------------------------------------

def run_inplace(torch, eng, frames, stride=None, flags=0):
    """decode_inplace (offsets, or a fixed stride) then validate_utf8_inplace -> verdict"""
    import uvhttp_amd as U
    n = len(frames)
    wire = np.frombuffer(b"".join(f.bytes for f in frames), np.uint8).copy()
    dw = _dev(torch, wire)
    if stride:
        assert all(len(f.bytes) == stride for f in frames)
        kw = dict(stride=stride)
        ref = O.decode_batch(wire, n, stride=stride, max_frame_size=FR.MF, max_message_size=FR.MM)
    else:
        offs = np.cumsum([0] + [len(f.bytes) for f in frames[:-1]]).astype(np.uint64)
        kw = dict(offsets=torch.from_numpy(offs.view(np.int64)).to("cuda"))
        ref = O.decode_batch(wire, n, offsets=offs, max_frame_size=FR.MF, max_message_size=FR.MM)
    desc, summ = eng.decode_inplace(dw, n, wire_len=wire.size, max_frame_size=FR.MF, max_message_size=FR.MM, **kw)
    v, sm = eng.validate_utf8_inplace(dw, desc, n, summ, flags=flags, wire_len=wire.size)
    torch.cuda.synchronize()
    nd = ref["summary"]["n_delivered"]
    assert eng.read_summary(summ)["n_delivered"] == nd
    got = eng.read_utf8_conn_verdicts(v, 1)[0]
    want = FR.judge(frames[:nd], flags=flags)
    host = U.utf8_judge_frames(dw[: wire.size].cpu().numpy(), eng.read_desc(desc, n), 0, nd, 0, None, flags)
    assert got == want == host, (got, want, host)
    assert eng.read_utf8_frames_summary(sm) == FR.summary([want])
    return got, nd


def _inplace_frames(rng, n_msgs, bad_at=None, fail_at=None):
    frames = []
    for m in range(n_msgs):
        text = "".join(rng.choice("aé€\U0001F600 ") for _ in range(rng.randint(1, 40))).encode()
        if m == bad_at:
            text = text[: len(text) // 2] + b"\xc0" + text[len(text) // 2:]
        cuts = sorted(rng.randint(1, len(text)) for _ in range(rng.randint(0, 3)))
        frames += FR.fragments(text, cuts, op=1 if m % 4 else 2 if m % 8 else 1, between=(FR.PING(),) if m % 3 == 0 else ())
        if m == fail_at:
            frames.append(FR.Fr(1, 1, b"\xff\xff", rsv=True))
    return frames


@pytest.mark.parametrize("bad_at", [None, 17])
def test_inplace_offsets(torch, eng, bad_at):
    frames = _inplace_frames(random.Random(11), 40, bad_at=bad_at)
    got, nd = run_inplace(torch, eng, frames)
    assert nd == len(frames) and got["status"] == (R.VALID if bad_at is None else R.INVALID)


def test_inplace_batch_that_fails_part_way(torch, eng):
    frames = _inplace_frames(random.Random(12), 30, bad_at=25, fail_at=20)
    got, nd = run_inplace(torch, eng, frames)
    assert nd < len(frames) and got["status"] == R.VALID
    # the failure inside an open message: PREFIX with what the delivered frames left open
    frames = [FR.Fr(1, 0, b"abc\xf0\x9f"), FR.Fr(0, 0, b"\x98"), FR.Fr(1, 1, b"data inside a message fails"),
              FR.Fr(0, 1, b"\xff")]
    got, nd = run_inplace(torch, eng, frames)
    assert nd == 2 and got["status"] == R.PREFIX and got["state"] == (b"\xf0\x9f\x98", 3)


@pytest.mark.parametrize("mode", ["valid", "invalid", "open"])
def test_inplace_fixed_stride_fused_path(torch, eng, mode):
    """200-byte payloads (stride 208 >= 140: the fused small-frame decode), every message four
    fragments cut inside 4-byte characters"""
    P, n_msgs = 200, 24
    frames = []
    for m in range(n_msgs):
        e = "\U0001F600"  # the fragment boundaries cut a character after 1, 2 and 3 bytes
        body = bytearray((e * 49 + "abc" + e + e * 48 + "abc" + e + e * 48 + "abc" + e + e * 49 + "abc").encode())
        assert len(body) == 4 * P
        if mode == "invalid" and m == 13:
            body[2 * P + 1] = 0x20
        fr = FR.fragments(bytes(body), [P, 2 * P, 3 * P], op=1 if m % 5 else 2)
        if mode == "open" and m == n_msgs - 1:
            fr = fr[:2]
        frames += fr
    got, nd = run_inplace(torch, eng, frames, stride=P + 8)
    assert nd == len(frames)
    assert got["status"] == {"valid": R.VALID, "invalid": R.INVALID, "open": R.PREFIX}[mode]
    if mode == "invalid":
        assert got["first_invalid"] == 13 * 4 + 2
    if mode == "open":
        assert got["state"] == (b"\xf0\x9f", 2)


def test_inplace_64k_frame(torch, eng):
    body = ("\U0001F600" * (16 * 1024)).encode()
    assert len(body) == 65536
    for bad_at in (None, 3, 40000, 65535):
        b = bytearray(body)
        if bad_at is not None:
            b[bad_at] = 0x41
        got, _ = run_inplace(torch, eng, [FR.Fr(1, 1, b"a"), FR.Fr(1, 1, bytes(b)), FR.Fr(1, 1, b"z")])
        assert got["first_invalid"] == (FR.NONE if bad_at is None else 1)


# ---- CLOSE reasons, fuzz, arguments, graphs, streams ------------------------------------------

@pytest.mark.parametrize("flags", [0, FR.CHECK_CLOSE])
def test_close_reasons(torch, eng, flags):
    def close(reason):
        return FR.Fr(8, 1, (1000).to_bytes(2, "big") + reason)
    conns = [[FR.Fr(1, 1, b"hi"), FR.PING(), close(r)] for r in (b"bye \xe2\x82\xac", b"\xc0\x80", b"bye \xe2\x82", b"")]
    conns.append([FR.Fr(1, 0, b"open \xe2"), close(b"\x82\xac")])  # the reason is its own message
    got, summ, _ = run_streams(torch, eng, conns, flags=flags)
    inv = [g["status"] == R.INVALID for g in got]
    assert inv == ([False, True, True, False, True] if flags else [False] * 5)
    assert got[4]["status"] == (R.INVALID if flags else R.PREFIX)
    got, _ = run_inplace(torch, eng, conns[1], flags=flags)
    assert got["first_invalid"] == (2 if flags else FR.NONE)


@pytest.mark.parametrize("seed", range(4))
def test_fuzz(torch, eng, seed):
    """the fuzz corpus, every message cut into 1-5 fragments, PINGs sprinkled in, dealt over 64
    connections: every connection's verdict"""
    rng = random.Random(100 + seed)
    rows = R.fuzz_messages(seed)
    frames = [FR.fragment_randomly(rng, [row]) for row in rows]
    conns = [[] for _ in range(64)]
    # a connection stays interesting while it is valid: deal the invalid messages late
    order = sorted(range(len(rows)), key=lambda k: (rows[k][0] == 1 and not R.is_valid(rows[k][1]), k))
    for j, k in enumerate(order):
        conns[j % 64] += frames[k]
    got, summ, res = run_streams(torch, eng, conns, gap=seed * 5)
    assert summ["n_invalid_conns"] == 64 and summ["n_text_frames"] > 3000
    assert min(g["first_invalid"] - r.first_frame for g, r in zip(got, res)) > 30


def test_arguments(torch, eng):
    import uvhttp_amd as U
    conns = [[FR.Fr(1, 1, b"ok")]]
    wire, st = FR.streams_of(conns)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 1, 4, wire_len=wire.size)
    v = torch.zeros(64, dtype=torch.uint8, device="cuda")
    sm = torch.zeros(64, dtype=torch.uint8, device="cuda")
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.validate_utf8_streams(dw, desc, 4, dst, res, 1, verdict=v, summary=sm, wire_len=wire.size)

    class Null:
        def data_ptr(self):
            return None

    def streams(**kw):
        a = dict(wire=dw, desc=desc, streams_dev=dst, results=res, verdict=v, summary=sm)
        a.update(kw)
        eng.validate_utf8_streams(a["wire"], a["desc"], 4, a["streams_dev"], a["results"], 1, verdict=a["verdict"],
                                  summary=a["summary"], state_in=a.get("state_in"), wire_len=wire.size)

    def inplace(**kw):
        a = dict(wire=dw, desc=desc, batch_summary=summ, verdict=v, summary=sm)
        a.update(kw)
        eng.validate_utf8_inplace(a["wire"], a["desc"], 1, a["batch_summary"], verdict=a["verdict"],
                                  summary=a["summary"], wire_len=wire.size)

    inplace()
    for call, names in ((streams, ["wire", "desc", "streams_dev", "results", "verdict", "summary"]),
                        (inplace, ["wire", "desc", "batch_summary", "verdict", "summary"])):
        for name in names:
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**{name: Null()})
            base = dict(wire=dw, desc=desc, streams_dev=dst, results=res, verdict=v, summary=sm, batch_summary=summ)
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**{name: base[name][1:]})
    with pytest.raises(U.GpuError, match="rc=-1"):
        streams(state_in=v[1:])
    torch.cuda.synchronize()


def _graph_wires(rng):
    conns = [FR.fragment_randomly(rng, [(1, ("héllo €uro \U0001F600 " * 6).encode())] * 3) for _ in range(8)]
    bad = [list(c) for c in conns]
    victim = next(i for i, f in enumerate(bad[5]) if f.op == 0 and len(f.payload) > 4)
    f = bad[5][victim]
    bad[5][victim] = FR.Fr(0, f.fin, f.payload[:3] + b"\xff" * 2 + f.payload[5:])
    return conns, bad


def test_graph_replay(torch, eng):
    """decode_streams + validate_utf8_streams captured on a side stream after one uncaptured
    call of the shape, replayed over two wires: the verdicts follow the wire"""
    rng = random.Random(9)
    good, bad = _graph_wires(rng)
    (w0, st), (w1, st1) = FR.streams_of(good), FR.streams_of(bad)
    assert w0.size == w1.size and (st == st1).all()
    S, mf = len(good), sum(len(c) for c in good) + 2
    dw, dst = _dev(torch, w0), _dev(torch, st, 0)
    desc = torch.zeros(mf * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
    v = torch.zeros(S * 16, dtype=torch.uint8, device="cuda")
    sm = torch.zeros(16, dtype=torch.uint8, device="cuda")

    def both(stream=None):
        eng.decode_streams(dw, dst, S, mf, desc=desc, results=res, wire_len=w0.size, stream=stream)
        eng.validate_utf8_streams(dw, desc, mf, dst, res, S, verdict=v, summary=sm, wire_len=w0.size, stream=stream)

    both()
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        both(cs)
    seen = []
    for w, conns in ((w0, good), (w1, bad), (w0, good), (w1, bad)):
        dw[: w.size] = torch.from_numpy(w).to("cuda")
        v.fill_(0xEE)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        results = eng.read_stream_results(res, S)
        want = [FR.judge(c, first_frame=r.first_frame) for c, r in zip(conns, results)]
        assert eng.read_utf8_conn_verdicts(v, S) == want
        assert eng.read_utf8_frames_summary(sm) == FR.summary(want)
        seen.append(FR.summary(want)["first_invalid_conn"])
    assert seen == [FR.NONE, 5, FR.NONE, 5]


def test_decode_and_validate_on_two_streams(torch, eng):
    """decode on stream A, validate on stream B, no explicit sync between: the engine's stream
    hand-over orders them"""
    rng = random.Random(21)
    text = ("ünïcödé €€€ \U0001F600\U0001F601 " * 40).encode()
    conns = [FR.fragment_randomly(rng, [(1, text)] * 6 + [(1, text[:-2] if s % 3 == 0 else text)]) for s in range(256)]
    wire, st = FR.streams_of(conns)
    S, mf = len(conns), sum(len(c) for c in conns)
    dw0, dst = _dev(torch, wire), _dev(torch, st, 0)
    dw = dw0.clone()
    desc = torch.zeros(mf * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
    v = torch.zeros(S * 16, dtype=torch.uint8, device="cuda")
    sm = torch.zeros(16, dtype=torch.uint8, device="cuda")
    want = None
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        eng.decode_streams(dw, dst, S, mf, desc=desc, results=res, wire_len=wire.size, stream=sa)
        eng.validate_utf8_streams(dw, desc, mf, dst, res, S, verdict=v, summary=sm, wire_len=wire.size, stream=sb)
        sb.synchronize()
        if want is None:
            want = [FR.judge(c, first_frame=r.first_frame) for c, r in zip(conns, eng.read_stream_results(res, S))]
        assert eng.read_utf8_conn_verdicts(v, S) == want
        assert eng.read_utf8_frames_summary(sm) == FR.summary(want)
        assert FR.summary(want)["n_invalid_conns"] == 86
        dw.copy_(dw0)
        v.fill_(0xEE)
        torch.cuda.synchronize()
