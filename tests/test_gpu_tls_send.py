"""uvhttp_tls_gpu_seal_frames (include/uvhttp_tls_amd.h): built WebSocket frames -> sealed TLS
records of many connections in one device call, against the Python reference over the CPU
oracle (tests/_tls_send_ref.py).  Every case compares the bytes of out (and that nothing else
of out was written), the per-send results, the summary and the record table."""
import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
import _tls_send_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def eng(torch):
    import uvhttp_amd as U
    e = U.TlsEngine(0)
    yield e
    e.close()


def _dev(torch, a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if not a.size:
        return torch.zeros(64, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.copy()).to("cuda")


def _sends(rows):
    """rows of (seq, first_frame, n_frames, key)"""
    s = np.zeros(len(rows), R.TLS_SEND_DT)
    for i, (seq, ff, n, key) in enumerate(rows):
        s[i] = (seq, ff, n, key, 23, 0, 0)
    return s


def _run(torch, eng, frames, off, sends, keys, max_fragment=0, max_records=None, out_cap=None,
         frames_len=None):
    """one seal_frames call checked against the reference -> (ref, device tensors)"""
    ref = R.seal_frames_ref(frames, off, sends, keys, max_fragment, frames_len=frames_len)
    exact = max_records is None and out_cap is None  # the buffers hold exactly what is needed
    max_records = len(ref["records"]) if max_records is None else max_records
    out_cap = len(ref["out"]) if out_cap is None else out_cap
    if not exact:
        ref = R.seal_frames_ref(frames, off, sends, keys, max_fragment, max_records, out_cap,
                                frames_len=frames_len)
    d_frames = _dev(torch, np.frombuffer(frames, np.uint8))
    out = torch.full((out_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    recs = torch.full(((max_records + 1) * 32,), FILL, dtype=torch.uint8, device="cuda")
    recs_t, res_t, sum_t = eng.seal_frames(
        d_frames, _dev(torch, off), len(off) - 1, _dev(torch, sends), len(sends),
        _dev(torch, keys), len(keys), max_records, out[:out_cap], max_fragment=max_fragment,
        records=recs, frames_len=len(frames) if frames_len is None else frames_len)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    n = len(ref["out"])
    assert got[:n].tobytes() == ref["out"]
    assert (got[n:] == FILL).all(), "out written outside the sends' records"
    res = res_t.cpu().numpy()[:len(sends) * 48].view(R.TLS_SEND_RESULT_DT)
    assert res.tobytes() == ref["results"].tobytes(), (res, ref["results"])
    assert sum_t.cpu().numpy().view(R.TLS_SEND_SUMMARY_DT).tobytes() == ref["summary"].tobytes()
    table = recs_t.cpu().numpy()
    k = len(ref["records"])
    assert table[:k * 32].tobytes() == ref["records"].tobytes()
    assert (table[k * 32:] == FILL).all(), "record table written past the call's records"
    for r, piece in zip(res, ref["per_send"]):  # each send is one contiguous write
        assert got[int(r["out_off"]):int(r["out_off"] + r["out_len"])].tobytes() == piece
    return ref, (d_frames, recs_t, out)


def _edge_case(rng, kind, mf):
    """frames whose sizes sit on the cut, and one per header form; two sends over all of them,
    the second from the sequence number whose successor carries into the high nonce word"""
    totals = [mf - 1, mf, mf + 1, 2 * mf, 2 * mf + 1]
    plens = [R.payload_len_for(t) for t in totals] + [125, 126, 65535, 65536]
    frames, off = R.build_frames([rng.randbytes(p) for p in plens])
    assert [int(off[i + 1] - off[i]) for i in range(5)] == totals
    keys = R.make_key(rng, R.KEY_KINDS[kind])
    return frames, off, _sends([(0, 0, len(plens), 0), ((1 << 32) - 1, 0, len(plens), 0)]), keys


@pytest.mark.parametrize("kind", range(6))
@pytest.mark.parametrize("max_fragment", [16384, 512])
def test_cut_edges(torch, eng, kind, max_fragment):
    rng = random.Random(1000 + kind)
    frames, off, sends, keys = _edge_case(rng, kind, max_fragment)
    ref, _ = _run(torch, eng, frames, off, sends, keys, max_fragment)
    assert int(ref["records"]["seq"].max()) > 1 << 32
    sizes = ref["records"]["plain_len"]
    assert sizes.max() == max_fragment and {max_fragment - 1, 1} <= set(sizes.tolist())


@pytest.mark.parametrize("kind", range(6))
def test_record_table_feeds_seal_records(torch, eng, kind):
    """records[] as seal_frames wrote it, handed to uvhttp_tls_gpu_seal_records: the same bytes"""
    rng = random.Random(1000 + kind)
    frames, off, sends, keys = _edge_case(rng, kind, 512)
    ref, (d_frames, recs, out) = _run(torch, eng, frames, off, sends, keys, 512)
    n = len(ref["records"])
    again = torch.full((len(ref["out"]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    eng.seal_records(d_frames, recs, n, _dev(torch, keys), len(keys), again[:len(ref["out"])])
    torch.cuda.synchronize()
    assert torch.equal(again, out)
    assert again[:len(ref["out"])].cpu().numpy().tobytes() == ref["out"]


def _mixed_keys(rng, n):
    return np.concatenate([R.make_key(rng, R.KEY_KINDS[i % 6]) for i in range(n)])


def test_many_sends_cross_scan_blocks(torch, eng):
    rng = random.Random(21)
    n = 2 * 256 + 1
    frames, off = R.build_frames([rng.randbytes(rng.choice([0, 1, 40, 125, 126])) for _ in range(n)])
    keys = _mixed_keys(rng, 7)
    _run(torch, eng, frames, off, _sends([(rng.getrandbits(40), i, 1, i % 7) for i in range(n)]), keys)


def test_one_send_of_many_frames(torch, eng):
    rng = random.Random(22)
    n = 2 * 256 + 1
    frames, off = R.build_frames([rng.randbytes(rng.choice([0, 1, 40, 125, 126, 700])) for _ in range(n)])
    keys = _mixed_keys(rng, 6)
    for kind in (0, 5):
        _run(torch, eng, frames, off, _sends([(5, 0, n, kind)]), keys, 512)


def test_one_frame_of_many_records(torch, eng):
    """a 5 000-byte frame at max_fragment 16 is more records than a scan block; the send after
    it starts in a later block of the record search"""
    rng = random.Random(23)
    frames, off = R.build_frames([rng.randbytes(R.payload_len_for(5000)), rng.randbytes(100)])
    keys = _mixed_keys(rng, 6)
    ref, _ = _run(torch, eng, frames, off, _sends([(9, 0, 1, 2), (1 << 40, 0, 2, 3)]), keys, 16)
    assert ref["results"][0]["n_records"] == 313 and ref["results"][1]["first_record"] == 313


def test_broadcast(torch, eng):
    """one range of two built frames to 300 connections, each with its own key and sequence"""
    rng = random.Random(31)
    frames, off = R.build_frames([rng.randbytes(R.payload_len_for(300)),
                                  rng.randbytes(R.payload_len_for(20000))])
    n = 300
    keys = _mixed_keys(rng, n)
    sends = _sends([(1000 * i + 3, 0, 2, i) for i in range(n)])
    ref, _ = _run(torch, eng, frames, off, sends, keys)
    for i in range(n):  # every connection's bytes open to the same plaintext
        wire = np.frombuffer(ref["per_send"][i], np.uint8)
        plain = np.zeros(wire.size, np.uint8)
        got = O.tls_open_stream_bytes(keys[i:i + 1], int(sends[i]["seq"]), wire, plain)
        assert plain[:got].tobytes() == frames
    assert len(set(ref["per_send"])) == n


def test_overlapping_ranges(torch, eng):
    rng = random.Random(32)
    frames, off = R.build_frames([rng.randbytes(n) for n in (100, 20000, 0, 3000, 17000)])
    keys = _mixed_keys(rng, 6)
    _run(torch, eng, frames, off, _sends([(1, 0, 3, 0), (2, 1, 4, 4), (3, 1, 1, 0)]), keys)


def _failure_base(rng):
    frames, off = R.build_frames([rng.randbytes(n) for n in (10, 300, 700, 20, 40)])
    keys = _mixed_keys(rng, 6)
    return frames, off, keys


@pytest.mark.parametrize("case", ["bad_slot", "invalid_key", "slot_65536", "range", "decreasing",
                                  "past_frames"])
def test_a_failed_send_between_two_good_ones(torch, eng, case):
    rng = random.Random(41)
    frames, off, keys = _failure_base(rng)
    frames_len, bad = None, (7, 1, 2, 1)
    if case == "bad_slot":
        bad = (7, 1, 2, len(keys))
    elif case == "invalid_key":
        keys[1]["key_len"] = 24
    elif case == "slot_65536":
        keys = np.concatenate([keys, np.zeros(65536 - len(keys), O.TLS_KEY_DT),
                               R.make_key(rng, R.KEY_KINDS[0])])
        bad = (7, 1, 2, 65536)
    elif case == "range":
        bad = (7, 3, 3, 1)
    elif case == "decreasing":
        off = off.copy()
        off[3] = off[2] - 1  # frame 2 ends before it begins; frames 0, 1 and 4 stay good
        bad = (7, 2, 1, 1)
    elif case == "past_frames":
        frames_len = int(off[4]) + 1  # frame 4 reaches past the buffer
        bad = (7, 3, 2, 1)
    sends = _sends([(1, 0, 2, 0), bad, (2, 0, 2, 5)])
    if case == "decreasing":
        sends[2]["first_frame"], sends[2]["n_frames"] = 4, 1
    ref, _ = _run(torch, eng, frames, off, sends, keys, 256, frames_len=frames_len)
    want = R.REC_RANGE if case in ("range", "decreasing", "past_frames") else O.REC_KEY
    assert list(ref["results"]["status"]) == [0, want, 0] and ref["summary"][0]["n_failed"] == 1
    assert ref["results"][0]["n_records"] and ref["results"][2]["n_records"]


@pytest.mark.parametrize("short", ["out_cap", "max_records"])
def test_capacity(torch, eng, short):
    rng = random.Random(42)
    frames, off, keys = _failure_base(rng)
    sends = _sends([(1, 0, 3, 0), (5, 0, 1, 77), (2, 2, 3, 4)])
    full = R.seal_frames_ref(frames, off, sends, keys, 256)
    cap = dict(out_cap=len(full["out"]) - 1) if short == "out_cap" else \
        dict(max_records=len(full["records"]) - 1)
    ref, _ = _run(torch, eng, frames, off, sends, keys, 256, **cap)  # out stays 0xA5 throughout
    assert list(ref["results"]["status"]) == [O.REC_CAPACITY, O.REC_KEY, O.REC_CAPACITY]
    assert ref["out"] == b"" and ref["summary"][0]["n_failed"] == 3
    assert ref["summary"].tobytes()[:12] == full["summary"].tobytes()[:12]
    # a second call sized from the summary succeeds
    s = ref["summary"][0]
    again, _ = _run(torch, eng, frames, off, sends, keys, 256, max_records=int(s["n_records"]),
                    out_cap=int(s["out_bytes"]))
    assert again["out"] == full["out"] and list(again["results"]["status"]) == [0, O.REC_KEY, 0]


def test_empty_calls_and_arguments(torch, eng):
    import uvhttp_amd as U
    rng = random.Random(43)
    frames, off, keys = _failure_base(rng)
    # a send of no frames: no record, status 0; also at the very end of frame_off
    ref, _ = _run(torch, eng, frames, off, _sends([(1, 0, 1, 0), (9, 2, 0, 1), (9, 5, 0, 1),
                                                   (2, 4, 1, 2)]), keys, 256)
    assert list(ref["results"]["status"]) == [0, 0, 0, 0]
    assert list(ref["results"]["n_records"][1:3]) == [0, 0]
    assert list(ref["results"]["next_seq"][1:3]) == [9, 9]
    # only empty frames: no record at all
    eframes, eoff = b"", np.zeros(4, np.uint64)
    _run(torch, eng, eframes, eoff, _sends([(1, 0, 3, 0)]), keys)
    # n_sends = 0: OK, summary zeroed
    d = {k: _dev(torch, v) for k, v in (("frames", np.frombuffer(frames, np.uint8)), ("off", off),
                                        ("keys", keys), ("sends", _sends([(1, 0, 1, 0)])))}
    out = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    summ = torch.full((32,), FILL, dtype=torch.uint8, device="cuda")
    eng.seal_frames(d["frames"], d["off"], 5, d["sends"], 0, d["keys"], len(keys), 16, out,
                    summary=summ)
    torch.cuda.synchronize()
    assert not summ.any() and (out == FILL).all()
    # EINVAL
    L = U.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    recs = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(48, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(frames=p(d["frames"]), off=p(d["off"]), sends=p(d["sends"]), keys_=p(d["keys"]),
             mf=0, recs_=p(recs), res_=p(res), summ_=p(summ), out_=p(out)):
        return L.uvhttp_tls_gpu_seal_frames(eng.h, frames, len(frames_b), off, 5, sends, 1, keys_,
                                            len(keys), mf, recs_, 16, res_, summ_, out_, 4096, st)
    frames_b = frames
    assert call() == 0
    assert call(mf=16385) == -1
    for name in ("frames", "off", "sends", "keys_", "recs_", "res_", "summ_", "out_"):
        assert call(**{name: None}) == -1, name
    torch.cuda.synchronize()


def test_no_frames_no_table(torch, eng):
    """n_frames_total = 0 with frame_off = NULL (and no frames buffer): a send of no frames
    succeeds with no record, one that names a frame is out of range, a bad key slot is a key
    error; nothing of out or the record table is written although both have room"""
    import uvhttp_amd as U
    rng = random.Random(44)
    keys = _mixed_keys(rng, 6)
    sends = _sends([(3, 0, 0, 1), (4, 0, 1, 2), (5, 0, 0, len(keys))])
    ref = R.seal_frames_ref(b"", np.zeros(1, np.uint64), sends, keys)
    assert list(ref["results"]["status"]) == [0, R.REC_RANGE, O.REC_KEY]
    assert not len(ref["records"]) and ref["out"] == b""
    out_cap, max_records = 64, 4
    out = torch.full((out_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    recs = torch.full(((max_records + 1) * 32,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((len(sends) * 48,), FILL, dtype=torch.uint8, device="cuda")
    summ = torch.full((32,), FILL, dtype=torch.uint8, device="cuda")
    d_sends, d_keys = _dev(torch, sends), _dev(torch, keys)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = U.lib().uvhttp_tls_gpu_seal_frames(
        eng.h, None, 0, None, 0, p(d_sends), len(sends), p(d_keys), len(keys), 0, p(recs),
        max_records, p(res), p(summ), p(out), out_cap,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert res.cpu().numpy().view(R.TLS_SEND_RESULT_DT).tobytes() == ref["results"].tobytes()
    assert summ.cpu().numpy().view(R.TLS_SEND_SUMMARY_DT).tobytes() == ref["summary"].tobytes()
    assert (out == FILL).all() and (recs == FILL).all()


def test_cross_one_scan_block_after_growth(torch):
    """one engine of its own: a call with 3 frames, then one with 257 frames and 257 sends of one
    frame each: the scratch grows between the two, and the frame table's 258 scan entries end in
    a second workgroup that is all but empty"""
    import uvhttp_amd as U
    rng = random.Random(45)
    e = U.TlsEngine(0)
    try:
        keys = _mixed_keys(rng, 6)
        frames, off = R.build_frames([rng.randbytes(n) for n in (5, 0, 200)])
        _run(torch, e, frames, off, _sends([(1, 0, 3, 0), (2, 1, 2, 3)]), keys, 64)
        n = 256 + 1
        frames, off = R.build_frames([rng.randbytes(rng.choice([0, 1, 40, 126])) for _ in range(n)])
        _run(torch, e, frames, off, _sends([(rng.getrandbits(40), i, 1, i % 6) for i in range(n)]),
             keys, 64)
    finally:
        e.close()


def test_chain_without_host_sync(torch, eng):
    """build_frames -> seal_frames -> open_records -> ws_streams -> decode_reads on one stream,
    the descriptors between the calls made on the device, no synchronisation before the end:
    64 connections x 3 masked client messages, delivered payloads == inputs."""
    import uvhttp_amd as U
    from test_gpu_build import BUILD_DT
    t = torch
    rng = random.Random(51)
    n_conn, per = 64, 3
    sizes = [0, 1, 125, 126, 300, 4000, 16370, 16384, 20000, 40000]
    payloads = [rng.randbytes(40000 if i == 0 else rng.choice(sizes)) for i in range(n_conn * per)]
    mkeys = [rng.randbytes(4) for _ in payloads]
    src = b"".join(payloads)
    bd = np.zeros(len(payloads), BUILD_DT)
    bd["payload_off"] = np.cumsum([0] + [len(p) for p in payloads[:-1]])
    bd["payload_len"] = [len(p) for p in payloads]
    bd["key"] = [int.from_bytes(k, "little") for k in mkeys]
    bd["opcode"], bd["fin"], bd["mask"] = 2, 1, 1
    frames, off = R.build_frames(payloads, mask=1, keys=mkeys)
    keys = _mixed_keys(rng, n_conn)
    sends = _sends([(rng.getrandbits(40), per * c, per, c) for c in range(n_conn)])
    ref = R.seal_frames_ref(frames, off, sends, keys)
    n_rec, n_bytes = len(ref["records"]), len(ref["out"])

    weng = U.GpuEngine(0)
    conns = [U.WsConnection(1, 16 << 20, 64 << 20, user_data=False) for _ in range(n_conn)]
    ws = []
    for c in conns:
        s = U.Stream()
        U.lib().uvhttp_ws_stream_init(c.ptr, 0, 0, C.byref(s))
        ws.append(bytes(s))
    d_src, d_bd, d_keys, d_sends = (_dev(t, np.frombuffer(src, np.uint8)), _dev(t, bd),
                                    _dev(t, keys), _dev(t, sends))
    ws_dev = _dev(t, np.frombuffer(b"".join(ws), np.uint8))
    d_frames = t.zeros(len(frames) + 64, dtype=t.uint8, device="cuda")
    sealed = t.zeros(n_bytes + 64, dtype=t.uint8, device="cuda")
    plain = t.zeros(n_bytes + 64, dtype=t.uint8, device="cuda")
    read_end = t.zeros(n_rec + 1, dtype=t.int64, device="cuda")
    streams = t.zeros(n_conn * 4, dtype=t.int64, device="cuda")
    t.cuda.synchronize()
    st = t.cuda.Stream()
    with t.cuda.stream(st):
        d_off = weng.build_frames(d_src, d_bd, len(payloads), d_frames[:len(frames)], stream=st)
        recs, res, summ = eng.seal_frames(d_frames, d_off, len(payloads), d_sends, n_conn, d_keys,
                                          n_conn, n_rec, sealed[:n_bytes], frames_len=len(frames),
                                          stream=st)
        # uvhttp_tls_stream_t {begin, len, seq, key | ws_prefix << 32} from the send results, on
        # the device: what the peer's read side would be handed
        r64 = res.view(t.int64).view(n_conn, 6)
        s64 = streams.view(n_conn, 4)
        s64[:, 0], s64[:, 1] = r64[:, 0], r64[:, 1]
        s64[:, 2] = d_sends.view(t.int64).view(n_conn, 4)[:, 0]
        s64[:, 3] = t.arange(n_conn, dtype=t.int64, device="cuda")
        orecs, ores = eng.open_records(sealed, d_keys, n_conn, streams.view(t.uint8), n_conn, n_rec,
                                       plain[:n_bytes], wire_len=n_bytes, stream=st)
        eng.ws_streams(ores, orecs, n_conn, streams.view(t.uint8), plain, ws_dev, read_end,
                       stream=st)
        desc, wres = weng.decode_streams(plain, ws_dev, n_conn, len(payloads) + 16,
                                         wire_len=n_bytes, read_end=read_end, n_reads=n_rec,
                                         stream=st)
    st.synchronize()
    weng.sync(st)
    assert d_frames[:len(frames)].cpu().numpy().tobytes() == frames
    assert sealed[:n_bytes].cpu().numpy().tobytes() == ref["out"]
    assert res.cpu().numpy()[:n_conn * 48].view(R.TLS_SEND_RESULT_DT).tobytes() == \
        ref["results"].tobytes()
    assert summ.cpu().numpy().view(R.TLS_SEND_SUMMARY_DT).tobytes() == ref["summary"].tobytes()
    assert recs.cpu().numpy()[:n_rec * 32].tobytes() == ref["records"].tobytes()
    opened = ores.cpu().numpy().view(O.TLS_RESULT_DT)[:n_conn]
    assert (opened["status"] == 0).all() and (opened["n_delivered"] == ref["results"]["n_records"]).all()
    results = weng.read_stream_results(wres, n_conn)
    ws_host = [U.Stream.from_buffer_copy(bytes(ws_dev[k * 64:(k + 1) * 64].cpu().numpy()))
               for k in range(n_conn)]
    host_out, host_desc = plain.cpu().numpy(), desc.cpu().numpy()
    hw = (C.c_uint8 * host_out.size).from_buffer(host_out)
    hd = (C.c_uint8 * host_desc.size).from_buffer(host_desc)
    for c in range(n_conn):
        rc = U.lib().uvhttp_ws_deliver_stream(conns[c].ptr, hw, hd, C.byref(ws_host[c]),
                                              C.byref(results[c]))
        assert rc == 0, (c, results[c].as_dict())
        assert conns[c].events == [("message", 2, p) for p in payloads[per * c:per * c + per]], c

    # a build_frames whose out_cap is too small writes nothing; every send is out of range
    small = 16  # below the first frame
    with t.cuda.stream(st):
        d_off = weng.build_frames(d_src, d_bd, len(payloads), d_frames[:small], stream=st)
        sealed.fill_(FILL)
        recs, res, summ = eng.seal_frames(d_frames, d_off, len(payloads), d_sends, n_conn, d_keys,
                                          n_conn, n_rec, sealed[:n_bytes], frames_len=small,
                                          stream=st)
    st.synchronize()
    want = R.seal_frames_ref(frames, off, sends, keys, frames_len=small)
    got = res.cpu().numpy()[:n_conn * 48].view(R.TLS_SEND_RESULT_DT)
    assert (got["status"] == R.REC_RANGE).all() and got.tobytes() == want["results"].tobytes()
    assert summ.cpu().numpy().view(R.TLS_SEND_SUMMARY_DT).tobytes() == want["summary"].tobytes()
    assert (sealed == FILL).all()
    weng.close()


@pytest.mark.parametrize("seed", range(4))
def test_fuzz(torch, eng, seed):
    rng = random.Random(600 + seed)
    mf = [16, 512, 4096, 16384][seed]

    def size():
        x = rng.random()
        if x < 0.7:
            return rng.randint(0, 300)
        if x < 0.9:
            return 16384 + rng.randint(-20, 20)
        return rng.randint(301, 70000)
    n_frames = 96
    frames, off = R.build_frames([rng.randbytes(size()) for _ in range(n_frames)],
                                 mask=seed & 1, keys=[rng.randbytes(4) for _ in range(n_frames)])
    keys = _mixed_keys(rng, 24)
    order = list(range(24))
    rng.shuffle(order)
    keys = keys[order]
    keys[5]["key_len"] = 24
    keys[11]["version"] = 0x0302
    rows = []
    for _ in range(64):
        n = rng.randint(1, 8)
        ff = rng.randint(0, n_frames - n)
        key = rng.choice([k for k in range(24) if k not in (5, 11)])
        x = rng.random()
        if x < 0.03:
            key = rng.choice([5, 11])
        elif x < 0.06:
            key = rng.choice([24, 70000, 0xFFFFFFFF])
        elif x < 0.10:
            ff = n_frames - n + rng.randint(1, 3)
        rows.append((rng.choice([0, (1 << 32) - 2, rng.getrandbits(63)]), ff, n, key))
    ref, _ = _run(torch, eng, frames, off, _sends(rows), keys, mf)
    assert 0 < ref["summary"][0]["n_failed"] < 64
