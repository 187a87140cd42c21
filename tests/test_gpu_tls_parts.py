"""uvhttp_tls_gpu_seal_parts (include/uvhttp_tls_amd.h): several frame tables and runs per send,
sealed as one numbered, contiguous send per connection, against the Python reference over the CPU
oracle (tests/_tls_parts_ref.py) and against the device's own seal_frames over the same frames
copied back to back on the host.  Every case compares the bytes of out (and that nothing else of
out was written), the per-send results, the summary and the record table."""
import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
import _tls_parts_ref as P
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
    """rows of (seq, key); first_frame / n_frames hold rubbish the call must ignore"""
    s = np.zeros(len(rows), R.TLS_SEND_DT)
    for i, (seq, key) in enumerate(rows):
        s[i] = (seq, 0xDEAD0000 + i, 0xFFFFFFFF - i, key, 23, 0, 0)
    return s


def _mixed_keys(rng, n):
    return np.concatenate([R.make_key(rng, R.KEY_KINDS[i % 6]) for i in range(n)])


def _table(rng, sizes):
    """frames of the given sizes back to back -> (bytes, offsets)"""
    return rng.randbytes(sum(sizes)), np.cumsum([0] + list(sizes)).astype(np.uint64)


def _arena(rng, tables, gaps=None):
    """the tables' bytes in one buffer with gaps (unaligned bases) -> (bytes, bases)"""
    buf, bases = bytearray(), []
    for k, (b, _) in enumerate(tables):
        buf += bytes([0xEE]) * (gaps[k] if gaps else rng.choice([0, 1, 3, 7, 13]))
        bases.append(len(buf))
        buf += b
    return bytes(buf) + bytes([0xEE]) * 5, bases


def _dev_parts(torch, parts, strides=None):
    """device tables of the parts: runs at stride 8, or inside rows of strides[k] bytes"""
    rows, keep = [], []
    for k, p in enumerate(parts):
        stride = strides[k] if strides else 8
        n = len(p["runs"])
        tab = np.full((max(1, n), stride // 4), 0x7E7E7E7E, np.uint32)
        tab[:n, 0:2] = p["runs"]
        d_off, d_runs = _dev(torch, p["off"]), _dev(torch, tab)
        keep += [d_off, d_runs]
        rows.append((p["base"], p["len"], d_off, d_runs, stride, len(p["off"]) - 1))
    return rows, keep


def _run(torch, eng, arena, parts, sends, keys, max_fragment=0, max_records=None, out_cap=None,
         strides=None, against_seal_frames=True):
    """one seal_parts call checked against the reference (and the device's seal_frames over the
    reference's concatenated frames) -> ref"""
    ref = P.seal_parts_ref(arena, parts, sends, keys, max_fragment)
    exact = max_records is None and out_cap is None
    max_records = len(ref["records"]) if max_records is None else max_records
    out_cap = len(ref["out"]) if out_cap is None else out_cap
    if not exact:
        ref = P.seal_parts_ref(arena, parts, sends, keys, max_fragment, max_records, out_cap)
    d_arena = _dev(torch, np.frombuffer(arena, np.uint8))
    d_sends, d_keys = _dev(torch, sends), _dev(torch, keys)
    rows, keep = _dev_parts(torch, parts, strides)
    out = torch.full((out_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    recs = torch.full(((max_records + 1) * 32,), FILL, dtype=torch.uint8, device="cuda")
    res_t = torch.full((len(sends) * 48 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    sum_t = torch.full((32 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    eng.seal_parts(d_arena, rows, d_sends, len(sends), d_keys, len(keys), max_records, out[:out_cap],
                   max_fragment=max_fragment, records=recs, results=res_t, summary=sum_t,
                   frames_len=len(arena))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    n = len(ref["out"])
    assert got[:n].tobytes() == ref["out"]
    assert (got[n:] == FILL).all(), "out written outside the sends' records"
    res_h, sum_h = res_t.cpu().numpy(), sum_t.cpu().numpy()
    res = res_h[:len(sends) * 48].view(R.TLS_SEND_RESULT_DT)
    assert res.tobytes() == ref["results"].tobytes(), (res, ref["results"])
    assert sum_h[:32].view(R.TLS_SEND_SUMMARY_DT).tobytes() == ref["summary"].tobytes()
    assert (res_h[len(sends) * 48:] == FILL).all() and (sum_h[32:] == FILL).all()
    table = recs.cpu().numpy()
    k = len(ref["records"])
    assert table[:k * 32].tobytes() == ref["records"].tobytes()
    assert (table[k * 32:] == FILL).all(), "record table written past the call's records"
    for r, piece in zip(res, ref["per_send"]):  # each send is one contiguous write
        assert got[int(r["out_off"]):int(r["out_off"] + r["out_len"])].tobytes() == piece
    if against_seal_frames:
        out2 = torch.full((out_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        _, res2, sum2 = eng.seal_frames(_dev(torch, np.frombuffer(ref["cat"], np.uint8)), _dev(torch, ref["cat_off"]),
                                        len(ref["cat_off"]) - 1, _dev(torch, ref["cat_sends"]), len(sends), d_keys,
                                        len(keys), max_records, out2[:out_cap], max_fragment=max_fragment,
                                        frames_len=len(ref["cat"]))
        torch.cuda.synchronize()
        assert torch.equal(out2, out)
        assert res2.cpu().numpy()[:len(sends) * 48].tobytes() == res.tobytes()
        assert sum2.cpu().numpy()[:32].tobytes() == sum_h[:32].tobytes()
    del keep
    return ref


def _random_batch(rng, n_sends, n_parts, mf, max_run=3, n_keys=7):
    sizes = [0, 1, mf - 1, mf, mf + 1, 2 * mf]
    tables = []
    for _ in range(n_parts):
        nf = rng.randint(1, max(2, min(2 * n_sends, 40)))
        tables.append(_table(rng, [rng.choice(sizes) for _ in range(nf)]))
    arena, bases = _arena(rng, tables)
    parts = []
    for (b, off), base in zip(tables, bases):
        nf = len(off) - 1
        runs = []
        for _ in range(n_sends):
            n = rng.randint(0, min(max_run, nf))
            runs.append((rng.randint(0, nf - n), n))
        parts.append(P.part(base, len(b), off, runs))
    sends = _sends([(rng.choice([0, (1 << 32) - 2, rng.getrandbits(62)]), rng.randrange(n_keys))
                    for _ in range(n_sends)])
    return arena, parts, sends


@pytest.mark.parametrize("n_parts", [1, 2, 3, 8])
@pytest.mark.parametrize("n_sends", [1, 255, 256, 257, 513])
def test_sends_and_parts(torch, eng, n_sends, n_parts):
    rng = random.Random(1000 * n_parts + n_sends)
    keys = _mixed_keys(rng, 7)
    arena, parts, sends = _random_batch(rng, n_sends, n_parts, 16, max_run=2 if n_parts == 8 else 3)
    ref = _run(torch, eng, arena, parts, sends, keys, 16)
    assert ref["summary"][0]["n_failed"] == 0 and (n_sends == 1 or len(ref["records"]) > 0)


def test_tables_cross_scan_blocks(torch, eng):
    """tables of 255, 256 and 600 frames: 256, 257 and 601 scan entries, so one, two and three
    workgroups of the frame scan, each part's prefix starting again at 0; one send takes every
    frame, the others runs that straddle the block edges; and one frame of 313 records"""
    rng = random.Random(33)
    tables = [_table(rng, [rng.choice([0, 1, 15, 16, 17, 40]) for _ in range(n)]) for n in (255, 256, 600)]
    tables.append(_table(rng, [5000, 100]))
    arena, bases = _arena(rng, tables)
    keys = _mixed_keys(rng, 6)
    runs = [[(0, 255), (250, 5), (0, 0), (100, 3)], [(0, 256), (254, 2), (255, 1), (0, 1)],
            [(0, 600), (255, 3), (510, 90), (599, 1)], [(0, 2), (0, 1), (1, 1), (0, 2)]]
    parts = [P.part(bases[k], len(tables[k][0]), tables[k][1], runs[k]) for k in range(4)]
    ref = _run(torch, eng, arena, parts, _sends([(9, 2), (1 << 40, 3), (5, 0), (7, 5)]), keys, 16)
    assert ref["summary"][0]["n_failed"] == 0 and ref["results"][1]["n_records"] > 313


# TLS 1.3 AES-128-GCM, TLS 1.3 ChaCha20-Poly1305, TLS 1.2 AES-128-GCM
@pytest.mark.parametrize("kind", [0, 2, 3])
@pytest.mark.parametrize("max_fragment", [1, 16, 16384])
def test_cut_edges(torch, eng, kind, max_fragment):
    """every frame size on the cut, in each of three parts; one send takes all of them, one a
    frame of each, the third starts at the sequence number whose successor carries"""
    rng = random.Random(300 + kind)
    mf = max_fragment
    sizes = [0, 1, mf - 1, mf, mf + 1, 2 * mf]
    tables = [_table(rng, sizes), _table(rng, sizes[::-1]), _table(rng, sizes[3:] + sizes[:3])]
    arena, bases = _arena(rng, tables, gaps=[1, 3, 5])
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[kind]), R.make_key(rng, R.KEY_KINDS[kind])])
    parts = [P.part(bases[k], len(tables[k][0]), tables[k][1], [(0, 6), (k, 1), (2, 3)]) for k in range(3)]
    ref = _run(torch, eng, arena, parts, _sends([(0, 0), (5, 1), ((1 << 32) - 1, 0)]), keys, mf)
    assert ref["results"][0]["n_records"] == 3 * sum((s + mf - 1) // mf for s in sizes)
    assert int(ref["records"]["plain_len"].max()) == mf and ref["summary"][0]["n_failed"] == 0
    assert int(ref["records"]["seq"].max()) > 1 << 32
    # a record never holds bytes of two frames: it lies inside one frame of one part
    spans = [(bases[k] + int(a), bases[k] + int(b)) for k in range(3)
             for a, b in zip(tables[k][1][:-1], tables[k][1][1:])]
    for q in ref["records"]:
        a, b = int(q["src_off"]), int(q["src_off"]) + int(q["plain_len"])
        assert any(lo <= a and b <= hi for lo, hi in spans)


@pytest.mark.parametrize("kind", range(6))
def test_one_part_is_seal_frames_byte_for_byte(torch, eng, kind):
    """n_parts = 1 at base 0: out, records, results and summary are seal_frames' own"""
    rng = random.Random(400 + kind)
    frames, off = R.build_frames([rng.randbytes(n) for n in (0, 1, 125, 126, 510, 600, 20000)])
    keys = _mixed_keys(rng, 6)
    runs = [(0, 7), (2, 3), (7, 0), (6, 1), (0, 0)]
    sends = _sends([(rng.getrandbits(40), (kind + i) % 6) for i in range(len(runs))])
    ref = _run(torch, eng, frames, [P.part(0, len(frames), off, runs)], sends, keys, 512, strides=[32])
    sf = np.array(sends)
    sf["first_frame"], sf["n_frames"] = [r[0] for r in runs], [r[1] for r in runs]
    out = torch.full((len(ref["out"]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    recs, res, summ = eng.seal_frames(_dev(torch, np.frombuffer(frames, np.uint8)), _dev(torch, off), 7, _dev(torch, sf),
                                      len(runs), _dev(torch, keys), 6, len(ref["records"]), out[:len(ref["out"])],
                                      max_fragment=512)
    torch.cuda.synchronize()
    assert out.cpu().numpy()[:len(ref["out"])].tobytes() == ref["out"]
    assert recs.cpu().numpy()[:len(ref["records"]) * 32].tobytes() == ref["records"].tobytes()
    assert res.cpu().numpy()[:len(runs) * 48].tobytes() == ref["results"].tobytes()
    assert summ.cpu().numpy()[:32].tobytes() == ref["summary"].tobytes()


@pytest.mark.parametrize("empty", ["first", "middle", "last", "all"])
def test_empty_runs(torch, eng, empty):
    rng = random.Random(51)
    tables = [_table(rng, [30, 0, 17, 100]) for _ in range(3)]
    arena, bases = _arena(rng, tables)
    keys = _mixed_keys(rng, 6)
    which = {"first": [0], "middle": [1], "last": [2], "all": [0, 1, 2]}[empty]
    parts = []
    for k in range(3):
        # an empty run at the start, in the middle and at the very end of the table
        runs = [(0, 0), (2, 0), (4, 0)] if k in which else [(0, 4), (1, 2), (3, 1)]
        parts.append(P.part(bases[k], len(tables[k][0]), tables[k][1], runs))
    ref = _run(torch, eng, arena, parts, _sends([(1, 0), (2, 3), (3, 5)]), keys, 16)
    assert list(ref["results"]["status"]) == [0, 0, 0]
    if empty == "all":
        assert ref["out"] == b"" and list(ref["results"]["next_seq"]) == [1, 2, 3]
    else:
        assert int(ref["results"][0]["plain_len"]) == 2 * 147


def test_same_table_twice_around_an_excluded_frame(torch, eng):
    """relay without the sender: the room's table is part 0 with the frames before the receiver's
    own and part 1 with those after; then a table of the receiver's own (the replies)"""
    rng = random.Random(61)
    room, room_off = R.build_frames([rng.randbytes(rng.choice([5, 130, 400])) for _ in range(9)])
    own, own_off = R.build_frames([rng.randbytes(3) for _ in range(4)])
    arena, bases = _arena(rng, [(room, room_off), (own, own_off)], gaps=[5, 3])
    keys = _mixed_keys(rng, 9)
    # receiver i sent frame i of the room
    before = [(0, i) for i in range(9)]
    after = [(i + 1, 8 - i) for i in range(9)]
    mine = [(i % 4, 1) for i in range(9)]
    parts = [P.part(bases[0], len(room), room_off, before), P.part(bases[0], len(room), room_off, after),
             P.part(bases[1], len(own), own_off, mine)]
    ref = _run(torch, eng, arena, parts, _sends([(100 * i, i) for i in range(9)]), keys, 128)
    for i in range(9):
        want = room[:int(room_off[i])] + room[int(room_off[i + 1]):] + own[int(own_off[i % 4]):int(own_off[i % 4 + 1])]
        assert ref["plain"][i] == want
        wire = np.frombuffer(ref["per_send"][i], np.uint8)
        plain = np.zeros(wire.size, np.uint8)
        n = O.tls_open_stream_bytes(keys[i:i + 1], 100 * i, wire, plain)
        assert plain[:n].tobytes() == want


def test_overlapping_broadcast_runs_with_distinct_keys(torch, eng):
    rng = random.Random(62)
    t0, t1 = _table(rng, [100, 20000, 0, 3000]), _table(rng, [17, 16384])
    arena, bases = _arena(rng, [t0, t1])
    n = 24
    keys = _mixed_keys(rng, n)
    # the two parts overlap in the arena as well: part 2 is part 0's range again
    parts = [P.part(bases[0], len(t0[0]), t0[1], [(i % 3, 2) for i in range(n)]),
             P.part(bases[1], len(t1[0]), t1[1], [(0, 2)] * n),
             P.part(bases[0], len(t0[0]), t0[1], [(0, 4)] * n)]
    ref = _run(torch, eng, arena, parts, _sends([(1000 * i + 3, i) for i in range(n)]), keys)
    assert len(set(ref["per_send"])) == n and len({p for p in ref["plain"]}) == 3


def test_failures(torch, eng):
    rng = random.Random(71)
    t0, t1 = _table(rng, [10, 300]), _table(rng, [20, 40, 60, 5])
    arena, bases = _arena(rng, [t0, t1])
    keys = _mixed_keys(rng, 6)
    keys[1]["key_len"] = 24  # invalid
    bad = t1[1].copy()
    bad[2] = bad[1] - 1      # frame 1 of the last part ends before it begins
    sends = _sends([(1, 0), (2, 1), (3, 9), (4, 0), (5, 2), (6, 3), (7, 4), (8, 5)])
    runs0 = [(0, 2), (0, 3), (0, 2), (0, 2), (0, 1), (2, 0), (3, 0), (1, 1)]
    runs1 = [(0, 1), (0, 9), (0, 1), (3, 2), (1, 1), (2, 2), (0, 1), (3, 1)]
    parts = [P.part(bases[0], len(t0[0]), t0[1], runs0), P.part(bases[1], len(t1[0]), bad, runs1)]
    ref = _run(torch, eng, arena, parts, sends, keys, 128)
    # 1: invalid key and a bad range -> the key; 2: slot past the table; 3: range, raised by the
    # last part alone; 4: the bad frame; 5: a frame after the bad one is good (offsets rise again);
    # 6: first_frame past the table of part 0, with n = 0
    assert list(ref["results"]["status"]) == [0, O.REC_KEY, O.REC_KEY, R.REC_RANGE, R.REC_RANGE, 0, R.REC_RANGE, 0]
    assert ref["summary"][0]["n_failed"] == 5
    assert list(ref["results"]["next_seq"][[1, 2, 3, 4, 6]]) == [2, 3, 4, 5, 7]
    # the last part's len one short of its last frame: only the sends that name that frame fail
    short = [P.part(bases[0], len(t0[0]), t0[1], [(0, 2)] * 3),
             P.part(bases[1], len(t1[0]) - 1, t1[1], [(0, 3), (3, 1), (4, 0)])]
    ref = _run(torch, eng, arena, short, _sends([(1, 0), (2, 2), (3, 3)]), keys, 128)
    assert list(ref["results"]["status"]) == [0, R.REC_RANGE, 0]


@pytest.mark.parametrize("short", ["out_cap", "max_records"])
def test_capacity(torch, eng, short):
    rng = random.Random(72)
    arena, parts, sends = _random_batch(rng, 9, 3, 64, n_keys=6)
    keys = _mixed_keys(rng, 6)
    sends[4]["key"] = 77
    full = P.seal_parts_ref(arena, parts, sends, keys, 64)
    cap = dict(out_cap=len(full["out"]) - 1) if short == "out_cap" else dict(max_records=len(full["records"]) - 1)
    ref = _run(torch, eng, arena, parts, sends, keys, 64, **cap)  # out stays 0xA5 throughout
    want = [O.REC_CAPACITY] * 9
    want[4] = O.REC_KEY
    assert list(ref["results"]["status"]) == want
    assert ref["out"] == b"" and ref["summary"][0]["n_failed"] == 9
    assert ref["summary"].tobytes()[:12] == full["summary"].tobytes()[:12]
    s = ref["summary"][0]
    again = _run(torch, eng, arena, parts, sends, keys, 64, max_records=int(s["n_records"]), out_cap=int(s["out_bytes"]))
    assert again["out"] == full["out"] and again["summary"][0]["n_failed"] == 1


def test_empty_call_and_every_einval(torch, eng):
    import uvhttp_amd as U
    rng = random.Random(73)
    t0 = _table(rng, [10, 300])
    arena = t0[0] + b"\0" * 8
    keys = _mixed_keys(rng, 6)
    d = {"arena": _dev(torch, np.frombuffer(arena, np.uint8)), "off": _dev(torch, t0[1]),
         "runs": _dev(torch, np.array([[0, 2]], np.uint32)), "keys": _dev(torch, keys),
         "sends": _dev(torch, _sends([(1, 0)]))}
    out = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    summ = torch.full((32,), FILL, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(48, dtype=torch.uint8, device="cuda")
    good = (0, len(t0[0]), d["off"], d["runs"], 8, 2)
    # n_sends = 0: OK, summary zeroed, nothing written
    eng.seal_parts(d["arena"], [good], d["sends"], 0, d["keys"], 6, 16, out, records=recs, results=res, summary=summ)
    torch.cuda.synchronize()
    assert not summ.any() and (out == FILL).all()
    L = U.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(parts=(good,), n_parts=None, frames=p(d["arena"]), frames_len=len(arena), sends=p(d["sends"]),
             keys_=p(d["keys"]), mf=0, recs_=p(recs), max_records=16, res_=p(res), summ_=p(summ), out_=p(out),
             n_sends=1):
        tab = (U.TlsPart * 9)()
        for k, (base, ln, off, runs, stride, n) in enumerate(parts):
            tab[k] = U.TlsPart(base, ln, off.data_ptr() if off is not None else None,
                               runs.data_ptr() if runs is not None else None, stride, n)
        return L.uvhttp_tls_gpu_seal_parts(eng.h, frames, frames_len, tab, len(parts) if n_parts is None else n_parts,
                                           sends, n_sends, keys_, 6, mf, recs_, max_records, res_, summ_, out_, 4096, st)
    assert call() == 0
    assert call(parts=(good,) * 8) == 0
    assert call(n_parts=0) == -1 and call(parts=(good,) * 9) == -1
    assert call(parts=((1, len(arena), d["off"], d["runs"], 8, 2),)) == -1       # base + len > frames_len
    assert call(parts=((len(arena) + 1, 0, d["off"], d["runs"], 8, 2),)) == -1
    assert call(parts=((0, 1 << 63, d["off"], d["runs"], 8, 2),)) == -1
    assert call(parts=((0, 10, None, d["runs"], 8, 2),)) == -1
    assert call(parts=((0, 10, d["off"], None, 8, 2),)) == -1
    for stride in (0, 4, 10, 7):
        assert call(parts=((0, 10, d["off"], d["runs"], stride, 2),)) == -1, stride
    assert call(mf=16385) == -1
    for name in ("frames", "sends", "keys_", "recs_", "res_", "summ_", "out_"):
        assert call(**{name: None}) == -1, name
    assert call(n_sends=(1 << 26) + 1) == -1 and call(max_records=(1 << 28) + 1) == -1
    assert call(parts=((0, 10, d["off"], d["runs"], 8, 1 << 27),) * 3) == -1     # 2^28 frames over all parts
    assert call() == 0
    torch.cuda.synchronize()


def test_captured_graph_over_two_arenas(torch, eng):
    """one capture, replayed over the bytes, offsets, runs and sequence numbers of two batches of
    the same shape: the call reads everything on the device"""
    rng = random.Random(81)
    keys = _mixed_keys(rng, 6)
    n_sends, nf, mf = 40, 12, 64
    batches = []
    for _ in range(2):
        tables = [_table(rng, [rng.choice([0, 1, 63, 64, 65, 128]) for _ in range(nf)]) for _ in range(3)]
        span = 2 * 128 * nf
        arena = b"".join(b.ljust(span, b"\xEE") for b, _ in tables)
        parts = []
        for k, (b, off) in enumerate(tables):
            runs = []
            for _ in range(n_sends):
                n = rng.randint(0, 3)
                runs.append((rng.randint(0, nf - n), n))
            parts.append(P.part(k * span, span, off, runs))
        sends = _sends([(rng.getrandbits(48), rng.randrange(6)) for _ in range(n_sends)])
        batches.append((arena, parts, sends, P.seal_parts_ref(arena, parts, sends, keys, mf)))
    max_records = max(len(b[3]["records"]) for b in batches) + 3
    out_cap = max(len(b[3]["out"]) for b in batches) + 40
    d_arena = torch.zeros(3 * 2 * 128 * nf, dtype=torch.uint8, device="cuda")
    d_sends, d_keys = _dev(torch, batches[0][2]), _dev(torch, keys)
    rows, keep = _dev_parts(torch, batches[0][1])
    out = torch.zeros(out_cap + GUARD, dtype=torch.uint8, device="cuda")
    recs = torch.zeros((max_records + 1) * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n_sends * 48, dtype=torch.uint8, device="cuda")
    summ = torch.zeros(32, dtype=torch.uint8, device="cuda")

    def call(stream):
        eng.seal_parts(d_arena, rows, d_sends, n_sends, d_keys, 6, max_records, out[:out_cap], max_fragment=mf,
                       records=recs, results=res, summary=summ, stream=stream)
    cs = torch.cuda.Stream()
    with torch.cuda.stream(cs):
        call(cs)  # (the engine's scratch grows here, not in the capture)
    cs.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        call(cs)
    for arena, parts, sends, ref in (batches[0], batches[1], batches[0]):
        d_arena.copy_(torch.from_numpy(np.frombuffer(arena, np.uint8).copy()))
        d_sends.copy_(torch.from_numpy(sends.view(np.uint8).copy()))
        for k, p in enumerate(parts):
            keep[2 * k].copy_(torch.from_numpy(p["off"].view(np.uint8).copy()))
            keep[2 * k + 1].copy_(torch.from_numpy(np.ascontiguousarray(p["runs"]).view(np.uint8).reshape(-1).copy()))
        out.fill_(FILL)
        recs.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        n = len(ref["out"])
        assert got[:n].tobytes() == ref["out"] and (got[n:] == FILL).all()
        assert res.cpu().numpy().tobytes() == ref["results"].tobytes()
        assert summ.cpu().numpy().tobytes() == ref["summary"].tobytes()
        k = len(ref["records"])
        table = recs.cpu().numpy()
        assert table[:k * 32].tobytes() == ref["records"].tobytes() and (table[k * 32:] == FILL).all()


@pytest.mark.parametrize("seed", range(4))
def test_fuzz(torch, eng, seed):
    """50 batches per case, 200 in all: random parts, runs, keys and failures of every kind"""
    rng = random.Random(900 + seed)
    keys = _mixed_keys(rng, 12)
    keys[5]["key_len"] = 24
    keys[11]["version"] = 0x0302
    failed = 0
    for _ in range(50):
        mf = rng.choice([1, 7, 16, 64, 16384])
        n_parts, n_sends = rng.randint(1, 8), rng.randint(1, 12)
        small = [0, 1, 2, 5] if mf == 1 else [0, 1, mf - 1, mf, mf + 1, 2 * mf] if mf <= 64 else [0, 1, 300, 16383, 16385]
        tables = [_table(rng, [rng.choice(small) for _ in range(rng.randint(0, 6))]) for _ in range(n_parts)]
        arena, bases = _arena(rng, tables)
        parts, strides = [], []
        for (b, off), base in zip(tables, bases):
            nf = len(off) - 1
            off = off.copy()
            ln = len(b)
            x = rng.random()
            if x < 0.05 and nf >= 2:
                off[rng.randint(1, nf - 1)] = int(off[nf]) + 1 + rng.randint(0, 3)   # a decreasing pair, and past len
            elif x < 0.10 and ln:
                ln -= 1                                                        # the last frame reaches past len
            runs = []
            for _ in range(n_sends):
                n = rng.randint(0, min(3, nf))
                first = rng.randint(0, nf - n)
                if rng.random() < 0.03:
                    first = nf - n + rng.randint(1, 3)
                runs.append((first, n))
            parts.append(P.part(base, ln, off, runs))
            strides.append(rng.choice([8, 12, 32]))
        rows = []
        for _ in range(n_sends):
            key = rng.choice([k for k in range(12) if k not in (5, 11)])
            x = rng.random()
            if x < 0.03:
                key = rng.choice([5, 11])
            elif x < 0.06:
                key = rng.choice([12, 70000, 0xFFFFFFFF])
            rows.append((rng.choice([0, (1 << 32) - 2, rng.getrandbits(63)]), key))
        ref = _run(torch, eng, arena, parts, _sends(rows), keys, mf, strides=strides, against_seal_frames=False)
        failed += int(ref["summary"][0]["n_failed"])
    assert failed > 0
