"""uvhttp_tls_gpu_seal_parts_coalesced (include/uvhttp_tls_amd.h): a send's frames packed into
ceil(B / max_fragment) full records, gathered into out and sealed there in place, against the
Python reference over the CPU oracle (tests/_tls_coalesce_ref.py).  Every case compares the bytes of
out inside a guarded buffer (nothing before out, nothing past summary.out_bytes), the record table
(nothing past n_records), the per-send results and the summary; has the oracle open every send's
records to its stream; and lays the streams into a second buffer at records[].src_off, where
seal_records must reproduce out."""
import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
import _tls_coalesce_ref as K
import _tls_parts_ref as P
import _tls_send_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5
TILE = 4096  # kGatherTile (uvhttp_amd/csrc/tls_gpu.hip): record content bytes per workgroup pass


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


def _opened(keys, sends, res, out_bytes):
    """what the oracle opens from every send's bytes of out under seq, seq + 1, ..."""
    got = []
    for s, r in zip(sends, res):
        wire = np.frombuffer(out_bytes[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])], np.uint8)
        if not wire.size:
            got.append(b"")
            continue
        plain = np.zeros(wire.size + 16, np.uint8)
        n = O.tls_open_stream_bytes(keys[int(s["key"]):int(s["key"]) + 1], int(s["seq"]), wire, plain)
        got.append(plain[:n].tobytes())
    return got


def _run(torch, eng, arena, parts, sends, keys, max_fragment=0, max_records=None, out_cap=None, strides=None,
         shift=0):
    """one coalesced call checked against the reference, the oracle's open and the records[]
    contract; out begins `shift` bytes past a 256-byte boundary -> (ref, device out tensor)"""
    ref = K.seal_parts_coalesced_ref(arena, parts, sends, keys, max_fragment)
    exact = max_records is None and out_cap is None
    max_records = len(ref["records"]) if max_records is None else max_records
    out_cap = len(ref["out"]) if out_cap is None else out_cap
    if not exact:
        ref = K.seal_parts_coalesced_ref(arena, parts, sends, keys, max_fragment, max_records, out_cap)
    d_arena = _dev(torch, np.frombuffer(arena, np.uint8))
    d_sends, d_keys = _dev(torch, sends), _dev(torch, keys)
    rows, keep = _dev_parts(torch, parts, strides)
    lead = GUARD + shift
    big = torch.full((lead + out_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    out = big[lead:lead + out_cap]
    recs = torch.full(((max_records + 1) * 32,), FILL, dtype=torch.uint8, device="cuda")
    res_t = torch.full((len(sends) * 48 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    sum_t = torch.full((32 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    eng.seal_parts_coalesced(d_arena, rows, d_sends, len(sends), d_keys, len(keys), max_records, out,
                             max_fragment=max_fragment, records=recs, results=res_t, summary=sum_t,
                             frames_len=len(arena))
    torch.cuda.synchronize()
    whole = big.cpu().numpy()
    got = whole[lead:]
    n = len(ref["out"])
    assert (whole[:lead] == FILL).all(), "bytes before out written"
    assert (got[n:] == FILL).all(), "out written past the sends' records"
    assert got[:n].tobytes() == ref["out"]
    res_h, sum_h = res_t.cpu().numpy(), sum_t.cpu().numpy()
    res = res_h[:len(sends) * 48].view(R.TLS_SEND_RESULT_DT)
    assert res.tobytes() == ref["results"].tobytes(), (res, ref["results"])
    assert sum_h[:32].view(R.TLS_SEND_SUMMARY_DT).tobytes() == ref["summary"].tobytes()
    assert (res_h[len(sends) * 48:] == FILL).all() and (sum_h[32:] == FILL).all()
    table = recs.cpu().numpy()
    k = len(ref["records"])
    assert table[:k * 32].tobytes() == ref["records"].tobytes()
    assert (table[k * 32:] == FILL).all(), "record table written past the call's records"
    mf = max_fragment or 16384
    assert [int(r["n_records"]) for r in res] == [(len(p) + mf - 1) // mf for p in ref["plain"]]
    assert _opened(keys, sends, res, got[:n].tobytes()) == ref["plain"]
    if k:
        # records[] over a buffer that holds the streams at src_off is a seal_records input
        staged = np.full(n, 0x3C, np.uint8)
        for r, plain in zip(res, ref["plain"]):
            for j in range(int(r["n_records"])):
                q = ref["records"][int(r["first_record"]) + j]
                staged[int(q["src_off"]):int(q["src_off"]) + int(q["plain_len"])] = \
                    np.frombuffer(plain[j * mf:j * mf + int(q["plain_len"])], np.uint8)
        out2 = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        eng.seal_records(_dev(torch, staged), recs, k, d_keys, len(keys), out2[:n])
        torch.cuda.synchronize()
        assert out2.cpu().numpy().tobytes() == got[:n + GUARD].tobytes()
    del keep
    return ref, out


def _random_batch(rng, n_sends, n_parts, sizes, max_run=3, n_keys=7):
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


@pytest.mark.parametrize("kind", range(6))
def test_every_key_kind_against_reference_and_oracle(torch, eng, kind):
    """three parts, frames that straddle the cuts, streams of 0 to 9 records, one key kind"""
    rng = random.Random(100 + kind)
    tables = [_table(rng, [7, 0, 130, 64, 1]), _table(rng, [300, 63, 65]), _table(rng, [2, 2, 500])]
    arena, bases = _arena(rng, tables, gaps=[1, 6, 11])
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[kind]) for _ in range(3)])
    runs = [[(0, 5), (1, 3), (5, 0), (2, 1)], [(0, 3), (1, 1), (0, 0), (3, 0)], [(0, 3), (2, 1), (3, 0), (0, 2)]]
    parts = [P.part(bases[k], len(tables[k][0]), tables[k][1], runs[k]) for k in range(3)]
    ref, _ = _run(torch, eng, arena, parts, _sends([((1 << 32) - 1, 0), (5, 1), (9, 2), (1 << 50, 0)]), keys, 128,
                  shift=kind)
    assert list(ref["results"]["n_records"]) == [9, 6, 0, 2] and ref["summary"][0]["n_failed"] == 0
    assert int(ref["records"]["seq"].max()) > 1 << 50


@pytest.mark.parametrize("mf", [1, 16, 64, 4096, 16384])
def test_stream_lengths_around_the_cut(torch, eng, mf):
    """B = 0, 1, mf - 1, mf, mf + 1, 2 mf, 2 mf + 1: part 0 gives the first min(B, mf) bytes, so the
    first record boundary lies exactly on a segment boundary; part 1's first frame is min(rest, mf)
    bytes, so the second lies exactly on a frame boundary inside a segment"""
    rng = random.Random(200 + mf)
    lens = sorted({0, 1, mf - 1, mf, mf + 1, 2 * mf, 2 * mf + 1})
    assert mf > 1 or max(lens) <= 64
    s0, s1, runs0, runs1 = [], [], [], []
    for b in lens:
        first = min(b, mf)
        rest = b - first
        cut = [first // 2, first - first // 2] if first > 1 else [first]  # two frames, or one
        runs0.append((len(s0), len(cut)))
        s0 += cut
        mid = [min(rest, mf), rest - min(rest, mf)]
        runs1.append((len(s1), 2))
        s1 += mid
    t0, t1 = _table(rng, s0), _table(rng, s1)
    arena, bases = _arena(rng, [t0, t1], gaps=[3, 9])
    keys = _mixed_keys(rng, 6)
    parts = [P.part(bases[0], len(t0[0]), t0[1], runs0), P.part(bases[1], len(t1[0]), t1[1], runs1)]
    ref, _ = _run(torch, eng, arena, parts, _sends([(i * 1000, i % 6) for i in range(len(lens))]), keys, mf)
    assert [len(p) for p in ref["plain"]] == lens
    assert list(ref["results"]["n_records"]) == [(b + mf - 1) // mf for b in lens]
    assert int(ref["records"]["plain_len"].max()) == mf


@pytest.mark.parametrize("align", range(16))
def test_alignment_sweep(torch, eng, align):
    """segments of 0 to 33 bytes and of 97 from every source alignment (frame j of a table lies
    j (j - 1) / 2 bytes past a base of the given alignment) to destinations that the records' 21-,
    22-, 29- and 30-byte overheads and the start of out shift to every alignment"""
    rng = random.Random(300 + align)
    tables = [_table(rng, list(range(34))), _table(rng, list(range(34))), _table(rng, list(range(35))),
              _table(rng, [97] * 17)]
    # bases at 16 k + align, + 5, + 10, + 15 (mod 16)
    buf, bases = bytearray(), []
    for k, (b, _) in enumerate(tables):
        buf += bytes([0xEE]) * ((align + 5 * k - len(buf)) % 16 + 16)
        bases.append(len(buf))
        buf += b
    arena = bytes(buf) + b"\xEE" * 3
    assert [b % 16 for b in bases] == [(align + 5 * k) % 16 for k in range(4)]
    keys = _mixed_keys(rng, 6)
    n = 34
    parts = [P.part(bases[0], len(tables[0][0]), tables[0][1], [(j, 1) for j in range(n)]),
             P.part(bases[1], len(tables[1][0]), tables[1][1], [(33 - j, 1) for j in range(n)]),
             P.part(bases[2], len(tables[2][0]), tables[2][1], [(j, 2) for j in range(n)]),
             P.part(bases[3], len(tables[3][0]), tables[3][1], [(j % 16, 1 + j % 2) for j in range(n)])]
    ref, _ = _run(torch, eng, arena, parts, _sends([(j, (j + align) % 6) for j in range(n)]), keys, 0, shift=align)
    assert ref["summary"][0]["n_failed"] == 0
    # (the test's own coverage) a segment of 31 bytes or more holds a whole aligned vector of out:
    # those segments meet every byte shift between source and destination
    shifts = set()
    for s, r in enumerate(ref["results"]):
        dst = align + int(ref["records"][int(r["first_record"])]["src_off"])
        for p in parts:
            f, cnt = (int(x) for x in p["runs"][s])
            a, b = int(p["off"][f]), int(p["off"][f + cnt])
            if b - a >= 31:
                shifts.add((p["base"] + a - dst) % 16)
            dst += b - a
    assert len(shifts) == 16


def test_eight_parts_of_one_to_three_bytes_in_one_record(torch, eng):
    rng = random.Random(41)
    tables = [_table(rng, [1 + (k + j) % 3 for j in range(6)]) for k in range(8)]
    arena, bases = _arena(rng, tables)
    keys = _mixed_keys(rng, 6)
    n = 12
    parts = [P.part(bases[k], len(tables[k][0]), tables[k][1], [((s + k) % 6, 1) for s in range(n)]) for k in range(8)]
    ref, _ = _run(torch, eng, arena, parts, _sends([(s, s % 6) for s in range(n)]), keys, 64, shift=7)
    assert list(ref["results"]["n_records"]) == [1] * n
    assert all(8 <= len(p) <= 24 for p in ref["plain"])


@pytest.mark.parametrize("mf", [0, TILE, TILE + 1, 5000])
def test_segments_around_the_gather_tile(torch, eng, mf):
    """segments of tile - 1, tile, tile + 1 and 2 tile + 1 bytes, before and after a short one"""
    rng = random.Random(500 + mf)
    sizes = [TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 77, 77, 77, 77]
    tables = [_table(rng, sizes), _table(rng, sizes)]
    arena, bases = _arena(rng, tables, gaps=[5, 11])
    keys = _mixed_keys(rng, 6)
    runs0 = [(i, 1) for i in range(4)] + [(4 + i, 1) for i in range(4)]
    runs1 = [(4 + i, 1) for i in range(4)] + [(i, 1) for i in range(4)]
    parts = [P.part(bases[0], len(tables[0][0]), tables[0][1], runs0),
             P.part(bases[1], len(tables[1][0]), tables[1][1], runs1)]
    ref, _ = _run(torch, eng, arena, parts, _sends([(i, (i + 1) % 6) for i in range(8)]), keys, mf, shift=3)
    assert sorted(len(p) for p in ref["plain"]) == sorted(2 * [s + 77 for s in sizes[:4]])


@pytest.mark.parametrize("n_parts", [1, 2, 3, 8])
@pytest.mark.parametrize("n_sends", [1, 255, 256, 257, 513])
def test_many_sends_of_tiny_frames(torch, eng, n_sends, n_parts):
    """0 to 3 frames per run: the sends' scan crosses its block edges, many sends have no record"""
    rng = random.Random(1000 * n_parts + n_sends)
    keys = _mixed_keys(rng, 7)
    arena, parts, sends = _random_batch(rng, n_sends, n_parts, [0, 1, 2, 15, 16, 17, 32],
                                        max_run=2 if n_parts == 8 else 3)
    ref, _ = _run(torch, eng, arena, parts, sends, keys, 16)
    assert ref["summary"][0]["n_failed"] == 0 and (n_sends == 1 or len(ref["records"]) > 0)


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
    ref, _ = _run(torch, eng, arena, parts, _sends([(1, 0), (2, 3), (3, 5)]), keys, 16)
    assert list(ref["results"]["status"]) == [0, 0, 0]
    if empty == "all":
        assert ref["out"] == b"" and list(ref["results"]["next_seq"]) == [1, 2, 3]
    else:
        assert int(ref["results"][0]["plain_len"]) == 2 * 147 and int(ref["results"][0]["n_records"]) == 19


def test_same_table_twice_around_an_excluded_frame(torch, eng):
    """relay without the sender: the room's table is part 0 with the frames before the receiver's
    own and part 1 with those after; then a table of the receiver's own (the replies)"""
    rng = random.Random(61)
    room, room_off = R.build_frames([rng.randbytes(rng.choice([5, 130, 400])) for _ in range(9)])
    own, own_off = R.build_frames([rng.randbytes(3) for _ in range(4)])
    arena, bases = _arena(rng, [(room, room_off), (own, own_off)], gaps=[5, 3])
    keys = _mixed_keys(rng, 9)
    before = [(0, i) for i in range(9)]
    after = [(i + 1, 8 - i) for i in range(9)]
    mine = [(i % 4, 1) for i in range(9)]
    parts = [P.part(bases[0], len(room), room_off, before), P.part(bases[0], len(room), room_off, after),
             P.part(bases[1], len(own), own_off, mine)]
    ref, _ = _run(torch, eng, arena, parts, _sends([(100 * i, i) for i in range(9)]), keys, 128)
    for i in range(9):
        want = room[:int(room_off[i])] + room[int(room_off[i + 1]):] + own[int(own_off[i % 4]):int(own_off[i % 4 + 1])]
        assert ref["plain"][i] == want


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
    ref, _ = _run(torch, eng, arena, parts, _sends([(1000 * i + 3, i) for i in range(n)]), keys)
    assert len(set(ref["per_send"])) == n and len({p for p in ref["plain"]}) == 3
    assert int(ref["summary"][0]["n_records"]) == sum((len(p) + 16383) // 16384 for p in ref["plain"])


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
    ref, _ = _run(torch, eng, arena, parts, sends, keys, 128)
    # 1: invalid key and a bad range -> the key; 2: slot past the table; 3: range, raised by the
    # last part alone; 4: the bad frame; 5: a frame after the bad one is good (offsets rise again);
    # 6: first_frame past the table of part 0, with n = 0.  The failed sends have no byte of out:
    # their neighbours' records lie back to back (the reference's out, compared in _run)
    assert list(ref["results"]["status"]) == [0, O.REC_KEY, O.REC_KEY, R.REC_RANGE, R.REC_RANGE, 0, R.REC_RANGE, 0]
    assert ref["summary"][0]["n_failed"] == 5
    assert list(ref["results"]["next_seq"][[1, 2, 3, 4, 6]]) == [2, 3, 4, 5, 7]
    assert list(ref["results"]["out_len"][[1, 2, 3, 4, 6]]) == [0] * 5
    # a bad frame outside every run harms nobody
    clear = [P.part(bases[0], len(t0[0]), t0[1], [(0, 2)] * 3), P.part(bases[1], len(t1[0]), bad, [(0, 1), (2, 2), (4, 0)])]
    ref, _ = _run(torch, eng, arena, clear, _sends([(1, 0), (2, 2), (3, 3)]), keys, 128)
    assert list(ref["results"]["status"]) == [0, 0, 0]
    # the last part's len one short of its last frame: only the sends that name that frame fail
    short = [P.part(bases[0], len(t0[0]), t0[1], [(0, 2)] * 3),
             P.part(bases[1], len(t1[0]) - 1, t1[1], [(0, 3), (3, 1), (4, 0)])]
    ref, _ = _run(torch, eng, arena, short, _sends([(1, 0), (2, 2), (3, 3)]), keys, 128)
    assert list(ref["results"]["status"]) == [0, R.REC_RANGE, 0]


@pytest.mark.parametrize("short", ["out_cap", "max_records"])
def test_capacity(torch, eng, short):
    rng = random.Random(72)
    arena, parts, sends = _random_batch(rng, 9, 3, [0, 1, 63, 64, 65, 128, 700], n_keys=6)
    keys = _mixed_keys(rng, 6)
    sends[4]["key"] = 77
    full = K.seal_parts_coalesced_ref(arena, parts, sends, keys, 64)
    cap = dict(out_cap=len(full["out"]) - 1) if short == "out_cap" else dict(max_records=len(full["records"]) - 1)
    ref, _ = _run(torch, eng, arena, parts, sends, keys, 64, **cap)  # out and records stay 0xA5 throughout
    want = [O.REC_CAPACITY] * 9
    want[4] = O.REC_KEY
    assert list(ref["results"]["status"]) == want
    assert ref["out"] == b"" and len(ref["records"]) == 0 and ref["summary"][0]["n_failed"] == 9
    assert ref["summary"].tobytes()[:12] == full["summary"].tobytes()[:12]
    s = ref["summary"][0]
    again, _ = _run(torch, eng, arena, parts, sends, keys, 64, max_records=int(s["n_records"]),
                    out_cap=int(s["out_bytes"]))
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
    eng.seal_parts_coalesced(d["arena"], [good], d["sends"], 0, d["keys"], 6, 16, out, records=recs, results=res,
                             summary=summ)
    torch.cuda.synchronize()
    assert not summ.any() and (out == FILL).all()
    L = U.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(parts=(good,), n_parts=None, frames=p(d["arena"]), frames_len=len(arena), sends=p(d["sends"]),
             keys_=p(d["keys"]), mf=0, recs_=p(recs), max_records=16, res_=p(res), summ_=p(summ), out_=p(out),
             n_sends=1, out_cap=4096):
        tab = (U.TlsPart * 9)()
        for k, (base, ln, off, runs, stride, n) in enumerate(parts):
            tab[k] = U.TlsPart(base, ln, off.data_ptr() if off is not None else None,
                               runs.data_ptr() if runs is not None else None, stride, n)
        return L.uvhttp_tls_gpu_seal_parts_coalesced(eng.h, frames, frames_len, tab,
                                                     len(parts) if n_parts is None else n_parts, sends, n_sends,
                                                     keys_, 6, mf, recs_, max_records, res_, summ_, out_, out_cap, st)
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
    # out inside, across either end of, and around the frames; touching ranges are fine
    both = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")
    fr = lambda a, n: dict(frames=C.c_void_p(both.data_ptr() + a), frames_len=n)  # noqa: E731
    ou = lambda a, n: dict(out_=C.c_void_p(both.data_ptr() + a), out_cap=n)      # noqa: E731
    small = ((0, 0, d["off"], d["runs"], 8, 0),)  # (the frames here are rubbish: no run names any)
    for a, n in ((1024, 2048), (0, 1025), (3071, 2048), (0, 8192), (2000, 1)):
        assert call(parts=small, **fr(1024, 2048), **ou(a, n)) == -1, (a, n)
    for a, n in ((0, 1024), (3072, 2048)):
        assert call(parts=small, **fr(1024, 2048), **ou(a, n)) == 0, (a, n)
    assert call() == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", range(6))
def test_one_short_frame_per_send_is_seal_parts_byte_for_byte(torch, eng, kind):
    """a stream of one frame no longer than max_fragment: out, results and summary of the device's
    seal_parts, byte for byte"""
    rng = random.Random(400 + kind)
    frames, off = R.build_frames([rng.randbytes(n) for n in (1, 15, 16, 125, 126, 508, 200)])
    arena = b"\xEE" * 9 + frames
    keys = _mixed_keys(rng, 6)
    n = 7
    sends = _sends([(rng.getrandbits(40), (kind + i) % 6) for i in range(n)])
    parts = [P.part(9, len(frames), off, [(i, 1) for i in range(n)]), P.part(9, len(frames), off, [(i, 0) for i in range(n)])]
    ref, out = _run(torch, eng, arena, parts, sends, keys, 512)
    assert int(ref["records"]["plain_len"].max()) == 512
    rows, keep = _dev_parts(torch, parts)
    out2 = torch.full((len(ref["out"]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    recs2, res2, sum2 = eng.seal_parts(_dev(torch, np.frombuffer(arena, np.uint8)), rows, _dev(torch, sends), n,
                                       _dev(torch, keys), 6, len(ref["records"]), out2[:len(ref["out"])],
                                       max_fragment=512)
    torch.cuda.synchronize()
    assert torch.equal(out2[:len(ref["out"])], out)
    assert res2.cpu().numpy()[:n * 48].tobytes() == ref["results"].tobytes()
    assert sum2.cpu().numpy()[:32].tobytes() == ref["summary"].tobytes()


@pytest.mark.parametrize("seed", range(2))
def test_opened_streams_equal_those_of_seal_parts(torch, eng, seed):
    """any input: what a receiver reads is the same under both cuttings"""
    rng = random.Random(450 + seed)
    keys = _mixed_keys(rng, 7)
    arena, parts, sends = _random_batch(rng, 40, 1 + 3 * seed, [0, 1, 63, 64, 65, 300, 20000])
    ref, _ = _run(torch, eng, arena, parts, sends, keys, 0)
    per_frame = P.seal_parts_ref(arena, parts, sends, keys, 0)
    rows, keep = _dev_parts(torch, parts)
    out2 = torch.zeros(len(per_frame["out"]) + 64, dtype=torch.uint8, device="cuda")
    _, res2, _ = eng.seal_parts(_dev(torch, np.frombuffer(arena, np.uint8)), rows, _dev(torch, sends), len(sends),
                                _dev(torch, keys), len(keys), len(per_frame["records"]), out2[:len(per_frame["out"])])
    torch.cuda.synchronize()
    res2 = res2.cpu().numpy()[:len(sends) * 48].view(R.TLS_SEND_RESULT_DT)
    assert _opened(keys, sends, res2, out2.cpu().numpy().tobytes()) == ref["plain"]
    assert int(ref["summary"][0]["n_records"]) < len(per_frame["records"])


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
        batches.append((arena, parts, sends, K.seal_parts_coalesced_ref(arena, parts, sends, keys, mf)))
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
        eng.seal_parts_coalesced(d_arena, rows, d_sends, n_sends, d_keys, 6, max_records, out[:out_cap],
                                 max_fragment=mf, records=recs, results=res, summary=summ, stream=stream)
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
    """30 batches per case: random parts, runs, keys, cuts, alignments and failures of every kind"""
    rng = random.Random(900 + seed)
    keys = _mixed_keys(rng, 12)
    keys[5]["key_len"] = 24
    keys[11]["version"] = 0x0302
    failed = 0
    for _ in range(30):
        mf = rng.choice([1, 7, 16, 64, 4096, 16384])
        n_parts, n_sends = rng.randint(1, 8), rng.randint(1, 12)
        small = [0, 1, 2, 5] if mf == 1 else [0, 1, mf - 1, mf, mf + 1, 2 * mf] if mf <= 64 else [0, 1, 300, 4095, 4097, 16385]
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
        ref, _ = _run(torch, eng, arena, parts, _sends(rows), keys, mf, strides=strides, shift=rng.randrange(16))
        failed += int(ref["summary"][0]["n_failed"])
    assert failed > 0
