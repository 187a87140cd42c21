"""TLS record open / seal on the MI355X at the edges random batches do not reach, bit-exact
against the CPU oracle (oracle/tls_oracle.c) and against the plain-integer reference
(tests/_aead_ref.py) through tests/golden/tls_edge_vectors.json:

  - the directed vectors (Poly1305 accumulators solved to end at 0..4, p-1, p-2, 2^128, ...,
    tags of all zeros / ones, a full ripple carry of h + s; all-0x00 / all-0xff / single-bit
    ciphertexts) on every route: the packed open kernels, the one-record-per-wave open kernels
    and the seal kernels;
  - all-0xff and all-0x00 ciphertext at 4 KiB, 8 KiB, both pack limits +-1 and the maximum;
  - a sweep of every content length 0..1100 and +-24 around each multiple of 1024, in an order
    that keeps groups homogeneous and in a shuffled one (short records in long groups);
  - TLS 1.3 padding across the 4 KiB rounds, all-zero inner plaintexts, control types.

Routes.  Counted records are numbered across connections in index order; a group of 4
consecutive records holding a record of a cipher longer than that cipher's pack limit is opened
one record per wave, every other record of that cipher by the packed kernel (tls_gpu.hip:
kPack, kPackMaxLen, kPackMaxLenAes).  _routes() restates that rule and the tests assert that
each record went where the case wants it.
"""
import base64
import hashlib
import importlib.util
import json
import os
import random

import numpy as np
import pytest

import _aead_ref as R
import _oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

K_PACK = 4
# TLSCiphertext.length up to which a record is packed (kPackMaxLenAes, kPackMaxLen)
PACK_LIMIT = {O.AES_GCM: 4096 + 1 + 24, O.CHACHA: 8192 + 1 + 16}
# content of the long companion record that sends its group to the per-wave kernel
LONG_CONTENT = {O.AES_GCM: 4200, O.CHACHA: 8300}


def _load_generator():
    spec = importlib.util.spec_from_file_location(
        "make_tls_edge_vectors", os.path.join(GOLD, "make_tls_edge_vectors.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _load_generator()
KINDS = GEN.KINDS
KIND_IDX = {k["name"]: i for i, k in enumerate(KINDS)}
KEYS = np.concatenate([O.tls_key(k["key"], k["iv"], k["version"], k["cipher"]) for k in KINDS])
KIND_NAMES = [k["name"] for k in KINDS]


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


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(GOLD, "tls_edge_vectors.json")) as f:
        return json.load(f)


# ---- the shapes of tests/test_gpu_tls.py ---------------------------------------------------


def _dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if b.size == 0:
        b = np.zeros(16, np.uint8)
    return torch.from_numpy(b.copy()).to("cuda")


def _run(torch, eng, wire, keys, streams):
    w = np.ascontiguousarray(wire, np.uint8)
    max_records = max(1, w.size // 5 + 1)
    out = torch.zeros(max(16, w.size), dtype=torch.uint8, device="cuda")
    recs, res = eng.open_records(_dev(torch, w), _dev(torch, keys), len(keys),
                                 _dev(torch, streams), len(streams), max_records,
                                 out[:w.size], wire_len=w.size)
    torch.cuda.synchronize()
    res_h = res.cpu().numpy().view(O.TLS_RESULT_DT)[:len(streams)]
    n = int(res_h["n_records"].sum()) if len(res_h) else 0
    return recs.cpu().numpy().view(O.TLS_RECORD_DT)[:n], res_h, out.cpu().numpy()


def check(torch, eng, wire, keys, streams):
    """device == oracle: records, connection results, delivered bytes"""
    ro, so, oo = O.tls_open_batch(wire, keys, streams)
    rd, sd, od = _run(torch, eng, wire, keys, streams)
    assert so.tobytes() == sd.tobytes(), (so, sd)
    assert ro.tobytes() == rd.tobytes(), _first_diff(ro, rd)
    for r in so:
        a, b = int(r["out_off"]), int(r["out_off"] + r["plain_len"])
        assert np.array_equal(oo[a:b], od[a:b])
    return ro, so, oo


def _first_diff(ro, rd):
    for i, (a, b) in enumerate(zip(ro, rd)):
        if a.tobytes() != b.tobytes():
            return i, a, b
    return len(ro), len(rd)


def _seal_dev(torch, eng, src, descs, keys, out_bytes):
    out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    eng.seal_records(_dev(torch, src), _dev(torch, descs), len(descs), _dev(torch, keys),
                     len(keys), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- laying records out on a route ---------------------------------------------------------


def _rec_len(rec):
    return (rec[3] << 8) | rec[4]


def _is_long(kind, rec):
    return _rec_len(rec) > PACK_LIMIT[KINDS[kind]["cipher"]]


class Batch:
    """connections appended in index order; every record added is complete and passes the
    header checks, so the n-th record added is counted record n"""

    def __init__(self):
        self.wire = bytearray()
        self.conns = []  # (begin, len, seq, key)
        self.n_records = 0

    def conn(self, kind, seq, records):
        begin = len(self.wire)
        for r in records:
            self.wire += r
        self.conns.append((begin, len(self.wire) - begin, seq, kind))
        first = self.n_records
        self.n_records += len(records)
        return len(self.conns) - 1, first

    def align(self):
        """fill the current group of K_PACK with short records (one connection each)"""
        while self.n_records % K_PACK:
            self.conn(0, 7, [O.tls_seal(KEYS[0:1], 7, 23, b"fill")])

    def arrays(self):
        st = np.zeros(len(self.conns), O.TLS_STREAM_DT)
        for i, (b, ln, seq, k) in enumerate(self.conns):
            st[i]["begin"], st[i]["len"], st[i]["seq"], st[i]["key"] = b, ln, seq, k
        return np.frombuffer(bytes(self.wire), np.uint8), st


_LONG_BODY = bytes(range(256)) * 33


def place(items, mode):
    """items: (kind, seq, record) -> Batch, and the counted-record index of every item.
    mode "packed": the short records fill groups of their own, the long ones follow;
    mode "wave": every short record shares its group with a long record of its own key (a
    connection of the long record at seq - 1 and the item), so the per-wave kernel opens it."""
    b = Batch()
    where = [None] * len(items)
    for i, (kind, seq, rec) in enumerate(items):
        if _is_long(kind, rec):
            continue
        if mode == "packed":
            where[i] = b.conn(kind, seq, [rec])[1]
        else:
            b.align()
            body = _LONG_BODY[:LONG_CONTENT[KINDS[kind]["cipher"]]]
            long_rec = O.tls_seal(KEYS[kind:kind + 1], seq - 1, 23, body)
            assert _is_long(kind, long_rec)
            where[i] = b.conn(kind, seq - 1, [long_rec, rec])[1] + 1
            b.align()
    b.align()
    for i, (kind, seq, rec) in enumerate(items):
        if _is_long(kind, rec):
            where[i] = b.conn(kind, seq, [rec])[1]
    return b, where


def _routes(wire, keys, st, recs):
    """per counted record: True = one record per wave (its group of K_PACK holds a record of
    its cipher over the pack limit), False = packed"""
    off = recs["rec_off"].astype(np.int64)
    ln = (wire[off + 3].astype(np.int64) << 8) | wire[off + 4]
    cipher = keys["cipher"][st["key"][recs["stream"]]].astype(np.int64)
    lim = np.where(cipher == O.AES_GCM, PACK_LIMIT[O.AES_GCM], PACK_LIMIT[O.CHACHA])
    big = ln > lim
    wave = np.zeros(len(recs), bool)
    for g in range(0, len(recs), K_PACK):
        for c in (O.AES_GCM, O.CHACHA):
            sel = cipher[g:g + K_PACK] == c
            if (big[g:g + K_PACK] & sel).any():
                wave[g:g + K_PACK] |= sel
    return wave


def open_placed(torch, eng, items, mode):
    """open the items on the route `mode` asks for -> each item's (record, delivered bytes)"""
    b, where = place(items, mode)
    wire, st = b.arrays()
    ro, so, oo = check(torch, eng, wire, KEYS, st)
    assert len(ro) == b.n_records
    wave = _routes(wire, KEYS, st, ro)
    got = []
    for (kind, seq, rec), w in zip(items, where):
        r = ro[w]
        assert wire[int(r["rec_off"]):int(r["rec_off"]) + len(rec)].tobytes() == rec, "record misplaced"
        assert wave[w] == (mode == "wave" or _is_long(kind, rec)), (mode, kind, len(rec))
        o = int(r["out_off"])
        got.append((r, oo[o:o + int(r["content_len"])].tobytes() if r["status"] == O.REC_OK else b""))
    return got


def _expect_entry(e, r, content, what):
    assert (int(r["status"]), int(r["type"]), int(r["content_len"])) == \
        (e["status"], e["type"], e["content_len"]), (what, e["why"])
    if e["status"] == O.REC_OK:
        assert hashlib.sha256(content).hexdigest() == e["content_sha256"], (what, e["why"])


def _item(e):
    return KIND_IDX[e["kind"]], e["seq"], base64.b64decode(e["record_b64"])


# ---- directed vectors ----------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["packed", "wave"])
def test_directed_vectors_open(torch, eng, vectors, mode):
    """Every fixture vector opens to the status and content the reference predicts, on the
    packed kernels and on the one-record-per-wave kernels; a solved vector with one tag bit or
    one ciphertext bit flipped fails authentication."""
    rng = random.Random(0xED6E)
    entries = vectors["solved"] + vectors["pattern"]
    items = [_item(e) for e in entries]
    n_plain = len(items)
    for e in vectors["solved"]:
        kind, seq, rec = _item(e)
        for lo, hi in ((len(rec) - 16, len(rec)), (5, len(rec) - 16)):  # tag, ciphertext
            bad = bytearray(rec)
            bad[rng.randrange(lo, hi)] ^= 1 << rng.randrange(8)
            items.append((kind, seq, bytes(bad)))
    got = open_placed(torch, eng, items, mode)
    for i, e in enumerate(entries):
        _expect_entry(e, got[i][0], got[i][1], i)
    for i in range(n_plain, len(items)):
        assert got[i][0]["status"] == O.REC_BAD_MAC, i


def _plaintext(e):
    """content of a fixture record (the inner type byte dropped), from the reference"""
    kind, seq, rec = _item(e)
    k = KINDS[kind]
    ct = rec[5 + R.explicit_len(k["version"], k["cipher"]):-16]
    pt = R._xor(ct, R.record_keystream(k["key"], k["iv"], k["version"], k["cipher"], seq, len(ct)))
    return pt[:-1] if k["version"] == R.TLS13 else pt


def _seal_entries(torch, eng, entries):
    """seal the entries' plaintext on the device: the wire bytes must be the entries' records"""
    entries = [e for e in entries if e["seal_pad"] == 0]  # the device seal writes no padding
    src, descs, off = bytearray(), np.zeros(len(entries), O.TLS_SEAL_DT), 0
    want = []
    for i, e in enumerate(entries):
        kind, seq, rec = _item(e)
        pt = _plaintext(e)
        descs[i] = (len(src), off, seq, len(pt), kind, e["seal_type"], 0)
        src += pt
        want.append((off, rec))
        off += len(rec) + (0, 3, 16)[i % 3]
    got = _seal_dev(torch, eng, np.frombuffer(bytes(src) + bytes(16), np.uint8), descs, KEYS, off + 64)
    for i, (o, rec) in enumerate(want):
        assert got[o:o + len(rec)].tobytes() == rec, (i, entries[i]["why"])
    return len(entries)


def test_directed_vectors_seal(torch, eng, vectors):
    entries = vectors["solved"] + vectors["pattern"]
    assert _seal_entries(torch, eng, entries) == len(entries)


# ---- long pattern records ------------------------------------------------------------------


def _long_pattern_lengths(kind):
    """ciphertext bytes: 4 KiB, 8 KiB, both pack limits +-1 (as ciphertext of this key kind)
    and the largest record"""
    k = KINDS[kind]
    over = 16 + R.explicit_len(k["version"], k["cipher"])
    s = {4096, 8192, 16384 + (1 if k["version"] == R.TLS13 else 0)}
    for lim in PACK_LIMIT.values():
        s.update(lim - over + d for d in (-1, 0, 1))
    return sorted(s)


@pytest.mark.parametrize("kind", range(6), ids=KIND_NAMES)
def test_long_pattern_records(torch, eng, kind):
    """all-0xff ciphertext has every Poly1305 limb and every GHASH bit at its maximum through
    every Horner step and tree level of a full record; all-0x00 is the other end.  Tags from
    the reference; open on both routes, then seal."""
    entries = [GEN.pattern_entry(KINDS[kind], 900000 + 16 * j + p, name, n)
               for j, n in enumerate(_long_pattern_lengths(kind))
               for p, name in enumerate(("ff", "zero"))]
    items = [_item(e) for e in entries]
    assert any(_is_long(*it[::2]) for it in items) and not all(_is_long(*it[::2]) for it in items)
    for mode in ("packed", "wave"):
        for i, (r, content) in enumerate(open_placed(torch, eng, items, mode)):
            assert entries[i]["status"] in (O.REC_OK, O.REC_CONTROL)
            _expect_entry(entries[i], r, content, (mode, i))
    assert _seal_entries(torch, eng, entries) >= len(entries) - 1


# ---- length sweep --------------------------------------------------------------------------


def sweep_lengths():
    """every content length 0..1100, and within +-24 of each multiple of 1024 up to 16384"""
    s = set(range(1101))
    for m in range(1024, 16385, 1024):
        s.update(range(m - 24, min(m + 24, 16384) + 1))
    return sorted(s)


_SWEEP = {}


def _sweep(kind, order):
    """-> (wire, streams, [(connection, seq, content)] in wire order), sealed by the oracle:
    the sweep's records in connections of 1 to 8"""
    if (kind, order) in _SWEEP:
        return _SWEEP[kind, order]
    lengths = sweep_lengths()
    blob = np.random.default_rng(1000 + kind).integers(0, 256, 16384 + len(lengths), dtype=np.uint8).tobytes()
    rng = random.Random(50 + kind)
    if order == "shuffled":
        rng.shuffle(lengths)
    wire, conns, recs, i = bytearray(), [], [], 0
    while i < len(lengths):
        n = min(rng.randint(1, 8), len(lengths) - i)
        seq = rng.randrange(1 << 48)
        begin = len(wire)
        for j in range(n):
            ln = lengths[i + j]
            content = blob[(i + j):(i + j) + ln]
            wire += O.tls_seal(KEYS[kind:kind + 1], seq + j, 23, content)
            recs.append((len(conns), seq + j, content))
        conns.append((begin, len(wire) - begin, seq, kind))
        i += n
    st = np.zeros(len(conns), O.TLS_STREAM_DT)
    for c, (b, ln, seq, k) in enumerate(conns):
        st[c]["begin"], st[c]["len"], st[c]["seq"], st[c]["key"] = b, ln, seq, k
    _SWEEP[kind, order] = np.frombuffer(bytes(wire), np.uint8), st, recs
    return _SWEEP[kind, order]


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("kind", range(6), ids=KIND_NAMES)
def test_length_sweep_open(torch, eng, kind, order):
    wire, st, recs = _sweep(kind, order)
    ro, so, oo = check(torch, eng, wire, KEYS, st)
    assert len(ro) == len(recs) and (ro["status"] == O.REC_OK).all()
    want = [bytearray() for _ in so]
    for c, _, content in recs:
        want[c] += content
    for c, r in enumerate(so):  # the oracle's (= the device's) plaintext is what was sealed
        assert oo[int(r["out_off"]):int(r["out_off"] + r["plain_len"])].tobytes() == want[c]
    # a seeded sample of about 40 records against the reference: the delivered bytes (the
    # device's, equal to the oracle's by check()) are what the reference opens the record to
    k = KINDS[kind]
    rng = random.Random(400 + kind)
    edges = {1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384}
    for i in [i for i, x in enumerate(recs) if len(x[2]) in edges] + rng.sample(range(len(recs)), 29):
        r = ro[i]
        a, b = int(r["rec_off"]), int(ro[i + 1]["rec_off"]) if i + 1 < len(ro) else wire.size
        status, type_, content = R.open_record(k["key"], k["iv"], k["version"], k["cipher"],
                                               recs[i][1], wire[a:b].tobytes())
        assert (status, type_) == (R.REC_OK, 23) and len(content) == r["content_len"]
        assert oo[int(r["out_off"]):int(r["out_off"]) + len(content)].tobytes() == content
    wave = _routes(wire, KEYS, st, ro)
    cipher = KINDS[kind]["cipher"]
    off = ro["rec_off"].astype(np.int64)
    short = ((wire[off + 3].astype(np.int64) << 8) | wire[off + 4]) <= PACK_LIMIT[cipher]
    if order == "ascending":  # short records packed (but the group the limit falls in)
        assert (short & wave).sum() < K_PACK and (short & ~wave).sum() > 1100
    else:                     # short records ride in long groups, and some stay packed
        assert (short & wave).sum() > 300 and (short & ~wave).sum() > 100


@pytest.mark.parametrize("kind", range(6), ids=KIND_NAMES)
def test_length_sweep_seal(torch, eng, kind):
    """the device seals the sweep's contents to the oracle's wire, and a seeded sample of about
    40 records (the lengths around the rotation period, the LDS round and the pack limits
    among them) equals the reference's seal"""
    wire, st, recs = _sweep(kind, "ascending")
    src = bytearray()
    descs = np.zeros(len(recs), O.TLS_SEAL_DT)
    k = KINDS[kind]
    over = 5 + 16 + R.explicit_len(k["version"], k["cipher"]) + (1 if k["version"] == R.TLS13 else 0)
    off, offs = 0, []
    for i, (_, seq, content) in enumerate(recs):
        descs[i] = (len(src), off, seq, len(content), kind, 23, 0)
        src += content
        offs.append(off)
        off += len(content) + over
    assert off == wire.size
    got = _seal_dev(torch, eng, np.frombuffer(bytes(src) + bytes(16), np.uint8), descs, KEYS, off)
    assert np.array_equal(got, wire)
    rng = random.Random(600 + kind)
    edges = {1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384}
    sample = [i for i, x in enumerate(recs) if len(x[2]) in edges] + rng.sample(range(len(recs)), 29)
    for i in sample:
        _, seq, content = recs[i]
        want = R.seal_record(k["key"], k["iv"], k["version"], k["cipher"], seq, 23, content)
        assert got[offs[i]:offs[i] + len(want)].tobytes() == want, len(content)


# ---- TLS 1.3 padding -----------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["packed", "wave"])
@pytest.mark.parametrize("kind", [0, 2, 4], ids=[KIND_NAMES[i] for i in (0, 2, 4)])
def test_tls13_padding(torch, eng, kind, mode):
    """The last-non-zero search over padding that spans the 4 KiB rounds: padded application
    data is delivered without its padding, an all-zero inner plaintext is ERR_EMPTY, an inner
    alert / handshake type before long padding is CONTROL (include/uvhttp_tls_amd.h)."""
    assert KINDS[kind]["version"] == R.TLS13
    key = KEYS[kind:kind + 1]
    blob = random.Random(70 + kind).randbytes(100)
    cases = []  # (type, content, pad, status)
    for n in (0, 1, 100):
        for pad in (4095, 4096, 8191, 16384 - n):
            cases.append((23, blob[:n], pad, O.REC_OK))
    for n in (1, 64, 4097, 16385):
        cases.append((0, b"", n - 1, O.REC_EMPTY))
    for t in (21, 22):
        for pad in (4096, 16382):
            cases.append((t, blob[:2], pad, O.REC_CONTROL))
    items = [(kind, 3000 + 2 * i, O.tls_seal(key, 3000 + 2 * i, t, c, pad))
             for i, (t, c, pad, _) in enumerate(cases)]
    got = open_placed(torch, eng, items, mode)
    for (t, c, pad, status), (r, content) in zip(cases, got):
        assert r["status"] == status, (t, len(c), pad)
        if status == O.REC_EMPTY:
            assert (r["type"], r["content_len"]) == (0, 0)
        else:
            assert (r["type"], r["content_len"]) == (t, len(c)), (t, len(c), pad)
        if status == O.REC_OK:
            assert content == c
