"""The reference's own WebSocket unit, compiled as it stands (oracle/ref.mk ->
oracle/_ref/libws_ref.so), run against the oracle's restatement (oracle/ws_oracle.c) and the
product's host surface (uvhttp_amd/csrc/ws_host.c): reference == oracle == host, byte for byte.

parse_frame_header over every value of the first two header bytes at every buffer length, apply_mask
over lengths, keys and alignments, build_frame over the lengths at which the header changes, and
seeded process_data sessions from the grammar of tests/_reference.py, cut into reads four ways.
The census test counts, per branch and side, the sessions in which the reference took the branch
(judged from its transcript) and fails if a branch never occurred.  The last test regenerates
tests/golden/reference_transcripts.json in memory and compares it with the committed file.

Without the reference tree AND without the library (a clean checkout elsewhere) the file skips:
tests/test_reference_transcripts_host.py then guards the same behaviour from the committed
transcripts.  With the tree but no library it fails: the library is part of the build."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import _oracle as O
import _reference as RF
import uvhttp_amd as U

pytestmark = pytest.mark.skipif(
    RF.load_ref() is None and not RF.have_reference_tree(),
    reason="no reference tree and no oracle/_ref/libws_ref.so: the committed transcripts stand in")


@pytest.fixture(scope="module")
def R():
    lib = RF.load_ref()
    assert lib is not None, ("the reference tree is at %s but oracle/_ref/libws_ref.so is not built "
                             "(make -C oracle)" % RF.REFERENCE_DIR)
    return lib


@pytest.fixture(scope="module")
def host_hooks():
    RF.install_host_hooks()
    yield
    RF.remove_host_hooks()


def test_key_stream_is_the_drivers(R):
    for seed in (0, 1, 0xC0FFEE00, (1 << 64) - 1):
        for i in (0, 1, 2, 1000):
            assert RF.key_word(seed, i) == R.ws_ref_key_word(seed, i)


# ---- parse_frame_header ------------------------------------------------------------------------

def _parse_all(R, bufs, lens):
    """-> (rc, fields [n, 8], header_size) of the three implementations for n 16-byte buffers"""
    n = len(lens)
    raw = np.ascontiguousarray(bufs, dtype=np.uint8)
    ln = np.ascontiguousarray(lens, dtype=np.uint32)
    rc = np.zeros(n, np.int32)
    fields = np.zeros((n, 8), np.uint64)
    hs = np.zeros(n, np.uint64)
    R.ws_ref_parse_many(raw.ctypes.data, 16, ln.ctypes.data, n, rc.ctypes.data, fields.ctypes.data,
                        hs.ctypes.data)
    out = [(rc, fields, hs)]
    base = raw.ctypes.data
    # the oracle: one byte per field
    L = O.load()
    hdr = (O.OrcHeader * n)()
    hsz = (C.c_size_t * n)()
    orc = np.zeros(n, np.int32)
    fn, hb, sb = L.oracle_parse_frame_header, C.sizeof(O.OrcHeader), C.sizeof(C.c_size_t)
    hp = C.cast(hdr, C.c_void_p).value
    sp = C.cast(hsz, C.c_void_p).value
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    try:
        for i in range(n):
            orc[i] = fn(base + 16 * i, int(ln[i]), hp + hb * i, sp + sb * i)
    finally:
        fn.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(O.OrcHeader), C.POINTER(C.c_size_t)]
    a = np.frombuffer(hdr, np.uint8).reshape(n, hb)
    of = np.zeros((n, 8), np.uint64)
    of[:, :7] = a[:, :7]
    of[:, 7] = np.frombuffer(hdr, np.uint64).reshape(n, hb // 8)[:, 1]
    out.append((orc, of, np.frombuffer(hsz, np.uint64).copy()))
    # the product: the reference's own bitfield struct
    PL = U.lib()
    ph = (U.FrameHeader * n)()
    psz = (C.c_size_t * n)()
    prc = np.zeros(n, np.int32)
    pfn = PL.uvhttp_ws_parse_frame_header
    saved = pfn.argtypes
    pfn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    pp, qp = C.cast(ph, C.c_void_p).value, C.cast(psz, C.c_void_p).value
    try:
        for i in range(n):
            prc[i] = pfn(base + 16 * i, int(ln[i]), pp + 16 * i, qp + sb * i)
    finally:
        pfn.argtypes = saved
    b = np.frombuffer(ph, np.uint8).reshape(n, 16)
    pf = np.zeros((n, 8), np.uint64)
    b0, b1 = b[:, 0].astype(np.uint64), b[:, 1].astype(np.uint64)
    for k in range(4):  # fin, rsv1, rsv2, rsv3: bits 0-3 of byte 0 (gcc's little-endian bitfields)
        pf[:, k] = (b0 >> np.uint64(k)) & np.uint64(1)
    pf[:, 4] = b0 >> np.uint64(4)
    pf[:, 5] = b1 & np.uint64(1)
    pf[:, 6] = b1 >> np.uint64(1)
    pf[:, 7] = np.frombuffer(ph, np.uint64).reshape(n, 2)[:, 1]
    out.append((prc, pf, np.frombuffer(psz, np.uint64).copy()))
    return out


def _assert_parse_equal(res, bufs, lens, what):
    ref = res[0]
    for name, got in zip(("oracle", "host"), res[1:]):
        for part, x, y in zip(("rc", "fields", "header_size"), ref, got):
            bad = np.nonzero((x != y).reshape(len(lens), -1).any(axis=1))[0]
            assert bad.size == 0, "%s: %s differs from the reference in %s at head %s, length %d" % (
                what, name, part, bytes(bufs[bad[0]][:10]).hex(), lens[bad[0]])


def test_bitfield_layout_of_the_header():
    """the decoding of the product's header struct above is the compiler's layout"""
    h = U.FrameHeader(fin=1, rsv1=0, rsv2=1, rsv3=0, opcode=0xA, mask=1, payload_len=0x55)
    raw = bytes(h)
    assert raw[0] == 0b10100101 and raw[1] == (0x55 << 1 | 1)


@pytest.mark.parametrize("length", range(15))
def test_parse_every_head_at_every_length(R, length):
    """every value of bytes 0 and 1 with a seeded tail, at one buffer length"""
    rng = np.random.default_rng(0x9A55E + length)
    bufs = rng.integers(0, 256, (65536, 16), dtype=np.uint8)
    heads = np.arange(65536, dtype=np.uint32)
    bufs[:, 0] = heads >> 8
    bufs[:, 1] = heads & 0xFF
    lens = np.full(65536, length, np.uint32)
    res = _parse_all(R, bufs, lens)
    _assert_parse_equal(res, bufs, lens, "length %d" % length)
    rc = res[0][0]
    assert (rc == 0).any() == (length >= 2)  # the cases are not all failures


def test_parse_the_64_bit_lengths(R):
    rows = []
    for value in ((1 << 63) - 1, 1 << 63, (1 << 64) - 1, 65535, 65536, 0, 125):
        for b0 in (0x82, 0x01, 0xF9):
            for mask in (0, 0x80):
                for length in range(15):
                    rows.append((bytes([b0, mask | 127]) + value.to_bytes(8, "big") + b"\xa5" * 6, length))
    bufs = np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(-1, 16).copy()
    lens = np.array([r[1] for r in rows], np.uint32)
    res = _parse_all(R, bufs, lens)
    _assert_parse_equal(res, bufs, lens, "64-bit lengths")
    rc, fields, hs = res[0]
    ok = {(bytes(b[2:10]), int(n)): int(c) for b, n, c in zip(bufs, lens, rc)}
    assert ok[(((1 << 63) - 1).to_bytes(8, "big"), 10)] == 0
    assert ok[((1 << 63).to_bytes(8, "big"), 14)] != 0  # RFC 6455 §5.2 (:178)
    assert ok[((65535).to_bytes(8, "big"), 9)] != 0


# ---- apply_mask --------------------------------------------------------------------------------

MASK_KEYS = [b"\0\0\0\0", b"\xff\xff\xff\xff", b"\x37\x37\x37\x37", b"\0\x01\0\x02", b"\x80\0\0\0", b"\0\0\0\x01",
             b"\x12\x34\x56\x78"] + [random.Random(0x3A5C + i).randbytes(4) for i in range(6)]


def test_apply_mask_lengths_keys_and_alignments(R):
    rng = random.Random(0xA11)
    PL, OL = U.lib(), O.load()
    for key in MASK_KEYS:
        kb = (C.c_uint8 * 4).from_buffer_copy(key)
        for off in range(16):
            for n in range(68):
                src = rng.randbytes(off + n + 16)
                got = []
                for fn in (R.ws_ref_apply_mask, OL.oracle_apply_mask, PL.uvhttp_ws_apply_mask):
                    raw = (C.c_uint8 * (len(src) + 16))()
                    base = C.addressof(raw)
                    start = (-base) % 16 + off  # the buffer starts at offset `off` of a 16-byte line
                    C.memmove(base + start - off, src, len(src))
                    fn(C.c_void_p(base + start), n, kb)
                    got.append(C.string_at(base + start - off, len(src)))
                want = src[:off] + bytes(b ^ key[i & 3] for i, b in enumerate(src[off:off + n])) + src[off + n:]
                assert got[0] == want, (key.hex(), off, n)  # the reference, against the plain rule
                assert got[1] == got[0] and got[2] == got[0], (key.hex(), off, n)


# ---- build_frame -------------------------------------------------------------------------------

BUILD_LENGTHS = [0, 1, 125, 126, 127, 65535, 65536, 70000]


def _product_frame(payload, opcode, mask, key):
    """the product's host surface has no build_frame of its own; what it builds is a message's
    echo: uvhttp_ws_echo_messages over one delivered frame (opcode 1 / 2, fin = 1)"""
    n = len(payload)
    desc = np.zeros(1, RF.DESC_DT)
    desc[0] = (0, n, 0, 0, opcode, 1, 2, 0, n)
    out, off, _, res = U.echo_messages(payload or b"\0", desc, 0, 1, 0 if mask else 1, 1,
                                       [int.from_bytes(key, "little")], wire_len=n)
    assert res["status"] == 0 and res["n_echoes"] == 1
    return out


@pytest.mark.parametrize("n", BUILD_LENGTHS)
def test_build_frame(R, n):
    payload = RF.gen_bytes(n + 7, n)
    seed = 0xB01D + n
    c = R.ws_ref_conn_new(0, -1, -1, 0, 0, seed)
    try:
        used = 0
        for opcode in range(16):
            for mask in (0, 1):
                for fin in (0, 1):
                    hs = 2 if n < 126 else 4 if n < 65536 else 10
                    total = hs + n + (4 if mask else 0)
                    for cap in (total - 1, total, total + 1):
                        buf = (C.c_uint8 * (cap + 1))()
                        src = (C.c_uint8 * max(1, n)).from_buffer_copy(payload or b"\0")
                        rc = R.ws_ref_build_frame(c, buf, cap, src if n else None, n, opcode, mask, fin)
                        key = RF.key_bytes(seed, used)
                        orc, ob = O.build_frame(payload, opcode, mask, fin, key, cap=cap)
                        assert (rc, bytes(buf)[:max(rc, 0)]) == (orc, ob), (n, opcode, mask, fin, cap)
                        if rc < 0:
                            assert cap < total  # and the refusal came before a key was drawn (:228)
                            continue
                        assert rc == total
                        used += mask
                        if opcode in (1, 2) and fin and cap == total:
                            assert _product_frame(payload, opcode, mask, key) == ob, (n, opcode, mask)
        st = (C.c_uint64 * 8)()
        R.ws_ref_end_state(c, C.byref(st))
        assert st[7] == 4 * used
    finally:
        R.ws_ref_conn_free(c)


# ---- process_data sessions ----------------------------------------------------------------------

MODES = ("one", "frame", "cuts")
BYTE_CUT_SESSIONS = 100
_CENSUS = {}


def _three_way(sess, mode):
    reads = sess.reads(mode)
    ref = RF.run_reference(sess, reads)
    for name, run in (("oracle", RF.run_oracle), ("host", RF.run_host)):
        got = run(sess, reads)
        diff = RF.first_difference(ref, got)
        assert diff is None, "session seed %d (template %d, %s, %s cut): reference != %s at %s" % (
            sess.seed, sess.template, sess.config(), mode, name, diff)
    assert not any(e[0] == "e" for e in ref["events"])  # process_data never calls on_error
    return ref


@pytest.mark.parametrize("block", range(24))
def test_sessions_three_way(R, host_hooks, block):
    """96 sessions of the grammar, each cut three ways; the reference's transcripts feed the census"""
    per = RF.N_SESSIONS // 24
    for seed in range(block * per, (block + 1) * per):
        sess = RF.make_session(seed)
        runs = {mode: _three_way(sess, mode) for mode in MODES}
        _CENSUS[seed] = (sess.side, RF.branches_taken(sess, runs))


def test_sessions_cut_at_every_byte(R, host_hooks):
    done, seed = 0, 0
    while done < BYTE_CUT_SESSIONS:
        sess = RF.make_session(seed)
        seed += 1
        if len(sess.wire) > 600:
            continue
        whole = RF.run_reference(sess, sess.reads("one"))
        cut = _three_way(sess, "bytes")
        # the events do not depend on the cuts while every read succeeds; a failing read is the one
        # whose byte completes the failing header
        if whole["reads"][-1][0] == 0:
            assert cut["events"] == whole["events"] and cut["end"] == whole["end"], sess.seed
        done += 1
    assert seed <= RF.N_SESSIONS


def test_every_branch_occurred(R):
    """the census of test_sessions_three_way: every branch, on every side it exists on"""
    for seed in range(RF.N_SESSIONS):  # (only when run without test_sessions_three_way)
        if seed not in _CENSUS:
            sess = RF.make_session(seed)
            runs = {mode: RF.run_reference(sess, sess.reads(mode)) for mode in MODES}
            _CENSUS[seed] = (sess.side, RF.branches_taken(sess, runs))
    assert len(_CENSUS) >= 2000
    counts = {key: 0 for key in RF.required()}
    for side, took in _CENSUS.values():
        for b in took:
            if (b, side) in counts:
                counts[(b, side)] += 1
    print("branch census:", {"%s/%s" % k: v for k, v in sorted(counts.items())})
    missing = sorted(k for k, v in counts.items() if v == 0)
    assert not missing, "branches the reference never took: %s" % missing


# ---- the committed transcripts ------------------------------------------------------------------

def test_committed_transcripts_are_what_the_reference_gives(R):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, golden)
    try:
        import make_reference_transcripts as maker
    finally:
        sys.path.remove(golden)
    with open(os.path.join(golden, "reference_transcripts.json"), "rb") as f:
        committed = f.read()
    assert maker.render() == committed, ("tests/golden/reference_transcripts.json is stale: run "
                                         "tests/golden/make_reference_transcripts.py")
