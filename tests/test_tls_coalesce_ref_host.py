"""Host side of uvhttp_tls_gpu_seal_parts_coalesced: the Python reference
(tests/_tls_coalesce_ref.py) pinned to the oracle's record open, to seal_parts_ref's streams and to
seal_parts_ref's bytes where the two calls must agree; the declaration and the refusal without a
device.  No GPU."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import _oracle as O
import _tls_coalesce_ref as K
import _tls_parts_ref as P
import _tls_send_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sends(rows):
    s = np.zeros(len(rows), R.TLS_SEND_DT)
    for i, (seq, key) in enumerate(rows):
        s[i] = (seq, 0, 0, key, 23, 0, 0)
    return s


def _batch(rng, kind):
    a_frames, a_off = R.build_frames([rng.randbytes(n) for n in (10, 0, 200, 63)])
    b_frames, b_off = R.build_frames([rng.randbytes(n) for n in (62, 64, 130)])
    c_frames, c_off = R.build_frames([rng.randbytes(n) for n in (5,)])
    gap = b"\xEE" * 3
    arena = gap + a_frames + gap + b_frames + gap + c_frames
    bases = [3, 6 + len(a_frames), 9 + len(a_frames) + len(b_frames)]
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[kind]), R.make_key(rng, R.KEY_KINDS[(kind + 1) % 6])])
    sends = _sends([((1 << 32) - 2, 0), (77, 1), (0, 0)])
    parts = [P.part(bases[0], len(a_frames) + 2, a_off, [(0, 4), (1, 2), (4, 0)]),
             P.part(bases[1], len(b_frames), b_off, [(0, 1), (0, 0), (0, 0)]),   # before an excluded frame
             P.part(bases[1], len(b_frames), b_off, [(2, 1), (0, 3), (3, 0)]),   # and after it
             P.part(bases[2], len(c_frames), c_off, [(0, 1), (0, 0), (1, 0)])]
    return arena, parts, sends, keys


@pytest.mark.parametrize("max_fragment", [1, 16, 64, 0])
@pytest.mark.parametrize("kind", range(6))
def test_reference_opens_to_the_streams_of_seal_parts(kind, max_fragment):
    """every send's records, opened by the oracle from the send's seq on, give its stream; the
    stream is seal_parts_ref's plaintext; the send has ceil(B / mf) records, all full but the last"""
    rng = random.Random(700 + kind)
    arena, parts, sends, keys = _batch(rng, kind)
    mf = max_fragment or 16384
    ref = K.seal_parts_coalesced_ref(arena, parts, sends, keys, max_fragment)
    per_frame = P.seal_parts_ref(arena, parts, sends, keys, max_fragment)
    assert not ref["failed"] and list(ref["results"]["status"]) == [0, 0, 0]
    assert ref["plain"] == per_frame["plain"] and ref["plain"][2] == b"" and len(ref["plain"][0]) > 256
    for i, s in enumerate(sends):
        r, stream = ref["results"][i], ref["plain"][i]
        wire = np.frombuffer(ref["per_send"][i], np.uint8)
        out = np.zeros(wire.size + 16, np.uint8)
        n = O.tls_open_stream_bytes(keys[s["key"]:s["key"] + 1], int(s["seq"]), wire, out)
        assert out[:n].tobytes() == stream
        assert int(r["n_records"]) == (len(stream) + mf - 1) // mf and int(r["plain_len"]) == len(stream)
        assert int(r["next_seq"]) == (int(s["seq"]) + int(r["n_records"])) & 0xFFFFFFFFFFFFFFFF
        recs = ref["records"][r["first_record"]:r["first_record"] + r["n_records"]]
        assert (recs["seq"] == int(s["seq"]) + np.arange(len(recs), dtype=np.uint64)).all()
        assert list(recs["plain_len"]) == [mf] * (len(recs) - 1) + [len(stream) - mf * (len(recs) - 1)][:len(recs)]
        assert (recs["src_off"] - recs["out_off"] == K.header_len(keys[s["key"]])).all()
        assert int(r["out_len"]) == len(stream) + len(recs) * R.overhead(keys[s["key"]])
    assert int(ref["summary"][0]["n_records"]) <= int(per_frame["summary"][0]["n_records"])


@pytest.mark.parametrize("kind", range(6))
def test_one_short_frame_per_send_is_seal_parts_byte_for_byte(kind):
    """a stream of one frame no longer than max_fragment is cut the same by both calls: the bytes of
    out, results and summary are equal; the record tables differ only in src_off"""
    rng = random.Random(800 + kind)
    sizes = [1, 15, 16, 17, 61, 62]  # + 2 header bytes: the longest frame is exactly max_fragment
    frames, off = R.build_frames([rng.randbytes(n) for n in sizes])
    arena = b"\xEE" * 5 + frames
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[(kind + i) % 6]) for i in range(3)])
    sends = _sends([(rng.getrandbits(40), i % 3) for i in range(len(sizes))])
    parts = [P.part(5, len(frames), off, [(i, 1) for i in range(len(sizes))]),
             P.part(5, len(frames), off, [(i, 0) for i in range(len(sizes))])]
    got = K.seal_parts_coalesced_ref(arena, parts, sends, keys, 64)
    want = P.seal_parts_ref(arena, parts, sends, keys, 64)
    assert got["out"] == want["out"] and got["per_send"] == want["per_send"] and got["plain"] == want["plain"]
    assert got["results"].tobytes() == want["results"].tobytes()
    assert got["summary"].tobytes() == want["summary"].tobytes()
    for f in ("out_off", "seq", "plain_len", "key", "type"):
        assert (got["records"][f] == want["records"][f]).all(), f


def test_reference_failures_and_capacity():
    rng = random.Random(8)
    a_frames, a_off = R.build_frames([rng.randbytes(n) for n in (10, 300)])
    b_frames, b_off = R.build_frames([rng.randbytes(n) for n in (20, 40, 60)])
    arena = a_frames + b_frames
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[0]), R.make_key(rng, R.KEY_KINDS[5])])
    keys[1]["key_len"] = 24  # invalid
    bad_off = b_off.copy()
    bad_off[2] = b_off[1] - 1  # frame 1 of part b ends before it begins
    sends = _sends([(1, 0), (2, 1), (3, 0), (4, 0), (5, 0)])
    parts = [P.part(0, len(a_frames), a_off, [(0, 2), (0, 3), (0, 2), (0, 1), (2, 0)]),
             P.part(len(a_frames), len(b_frames), bad_off, [(0, 1), (0, 4), (2, 2), (1, 1), (2, 1)])]
    ref = K.seal_parts_coalesced_ref(arena, parts, sends, keys, 128)
    # the statuses are seal_parts'; the good sends' 338 and 105 bytes make 3 + 1 records, not 5 + 1
    assert list(ref["results"]["status"]) == list(P.seal_parts_ref(arena, parts, sends, keys, 128)["results"]["status"])
    assert list(ref["results"]["status"]) == [0, O.REC_KEY, R.REC_RANGE, R.REC_RANGE, 0]
    assert list(ref["results"]["next_seq"]) == [1 + 3, 2, 3, 4, 5 + 1]
    assert list(ref["results"]["out_len"][[1, 2, 3]]) == [0, 0, 0] and ref["summary"][0]["n_failed"] == 3
    for cap in (dict(max_records=3), dict(out_cap=len(ref["out"]) - 1)):
        short = K.seal_parts_coalesced_ref(arena, parts, sends, keys, 128, **cap)
        assert list(short["results"]["status"]) == [O.REC_CAPACITY, O.REC_KEY, R.REC_RANGE, R.REC_RANGE,
                                                    O.REC_CAPACITY]
        assert short["out"] == b"" and len(short["records"]) == 0 and short["summary"][0]["n_failed"] == 5
        assert short["summary"][0]["out_bytes"] == len(ref["out"]) and short["summary"][0]["n_records"] == 4
        assert list(short["results"]["next_seq"]) == [1, 2, 3, 4, 5]


def test_declared_beside_seal_parts():
    """the header declares the call with seal_parts' parameter list, and the ctypes table mirrors it"""
    import re
    import uvhttp_amd as U
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uvhttp_tls_amd.h")).read(), flags=re.S)
    a = re.search(r"int uvhttp_tls_gpu_seal_parts\(([^)]*)\)", hdr).group(1)
    b = re.search(r"int uvhttp_tls_gpu_seal_parts_coalesced\(([^)]*)\)", hdr).group(1)
    assert " ".join(a.split()) == " ".join(b.split())
    L = U.lib()
    assert L.uvhttp_tls_gpu_seal_parts_coalesced.argtypes == L.uvhttp_tls_gpu_seal_parts.argtypes
    assert hasattr(U.TlsEngine, "seal_parts_coalesced")


def test_no_engine_is_refused():
    """There is no engine without a device: ENODEV there, EINVAL for a null engine beside one."""
    import torch
    import uvhttp_amd as U
    z = C.c_void_p(None)
    tab = (U.TlsPart * 1)()
    rc = U.lib().uvhttp_tls_gpu_seal_parts_coalesced(None, z, 0, tab, 1, z, 0, z, 0, 0, z, 0, z, z, z, 0, z)
    assert rc == (-1 if torch.cuda.is_available() else -2)
