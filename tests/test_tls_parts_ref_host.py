"""Host side of uvhttp_tls_gpu_seal_parts: the Python reference (tests/_tls_parts_ref.py) pinned
to seal_frames_ref and to the oracle's record open, the ABI of uvhttp_tls_part_t, and the refusal
without a device.  No GPU."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import _oracle as O
import _tls_parts_ref as P
import _tls_send_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sends(rows):
    s = np.zeros(len(rows), R.TLS_SEND_DT)
    for i, (seq, key) in enumerate(rows):
        s[i] = (seq, 0, 0, key, 23, 0, 0)
    return s


@pytest.mark.parametrize("max_fragment", [0, 16, 512])
def test_one_part_is_seal_frames(max_fragment):
    rng = random.Random(3)
    frames, off = R.build_frames([rng.randbytes(n) for n in (0, 1, 15, 16, 17, 600, 20000)])
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[k]) for k in (0, 2, 3)])
    sends = _sends([(5, 0), ((1 << 32) - 1, 1), (9, 2), (1, 7)])
    runs = [(0, 7), (2, 3), (7, 0), (0, 1)]
    sends["first_frame"], sends["n_frames"] = [r[0] for r in runs], [r[1] for r in runs]
    want = R.seal_frames_ref(frames, off, sends, keys, max_fragment)
    got = P.seal_parts_ref(frames, [P.part(0, len(frames), off, runs)], sends, keys, max_fragment)
    for k in ("out", "per_send", "plain", "failed"):
        assert got[k] == want[k], k
    for k in ("results", "summary", "records"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert list(got["results"]["status"]) == [0, 0, 0, O.REC_KEY]


# TLS 1.3 AES-GCM, TLS 1.3 ChaCha20-Poly1305, TLS 1.2 AES-GCM
@pytest.mark.parametrize("kind", [0, 2, 3])
def test_reference_opens_with_consecutive_sequence_numbers(kind):
    """Three parts at unaligned bases, the middle one listed twice around an excluded frame: each
    send's bytes, opened by the oracle from the send's seq on, are its runs' frames in part order;
    a record never spans two frames; src_off points into the arena."""
    rng = random.Random(50 + kind)
    mf = 64
    a_frames, a_off = R.build_frames([rng.randbytes(n) for n in (10, 0, 200, 63)])
    b_frames, b_off = R.build_frames([rng.randbytes(n) for n in (62, 64, 130)])
    c_frames, c_off = R.build_frames([rng.randbytes(n) for n in (5,)])
    gap = b"\xEE" * 3
    arena = gap + a_frames + gap + b_frames + gap + c_frames
    bases = [3, 6 + len(a_frames), 9 + len(a_frames) + len(b_frames)]
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[kind]), R.make_key(rng, R.KEY_KINDS[(kind + 1) % 6])])
    sends = _sends([((1 << 32) - 2, 0), (77, 1), (0, 0)])
    parts = [P.part(bases[0], len(a_frames) + 2, a_off, [(0, 4), (1, 2), (4, 0)]),
             P.part(bases[1], len(b_frames), b_off, [(0, 1), (0, 0), (0, 0)]),   # before the excluded frame
             P.part(bases[1], len(b_frames), b_off, [(2, 1), (0, 3), (3, 0)]),   # and after it
             P.part(bases[2], len(c_frames), c_off, [(0, 1), (0, 0), (1, 0)])]
    ref = P.seal_parts_ref(arena, parts, sends, keys, mf)
    assert not ref["failed"] and list(ref["results"]["status"]) == [0, 0, 0]

    def fr(buf, off, lo, hi):
        return buf[int(off[lo]):int(off[hi])]
    want = [fr(a_frames, a_off, 0, 4) + fr(b_frames, b_off, 0, 1) + fr(b_frames, b_off, 2, 3) + c_frames,
            fr(a_frames, a_off, 1, 3) + b_frames, b""]
    for i, s in enumerate(sends):
        r = ref["results"][i]
        wire = np.frombuffer(ref["per_send"][i], np.uint8)
        out = np.zeros(wire.size + 16, np.uint8)
        n = O.tls_open_stream_bytes(keys[s["key"]:s["key"] + 1], int(s["seq"]), wire, out)
        assert out[:n].tobytes() == want[i] == ref["plain"][i]
        assert int(r["plain_len"]) == len(want[i])
        recs = ref["records"][r["first_record"]:r["first_record"] + r["n_records"]]
        assert (recs["seq"] == int(s["seq"]) + np.arange(len(recs), dtype=np.uint64)).all()
        assert b"".join(arena[int(q["src_off"]):int(q["src_off"]) + int(q["plain_len"])] for q in recs) == want[i]
    # send 0's frames: 10 + 2 | 0 + 2 | 200 + 4 | 63 + 2, then 62 + 2, 130 + 4, then 5 + 2
    assert list(ref["records"]["plain_len"][:ref["results"][0]["n_records"]]) == \
        [12, 2, 64, 64, 64, 12, 64, 1, 64, 64, 64, 6, 7]
    assert ref["results"][2]["n_records"] == 0 and ref["results"][2]["next_seq"] == 0


def test_reference_failures():
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
    ref = P.seal_parts_ref(arena, parts, sends, keys, 128)
    # the key error comes before the range error; the range error of the last part alone fails
    # the send; the bad frame harms only the send that names it
    assert list(ref["results"]["status"]) == [0, O.REC_KEY, R.REC_RANGE, R.REC_RANGE, 0]
    assert list(ref["results"]["next_seq"]) == [1 + 5, 2, 3, 4, 5 + 1]
    assert ref["summary"][0]["n_failed"] == 3
    short = P.seal_parts_ref(arena, parts, sends, keys, 128, max_records=len(ref["records"]) - 1)
    assert list(short["results"]["status"]) == [O.REC_CAPACITY, O.REC_KEY, R.REC_RANGE, R.REC_RANGE,
                                                O.REC_CAPACITY]
    assert short["out"] == b"" and short["summary"][0]["n_failed"] == 5
    assert short["summary"][0]["out_bytes"] == ref["summary"][0]["out_bytes"]


def test_part_struct_layout():
    import uvhttp_amd as U
    hdr = open(os.path.join(REPO, "include", "uvhttp_tls_amd.h")).read()
    assert "#define UVHTTP_TLS_MAX_PARTS 8" in hdr and U.TLS_MAX_PARTS == 8
    body = re.search(r"typedef struct \{([^}]*)\} uvhttp_tls_part_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [f for f, _ in U.TlsPart._fields_]
    assert C.sizeof(U.TlsPart) == 40
    assert [getattr(U.TlsPart, f).offset for f, _ in U.TlsPart._fields_] == [0, 8, 16, 24, 32, 36]


def test_no_engine_is_refused():
    """There is no engine without a device: ENODEV there, EINVAL for a null engine beside one."""
    import torch
    import uvhttp_amd as U
    z = C.c_void_p(None)
    tab = (U.TlsPart * 1)()
    rc = U.lib().uvhttp_tls_gpu_seal_parts(None, z, 0, tab, 1, z, 0, z, 0, 0, z, 0, z, z, z, 0, z)
    assert rc == (-1 if torch.cuda.is_available() else -2)
