"""Host side of uvhttp_tls_gpu_seal_frames: the Python reference (tests/_tls_send_ref.py) against
the oracle's record open, the ABI of the three send-side structs, and the refusal without a
device.  No GPU."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import _oracle as O
import _tls_send_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", range(6))
@pytest.mark.parametrize("max_fragment", [0, 512])
def test_reference_opens_to_the_frames(kind, max_fragment):
    """Each send's reference bytes, opened by the oracle under the send's key and first sequence
    number, give back its frames back to back."""
    rng = random.Random(100 + kind)
    mf = max_fragment or 16384
    totals = [mf - 1, mf, mf + 1, 2 * mf, 2 * mf + 1, 2, 127]
    frames, off = R.build_frames([rng.randbytes(R.payload_len_for(t)) for t in totals] + [b""])
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[kind]), R.make_key(rng, R.KEY_KINDS[(kind + 1) % 6])])
    sends = np.zeros(3, R.TLS_SEND_DT)
    sends["type"] = 23
    sends[0] = (0, 0, len(off) - 1, 0, 23, 0, 0)
    sends[1] = ((1 << 32) - 1, 2, 4, 0, 23, 0, 0)
    sends[2] = (7, 1, 5, 1, 23, 0, 0)
    ref = R.seal_frames_ref(frames, off, sends, keys, max_fragment)
    assert not ref["failed"] and ref["summary"][0]["n_failed"] == 0
    assert b"".join(ref["per_send"]) == ref["out"]
    assert int(ref["summary"][0]["out_bytes"]) == len(ref["out"])
    for i, s in enumerate(sends):
        a, b = int(off[s["first_frame"]]), int(off[s["first_frame"] + s["n_frames"]])
        r = ref["results"][i]
        assert ref["plain"][i] == frames[a:b] and int(r["plain_len"]) == b - a
        wire = np.frombuffer(ref["per_send"][i], np.uint8)
        out = np.zeros(wire.size + 16, np.uint8)
        n = O.tls_open_stream_bytes(keys[s["key"]:s["key"] + 1], int(s["seq"]), wire, out)
        assert out[:n].tobytes() == frames[a:b]
        recs = ref["records"][r["first_record"]:r["first_record"] + r["n_records"]]
        assert (recs["seq"] == int(s["seq"]) + np.arange(len(recs), dtype=np.uint64)).all()
        assert int(r["next_seq"]) == int(s["seq"]) + len(recs)
        assert recs["plain_len"].max() <= mf and int(recs["plain_len"].sum()) == b - a


def test_reference_failures():
    rng = random.Random(7)
    frames, off = R.build_frames([rng.randbytes(n) for n in (10, 300, 0, 700)])
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[0]), R.make_key(rng, R.KEY_KINDS[5])])
    keys[1]["key_len"] = 24  # invalid
    sends = np.zeros(5, R.TLS_SEND_DT)
    sends["type"] = 23
    sends["n_frames"] = 2
    sends["key"] = [0, 1, 2, 0, 0]
    sends["first_frame"] = [0, 0, 0, 3, 2]
    ref = R.seal_frames_ref(frames, off, sends, keys, 256)
    assert list(ref["results"]["status"]) == [0, O.REC_KEY, O.REC_KEY, R.REC_RANGE, 0]
    assert ref["summary"][0]["n_failed"] == 3
    short = R.seal_frames_ref(frames, off, sends, keys, 256, out_cap=len(ref["out"]) - 1)
    assert list(short["results"]["status"]) == [O.REC_CAPACITY, O.REC_KEY, O.REC_KEY, R.REC_RANGE,
                                                O.REC_CAPACITY]
    assert short["out"] == b"" and short["summary"][0]["n_failed"] == 5
    assert short["summary"][0]["out_bytes"] == ref["summary"][0]["out_bytes"]
    assert short["summary"][0]["n_records"] == ref["summary"][0]["n_records"] == len(ref["records"])


def test_struct_sizes_and_layout():
    """The numpy layouts are the header's: sizes through ctypes, field order from the text."""
    class Send(C.Structure):
        _fields_ = [("seq", C.c_uint64), ("first_frame", C.c_uint32), ("n_frames", C.c_uint32),
                    ("key", C.c_uint32), ("type", C.c_uint8), ("reserved", C.c_uint8 * 3),
                    ("reserved2", C.c_uint64)]

    class Result(C.Structure):
        _fields_ = [("out_off", C.c_uint64), ("out_len", C.c_uint64), ("next_seq", C.c_uint64),
                    ("first_record", C.c_uint32), ("n_records", C.c_uint32),
                    ("status", C.c_int32), ("reserved", C.c_uint32), ("plain_len", C.c_uint64)]

    class Summary(C.Structure):
        _fields_ = [("out_bytes", C.c_uint64), ("n_records", C.c_uint32),
                    ("n_failed", C.c_uint32), ("reserved", C.c_uint64 * 2)]

    hdr = open(os.path.join(REPO, "include", "uvhttp_tls_amd.h")).read()
    for cls, dt, name in ((Send, R.TLS_SEND_DT, "uvhttp_tls_send_t"),
                          (Result, R.TLS_SEND_RESULT_DT, "uvhttp_tls_send_result_t"),
                          (Summary, R.TLS_SEND_SUMMARY_DT, "uvhttp_tls_send_summary_t")):
        assert C.sizeof(cls) == dt.itemsize
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == dt.fields[fname][1], (name, fname)
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = re.findall(r"(\w+)(?:\[\d+\])?;", body)
        assert declared == [f for f, _ in cls._fields_], name
    assert "#define UVHTTP_TLS_REC_ERR_RANGE (-8)" in hdr
    import uvhttp_amd as U
    assert (U.TLS_SEND_BYTES, U.TLS_SEND_RESULT_BYTES, U.TLS_SEND_SUMMARY_BYTES) == (32, 48, 32)


def test_no_engine_is_refused():
    """There is no engine without a device: ENODEV there, EINVAL for a null engine beside one."""
    import torch
    import uvhttp_amd as U
    z = C.c_void_p(None)
    rc = U.lib().uvhttp_tls_gpu_seal_frames(None, z, 0, z, 0, z, 0, z, 0, 0, z, 0, z, z, z, 0, z)
    assert rc == (-1 if torch.cuda.is_available() else -2)
