"""uvhttp_ws_close_frames, the host twin of uvhttp_ws_gpu_close_frames_streams
(include/uvhttp_ws_amd.h): the server's own 1002 / 1007 CLOSE frames for a decoded batch, against
the Python restatement of the rule and the oracle's build_frame (tests/_close_ref.py).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _close_ref as CR
import uvhttp_amd as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(st, res, n, ver=None, rep=None, en=None, keys=None, out_cap=None, clear=(), stride=8):
    """one twin call against the reference -> the reference"""
    want_clear = [c.copy() for c in clear]
    ref = CR.close_frames_ref(st, res, n, ver, rep, en, keys, out_cap, want_clear)
    got_clear = [c.copy() for c in clear]
    out, off, runs, conn, summ = U.close_frames(
        st, res, n, ver, rep, en, keys, out_cap=out_cap, run_stride=stride, clear_runs=got_clear,
        clear_stride=[c.strides[0] for c in got_clear])
    assert out == ref["out"]
    assert [int(x) for x in off] == ref["out_off"]
    assert [(int(r[0]), int(r[1])) for r in runs[:n]] == ref["runs"]
    assert conn == ref["conn"] and summ == ref["summary"]
    for g, w in zip(got_clear, want_clear):
        assert np.array_equal(g, w)
    return ref


def test_every_rule_once():
    st, res, ver, rep, en, keys, want = CR.rule_cases()
    ref = _check(st, res, len(want), ver, rep, en, keys)
    assert [c["code"] for c in ref["conn"]] == want
    assert ref["summary"]["n_1002"] == want.count(1002) > 0 and ref["summary"]["n_1007"] == want.count(1007) > 0
    # the same without the optional inputs: no verdict -> no 1007, no reply results -> closed unseen
    _check(st, res, len(want), None, rep, en, keys)
    _check(st, res, len(want), ver, None, en, keys)
    _check(st, res, len(want), ver, rep, None, keys)


def test_frame_bytes_are_the_references():
    """byte for byte what uvhttp_ws_close -> uvhttp_ws_build_frame(opcode 8, mask = !is_server, fin 1)
    writes: 88 10 03 EA "protocol error" for a server; a client adds the mask bit, the key, the mask"""
    st, res, ver, rep, en, keys = CR.tables(4)
    st["is_server"] = [1, 0, 1, 0]
    res["first_status"] = [-1, -4, 0, 0]
    ver["status"] = [0, 0, 1, 1]
    keys[:] = [0, 0x44332211, 0, 0xA1B2C3D4]
    ref = _check(st, res, 4, ver, rep, en, keys)
    f = [ref["out"][ref["out_off"][j]:ref["out_off"][j + 1]] for j in range(4)]
    assert f[0] == bytes([0x88, 16, 0x03, 0xEA]) + b"protocol error"
    plain = bytes([0x03, 0xEA]) + b"protocol error"
    k = bytes([0x11, 0x22, 0x33, 0x44])
    assert f[1] == bytes([0x88, 0x90]) + k + bytes(b ^ k[i & 3] for i, b in enumerate(plain))
    assert f[2] == bytes([0x88, 2, 0x03, 0xEF])
    assert f[3] == bytes([0x88, 0x82, 0xD4, 0xC3, 0xB2, 0xA1, 0x03 ^ 0xD4, 0xEF ^ 0xC3])
    assert [c["out_len"] for c in ref["conn"]] == [18, 22, 4, 8]


def test_client_streams_without_keys():
    st, res, ver, rep, en, keys = CR.tables(5)
    st["is_server"] = [0, 1, 0, 0, 1]
    res["first_status"] = [-2, -2, 0, 0, 0]
    ver["status"] = [0, 0, 1, 0, 1]
    ref = _check(st, res, 5, ver, rep, en, None)
    assert [c["status"] for c in ref["conn"]] == [CR.NO_KEYS, 0, CR.NO_KEYS, 0, 0]
    assert [c["code"] for c in ref["conn"]] == [0, 1002, 0, 0, 1007]
    assert ref["runs"] == [(0, 0), (0, 1), (1, 0), (1, 0), (1, 1)]


def test_capacity_one_byte_short_then_the_reported_size():
    st, res, ver, rep, en, keys, want = CR.rule_cases()
    n = len(want)
    full = CR.close_frames_ref(st, res, n, ver, rep, en, keys)
    clear = [np.full((n, 2), 7, np.uint32)]
    short = _check(st, res, n, ver, rep, en, keys, out_cap=len(full["out"]) - 1, clear=clear)
    assert short["summary"]["status"] == CR.ERR_CAPACITY and short["out"] == b""
    assert {k: short["summary"][k] for k in ("out_bytes", "n_closes", "n_1002", "n_1007")} == \
        {k: full["summary"][k] for k in ("out_bytes", "n_closes", "n_1002", "n_1007")}
    assert all(c == {"code": 0, "out_len": 0, "status": CR.ERR_CAPACITY} for c in short["conn"])
    again = _check(st, res, n, ver, rep, en, keys, out_cap=short["summary"]["out_bytes"])
    assert again["out"] == full["out"] and again["summary"]["status"] == CR.OK


def test_clear_runs():
    """a 1007 connection's runs in the named tables lose their frames; nobody else's change, the
    first word stays, and bytes between the runs (a 32-byte send table) are left alone"""
    st, res, ver, rep, en, keys, want = CR.rule_cases()
    n = len(want)
    echo = np.arange(2 * n, dtype=np.uint32).reshape(n, 2) + 1
    sends = np.arange(8 * n, dtype=np.uint32).reshape(n, 8) + 100   # the run at words 2, 3
    got_e, got_s = echo.copy(), sends.copy()
    U.close_frames(st, res, n, ver, rep, en, keys, clear_runs=[got_e, got_s[:, 2:]],
                   clear_stride=[8, 32])
    for s in range(n):
        if want[s] == 1007:
            echo[s][1] = 0
            sends[s][3] = 0
    assert np.array_equal(got_e, echo) and np.array_equal(got_s, sends)
    assert (got_e[:, 1] == 0).sum() == want.count(1007)
    # through the reference too
    _check(st, res, n, ver, rep, en, keys, clear=[np.full((n, 2), 9, np.uint32), np.full((n, 4), 5, np.uint32)])


@pytest.mark.parametrize("seed", range(40))
def test_seeded_mixes(seed):
    st, res, ver, rep, en, keys = CR.mixed_case(7000 + seed)
    n = len(st)
    clear = [np.full((n, 2), 3, np.uint32)] if seed & 1 else []
    ref = _check(st, res, n, ver if seed % 5 else None, rep if seed % 7 else None, en if seed % 3 else None,
                 keys if seed % 4 else None, clear=clear, stride=8 if seed & 2 else 32)
    if seed % 6 == 0 and ref["out"]:
        _check(st, res, n, ver if seed % 5 else None, rep if seed % 7 else None, en if seed % 3 else None,
               keys if seed % 4 else None, out_cap=len(ref["out"]) - 1, clear=clear)


def test_no_connections_and_bad_arguments():
    st, res, ver, rep, en, keys = CR.tables(1)
    ref = _check(st, res, 0)
    assert ref["out_off"] == [0] and ref["summary"]["n_closes"] == 0
    with pytest.raises(ValueError):
        U.close_frames(st, res, 1, flags=1)
    with pytest.raises(ValueError):
        U.close_frames(st, res, 1, run_stride=6)
    with pytest.raises(ValueError):
        U.close_frames(st, res, 1, clear_runs=[np.zeros((1, 2), np.uint32)] * 5, clear_stride=[8] * 5)
    with pytest.raises(ValueError):
        U.close_frames(st, res, 1, clear_runs=[np.zeros((1, 2), np.uint32)], clear_stride=[4])


def test_twin_under_asan_ubsan():
    """tests/c/close_check.c: the twin compiled with -fsanitize=address,undefined into a program of
    its own, every output in a heap block of exactly its size, seeded mixes of every input"""
    import subprocess
    subprocess.run(["make", "-C", REPO, "tests/c/_build/close_check"], check=True,
                   stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(REPO, "tests", "c", "_build", "close_check"), "300", "7"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert p.stdout.startswith("ok 300 ")


def test_struct_layouts():
    hdr = open(os.path.join(REPO, "include", "uvhttp_ws_amd.h")).read()
    for cls, dt, name in ((U.CloseConn, CR.CLOSE_CONN_DT, "uvhttp_ws_close_conn_t"),
                          (U.CloseSummary, CR.CLOSE_SUMMARY_DT, "uvhttp_ws_close_summary_t")):
        assert C.sizeof(cls) == dt.itemsize
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == dt.fields[fname][1], (name, fname)
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == [f for f, _ in cls._fields_], name
    for text in ("#define UVHTTP_WS_CLOSE_ERR_CAPACITY 1", "#define UVHTTP_WS_CLOSE_NO_KEYS 3",
                 "#define UVHTTP_WS_CLOSE_MAX_CLEAR 4"):
        assert text in hdr
    assert (U.CLOSE_ERR_CAPACITY, U.CLOSE_NO_KEYS, U.CLOSE_MAX_CLEAR) == (1, 3, 4)
    assert CR.VERDICT_DT.itemsize == C.sizeof(U.Utf8ConnVerdict)
    assert CR.REPLY_CONN_DT.itemsize == C.sizeof(U.ReplyConn)
    assert CR.VERDICT_DT.fields["status"][1] == U.Utf8ConnVerdict.status.offset
    assert CR.REPLY_CONN_DT.fields["closed"][1] == U.ReplyConn.closed.offset
