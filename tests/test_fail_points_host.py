"""uvhttp_ws_fail_points, the host twin of uvhttp_ws_gpu_fail_points_streams
(include/uvhttp_ws_amd.h): the frame at which each connection is failed and the rewritten result
and verdict tables, against the Python restatement of the rule (tests/_fail_ref.py), and the
existing host twins of the send passes over the rewritten tables against their own references
over the connection's bytes before the cut.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _close_ref as CR
import _echo_ref as ER
import _fail_ref as F
import _relay_ref as RL
import _replies_ref as RR
import uvhttp_amd as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(wire, desc, max_frames, res, n, ver=None, en=None, flags=F.CHECK_CLOSE, wire_len=None):
    """one twin call, out of place and in place, against the reference -> the reference"""
    ref = F.fail_points_ref(wire, desc, max_frames, res, n, ver, en, flags, wire_len)
    want = F.ref_bytes(ref, n)
    res_in, ver_in = res.copy(), None if ver is None else ver.copy()
    got = U.fail_points(wire, desc, max_frames, res, n, ver, en, flags, wire_len=wire_len)
    assert F.as_bytes(res) == F.as_bytes(res_in) and F.as_bytes(ver) == F.as_bytes(ver_in), "inputs written"
    got = tuple(None if g is None else g.tobytes()[:len(w)] for g, w in zip(got, want))
    assert got == want
    r2, v2 = res.copy(), None if ver is None else ver.copy()
    _, _, f2, s2 = U.fail_points(wire, desc, max_frames, r2, n, v2, en, flags, in_place=True, wire_len=wire_len)
    assert (F.as_bytes(r2[:n]), None if v2 is None else F.as_bytes(v2[:n]), f2.tobytes()[:16 * n], s2.tobytes()) == want
    return ref


@pytest.fixture(scope="module")
def rules():
    return F.rule_cases()


def test_every_rule_once(rules):
    b, names = rules
    res, ver, fail, summ = _check(*b.tables(), b.ver, b.en)
    for s, (name, want) in enumerate(zip(names, b.wants)):
        reason, rel, code, status = want
        frame = F.NONE if rel is None else b.first[s] + rel
        if reason == F.R_DECODE:
            frame = b.first[s] + b.nd[s]
        assert (int(fail[s]["reason"]), int(fail[s]["frame"]), int(fail[s]["code"]), int(fail[s]["status"])) == \
            (reason, frame, code, status), name
        if rel is not None:
            assert int(res[s]["n_delivered"]) == rel and int(fail[s]["n_dropped"]) == b.nd[s] - rel, name
            assert int(res[s]["first_status"]) == (F.ERR_UTF8 if reason == F.R_UTF8 else F.ERR_CLOSE), name
    for reason, key in ((F.R_DECODE, "n_decode"), (F.R_UTF8, "n_utf8"), (F.R_CLOSE_LEN, "n_close_len"),
                        (F.R_CLOSE_CODE, "n_close_code")):
        assert int(summ[key][0]) == sum(1 for w in b.wants if w[0] == reason) > 0
    assert int(summ["n_bad_range"][0]) == 2
    # the verdict over the kept frames: a bad CLOSE at or before the invalid frame, or one after the CLOSE
    for name in ("utf8 after the close", "both on one frame", "bad close before invalid text"):
        s = names.index(name)
        assert b.ver[s]["status"] == CR.UTF8_INVALID and ver[s]["status"] == CR.UTF8_VALID, name
        assert ver[s]["first_invalid"] == F.NONE and ver[s]["n_text_frames"] == b.ver[s]["n_text_frames"]
    # the same without the optional inputs and without the flag
    _check(*b.tables(), None, b.en)
    _check(*b.tables(), b.ver, None)
    noflag = _check(*b.tables(), b.ver, b.en, flags=0)
    assert int(noflag[3]["n_close_len"][0]) == int(noflag[3]["n_close_code"][0]) == int(noflag[3]["n_bad_range"][0]) == 0
    # fewer descriptors than the results name: the considered range is clipped as the echo clips it
    for mf in (0, 1, b.max_frames // 2, b.max_frames - 1):
        _check(b.wire, b.desc, mf, b.res, b.n, b.ver, b.en)


def test_nothing_fails_nothing_changes():
    b = F.clean_batch()
    for flags in (0, F.CHECK_CLOSE):
        res, ver, fail, summ = _check(*b.tables(), b.ver, b.en, flags=flags)
        assert F.as_bytes(res[:b.n]) == F.as_bytes(b.res[:b.n]) and F.as_bytes(ver[:b.n]) == F.as_bytes(b.ver[:b.n])
        assert (fail["reason"] == 0).all() and (fail["frame"][:b.n] == F.NONE).all()
        assert summ.tobytes() == np.array([(0, 0, 0, 0, 0, 0, F.NONE)], F.SUMMARY_DT).tobytes()
    out = U.fail_points(*b.tables(), b.ver, b.en, F.CHECK_CLOSE)
    assert out[0].tobytes()[:64 * b.n] == F.as_bytes(b.res[:b.n]) and out[1].tobytes()[:16 * b.n] == F.as_bytes(b.ver[:b.n])


def _truncated(b, fail):
    """every connection's frames up to its cut"""
    return [c[:int(fail[s]["frame"]) - b.first[s]] if fail[s]["reason"] >= F.R_UTF8 else c for s, c in enumerate(b.conns)]


def _judged(b):
    """the batch without its caller errors (the references know neither a disabled connection's
    frames nor a forced status)"""
    keep = [s for s in range(b.n) if b.en[s] and int(b.res[s]["first_status"]) not in F.CALL_FAILED and
            b.wants[s][3] == F.OK]
    rows = F.rule_rows()
    return F.Batch([rows[s][1] for s in keep], [rows[s][2] for s in keep], None, [rows[s][4] for s in keep])


def test_send_passes_over_the_rewritten_tables(rules):
    """what the existing host twins build from the rewritten tables == what their references build
    from the connection's bytes ending just before the cut frame"""
    b = _judged(rules[0])
    n = b.n
    res, ver, fail, _ = _check(*b.tables(), b.ver, b.en)
    assert sum(1 for s in range(n) if fail[s]["reason"] >= F.R_UTF8) >= 10
    cut = _truncated(b, fail)
    first, nd = b.first, [int(x) for x in res["n_delivered"][:n]]
    # echo
    assert ER.host_batch(U, b.wire, b.desc, first, nd, pending=b.pending) == ER.expected_batch(cut, pending=b.pending)
    # replies: no PONG for a PING after the cut, no echo of a bad CLOSE, `closed` unset
    got_r = RR.host_batch(U, b.wire, b.desc, first, nd)
    assert got_r == RR.expected_batch(cut)
    whole = RR.host_batch(U, b.wire, b.desc, first, b.nd)
    assert whole["summary"]["n_replies"] > got_r["summary"]["n_replies"]
    # relay: rooms of several senders, an offender's message in none
    room = [s % 5 for s in range(n)]
    got_l = RL.host_batch(U, b.wire, b.desc, b.max_frames, b.st, res, room, 5, room, pending=b.pending)
    assert got_l == RL.expected(cut, room, 5, room, pending=b.pending, max_frames_out=b.max_frames)
    assert BAD_IN(RL.host_batch(U, b.wire, b.desc, b.max_frames, b.st, b.res, room, 5, room, pending=b.pending)["out"])
    assert not BAD_IN(got_l["out"])
    # close: the code the fail entry names
    rep = np.zeros(n, CR.REPLY_CONN_DT)
    rep["closed"] = [c["closed"] for c in got_r["conn"]]
    closes = CR.close_frames_ref(b.st, res, n, ver, rep)
    assert [c["code"] for c in closes["conn"]] == [int(x) for x in fail["code"][:n]]
    assert U.close_frames(b.st, res, n, ver, rep)[3] == closes["conn"]


def BAD_IN(out):
    return F.BAD in out


@pytest.mark.parametrize("seed", range(40))
def test_seeded_tables(seed):
    specs, rng = F.seeded_specs(3000 + seed)
    wire, desc, mf, res, n, ver, en = F.synth_batch(specs, rng, gap=seed % 3)
    _, _, _, summ = _check(wire, desc, mf, res, n, ver if seed % 5 else None, en if seed % 3 else None,
                           F.CHECK_CLOSE if seed % 4 else 0)
    if seed % 5 and seed % 3 and seed % 4:
        assert all(int(summ[k][0]) > 0 for k in ("n_decode", "n_utf8", "n_close_len", "n_close_code", "n_bad_range"))
    if seed % 7 == 0:
        _check(wire, desc, mf - min(mf, 3), res, n, ver, en)


def test_no_connections_and_bad_arguments():
    wire, desc, mf, res, n, ver, en = F.synth_batch(F.every_reason())
    ref = _check(wire, desc, mf, res, 0, ver, en)
    assert int(ref[3]["first_failed"][0]) == F.NONE
    _check(wire[:0], desc, mf, res, n, None, en, flags=0)   # no wire at all: nothing is read from it
    L = U.lib()
    ro, vo = np.zeros_like(res), np.zeros_like(ver)
    fl, sm = np.zeros(n, F.FAIL_DT), np.zeros(1, F.SUMMARY_DT)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    odd = lambda a, k: C.c_void_p(a.ctypes.data + k)  # noqa: E731

    def call(wire=wire, wire_len=len(wire), desc=p(desc), mf=mf, res=p(res), n=n, ver=p(ver), en=p(en), flags=1,
             ro=p(ro), vo=p(vo), fl=p(fl), sm=p(sm)):
        return L.uvhttp_ws_fail_points(p(wire), wire_len, desc, mf, res, n, ver, en, flags, ro, vo, fl, sm)
    assert call() == 0 and call(en=None) == 0 and call(ver=None, vo=None) == 0 and call(wire=None, wire_len=0, flags=0) == 0
    for name in ("desc", "res", "ro", "fl", "sm"):
        assert call(**{name: None}) == -1, name
    assert call(wire=None) == -1                              # a length without bytes
    assert call(ver=None) == -1 and call(vo=None) == -1       # one verdict table without the other
    assert call(flags=2) == -1 and call(flags=0x80000001) == -1
    assert call(mf=(1 << 28) + 1) == -1 and call(n=(1 << 31) + 1) == -1
    for name, a in (("desc", desc), ("res", res), ("ro", ro), ("sm", sm)):
        assert call(**{name: odd(a, 4)}) == -1, name          # 8-byte tables at 4
    for name, a in (("ver", ver), ("vo", vo), ("fl", fl)):
        assert call(**{name: odd(a, 2)}) == -1, name
    with pytest.raises(ValueError):
        U.fail_points(wire, desc, mf, res, n, flags=4)


def test_twin_under_asan_ubsan():
    """tests/c/fail_check.c: the twin compiled with -fsanitize=address,undefined into a program of
    its own, the wire and every table in a heap block of exactly its size, seeded mixes of every
    input, out of place and in place"""
    import subprocess
    subprocess.run(["make", "-C", REPO, "tests/c/_build/fail_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(REPO, "tests", "c", "_build", "fail_check"), "400", "11"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert p.stdout.startswith("ok 400 ") and int(p.stdout.split()[2]) > 400


def test_struct_layouts():
    hdr = open(os.path.join(REPO, "include", "uvhttp_ws_amd.h")).read()
    for cls, dt, name in ((U.FailConn, F.FAIL_DT, "uvhttp_ws_fail_conn_t"),
                          (U.FailSummary, F.SUMMARY_DT, "uvhttp_ws_fail_summary_t")):
        assert C.sizeof(cls) == dt.itemsize
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == dt.fields[fname][1], (name, fname)
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == [f for f, _ in cls._fields_], name
    for text in ("#define UVHTTP_WS_FRAME_ERR_UTF8 (-12)", "#define UVHTTP_WS_FRAME_ERR_CLOSE (-13)",
                 "#define UVHTTP_WS_FAIL_CHECK_CLOSE 0x1u", "#define UVHTTP_WS_FAIL_BAD_RANGE 2",
                 "#define UVHTTP_WS_FAIL_DECODE 1", "#define UVHTTP_WS_FAIL_UTF8 2", "#define UVHTTP_WS_FAIL_CLOSE_LEN 3",
                 "#define UVHTTP_WS_FAIL_CLOSE_CODE 4"):
        assert text in hdr
    assert (U.FRAME_ERR_UTF8, U.FRAME_ERR_CLOSE, U.FAIL_CHECK_CLOSE, U.FAIL_BAD_RANGE) == (F.ERR_UTF8, F.ERR_CLOSE, 1, 2)
    assert (U.FAIL_NONE, U.FAIL_DECODE, U.FAIL_UTF8, U.FAIL_CLOSE_LEN, U.FAIL_CLOSE_CODE) == tuple(range(5))
