"""uvhttp_ws_gpu_close_frames_streams (include/uvhttp_ws_amd.h): the server's own 1002 / 1007
CLOSE frames for a decoded batch, against the Python restatement of the rule over the oracle's
build_frame (tests/_close_ref.py) and against the host twin.  Every output lies in one guarded
buffer: bytes outside what the call may write keep their fill."""
import ctypes as C

import numpy as np
import pytest

import _close_ref as CR
from test_gpu_epoch_wrap import _engine

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
KNOB = "UVHTTP_WS_GRID_PIECE"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def eng(torch):
    import uvhttp_amd as U
    e = U.GpuEngine(0)
    yield e
    e.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


class Out:
    """the call's outputs as guarded slices of one filled buffer (8-byte aligned starts)"""

    def __init__(self, torch, n, out_cap, stride=8, clear=()):
        sizes = [out_cap, 8 * (n + 1), 16 * max(1, n), 32, stride * max(1, n)] + [c.size * 4 for c in clear]
        at, self.spans = GUARD, []
        for sz in sizes:
            self.spans.append((at, sz))
            at += (sz + 7) // 8 * 8 + GUARD
        self.buf = torch.full((at,), FILL, dtype=torch.uint8, device="cuda")
        cut = [self.buf[a:a + sz] for a, sz in self.spans]
        self.out, self.off, self.conn, self.summ, self.runs = cut[:5]
        self.off = self.off.view(torch.int64)
        self.clear = cut[5:]
        for t, c in zip(self.clear, clear):
            t.copy_(_dev(torch, c))
        self.n, self.out_cap, self.stride = n, out_cap, stride
        self.clear_stride = [c.strides[0] for c in clear]

    def read(self, eng):
        host = self.buf.cpu().numpy()
        inside = np.zeros(host.size, bool)
        for a, sz in self.spans:
            inside[a:a + sz] = True
        assert (host[~inside] == FILL).all(), "written outside the outputs"
        n = self.n
        off = self.off.cpu().numpy().astype(np.uint64)
        total = int(off[n])
        out = self.out.cpu().numpy()
        assert (out[total:] == FILL).all(), "d_out written past the frames"
        runs = self.runs.cpu().numpy().view(np.uint32).reshape(max(1, n), self.stride // 4)
        assert (runs[:, 2:] == 0xA5A5A5A5).all(), "bytes between the runs written"
        return {"out": out[:total].tobytes(), "out_off": [int(x) for x in off],
                "runs": [(int(r[0]), int(r[1])) for r in runs[:n]], "conn": eng.read_close_conns(self.conn, n),
                "summary": eng.read_close_summary(self.summ),
                "clear": [t.cpu().numpy().view(np.uint32) for t in self.clear]}


def _call(torch, eng, o, d, n, use, stream=None):
    """use = which optional inputs are passed: a set of "ver", "rep", "en", "keys" """
    eng.close_frames_streams(d["st"], d["res"], n, o.out_cap, verdict=d["ver"] if "ver" in use else None,
                             reply_conn=d["rep"] if "rep" in use else None, enable=d["en"] if "en" in use else None,
                             mask_keys=d["keys"] if "keys" in use else None, out=o.out, out_off=o.off, runs=o.runs,
                             run_stride=o.stride, clear_runs=o.clear, clear_stride=o.clear_stride, conn=o.conn,
                             summary=o.summ, stream=stream)


ALL = frozenset(("ver", "rep", "en", "keys"))


def _check(torch, eng, case, n, use=ALL, out_cap=None, stride=8, clear=(), twin=True):
    """one device call against the reference (and the host twin) -> the reference"""
    import uvhttp_amd as U
    st, res, ver, rep, en, keys = case
    args = (ver if "ver" in use else None, rep if "rep" in use else None, en if "en" in use else None,
            keys if "keys" in use else None)
    want_clear = [c.copy() for c in clear]
    ref = CR.close_frames_ref(st, res, n, *args, out_cap, want_clear)
    cap = out_cap if out_cap is not None else len(ref["out"])
    o = Out(torch, n, cap, stride, clear)
    d = dict(st=_dev(torch, st), res=_dev(torch, res), ver=_dev(torch, ver), rep=_dev(torch, rep),
             en=_dev(torch, en), keys=_dev(torch, keys))
    _call(torch, eng, o, d, n, use)
    torch.cuda.synchronize()
    got = o.read(eng)
    got_clear = got.pop("clear")
    assert got == ref
    for g, w in zip(got_clear, want_clear):
        assert np.array_equal(g.reshape(w.shape), w)
    if twin:
        tc = [c.copy() for c in clear]
        out, off, runs, conn, summ = U.close_frames(st, res, n, *args, out_cap=cap, run_stride=stride, clear_runs=tc,
                                                    clear_stride=[c.strides[0] for c in tc])
        assert (out, [int(x) for x in off], conn, summ) == (got["out"], got["out_off"], got["conn"], got["summary"])
        for g, w in zip(got_clear, tc):
            assert np.array_equal(g.reshape(w.shape), w)
    return ref


def test_every_rule_as_one_batch(torch, eng):
    """the CPU cases (tests/test_close_frames_host.py) on the device: every frame status, every
    verdict, closed, not enabled, client and server streams, 1007 over 1002"""
    *case, want = CR.rule_cases()
    n = len(want)
    ref = _check(torch, eng, case, n)
    assert [c["code"] for c in ref["conn"]] == want
    for use in (ALL - {"ver"}, ALL - {"rep"}, ALL - {"en"}, ALL - {"keys"}, frozenset()):
        _check(torch, eng, case, n, use)
    no_keys = _check(torch, eng, case, n, ALL - {"keys"})
    assert CR.NO_KEYS in [c["status"] for c in no_keys["conn"]]
    assert no_keys["summary"]["n_closes"] < ref["summary"]["n_closes"]


def test_capacity_and_clear_runs(torch, eng):
    *case, want = CR.rule_cases()
    n = len(want)
    full = CR.close_frames_ref(*case[:2], n, *case[2:])
    clear = [np.arange(2 * n, dtype=np.uint32).reshape(n, 2) + 1, np.arange(8 * n, dtype=np.uint32).reshape(n, 8) + 100]
    short = _check(torch, eng, case, n, out_cap=len(full["out"]) - 1, clear=clear, stride=32)
    assert short["summary"]["status"] == CR.ERR_CAPACITY and short["out"] == b""
    assert short["summary"]["out_bytes"] == len(full["out"]) and short["summary"]["n_closes"] == full["summary"]["n_closes"]
    again = _check(torch, eng, case, n, out_cap=short["summary"]["out_bytes"], clear=clear, stride=32)
    assert again["out"] == full["out"] and again["summary"]["n_1007"] == want.count(1007) > 0


def _failing(n, which):
    st, res, ver, rep, en, keys = CR.tables(n)
    keys[:] = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    st["is_server"] = np.arange(n) % 3 != 0
    for k, s in enumerate(which):
        if k & 1:
            ver[s]["status"] = CR.UTF8_INVALID
        else:
            res[s]["first_status"] = -1 - (k % 8)
    return st, res, ver, rep, en, keys


@pytest.mark.parametrize("who", ["none", "one", "first", "last", "all"])
# (the last two: more than 64 and more than 256 block aggregates, so the top scan carries across a
# wave boundary, and every lane of it folds a run of more than one aggregate)
@pytest.mark.parametrize("n", [255, 256, 257, 513, 64 * 256 + 1, 256 * 256 + 1])
def test_connections_across_scan_blocks(torch, eng, n, who):
    which = {"none": [], "one": [n // 2], "first": [0], "last": [n - 1], "all": list(range(n))}[who]
    ref = _check(torch, eng, _failing(n, which), n, twin=who != "all")
    assert ref["summary"]["n_closes"] == len(which)
    assert [s for s in range(n) if ref["conn"][s]["code"]] == which


def test_no_connections_and_bad_arguments(torch, eng):
    import uvhttp_amd as U
    case = CR.tables(1)
    ref = _check(torch, eng, case, 0, twin=False)
    assert ref["out_off"] == [0] and ref["summary"] == {"out_bytes": 0, "n_closes": 0, "n_1002": 0, "n_1007": 0, "status": 0}
    o = Out(torch, 1, 64)
    d = dict(st=_dev(torch, case[0]), res=_dev(torch, case[1]))
    run = torch.zeros(16, dtype=torch.uint8, device="cuda")
    L = U.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(st=d["st"], res=d["res"], out=o.out, off=o.off, conn=o.conn, summ=o.summ, flags=0, runs=None, stride=8,
             clear=(), cstride=(), n_clear=None, n=1):
        cp = (C.c_void_p * 5)(*[t.data_ptr() if t is not None else None for t in clear])
        cs = (C.c_uint32 * 5)(*cstride)
        return L.uvhttp_ws_gpu_close_frames_streams(eng.h, p(st), p(res), n, None, None, None, None, flags, p(out), 64,
                                                    p(off), p(runs), stride, cp, cs, len(clear) if n_clear is None else n_clear,
                                                    p(conn), p(summ), stream)
    assert call() == 0
    for name in ("st", "res", "out", "off", "conn", "summ"):
        assert call(**{name: None}) == -1, name
    assert call(flags=1) == -1
    assert call(runs=run, stride=4) == -1 and call(runs=run, stride=10) == -1 and call(runs=run, stride=12) == 0
    assert call(clear=(run,) * 5, cstride=(8,) * 5) == -1
    assert call(clear=(run,), cstride=(6,)) == -1 and call(clear=(None,), cstride=(8,)) == -1
    assert call(clear=(run,) * 4, cstride=(8, 12, 16, 8)) == 0
    assert call(st=d["st"][4:]) == -1 and call(off=o.off.view(torch.uint8)[4:]) == -1   # misaligned
    assert call(n=(1 << 31) + 1) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("piece", [1, 3])
def test_pieces_against_an_unsplit_engine(torch, monkeypatch, piece):
    """both chunked passes (size, emit) in launches of 1 and 3 workgroups, through the test-hook
    build's piece knob: the same bytes as the unsplit engine, and the hook counts the pieces"""
    n = 5 * 256 + 7   # six workgroups
    case = _failing(n, [0, 1, 255, 256, 257, 511, 512, 700, 1023, 1024, 1279, 1280, n - 1])
    split = _engine(monkeypatch, {KNOB: piece})
    whole = _engine(monkeypatch, {})
    try:
        assert split.grid_pieces() == (0, 0, 0)
        a = _check(torch, split, case, n, twin=False)
        b = _check(torch, whole, case, n, twin=False)
        assert a == b and a["summary"]["n_closes"] == 13
        passes, pieces, tiles = split.grid_pieces()
        assert (passes, tiles) == (2, 12) and pieces == 2 * -(-6 // piece)
    finally:
        whole.close()
        split.close()


def test_captured_graph(torch, eng):
    """one capture replayed over two batches of the same shape: every input is read on the device"""
    n = 300
    a = _failing(n, [0, 5, 255, 256, 299])
    b = _failing(n, list(range(0, n, 7)))
    o = Out(torch, n, 22 * n, clear=[np.zeros((n, 2), np.uint32)])
    d = {k: _dev(torch, v) for k, v in zip(("st", "res", "ver", "rep", "en", "keys"), a)}
    cs = torch.cuda.Stream()
    with torch.cuda.stream(cs):
        _call(torch, eng, o, d, n, ALL, cs)   # (the scratch grows here, not in the capture)
    cs.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        _call(torch, eng, o, d, n, ALL, cs)
    for case in (a, b, a):
        for k, v in zip(("st", "res", "ver", "rep", "en", "keys"), case):
            d[k].copy_(_dev(torch, v))
        o.buf.fill_(FILL)
        o.clear[0].copy_(_dev(torch, np.full((n, 2), 9, np.uint32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_clear = [np.full((n, 2), 9, np.uint32)]
        ref = CR.close_frames_ref(case[0], case[1], n, *case[2:], 22 * n, want_clear)
        got = o.read(eng)
        clear = got.pop("clear")
        assert got == ref and np.array_equal(clear[0].reshape(n, 2), want_clear[0])
