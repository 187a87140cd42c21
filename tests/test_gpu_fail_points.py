"""uvhttp_ws_gpu_fail_points_streams (include/uvhttp_ws_amd.h): every connection's fail point and
the rewritten result and verdict tables, against the Python restatement of the rule
(tests/_fail_ref.py) and against the host twin.  Every output lies in one guarded buffer: bytes
outside what the call may write keep their fill."""
import ctypes as C

import numpy as np
import pytest

import _fail_ref as F
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
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.zeros(16, np.uint8)])).to("cuda")  # (never empty)


class Out:
    """the call's four outputs as guarded slices of one filled buffer (8-byte aligned starts)"""

    def __init__(self, torch, n, with_ver=True):
        sizes = [64 * n, 16 * n if with_ver else 0, 16 * n, 32]
        at, self.spans = GUARD, []
        for sz in sizes:
            self.spans.append((at, sz))
            at += (sz + 7) // 8 * 8 + GUARD
        self.buf = torch.full((at,), FILL, dtype=torch.uint8, device="cuda")
        self.res, self.ver, self.fail, self.summ = [self.buf[a:a + max(sz, 8)] for a, sz in self.spans]
        if not with_ver:
            self.ver = None
        self.n = n

    def read(self):
        host = self.buf.cpu().numpy()
        inside = np.zeros(host.size, bool)
        for a, sz in self.spans:
            inside[a:a + sz] = True
        assert (host[~inside] == FILL).all(), "written outside the outputs"
        cut = [host[a:a + sz].tobytes() for a, sz in self.spans]
        return cut[0], cut[1] if self.ver is not None else None, cut[2], cut[3]


def _check(torch, eng, wire, desc, mf, res, n, ver=None, en=None, flags=F.CHECK_CLOSE, twin=True, in_place=True):
    """one device call against the reference (and the host twin), then in place -> the reference"""
    import uvhttp_amd as U
    ref = F.fail_points_ref(wire, desc, mf, res, n, ver, en, flags)
    want = F.ref_bytes(ref, n)
    o = Out(torch, n, ver is not None)
    d_wire, d_desc, d_res = _dev(torch, wire), _dev(torch, desc), _dev(torch, res)
    d_ver = None if ver is None else _dev(torch, ver)
    d_en = None if en is None else _dev(torch, en)
    eng.fail_points_streams(d_wire, d_desc, mf, d_res, n, d_ver, d_en, flags, o.res, o.ver, o.fail, o.summ,
                            wire_len=len(wire))
    torch.cuda.synchronize()
    assert o.read() == want
    assert d_res.cpu().numpy()[:64 * n].tobytes() == F.as_bytes(res[:n]), "d_results written"
    if twin:
        got = U.fail_points(wire, desc, mf, res, n, ver, en, flags)
        assert tuple(None if g is None else g.tobytes()[:len(w)] for g, w in zip(got, want)) == want
    if in_place:
        o2 = Out(torch, n, False)
        eng.fail_points_streams(d_wire, d_desc, mf, d_res, n, d_ver, d_en, flags, d_res, d_ver, o2.fail, o2.summ,
                                wire_len=len(wire))
        torch.cuda.synchronize()
        got = o2.read()
        assert (d_res.cpu().numpy()[:64 * n].tobytes(), None if ver is None else d_ver.cpu().numpy()[:16 * n].tobytes(),
                got[2], got[3]) == want
    return ref


def test_every_rule_as_one_batch(torch, eng):
    """the CPU cases (tests/test_fail_points_host.py) on the device: real frames through the
    oracle's decode and the reference verdicts; every reason, boundary code and CLOSE length"""
    b, names = F.rule_cases()
    _, _, fail, summ = _check(torch, eng, *b.tables(), b.ver, b.en)
    assert [int(r) for r in fail["reason"][:b.n]] == [w[0] for w in b.wants]
    assert [int(c) for c in fail["code"][:b.n]] == [w[2] for w in b.wants]
    assert int(summ["n_bad_range"][0]) == 2 and int(summ["n_decode"][0]) == 1
    _check(torch, eng, *b.tables(), None, b.en)
    _check(torch, eng, *b.tables(), b.ver, None)
    _check(torch, eng, *b.tables(), b.ver, b.en, flags=0)
    for mf in (0, 1, b.max_frames - 1):
        _check(torch, eng, b.wire, b.desc, mf, b.res, b.n, b.ver, b.en)
    c = F.clean_batch()
    res, ver, fail, _ = _check(torch, eng, *c.tables(), c.ver, c.en)
    assert F.as_bytes(res[:c.n]) == F.as_bytes(c.res[:c.n]) and F.as_bytes(ver[:c.n]) == F.as_bytes(c.ver[:c.n])
    assert (fail["reason"] == 0).all()


def _kinds(k, n):
    """the k-th failing connection of a shape test: a reason in turn, n = its frames"""
    m = max(0, n - 1)
    if n == 0:
        return F.spec(0, fs=-2)
    return [F.spec(n, utf8=m), F.spec(n, close=[(0, 1, 0)]), F.spec(n, close=[(m, 2, 1004)]), F.spec(n, fs=-1),
            F.spec(n, close=[(0, 2, 1000)], utf8=0)][k % 5]


@pytest.mark.parametrize("who", ["none", "one", "first", "last", "all"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_connections_across_scan_blocks(torch, eng, n, who):
    which = {"none": [], "one": [n // 2], "first": [0], "last": [n - 1], "all": list(range(n))}[who]
    frames = [(0, 1, 2, 3)[(s * 7 + s // 4) % 4] for s in range(n)]
    specs = [_kinds(which.index(s) if who != "all" else s, frames[s]) if s in set(which) else F.spec(frames[s])
             for s in range(n)]
    _, _, fail, summ = _check(torch, eng, *F.synth_batch(specs, gap=n % 2), twin=who != "all")
    assert [s for s in range(n) if fail[s]["reason"]] == which
    assert int(summ["first_failed"][0]) == (which[0] if which else F.NONE)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("edge", [255, 256, 257])
def test_frames_across_scan_blocks(torch, eng, edge, lead):
    """a cut, a first CLOSE and a range's end on descriptor `edge`, after a connection of `lead`
    frames; then connections of 255 / 256 / 257 frames in a row, each failing at its last frame"""
    k = edge - lead
    cut = [F.spec(lead), F.spec(k + 3, utf8=k), F.spec(2, close=[(0, 1, 0)])]
    close = [F.spec(lead), F.spec(k + 3, close=[(k, 2, 1005), (k + 1, 1, 0)], utf8=k + 2), F.spec(1, utf8=0)]
    fine = [F.spec(lead), F.spec(k + 3, close=[(k, 2, 1001), (k + 2, 1, 0)], utf8=k + 1), F.spec(1)]
    end = [F.spec(lead), F.spec(k + 1, close=[(k, 1, 0)]), F.spec(3, close=[(0, 2, 1000), (1, 1, 0)], utf8=2)]
    nobody = [F.spec(lead), F.spec(k), F.spec(2, enable=0, close=[(0, 1, 0)]), F.spec(2, fs=-10, close=[(0, 1, 0)]),
              F.spec(2, utf8=1)]
    for specs, want in ((cut, [0, 2, 3]), (close, [0, 4, 2]), (fine, [0, 0, 0]), (end, [0, 3, 0]), (nobody, [0, 0, 0, 0, 2])):
        _, _, fail, _ = _check(torch, eng, *F.synth_batch(specs), in_place=False)
        assert [int(r) for r in fail["reason"][:len(specs)]] == want
        assert fail[1]["reason"] < F.R_UTF8 or int(fail[1]["frame"]) == edge
    specs = [F.spec(n, close=[(n - 1, 2, 5000)]) for n in (255, 256, 257, 255, 257, 256)]
    _, _, fail, summ = _check(torch, eng, *F.synth_batch(specs, gap=lead % 2), in_place=False)
    assert (fail["reason"] == F.R_CLOSE_CODE).all() and int(summ["n_dropped"][0]) == 6


@pytest.mark.parametrize("piece", [1, 3])
def test_pieces_against_an_unsplit_engine(torch, monkeypatch, piece):
    """the five chunked passes in launches of 1 and 3 workgroups, through the test-hook build's
    piece knob: the same bytes as the unsplit engine, and the hook counts the pieces"""
    specs, rng = F.seeded_specs(77)
    specs += [F.spec(2, utf8=1), F.spec(300, close=[(299, 1, 0)])] * 140   # 5 workgroups of connections, 166 of frames
    tables = F.synth_batch(specs, rng)
    blocks, grid_s = -(-tables[2] // 256), -(-len(specs) // 256)
    assert grid_s >= 2 and blocks > 100
    split = _engine(monkeypatch, {KNOB: piece})
    whole = _engine(monkeypatch, {})
    try:
        assert split.grid_pieces() == (0, 0, 0)
        a = _check(torch, split, *tables, twin=False)
        b = _check(torch, whole, *tables, twin=False)
        assert F.ref_bytes(a, len(specs)) == F.ref_bytes(b, len(specs))
        passes, pieces, tiles = split.grid_pieces()   # (two calls: out of place and in place)
        assert (passes, tiles) == (10, 2 * (3 * blocks + 2 * grid_s))
        assert pieces == 2 * (3 * -(-blocks // piece) + 2 * -(-grid_s // piece))
    finally:
        whole.close()
        split.close()


def test_captured_graph(torch, eng):
    """one capture replayed over two sets of tables of the same shape: every input is read on the
    device, nothing from the capture's time is kept"""
    a = F.synth_batch([_kinds(s, 3) if s % 3 == 0 else F.spec(3) for s in range(300)])
    b = F.synth_batch([_kinds(s + 1, 3) if s % 7 else F.spec(3, close=[(1, 2, 999)]) for s in range(300)])
    assert len(a[0]) <= len(b[0]) and a[2] == b[2]
    n, mf = 300, a[2]
    wl = len(b[0])
    pad = lambda t: (np.concatenate([t[0], np.zeros(wl - len(t[0]), np.uint8)]),) + t[1:]  # noqa: E731
    a = pad(a)
    o = Out(torch, n)
    d = [_dev(torch, x) for x in (a[0], a[1], a[3], a[5], a[6])]
    cs = torch.cuda.Stream()

    def call():
        eng.fail_points_streams(d[0], d[1], mf, d[2], n, d[3], d[4], F.CHECK_CLOSE, o.res, o.ver, o.fail, o.summ,
                                wire_len=wl, stream=cs)
    with torch.cuda.stream(cs):
        call()   # (the scratch grows here, not in the capture)
    cs.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        call()
    for case in (a, b, a):
        for t, x in zip(d, (case[0], case[1], case[3], case[5], case[6])):
            t.copy_(_dev(torch, x))
        o.buf.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert o.read() == F.ref_bytes(F.fail_points_ref(case[0], case[1], mf, case[3], n, case[5], case[6], F.CHECK_CLOSE), n)


def test_no_connections_and_bad_arguments(torch, eng):
    import uvhttp_amd as U
    wire, desc, mf, res, n, ver, en = F.synth_batch(F.every_reason())
    ref = _check(torch, eng, wire, desc, mf, res, 0, ver, en, in_place=False)
    assert ref[3].tobytes() == np.array([(0, 0, 0, 0, 0, 0, F.NONE)], F.SUMMARY_DT).tobytes()
    _check(torch, eng, wire, desc, 0, res, n, ver, en)          # no descriptor: only decode failures are left
    o = Out(torch, n)
    d = dict(wire=_dev(torch, wire), desc=_dev(torch, desc), res=_dev(torch, res), ver=_dev(torch, ver), en=_dev(torch, en))
    L = U.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(wire=d["wire"], wire_len=len(wire), desc=d["desc"], mf=mf, res=d["res"], n=n, ver=d["ver"], en=d["en"],
             flags=1, ro=o.res, vo=o.ver, fl=o.fail, sm=o.summ):
        return L.uvhttp_ws_gpu_fail_points_streams(eng.h, p(wire), wire_len, p(desc), mf, p(res), n, p(ver), p(en), flags,
                                                   p(ro), p(vo), p(fl), p(sm), stream)
    assert call() == 0 and call(en=None) == 0 and call(ver=None, vo=None) == 0 and call(wire=None, wire_len=0, flags=0) == 0
    for name in ("desc", "res", "ro", "fl", "sm"):
        assert call(**{name: None}) == -1, name
    assert call(wire=None) == -1
    assert call(ver=None) == -1 and call(vo=None) == -1
    assert call(flags=2) == -1 and call(flags=0x80000001) == -1
    assert call(mf=(1 << 28) + 1) == -1 and call(n=(1 << 31) + 1) == -1
    for name, t in (("desc", d["desc"]), ("res", d["res"]), ("ro", o.res), ("sm", o.summ)):
        assert call(**{name: t[4:]}) == -1, name
    for name, t in (("ver", d["ver"]), ("vo", o.ver), ("fl", o.fail)):
        assert call(**{name: t[2:]}) == -1, name
    assert L.uvhttp_ws_gpu_fail_points_streams(None, p(d["wire"]), len(wire), p(d["desc"]), mf, p(d["res"]), n, None, None,
                                               0, p(o.res), None, p(o.fail), p(o.summ), stream) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed", range(40))
def test_seeded_batches(torch, eng, seed):
    """every reason at least once in each, and whatever else the seed brings"""
    specs, rng = F.seeded_specs(5000 + seed)
    wire, desc, mf, res, n, ver, en = F.synth_batch(specs, rng, gap=seed % 3)
    _, _, _, summ = _check(torch, eng, wire, desc, mf, res, n, ver if seed % 5 else None, en if seed % 3 else None,
                           F.CHECK_CLOSE if seed % 4 else 0, in_place=bool(seed & 1))
    if seed % 5 and seed % 3 and seed % 4:
        assert all(int(summ[k][0]) > 0 for k in ("n_decode", "n_utf8", "n_close_len", "n_close_code", "n_bad_range"))
