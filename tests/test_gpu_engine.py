"""Engine-level guarantees of the device surface (include/uvhttp_ws_amd.h, "Streams and graphs"
and UVHTTP_WS_FRAME_ERR_DEVICE):

* a look-back wait that gives up is reported, never turned into wrong descriptors: the call
  delivers nothing, its summary / results say ERR_DEVICE and engine_sync raises;
* a decode captured into a hipGraph and replayed over CHANGING frame bytes stays bit-exact
  (each replay draws a fresh device-side epoch, so tags left by the previous replay — first
  failure, tile maps, look-back records — never match);
* calls on different streams serialise on the engine's one workspace;
* a captured call that would have to grow an engine-owned scratch block is refused with its
  error, queues nothing, and the same call uncaptured then works; a block grows, is reused and
  grows again under one engine.
Every check compares with the oracle (oracle/ws_oracle.c) or the host twins."""
import ctypes
import gc
import os
import random

import numpy as np
import pytest

import _oracle
import _replies_ref as RR
import _utf8_frames_ref as FR
from test_gpu_build import _rand_frames
from test_gpu_control_replies import Out as ReplyOut, _dev
from test_gpu_parity import _frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _engine(env=None):
    import uvhttp_amd as U
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return U.GpuEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _batch(rng, n, fail_at=None, sizes=(0, 1, 125, 126, 300, 4000, 70000)):
    frames, offs, pos = [], [], 0
    for i in range(n):
        payload = rng.randbytes(rng.choice(sizes))
        f = _frame(2, 1, payload, rng.randbytes(4), True, 4 if i == fail_at else 0)
        frames.append(f)
        offs.append(pos)
        pos += len(f)
    return b"".join(frames), np.array(offs, np.uint64)


def test_lookback_give_up_is_reported(torch):
    """UVHTTP_WS_MAX_POLLS=0 makes every block with a predecessor give up at once: the call
    must report ERR_DEVICE, unmask nothing and make engine_sync fail — then a normal engine
    decodes the same bytes correctly."""
    import uvhttp_amd as U
    rng = random.Random(11)
    wire, offs = _batch(rng, 4096, sizes=(0, 1, 20, 125, 200))
    w = np.frombuffer(wire, np.uint8)
    eng = _engine({"UVHTTP_WS_MAX_POLLS": "0"})
    d = torch.from_numpy(np.concatenate([w, np.zeros(64, np.uint8)])).to("cuda")
    before = d.clone()
    o = torch.from_numpy(offs.view(np.int64)).to("cuda")
    desc, summ = eng.decode_inplace(d, len(offs), offsets=o, wire_len=w.size)
    torch.cuda.synchronize()
    s = eng.read_summary(summ)
    assert s["status"] == -1 and s["first_status"] == -11 and s["n_delivered"] == 0, s
    assert (eng.read_desc(desc, len(offs))["status"] == 2).all()
    assert torch.equal(d, before)
    with pytest.raises(U.GpuError):
        eng.sync()
    eng.sync()  # reported once
    # a stride batch of small frames: nothing unmasked either
    sw = b"".join(_frame(2, 1, rng.randbytes(40), rng.randbytes(4), True, 0) for _ in range(30000))
    sd = torch.from_numpy(np.frombuffer(sw + bytes(64), np.uint8).copy()).to("cuda")
    sbefore = sd.clone()
    desc, summ = eng.decode_inplace(sd, 30000, stride=len(sw) // 30000, wire_len=len(sw))
    torch.cuda.synchronize()
    s = eng.read_summary(summ)
    assert s["status"] == -1 and s["first_status"] == -11 and s["n_delivered"] == 0, s
    assert torch.equal(sd, sbefore)
    with pytest.raises(U.GpuError):
        eng.sync()
    # the stream decode has no look-back (per-connection walk + one-block scan) unless the wave
    # walk runs fused (UVHTTP_WS_WALK_FUSE=1: k_swalk_fused finds first frames by a look-back
    # over blocks of connections; the speculative decode, which has none and would take these
    # connections first, is off).  Fused, every block after the first gives up, so every
    # stream reports ERR_DEVICE and nothing is unmasked ...
    st = np.zeros(64, U.STREAM_DT)
    per = w.size // 64
    idx = np.minimum(np.searchsorted(offs, np.arange(64) * per), len(offs) - 1)
    cut = [int(offs[i]) for i in idx] + [w.size]
    for k in range(64):
        st[k] = (cut[k], cut[k + 1] - cut[k], 1 << 30, 0, 0, 1 << 24, 1 << 26, 1, 0, 0, 0)
    sdev = torch.from_numpy(st.view(np.uint8).copy()).to("cuda")
    eng.close()
    eng = _engine({"UVHTTP_WS_MAX_POLLS": "0", "UVHTTP_WS_WALK_FUSE": "1", "UVHTTP_WS_STREAM_SPEC": "0"})
    d2 = before.clone()
    _, res = eng.decode_streams(d2, sdev, 64, 8192, wire_len=w.size)
    torch.cuda.synchronize()
    rs = eng.read_stream_results(res, 64)
    assert all(r.status == -1 and r.first_status == -11 and r.n_delivered == 0 for r in rs)
    assert torch.equal(d2, before)
    with pytest.raises(U.GpuError):
        eng.sync()
    eng.close()
    # ... while the walk, its one-block scan and k_stream_desc apart (the default) have no
    # look-back: an engine with the same poll bound decodes the streams normally
    eng = _engine({"UVHTTP_WS_MAX_POLLS": "0"})
    d2 = before.clone()
    _, res = eng.decode_streams(d2, sdev, 64, 8192, wire_len=w.size)
    torch.cuda.synchronize()
    rs = eng.read_stream_results(res, 64)
    assert all(r.status == 0 for r in rs)
    assert sum(r.n_delivered for r in rs) == len(offs)
    eng.sync()
    eng.close()
    good = _engine()
    desc, summ = good.decode_inplace(d, len(offs), offsets=o, wire_len=w.size)
    torch.cuda.synchronize()
    good.sync()
    ref = _oracle.decode_batch(w, len(offs), offsets=offs)
    assert good.read_summary(summ) == ref["summary"]
    assert np.array_equal(d[:w.size].cpu().numpy(), ref["wire"])
    good.close()


def test_graph_capture_replay_changing_batches(torch):
    """Capture one decode_inplace (offset-table layout) and replay it over four different
    batches of the same frame count and wire length: a failing frame early, none, a failure
    late, then different frame sizes.  Each replay must equal the oracle; a stale first-
    failure tag or tile map from the previous replay would break the second and fourth."""
    t = torch
    rng = random.Random(12)
    n = 3000
    batches = [_batch(rng, n, fail_at=40), _batch(rng, n), _batch(rng, n, fail_at=2500),
               _batch(rng, n, sizes=(2, 60, 9000))]
    wl = max(len(b[0]) for b in batches)
    eng = _engine()
    wire = t.zeros(wl + 64, dtype=t.uint8, device="cuda")
    offs = t.zeros(n, dtype=t.int64, device="cuda")
    desc, summ = eng.alloc_outputs(n)
    eng.reserve(n, wl, 0)

    def load(k):
        b, o = batches[k]
        host = np.zeros(wl, np.uint8)
        host[:len(b)] = np.frombuffer(b, np.uint8)
        wire[:wl].copy_(t.from_numpy(host))
        offs.copy_(t.from_numpy(o.view(np.int64)))
        return host

    # warm (uncaptured) call on the capture stream's shapes, then capture
    load(0)
    s = t.cuda.Stream()
    with t.cuda.stream(s):
        eng.decode_inplace(wire, n, offsets=offs, wire_len=wl, desc=desc, summary=summ, stream=s)
    s.synchronize()
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g, stream=s):
        eng.decode_inplace(wire, n, offsets=offs, wire_len=wl, desc=desc, summary=summ, stream=s)
    for k in [0, 1, 2, 3, 1]:
        host = load(k)
        t.cuda.synchronize()
        g.replay()
        t.cuda.synchronize()
        ref = _oracle.decode_batch(host, n, offsets=batches[k][1], wire_len=wl)
        got = eng.read_summary(summ)
        assert got == ref["summary"], (k, got, ref["summary"])
        assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), k
        assert np.array_equal(eng.read_desc(desc, n)["status"], ref["status"]), k
    # host calls after the replays, then replays again: the workspace holds the replays' tags,
    # whose device epochs are larger than any host call's — the host call's claims (first
    # failure, tile maps) must still win over them (round 5: they did not, and a host call after
    # a replay delivered frames after a failure)
    for k in [2, 0, 3]:
        host = load(k)
        eng.decode_inplace(wire, n, offsets=offs, wire_len=wl, desc=desc, summary=summ, stream=s)
        s.synchronize()
        ref = _oracle.decode_batch(host, n, offsets=batches[k][1], wire_len=wl)
        assert eng.read_summary(summ) == ref["summary"], ("host after replay", k)
        assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), ("host after replay", k)
        assert np.array_equal(eng.read_desc(desc, n)["status"], ref["status"]), ("host after replay", k)
        host = load((k + 1) % 4)
        t.cuda.synchronize()
        g.replay()
        t.cuda.synchronize()
        ref = _oracle.decode_batch(host, n, offsets=batches[(k + 1) % 4][1], wire_len=wl)
        assert eng.read_summary(summ) == ref["summary"], ("replay after host", k)
        assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), ("replay after host", k)
    eng.sync()
    eng.close()


def test_calls_on_two_streams_serialise(torch):
    """Back-to-back calls on two streams with no host sync between them share one workspace;
    the engine orders the second after the first.  Both must equal the oracle."""
    t = torch
    rng = random.Random(13)
    eng = _engine()
    runs = []
    s1, s2 = t.cuda.Stream(), t.cuda.Stream()
    for k in range(4):
        b, o = _batch(rng, 5000, fail_at=[None, 1000, 4000, None][k], sizes=(0, 1, 126, 600))
        w = np.frombuffer(b, np.uint8)
        d = t.from_numpy(np.concatenate([w, np.zeros(64, np.uint8)])).to("cuda")
        od = t.from_numpy(o.view(np.int64)).to("cuda")
        desc, summ = eng.alloc_outputs(len(o))
        runs.append((w, o, d, od, desc, summ))
    t.cuda.synchronize()
    for (w, o, d, od, desc, summ), s in zip(runs, [s1, s2, s1, s2]):
        eng.decode_inplace(d, len(o), offsets=od, wire_len=w.size, desc=desc, summary=summ,
                           stream=s)
    t.cuda.synchronize()
    for w, o, d, od, desc, summ in runs:
        ref = _oracle.decode_batch(w, len(o), offsets=o)
        assert eng.read_summary(summ) == ref["summary"]
        assert np.array_equal(d[:w.size].cpu().numpy(), ref["wire"])
    eng.close()


def test_graph_capture_replay_stride_batches(torch):
    """A stride-layout decode captured and replayed over changing frame bytes of one stride: no
    failure, a state-machine failure early, none again, a failure late."""
    t = torch
    rng = random.Random(14)
    n, plen = 20000, 200

    def batch(fail_at):
        frames = []
        for i in range(n):
            op = 0 if i == fail_at else 2  # CONTINUATION with nothing open
            frames.append(_frame(op, 1, rng.randbytes(plen), rng.randbytes(4), True, 0))
        return b"".join(frames)
    batches = [batch(None), batch(37), batch(None), batch(19000)]
    stride = len(batches[0]) // n
    wl = len(batches[0])
    eng = _engine()
    wire = t.zeros(wl + 64, dtype=t.uint8, device="cuda")
    desc, summ = eng.alloc_outputs(n)
    eng.reserve(n, wl, 0)
    s = t.cuda.Stream()
    wire[:wl].copy_(t.from_numpy(np.frombuffer(batches[0], np.uint8).copy()))
    with t.cuda.stream(s):
        eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s)
    s.synchronize()
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g, stream=s):
        eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s)
    for k in [0, 1, 2, 3, 1]:
        host = np.frombuffer(batches[k], np.uint8).copy()
        wire[:wl].copy_(t.from_numpy(host))
        t.cuda.synchronize()
        g.replay()
        t.cuda.synchronize()
        ref = _oracle.decode_batch(host, n, stride=stride, wire_len=wl)
        assert eng.read_summary(summ) == ref["summary"], k
        assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), k
        assert np.array_equal(eng.read_desc(desc, n)["status"], ref["status"]), k
    # host calls (fused path, summary-only, compact) after the replays: their failure claims must
    # displace the replays' larger-epoch tags
    for k, mode in ((1, "desc"), (3, "no_desc"), (1, "compact")):
        host = np.frombuffer(batches[k], np.uint8).copy()
        wire[:wl].copy_(t.from_numpy(host))
        ref = _oracle.decode_batch(host, n, stride=stride, wire_len=wl, compact=mode == "compact",
                                   arena_cap=wl + 64)
        if mode == "compact":
            arena = t.zeros(wl + 64, dtype=t.uint8, device="cuda")
            eng.decode_compact(wire, n, arena, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s)
        else:
            eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s,
                               no_desc=mode == "no_desc")
        s.synchronize()
        assert eng.read_summary(summ) == ref["summary"], ("host after replay", k, mode)
        assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), ("host after replay", k, mode)
        g.replay()
        t.cuda.synchronize()
    eng.sync()
    eng.close()


# ---- engine-owned scratch: refused growth in a captured call; grow, reuse, grow again -----------

def _hooks_engine():
    import uvhttp_amd as U
    return U.GpuEngine(0, library=U.test_hooks_library())


def _small_frames(rng, n):
    """n masked frames of at most 126 payload bytes: TEXT (valid UTF-8), every fifth a PING"""
    return [RR.ping(rng.randbytes(rng.choice((0, 9, 125)))) if i % 5 == 3 else
            FR.Fr(1, 1, "".join(rng.choice("aé€ ") for _ in range(rng.choice((0, 1, 20, 42)))).encode())
            for i in range(n)]


class _Decoded:
    """`frames` as an offset-table batch on the device, its outputs, and the oracle's decode"""

    def __init__(self, t, eng, frames):
        self.t, self.eng, self.frames, self.n = t, eng, frames, len(frames)
        self.wire = np.frombuffer(b"".join(f.bytes for f in frames), np.uint8).copy()
        self.offs = np.cumsum([0] + [len(f.bytes) for f in frames[:-1]]).astype(np.uint64)
        self.dw, self.do = _dev(t, self.wire), t.from_numpy(self.offs.view(np.int64)).to("cuda")
        self.desc, self.summ = eng.alloc_outputs(self.n)
        self.ref = _oracle.decode_batch(self.wire, self.n, offsets=self.offs, max_frame_size=FR.MF,
                                        max_message_size=FR.MM)

    def decode(self, stream=None, no_desc=False):
        self.eng.decode_inplace(self.dw, self.n, offsets=self.do, wire_len=self.wire.size, max_frame_size=FR.MF,
                                max_message_size=FR.MM, desc=self.desc, summary=self.summ, stream=stream,
                                no_desc=no_desc)

    def check(self, no_desc=False):
        self.t.cuda.synchronize()
        assert self.eng.read_summary(self.summ) == self.ref["summary"]
        assert np.array_equal(self.dw[:self.wire.size].cpu().numpy(), self.ref["wire"])
        if not no_desc:
            assert np.array_equal(self.eng.read_desc(self.desc, self.n)["status"], self.ref["status"])
        self.nd = self.ref["summary"]["n_delivered"]
        self.hw, self.hd = self.dw[:self.wire.size].cpu().numpy(), self.eng.read_desc(self.desc, self.n)


class _Utf8:
    """validate_utf8_inplace over a decoded batch, against the reference walk and the host twin"""

    def __init__(self, d):
        self.d = d
        self.v, self.sm = d.eng._utf8_frames_out(1, None, None)

    def call(self, stream=None):
        d = self.d
        d.eng.validate_utf8_inplace(d.dw, d.desc, d.n, d.summ, verdict=self.v, summary=self.sm,
                                    wire_len=d.wire.size, stream=stream)

    def check(self):
        import uvhttp_amd as U
        d = self.d
        d.t.cuda.synchronize()
        got = d.eng.read_utf8_conn_verdicts(self.v, 1)[0]
        want = FR.judge(d.frames[:d.nd])
        assert got == want == U.utf8_judge_frames(d.hw, d.hd, 0, d.nd, 0, None, 0), (got, want)
        assert d.eng.read_utf8_frames_summary(self.sm) == FR.summary([want])


class _Replies:
    """control_replies_inplace over a decoded batch, against the host twin and the sink's frames"""

    def __init__(self, d, rng):
        self.d = d
        self.keys = RR.keys_for(rng, d.n)
        self.dkeys = _dev(d.t, self.keys, 0)
        self.o = ReplyOut(d.t, 1, d.n, 131 * d.n)

    def call(self, stream=None):
        d, o = self.d, self.o
        d.eng.control_replies_inplace(d.dw, d.desc, d.n, d.summ, d.n, 131 * d.n, is_server=1, mask_keys=self.dkeys,
                                      out=o.out, out_off=o.off, runs=o.runs, conn=o.conn, summary=o.summ,
                                      wire_len=d.wire.size, stream=stream)

    def check(self):
        import uvhttp_amd as U
        d = self.d
        d.t.cuda.synchronize()
        got = self.o.read(d.eng)
        assert got == RR.host_batch(U, d.hw, d.hd, [0], [d.nd], [1], None, self.keys, 0, d.n)
        assert got == RR.expected_batch([b"".join(f.bytes for f in d.frames[:d.nd])], [1], None, self.keys, 0,
                                        None, {}, d.n)
        assert got["summary"]["n_replies"] == sum(f.op == 9 for f in d.frames[:d.nd])


def _refused_in_capture(t, call, text):
    """`call(stream)` inside a stream capture must raise GpuError(text); the graph (one trivial
    op, so it is not empty) is never replayed.  No finalizer of a device object may run inside a
    capture (a graph, tensor or engine freed there makes calls the capture forbids, and the process
    aborts): dead cycles are collected before it, the collector rests during it, and the error is
    kept as text only, since a kept exception's traceback holds this frame, and with it the graph,
    in a cycle that the collector would free at some later moment, such as the next capture."""
    import uvhttp_amd as U
    s = t.cuda.Stream()
    tick = t.zeros(16, device="cuda")
    t.cuda.synchronize()
    g = t.cuda.CUDAGraph()
    got = None
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        with t.cuda.graph(g, stream=s):
            tick.add_(1)
            try:
                call(s)
            except U.GpuError as e:
                got = str(e)
    finally:
        if was_on:
            gc.enable()
    t.cuda.synchronize()
    assert got == text


# what each call answers when a capture would make it allocate (uvhttp_amd/csrc: reserve_ws,
# build_frames, fu_run, rp_run), as GpuEngine._check formats it: "<call> rc=<code>: <last_error>"
_REFUSALS = {
    "decode_inplace": "decode_inplace rc=-1: workspace too small for a captured call: reserve first: ",
    "decode_streams": "decode_streams rc=-1: workspace too small for a captured call: reserve first: ",
    "build_frames": "build_frames rc=-1: build map too small for a captured call: ",
    "validate_utf8_inplace": "validate_utf8_inplace rc=-3: validate_utf8 frame scratch (a captured call must "
                             "not grow it): ",
    "control_replies_inplace": "control_replies_inplace rc=-3: control_replies scratch (a captured call must "
                               "not grow it): ",
}


@pytest.mark.parametrize("what", list(_REFUSALS))
def test_captured_call_that_would_allocate_is_refused(torch, what):
    """A captured call must not allocate: with its scratch block missing or too small it returns
    its error and queues nothing.  The same call, uncaptured, on the same engine then equals the
    oracle / the host twin: the engine left capture mode, and the refused growth left no
    capacity behind that the block does not have."""
    import uvhttp_amd as U
    t = torch
    rng = random.Random(21)
    eng = _hooks_engine()
    frames = _small_frames(rng, 64)
    if what == "decode_inplace":  # an engine that was never reserved
        d = _Decoded(t, eng, frames)
        call, check = d.decode, d.check
    elif what == "decode_streams":  # reserved for too few frames
        conns = [frames[k:k + 16] for k in range(0, 64, 16)]
        wire, st = FR.streams_of(conns)
        dw, dst = _dev(t, wire), _dev(t, st, 0)
        desc = t.zeros(64 * eng.DESC_BYTES, dtype=t.uint8, device="cuda")
        res = t.zeros(4 * ctypes.sizeof(U.StreamResult), dtype=t.uint8, device="cuda")
        eng.reserve(8, wire.size, 0)

        def call(stream=None):
            eng.decode_streams(dw, dst, 4, 64, desc=desc, results=res, wire_len=wire.size, stream=stream)

        def check():
            t.cuda.synchronize()
            ref_wire, _, first, nd, _ = FR.oracle_decode(wire, st)
            rs = eng.read_stream_results(res, 4)
            assert [(r.status, r.first_frame, r.n_delivered) for r in rs] == [(0, f, n) for f, n in zip(first, nd)]
            assert nd == [16] * 4 and np.array_equal(dw[:wire.size].cpu().numpy(), ref_wire)
    elif what == "build_frames":  # the workspace reserved, no output map yet
        src = np.frombuffer(rng.randbytes(1000), np.uint8).copy()
        fr = _rand_frames(rng, src.size, 8, [0, 5, 126])
        exp = b"".join(_oracle.build_frame(src[f["payload_off"]:f["payload_off"] + f["payload_len"]].tobytes(),
                                           int(f["opcode"]), int(f["mask"]), int(f["fin"]),
                                           int(f["key"]).to_bytes(4, "little"))[1] for f in fr)
        dsrc, dfr = _dev(t, src, 0), _dev(t, fr, 0)
        out = t.zeros(8 * 4096, dtype=t.uint8, device="cuda")  # 4 KiB per frame: the map path
        off = t.zeros(9, dtype=t.int64, device="cuda")
        eng.reserve(8, 0, 0)

        def call(stream=None):
            eng.build_frames(dsrc, dfr, 8, out, out_off=off, stream=stream)

        def check():
            t.cuda.synchronize()
            assert int(off[8]) == len(exp) and out[:len(exp)].cpu().numpy().tobytes() == exp
            assert not out[len(exp):].any()
    else:  # after an uncaptured decode with descriptors: the call's own scratch does not exist yet
        d = _Decoded(t, eng, frames)
        d.decode()
        d.check()
        c = _Utf8(d) if what == "validate_utf8_inplace" else _Replies(d, rng)
        call, check = c.call, c.check
    _refused_in_capture(t, call, _REFUSALS[what])
    call()
    check()
    eng.sync()
    eng.close()


@pytest.mark.parametrize("route", ["descriptor_scratch", "validate_utf8_inplace", "control_replies_inplace"])
def test_scratch_grows_is_reused_and_grows_again(torch, route):
    """32 frames, then 5 000, then 32 again on one engine: the block is allocated, replaced by a
    larger one, and the larger one reused.  descriptor_scratch: decode_inplace of an offset-table
    batch without descriptors, which takes the engine's."""
    t = torch
    rng = random.Random(22)
    eng = _hooks_engine()
    for n in (32, 5000, 32):
        d = _Decoded(t, eng, _small_frames(rng, n))
        d.decode(no_desc=route == "descriptor_scratch")
        d.check(no_desc=route == "descriptor_scratch")
        if route != "descriptor_scratch":
            c = _Utf8(d) if route == "validate_utf8_inplace" else _Replies(d, rng)
            c.call()
            c.check()
    eng.sync()
    eng.close()
