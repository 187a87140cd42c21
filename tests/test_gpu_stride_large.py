"""In-place stride batches of large frames (ws_gpu.hip: k_unmask_inplace<64, 1, true> ->
k_large_fix): the payload pass decodes from the headers its tiles find by arithmetic, unmasks
every simple frame (a complete, valid, unfragmented data frame), and the one launch behind it
writes the summary or, after a frame that is not simple, runs the state machine and repairs the
wire.  Every case is decoded with the path on (the product library, and the experiment build
with UVHTTP_WS_LARGE_SPEC=1) and off (UVHTTP_WS_LARGE_SPEC=0: k_plan first) and compared with
the CPU oracle: wire bytes, statuses, summary; every other descriptor field against the frames
the test built (delivered frames) and between the two paths (all frames).
"""
import os
import random

import numpy as np
import pytest

import _oracle
from test_gpu_parity import _frame

pytestmark = pytest.mark.gpu
MF, MM = 16 * 1024 * 1024, 64 * 1024 * 1024
FIN, MASK, MSG_END = 1, 2, 0x20


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


@pytest.fixture(scope="module")
def engines(torch):
    """(name, engine): the product library, the experiment build with the path on, and off"""
    engs = [("product", _engine()), ("on", _engine({"UVHTTP_WS_LARGE_SPEC": "1"})),
            ("off", _engine({"UVHTTP_WS_LARGE_SPEC": "0"}))]
    yield engs
    for _, e in engs:
        e.close()


class Fr:
    """one frame of a test batch and what its descriptor must say once delivered"""

    def __init__(self, rng, op, fin, plen, masked=True, rsv=0, form=None, msb=False):
        self.op, self.fin, self.plen, self.masked, self.rsv = op, fin, plen, masked, rsv
        self.key = rng.randbytes(4) if masked else None
        self.bytes = _frame(op, fin, rng.randbytes(plen), self.key, masked, rsv=rsv, len_form=form)
        self.hsz = len(self.bytes) - plen - (4 if masked else 0)
        if msb:  # the 64-bit length with its top bit set
            assert self.hsz == 10
            b = bytearray(self.bytes)
            b[2] |= 0x80
            self.bytes = bytes(b)


def _form(plen):
    """the length form that makes a masked frame plen + 14 bytes from 12 274 up (12 274 -> stride
    12 288, the threshold), except 16 384: the 16-bit form (stride 16 392)"""
    return 16 if plen == 16384 else 64


def _data(rng, n, plen, **kw):
    return [Fr(rng, 2 if i % 3 else 1, 1, plen, form=_form(plen), **kw) for i in range(n)]


def _wire(frames, stride, tail=b""):
    """frame i at i * stride (a shorter frame leaves its slot's rest as 0x5A filler)"""
    out = bytearray()
    for i, f in enumerate(frames):
        assert len(f.bytes) <= stride
        out += f.bytes
        if i + 1 < len(frames):
            out += b"\x5a" * (stride - len(f.bytes))
    return np.frombuffer(bytes(out + tail), np.uint8).copy()


def _decode(torch, eng, wire, n, stride, wl, mf=MF, mm=MM, is_server=1, no_desc=False):
    d = torch.from_numpy(np.concatenate([wire, np.full(64, 0xA5, np.uint8)])).to("cuda")
    desc, summ = eng.decode_inplace(d, n, stride=stride, wire_len=wl, max_frame_size=mf,
                                    max_message_size=mm, is_server=is_server, no_desc=no_desc)
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    assert (out[wire.size:] == 0xA5).all(), "write past the wire"
    return dict(summary=eng.read_summary(summ), desc=None if no_desc else eng.read_desc(desc, n),
                wire=out[:wire.size])


def _check_delivered(desc, frames, stride, nd):
    """descriptors of the delivered frames, field by field, from the frames the test built"""
    msgs = 0
    for i, f in enumerate(frames[:nd]):
        d = desc[i]
        km = 4 if f.masked else 0
        assert int(d["payload_off"]) == i * stride + f.hsz + km, i
        assert int(d["payload_len"]) == f.plen, i
        assert int(d["masking_key"]) == (int.from_bytes(f.key, "little") if f.masked else 0), i
        assert int(d["opcode"]) == f.op and int(d["header_size"]) == f.hsz, i
        assert int(d["wire_len"]) == f.hsz + km + f.plen, i
        data = f.op <= 2
        want = (FIN if f.fin else 0) | (MASK if f.masked else 0) | (MSG_END if data and f.fin else 0)
        assert int(d["flags"]) == want, (i, int(d["flags"]), want)
        assert int(d["message"]) == (msgs if data else 0), i
        msgs += 1 if data and f.fin else 0


def _check(torch, engines, wire, n, stride, wl=None, frames=None, **kw):
    wl = wire.size if wl is None else wl
    ref = _oracle.decode_batch(wire, n, stride=stride, wire_len=wl, max_frame_size=kw.get("mf", MF),
                               max_message_size=kw.get("mm", MM), is_server=kw.get("is_server", 1))
    outs = {}
    for name, e in engines:
        got = outs[name] = _decode(torch, e, wire, n, stride, wl, **kw)
        assert got["summary"] == ref["summary"], (name, got["summary"], ref["summary"])
        assert np.array_equal(got["wire"], ref["wire"]), (name, np.nonzero(got["wire"] != ref["wire"])[0][:8])
        if got["desc"] is None:
            continue
        assert np.array_equal(got["desc"]["status"], ref["status"]), (name, got["desc"]["status"], ref["status"])
        if frames is not None:
            _check_delivered(got["desc"], frames, stride, ref["summary"]["n_delivered"])
    if outs["off"]["desc"] is not None:
        for name in outs:  # every field of every frame, failed and skipped ones too
            assert np.array_equal(outs[name]["desc"], outs["off"]["desc"]), name
    nd = ref["summary"]["n_delivered"]
    if ref["summary"]["status"] != 0:  # the failing frame and everything after it: untouched
        assert np.array_equal(ref["wire"][nd * stride:wl], wire[nd * stride:wl])
        for name in outs:
            assert np.array_equal(outs[name]["wire"][nd * stride:], wire[nd * stride:]), name
    return ref


# ---- shapes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 65, 257])
@pytest.mark.parametrize("plen", [12274, 12275, 16384, 65536, 65537])
def test_shapes(torch, engines, plen, n):
    """16- and 64-bit length headers; strides that are and are not multiples of 16 and of 1 KiB (a
    tile with the tail of one frame and the head of the next); frame counts that are and are not
    multiples of the wave and block sizes; then the last slot longer than its frame"""
    rng = random.Random(plen * 1000 + n)
    frames = _data(rng, n, plen)
    stride = len(frames[0].bytes)
    assert stride >= 12288 and (plen != 12274 or stride == 12288)
    ref = _check(torch, engines, _wire(frames, stride), n, stride, frames=frames)
    assert ref["summary"]["n_delivered"] == n and ref["summary"]["n_messages"] == n
    ref = _check(torch, engines, _wire(frames, stride, tail=rng.randbytes(37)), n, stride, frames=frames)
    assert ref["summary"]["n_delivered"] == n


def test_slot_longer_than_frame(torch, engines):
    """a stride above the frames' wire length: every frame but the last breaks the layout; with one
    frame the slot is simply long"""
    rng = random.Random(5)
    for n in (1, 3):
        frames = _data(rng, n, 16384)
        stride = len(frames[0].bytes) + 24
        ref = _check(torch, engines, _wire(frames, stride, tail=bytes(24)), n, stride, frames=frames)
        assert ref["summary"]["n_delivered"] == (1 if n == 1 else 0)


# ---- the end of the wire -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 65])
def test_wire_end(torch, engines, n):
    rng = random.Random(n)
    for plen in (12274, 16384):
        frames = _data(rng, n, plen)
        stride = len(frames[0].bytes)
        wire = _wire(frames, stride)
        last = (n - 1) * stride
        for wl in (wire.size - 1, wire.size - 100, last + 4096 + 7,  # the last payload cut
                   last + 1, last + 3, last + 9, last + 13):        # the last header cut
            ref = _check(torch, engines, wire, n, stride, wl=wl, frames=frames)
            assert ref["summary"]["n_delivered"] == n - 1, wl
            assert ref["summary"]["first_status"] > 0  # INCOMPLETE
        # a whole batch whose length is no multiple of 16 (trailing bytes after the last frame)
        for extra in (1, 7, 15, 21):
            ref = _check(torch, engines, _wire(frames, stride, tail=rng.randbytes(extra)), n, stride,
                         frames=frames)
            assert ref["summary"]["n_delivered"] == n


# ---- breaks --------------------------------------------------------------------------------------------

KINDS = ["frag", "frag_open", "lone_cont", "ping", "close", "rsv", "unmasked", "unmasked_client", "msb",
         "too_big", "msg_limit"]


def _broken(rng, n, plen, kind, where):
    """-> frames, decode keywords"""
    form = _form(plen)
    frames = _data(rng, n, plen)
    kw = {}
    if kind == "frag":  # FIN = 0 start + continuation (a start in the last frame leaves it open)
        frames[where] = Fr(rng, 2, 0, plen, form=form)
        if where + 1 < n:
            frames[where + 1] = Fr(rng, 0, 1, plen, form=form)
    elif kind == "frag_open":  # a start that the next data frame does not continue
        frames[where] = Fr(rng, 1, 0, plen, form=form)
    elif kind == "lone_cont":
        frames[where] = Fr(rng, 0, 1, plen, form=form)
    elif kind == "ping":
        frames[where] = Fr(rng, 9, 1, 125)
    elif kind == "close":
        frames[where] = Fr(rng, 8, 1, 2)
    elif kind == "rsv":
        frames[where] = Fr(rng, 2, 1, plen, rsv=4, form=form)
    elif kind in ("unmasked", "unmasked_client"):  # 4 more payload bytes keep the stride
        frames[where] = Fr(rng, 2, 1, plen + 4, masked=False, form=form)
        kw["is_server"] = 1 if kind == "unmasked" else 0
    elif kind == "msb":
        frames[where] = Fr(rng, 2, 1, plen, form=64, msb=True)
    elif kind == "too_big":  # 6 more payload bytes under a 16-bit length: the same stride
        assert form == 64
        frames[where] = Fr(rng, 2, 1, plen + 6, form=16)
        kw["mf"] = plen + 5
    elif kind == "msg_limit":  # a fragmented message that crosses max_message_size at `where`
        frames = [Fr(rng, 2 if i == 0 else 0, 0, plen, form=form) for i in range(n)]
        kw["mm"] = plen * (where + 1) - 1
    return frames, kw


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", KINDS)
def test_breaks(torch, engines, kind, where):
    rng = random.Random(KINDS.index(kind) * 3 + ["first", "middle", "last"].index(where))
    for plen, n in ((12274, 5), (12275, 67)):  # (64-bit lengths: strides 12 288 and 12 289)
        w = {"first": 0, "middle": n // 2, "last": n - 1}[where]
        frames, kw = _broken(rng, n, plen, kind, w)
        stride = plen + 14
        ref = _check(torch, engines, _wire(frames, stride), n, stride, frames=frames, **kw)
        if kind in ("lone_cont", "rsv", "unmasked", "msb", "too_big", "frag_open") and \
                (kind != "frag_open" or w < n - 1):
            assert ref["summary"]["status"] == -1
            assert ref["summary"]["n_delivered"] == (w + 1 if kind == "frag_open" else w)
        if kind in ("unmasked_client",) or (kind == "frag" and w < n - 1):
            assert ref["summary"]["n_delivered"] == n


def test_two_breaks(torch, engines):
    rng = random.Random(77)
    n, plen = 9, 16384
    frames = _data(rng, n, plen)
    stride = len(frames[0].bytes)
    frames[2] = Fr(rng, 1, 0, plen, form=16)   # a valid fragmented message first
    frames[3] = Fr(rng, 0, 1, plen, form=16)
    frames[5] = Fr(rng, 2, 1, plen, rsv=2, form=16)
    frames[7] = Fr(rng, 0, 1, plen, form=16)
    ref = _check(torch, engines, _wire(frames, stride), n, stride, frames=frames)
    assert ref["summary"]["n_delivered"] == 5 and ref["summary"]["n_messages"] == 4


# ---- calls -----------------------------------------------------------------------------------------------

def test_no_descriptors(torch, engines):
    rng = random.Random(8)
    n, plen = 65, 12275
    frames = _data(rng, n, plen)
    stride = len(frames[0].bytes)
    _check(torch, engines, _wire(frames, stride), n, stride, no_desc=True)
    frames[40] = Fr(rng, 0, 1, plen, form=64)
    _check(torch, engines, _wire(frames, stride), n, stride, no_desc=True)
    frames[40] = Fr(rng, 1, 0, plen, form=64)
    frames[41] = Fr(rng, 0, 1, plen, form=64)
    _check(torch, engines, _wire(frames, stride), n, stride, no_desc=True)


def _batches(rng, n, plen):
    """a clean batch, one with a failure in the middle, one with a valid fragmented message"""
    clean = _data(rng, n, plen)
    bad = _data(rng, n, plen)
    bad[n // 2] = Fr(rng, 0, 1, plen, form=_form(plen))
    frag = _data(rng, n, plen)
    frag[1] = Fr(rng, 1, 0, plen, form=_form(plen))
    frag[2] = Fr(rng, 0, 1, plen, form=_form(plen))
    return [clean, bad, frag]


def _same_engine(torch, eng, batches, order, n, stride):
    t = torch
    wl = n * stride
    wire = t.zeros(wl + 64, dtype=t.uint8, device="cuda")
    desc, summ = eng.alloc_outputs(n)
    for k in order:
        host = _wire(batches[k], stride)
        wire[:wl].copy_(t.from_numpy(host))
        eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ)
        t.cuda.synchronize()
        ref = _oracle.decode_batch(host, n, stride=stride, wire_len=wl)
        assert eng.read_summary(summ) == ref["summary"], k
        assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), k
        assert np.array_equal(eng.read_desc(desc, n)["status"], ref["status"]), k
        _check_delivered(eng.read_desc(desc, n), batches[k], stride, ref["summary"]["n_delivered"])


def test_break_then_clean_then_break(torch, engines):
    """stale state of a break call (the ctl word, descriptors, info bytes) must not reach the next"""
    rng = random.Random(21)
    n, plen = 65, 12274
    batches = _batches(rng, n, plen)
    for name, eng in engines:
        _same_engine(torch, eng, batches, [1, 0, 1, 2, 0, 0, 1], n, len(batches[0][0].bytes))


def test_epoch_wrap(torch, monkeypatch):
    """host epochs started just below the wrap: calls across it, a break on each side"""
    import uvhttp_amd as U
    monkeypatch.setenv("UVHTTP_WS_EPOCH_START", str(U.epoch_limits()[0] - 3))
    monkeypatch.setenv("UVHTTP_WS_LARGE_SPEC", "1")
    eng = U.GpuEngine(0)
    try:
        rng = random.Random(22)
        n, plen = 5, 16384
        batches = _batches(rng, n, plen)
        seen = []
        for order in ([1, 0], [0, 1], [1, 2], [0]):
            _same_engine(torch, eng, batches, order, n, len(batches[0][0].bytes))
            seen.append(eng.epochs()[0])
        assert min(seen) < seen[0], seen  # the epoch fell: the calls crossed the wrap
    finally:
        eng.close()


def test_three_launch_pieces(torch, monkeypatch):
    rng = random.Random(23)
    n, plen = 3, 16384
    batches = _batches(rng, n, plen)
    stride = len(batches[0][0].bytes)
    tiles = (n * stride + 1023) // 1024
    monkeypatch.setenv("UVHTTP_WS_GRID_PIECE", str((tiles + 2) // 3))
    monkeypatch.setenv("UVHTTP_WS_LARGE_SPEC", "1")
    import uvhttp_amd as U
    eng = U.GpuEngine(0)
    try:
        eng.grid_pieces()
        _same_engine(torch, eng, batches, [0], n, stride)
        assert eng.grid_pieces() == (1, 3, tiles)
        _same_engine(torch, eng, batches, [1, 2, 0], n, stride)
    finally:
        eng.close()


def test_captured_and_replayed(torch):
    """one captured call replayed over re-masked wires: clean, clean again, a failure, clean"""
    t = torch
    rng = random.Random(24)
    n, plen = 65, 12275
    batches = _batches(rng, n, plen)
    stride = len(batches[0][0].bytes)
    wl = n * stride
    eng = _engine()
    try:
        wire = t.zeros(wl + 64, dtype=t.uint8, device="cuda")
        desc, summ = eng.alloc_outputs(n)
        eng.reserve(n, wl, 0)
        s = t.cuda.Stream()
        wire[:wl].copy_(t.from_numpy(_wire(batches[0], stride)))
        with t.cuda.stream(s):
            eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s)
        s.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=s):
            eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s)
        for k in (0, 0, 1, 2, 0):
            host = _wire(batches[k], stride)
            wire[:wl].copy_(t.from_numpy(host))
            t.cuda.synchronize()
            g.replay()
            t.cuda.synchronize()
            ref = _oracle.decode_batch(host, n, stride=stride, wire_len=wl)
            assert eng.read_summary(summ) == ref["summary"], k
            assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), k
            assert np.array_equal(eng.read_desc(desc, n)["status"], ref["status"]), k
            _check_delivered(eng.read_desc(desc, n), batches[k], stride, ref["summary"]["n_delivered"])
        # a host call between replays
        _same_engine(t, eng, batches, [1, 0], n, stride)
        wire[:wl].copy_(t.from_numpy(_wire(batches[0], stride)))
        t.cuda.synchronize()
        g.replay()
        t.cuda.synchronize()
        assert eng.read_summary(summ)["n_delivered"] == n
        eng.sync()
    finally:
        eng.close()


# ---- breaks in batches of several k_large_fix rounds (1 024 frames a round) ---------------------------
# 2 100 frames: rounds 0 and 1 whole, round 2 partial, a grid of 128 workgroups — the scan value
# carried across rounds, round r's descriptors stored by workgroup r, the SKIPPED tail rebuilt from
# the headers after the failing round.

N_ROUNDS, P_ROUNDS = 2100, 12274


@pytest.fixture(scope="module")
def round_frames():
    rng = random.Random(31)
    return _data(rng, N_ROUNDS, P_ROUNDS)


ROUND_CASES = {
    "fail_round0": [(300, (0, 1))],                      # a lone continuation: ERR_FRAGMENT
    "fail_round0_end": [(1023, (2, 1, 4))],              # RSV at the last frame of round 0
    "fail_round1_start": [(1024, (0, 1))],
    "fail_round1": [(1500, (2, 1, 4))],
    "fail_last_round": [(2080, (0, 1))],
    "fail_last_frame": [(2099, (2, 1, 4))],
    "frag_across_rounds": [(1023, (1, 0)), (1024, (0, 0)), (1025, (0, 1))],   # valid: no failure
    "frag_then_fail": [(1023, (2, 0)), (1024, (0, 1)), (2050, (1, 0)), (2051, (2, 1))],
    "open_at_end": [(2047, (1, 0)), (2048, (0, 0)), (2099, (0, 0))],
}


@pytest.mark.parametrize("no_desc", [False, True])
@pytest.mark.parametrize("case", sorted(ROUND_CASES))
def test_breaks_over_rounds(torch, engines, round_frames, case, no_desc):
    rng = random.Random(sorted(ROUND_CASES).index(case))
    frames = list(round_frames)
    for i, spec in ROUND_CASES[case]:
        op, fin = spec[0], spec[1]
        frames[i] = Fr(rng, op, fin, P_ROUNDS, rsv=spec[2] if len(spec) > 2 else 0, form=64)
    if case == "open_at_end":  # every data frame between the start and the end continues it
        for i in range(2049, 2099):
            frames[i] = Fr(rng, 0, 0, P_ROUNDS, form=64)
    stride = P_ROUNDS + 14
    ref = _check(torch, engines, _wire(frames, stride), N_ROUNDS, stride, frames=frames, no_desc=no_desc)
    s = ref["summary"]
    if case.startswith("fail_"):
        assert s["status"] == -1 and s["n_delivered"] == ROUND_CASES[case][0][0]
    elif case == "frag_across_rounds":
        assert s["n_delivered"] == N_ROUNDS and s["n_messages"] == N_ROUNDS - 2 and s["pending_bytes"] == 0
    elif case == "frag_then_fail":
        assert s["status"] == -1 and s["n_delivered"] == 2051
    else:
        assert s["n_delivered"] == N_ROUNDS and s["pending_bytes"] == 53 * P_ROUNDS


def test_breaks_over_five_rounds(torch, engines):
    """4 100 frames (five rounds, the last of 4 frames): a fragmented message over a round boundary
    and a failure in the last round"""
    rng = random.Random(41)
    n, plen = 4100, 12275
    frames = _data(rng, n, plen)
    frames[2047] = Fr(rng, 2, 0, plen, form=64)
    frames[2048] = Fr(rng, 0, 1, plen, form=64)
    stride = plen + 14
    ref = _check(torch, engines, _wire(frames, stride), n, stride, frames=frames)
    assert ref["summary"]["n_delivered"] == n and ref["summary"]["n_messages"] == n - 1
    frames[4097] = Fr(rng, 0, 1, plen, form=64)
    ref = _check(torch, engines, _wire(frames, stride), n, stride, frames=frames)
    assert ref["summary"]["n_delivered"] == 4097 and ref["summary"]["status"] == -1


# 16 500 frames: k_large_fix passes eight rounds of simple frames in one step where it can (twice
# here), single rounds from their info bytes elsewhere, and reads headers only in a round with a
# frame that is not simple, one entered with a message open, and the last.

SUPER_CASES = {
    # a fragmented message early: every later round and the second eight-round step renumber messages
    "frag_early": ([(100, (1, 0)), (101, (0, 1))], 16500, 16499),
    # the first eight-round step whole, a failure inside the second: single rounds, then the SKIPPED tail
    "fail_in_second_step": ([(12000, (0, 1))], 12000, None),
    # a message open across the boundary of the first step, closed in the next round
    "open_across_steps": ([(8191, (2, 0)), (8192, (0, 1))], 16500, 16499),
}


@pytest.mark.parametrize("case", sorted(SUPER_CASES))
def test_breaks_over_eight_round_steps(torch, engines, case):
    rng = random.Random(61)
    n, plen = 16500, 12274
    frames = [Fr(rng, 2, 1, plen, form=64)] * n  # (one frame's bytes in every slot)
    edits, delivered, messages = SUPER_CASES[case]
    for i, (op, fin) in edits:
        frames[i] = Fr(rng, op, fin, plen, form=64)
    stride = plen + 14
    ref = _check(torch, [e for e in engines if e[0] != "product"], _wire(frames, stride), n, stride,
                 frames=frames)
    assert ref["summary"]["n_delivered"] == delivered
    assert messages is None or ref["summary"]["n_messages"] == messages


# ---- which launches ran -------------------------------------------------------------------------------

def test_paths_taken(torch, engines):
    """the product library and UVHTTP_WS_LARGE_SPEC=1 take decode_large (the payload kernel first,
    then k_large_fix, stamped "plan"); UVHTTP_WS_LARGE_SPEC=0 runs k_plan before the payload kernel;
    a stride below 12 KiB keeps k_plan first on every engine"""
    rng = random.Random(51)
    for plen, form, large in ((12274, 64, True), (12274, 16, False)):
        n = 5
        frames = [Fr(rng, 2, 1, plen, form=form) for _ in range(n)]
        stride = len(frames[0].bytes)
        assert (stride >= 12288) == large
        wire = _wire(frames, stride)
        for name, eng in engines:
            eng.set_stamps(True)
            eng.read_stamps()
            try:
                _decode(torch, eng, wire, n, stride, wire.size)
                recs = eng.read_stamps()
            finally:
                eng.set_stamps(False)
            order = [k for _, _, k in sorted((b, e, k) for _, k, b, e in recs)]
            want = ["payload", "plan"] if large and name != "off" else ["plan", "payload"]
            assert order == want, (name, plen, form, order)
