"""The epoch wrap (ws_gpu.hip next_epoch / k_epoch; DESIGN.md "Epoch-tagged state").

Every decode and build call takes a fresh epoch and tags the scratch that replaces reset passes
with it.  Host epochs run 1 .. kMaxHostEpoch, the epochs of replayed captured calls
kMaxHostEpoch + 1 .. kMaxEpoch; when either half is used up every tagged item must be cleared
before the first epoch is issued again, or an entry of an earlier call matches a live tag (the ==
compared ones) or outranks a live claim (the max-claimed ones).  These tests run calls across
that event three ways — an engine started a few calls before the end of the host's half
(UVHTTP_WS_EPOCH_START), an engine whose host epochs run 1 .. 5 (UVHTTP_WS_EPOCH_PERIOD=5: within
16 calls every epoch value meets every call shape again, a good call the epoch a broken one used
a cycle earlier), and a captured call replayed from a few replays before the end of the device's
half (UVHTTP_WS_DEV_EPOCH_START) — and compare every call with the CPU oracle, bytes and records.
Each asserts through GpuEngine.epochs() that the epoch really fell: a start value the library
silently replaced is how the older wrap test came to run at epochs 1 .. 16.

The start values come from U.epoch_limits() (the library's constants), see starts()."""
import random

import numpy as np
import pytest

import _oracle
import test_gpu_build as TB
import test_gpu_desc_emit as TD
import test_gpu_summary_compact as TS
from test_gpu_parity import _compare, _frame, _rand_batch, _run_both
from test_gpu_stream_spec import _build, _conn_frames, _run

pytestmark = pytest.mark.gpu

HOST_BACK = 3    # calls before the last host epoch at which the host-wrap engines start
DEV_BACK = 3     # replays before the last device epoch at which the captured-call engines start
PERIOD = 5       # UVHTTP_WS_EPOCH_PERIOD of the full-cycle tests (coprime with their 3-call pattern)


def starts():
    """every epoch start value these tests set, by knob (test_epoch_wrap_host.py checks them
    against the limits without a GPU)"""
    import uvhttp_amd as U
    max_host, max_epoch = U.epoch_limits()
    return {"UVHTTP_WS_EPOCH_START": [max_host - HOST_BACK],
            "UVHTTP_WS_DEV_EPOCH_START": [max_epoch - DEV_BACK],
            "UVHTTP_WS_EPOCH_PERIOD": [PERIOD]}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _engine(monkeypatch, env, stamps=False):
    import uvhttp_amd as U
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        e = U.GpuEngine(0)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    if stamps:
        e.set_stamps(True)
    return e


def _stream_engines(monkeypatch, env, first=None):
    """(the engine under test with stamps on, the walk-only engine), both with `env`"""
    a = _engine(monkeypatch, dict(env, **(first or {})), stamps=True)
    b = _engine(monkeypatch, dict(env, UVHTTP_WS_STREAM_SPEC="0"))
    return a, b


def _wrap_env(wrap):
    s = starts()
    return {"UVHTTP_WS_EPOCH_START": s["UVHTTP_WS_EPOCH_START"][0]} if wrap == "end" else \
        {"UVHTTP_WS_EPOCH_PERIOD": s["UVHTTP_WS_EPOCH_PERIOD"][0]}


def _falls(seen):
    return sum(1 for i in range(1, len(seen)) if seen[i] < seen[i - 1])


# ---- stream shapes ------------------------------------------------------------------------------
# A: 48 connections x 12 frames of 250 payload bytes (258 on the wire): 10 tiles of 16 KiB, five
#    or six connections a tile, so the pass's general path (a third connection sets kStMore)
# B: 300 connections x 10 frames of 58 payload bytes (64 on the wire): 12 tiles, 25 or 26
#    connections a tile (general path); its tile claims name other connection indices than A's
# C: 6 connections x 100 frames of 250 bytes: 10 tiles, at most 2 connections a tile — the
#    SpecTile fast path
SHAPES = {"A": (48, 12, 250), "B": (300, 10, 58), "C": (6, 100, 250)}


def _streams(rng, shape, broken=None, gap=0):
    """fresh random payloads and keys; broken = (kind, connection): "other_length" (one frame 9
    bytes longer: the pass breaks the speculation), "rsv" (one frame with a reserved bit: the
    same, at the same wire length) or "limit" (a max_message_size the connection's frames could
    reach: k_sspec_plan leaves the call to the walk); gap: zero bytes between connections"""
    n_conns, per, plen = SHAPES[shape]
    conns = []
    for i in range(n_conns):
        frames, _ = _conn_frames(rng, per, plen, False, p_frag=0.3)
        mm = 0
        if broken and i == broken[1]:
            if broken[0] == "other_length":
                frames[per // 2] = _frame(2, 1, rng.randbytes(plen + 9), rng.randbytes(4))
            elif broken[0] == "rsv":
                frames[per // 2] = _frame(2, 1, rng.randbytes(plen), rng.randbytes(4), rsv=2)
            else:
                mm = 1000
        conns.append((frames, b"", 0, 0, 16 << 20, mm))
    wire, st = _build(conns, gap=gap)
    n = n_conns * per
    return wire, st, max(8 * n_conns, n + n_conns, 64)


def _oracle_delivers_all(shape):
    """on the CPU: the oracle alone delivers every frame of the shape, so a fall-back on the
    device can only come from the device"""
    n_conns, per, _ = SHAPES[shape]
    wire, st, cap = _streams(random.Random(shape), shape)
    out, _, total = _oracle.decode_streams(wire.copy(), st, None, max_frames=cap)
    assert (out["rc"] == 0).all() and (out["n_frames"] == per).all() and total == n_conns * per
    assert wire.size < 1 << 20


# ---- (b) the speculative stream decode across the host wrap -----------------------------------------

@pytest.mark.parametrize("pair", ["AB", "CB"])
def test_stream_spec_across_host_wrap(torch, monkeypatch, pair):
    """Six calls alternating two shapes on fresh engines that start three calls before the last
    host epoch and never capture a graph: every call must take the speculative path and equal
    the walk engine and the oracle.  Left uncleared, the tile claims in kScrSp (conn_tile,
    claimed with a plain atomicMax of (epoch << 32) | ~connection) of the calls before the wrap
    outrank every claim after it: tag_get finds no connection for the tile, k_sspec_tiles writes no
    SpecTile, k_sspec_pass returns at "no connection's frames touch the tile" without a break, and
    k_sspec_emit reports frames decoded that nobody unmasked (the payloads and keys are fresh in
    every call, so masked bytes cannot equal the oracle's)."""
    import uvhttp_amd as U
    for sh in pair:
        _oracle_delivers_all(sh)
    engines = _stream_engines(monkeypatch, _wrap_env("end"))
    try:
        max_host = U.epoch_limits()[0]
        assert [e.epochs()[0] for e in engines] == [max_host - HOST_BACK] * 2
        rng = random.Random("b" + pair)
        seen = []
        for k in range(6):
            wire, st, cap = _streams(rng, pair[k % 2])
            _run(torch, engines, wire, st, max_frames=cap, spec_expected=True)
            seen.append([e.epochs()[0] for e in engines])
        want = [max_host - 2, max_host - 1, max_host, 1, 2, 3]
        assert seen == [[w, w] for w in want], seen
    finally:
        for e in engines:
            e.close()


# ---- (c) full cycles: every epoch value meets every shape again --------------------------------------

@pytest.mark.parametrize("variant", ["other_length", "limit", "gaps"])
def test_stream_calls_full_cycle(torch, monkeypatch, variant):
    """16 stream calls in a repeating pattern of three on engines whose host epochs run 1 .. 5.
    Good calls must speculate, the broken one must not, all equal the oracle.
    other_length — A good, B good, A with one frame of another length in connection 10: the pass
      sets ctl[kCtlSpecBreak] = epoch; left there, the good call that takes the epoch a cycle
      later goes down the fall-back (spec_expected);
    limit — the broken call has a message limit connection 3 could reach instead, so
      k_sspec_plan sets ctl[kCtlSpecOff] = epoch: the same for that word;
    gaps — C good, C with 40 000 zero bytes between its connections (tiles 2 and 3 lie inside the
      first gap: no claim, no SpecTile written), C broken: a SpecTile of the gapless call with
      SpecTile.tag = epoch is still there a cycle later, and k_sspec_pass would decode the gap's
      zero bytes by it."""
    shapes = "CC" if variant == "gaps" else "AB"
    for sh in set(shapes):
        _oracle_delivers_all(sh)
    engines = _stream_engines(monkeypatch, _wrap_env("period"))
    try:
        rng = random.Random("c-streams-" + variant)
        seen = []
        for k in range(16):
            broken = None
            if k % 3 == 2:
                broken = ("limit", 3) if variant == "limit" else ("other_length", 10 % SHAPES[shapes[0]][0])
            wire, st, cap = _streams(rng, shapes[k % 3 == 1], broken,
                                     gap=40000 if variant == "gaps" and k % 3 == 1 else 0)
            _run(torch, engines, wire, st, max_frames=cap, spec_expected=broken is None)
            seen.append(engines[0].epochs()[0])
        assert seen == [k % PERIOD + 1 for k in range(16)] and _falls(seen) == 3, seen
    finally:
        for e in engines:
            e.close()


def test_fused_walk_full_cycle(torch, monkeypatch):
    """The same cycle through k_swalk_fused (UVHTTP_WS_WALK_FUSE=1, no speculation), whose tags
    live in kScrSs: the look-back records (srec, (epoch << 2) | kind) and ctr[2], the epoch of the
    latest call over capacity.  Every third call has a frame capacity below its frames
    (ERR_CAPACITY, nothing decoded); left uncleared, ctr[2] makes the good call that takes the
    same epoch a cycle later report ERR_CAPACITY too."""
    engines = _stream_engines(monkeypatch, _wrap_env("period"),
                              first={"UVHTTP_WS_WALK_FUSE": "1", "UVHTTP_WS_STREAM_SPEC": "0"})
    try:
        rng = random.Random("c-fused")
        seen = []
        for k in range(16):
            sh = "AB"[k % 3 == 1]
            wire, st, cap = _streams(rng, sh)
            over = k % 3 == 2
            a = _run(torch, engines, wire, st, max_frames=SHAPES[sh][0] * SHAPES[sh][1] - 1 if over else cap)
            assert (a["res"]["first_status"] == -10).all() == over, k
            assert "walk" in a["kinds"] and "spec_plan" not in a["kinds"], a["kinds"]
            seen.append(engines[0].epochs()[0])
        assert _falls(seen) == 3, seen
    finally:
        for e in engines:
            e.close()


def _stride_frames(rng, n, plen, bad=None):
    frames = [_frame(rng.choice([1, 2]), 1, rng.randbytes(plen), rng.randbytes(4)) for _ in range(n)]
    if bad == "layout":  # test_gpu_parity.test_stride_layouts' "layout": a frame one byte longer
        frames[n // 2] = _frame(2, 1, rng.randbytes(plen + 1), rng.randbytes(4))
    return np.frombuffer(b"".join(frames), np.uint8).copy(), len(frames[0])


@pytest.mark.parametrize("kind", ["summary_compact", "desc_emit", "fused_inplace", "offset_table"])
def test_stride_and_table_calls_full_cycle(torch, monkeypatch, kind):
    """16 batch calls (good, good of another size, broken) on one engine whose host epochs run
    1 .. 5, each against the oracle:
    summary_compact — summary-only compact decode; the broken call (a reserved opcode) sets
      ctl[kCtlGate] = epoch and is decoded again by k_plan + k_spec_fix.  A stale gate sends the
      good call of that epoch a cycle later the same way (read off the stamps);
    desc_emit — in place with descriptors through k_desc_emit (asserted from the stamps), the
      broken call a reserved bit: first_bad / spec_bad and the scan's records in kScrWs;
    fused_inplace — 600 frames of 60 and of 1000 payload bytes in place, the broken call with one
      frame a byte longer (ERR_LAYOUT): tile_first, first_bad and k_plan's look-back records
      ((epoch << 2) | kind, accepted by ==) in kScrWs;
    offset_table — 3000 and 40 frames by offset table, in place and compact, the broken call with
      failing frames: tile_first, arena_first, first_bad, the look-back records."""
    e = _engine(monkeypatch, _wrap_env("period"), stamps=True)
    try:
        rng = random.Random("c-" + kind)
        seen = []
        for k in range(16):
            bad = k % 3 == 2
            if kind == "summary_compact":
                stride, n = (1000, 800) if k % 3 == 1 else (264, 3000)
                tw = TS._tweak("reserved_opcode", 777, TS._uniform_p(stride)) if bad else None
                # (the frame off the speculation counts only when it is delivered)
                TS._check(torch, (e,), TS._batch(rng, n, stride, frag=0.3, tweak=tw), n, stride,
                          fast=(lambda r: r["summary"]["n_delivered"] <= 777) if bad else True)
            elif kind == "desc_emit":
                plen, n = (1000, 700) if k % 3 == 1 else (256, 3000)

                def tw(i, f, fin, open_msg, at=n // 2):
                    return (bytes([f[0] | 0x20]) + f[1:], fin) if i == at else (f, fin)
                wire = TD._frag_batch(rng, n, plen, 0.4, tw if bad else None)
                ref = TD._check(torch, [e], wire, n, wire.size // n, emit=True)
                assert (ref["summary"]["status"] != 0) == bad
            elif kind == "fused_inplace":
                wire, stride = _stride_frames(rng, 600, 1000 if k % 3 == 1 else 60,
                                              "layout" if bad else None)
                ref, got = _run_both(torch, e, wire, 600, stride=stride)
                assert (ref["summary"]["status"] != 0) == bad
                _compare(ref, got)
            else:
                n = 40 if k % 3 == 1 else 3000
                wire, offs = _rand_batch(rng, n, [0, 3, 125, 300, 1000], p_ctrl=0.1, p_frag=0.3,
                                         p_bad=0.002 if bad else 0.0)
                for compact in (False, True):
                    ref, got = _run_both(torch, e, wire, n, offs=offs, mm=0, compact=compact)
                    _compare(ref, got, compact)
            seen.append(e.epochs()[0])
        assert _falls(seen) >= 3 and max(seen) == PERIOD and min(seen) == 1, seen
    finally:
        e.close()


# ---- (d) the send side ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "tiles"])
@pytest.mark.parametrize("wrap", ["end", "period"])
def test_build_frames_across_wrap(torch, monkeypatch, wrap, path):
    """build_frames, server and masked frames mixed, alternating 2000 x 60-byte frames (the small-
    frame emit) and 40 x 20000-byte frames (the >= 4 KiB shape) across the host wrap and through
    full cycles, against the oracle's build_frame.  The output map records (BuildRec.tag, ==) live
    in kScrBs; "tiles" (UVHTTP_WS_BUILD_FRAMES=0) makes the small frames take map records too, at
    another map granularity than the large ones."""
    import uvhttp_amd as U
    env = _wrap_env(wrap)
    if path == "tiles":
        env["UVHTTP_WS_BUILD_FRAMES"] = "0"
    e = _engine(monkeypatch, env)
    try:
        rng = random.Random(f"d-{wrap}-{path}")
        seen = []
        for k in range(6 if wrap == "end" else 11):
            n, plen = (40, 20000) if k % 2 else (2000, 60)
            src = np.frombuffer(rng.randbytes(200000), np.uint8).copy()
            frames = TB._rand_frames(rng, src.size, n, [plen])
            exp, total, out, off = TB._build(torch, e, src, frames)
            assert int(off[n]) == total
            assert np.array_equal(off[:n], np.cumsum([0] + [len(b) for b in exp[:-1]]))
            assert out[:total].tobytes() == b"".join(exp), k
            assert not out[total:].any()
            seen.append(e.epochs()[0])
        if wrap == "end":
            mh = U.epoch_limits()[0]
            assert seen == [mh - 2, mh - 1, mh, 1, 2, 3], seen
        else:
            assert seen == [k % PERIOD + 1 for k in range(11)], seen
    finally:
        e.close()


# ---- (e) captured calls across the device wrap ----------------------------------------------------

def _device_wrapped(dev, first):
    """the device epochs read after each replay: one more per replay from `first`, up to
    kMaxEpoch, then kMaxHostEpoch + 1 and on"""
    import uvhttp_amd as U
    max_host, max_epoch = U.epoch_limits()
    want, v = [], first
    for _ in dev:
        v = max_host + 1 if v >= max_epoch else v + 1
        want.append(v)
    assert dev == want and max(dev) == max_epoch and dev[-1] > max_host and _falls(dev) == 1, dev


def test_captured_stride_across_device_wrap(torch, monkeypatch):
    """A stride decode_inplace captured after uncaptured warm calls and replayed eight times over
    changing bytes (no failure, an early state-machine failure, none, a late one) from three
    replays before the last device epoch, with a host call of another shape after replays 3 and
    6: k_epoch's wrap branch clears the scratch and the epoch-holding ctl words and restarts the
    device epochs, and every result equals the oracle's."""
    import uvhttp_amd as U
    t = torch
    first = starts()["UVHTTP_WS_DEV_EPOCH_START"][0]
    eng = _engine(monkeypatch, {"UVHTTP_WS_DEV_EPOCH_START": first})
    try:
        rng = random.Random("e-stride")
        n, plen = 3000, 200

        def batch(fail_at):
            return b"".join(_frame(0 if i == fail_at else 2, 1, rng.randbytes(plen), rng.randbytes(4))
                            for i in range(n))
        stride = len(batch(None)) // n
        wl = stride * n
        wire = t.zeros(wl + 64, dtype=t.uint8, device="cuda")
        desc, summ = eng.alloc_outputs(n)
        s = t.cuda.Stream()

        def host_call(k):  # another shape, uncaptured: 600 frames of 60 / 1000 bytes, in place
            w, st2 = _stride_frames(rng, 600, 1000 if k % 2 else 60, "layout" if k == 1 else None)
            ref, got = _run_both(t, eng, w, 600, stride=st2)
            _compare(ref, got)
        eng.reserve(n, wl, 0)
        host_call(0)
        host_call(3)
        wire[:wl].copy_(t.from_numpy(np.frombuffer(batch(None), np.uint8).copy()))
        with t.cuda.stream(s):
            eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s)
        s.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=s):
            eng.decode_inplace(wire, n, stride=stride, wire_len=wl, desc=desc, summary=summ, stream=s)
        assert eng.epochs(s)[1] == first
        dev = []
        for r, fail_at in enumerate([None, 37, None, 2900, 37, None, 1500, None]):
            host = np.frombuffer(batch(fail_at), np.uint8).copy()
            wire[:wl].copy_(t.from_numpy(host))
            t.cuda.synchronize()
            g.replay()
            t.cuda.synchronize()
            ref = _oracle.decode_batch(host, n, stride=stride, wire_len=wl)
            assert (ref["summary"]["status"] != 0) == (fail_at is not None)
            assert eng.read_summary(summ) == ref["summary"], r
            assert np.array_equal(wire[:wl].cpu().numpy(), ref["wire"]), r
            assert np.array_equal(eng.read_desc(desc, n)["status"], ref["status"]), r
            dev.append(eng.epochs(s)[1])
            if r in (2, 5):
                host_call(r - 1)  # (1: a failing batch, 4: a good one)
        _device_wrapped(dev, first)
        eng.sync()
        assert U
    finally:
        eng.close()


def test_captured_streams_across_device_wrap(torch, monkeypatch):
    """The same for a captured decode_streams of shape A: replays alternate between bytes whose
    speculation holds and bytes with a reserved bit in connection 10 (same wire length: the
    captured call's fall-back, kCtlSpecBreak = the device epoch), with an uncaptured call of shape
    B after replays 3 and 6.  Results and wire equal the oracle's; results, descriptors and wire
    equal the walk engine's."""
    import uvhttp_amd as U
    t = torch
    first = starts()["UVHTTP_WS_DEV_EPOCH_START"][0]
    eng = _engine(monkeypatch, {"UVHTTP_WS_DEV_EPOCH_START": first})
    walk = _engine(monkeypatch, {"UVHTTP_WS_STREAM_SPEC": "0"})
    try:
        rng = random.Random("e-streams")

        def host_call():
            w, st2, cap2 = _streams(rng, "B")
            _run(t, (eng, walk), w, st2, max_frames=cap2)
        wire0, st, cap = _streams(rng, "A")
        n_st, wl = st.size, wire0.size
        d = t.full((wl + 64,), 0xA5, dtype=t.uint8, device="cuda")
        d[:wl] = t.from_numpy(wire0).to("cuda")
        dev_st = t.from_numpy(st.view(np.uint8).copy()).to("cuda")
        desc = t.zeros((cap + 1) * 32, dtype=t.uint8, device="cuda")
        res = t.zeros(n_st * U.STREAM_RESULT_BYTES, dtype=t.uint8, device="cuda")
        s = t.cuda.Stream()
        host_call()  # (the larger shape first: nothing grows after the capture)
        with t.cuda.stream(s):
            eng.decode_streams(d, dev_st, n_st, cap, desc=desc, results=res, wire_len=wl, stream=s)
        s.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=s):
            eng.decode_streams(d, dev_st, n_st, cap, desc=desc, results=res, wire_len=wl, stream=s)
        assert eng.epochs(s)[1] == first
        dev = []
        for r in range(8):
            wire, st_r, _ = _streams(rng, "A", ("rsv", 10) if r % 2 else None)
            assert wire.size == wl and (st_r == st).all()
            d[:wl] = t.from_numpy(wire).to("cuda")
            t.cuda.synchronize()
            g.replay()
            t.cuda.synchronize()
            got = res.cpu().numpy().view(U.STREAM_RESULT_DT).copy()
            got_wire = d[:wl].cpu().numpy()
            host = wire.copy()
            o, _, total = _oracle.decode_streams(host, st, None, max_frames=cap)
            assert (o["rc"] != 0).any() == bool(r % 2)
            assert np.array_equal(got["n_delivered"], o["n_frames"]), r
            assert np.array_equal(got["status"], o["rc"]) and np.array_equal(got["first_status"], o["reason"]), r
            assert np.array_equal(got["calls"], o["calls"])
            assert np.array_equal(got["consumed_bytes"], o["consumed"])
            assert np.array_equal(got["pending_bytes"], o["frag_size"])
            assert np.array_equal(got["buffered_end"], o["consumed"] + o["recv_pos"])
            assert np.array_equal(got_wire, host), (r, np.nonzero(got_wire != host)[0][:8])
            assert (d[wl:] == 0xA5).all()
            nf = int(got["n_frames"].sum())
            got_desc = eng.read_desc(desc, max(nf, 1))[:nf].copy()
            # the walk engine on the same bytes
            d2 = t.from_numpy(np.concatenate([wire, np.full(64, 0xA5, np.uint8)])).to("cuda")
            desc2, res2 = walk.decode_streams(d2, dev_st, n_st, cap, wire_len=wl)
            t.cuda.synchronize()
            ref = res2[: n_st * U.STREAM_RESULT_BYTES].cpu().numpy().view(U.STREAM_RESULT_DT)
            assert np.array_equal(got, ref), r
            assert np.array_equal(got_desc, walk.read_desc(desc2, max(nf, 1))[:nf]), r
            assert np.array_equal(got_wire, d2[:wl].cpu().numpy()), r
            dev.append(eng.epochs(s)[1])
            if r in (2, 5):
                host_call()
        _device_wrapped(dev, first)
        eng.sync()
    finally:
        eng.close()
        walk.close()


# ---- the knobs refuse what they cannot honour -----------------------------------------------------

@pytest.mark.parametrize("knob,value", [
    ("UVHTTP_WS_EPOCH_START", lambda mh, me: mh),          # the last host epoch is not a start
    ("UVHTTP_WS_EPOCH_START", lambda mh, me: (1 << 30) - 4),  # (what the older wrap test set)
    ("UVHTTP_WS_EPOCH_START", lambda mh, me: "soon"),
    ("UVHTTP_WS_EPOCH_PERIOD", lambda mh, me: 1),
    ("UVHTTP_WS_EPOCH_PERIOD", lambda mh, me: mh + 1),
    ("UVHTTP_WS_DEV_EPOCH_START", lambda mh, me: mh),
    ("UVHTTP_WS_DEV_EPOCH_START", lambda mh, me: me + 1)],
    ids=["start=max_host", "start=2^30-4", "start=word", "period=1", "period=max_host+1",
         "dev_start=max_host", "dev_start=max_epoch+1"])
def test_out_of_range_epoch_knobs_fail_engine_creation(torch, monkeypatch, knob, value):
    import uvhttp_amd as U
    monkeypatch.setenv(knob, str(value(*U.epoch_limits())))
    with pytest.raises(U.GpuError, match=knob):
        U.GpuEngine(0)
