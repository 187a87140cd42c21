"""Every chunked pass in more than one piece (ws_engine_int.h for_grid_chunks; DESIGN.md "The
host call frame and the scratch blocks").

A pass of more than 2^24 workgroups goes out in several launches, each handed its first
workgroup's index in the whole pass (tile_base).  The kernels use that index for more than the
tile's address: which workgroups also finalize descriptors, which one writes the summary, which
one does the plain unmask's head and tail bytes, where a stamp word goes, which UTF-8 tile a wave
judges.  The smallest pass that splits on its own covers 16 GiB of wire, so these tests make the
piece small instead (UVHTTP_WS_GRID_PIECE=N, the experiment build only) and run every chunked
pass at the smallest shapes with at least five tiles in pieces of N = 1 and 3 workgroups — and,
on one case per path, N = tiles - 1 (a last piece of one workgroup) and N = tiles (one piece).

Every case is compared with the CPU oracle or the Python reference exactly as the existing test
of its path compares it (the helpers are those tests' own), and byte for byte with an unsplit
engine (the product library, or the experiment build without the knob) on the same input.  Each
asserts through GpuEngine.grid_pieces() that its calls really went out in the pieces it meant: a
knob the library silently ignored would leave these tests running what every other test runs.

The piece values that do not depend on a tile count come from pieces(); test_grid_pieces_host.py
checks them against the accepted range without a GPU."""
import contextlib
import random

import numpy as np
import pytest

import _oracle
import _utf8_frames_ref as FR
import _utf8_ref as R
import test_gpu_build as TB
import test_gpu_epoch_wrap as W
import test_gpu_summary_compact as TS
import test_gpu_summary_only as SO
import test_gpu_utf8 as T8
import test_gpu_utf8_frames as TF
from test_gpu_epoch_wrap import _engine
from test_gpu_parity import _compare, _frame, _rand_batch, _run_both, _to_dev
from test_gpu_stream_spec import _run

pytestmark = pytest.mark.gpu

KNOB = "UVHTTP_WS_GRID_PIECE"
TILE_SHAPES = [(64, 1), (64, 2), (64, 4), (128, 1), (128, 2), (256, 1), (256, 2), (256, 4)]


def pieces():
    """the piece sizes every case runs with (the edge cases add tiles - 1 and tiles, read off
    the hook)"""
    return [1, 3]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _ceil(a, b):
    return -(-a // b)


@contextlib.contextmanager
def _pair(monkeypatch, n, env=None, stamps=False):
    """(the engine whose passes go out in pieces of n workgroups, the unsplit engine), both
    with `env`"""
    import uvhttp_amd as U
    assert 1 <= n <= U.max_grid(), n
    env = dict(env or {})
    split = _engine(monkeypatch, dict(env, **{KNOB: n}), stamps=stamps)
    try:
        whole = _engine(monkeypatch, env, stamps=stamps)
        try:
            assert split.grid_pieces() == (0, 0, 0)
            yield split, whole
        finally:
            whole.close()
    finally:
        split.close()


def _took(eng, n, passes=1, tiles=None, least=5):
    """the hook's figures for the calls since the last read: `passes` chunked passes, each in
    ceil(tiles / n) launches (asserted exactly for a single pass), at least two per pass unless
    n covers the pass -> the tiles covered"""
    p, pc, t = eng.grid_pieces()
    assert p == passes, (p, pc, t)
    assert t >= least * passes, (p, pc, t)
    if tiles is not None:
        assert t == tiles, (t, tiles)
    if passes == 1:
        assert pc == _ceil(t, n), (pc, t, n)
        assert pc >= 2 or n >= t
    else:
        assert _ceil(t, n) <= pc <= _ceil(t, n) + passes - 1 and pc >= 2 * passes, (p, pc, t, n)
    return t


def _same(a, b, compact=False):
    """two engines' outputs of _run_both on the same input, byte for byte"""
    assert a["summary"] == b["summary"]
    assert a["desc"].tobytes() == b["desc"].tobytes(), np.nonzero(a["desc"] != b["desc"])[0][:5]
    assert np.array_equal(a["wire"], b["wire"])
    if compact:
        nb = a["summary"]["arena_bytes"]
        assert np.array_equal(a["arena"][:nb], b["arena"][:nb])
        assert a["msgs"].tobytes() == b["msgs"].tobytes()


def _batch_both(torch, engines, wire, n, compact=False, **kw):
    """_run_both + _compare on the split engine and on the unsplit one, and the two against
    each other -> the oracle's result"""
    outs = []
    for e in engines:
        ref, got = _run_both(torch, e, wire.copy(), n, compact=compact, **kw)
        _compare(ref, got, compact)
        outs.append(got)
    _same(outs[0], outs[1], compact)
    return ref


def _with_edges(monkeypatch, env, run, stamps=False, passes=1):
    """run(engines, n) at N = 1 and 3, then at N = tiles - 1 and N = tiles with the tile count
    the hook gave; run returns after its calls, _took checks the pieces"""
    tiles = None
    for n in pieces():
        with _pair(monkeypatch, n, env, stamps) as engines:
            run(engines, n)
            tiles = _took(engines[0], n, passes=passes)
    assert passes == 1
    for n, want in ((tiles - 1, 2), (tiles, 1)):
        with _pair(monkeypatch, n, env, stamps) as engines:
            run(engines, n)
            p, pc, t = engines[0].grid_pieces()
            assert (p, pc, t) == (1, want, tiles), (n, p, pc, t)


# ---- offset-table batches: k_unmask_inplace, k_scatter_compact, k_gather_compact -----------------

TABLE_SIZES = [0, 1, 125, 126, 4096, 65536]


def _table_batch(bad):
    """40 frames by offset table (seeds chosen on the CPU oracle): all delivered; or, bad, with
    failing frames among them, the first one 135 498 bytes into the wire — past the first piece
    at every tile shape"""
    rng = random.Random("table-2-True" if bad else "table-8-False")
    return _rand_batch(rng, 40, TABLE_SIZES, p_bad=0.1 if bad else 0.0) + (40,)


def _zero_batch(bad_at=None):
    """5 000 masked zero-payload frames: 30 000 wire bytes, so ceil(n / BLOCK) finalizing
    workgroups reach past the wire's tiles at every tile shape; bad_at: that frame has a reserved
    bit, so every finalizing workgroup has statuses to rewrite (SKIPPED from there on)"""
    rng = random.Random("zero")
    frames = [_frame(2, 1, b"", rng.randbytes(4), rsv=4 if i == bad_at else 0) for i in range(5000)]
    wire = np.frombuffer(b"".join(frames), np.uint8).copy()
    assert wire.size == 30000
    return wire, (np.arange(5000, dtype=np.uint64) * 6), 5000


def _big_batch():
    """3 frames of 65 536 payload bytes: the gather's arena tiles"""
    rng = random.Random("big")
    frames = [_frame(2, 1, rng.randbytes(65536), rng.randbytes(4)) for _ in range(3)]
    offs = np.cumsum([0] + [len(f) for f in frames[:-1]]).astype(np.uint64)
    return np.frombuffer(b"".join(frames), np.uint8).copy(), offs, 3


@pytest.mark.parametrize("bad", [False, True], ids=["valid", "failing"])
def test_planned_in_place(torch, monkeypatch, bad):
    """k_unmask_inplace behind k_plan: the payload tiles and the finalize fold (tile_base +
    blockIdx.x < ceil(n / BLOCK)) across pieces; the valid batch also at N = tiles - 1 and tiles"""
    wire, offs, n = _table_batch(bad)

    def run(engines, _):
        ref = _batch_both(torch, engines, wire, n, offs=offs, mm=0)
        assert (ref["summary"]["status"] != 0) == bad
        assert ref["summary"]["consumed_bytes"] > 3 * 16384
        assert ref["summary"]["n_delivered"] == (9 if bad else n)
    if bad:
        for k in pieces():
            with _pair(monkeypatch, k) as engines:
                run(engines, k)
                _took(engines[0], k)
    else:
        _with_edges(monkeypatch, {}, run)


def test_planned_in_place_every_tile_shape(torch, monkeypatch):
    wire, offs, n = _table_batch(False)
    with _pair(monkeypatch, 3) as engines:
        for blk, vpt in TILE_SHAPES:
            for e in engines:
                e.set_tile(blk, vpt)
            _batch_both(torch, engines, wire, n, offs=offs, mm=0)
            _took(engines[0], 3, tiles=max(_ceil(wire.size, blk * vpt * 16), _ceil(n, blk)))


@pytest.mark.parametrize("n_piece", pieces())
def test_finalize_fold_past_the_wire(torch, monkeypatch, n_piece):
    """decode_planned extends the pass past the wire (n_ptiles < n_fin): the finalizing
    workgroups span pieces that lie wholly beyond the wire, at every tile shape.  All frames
    delivered (the issue's case; the oracle delivers all 5 000), and the same frames with frame 70
    failing: in a batch without a failure the fold rewrites no status, so a finalizing workgroup
    that never ran would go unnoticed"""
    batches = []
    for bad_at in (None, 70):
        wire, offs, n = _zero_batch(bad_at)
        ref = _oracle.decode_batch(wire.copy(), n, offsets=offs, wire_len=wire.size, max_message_size=0)
        assert ref["summary"]["n_delivered"] == (n if bad_at is None else bad_at)
        assert (ref["summary"]["status"] != 0) == (bad_at is not None)
        # (the failing batch: a status only a finalizing workgroup writes, in the last block too)
        assert bad_at is None or (ref["status"][bad_at + 1:] != 0).all()
        batches.append((wire, offs, n))
    with _pair(monkeypatch, n_piece) as engines:
        for blk, vpt in TILE_SHAPES:
            for e in engines:
                e.set_tile(blk, vpt)
            for wire, offs, n in batches:
                _batch_both(torch, engines, wire, n, offs=offs, mm=0)
                wire_tiles, n_fin = _ceil(wire.size, blk * vpt * 16), _ceil(n, blk)
                assert n_fin > wire_tiles + n_piece  # (a whole piece beyond the wire)
                _took(engines[0], n_piece, tiles=n_fin)


@pytest.mark.parametrize("n_piece", pieces())
@pytest.mark.parametrize("mode", ["scatter", "gather"])
def test_compact_scatter_and_gather(torch, monkeypatch, mode, n_piece):
    """the same batches compact, with the wire-driven scatter (which folds the finalize too) and
    the arena-driven gather, and three 64 KiB frames for the gather's arena tiles"""
    with _pair(monkeypatch, n_piece, {"UVHTTP_WS_COMPACT": mode}) as engines:
        for name, (wire, offs, n) in (("valid", _table_batch(False)), ("failing", _table_batch(True)),
                                      ("zero", _zero_batch()), ("zero", _zero_batch(70)),
                                      ("big", _big_batch())):
            _batch_both(torch, engines, wire, n, compact=True, offs=offs, mm=0)
            # (no payload byte: the gather's pass over the empty arena is its smallest, 4 workgroups)
            _took(engines[0], n_piece, least=4 if name == "zero" and mode == "gather" else 5)


def test_compact_edges(torch, monkeypatch):
    wire, offs, n = _table_batch(False)
    for mode in ("scatter", "gather"):
        _with_edges(monkeypatch, {"UVHTTP_WS_COMPACT": mode},
                    lambda engines, _: _batch_both(torch, engines, wire, n, compact=True, offs=offs, mm=0))


# ---- stride batches: k_unmask_stride (fused in place, speculative compact) -------------------------

N_STRIDE, STRIDE, ODD_AT = 640, 264, 500   # 10.3 tiles of 16 KiB; frame 500 lies in tile 8


def _stride_batch(odd=None):
    """640 frames of 256 payload bytes in 264-byte slots, fragmented messages; odd: frame 500
    with a reserved bit ("rsv": it fails, and everything the pass unmasked from it on is restored)
    or delivered at another length in the same slot ("length": 250 bytes behind a 64-bit length
    field, which breaks the compact speculation)"""
    rng = random.Random(f"stride-{odd}")
    frames, open_msg = [], False
    for i in range(N_STRIDE):
        op, fin = (0 if open_msg else rng.choice([1, 2])), rng.random() > 0.4
        if i == ODD_AT and odd == "length":
            f = _frame(op, fin, rng.randbytes(250), rng.randbytes(4), len_form=64)
        else:
            f = _frame(op, fin, rng.randbytes(256), rng.randbytes(4), rsv=2 if i == ODD_AT and odd else 0)
        assert len(f) == STRIDE
        frames.append(f)
        open_msg = not fin
    return np.frombuffer(b"".join(frames), np.uint8).copy()


@pytest.mark.parametrize("n_piece", pieces())
@pytest.mark.parametrize("form", ["emit2", "emit1", "emit0", "summary", "tile128x2"])
def test_fused_stride_pass(torch, monkeypatch, form, n_piece):
    """k_unmask_stride in place: descriptors through k_desc_emit from the records (2) or the info
    bytes (1), through k_plan + k_fixup (0), summary-only, and a non-default tile shape; clean,
    and with a failing frame in tile 8 — past the first piece, so k_fixup / k_sum_tail restore
    bytes a later piece wrote"""
    env = {"UVHTTP_WS_DESC_EMIT": form[4]} if form.startswith("emit") else {}
    with _pair(monkeypatch, n_piece, env) as engines:
        tile = 16384
        if form == "tile128x2":
            tile = 128 * 2 * 16
            for e in engines:
                e.set_tile(128, 2)
        for odd in (None, "rsv"):
            wire = _stride_batch(odd)
            assert ODD_AT * STRIDE // tile >= n_piece
            if form == "summary":
                ref = SO._check(torch, engines, wire, N_STRIDE, STRIDE)
            else:
                ref = _batch_both(torch, engines, wire, N_STRIDE, stride=STRIDE, mm=0)
            assert ref["summary"]["n_delivered"] == (ODD_AT if odd else N_STRIDE)
            _took(engines[0], n_piece, tiles=_ceil(wire.size, tile))


def test_fused_stride_edges(torch, monkeypatch):
    wire = _stride_batch("rsv")
    _with_edges(monkeypatch, {}, lambda engines, _: _batch_both(torch, engines, wire, N_STRIDE,
                                                                 stride=STRIDE, mm=0))


@pytest.mark.parametrize("n_piece", pieces())
@pytest.mark.parametrize("form", ["desc", "summary", "emit0"])
def test_speculative_compact_stride(torch, monkeypatch, form, n_piece):
    """decode_spec: the compact stride pass with descriptors, summary-only and with
    UVHTTP_WS_DESC_EMIT=0; clean, and with frame 500 delivered at another length, so that
    k_spec_fix redoes the batch with the s_tiles of the whole pass"""
    env = {"UVHTTP_WS_DESC_EMIT": "0"} if form == "emit0" else {}
    with _pair(monkeypatch, n_piece, env, stamps=True) as engines:
        for odd in (None, "length"):
            wire = _stride_batch(odd)
            if form == "summary":
                ref = TS._check(torch, engines, wire, N_STRIDE, STRIDE, fast=odd is None)
            else:
                ref = _batch_both(torch, engines, wire, N_STRIDE, compact=True, stride=STRIDE, mm=0)
            assert ref["summary"]["n_delivered"] == N_STRIDE and ref["summary"]["status"] == 0
            assert ref["summary"]["arena_bytes"] == N_STRIDE * 256 - (6 if odd else 0)
            _took(engines[0], n_piece, tiles=_ceil(wire.size, 16384))


def test_speculative_compact_edges(torch, monkeypatch):
    wire = _stride_batch("length")
    _with_edges(monkeypatch, {}, lambda engines, _: _batch_both(torch, engines, wire, N_STRIDE, compact=True,
                                                                 stride=STRIDE, mm=0))


# ---- streams: k_sspec_pass, and the walk path's k_unmask_inplace -------------------------------------

@pytest.mark.parametrize("n_piece", pieces())
@pytest.mark.parametrize("case", ["A", "C", "A-walk", "A-other_length"])
def test_streams(torch, monkeypatch, case, n_piece):
    """test_gpu_epoch_wrap's shapes A and C (10 tiles of 16 KiB) through the speculative pass,
    A through the walk path's payload pass, A with a frame of another length in connection 10
    (the pass breaks the speculation; its unmask is undone); results, descriptors and wire
    against the oracle's decode_streams and the unsplit engine"""
    shape = case[0]
    W._oracle_delivers_all(shape)
    env = {"UVHTTP_WS_STREAM_SPEC": "0"} if case == "A-walk" else {}
    broken = ("other_length", 10) if case == "A-other_length" else None
    wire, st, cap = W._streams(random.Random("pieces-" + case), shape, broken)
    with _pair(monkeypatch, n_piece, env, stamps=True) as engines:
        a = _run(torch, engines, wire, st, max_frames=cap, spec_expected=case in ("A", "C"))
        assert ("spec_plan" in a["kinds"]) == (case != "A-walk"), a["kinds"]
        _took(engines[0], n_piece, tiles=None if case == "A-walk" else _ceil(wire.size, 16384))


def test_streams_edges(torch, monkeypatch):
    wire, st, cap = W._streams(random.Random("pieces-edges"), "A")
    _with_edges(monkeypatch, {}, lambda engines, _: _run(torch, engines, wire, st, max_frames=cap,
                                                         spec_expected=True), stamps=True)
    _with_edges(monkeypatch, {"UVHTTP_WS_STREAM_SPEC": "0"},
                lambda engines, _: _run(torch, engines, wire, st, max_frames=cap), stamps=True)


# ---- the send side: kb_emit ---------------------------------------------------------------------------

def _build_both(torch, engines, src, frames, **kw):
    outs = [TB._build(torch, e, src, frames, **kw) for e in engines]
    (exp, total, out, off), (_, _, out1, off1) = outs
    assert np.array_equal(out, out1) and np.array_equal(off, off1)
    return exp, total, out, off


@pytest.mark.parametrize("n_piece", pieces())
@pytest.mark.parametrize("seed", range(3))
def test_send_side_tiles(torch, monkeypatch, seed, n_piece):
    """test_gpu_build.test_build_matches_oracle's seeds 0-2 at cap_extra = 64 through the
    output-tile kernels (UVHTTP_WS_BUILD_FRAMES=0)"""
    rng = random.Random(seed)
    src = np.frombuffer(rng.randbytes(300000), np.uint8).copy()
    sizes = [[0, 1, 5, 125, 126, 127, 200], [1000, 4095, 65535, 65536, 70000], [0, 3, 300, 65536]][seed % 3]
    frames = TB._rand_frames(rng, src.size, rng.choice([1, 17, 300, 2000]), sizes)
    with _pair(monkeypatch, n_piece, {"UVHTTP_WS_BUILD_FRAMES": "0"}) as engines:
        exp, total, out, off = _build_both(torch, engines, src, frames, cap_extra=64)
        assert int(off[len(frames)]) == total
        assert np.array_equal(off[:len(frames)], np.cumsum([0] + [len(b) for b in exp[:-1]]))
        assert out[:total].tobytes() == b"".join(exp)
        assert not out[total:].any()
        _took(engines[0], n_piece)


def test_send_side_edges_and_capacity(torch, monkeypatch):
    """N = tiles - 1 and tiles on a small batch; and a capacity one byte short of 40 frames of up
    to 20 000 bytes: every piece of the pass runs and none writes anything"""
    rng = random.Random("send-edges")
    src = np.frombuffer(rng.randbytes(200000), np.uint8).copy()
    frames = TB._rand_frames(rng, src.size, 40, [10, 100, 1000, 20000])
    env = {"UVHTTP_WS_BUILD_FRAMES": "0"}

    def good(engines, _):
        exp, total, out, off = _build_both(torch, engines, src, frames)
        assert int(off[40]) == total and out[:total].tobytes() == b"".join(exp) and not out[total:].any()
    _with_edges(monkeypatch, env, good)
    need = sum(len(_oracle.build_frame(src[f["payload_off"]:f["payload_off"] + f["payload_len"]].tobytes(),
                                       int(f["opcode"]), int(f["mask"]), int(f["fin"]))[1]) for f in frames)
    for k in pieces():
        with _pair(monkeypatch, k, env) as engines:
            exp, total, out, off = _build_both(torch, engines, src, frames, cap=need - 1)
            assert int(off[40]) == total == need
            assert not out.any()  # all-or-nothing, in every piece
            _took(engines[0], k)


# ---- the plain unmask: k_apply_mask ---------------------------------------------------------------------

@pytest.mark.parametrize("n_piece", pieces() + [4, 5])
@pytest.mark.parametrize("off", [0, 1, 3, 15])
def test_plain_unmask(torch, monkeypatch, off, n_piece):
    """tile 0 does the unaligned head and tail bytes, whichever piece the tail's vectors lie in:
    a head of (16 - off) % 16 bytes, 5 full tiles of 64 vectors and tails of 1 .. 15 bytes, with
    guard bytes on both sides, against the oracle's mask (4 = tiles - 1 and 5 = tiles)"""
    rng = np.random.default_rng(off)
    head = (16 - off) % 16
    with _pair(monkeypatch, n_piece) as engines:
        for tail in (1, 2, 7, 15):
            n = head + 5 * 64 * 16 + tail
            host = rng.integers(0, 256, off + n, dtype=np.uint8)
            key = bytes(rng.integers(0, 256, 4, dtype=np.uint8))
            exp = host.copy()
            exp[off:] = np.frombuffer(bytes(_oracle.apply_mask(bytearray(host[off:].tobytes()), key)), np.uint8)
            got = []
            for e in engines:
                d = _to_dev(torch, host)
                e.apply_mask(d, key, length=n, offset=off)
                torch.cuda.synchronize()
                got.append(d.cpu().numpy())
                assert np.array_equal(got[-1][:off + n], exp), np.nonzero(got[-1][:off + n] != exp)[0][:8]
                assert (got[-1][off + n:] == 0xA5).all() and np.array_equal(got[-1][:off], host[:off])
            assert np.array_equal(got[0], got[1])
            p, pc, t = engines[0].grid_pieces()
            assert (p, pc, t) == (1, _ceil(5, n_piece), 5)


# ---- UTF-8: k_utf8_tiles, k_fu_tiles --------------------------------------------------------------------

CH4 = "\U0001F600".encode()
EDGE = 16384


def _arena_text(bad):
    """six TEXT messages of 15 000 bytes in fragments of 5 000: in the arena a 4-byte character
    lies across every 16 KiB boundary (1, 2, 3, 1, 2 bytes before it); bad: a stray continuation
    byte in the last tile"""
    text = bytearray(b"a" * 90000)
    for k in range(1, 6):
        at = EDGE * k - (1 + (k - 1) % 3)
        text[at:at + 4] = CH4
    if bad:
        text[5 * EDGE + 3000] = 0x80
    rng = random.Random("utf8-arena")
    frames = []
    for i in range(18):
        frames.append(T8.D.Frame(1 if i % 3 == 0 else 0, i % 3 == 2, bytes(text[i * 5000:(i + 1) * 5000]),
                                 key=rng.randbytes(4)))
    return frames


@pytest.mark.parametrize("n_piece", pieces())
def test_utf8_after_compact_decode(torch, monkeypatch, n_piece):
    """validate_utf8 over a compact decode's arena, against _utf8_ref: every 16 KiB tile edge
    (and so every piece edge at N = 1) cuts a 4-byte character of a message that spans it"""
    with _pair(monkeypatch, n_piece) as engines:
        for bad in (False, True):
            frames = _arena_text(bad)
            outs = [T8._decode_validate(torch, e, frames, False) for e in engines]
            assert outs[0] == outs[1]
            got, summ, s = outs[0]
            assert s["n_delivered"] == 18 and s["n_messages"] == 6
            assert [v for v, _ in got] == [R.VALID] * 5 + [R.INVALID if bad else R.VALID]
            _took(engines[0], n_piece, passes=2)  # (the compact decode's pass and k_utf8_tiles)


def _edge_fragments(bad):
    """one connection's TEXT message in six fragments; each of the first five ends on a 16 KiB
    wire edge with 1, 2, 3, 1, 2 bytes of a 4-byte character before the cut; bad: the last
    character's last byte is 41"""
    frames, pos, carry = [], 0, b""
    for k in range(1, 6):
        split = 1 + (k - 1) % 3
        ch = CH4[:3] + b"\x41" if bad and k == 5 else CH4
        plen = EDGE * k - pos - 8
        payload = carry + b"a" * (plen - len(carry) - split) + ch[:split]
        frames.append(FR.Fr(1 if k == 1 else 0, 0, payload))
        assert len(frames[-1].bytes) == plen + 8
        pos += plen + 8
        carry = ch[split:]
    frames.append(FR.Fr(0, 1, carry + b"a" * 100))
    return frames


@pytest.mark.parametrize("n_piece", pieces())
@pytest.mark.parametrize("api", ["streams", "inplace"])
def test_utf8_frames_across_tile_edges(torch, monkeypatch, api, n_piece):
    """validate_utf8_streams / _inplace after the decode, against _utf8_frames_ref: fragments
    that end on the 16 KiB tile edges inside a character, the invalid twin's bad byte in the
    last tile"""
    with _pair(monkeypatch, n_piece) as engines:
        for bad in (False, True):
            frames = _edge_fragments(bad)
            if api == "streams":
                outs = [TF.run_streams(torch, e, [frames])[:2] for e in engines]
                verdict = outs[0][0][0]
            else:
                outs = [TF.run_inplace(torch, e, frames) for e in engines]
                verdict = outs[0][0]
            assert outs[0] == outs[1]
            assert verdict["status"] == (R.INVALID if bad else R.VALID)
            assert verdict["first_invalid"] == (5 if bad else FR.NONE)
            _took(engines[0], n_piece, passes=2)  # (the decode's payload pass and k_fu_tiles)


def test_utf8_edges(torch, monkeypatch):
    """k_fu_tiles at N = tiles - 1 and tiles: validate_utf8_inplace alone on a decoded batch"""
    frames = _edge_fragments(True)
    wire = np.frombuffer(b"".join(f.bytes for f in frames), np.uint8).copy()
    offs = np.cumsum([0] + [len(f.bytes) for f in frames[:-1]]).astype(np.int64)
    want = FR.judge(frames)

    def run(engines, _):
        got = []
        for e in engines:
            dw = TF._dev(torch, wire)
            desc, summ = e.decode_inplace(dw, len(frames), offsets=torch.from_numpy(offs).to("cuda"),
                                          wire_len=wire.size, max_frame_size=FR.MF, max_message_size=FR.MM)
            torch.cuda.synchronize()
            if e is engines[0]:
                e.grid_pieces()  # (count the validation alone)
            v, sm = e.validate_utf8_inplace(dw, desc, len(frames), summ, flags=0, wire_len=wire.size)
            torch.cuda.synchronize()
            got.append((e.read_utf8_conn_verdicts(v, 1)[0], e.read_utf8_frames_summary(sm)))
            assert got[-1] == (want, FR.summary([want]))
        assert got[0] == got[1]
    _with_edges(monkeypatch, {}, run)


# ---- stamps ------------------------------------------------------------------------------------------------

def test_stamps_one_record_per_pass(torch, monkeypatch):
    """StampScope places the stamp words by tile_base + blockIdx.x: with stamps on at N = 3 the
    calls leave the same (call, kernel) records as on an engine without the knob — one record
    per kernel of a call, not one per piece — and every record ends no earlier than it begins
    (no assertion on the durations)"""
    table, offs, n = _table_batch(False)
    stride_wire = _stride_batch()
    swire, st, cap = W._streams(random.Random("pieces-stamps"), "A")
    rng = random.Random("pieces-stamps-send")
    src = np.frombuffer(rng.randbytes(200000), np.uint8).copy()
    frames = TB._rand_frames(rng, src.size, 40, [10, 100, 1000, 20000])
    env = {"UVHTTP_WS_BUILD_FRAMES": "0"}
    with _pair(monkeypatch, 3, env, stamps=True) as engines:
        recs = []
        for e in engines:
            e.read_stamps()
            ref, got = _run_both(torch, e, stride_wire.copy(), N_STRIDE, stride=STRIDE, mm=0)
            _compare(ref, got)
            ref, got = _run_both(torch, e, stride_wire.copy(), N_STRIDE, stride=STRIDE, mm=0, compact=True)
            _compare(ref, got, True)
            ref, got = _run_both(torch, e, table.copy(), n, offs=offs, mm=0)
            _compare(ref, got)
            d = torch.from_numpy(np.concatenate([swire, np.full(64, 0xA5, np.uint8)])).to("cuda")
            e.decode_streams(d, torch.from_numpy(st.view(np.uint8).copy()).to("cuda"), st.size, cap,
                             wire_len=swire.size)
            TB._build(torch, e, src, frames)
            torch.cuda.synchronize()
            recs.append(e.read_stamps())
        _took(engines[0], 3, passes=5)
        for r in recs:
            assert all(end >= begin for _, _, begin, end in r), r
        seq = [[(call - r[0][0], kern) for call, kern, _, _ in r] for r in recs]
        assert seq[0] == seq[1], seq
        assert len(set(seq[0])) == len(seq[0]), seq[0]          # no kernel of a call twice
        assert sorted({c for c, _ in seq[0]}) == list(range(5))
        assert sum(1 for _, k in seq[0] if k == "payload") == 5, seq[0]  # one payload record per call


# ---- one captured call ---------------------------------------------------------------------------------------

def test_captured_fused_stride(torch, monkeypatch):
    """the fused stride batch at N = 3 captured into a graph (its pieces are one serial chain on
    the call's stream) and replayed twice over other bytes, the second with the failing frame;
    scratch reserved and the call run uncaptured first"""
    t = torch
    with _pair(monkeypatch, 3) as (eng, whole):
        wl = N_STRIDE * STRIDE
        wire = t.full((wl + 64,), 0xA5, dtype=t.uint8, device="cuda")
        desc, summ = eng.alloc_outputs(N_STRIDE)
        s = t.cuda.Stream()
        eng.reserve(N_STRIDE, wl, 0)
        wire[:wl].copy_(t.from_numpy(_stride_batch()))
        with t.cuda.stream(s):
            eng.decode_inplace(wire, N_STRIDE, stride=STRIDE, wire_len=wl, max_message_size=0, desc=desc,
                               summary=summ, stream=s)
        s.synchronize()
        _took(eng, 3, tiles=_ceil(wl, 16384))
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=s):
            eng.decode_inplace(wire, N_STRIDE, stride=STRIDE, wire_len=wl, max_message_size=0, desc=desc,
                               summary=summ, stream=s)
        _took(eng, 3, tiles=_ceil(wl, 16384))  # (counted when captured)
        for odd in ("length", "rsv"):
            host = _stride_batch(odd)
            wire[:wl].copy_(t.from_numpy(host))
            t.cuda.synchronize()
            g.replay()
            t.cuda.synchronize()
            ref, unsplit = _run_both(t, whole, host.copy(), N_STRIDE, stride=STRIDE, mm=0)
            _compare(ref, unsplit)
            got = dict(summary=eng.read_summary(summ), desc=eng.read_desc(desc, N_STRIDE),
                       wire=wire[:wl].cpu().numpy())
            _compare(ref, got)
            _same(got, unsplit)
            assert (ref["summary"]["status"] != 0) == (odd == "rsv")
            assert (wire[wl:] == 0xA5).all()
        assert eng.grid_pieces() == (0, 0, 0)
        eng.sync()


# ---- the knob refuses what it cannot honour ----------------------------------------------------------------

@pytest.mark.parametrize("value", ["0", str((1 << 24) + 1), "-1", "three", "3x", ""])
def test_out_of_range_piece_fails_engine_creation(torch, monkeypatch, value):
    import uvhttp_amd as U
    monkeypatch.setenv(KNOB, value)
    with pytest.raises(U.GpuError, match=KNOB):
        U.GpuEngine(0)


def test_product_library_has_no_hook(torch):
    import uvhttp_amd as U
    e = U.GpuEngine(0, library=U.lib())
    try:
        with pytest.raises(U.GpuError, match="experiment build"):
            e.grid_pieces()
    finally:
        e.close()
