#!/usr/bin/env python3
"""UTF-8 validation throughput on one MI355X (uvhttp_ws_gpu_validate_utf8; not the BASELINE
metric, bench.py is untouched).

Workload: an arena of synthetic text resident in HBM, cut into equal messages, judged through
the generic form (a caller's table of complete TEXT messages).  Shapes: C3-sized messages
(64 KiB) and C4-sized messages (246 B), each with as many bytes as the compact bench line of
that config decodes (65 536 x 64 KiB = 4 GiB; 1 048 576 x 256 B = 256 MiB).  Contents: pure
ASCII, and a mix of 40 % ASCII and 20 % each of 2-, 3- and 4-byte characters (one message built
on the host, repeated on the device; every message is valid, which a check of the summary
confirms — an invalid message costs the same reads).  The text is written with torch; no frame
generator runs (its payload is random bytes).

Each call is bracketed by HIP events; a line reports the median call, GiB/s of text and the
fraction of the 8 TB/s HBM peak.  In the same process the tool times the compact decode of the
same byte count (the config's frames, generated on the device as bench.py does), so each
validation time has the decode step it would follow beside it: `vs_decode` = validate / decode.

    python tools/bench_utf8.py [--steps K] [--warmup W] [--shapes c3,c4] [--scale S]

--decode inplace | streams times the frame-level calls instead (uvhttp_ws_gpu_validate_utf8_inplace
after decode_inplace with descriptors; _streams after decode_streams, C4 only: 4 096 connections
x 256 frames).  The config's TEXT frames are generated on the device, decoded, and their
payloads overwritten with the text (every frame its own message; for C4 also every message cut
into 4 fragments, the mixed text's characters crossing the cuts).  `vs_decode` = validate / the
same-run decode step of the same wire; for unfragmented runs the compact form's validator over
the same payload ranges (generic form, the wire as its data) is timed beside it.

One JSON line per (shape, content[, fragments]), then nothing else on stdout.
"""
import argparse
import json
import os
import random
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GIB = float(1 << 30)
HBM_PEAK = 8e12

# name: (message bytes, frames of the bench config, payload bytes per frame, fragmented, max_message_size)
SHAPES = {
    "c3": (65536, 65536, 65536, False, 64 * 1024 * 1024),
    "c4": (246, 1048576, 256, True, 256 * 1024 * 1024),
}


def mixed_message(nbytes, seed=11):
    """nbytes of valid UTF-8: 40 % ASCII characters, 20 % each of 2-, 3- and 4-byte ones"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < nbytes:
        room = nbytes - len(out)
        r = rng.random()
        k = 1 if r < 0.4 else 2 if r < 0.6 else 3 if r < 0.8 else 4
        k = min(k, room)
        c = (rng.randrange(0x20, 0x7F) if k == 1 else rng.randrange(0x80, 0x800) if k == 2 else
             rng.randrange(0x800, 0xD800) if k == 3 else rng.randrange(0x10000, 0x110000))
        out += chr(c).encode("utf-8")
    assert len(out) == nbytes
    bytes(out).decode("utf-8")
    return bytes(out)


def timed(torch, fn, steps, warmup):
    """median / min / mean milliseconds of fn() between HIP events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0], sum(ms) / len(ms)


def frames_mode(args, t, U, eng, dev):
    """--decode inplace | streams"""
    for shape in args.shapes.split(","):
        _, frames, plen, _, mm = SHAPES[shape]
        if args.decode == "streams" and shape != "c4":
            continue
        per = 256  # frames per connection (streams)
        frames = max(per, int(frames * args.scale)) // per * per
        conns = frames // per if args.decode == "streams" else 1
        stride = U.gen_frame_stride(plen)
        hdr, wire_len = stride - plen, stride * frames
        wire = t.empty(wire_len + 64, dtype=t.uint8, device=dev)
        eng.gen_frames(wire, frames, plen, 0x5EED, opcode0=1, fragmented=False)
        rows = wire[:wire_len].view(frames, stride)
        desc, summ = eng.alloc_outputs(frames)
        verdict = t.zeros(conns * 16, dtype=t.uint8, device=dev)
        usum = t.zeros(16, dtype=t.uint8, device=dev)
        if args.decode == "streams":
            st = np.zeros(conns, dtype=U.STREAM_DT)
            st["begin"] = np.arange(conns, dtype=np.uint64) * per * stride
            st["len"] = per * stride
            st["recv_buffer_size"] = max(65536, per * stride)
            st["max_frame_size"], st["max_message_size"], st["is_server"] = 16 << 20, mm, 1
            d_st = t.from_numpy(st.view(np.uint8).copy()).to(dev)
            res = t.zeros(conns * 64, dtype=t.uint8, device=dev)
            decode_name = "decode_streams"

            def decode():
                eng.decode_streams(wire, d_st, conns, frames, desc=desc, results=res, wire_len=wire_len)

            def validate():
                eng.validate_utf8_streams(wire, desc, frames, d_st, res, conns, verdict=verdict, summary=usum,
                                          wire_len=wire_len)
        else:
            eng.reserve(frames, wire_len, 0)
            decode_name = "decode_inplace"

            def decode():
                eng.decode_inplace(wire, frames, stride=stride, max_message_size=mm, wire_len=wire_len,
                                   desc=desc, summary=summ)

            def validate():
                eng.validate_utf8_inplace(wire, desc, frames, summ, verdict=verdict, summary=usum, wire_len=wire_len)

        table = np.zeros(frames, dtype=[("arena_off", "<u8"), ("len", "<u8"), ("first_frame", "<u4"),
                                        ("last_frame", "<u4"), ("opcode", "<i4"), ("reserved", "<u4")])
        table["arena_off"] = np.arange(frames, dtype=np.uint64) * stride + hdr
        table["len"], table["opcode"] = plen, 1
        d_table = t.from_numpy(table.view(np.uint8).copy()).to(dev)
        cverdict = t.zeros(frames * 4, dtype=t.uint8, device=dev)
        csum = t.zeros(16, dtype=t.uint8, device=dev)
        for cut in ((1, 4) if shape == "c4" else (1,)):
            # byte 0 of every header: FIN | TEXT, or TEXT, CONT, CONT, FIN | CONT
            b0 = t.tensor([0x81] if cut == 1 else [0x01, 0x00, 0x00, 0x80], dtype=t.uint8, device=dev)
            rows[:, 0] = b0.repeat(frames // cut)
            d_med, d_lo, d_mean = timed(t, decode, args.steps, args.warmup)
            if args.decode == "streams":
                assert all(r.n_delivered == per and r.status == 0 for r in eng.read_stream_results(res, conns))
            else:
                assert eng.read_summary(summ)["n_delivered"] == frames
            dec = {"ms": round(d_med, 4), "min_ms": round(d_lo, 4), "mean_ms": round(d_mean, 4),
                   "payload_gibs": round(frames * plen / (d_med * 1e-3) / GIB, 1)}
            for content in ("ascii", "mixed"):
                if content == "ascii":
                    tmp = t.empty(frames * plen, dtype=t.uint8, device=dev).random_(0x20, 0x7F)
                    rows[:, hdr:] = tmp.view(frames, plen)
                    del tmp
                else:
                    one = t.from_numpy(np.frombuffer(mixed_message(plen * cut), np.uint8).copy()).to(dev)
                    rows.view(frames // cut, cut, stride)[:, :, hdr:] = one.view(1, cut, plen)
                med, lo, mean = timed(t, validate, args.steps, args.warmup)
                v = eng.read_utf8_conn_verdicts(verdict, conns)
                assert all(x["status"] == U.UTF8_VALID and x["first_invalid"] == 0xFFFFFFFF for x in v), v[:2]
                us = eng.read_utf8_frames_summary(usum)
                assert us == {"n_text_frames": frames, "n_invalid_conns": 0, "first_invalid_conn": 0xFFFFFFFF,
                              "n_open_conns": 0}, us
                nbytes = frames * plen
                line = {
                    "metric": "UTF-8 validation GiB/s of text (device-resident, after %s)" % decode_name,
                    "value": round(nbytes / (med * 1e-3) / GIB, 1), "unit": "GiB/s", "n_gpus": 1,
                    "higher_is_better": True, "steps": args.steps, "warmup": args.warmup,
                    "shape": shape, "decode": args.decode, "content": content, "fragments": cut,
                    "config": {"frames": frames, "payload_bytes": plen, "connections": conns, "text_bytes": nbytes},
                    "ms": round(med, 4), "min_ms": round(lo, 4), "mean_ms": round(mean, 4),
                    "hbm_fraction_of_8TBs": round(nbytes / (med * 1e-3) / HBM_PEAK, 3),
                    "same_run_decode": {decode_name: dec},
                    "vs_decode": round(med / d_med, 3),
                }
                if cut == 1:
                    c_med, c_lo, _ = timed(t, lambda: eng.validate_utf8(
                        wire[:wire_len], d_table, frames, n_msgs=frames, verdict=cverdict, summary=csum),
                        args.steps, args.warmup)
                    cs = eng.read_utf8_summary(csum)
                    assert cs["n_text"] == frames and cs["n_invalid"] == 0, cs
                    line["same_run_compact_form"] = {"ms": round(c_med, 4), "min_ms": round(c_lo, 4),
                                                     "gibs": round(nbytes / (c_med * 1e-3) / GIB, 1)}
                print(json.dumps(line), flush=True)
        del wire, rows, desc, d_table, cverdict
        t.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="c3,c4")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the config's frames (smoke runs)")
    ap.add_argument("--decode", choices=["compact", "inplace", "streams"], default="compact",
                    help="which decode the validation follows (compact: the generic form over an arena)")
    args = ap.parse_args()

    import torch
    import uvhttp_amd as U
    t, dev = torch, "cuda:0"
    eng = U.GpuEngine(0)
    if args.decode != "compact":
        frames_mode(args, t, U, eng, dev)
        eng.close()
        return
    for shape in args.shapes.split(","):
        mlen, frames, plen, frag, mm = SHAPES[shape]
        frames = max(1, int(frames * args.scale))
        total = frames * plen
        n = total // mlen
        nbytes = n * mlen

        # the compact decode step of the same byte count (bench.py --mode compact, this config)
        stride = U.gen_frame_stride(plen)
        wire = t.empty(stride * frames + 64, dtype=t.uint8, device=dev)
        eng.gen_frames(wire, frames, plen, 0x5EED, opcode0=2, fragmented=frag)
        arena = t.empty(total + 64, dtype=t.uint8, device=dev)
        msgs = t.empty(frames * 32, dtype=t.uint8, device=dev)
        desc, summ = eng.alloc_outputs(frames)
        eng.reserve(frames, stride * frames, total)
        decode = {}
        for name, kw in (("decode_compact", dict(desc=desc)), ("decode_compact_no_desc", dict(no_desc=True))):
            med, lo, mean = timed(t, lambda: eng.decode_compact(
                wire, frames, arena, stride=stride, max_message_size=mm, wire_len=stride * frames,
                msgs=msgs, summary=summ, **kw), args.steps, args.warmup)
            s = eng.read_summary(summ)
            assert s["n_delivered"] == frames and s["arena_bytes"] == total, s
            decode[name] = {"ms": round(med, 4), "min_ms": round(lo, 4), "mean_ms": round(mean, 4),
                            "payload_gibs": round(total / (med * 1e-3) / GIB, 1)}
        del wire, desc

        table = np.zeros(n, dtype=[("arena_off", "<u8"), ("len", "<u8"), ("first_frame", "<u4"),
                                   ("last_frame", "<u4"), ("opcode", "<i4"), ("reserved", "<u4")])
        table["arena_off"] = np.arange(n, dtype=np.uint64) * mlen
        table["len"], table["opcode"] = mlen, 1
        d_table = t.from_numpy(table.view(np.uint8).copy()).to(dev)
        verdict = t.zeros(n * 4, dtype=t.uint8, device=dev)
        usum = t.zeros(16, dtype=t.uint8, device=dev)
        text = arena[:nbytes]  # the decode's arena, reused for the text
        for content in ("ascii", "mixed"):
            if content == "ascii":
                text.random_(0x20, 0x7F)
            else:
                one = t.from_numpy(np.frombuffer(mixed_message(mlen), np.uint8).copy()).to(dev)
                text.view(n, mlen).copy_(one.unsqueeze(0).expand(n, mlen))
            med, lo, mean = timed(t, lambda: eng.validate_utf8(text, d_table, n, n_msgs=n, verdict=verdict,
                                                               summary=usum), args.steps, args.warmup)
            us = eng.read_utf8_summary(usum)
            assert us == {"n_text": n, "n_invalid": 0, "first_invalid": 0xFFFFFFFF, "open_verdict": 0}, us
            line = {
                "metric": "UTF-8 validation GiB/s of text (device-resident, generic form)",
                "value": round(nbytes / (med * 1e-3) / GIB, 1), "unit": "GiB/s", "n_gpus": 1,
                "higher_is_better": True, "steps": args.steps, "warmup": args.warmup,
                "shape": shape, "content": content,
                "config": {"messages": n, "message_bytes": mlen, "text_bytes": nbytes},
                "ms": round(med, 4), "min_ms": round(lo, 4), "mean_ms": round(mean, 4),
                "hbm_fraction_of_8TBs": round(nbytes / (med * 1e-3) / HBM_PEAK, 3),
                "same_run_decode": decode,
                "vs_decode": round(med / decode["decode_compact"]["ms"], 3),
                "vs_decode_no_desc": round(med / decode["decode_compact_no_desc"]["ms"], 3),
            }
            print(json.dumps(line), flush=True)
        del arena, text, msgs, d_table, verdict
        t.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
