#!/usr/bin/env python3
"""Echo of data messages on one MI355X (uvhttp_ws_gpu_echo_messages_streams; not the BASELINE
metric, bench.py is untouched).

Shapes, all resident in HBM, every connection a server connection fed masked client frames:
  c3        4 096 connections x 16 single-frame messages of 64 KiB (65 536 messages, 4 GiB)
  c4        4 096 connections x 256 single-frame messages of 256 bytes
  c4_frag4  the c4 shape with every message in 4 fragments of 64 bytes
  c4_carry  the c4 shape with 1 % of the connections carrying a 256-byte message in, completed
            by their first frame
One connection's bytes are built on the host and repeated on the device (the payload bytes do
not matter to any of the three calls).

Three calls are timed in one process, alternating, each bracketed by HIP events: the echo call,
the decode_streams it follows over the same wire, and — for the unfragmented shapes — build_frames
over the same messages from a host-made descriptor table; for those shapes the two outputs are
compared byte for byte.  A line reports the medians, `vs_decode` = echo / decode and `vs_build` =
echo / build_frames.

    python tools/bench_echo.py [--steps K] [--warmup W] [--shapes c3,c4,c4_frag4,c4_carry] [--scale S] [--out FILE]

One JSON line per shape on stdout (and appended to FILE), then nothing else.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {  # messages per connection, message bytes, fragments per message, fraction carrying in
    "c3": (16, 65536, 1, 0.0),
    "c4": (256, 256, 1, 0.0),
    "c4_frag4": (256, 256, 4, 0.0),
    "c4_carry": (256, 256, 1, 0.01),
}
BUILD_DT = np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("key", "<u4"), ("opcode", "u1"),
                     ("fin", "u1"), ("mask", "u1"), ("r0", "u1"), ("r1", "<u8")])


def frame(op, fin, payload, key):
    n = len(payload)
    h = bytes([(0x80 if fin else 0) | op])
    h += bytes([0x80 | n]) if n <= 125 else bytes([0x80 | 126]) + n.to_bytes(2, "big") if n <= 65535 \
        else bytes([0x80 | 127]) + n.to_bytes(8, "big")
    return h + key + payload


def connection_bytes(per, mlen, frags, seed):
    rng = np.random.default_rng(seed)
    out = bytearray()
    flen = mlen // frags
    for _ in range(per):
        for k in range(frags):
            out += frame(2 if k == 0 else 0, k == frags - 1, rng.integers(0, 256, flen, dtype=np.uint8).tobytes(),
                         rng.integers(0, 256, 4, dtype=np.uint8).tobytes())
    return np.frombuffer(bytes(out), np.uint8)


def header_bytes(n):
    return 2 if n <= 125 else 4 if n <= 65535 else 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="c3,c4,c4_frag4,c4_carry")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 4 096 connections (smoke runs)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()

    import torch
    import uvhttp_amd as U
    t, dev = torch, "cuda:0"
    eng = U.GpuEngine(0)
    conns = max(1, int(4096 * args.scale))
    for name in args.shapes.split(","):
        per, mlen, frags, carry_frac = SHAPES[name]
        one = connection_bytes(per, mlen, frags, 0x5EED)
        clen, frames = one.size, conns * per * frags
        wire_len = clen * conns
        d_wire = t.zeros(wire_len + 64, dtype=t.uint8, device=dev)
        d_wire[:wire_len] = t.from_numpy(one.copy()).to(dev).repeat(conns)
        st = np.zeros(conns, dtype=U.STREAM_DT)
        st["begin"], st["len"] = np.arange(conns, dtype=np.uint64) * clen, clen
        st["recv_buffer_size"] = max(65536, clen)
        st["max_frame_size"], st["max_message_size"], st["is_server"] = 16 << 20, 64 << 20, 1
        carrying = np.zeros(conns, bool)
        if carry_frac:
            carrying[:: int(round(1 / carry_frac))] = True
            st["pending_bytes"][carrying], st["pending_opcode"][carrying] = mlen, 2
            # a carrying connection's first frame is the CONTINUATION that completes the message
            d_wire[t.from_numpy(st["begin"][carrying].astype(np.int64)).to(dev)] = 0x80
        n_carry = int(carrying.sum())
        d_carry = t.zeros(max(16, n_carry * mlen), dtype=t.uint8, device=dev)
        d_coff = t.from_numpy(np.concatenate([[0], np.cumsum(carrying * mlen)]).astype(np.int64)).to(dev)
        d_st = t.from_numpy(st.view(np.uint8).copy()).to(dev)
        desc = t.empty(frames * 32, dtype=t.uint8, device=dev)
        res = t.zeros(conns * 64, dtype=t.uint8, device=dev)
        msgs = conns * per
        want_bytes = msgs * (header_bytes(mlen) + mlen) + n_carry * (header_bytes(2 * mlen) - header_bytes(mlen) + mlen)
        out = t.zeros(want_bytes + 64, dtype=t.uint8, device=dev)
        off = t.zeros(msgs + 1, dtype=t.int64, device=dev)
        ooff = t.zeros(conns + 1, dtype=t.int64, device=dev)
        opn = t.zeros(16, dtype=t.uint8, device=dev)
        econn = t.zeros(conns * 32, dtype=t.uint8, device=dev)
        esum = t.zeros(32, dtype=t.uint8, device=dev)
        runs = t.zeros(conns * 2, dtype=t.int32, device=dev)

        def decode():
            eng.decode_streams(d_wire, d_st, conns, frames, desc=desc, results=res, wire_len=wire_len)

        def echo():
            eng.echo_messages_streams(d_wire, desc, frames, d_st, res, conns, msgs, want_bytes, carry=d_carry,
                                      carry_len=n_carry * mlen, carry_off=d_coff, out=out, out_off=off, runs=runs,
                                      open=opn, open_cap=16, open_off=ooff, conn=econn, summary=esum, wire_len=wire_len)

        decode()
        t.cuda.synchronize()
        assert all(r.n_delivered == per * frags and r.status == 0 for r in eng.read_stream_results(res, conns))
        calls = {"decode_streams": decode, "echo_messages": echo}
        if frags == 1 and not n_carry:
            hd = eng.read_desc(desc, frames)
            table = np.zeros(frames, BUILD_DT)
            table["payload_off"], table["payload_len"], table["opcode"], table["fin"] = hd["payload_off"], hd["payload_len"], 2, 1
            d_table = t.from_numpy(table.view(np.uint8).copy()).to(dev)
            out2 = t.zeros(want_bytes + 64, dtype=t.uint8, device=dev)
            off2 = t.zeros(frames + 1, dtype=t.int64, device=dev)
            calls["build_frames"] = lambda: eng.build_frames(d_wire[:wire_len], d_table, frames, out2[:want_bytes], out_off=off2)

        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        t.cuda.synchronize()
        ev = {k: [(t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
              for k in calls}
        for i in range(args.steps):
            for k, fn in calls.items():
                ev[k][i][0].record()
                fn()
                ev[k][i][1].record()
        t.cuda.synchronize()
        ms = {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
        stat = {k: {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "mean_ms": round(sum(v) / len(v), 4)}
                for k, v in ms.items()}
        s = eng.read_echo_summary(esum)
        assert s == {"out_bytes": want_bytes, "open_bytes": 0, "n_echoes": msgs, "status": U.ECHO_OK}, s
        if "build_frames" in calls:
            assert t.equal(off, off2) and t.equal(out[:want_bytes], out2[:want_bytes]), "echo != build_frames"
        med = stat["echo_messages"]["ms"]
        payload = msgs * mlen + n_carry * mlen
        line = {
            "metric": "echo of data messages after decode_streams, ms per call (device-resident)",
            "value": med, "unit": "ms", "n_gpus": 1, "higher_is_better": False,
            "steps": args.steps, "warmup": args.warmup, "shape": name,
            "config": {"connections": conns, "frames": frames, "messages": msgs, "message_bytes": mlen,
                       "fragments_per_message": frags, "carrying_connections": n_carry, "wire_bytes": int(wire_len),
                       "echo_bytes": int(want_bytes)},
            **stat["echo_messages"],
            "ns_per_frame": round(med * 1e6 / frames, 3),
            "gib_per_s_moved": round((payload + want_bytes) / (med * 1e-3) / 2**30, 1),
            "same_run": {k: v for k, v in stat.items() if k != "echo_messages"},
            "vs_decode": round(med / stat["decode_streams"]["ms"], 3),
            "vs_build": round(med / stat["build_frames"]["ms"], 3) if "build_frames" in stat else None,
        }
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del d_wire, desc, out, off
        if "build_frames" in calls:
            del out2, off2, d_table
        calls.clear()
        t.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
