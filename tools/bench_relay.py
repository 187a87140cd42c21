#!/usr/bin/env python3
"""Relay of data messages to the members of their rooms on one MI355X
(uvhttp_ws_gpu_relay_messages_streams; not the BASELINE metric, bench.py is untouched).

The shapes are tools/bench_echo.py's c3 (4 096 connections x 16 messages of 64 KiB) and c4
(4 096 x 256 messages of 256 bytes), every connection a server connection, so the relay moves
exactly the bytes the echo moves; every connection is also a receiver.  Three room maps:
  one     every connection in room 0                     (one radix pass)
  mod64   room = s % 64                                  (one radix pass)
  own     room = s, n_rooms = the connections            (two radix passes); the relay's d_out,
          d_out_off, d_open_off and per-connection results are asserted equal to the echo's
The relay call and the same-run echo_messages_streams over the same decoded wire alternate, each
bracketed by HIP events.

    python tools/bench_relay.py [--steps K] [--warmup W] [--shapes c3,c4] [--maps one,mod64,own]
                                [--scale S] [--out FILE]

One JSON line per shape and map on stdout (and appended to FILE), then nothing else.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_echo import SHAPES, connection_bytes, header_bytes  # noqa: E402


def median_ms(t, calls, steps, warmup):
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t.cuda.synchronize()
    ev = {k: [(t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)) for _ in range(steps)] for k in calls}
    for i in range(steps):
        for k, fn in calls.items():
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    t.cuda.synchronize()
    ms = {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
    return {k: {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "mean_ms": round(sum(v) / len(v), 4)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="c3,c4")
    ap.add_argument("--maps", default="one,mod64,own")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 4 096 connections (smoke runs)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()

    import torch
    import uvhttp_amd as U
    t, dev = torch, "cuda:0"
    eng = U.GpuEngine(0)
    conns = max(1, int(4096 * args.scale))
    for name in args.shapes.split(","):
        per, mlen, frags, _ = SHAPES[name]
        one = connection_bytes(per, mlen, frags, 0x5EED)
        clen, frames = one.size, conns * per * frags
        wire_len = clen * conns
        d_wire = t.zeros(wire_len + 64, dtype=t.uint8, device=dev)
        d_wire[:wire_len] = t.from_numpy(one.copy()).to(dev).repeat(conns)
        st = np.zeros(conns, dtype=U.STREAM_DT)
        st["begin"], st["len"] = np.arange(conns, dtype=np.uint64) * clen, clen
        st["recv_buffer_size"] = max(65536, clen)
        st["max_frame_size"], st["max_message_size"], st["is_server"] = 16 << 20, 64 << 20, 1
        d_st = t.from_numpy(st.view(np.uint8).copy()).to(dev)
        desc = t.empty(frames * 32, dtype=t.uint8, device=dev)
        res = t.zeros(conns * 64, dtype=t.uint8, device=dev)
        msgs = conns * per
        want_bytes = msgs * (header_bytes(mlen) + mlen)

        def outputs():
            return dict(out=t.zeros(want_bytes + 64, dtype=t.uint8, device=dev),
                        out_off=t.zeros(msgs + 1, dtype=t.int64, device=dev),
                        open_off=t.zeros(conns + 1, dtype=t.int64, device=dev),
                        open=t.zeros(16, dtype=t.uint8, device=dev), open_cap=16,
                        conn=t.zeros(conns * 32, dtype=t.uint8, device=dev),
                        summary=t.zeros(32, dtype=t.uint8, device=dev))
        eo, ro = outputs(), outputs()
        runs = t.zeros(conns * 2, dtype=t.int32, device=dev)
        sends = t.zeros(conns * 2, dtype=t.int32, device=dev)
        eng.decode_streams(d_wire, d_st, conns, frames, desc=desc, results=res, wire_len=wire_len)
        t.cuda.synchronize()
        assert all(r.n_delivered == per * frags and r.status == 0 for r in eng.read_stream_results(res, conns))

        def echo():
            eng.echo_messages_streams(d_wire, desc, frames, d_st, res, conns, msgs, want_bytes, runs=runs,
                                      wire_len=wire_len, **eo)

        for room_map in args.maps.split(","):
            room = {"one": np.zeros(conns, np.uint32), "mod64": np.arange(conns, dtype=np.uint32) % 64,
                    "own": np.arange(conns, dtype=np.uint32)}[room_map]
            n_rooms = int(room.max()) + 1
            d_room = t.from_numpy(room.view(np.int32).copy()).to(dev)
            rooms = t.zeros(n_rooms * 32, dtype=t.uint8, device=dev)

            def relay():
                eng.relay_messages_streams(d_wire, desc, frames, d_st, res, conns, d_room, n_rooms, msgs, want_bytes,
                                           rooms=rooms, recv_room=d_room, n_receivers=conns, sends=sends,
                                           wire_len=wire_len, **ro)

            stat = median_ms(t, {"echo_messages": echo, "relay_messages": relay}, args.steps, args.warmup)
            s = eng.read_relay_summary(ro["summary"])
            assert s == {"out_bytes": want_bytes, "open_bytes": 0, "n_frames": msgs, "status": U.ECHO_OK,
                         "n_bad_rooms": 0, "n_bad_receivers": 0}, s
            rr = eng.read_relay_rooms(rooms, n_rooms)
            assert sum(r["n_frames"] for r in rr) == msgs and rr[-1]["out_off"] + rr[-1]["out_len"] == want_bytes
            if room_map == "own":
                assert t.equal(ro["out_off"], eo["out_off"]) and t.equal(ro["out"][:want_bytes], eo["out"][:want_bytes])
                assert t.equal(ro["open_off"], eo["open_off"]) and t.equal(ro["conn"], eo["conn"]) and t.equal(sends, runs)
            else:  # the same frames in another order: the same byte sum
                assert int(ro["out"][:want_bytes].sum(dtype=t.int64)) == int(eo["out"][:want_bytes].sum(dtype=t.int64))
            med, emed = stat["relay_messages"]["ms"], stat["echo_messages"]["ms"]
            line = {
                "metric": "relay of data messages after decode_streams, ms per call (device-resident)",
                "value": med, "unit": "ms", "n_gpus": 1, "higher_is_better": False,
                "steps": args.steps, "warmup": args.warmup, "shape": name, "rooms": room_map,
                "config": {"connections": conns, "frames": frames, "messages": msgs, "message_bytes": mlen,
                           "n_rooms": n_rooms, "receivers": conns, "wire_bytes": int(wire_len),
                           "relay_bytes": int(want_bytes)},
                **stat["relay_messages"],
                "same_run": {"echo_messages": stat["echo_messages"]},
                "vs_echo": round(med / emed, 3), "over_echo_us": round((med - emed) * 1e3, 1),
            }
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
        del d_wire, desc, eo, ro
        t.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
