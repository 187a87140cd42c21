#!/usr/bin/env python3
"""Fail points on one MI355X (uvhttp_ws_gpu_fail_points_streams; not the BASELINE metric, bench.py
is untouched).

Workload: the C4-shaped stream batch of tools/bench_replies.py resident in HBM, 4 096 connections
x 256 masked frames of 256 payload bytes, 1 % of the frames PINGs, with 0 %, 1 % and 10 % of the
connections failing at a random frame: every other one through its UTF-8 verdict (the verdict
table is written directly, the pass reads nothing else of the text), the others through a CLOSE
frame with a 1-byte payload put in place of that frame.

Each call is bracketed by HIP events; a line reports the median, minimum and mean of the pass and,
from the same process and the same tables, of control_replies_streams (the same kind of descriptor
pass: `vs_replies` = fail points / replies), and of the echo and the relay (64 rooms) over the
original and over the rewritten tables (`echo_cut_vs_whole`, `relay_cut_vs_whole`: unchanged code,
so they should differ by the dropped frames only: `dropped_fraction`).  The pass's summary is
checked against the mix.

    python tools/bench_fail.py [--steps K] [--warmup W] [--mixes 0,0.01,0.1] [--scale S] [--out FILE]

One JSON line per mix on stdout (and appended to FILE), then nothing else.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_replies import PER, PLEN, timed  # noqa: E402

PINGS = 0.01


def build_wire(conns, fail_at, seed):
    """fail_at = {connection: frame} of the connections that get a 1-byte CLOSE there
    -> (wire uint8, per-connection begin / len, number of PINGs)"""
    rng = np.random.default_rng(seed)
    n = conns * PER
    is_close = np.zeros(n, bool)
    for s, f in fail_at.items():
        is_close[s * PER + f] = True
    is_ping = (rng.random(n) < PINGS) & ~is_close
    plen = np.where(is_close, 1, np.where(is_ping, rng.integers(0, 126, n), PLEN)).astype(np.int64)
    size = np.where(is_close | is_ping, 6 + plen, 8 + PLEN)  # 2-byte header (+ 2 length bytes) + 4 key bytes
    off = np.concatenate([[0], np.cumsum(size)])
    wire = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    o = off[:-1]
    wire[o] = np.where(is_close, 0x88, np.where(is_ping, 0x89, 0x82))
    wire[o + 1] = np.where(is_close | is_ping, 0x80 | plen, 0x80 | 126)
    d = o[~(is_ping | is_close)]
    wire[d + 2], wire[d + 3] = PLEN >> 8, PLEN & 0xFF
    begin = off[:-1:PER]
    return wire, begin, off[PER::PER] - begin, is_ping


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mixes", default="0,0.01,0.1")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 4 096 connections (smoke runs)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()

    import torch
    import uvhttp_amd as U
    t, dev = torch, "cuda:0"
    eng = U.GpuEngine(0)
    conns = max(1, int(4096 * args.scale))
    frames = conns * PER
    for mix in (float(x) for x in args.mixes.split(",")):
        rng = np.random.default_rng(0xFA11)
        failing = np.linspace(0, conns - 1, int(round(conns * mix))).astype(np.int64) if mix else np.zeros(0, np.int64)
        failing = np.unique(failing)
        at = rng.integers(0, PER, failing.size)
        by_close = {int(s): int(f) for k, (s, f) in enumerate(zip(failing, at)) if k & 1}
        by_utf8 = {int(s): int(f) for k, (s, f) in enumerate(zip(failing, at)) if not k & 1}
        wire, begin, length, is_ping = build_wire(conns, by_close, 0x5EED)
        wire_len = wire.size
        d_wire = t.zeros(wire_len + 64, dtype=t.uint8, device=dev)
        d_wire[:wire_len] = t.from_numpy(wire).to(dev)
        st = np.zeros(conns, dtype=U.STREAM_DT)
        st["begin"], st["len"] = begin, length
        st["recv_buffer_size"] = max(65536, int(length.max()))
        st["max_frame_size"], st["max_message_size"], st["is_server"] = 16 << 20, 64 << 20, 1
        d_st = t.from_numpy(st.view(np.uint8).copy()).to(dev)
        desc = t.empty(frames * 32, dtype=t.uint8, device=dev)
        res = t.zeros(conns * 64, dtype=t.uint8, device=dev)
        ver = np.zeros((conns, 4), np.uint32)   # first_invalid, n_text_frames, state, status
        ver[:, 0] = 0xFFFFFFFF
        for s, f in by_utf8.items():
            ver[s] = (s * PER + f, 0, 0, U.UTF8_INVALID)
        d_ver = t.from_numpy(ver.view(np.uint8).reshape(-1).copy()).to(dev)
        res2, ver2 = t.zeros_like(res), t.zeros_like(d_ver)
        fail = t.zeros(conns * 16, dtype=t.uint8, device=dev)
        fsum = t.zeros(32, dtype=t.uint8, device=dev)
        n_ping = int(is_ping.sum())
        max_replies, reply_cap = n_ping + conns, 131 * (n_ping + conns)
        r_out = t.zeros(reply_cap, dtype=t.uint8, device=dev)
        r_off = t.zeros(max_replies + 1, dtype=t.int64, device=dev)
        rconn, rsum = t.zeros(conns * 16, dtype=t.uint8, device=dev), t.zeros(32, dtype=t.uint8, device=dev)
        echo_cap = frames * (PLEN + 4)
        e_out = t.zeros(echo_cap, dtype=t.uint8, device=dev)
        e_off = t.zeros(frames + 1, dtype=t.int64, device=dev)
        o_off = t.zeros(conns + 1, dtype=t.int64, device=dev)
        econn, esum = t.zeros(conns * 32, dtype=t.uint8, device=dev), t.zeros(32, dtype=t.uint8, device=dev)
        runs = t.zeros(conns * 2, dtype=t.int32, device=dev)
        n_rooms = min(64, conns)
        d_room = t.from_numpy((np.arange(conns, dtype=np.uint32) % n_rooms).view(np.uint8).copy()).to(dev)
        rooms = t.zeros(n_rooms * 32, dtype=t.uint8, device=dev)

        eng.decode_streams(d_wire, d_st, conns, frames, desc=desc, results=res, wire_len=wire_len)
        t.cuda.synchronize()
        assert all(r.n_delivered == PER and r.status == 0 for r in eng.read_stream_results(res, conns))

        def fail_points():
            eng.fail_points_streams(d_wire, desc, frames, res, conns, d_ver, None, U.FAIL_CHECK_CLOSE, res2, ver2, fail,
                                    fsum, wire_len=wire_len)

        def replies():
            eng.control_replies_streams(d_wire, desc, frames, d_st, res, conns, max_replies, reply_cap, out=r_out,
                                        out_off=r_off, runs=runs, conn=rconn, summary=rsum, wire_len=wire_len)

        def echo(tab):
            return lambda: eng.echo_messages_streams(d_wire, desc, frames, d_st, tab, conns, frames, echo_cap, out=e_out,
                                                     out_off=e_off, runs=runs, open_off=o_off, conn=econn, summary=esum,
                                                     wire_len=wire_len)

        def relay(tab):
            return lambda: eng.relay_messages_streams(d_wire, desc, frames, d_st, tab, conns, d_room, n_rooms, frames,
                                                      echo_cap, out=e_out, out_off=e_off, rooms=rooms, open_off=o_off,
                                                      conn=econn, summary=esum, wire_len=wire_len)

        stat = {}
        for name, fn in (("fail_points", fail_points), ("control_replies", replies), ("echo_whole", echo(res)),
                         ("echo_cut", echo(res2)), ("relay_whole", relay(res)), ("relay_cut", relay(res2))):
            med, lo, mean = timed(t, fn, args.steps, args.warmup)
            stat[name] = {"ms": round(med, 4), "min_ms": round(lo, 4), "mean_ms": round(mean, 4)}
            if name.startswith(("echo", "relay")):
                s = eng.read_echo_summary(esum) if name.startswith("echo") else eng.read_relay_summary(esum)
                assert s["status"] == U.ECHO_OK, s
                stat[name]["frames_out"] = s["n_echoes"] if name.startswith("echo") else s["n_frames"]
        dropped = sum(PER - f for f in by_close.values()) + sum(PER - f for f in by_utf8.values())
        s = eng.read_fail_summary(fsum)
        assert s == {"n_dropped": dropped, "n_decode": 0, "n_utf8": len(by_utf8), "n_close_len": len(by_close),
                     "n_close_code": 0, "n_bad_range": 0, "first_failed": int(failing[0]) if failing.size else 0xFFFFFFFF}, s
        ms = stat["fail_points"]["ms"]
        line = {
            "metric": "fail points after decode_streams, ms per call (device-resident)",
            "value": ms, "unit": "ms", "n_gpus": 1, "higher_is_better": False,
            "steps": args.steps, "warmup": args.warmup, "failing_fraction": mix,
            "config": {"connections": conns, "frames": frames, "payload_bytes": PLEN, "wire_bytes": int(wire_len),
                       "pings": n_ping, "failed_by_utf8": len(by_utf8), "failed_by_close": len(by_close),
                       "dropped_frames": dropped},
            **stat,
            "ns_per_frame": round(ms * 1e6 / frames, 3),
            "vs_replies": round(ms / stat["control_replies"]["ms"], 3),
            "echo_cut_vs_whole": round(stat["echo_cut"]["ms"] / stat["echo_whole"]["ms"], 3),
            "relay_cut_vs_whole": round(stat["relay_cut"]["ms"] / stat["relay_whole"]["ms"], 3),
            "dropped_fraction": round(dropped / frames, 4),
        }
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
