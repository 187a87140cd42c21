#!/usr/bin/env python3
"""Control replies on one MI355X (uvhttp_ws_gpu_control_replies_streams; not the BASELINE
metric, bench.py is untouched).

Workload: a C4-shaped stream batch resident in HBM, 4 096 connections x 256 masked frames of
256 payload bytes, with 0 %, 1 % and 10 % of the frames replaced by PINGs of 0-125 payload bytes
(every connection a server connection, every PING answered).  The wire is built on the host with
numpy (random keys and payloads) and uploaded once per mix.

Each call is bracketed by HIP events; a line reports the median, minimum and mean of the replies
call and, from the same process and the same wire, of the decode_streams step it follows:
`vs_decode` = replies / decode.  The reply count and bytes are checked against the mix.

    python tools/bench_replies.py [--steps K] [--warmup W] [--mixes 0,0.01,0.1] [--scale S] [--out FILE]

One JSON line per mix on stdout (and appended to FILE), then nothing else.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PER, PLEN = 256, 256  # frames per connection, payload bytes of a data frame


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


def build_wire(conns, mix, seed):
    """-> (wire uint8, per-connection begin / len, PING payload lengths)"""
    rng = np.random.default_rng(seed)
    n = conns * PER
    is_ping = rng.random(n) < mix
    plen = np.where(is_ping, rng.integers(0, 126, n), PLEN).astype(np.int64)
    size = np.where(is_ping, 6 + plen, 8 + PLEN)  # 2-byte header (+ 2 length bytes) + 4 key bytes
    off = np.concatenate([[0], np.cumsum(size)])
    wire = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    o = off[:-1]
    wire[o] = np.where(is_ping, 0x89, 0x82)
    wire[o + 1] = np.where(is_ping, 0x80 | plen, 0x80 | 126)
    d = o[~is_ping]
    wire[d + 2], wire[d + 3] = PLEN >> 8, PLEN & 0xFF
    begin = off[:-1:PER]
    length = off[PER::PER] - begin
    return wire, begin, length, plen[is_ping]


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
        wire, begin, length, pings = build_wire(conns, mix, 0x5EED)
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
        max_replies = max(1, pings.size)
        out_cap = max(16, int((2 + pings).sum()))
        out = t.zeros(out_cap, dtype=t.uint8, device=dev)
        off = t.zeros(max_replies + 1, dtype=t.int64, device=dev)
        rconn = t.zeros(conns * 16, dtype=t.uint8, device=dev)
        rsum = t.zeros(32, dtype=t.uint8, device=dev)
        runs = t.zeros(conns * 2, dtype=t.int32, device=dev)

        def decode():
            eng.decode_streams(d_wire, d_st, conns, frames, desc=desc, results=res, wire_len=wire_len)

        def replies():
            eng.control_replies_streams(d_wire, desc, frames, d_st, res, conns, max_replies, out_cap, out=out,
                                        out_off=off, runs=runs, conn=rconn, summary=rsum, wire_len=wire_len)

        d_med, d_lo, d_mean = timed(t, decode, args.steps, args.warmup)
        assert all(r.n_delivered == PER and r.status == 0 for r in eng.read_stream_results(res, conns))
        med, lo, mean = timed(t, replies, args.steps, args.warmup)
        s = eng.read_reply_summary(rsum)
        assert s == {"out_bytes": int((2 + pings).sum()), "n_replies": int(pings.size), "n_closed_conns": 0,
                     "status": U.REPLY_OK}, s
        line = {
            "metric": "control replies after decode_streams, ms per call (device-resident)",
            "value": round(med, 4), "unit": "ms", "n_gpus": 1, "higher_is_better": False,
            "steps": args.steps, "warmup": args.warmup, "ping_fraction": mix,
            "config": {"connections": conns, "frames": frames, "payload_bytes": PLEN, "wire_bytes": int(wire_len),
                       "replies": int(pings.size), "reply_bytes": int((2 + pings).sum())},
            "ms": round(med, 4), "min_ms": round(lo, 4), "mean_ms": round(mean, 4),
            "ns_per_frame": round(med * 1e6 / frames, 3),
            "same_run_decode": {"decode_streams": {"ms": round(d_med, 4), "min_ms": round(d_lo, 4),
                                                   "mean_ms": round(d_mean, 4)}},
            "vs_decode": round(med / d_med, 3),
        }
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del d_wire, desc, out, off
        t.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
