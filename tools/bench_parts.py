#!/usr/bin/env python3
"""One seal over three parts beside three seals (uvhttp_tls_gpu_seal_parts against
uvhttp_tls_gpu_seal_frames; not the BASELINE metric, bench.py is untouched), and the close pass
beside the control replies.

Workload: what a TLS echo server's batch leaves in its send arena, resident in HBM, one
AES-128-GCM TLS 1.3 key per connection:
  c4   4 096 connections x 256 echoes of 256 payload bytes, 1 % of the frames PINGs (a PONG of
       0-125 bytes each, part 1), 1 % of the connections closed (an 18-byte CLOSE, part 2)
  c3   4 096 connections x 16 echoes of 64 KiB, the same replies and closes
The frame bytes are random (the seal does not parse them); offsets and runs are built with numpy.

`parts` is one seal_parts call over the three parts.  `three_calls` is the baseline the call
replaces, from the same process over the same frames and keys: three seal_frames calls, the second
and third taking their sequence numbers from the previous call's results with a device-side copy
of next_seq into the sends table (no host read), each into an output buffer of its own.  Both are
bracketed by HIP events; `crypto_ms` is the engine's own HIP-event time of the record-crypto
kernels inside the calls and `plan_ms` what is left (the plan passes, the key schedules and, for
the baseline, the two copies).  The record counts and bytes of the two are compared.

--close adds, on the c4 shape, uvhttp_ws_gpu_close_frames_streams beside the same-run
control_replies_streams after one decode_streams (tools/bench_replies.py's wire, 1 % PINGs; 1 % of
the results marked failed on the host before the timed calls).

--coalesce times, per shape and for AES-128-GCM and ChaCha20-Poly1305 keys, uvhttp_tls_gpu_seal_parts_coalesced
beside the same-run seal_parts over the same arena (the two alternate inside every step), with the
records and output bytes of each and the coalesced call's time outside its seal kernels.

    python tools/bench_parts.py [--steps K] [--warmup W] [--shapes c4,c3] [--scale S] [--close] [--coalesce]
                                [--out FILE]

One JSON line per shape on stdout (and appended to FILE), then nothing else.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

SHAPES = {"c4": (256, 256), "c3": (16, 65536)}  # echoes per connection, payload bytes
SEND_DT = np.dtype([("seq", "<u8"), ("first_frame", "<u4"), ("n_frames", "<u4"), ("key", "<u4"), ("type", "u1"),
                    ("reserved", "u1", 3), ("reserved2", "<u8")])
KEY_DT = np.dtype([("key", "u1", 32), ("iv", "u1", 12), ("key_len", "<u4"), ("version", "<u4"), ("cipher", "<u4"),
                   ("reserved", "<u4", 2)])


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


def table(sizes_per_conn):
    """per-connection frame sizes (list of arrays) -> (offsets uint64 [n + 1], runs uint32 [conns, 2])"""
    counts = np.array([len(s) for s in sizes_per_conn], np.int64)
    flat = np.concatenate(sizes_per_conn) if counts.sum() else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(flat)]).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return off, np.stack([first, counts], 1).astype(np.uint32)


def workload(t, name, conns, cipher=0):
    """the send arena of `conns` connections, its three frame tables and run tables, one TLS 1.3 key
    per connection (cipher 0 = AES-128-GCM, 1 = ChaCha20-Poly1305) and the sends, on the device"""
    dev = "cuda:0"
    per, plen = SHAPES[name]
    rng = np.random.default_rng(0x5EED)
    hdr = 2 if plen < 126 else 4 if plen < 65536 else 10
    echo = [np.full(per, hdr + plen, np.int64) for _ in range(conns)]
    pongs = [2 + rng.integers(0, 126, rng.binomial(per, 0.01)) for _ in range(conns)]
    closes = [np.full(1 if rng.random() < 0.01 else 0, 18, np.int64) for _ in range(conns)]
    tabs = [table(x) for x in (echo, pongs, closes)]
    lens = [int(off[-1]) for off, _ in tabs]
    bases = [0, (lens[0] + 255) // 256 * 256, (lens[0] + 255) // 256 * 256 + (lens[1] + 255) // 256 * 256]
    arena = t.randint(0, 256, (bases[2] + lens[2] + 256,), dtype=t.uint8, device=dev)
    up = lambda a: t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_off = [up(off) for off, _ in tabs]
    d_runs = [up(runs) for _, runs in tabs]
    keys = np.zeros(conns, KEY_DT)
    keys["key"], keys["iv"] = rng.integers(0, 256, (conns, 32)), rng.integers(0, 256, (conns, 12))
    keys["key_len"], keys["version"], keys["cipher"] = 32 if cipher else 16, 0x0304, cipher
    d_keys = up(keys)
    sends = np.zeros(conns, SEND_DT)
    sends["seq"], sends["key"], sends["type"] = rng.integers(0, 1 << 40, conns), np.arange(conns), 23
    d_sends = up(sends)
    n_frames = [len(off) - 1 for off, _ in tabs]
    parts = [(bases[k], lens[k], d_off[k], d_runs[k], 8, n_frames[k]) for k in range(3)]
    return dict(hdr=hdr, plen=plen, echo=echo, pongs=pongs, closes=closes, tabs=tabs, lens=lens, bases=bases,
                arena=arena, up=up, d_off=d_off, d_keys=d_keys, sends=sends, d_sends=d_sends, n_frames=n_frames,
                parts=parts)


def seal_shape(t, U, name, conns, steps, warmup):
    dev = "cuda:0"
    w = workload(t, name, conns)
    hdr, plen, echo, pongs, closes, tabs, lens, bases = (w[k] for k in ("hdr", "plen", "echo", "pongs", "closes", "tabs",
                                                                        "lens", "bases"))
    arena, up, d_off, d_keys, sends, d_sends, n_frames, parts = (w[k] for k in ("arena", "up", "d_off", "d_keys", "sends",
                                                                                "d_sends", "n_frames", "parts"))
    records = [int(sum(-(-int(s) // 16384) for x in part for s in x)) for part in (echo, pongs, closes)]
    over = 5 + 1 + 16
    out_bytes = [ln + r * over for ln, r in zip(lens, records)]
    eng = U.TlsEngine(0)
    eng.set_timing(True)
    out = t.zeros(sum(out_bytes) + 64, dtype=t.uint8, device=dev)
    recs = t.zeros((sum(records) + 1) * 32, dtype=t.uint8, device=dev)
    res = t.zeros(conns * 48, dtype=t.uint8, device=dev)
    summ = t.zeros(32, dtype=t.uint8, device=dev)

    def one():
        eng.seal_parts(arena, parts, d_sends, conns, d_keys, conns, sum(records), out, records=recs, results=res,
                       summary=summ)

    # the baseline: a sends table, record table, results and output of its own per call
    b_sends = []
    for k in range(3):
        s = sends.copy()
        s["first_frame"], s["n_frames"] = tabs[k][1][:, 0], tabs[k][1][:, 1]
        b_sends.append(up(s))
    b_out = [t.zeros(n + 64, dtype=t.uint8, device=dev) for n in out_bytes]
    b_recs = [t.zeros((r + 1) * 32, dtype=t.uint8, device=dev) for r in records]
    b_res = [t.zeros(conns * 48, dtype=t.uint8, device=dev) for _ in range(3)]
    b_sum = [t.zeros(32, dtype=t.uint8, device=dev) for _ in range(3)]

    def three():
        for k in range(3):
            if k:  # next_seq of the previous call -> this call's seq, on the device
                b_sends[k].view(t.int64).view(conns, 4)[:, 0] = b_res[k - 1].view(t.int64).view(conns, 6)[:, 2]
            eng.seal_frames(arena[bases[k]:], d_off[k], n_frames[k], b_sends[k], conns, d_keys, conns, records[k],
                            b_out[k], records=b_recs[k], results=b_res[k], summary=b_sum[k], frames_len=lens[k])

    rows = {}
    for label, fn in (("parts", one), ("three_calls", three)):
        for _ in range(warmup):
            fn()
        t.cuda.synchronize()
        eng.kernel_time()
        med, lo, mean = timed(t, fn, steps, 0)
        crypto, _ = eng.kernel_time()
        rows[label] = {"ms": round(med, 4), "min_ms": round(lo, 4), "mean_ms": round(mean, 4),
                       "crypto_ms": round(crypto / steps, 4), "plan_ms": round(mean - crypto / steps, 4)}
    sm = np.frombuffer(summ.cpu().numpy().tobytes(), "<u8")
    base_bytes = sum(int(np.frombuffer(x.cpu().numpy().tobytes(), "<u8")[0]) for x in b_sum)
    assert int(sm[0]) == sum(out_bytes) == base_bytes, (int(sm[0]), sum(out_bytes), base_bytes)
    assert int(sm[1] >> 32) == 0 and int(sm[1] & 0xFFFFFFFF) == sum(records)
    # the same sequence numbers: the last call's next_seq is the one call's
    last = b_res[2].view(t.int64).view(conns, 6)[:, 2]
    assert t.equal(last, res.view(t.int64).view(conns, 6)[:, 2])
    eng.close()
    return {
        "metric": "seal_parts over three parts, ms per call (device-resident)", "value": rows["parts"]["ms"], "unit": "ms",
        "n_gpus": 1, "higher_is_better": False, "steps": steps, "warmup": warmup, "shape": name,
        "config": {"connections": conns, "echoes": n_frames[0], "echo_frame_bytes": hdr + plen, "replies": n_frames[1],
                   "closes": n_frames[2], "frame_bytes": sum(lens), "records": sum(records), "out_bytes": sum(out_bytes)},
        "parts": rows["parts"], "same_run_three_calls": rows["three_calls"],
        "vs_three_calls": round(rows["parts"]["ms"] / rows["three_calls"]["ms"], 3),
        "gb_per_s": round(sum(lens) / rows["parts"]["ms"] / 1e6, 2),
    }


def coalesce_shape(t, U, name, conns, steps, warmup, cipher):
    """uvhttp_tls_gpu_seal_parts_coalesced beside the same-run seal_parts over the same arena, the
    two calls alternating inside every step, each bracketed by HIP events of its own; then each call
    alone for the engine's own HIP-event time of the seal kernels (`crypto_ms`): what is left of a
    coalesced call (`gather_plan_ms`) is its gather and its plan kernels."""
    dev = "cuda:0"
    w = workload(t, name, conns, cipher)
    lens, arena, parts, d_sends, d_keys = w["lens"], w["arena"], w["parts"], w["d_sends"], w["d_keys"]
    over = 5 + 1 + 16
    per_frame = int(sum(-(-int(s) // 16384) for part in (w["echo"], w["pongs"], w["closes"]) for x in part for s in x))
    stream = [int(sum(int(x[c].sum()) for x in (w["echo"], w["pongs"], w["closes"]))) for c in range(conns)]
    packed = sum(-(-b // 16384) for b in stream)
    need = {"parts": (per_frame, sum(lens) + per_frame * over), "coalesced": (packed, sum(lens) + packed * over)}
    eng = U.TlsEngine(0)
    eng.set_timing(True)
    buf = {k: (t.zeros(b + 64, dtype=t.uint8, device=dev), t.zeros((r + 1) * 32, dtype=t.uint8, device=dev),
               t.zeros(conns * 48, dtype=t.uint8, device=dev), t.zeros(32, dtype=t.uint8, device=dev))
           for k, (r, b) in need.items()}
    call = {"parts": eng.seal_parts, "coalesced": eng.seal_parts_coalesced}

    def run(k):
        out, recs, res, summ = buf[k]
        call[k](arena, parts, d_sends, conns, d_keys, conns, need[k][0], out, records=recs, results=res, summary=summ)

    for _ in range(warmup):
        run("parts")
        run("coalesced")
    t.cuda.synchronize()
    ev = [[t.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    for a, b, c in ev:
        a.record()
        run("parts")
        b.record()
        run("coalesced")
        c.record()
    t.cuda.synchronize()
    ms = {"parts": sorted(a.elapsed_time(b) for a, b, _ in ev), "coalesced": sorted(b.elapsed_time(c) for _, b, c in ev)}
    rows = {}
    for k in ("parts", "coalesced"):
        eng.kernel_time()
        for _ in range(steps):
            run(k)
        t.cuda.synchronize()
        crypto, _ = eng.kernel_time()
        summ = np.frombuffer(buf[k][3].cpu().numpy().tobytes(), "<u8")
        assert (int(summ[1] & 0xFFFFFFFF), int(summ[0]), int(summ[1] >> 32)) == (*need[k], 0), (k, summ, need[k])
        med = ms[k][len(ms[k]) // 2]
        rows[k] = {"ms": round(med, 4), "min_ms": round(ms[k][0], 4), "mean_ms": round(sum(ms[k]) / steps, 4),
                   "crypto_ms": round(crypto / steps, 4), "records": need[k][0], "out_bytes": need[k][1]}
    rows["coalesced"]["gather_plan_ms"] = round(rows["coalesced"]["ms"] - rows["coalesced"]["crypto_ms"], 4)
    rows["coalesced"]["gather_plan_share"] = round(rows["coalesced"]["gather_plan_ms"] / rows["coalesced"]["ms"], 3)
    # the same sequence numbers' worth of plaintext: plain_len per send is equal
    assert t.equal(buf["parts"][2].view(t.int64).view(conns, 6)[:, 5], buf["coalesced"][2].view(t.int64).view(conns, 6)[:, 5])
    eng.close()
    return {
        "metric": "seal_parts_coalesced over three parts, ms per call (device-resident)",
        "value": rows["coalesced"]["ms"], "unit": "ms", "n_gpus": 1, "higher_is_better": False, "steps": steps,
        "warmup": warmup, "shape": name, "aead": "chacha20-poly1305" if cipher else "aes-128-gcm",
        "config": {"connections": conns, "echoes": w["n_frames"][0], "echo_frame_bytes": w["hdr"] + w["plen"],
                   "replies": w["n_frames"][1], "closes": w["n_frames"][2], "frame_bytes": sum(lens)},
        "coalesced": rows["coalesced"], "same_run_seal_parts": rows["parts"],
        "vs_seal_parts": round(rows["coalesced"]["ms"] / rows["parts"]["ms"], 3),
        "gb_per_s": round(sum(lens) / rows["coalesced"]["ms"] / 1e6, 2),
    }


def close_pass(t, U, conns, steps, warmup):
    import bench_replies as BR
    dev = "cuda:0"
    eng = U.GpuEngine(0)
    frames = conns * BR.PER
    wire, begin, length, pings = BR.build_wire(conns, 0.01, 0x5EED)
    d_wire = t.zeros(wire.size + 64, dtype=t.uint8, device=dev)
    d_wire[:wire.size] = t.from_numpy(wire).to(dev)
    st = np.zeros(conns, dtype=U.STREAM_DT)
    st["begin"], st["len"] = begin, length
    st["recv_buffer_size"] = max(65536, int(length.max()))
    st["max_frame_size"], st["max_message_size"], st["is_server"] = 16 << 20, 64 << 20, 1
    d_st = t.from_numpy(st.view(np.uint8).copy()).to(dev)
    desc = t.empty(frames * 32, dtype=t.uint8, device=dev)
    res = t.zeros(conns * 64, dtype=t.uint8, device=dev)
    eng.decode_streams(d_wire, d_st, conns, frames, desc=desc, results=res, wire_len=wire.size)
    t.cuda.synchronize()
    h = res.cpu().numpy().view(U.STREAM_RESULT_DT).copy()
    failed = np.random.default_rng(7).random(conns) < 0.01
    h["first_status"][failed] = -2
    res.copy_(t.from_numpy(h.view(np.uint8).reshape(-1)).to(dev))
    max_replies, out_cap = max(1, pings.size), max(16, int((2 + pings).sum()))
    r_out = eng.control_replies_streams(d_wire, desc, frames, d_st, res, conns, max_replies, out_cap, wire_len=wire.size)
    c_out = eng.close_frames_streams(d_st, res, conns, 22 * conns, reply_conn=r_out[2])
    runs_r = t.zeros(conns * 2, dtype=t.int32, device=dev)
    runs_c = t.zeros(conns * 2, dtype=t.int32, device=dev)

    def replies():
        eng.control_replies_streams(d_wire, desc, frames, d_st, res, conns, max_replies, out_cap, out=r_out[0],
                                    out_off=r_out[1], runs=runs_r, conn=r_out[2], summary=r_out[3], wire_len=wire.size)

    def closes():
        eng.close_frames_streams(d_st, res, conns, 22 * conns, reply_conn=r_out[2], out=c_out[0], out_off=c_out[1],
                                 runs=runs_c, conn=c_out[2], summary=c_out[3])

    r_med, r_lo, r_mean = timed(t, replies, steps, warmup)
    med, lo, mean = timed(t, closes, steps, warmup)
    s = eng.read_close_summary(c_out[3])
    assert s["n_1002"] == int(failed.sum()) and s["out_bytes"] == 18 * s["n_1002"] and s["status"] == 0, s
    eng.close()
    return {
        "metric": "close_frames_streams after decode_streams, ms per call (device-resident)", "value": round(med, 4),
        "unit": "ms", "n_gpus": 1, "higher_is_better": False, "steps": steps, "warmup": warmup,
        "config": {"connections": conns, "frames": frames, "closes": s["n_closes"], "replies": int(pings.size)},
        "ms": round(med, 4), "min_ms": round(lo, 4), "mean_ms": round(mean, 4),
        "same_run_control_replies": {"ms": round(r_med, 4), "min_ms": round(r_lo, 4), "mean_ms": round(r_mean, 4)},
        "vs_control_replies": round(med / r_med, 3),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="c4,c3")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 4 096 connections (smoke runs)")
    ap.add_argument("--close", action="store_true", help="also time the close pass beside the control replies")
    ap.add_argument("--coalesce", action="store_true",
                    help="time seal_parts_coalesced beside seal_parts, both AEADs, instead of the shapes' default rows")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()

    import torch
    import uvhttp_amd as U
    conns = max(1, int(4096 * args.scale))
    names = [name for name in args.shapes.split(",") if name]
    if args.coalesce:
        lines = [coalesce_shape(torch, U, name, conns, args.steps, args.warmup, cipher) for name in names
                 for cipher in (0, 1)]
    else:
        lines = [seal_shape(torch, U, name, conns, args.steps, args.warmup) for name in names]
    if args.close:
        lines.append(close_pass(torch, U, conns, args.steps, args.warmup))
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
