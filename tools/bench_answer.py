#!/usr/bin/env python3
"""Answers in frame order on one MI355X (uvhttp_ws_gpu_answer_messages_streams; not the BASELINE
metric, bench.py is untouched).

Shapes, resident in HBM, every connection a server connection fed masked client frames:
  c4_p1    4 096 connections x 256 frames: messages of 256 bytes, 1 % of the frames PINGs of
           0-125 bytes (tools/bench_replies.py's wire)
  c4_p10   the same with 10 % PINGs
  c3_p1    4 096 connections x 16 single-frame messages of 64 KiB; one connection in six has a
           PING of 64 bytes after its eighth message (1 % of the frames)
1 % of the stream results are marked failed on the host before the timed calls, so close_frames has
its 1002 closes to build.

Three comparisons, the calls of each alternating inside a step, each call bracketed by HIP events:
  answer   answer_messages_streams beside the same run's echo_messages_streams (timed twice a
           step: the gap between its two medians is the run's noise) and control_replies_streams.
           `fused_le_sum`: answer <= echo + replies + 2 x |echo - echo again|
  parts    seal_parts over (answers, closes) beside (echoes, replies, closes), one AES-128-GCM TLS
           1.3 key per connection, over the frames the calls above left on the device
  coalesced  seal_parts_coalesced likewise
The bytes are compared once: both seals carry the same plaintext length per connection.

    python tools/bench_answer.py [--steps K] [--warmup W] [--shapes c4_p1,c4_p10,c3_p1] [--scale S] [--out FILE]

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

import bench_echo as BE  # noqa: E402
import bench_parts as BP  # noqa: E402
import bench_replies as BR  # noqa: E402

SHAPES = ("c4_p1", "c4_p10", "c3_p1")


def build(t, name, conns):
    """-> (device wire, wire_len, begin, len per connection, frames, data frames, message bytes, PING payload lengths)"""
    dev = "cuda:0"
    if name.startswith("c4"):
        wire, begin, length, pings = BR.build_wire(conns, 0.10 if name == "c4_p10" else 0.01, 0x5EED)
        d_wire = t.zeros(wire.size + 64, dtype=t.uint8, device=dev)
        d_wire[:wire.size] = t.from_numpy(wire).to(dev)
        frames = conns * BR.PER
        return d_wire, wire.size, begin, length, frames, frames - pings.size, BR.PLEN, pings
    per, mlen = 16, 65536
    plain = BE.connection_bytes(per, mlen, 1, 0x5EED)
    flen = plain.size // per
    ping = np.frombuffer(BE.frame(9, 1, bytes(range(64)), b"\x01\x02\x03\x04"), np.uint8)
    with_ping = np.concatenate([plain[:8 * flen], ping, plain[8 * flen:]])
    group = t.from_numpy(np.concatenate([with_ping] + [plain] * 5)).to(dev)
    sizes = np.array(([with_ping.size] + [plain.size] * 5) * (conns // 6 + 1), np.int64)[:conns]
    begin = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    wire_len = int(sizes.sum())
    d_wire = t.zeros(wire_len + 64, dtype=t.uint8, device=dev)
    d_wire[:wire_len] = group.repeat(conns // 6 + 1)[:wire_len]
    n_ping = int((sizes == with_ping.size).sum())
    return d_wire, wire_len, begin, sizes, conns * per + n_ping, conns * per, mlen, np.full(n_ping, 64, np.int64)


def stats(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "mean_ms": round(sum(v) / len(v), 4)}


def alternate(t, calls, steps, warmup):
    """{name: fn} run in this order inside every step -> {name: stats}"""
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
    return {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def shape(t, U, name, conns, steps, warmup):
    dev = "cuda:0"
    eng = U.GpuEngine(0)
    d_wire, wire_len, begin, length, frames, msgs, mlen, pings = build(t, name, conns)
    st = np.zeros(conns, dtype=U.STREAM_DT)
    st["begin"], st["len"] = begin, length
    st["recv_buffer_size"] = max(65536, int(np.max(length)))
    st["max_frame_size"], st["max_message_size"], st["is_server"] = 16 << 20, 64 << 20, 1
    d_st = t.from_numpy(st.view(np.uint8).copy()).to(dev)
    desc = t.empty(frames * 32, dtype=t.uint8, device=dev)
    res = t.zeros(conns * 64, dtype=t.uint8, device=dev)
    eng.decode_streams(d_wire, d_st, conns, frames, desc=desc, results=res, wire_len=wire_len)
    t.cuda.synchronize()
    h = res.cpu().numpy().view(U.STREAM_RESULT_DT).copy()
    assert int(h["n_delivered"].sum()) == frames
    failed = np.random.default_rng(7).random(conns) < 0.01
    h["first_status"][failed] = -2
    res.copy_(t.from_numpy(h.view(np.uint8).reshape(-1)).to(dev))

    n_rep = int(pings.size)
    echo_bytes = msgs * (BE.header_bytes(mlen) + mlen)
    reply_bytes = int((2 + pings).sum())
    up16 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    close_cap = 22 * conns
    base_a, base_e = 0, up16(echo_bytes + reply_bytes)
    base_r = base_e + up16(echo_bytes)
    base_c = base_r + up16(max(16, reply_bytes))
    arena = t.zeros(base_c + close_cap + 256, dtype=t.uint8, device=dev)
    n_ans, max_rep = msgs + n_rep, max(1, n_rep)
    zeros = lambda n, dt=t.uint8: t.zeros(n, dtype=dt, device=dev)  # noqa: E731
    a = dict(out=arena[base_a:base_a + echo_bytes + reply_bytes], out_off=zeros(n_ans + 1, t.int64), runs=zeros(2 * conns, t.int32),
             open_off=zeros(conns + 1, t.int64), conn=zeros(32 * conns), summary=zeros(32), reply_conn=zeros(16 * conns))
    e = dict(out=arena[base_e:base_e + echo_bytes], out_off=zeros(msgs + 1, t.int64), runs=zeros(2 * conns, t.int32),
             open_off=zeros(conns + 1, t.int64), conn=zeros(32 * conns), summary=zeros(32))
    r = dict(out=arena[base_r:base_r + max(16, reply_bytes)], out_off=zeros(max_rep + 1, t.int64), runs=zeros(2 * conns, t.int32),
             conn=zeros(16 * conns), summary=zeros(32))
    c = dict(out=arena[base_c:base_c + close_cap], out_off=zeros(conns + 1, t.int64), runs=zeros(2 * conns, t.int32),
             conn=zeros(16 * conns), summary=zeros(32))

    def answer():
        eng.answer_messages_streams(d_wire, desc, frames, d_st, res, conns, n_ans, echo_bytes + reply_bytes,
                                    wire_len=wire_len, **a)

    def echo():
        eng.echo_messages_streams(d_wire, desc, frames, d_st, res, conns, msgs, echo_bytes, wire_len=wire_len, **e)

    def replies():
        eng.control_replies_streams(d_wire, desc, frames, d_st, res, conns, max_rep, max(16, reply_bytes),
                                    wire_len=wire_len, **r)

    rows = alternate(t, {"echo_messages": echo, "control_replies": replies, "answer_messages": answer,
                         "echo_messages_again": echo}, steps, warmup)
    s = eng.read_answer_summary(a["summary"])
    assert s == {"out_bytes": echo_bytes + reply_bytes, "open_bytes": 0, "n_answers": n_ans, "n_replies": n_rep,
                 "n_closed_conns": 0, "status": U.ECHO_OK}, s
    assert eng.read_echo_summary(e["summary"])["out_bytes"] == echo_bytes
    assert eng.read_reply_summary(r["summary"])["out_bytes"] == reply_bytes
    eng.close_frames_streams(d_st, res, conns, close_cap, reply_conn=a["reply_conn"], clear_runs=[a["runs"]],
                             clear_stride=[8], **c)
    t.cuda.synchronize()
    n_close = eng.read_close_summary(c["summary"])["n_closes"]
    assert n_close == int(failed.sum())
    noise = abs(rows["echo_messages"]["ms"] - rows["echo_messages_again"]["ms"])
    two = rows["echo_messages"]["ms"] + rows["control_replies"]["ms"]
    med = rows["answer_messages"]["ms"]

    # the seals over the frames the calls left: two parts beside three
    rng = np.random.default_rng(0x5EED)
    keys = np.zeros(conns, BP.KEY_DT)
    keys["key"], keys["iv"] = rng.integers(0, 256, (conns, 32)), rng.integers(0, 256, (conns, 12))
    keys["key_len"], keys["version"], keys["cipher"] = 16, 0x0304, 0
    sends = np.zeros(conns, BP.SEND_DT)
    sends["seq"], sends["key"], sends["type"] = rng.integers(0, 1 << 40, conns), np.arange(conns), 23
    up = lambda x: t.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_keys, d_sends = up(keys), up(sends)
    two_parts = [(base_a, echo_bytes + reply_bytes, a["out_off"], a["runs"], 8, n_ans),
                 (base_c, close_cap, c["out_off"], c["runs"], 8, conns)]
    three_parts = [(base_e, echo_bytes, e["out_off"], e["runs"], 8, msgs),
                   (base_r, max(16, reply_bytes), r["out_off"], r["runs"], 8, max_rep),
                   (base_c, close_cap, c["out_off"], c["runs"], 8, conns)]
    records = msgs * -(-(BE.header_bytes(mlen) + mlen) // 16384) + n_rep + n_close
    out_bytes = echo_bytes + reply_bytes + 18 * n_close + records * 22
    tls = U.TlsEngine(0)
    seal_rows = {}
    for label, fn in (("parts", tls.seal_parts), ("coalesced", tls.seal_parts_coalesced)):
        buf = {k: (zeros(out_bytes + 64), zeros((records + 1) * 32), zeros(conns * 48), zeros(32)) for k in ("two", "three")}

        def run(k, parts, fn=fn, buf=buf):
            out, recs, sres, ssum = buf[k]
            fn(arena, parts, d_sends, conns, d_keys, conns, records, out, records=recs, results=sres, summary=ssum)

        got = alternate(t, {"two_parts": lambda: run("two", two_parts), "three_parts": lambda: run("three", three_parts)},
                        steps, warmup)
        plain = [buf[k][2].view(t.int64).view(conns, 6)[:, 5] for k in ("two", "three")]
        assert t.equal(plain[0], plain[1]) and int(plain[0].sum()) == echo_bytes + reply_bytes + 18 * n_close
        seal_rows[label] = dict(got, vs_three_parts=round(got["two_parts"]["ms"] / got["three_parts"]["ms"], 3))
        del buf
    tls.close()
    eng.close()
    return {
        "metric": "answer_messages_streams after decode_streams, ms per call (device-resident)", "value": med, "unit": "ms",
        "n_gpus": 1, "higher_is_better": False, "steps": steps, "warmup": warmup, "shape": name,
        "config": {"connections": conns, "frames": frames, "messages": msgs, "message_bytes": mlen, "replies": n_rep,
                   "closes": n_close, "wire_bytes": int(wire_len), "answer_bytes": echo_bytes + reply_bytes},
        **rows["answer_messages"],
        "same_run": {k: v for k, v in rows.items() if k != "answer_messages"},
        "echo_plus_replies_ms": round(two, 4), "same_run_noise_ms": round(noise, 4),
        "vs_two_calls": round(med / two, 3), "fused_le_sum": bool(med <= two + 2 * noise),
        "seal_parts": seal_rows["parts"], "seal_parts_coalesced": seal_rows["coalesced"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 4 096 connections (smoke runs)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()

    import torch
    import uvhttp_amd as U
    conns = max(1, int(4096 * args.scale))
    for name in args.shapes.split(","):
        line = shape(torch, U, name, conns, args.steps, args.warmup)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
