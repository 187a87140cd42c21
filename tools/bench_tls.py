#!/usr/bin/env python3
"""TLS record open throughput on one MI355X (not the BASELINE metric).

Workload: `--conns` connections, each with `--records` application-data records of `--plen`
content bytes (default 65 536 x 4 x 16 KiB: 64 KiB of plaintext per connection, the C3 shape),
TLS 1.3 (or --version 12), AES-128-GCM (or --klen 32, or --cipher chacha: ChaCha20-Poly1305),
one key per connection.  The records
are sealed on the device (uvhttp_tls_gpu_seal_records), then each timed step opens all of them
(uvhttp_tls_gpu_open_records: key schedules, walk, crypto, finalize) with inputs resident in
HBM.  Prints one JSON line: plaintext GiB/s per step, the crypto kernel's time (HIP events),
its bytes moved (ciphertext read + plaintext written), and two single-core CPU baselines on a
bounded sample: the oracle restatement (byte-oriented C, the parity checker) and OpenSSL 3.0
EVP AES-GCM / ChaCha20-Poly1305 from the system libcrypto (AES-NI + PCLMUL / AVX2: what a
production CPU stack does).

    python tools/bench_tls.py [--conns N] [--records R] [--plen P] [--version 13|12] [--klen 16|32]
                              [--cipher aes|chacha] [--chain]

--chain: the TLS -> WebSocket chain the reference runs per read (src/uvhttp_connection.c:
1128-1158: mbedtls_ssl_read, then process_data on each decrypted chunk).  Each connection's
plaintext is one masked BINARY WebSocket frame filling its records (65 528-byte payload at the
default 4 x 16 KiB), and a step is open_records -> ws_streams (one process_data call per
record) -> decode_reads: ciphertext in HBM -> unmasked messages in HBM.  The rate is WebSocket
payload bytes per second.

--send: the send side.  `--conns` sends of `--frames` server (unmasked) BINARY frames of `--fsize`
bytes each (header included), or with --broadcast `--conns` sends that all name one frame.  Three
things are timed with device events in the same run, alternating: uvhttp_ws_gpu_build_frames +
uvhttp_tls_gpu_seal_frames (the send path), the uvhttp_tls_gpu_seal_frames call alone, and
uvhttp_tls_gpu_seal_records over the very record table seal_frames wrote (the crypto with a
host-made plan: what the device-side plan is compared against).  The two outputs are compared
byte for byte.  One JSON line, appended to --out (default profiles/tls_send_bench.jsonl).

    python tools/bench_tls.py --send [--broadcast] [--conns N] [--frames F] [--fsize B]
                              [--max-fragment M] [--version 13|12] [--klen 16|32] [--cipher aes|chacha]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GIB = float(1 << 30)


def openssl_baseline(keyrec, seq, wire, n_rec, rlen, version, seconds, chacha=False):
    """OpenSSL EVP AEAD decrypt of the same records, 1 thread (libcrypto.so.3)."""
    try:
        L = C.CDLL("libcrypto.so.3")
    except OSError:
        return None
    vp, ip = C.c_void_p, C.c_int
    for name, res, args in [("EVP_CIPHER_CTX_new", vp, []), ("EVP_CIPHER_CTX_free", None, [vp]),
                            ("EVP_aes_128_gcm", vp, []), ("EVP_aes_256_gcm", vp, []),
                            ("EVP_chacha20_poly1305", vp, []),
                            ("EVP_DecryptInit_ex", ip, [vp, vp, vp, vp, vp]),
                            ("EVP_DecryptUpdate", ip, [vp, vp, C.POINTER(ip), vp, ip]),
                            ("EVP_DecryptFinal_ex", ip, [vp, vp, C.POINTER(ip)]),
                            ("EVP_CIPHER_CTX_ctrl", ip, [vp, ip, ip, vp])]:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    klen = int(keyrec["key_len"])
    key = bytes(keyrec["key"][:klen])
    iv = bytes(keyrec["iv"])
    cipher = (L.EVP_chacha20_poly1305() if chacha else
              L.EVP_aes_128_gcm() if klen == 16 else L.EVP_aes_256_gcm())
    ctx = L.EVP_CIPHER_CTX_new()
    out = C.create_string_buffer(rlen)
    outl = ip(0)
    buf = wire.tobytes()
    done, t0, ok = 0, time.perf_counter(), True
    while time.perf_counter() - t0 < seconds:
        for j in range(n_rec):
            rec = buf[j * (5 + rlen):(j + 1) * (5 + rlen)]
            s = seq + j
            if version == 0x0304:
                nonce = bytes(a ^ b for a, b in zip(iv, bytes(4) + s.to_bytes(8, "big")))
                aad, ct = rec[:5], rec[5:5 + rlen - 16]
            elif chacha:  # RFC 7905: implicit nonce
                nonce = bytes(a ^ b for a, b in zip(iv, bytes(4) + s.to_bytes(8, "big")))
                ct = rec[5:5 + rlen - 16]
                aad = s.to_bytes(8, "big") + rec[:3] + len(ct).to_bytes(2, "big")
            else:
                nonce = iv[:4] + rec[5:13]
                ct = rec[13:5 + rlen - 16]
                aad = s.to_bytes(8, "big") + rec[:3] + len(ct).to_bytes(2, "big")
            tag = rec[5 + rlen - 16:5 + rlen]
            L.EVP_DecryptInit_ex(ctx, cipher, None, key, nonce)
            L.EVP_DecryptUpdate(ctx, None, C.byref(outl), aad, len(aad))
            L.EVP_DecryptUpdate(ctx, out, C.byref(outl), ct, len(ct))
            L.EVP_CIPHER_CTX_ctrl(ctx, 0x11, 16, tag)  # EVP_CTRL_GCM_SET_TAG
            ok &= L.EVP_DecryptFinal_ex(ctx, out, C.byref(outl)) == 1
            done += len(ct) - (1 if version == 0x0304 else 0)
    el = time.perf_counter() - t0
    L.EVP_CIPHER_CTX_free(ctx)
    return {"value": round(done / el / GIB, 3), "unit": "GiB/s", "cores": 1,
            "kind": "openssl-evp", "tags_ok": bool(ok),
            "sample": f"{n_rec} records x {rlen} B, {el:.1f} s"}


def frame_payload(fsize):
    """payload length of the unmasked frame of fsize bytes (header 2 / 4 / 10)"""
    for hdr, lo, hi in ((2, 0, 125), (4, 126, 65535), (10, 65536, 1 << 62)):
        if lo <= fsize - hdr <= hi:
            return fsize - hdr
    raise SystemExit(f"no frame is {fsize} bytes long")


def send_bench(args):
    import torch as t
    import _oracle as O  # test infrastructure: the key struct layout only
    import uvhttp_amd as U

    dev = "cuda:0"
    ver = 0x0304 if args.version == 13 else 0x0303
    chacha = args.cipher == "chacha"
    n_sends = args.conns
    per = 1 if args.broadcast else args.frames
    n_frames = 1 if args.broadcast else n_sends * per
    fsize, mf = args.fsize, args.max_fragment or 16384
    plen = frame_payload(fsize)
    rng = np.random.default_rng(7)
    nk = min(n_sends, 65536)  # the record table's slot is 16-bit: send i uses slot i % 65 536
    keys = np.zeros(nk, O.TLS_KEY_DT)
    keys["key"] = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    keys["iv"] = rng.integers(0, 256, (nk, 12), dtype=np.uint8)
    keys["key_len"], keys["version"] = (32 if chacha else args.klen), ver
    keys["cipher"] = O.CHACHA if chacha else O.AES_GCM
    over = 5 + 16 + (1 if ver == 0x0304 else 0 if chacha else 8)
    rec_per_frame = (fsize + mf - 1) // mf
    n_rec = n_sends * per * rec_per_frame
    out_bytes = n_sends * per * (fsize + rec_per_frame * over)
    # build descriptors: payloads from a shared 64 MiB (or smaller) random source
    src_len = max(plen, min(64 << 20, max(1, n_frames * plen)))
    src = t.randint(0, 256, (src_len,), dtype=t.uint8, device=dev)
    bd = np.zeros(n_frames, np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("key", "<u4"),
                                      ("opcode", "u1"), ("fin", "u1"), ("mask", "u1"), ("r0", "u1"),
                                      ("r1", "<u8")]))
    bd["payload_off"] = (np.arange(n_frames, dtype=np.uint64) * np.uint64(plen)) % np.uint64(max(1, src_len - plen + 1))
    bd["payload_len"], bd["opcode"], bd["fin"] = plen, 2, 1
    sends = np.zeros(n_sends, np.dtype([("seq", "<u8"), ("first_frame", "<u4"), ("n_frames", "<u4"),
                                        ("key", "<u4"), ("type", "u1"), ("r", "u1", 3), ("r2", "<u8")]))
    sends["seq"] = rng.integers(0, 1 << 40, n_sends, dtype=np.uint64)
    sends["first_frame"] = 0 if args.broadcast else np.arange(n_sends, dtype=np.uint64) * per
    sends["n_frames"], sends["type"] = per, 23
    sends["key"] = np.arange(n_sends) % nk
    up = lambda a: t.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_bd, d_sends, d_keys = up(bd), up(sends), up(keys)
    frames = t.empty(n_frames * fsize, dtype=t.uint8, device=dev)
    d_off = t.zeros(n_frames + 1, dtype=t.int64, device=dev)
    out = t.empty(out_bytes, dtype=t.uint8, device=dev)
    out2 = t.empty(out_bytes, dtype=t.uint8, device=dev)
    recs = t.zeros(n_rec * U.TLS_SEAL_BYTES, dtype=t.uint8, device=dev)
    res = t.zeros(n_sends * U.TLS_SEND_RESULT_BYTES, dtype=t.uint8, device=dev)
    summ = t.zeros(U.TLS_SEND_SUMMARY_BYTES, dtype=t.uint8, device=dev)
    weng = U.GpuEngine(0)
    eng = U.TlsEngine(0, library=U.load_library(args.lib) if args.lib else None)

    def build():
        weng.build_frames(src, d_bd, n_frames, frames, out_off=d_off)

    def seal_frames():
        eng.seal_frames(frames, d_off, n_frames, d_sends, n_sends, d_keys, nk, n_rec, out,
                        max_fragment=args.max_fragment, records=recs, results=res, summary=summ)

    def seal_records():
        eng.seal_records(frames, recs, n_rec, d_keys, nk, out2)

    def send_path():
        build()
        seal_frames()

    legs = {"build_frames+seal_frames": send_path, "seal_frames": seal_frames,
            "seal_records(same table)": seal_records}
    for _ in range(max(1, args.warmup)):
        for f in legs.values():
            f()
    t.cuda.synchronize()
    sm = summ.cpu().numpy()
    got_bytes, got_rec, got_failed = int(sm[:8].view("<u8")[0]), int(sm[8:12].view("<u4")[0]), int(sm[12:16].view("<u4")[0])
    assert (got_bytes, got_rec, got_failed) == (out_bytes, n_rec, 0), (got_bytes, got_rec, got_failed)
    assert t.equal(out, out2), "seal_frames and seal_records over its table differ"
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, f in legs.items():  # alternating: the legs share whatever else the machine does
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    # the seal kernels alone (engine HIP events), inside either call
    eng.set_timing(True)
    kern = {}
    for k in ("seal_frames", "seal_records(same table)"):
        eng.kernel_time()
        for _ in range(3):
            legs[k]()
        t.cuda.synchronize()
        ms, launches = eng.kernel_time()
        kern[k] = round(ms / max(1, launches), 4)
    eng.set_timing(False)
    med = {k: float(np.median(v)) for k, v in times.items()}
    plain = n_sends * per * fsize
    aead = "ChaCha20-Poly1305" if chacha else f"AES-{args.klen * 8}-GCM"
    shape = (f"broadcast of one {fsize}-byte frame to {n_sends} connections" if args.broadcast else
             f"{n_sends} sends x {per} frame(s) of {fsize} bytes")
    line = {
        "metric": "TLS send path: built frames -> sealed records (device-resident)",
        "value": round(plain / (med["seal_frames"] * 1e-3) / GIB, 2), "unit": "GiB/s of frame bytes (seal_frames)",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
        "config": {"workload": f"{shape}, TLS 1.{args.version % 10} {aead}, max_fragment {mf}",
                   "sends": n_sends, "frames": n_frames, "records": n_rec, "frame_bytes": fsize,
                   "out_bytes": out_bytes, "broadcast": bool(args.broadcast)},
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_max": {k: round(max(v), 4) for k, v in times.items()},
        "seal_kernels_ms": kern,
        "seal_frames_over_seal_records": round(med["seal_frames"] / med["seal_records(same table)"], 4),
        "timing": "device events around each call, legs alternating within a step, medians",
    }
    if args.lib:
        line["lib"] = os.path.basename(args.lib)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=65536)
    ap.add_argument("--records", type=int, default=4)
    ap.add_argument("--plen", type=int, default=16384)
    ap.add_argument("--version", type=int, default=13, choices=[12, 13])
    ap.add_argument("--klen", type=int, default=16, choices=[16, 32])
    ap.add_argument("--cipher", default="aes", choices=["aes", "chacha"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-seconds", type=float, default=4.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of the library (A/B runs)")
    ap.add_argument("--chain", action="store_true", help="open_records -> ws_streams -> decode_reads")
    ap.add_argument("--send", action="store_true", help="build_frames -> seal_frames beside seal_records")
    ap.add_argument("--broadcast", action="store_true", help="--send: one frame, --conns sends")
    ap.add_argument("--frames", type=int, default=1, help="--send: frames per send")
    ap.add_argument("--fsize", type=int, default=65536, help="--send: bytes of a frame, header included")
    ap.add_argument("--max-fragment", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tls_send_bench.jsonl"),
                    help="--send: the JSON line is appended here ('' = stdout only)")
    args = ap.parse_args()
    if args.send:
        return send_bench(args)

    import torch
    import _oracle as O  # test infrastructure: key structs and the CPU baseline leg only
    import uvhttp_amd as U

    ver = 0x0304 if args.version == 13 else 0x0303
    n, per, plen = args.conns, args.records, args.plen
    rng = np.random.default_rng(7)
    # one key slot per connection up to 65 536 (the seal descriptor's slot is 16-bit); beyond
    # that connection i uses slot i % 65 536 (synthetic data: shared keys change no work)
    nk = min(n, 65536)
    keys = np.zeros(nk, O.TLS_KEY_DT)
    keys["key"] = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    keys["iv"] = rng.integers(0, 256, (nk, 12), dtype=np.uint8)
    chacha = args.cipher == "chacha"
    keys["key_len"], keys["version"] = (32 if chacha else args.klen), ver
    keys["cipher"] = O.CHACHA if chacha else O.AES_GCM
    # TLSCiphertext.length: content + tag + (TLS 1.3 type byte | TLS 1.2 AES-GCM explicit nonce)
    rlen = plen + 16 + (1 if ver == 0x0304 else 0 if chacha else 8)
    aead = "ChaCha20-Poly1305" if chacha else f"AES-{args.klen * 8}-GCM"
    stride = 5 + rlen
    idx = np.arange(n * per, dtype=np.uint64)
    seals = np.zeros(n * per, O.TLS_SEAL_DT)
    seals["src_off"] = idx * plen
    seals["out_off"] = idx * stride
    seals["seq"] = idx % per
    seals["plain_len"] = plen
    seals["key"] = ((idx // per) % nk).astype(np.uint16)
    seals["type"] = 23
    streams = np.zeros(n, O.TLS_STREAM_DT)
    streams["begin"] = np.arange(n, dtype=np.uint64) * per * stride
    streams["len"] = per * stride
    streams["key"] = np.arange(n) % nk
    dev = "cuda:0"
    t = torch
    src = t.randint(0, 256, (n * per * plen,), dtype=t.uint8, device=dev)
    weng = None
    if args.chain:
        # one masked BINARY frame per connection filling its per * plen plaintext bytes
        weng = U.GpuEngine(0)
        conn_bytes = per * plen
        fp = conn_bytes - 8 if conn_bytes - 8 < 65536 else conn_bytes - 14
        assert U.gen_frame_stride(fp) == conn_bytes, "pick --records * --plen >= 134"
        weng.gen_frames(src, n, fp, 11, opcode0=2)
    wire = t.empty(n * per * stride, dtype=t.uint8, device=dev)
    out = t.empty(wire.numel(), dtype=t.uint8, device=dev)
    dk = t.from_numpy(keys.view(np.uint8).reshape(-1).copy()).to(dev)
    ds = t.from_numpy(seals.view(np.uint8).reshape(-1).copy()).to(dev)
    dst = t.from_numpy(streams.view(np.uint8).reshape(-1).copy()).to(dev)
    eng = U.TlsEngine(0, library=U.load_library(args.lib) if args.lib else None)
    eng.seal_records(src, ds, n * per, dk, nk, wire)
    recs = t.empty(n * per * 32, dtype=t.uint8, device=dev)
    res = t.empty(n * 64, dtype=t.uint8, device=dev)

    if args.chain:
        ws0 = np.zeros(n, U.STREAM_DT)  # fresh server connections (uvhttp_ws_stream_init)
        ws0["recv_buffer_size"] = 65536
        ws0["max_frame_size"], ws0["max_message_size"], ws0["is_server"] = 16 << 20, 64 << 20, 1
        ws_dev = t.from_numpy(ws0.view(np.uint8).reshape(-1).copy()).to(dev)
        read_end = t.zeros(n * per, dtype=t.int64, device=dev)
        wdesc = t.empty(n * 32, dtype=t.uint8, device=dev)
        wres = t.empty(n * U.STREAM_RESULT_BYTES, dtype=t.uint8, device=dev)
        weng.reserve(n, out.numel(), 0)

    def step():
        eng.open_records(wire, dk, nk, dst, n, n * per, out, records=recs, results=res)
        if args.chain:
            eng.ws_streams(res, recs, n, dst, out, ws_dev, read_end)
            weng.decode_streams(out, ws_dev, n, n, desc=wdesc, results=wres, read_end=read_end,
                                n_reads=n * per)

    for _ in range(args.warmup):
        step()
    t.cuda.synchronize()
    R = res.cpu().numpy().view(O.TLS_RESULT_DT)
    assert (R["n_delivered"] == per).all() and (R["plain_len"] == per * plen).all(), "open failed"
    if args.chain:
        # every connection: one message of fp bytes, unmasked in place inside `out`
        wr = weng.read_stream_results(wres, n)
        assert all(r.status == 0 and r.n_delivered == 1 and r.calls == per for r in wr[:64]), wr[0].as_dict()
        assert sum(r.n_delivered for r in wr) == n
        weng.sync()
    else:
        got = out.view(-1)[: per * plen]
        assert t.equal(got, src[: per * plen]), "plaintext mismatch"
    eng.set_timing(True)
    eng.kernel_time()
    t.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    t.cuda.synchronize()
    el = time.perf_counter() - t0
    kms, launches = eng.kernel_time()
    eng.set_timing(False)
    plain = n * per * plen
    kus = kms * 1e3 / max(1, launches)
    moved = n * per * (stride + plen)  # ciphertext records read + plaintext written
    if args.chain:
        plain = n * fp  # WebSocket payload delivered per step
    line = {
        "metric": ("TLS -> WebSocket chain GiB/s (ciphertext in HBM -> unmasked messages)"
                   if args.chain else "TLS record open GiB/s (device-resident)"),
        "value": round(plain * args.steps / el / GIB, 2),
        "unit": "GiB/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(el / args.steps * 1e3, 4), "higher_is_better": True,
        "dtype": "u8/u32 (ChaCha20-Poly1305)" if chacha else "u8/u32 (AES-GCM)", "data": "synthetic (random plaintext sealed on the device)",
        "config": {"workload": f"{n} connections x {per} x {plen} B TLS 1.{args.version % 10} "
                               f"{aead} records", "conns": n, "records": per,
                   "plen": plen},
        "kernel": {"name": "k_tls_open", "avg_us": round(kus, 2),
                   "plaintext_gbs": round(plain / (kus * 1e-6) / 1e9, 1),
                   "hbm_gbs": round(moved / (kus * 1e-6) / 1e9, 1), "launches": launches},
    }
    if args.lib:
        line["lib"] = os.path.basename(args.lib)
    if args.chain:
        line["config"]["chain"] = ("open_records -> ws_streams (one process_data call per record) "
                                   f"-> decode_reads; one {fp}-byte masked BINARY frame per connection")
    if not args.no_cpu_baseline and not args.chain:
        m = per  # connection 0's records (one key, sequence numbers 0 .. per-1)
        sample = wire[: m * stride].cpu().numpy()
        ob = np.zeros(m * stride, np.uint8)
        t1 = time.perf_counter()
        done = 0
        while time.perf_counter() - t1 < args.cpu_seconds:
            done += O.tls_open_stream_bytes(keys[0:1], 0, sample, ob)
        el1 = time.perf_counter() - t1
        line["cpu_baseline"] = {
            "oracle": {"value": round(done / el1 / GIB, 4), "unit": "GiB/s", "cores": 1,
                       "kind": "port", "sample": f"{m} records of connection 0, {el1:.1f} s"},
            "openssl": openssl_baseline(keys[0], 0, sample, m, rlen, ver, args.cpu_seconds, chacha),
        }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
