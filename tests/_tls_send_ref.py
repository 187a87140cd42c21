"""Reference of uvhttp_tls_gpu_seal_frames (include/uvhttp_tls_amd.h), in plain Python over the
CPU oracle: per send, per frame, the frame bytes are cut at max_fragment and every chunk is
sealed with tests/_oracle.py:tls_seal under seq, seq + 1, ... — what uvhttp_ws_send_frame's
mbedtls_ssl_write loop (src/uvhttp_websocket.c:543-575) puts on the wire for each frame.  Also
the numpy layouts of the three send-side structs and the expected results, summary and record
table."""
import numpy as np

import _oracle as O

TLS_SEND_DT = np.dtype([("seq", "<u8"), ("first_frame", "<u4"), ("n_frames", "<u4"),
                        ("key", "<u4"), ("type", "u1"), ("reserved", "u1", 3),
                        ("reserved2", "<u8")])
TLS_SEND_RESULT_DT = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("next_seq", "<u8"),
                               ("first_record", "<u4"), ("n_records", "<u4"), ("status", "<i4"),
                               ("reserved", "<u4"), ("plain_len", "<u8")])
TLS_SEND_SUMMARY_DT = np.dtype([("out_bytes", "<u8"), ("n_records", "<u4"), ("n_failed", "<u4"),
                                ("reserved", "<u8", 2)])
assert TLS_SEND_DT.itemsize == 32 and TLS_SEND_RESULT_DT.itemsize == 48
assert TLS_SEND_SUMMARY_DT.itemsize == 32

REC_RANGE = -8

# the six key kinds: (key_len, cipher, version)
KEY_KINDS = [(16, O.AES_GCM, O.TLS13), (32, O.AES_GCM, O.TLS13), (32, O.CHACHA, O.TLS13),
             (16, O.AES_GCM, O.TLS12), (32, O.AES_GCM, O.TLS12), (32, O.CHACHA, O.TLS12)]


def make_key(rng, kind):
    kl, cipher, version = kind
    return O.tls_key(rng.randbytes(kl), rng.randbytes(12), version, cipher)


def key_valid(k) -> bool:
    if k["version"] not in (O.TLS12, O.TLS13):
        return False
    if k["cipher"] == O.AES_GCM:
        return int(k["key_len"]) in (16, 32)
    return k["cipher"] == O.CHACHA and int(k["key_len"]) == 32


def overhead(k) -> int:
    """bytes a record adds to its content: header, TLS 1.2 AES-GCM explicit nonce, TLS 1.3 type
    byte, tag"""
    return 5 + 16 + (8 if k["version"] == O.TLS12 and k["cipher"] == O.AES_GCM else 0) + \
        (1 if k["version"] == O.TLS13 else 0)


def build_frames(payloads, mask=0, opcode=2, keys=None):
    """frames of tests/_oracle.py:build_frame back to back -> (bytes, offsets[n + 1])"""
    out, off = bytearray(), [0]
    for i, p in enumerate(payloads):
        rc, b = O.build_frame(p, opcode, mask, 1, keys[i] if keys else b"\0\0\0\0")
        assert rc == len(b)
        out += b
        off.append(len(out))
    return bytes(out), np.array(off, np.uint64)


def payload_len_for(total: int) -> int:
    """payload length of the server frame of `total` bytes (header 2 / 4 / 10)"""
    for hdr, lo, hi in ((2, 0, 125), (4, 126, 65535), (10, 65536, 1 << 62)):
        if lo <= total - hdr <= hi:
            return total - hdr
    raise ValueError(total)


def seal_frames_ref(frames: bytes, frame_off, sends, keys, max_fragment=0, max_records=None,
                    out_cap=None, frames_len=None):
    """-> dict(out=bytes, per_send=[bytes], plain=[bytes], results, summary, records)"""
    mf = max_fragment or 16384
    frames_len = len(frames) if frames_len is None else frames_len
    off = [int(x) for x in frame_off]
    n_total = len(off) - 1
    plans = []  # per send: (status, [(src_off, len)], overhead)
    for s in sends:
        key, ff, n = int(s["key"]), int(s["first_frame"]), int(s["n_frames"])
        if key >= len(keys) or key > 0xFFFF or not key_valid(keys[key]):
            plans.append((O.REC_KEY, [], 0))
            continue
        status, chunks = 0, []
        if ff + n > n_total:
            status = REC_RANGE
        else:
            for f in range(ff, ff + n):
                if off[f] > off[f + 1] or off[f + 1] > frames_len:
                    status = REC_RANGE
                    break
        if not status:
            for f in range(ff, ff + n):
                chunks += [(p, min(mf, off[f + 1] - p)) for p in range(off[f], off[f + 1], mf)]
        plans.append((status, chunks, overhead(keys[key])))
    need_rec = sum(len(c) for _, c, _ in plans)
    need_bytes = sum(sum(ln + ov for _, ln in c) for _, c, ov in plans)
    fail = (max_records is not None and need_rec > max_records) or \
        (out_cap is not None and need_bytes > out_cap)
    res = np.zeros(len(sends), TLS_SEND_RESULT_DT)
    summ = np.zeros(1, TLS_SEND_SUMMARY_DT)
    summ[0]["out_bytes"] = need_bytes
    summ[0]["n_records"] = min(need_rec, 0xFFFFFFFF)
    recs = np.zeros(0 if fail else need_rec, O.TLS_SEAL_DT)
    out, per_send, plain = bytearray(), [], []
    r = 0
    for i, (s, (status, chunks, ov)) in enumerate(zip(sends, plans)):
        res[i]["status"] = status
        res[i]["next_seq"] = s["seq"]
        if fail:
            if not status:
                res[i]["status"] = O.REC_CAPACITY
            per_send.append(b"")
            plain.append(b"")
            continue
        begin = len(out)
        res[i]["out_off"], res[i]["first_record"] = begin, r
        seq = int(s["seq"])
        for p, ln in chunks:
            recs[r] = (p, len(out), seq & 0xFFFFFFFFFFFFFFFF, ln, int(s["key"]), int(s["type"]), 0)
            out += O.tls_seal(keys[int(s["key"]):int(s["key"]) + 1], seq & 0xFFFFFFFFFFFFFFFF,
                              int(s["type"]), frames[p:p + ln])
            seq += 1
            r += 1
        res[i]["out_len"] = len(out) - begin
        res[i]["n_records"] = len(chunks)
        res[i]["next_seq"] = seq & 0xFFFFFFFFFFFFFFFF
        res[i]["plain_len"] = sum(ln for _, ln in chunks)
        per_send.append(bytes(out[begin:]))
        plain.append(b"".join(frames[p:p + ln] for p, ln in chunks))
    assert fail or len(out) == need_bytes
    summ[0]["n_failed"] = len(sends) if fail else int((res["status"] != 0).sum())
    return {"out": bytes(out), "per_send": per_send, "plain": plain, "results": res,
            "summary": summ, "records": recs, "failed": fail}
