"""Reference of uvhttp_tls_gpu_seal_parts_coalesced (include/uvhttp_tls_amd.h): a send's stream is
its parts' runs back to back (tests/_tls_parts_ref.py:concat lays them out), cut into
ceil(B / max_fragment) records of max_fragment content bytes but the last, each sealed by the CPU
oracle (tests/_oracle.py:tls_seal) under seq, seq + 1, ...  Frame boundaries play no part.  The
failure order (key, then range) and the capacity rule are seal_frames'.

records[r].src_off = out_off + 5 + the key's explicit-nonce length: where the content lies in out
before it is sealed in place."""
import numpy as np

import _oracle as O
import _tls_send_ref as R
from _tls_parts_ref import concat


def header_len(k) -> int:
    """bytes of a record before its content: header, TLS 1.2 AES-GCM explicit nonce"""
    return 5 + (8 if k["version"] == O.TLS12 and k["cipher"] == O.AES_GCM else 0)


def streams_of(frames: bytes, parts, sends, keys):
    """-> per send (status, stream bytes); a failed send has an empty stream"""
    cat, cat_off, cs, _ = concat(frames, parts, sends)
    n_total = len(cat_off) - 1
    rows = []
    for s, c in zip(sends, cs):
        key = int(s["key"])
        ff, n = int(c["first_frame"]), int(c["n_frames"])
        if key >= len(keys) or key > 0xFFFF or not R.key_valid(keys[key]):
            rows.append((O.REC_KEY, b""))
        elif ff + n > n_total:
            rows.append((R.REC_RANGE, b""))
        else:
            rows.append((0, cat[int(cat_off[ff]):int(cat_off[ff + n])]))
    return rows


def seal_parts_coalesced_ref(frames: bytes, parts, sends, keys, max_fragment=0, max_records=None,
                             out_cap=None):
    """-> dict(out, per_send, plain (the streams), results, summary, records, failed), the layout of
    tests/_tls_send_ref.py:seal_frames_ref"""
    mf = max_fragment or 16384
    rows = streams_of(frames, parts, sends, keys)
    n_rec = [(len(b) + mf - 1) // mf for _, b in rows]
    over = [R.overhead(keys[int(s["key"])]) if st == 0 else 0 for s, (st, _) in zip(sends, rows)]
    need_rec = sum(n_rec)
    need_bytes = sum(len(b) + n * ov for (_, b), n, ov in zip(rows, n_rec, over))
    fail = (max_records is not None and need_rec > max_records) or \
        (out_cap is not None and need_bytes > out_cap)
    res = np.zeros(len(sends), R.TLS_SEND_RESULT_DT)
    summ = np.zeros(1, R.TLS_SEND_SUMMARY_DT)
    summ[0]["out_bytes"] = need_bytes
    summ[0]["n_records"] = min(need_rec, 0xFFFFFFFF)
    recs = np.zeros(0 if fail else need_rec, O.TLS_SEAL_DT)
    out, per_send, plain = bytearray(), [], []
    r = 0
    for i, (s, (status, stream)) in enumerate(zip(sends, rows)):
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
        seq, key = int(s["seq"]), int(s["key"])
        for cut in range(0, len(stream), mf):
            chunk = stream[cut:cut + mf]
            recs[r] = (len(out) + header_len(keys[key]), len(out), seq & 0xFFFFFFFFFFFFFFFF, len(chunk), key,
                       int(s["type"]), 0)
            out += O.tls_seal(keys[key:key + 1], seq & 0xFFFFFFFFFFFFFFFF, int(s["type"]), chunk)
            seq += 1
            r += 1
        res[i]["out_len"] = len(out) - begin
        res[i]["n_records"] = n_rec[i]
        res[i]["next_seq"] = seq & 0xFFFFFFFFFFFFFFFF
        res[i]["plain_len"] = len(stream)
        per_send.append(bytes(out[begin:]))
        plain.append(stream)
    assert fail or (len(out) == need_bytes and r == need_rec)
    summ[0]["n_failed"] = len(sends) if fail else int((res["status"] != 0).sum())
    return {"out": bytes(out), "per_send": per_send, "plain": plain, "results": res, "summary": summ,
            "records": recs, "failed": fail}
