"""Reference of uvhttp_tls_gpu_seal_parts (include/uvhttp_tls_amd.h): a send is part 0's run, then
part 1's run, ...; so the parts' runs are concatenated into one frame list per send, the frames
copied back to back into one buffer, and tests/_tls_send_ref.py:seal_frames_ref does the rest.
Only the record table's src_off is put back to where the frame lies in the arena.

A part here is a dict: base, len, off (numpy uint64 [n_frames + 1], relative to base) and runs
(numpy uint32 [n_sends, 2]: first_frame, n_frames)."""
import numpy as np

import _tls_send_ref as R


def part(base, length, off, runs):
    return {"base": int(base), "len": int(length), "off": np.asarray(off, np.uint64),
            "runs": np.asarray(runs, np.uint32).reshape(-1, 2)}


def concat(frames: bytes, parts, sends):
    """-> (cat bytes, cat_off, cat_sends, origin): every send's frames back to back in a buffer of
    their own, the frame table and send table over it that uvhttp_tls_gpu_seal_frames would take, and
    per frame of that table where it starts in `frames`.  A send whose run is out of range in some
    part names a frame range past the table (seal_frames' ERR_RANGE)."""
    cat, off, origin = bytearray(), [0], []
    rows = []
    for s in range(len(sends)):
        lst, bad = [], False
        for p in parts:
            first, n = int(p["runs"][s][0]), int(p["runs"][s][1])
            o = [int(x) for x in p["off"]]
            if first + n > len(o) - 1:
                bad = True
                break
            for f in range(first, first + n):
                if o[f] > o[f + 1] or o[f + 1] > p["len"]:
                    bad = True
                    break
                lst.append((p["base"] + o[f], o[f + 1] - o[f]))
            if bad:
                break
        if bad:
            rows.append(None)
            continue
        rows.append((len(off) - 1, len(lst)))
        for a, ln in lst:
            cat += frames[a:a + ln]
            assert len(frames[a:a + ln]) == ln
            off.append(len(cat))
            origin.append(a)
    n_total = len(off) - 1
    cs = np.array(sends, R.TLS_SEND_DT)
    for s, row in enumerate(rows):
        cs[s]["first_frame"], cs[s]["n_frames"] = row if row is not None else (n_total + 1, 1)
    return bytes(cat), np.array(off, np.uint64), cs, origin


def seal_parts_ref(frames: bytes, parts, sends, keys, max_fragment=0, max_records=None, out_cap=None):
    """-> seal_frames_ref's dict (out, per_send, plain, results, summary, records, failed), the
    records' src_off pointing into `frames`, plus cat / cat_off / cat_sends (concat above)."""
    cat, cat_off, cs, origin = concat(frames, parts, sends)
    ref = R.seal_frames_ref(cat, cat_off, cs, keys, max_fragment, max_records, out_cap)
    mf = max_fragment or 16384
    if not ref["failed"]:
        r = 0
        for s, res in zip(cs, ref["results"]):
            if res["status"] != 0:
                continue
            for f in range(int(s["first_frame"]), int(s["first_frame"]) + int(s["n_frames"])):
                for cut in range(0, int(cat_off[f + 1] - cat_off[f]), mf):
                    assert int(ref["records"][r]["src_off"]) == int(cat_off[f]) + cut
                    ref["records"][r]["src_off"] = origin[f] + cut
                    r += 1
        assert r == len(ref["records"])
    ref.update(cat=cat, cat_off=cat_off, cat_sends=cs)
    return ref
