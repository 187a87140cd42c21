"""Writes tests/golden/reference_transcripts.json: a fixed subset of the sessions of
tests/_reference.py, run through the reference's own WebSocket unit (oracle/_ref/libws_ref.so,
built by oracle/ref.mk from the reference tree), recorded as data.  Needs that library;
tests/test_reference_diff.py re-runs render() and compares it with the committed file.

Selection, in a fixed order: sessions 0 .. N_SESSIONS - 1, each under its three cuts ("one": one
read, "frame": a read per frame, "cuts": seeded cuts).  A (session, cut) is taken while it shows a
branch (on its side) that fewer than PER_BRANCH entries show so far; then sessions are added in
seed order, session s under cut s mod 3, until there are N_ENTRIES.  The file records how many
entries show each branch.

An entry:
  seed, mode      the session of tests/_reference.make_session and its cut
  config          is_server, max_frame_size / max_message_size (null: a NULL config, the
                  reference's defaults), wired (user_data leads to a server context), echo (the
                  on_message hook sends the message back), key_seed
  wire            the bytes fed, as segments: a hex string, or {"g": [seed, n], "k": hex key} =
                  gen_bytes(seed, n) XORed with the 4-byte key ("" = as it is).  gen_bytes: byte i is
                  (x >> 8) & 0xFF of x = mix((seed * 0x9E3779B1 + i * 0x85EBCA6B) mod 2^32) with
                  mix(x): x ^= x >> 15; x = x * 0x2C1B3C6D mod 2^32; x ^= x >> 12.  Payloads of 4 KiB
                  and more are stored this way.
  reads           the length of every read, in order (they add up to the wire)
  keys            the driver's key sequence as far as the session drew from it: 32-bit words, a
                  frame's key bytes low first (word i = splitmix64(key_seed + (i + 1) * golden
                  gamma) >> 16, the driver's ws_ref_key_word); empty for a server
  results         per process_data call made (calls stop at the first failure):
                  [return code, recv_buffer_pos, recv_buffer_size, events so far]
  events          ["m", opcode, hex] on_message, ["c", code] on_close, ["s", hex] a frame handed to
                  the socket; a field of 4 KiB and more is {"n": length, "sha256": digest}
  end             state, recv_buffer_pos, recv_buffer_size, fragmented_size, fragmented_opcode,
                  fragmented_message == NULL, frames_sent
  branches        the branches of tests/_reference.BRANCHES this entry shows"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _reference as RF  # noqa: E402

N_ENTRIES = 320
PER_BRANCH = 2
MODES = ("one", "frame", "cuts")
OUT = os.path.join(HERE, "reference_transcripts.json")


def _field(b):
    if len(b) >= RF.BIG:
        return {"n": len(b), "sha256": hashlib.sha256(b).hexdigest()}
    return b.hex()


def _segments(sess):
    out = []
    for f in sess.frames:
        if f.gen and len(f.payload) >= RF.BIG:
            out += [f.head.hex(), {"g": list(f.gen), "k": f.key.hex() if f.masked else ""}]
        elif out and isinstance(out[-1], str):
            out[-1] += f.bytes.hex()
        else:
            out.append(f.bytes.hex())
    return out


def entry(sess, mode, tr, took):
    sent = tr["end"][6]
    return {"seed": sess.seed, "mode": mode, "config": sess.config(), "wire": _segments(sess),
            "reads": [len(r) for r in sess.reads(mode)],
            "keys": [] if sess.is_server else [RF.key_word(sess.key_seed, i) for i in range(sent)],
            "results": [list(r) for r in tr["reads"]],
            "events": [[_field(x) if isinstance(x, bytes) else x for x in e] for e in tr["events"]],
            "end": list(tr["end"]), "branches": sorted(took)}


def select():
    counts = {key: 0 for key in RF.required()}
    chosen, entries = set(), []

    def run(seed, mode):
        sess = RF.make_session(seed)
        tr = RF.run_reference(sess, sess.reads(mode))
        return sess, tr, RF.branches_taken(sess, {mode: tr})

    def take(sess, mode, tr, took):
        chosen.add((sess.seed, mode))
        entries.append(entry(sess, mode, tr, took))
        for b in took:
            if (b, sess.side) in counts:
                counts[(b, sess.side)] += 1

    for seed in range(RF.N_SESSIONS):
        if all(v >= PER_BRANCH for v in counts.values()):
            break
        for mode in MODES:
            sess, tr, took = run(seed, mode)
            if any(counts.get((b, sess.side), PER_BRANCH) < PER_BRANCH for b in took):
                take(sess, mode, tr, took)
    seed = 0
    while len(entries) < N_ENTRIES:
        mode = MODES[seed % 3]
        if (seed, mode) not in chosen:
            sess, tr, took = run(seed, mode)
            take(sess, mode, tr, took)
        seed += 1
    entries.sort(key=lambda e: (e["seed"], MODES.index(e["mode"])))
    return entries, counts


def render() -> bytes:
    entries, counts = select()
    head = {"source": "uvhttp_ws_process_data of the reference's src/uvhttp_websocket.c, run by oracle/ref_driver.c",
            "format": "tests/golden/make_reference_transcripts.py",
            "branch_counts": {"%s/%s" % k: v for k, v in sorted(counts.items())}}
    body = ",\n".join(json.dumps(e, separators=(",", ":")) for e in entries)
    text = json.dumps(head, indent=1)[:-2] + ',\n "sessions": [\n' + body + "\n]}\n"
    return text.encode()


if __name__ == "__main__":
    if RF.load_ref() is None:
        sys.exit("oracle/_ref/libws_ref.so is not built (make -C oracle, with the reference tree at hand)")
    data = render()
    json.loads(data)
    with open(OUT, "wb") as f:
        f.write(data)
    print("%s: %d bytes" % (OUT, len(data)))
