"""Generate tests/golden/tls_edge_vectors.json: directed TLS records for the branches that
random data never takes.

Uses only tests/_aead_ref.py (plain Python integers), a fixed seed, and no other input, so the
fixture is reproduced bit for bit (tests/test_aead_ref_host.py asserts it).

solved   ChaCha20-Poly1305 records in which one ciphertext block was solved for, so that the
         Poly1305 accumulator ends at a chosen value T = h mod p before the final reduction:
         with the AEAD's blocks m_0 .. m_{n-1} (AAD, ciphertext, lengths; all full, each with
         2^128 added), h = sum m_k r^(n-k) mod p, so for a block position i
             x = (T - sum_{k != i} m_k r^(n-k)) * r^-(n-i) mod p
         is a valid block when 2^128 <= x < 2^129 (about one nonce in four; the search takes
         the next sequence number until one fits, at most 64).  Targets: 0..4, p-1, p-2 (the
         accumulator may hold T or T + p: eight records each), 2^128 - 1, 2^128, 2^129,
         2^130 - 6, and values chosen against s: a tag of all zeros, of all ones, and a carry
         of h + s that ripples through all four words.  Solved positions: ciphertext block 0,
         1, 3, 4, 63, 64, 65 and the last one; TLS 1.3 records keep inner type 23 in the last
         byte (so a block other than the last is solved) and are delivered.
pattern  for all six key kinds, records whose *ciphertext* is all 0x00, all 0xff, or a single
         set bit (bit 0 or bit 127 of the first, second, 64th, 65th or last block), 16, 1024 and
         1040 bytes long, tag from the reference.  pattern_entry() makes the same records at
         any length for the tests that need long ones.

    python3 tests/golden/make_tls_edge_vectors.py        # rewrites the JSON
"""
import base64
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _aead_ref as R  # noqa: E402

OUT = os.path.join(HERE, "tls_edge_vectors.json")
SEED = 0x7157ED6E
P = R.P1305
MAX_NONCES = 64


def key_kinds():
    """AES-128-GCM, AES-256-GCM, ChaCha20-Poly1305 x TLS 1.3, TLS 1.2 (fixed keys)"""
    rng = random.Random(SEED ^ 0x6B65)
    return [{"name": "%s-%s" % (n, "13" if v == R.TLS13 else "12"), "key": rng.randbytes(kl),
             "iv": rng.randbytes(12), "version": v, "cipher": c}
            for n, kl, c in (("aes128", 16, R.AES_GCM), ("aes256", 32, R.AES_GCM),
                             ("chacha", 32, R.CHACHA))
            for v in (R.TLS13, R.TLS12)]


KINDS = key_kinds()


def entry(kind, seq, rec, why, **extra):
    """One fixture entry: the record, and what the reference says opening it gives."""
    k = kind
    status, type_, content = R.open_record(k["key"], k["iv"], k["version"], k["cipher"], seq, rec)
    ex = R.explicit_len(k["version"], k["cipher"])
    ct = rec[5 + ex:-16]
    pt = R._xor(ct, R.record_keystream(k["key"], k["iv"], k["version"], k["cipher"], seq, len(ct)))
    # how a seal reproduces the record: content || type || pad zero bytes (TLS 1.3)
    if k["version"] == R.TLS13:
        body = pt.rstrip(b"\0")
        seal_type, seal_pad = (body[-1], len(pt) - len(body)) if body else (None, None)
    else:
        seal_type, seal_pad = rec[0], 0
    e = {"kind": k["name"], "key": k["key"].hex(), "iv": k["iv"].hex(), "version": k["version"],
         "cipher": k["cipher"], "seq": seq, "record_b64": base64.b64encode(rec).decode(),
         "status": status, "type": type_, "content_len": len(content),
         "content_sha256": hashlib.sha256(content).hexdigest(),
         "seal_type": seal_type, "seal_pad": seal_pad, "why": why}
    e.update(extra)
    return e


# ---- solved Poly1305 vectors ---------------------------------------------------------------

M128 = (1 << 128) - 1
SMALL_TARGETS = [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("4", 4), ("p-1", P - 1), ("p-2", P - 2)]
SPECIAL_TARGETS = [
    ("2^128-1", lambda s: (1 << 128) - 1),
    ("2^128", lambda s: 1 << 128),
    ("2^129", lambda s: 1 << 129),
    ("2^130-6", lambda s: (1 << 130) - 6),
    ("tag all zeros: (2^128 - s) mod 2^128", lambda s: -s & M128),
    ("tag all ones: (2^128 - s - 1) mod 2^128", lambda s: (-s - 1) & M128),
    ("words ~s with the lowest one higher: the +1 carry of h + s ripples through all four "
     "words", lambda s: (s ^ M128) + 1),
    ("the same ripple with bit 129 of h set", lambda s: ((s ^ M128) + 1) % (1 << 128) + (1 << 129)),
]
# (ciphertext bytes, solved block) per version: block 0, 1, 3, 4, 63, 64, 65 and the last
COMBOS = {
    R.TLS12: [(16, 0), (64, 1), (64, 3), (80, 4), (1024, 63), (1040, 64), (1056, 65), (1056, 64)],
    R.TLS13: [(64, 0), (64, 1), (80, 3), (1024, 4), (1040, 63), (1056, 64), (1072, 65), (1024, 62)],
}


def solve(kind, seq0, n_ct, i, target, rng):
    """-> (seq, record, T): ciphertext block i solved so that h mod p = target(s)"""
    key, iv, version = kind["key"], kind["iv"], kind["version"]
    assert kind["cipher"] == R.CHACHA and n_ct % 16 == 0 and 16 * i < n_ct
    assert version == R.TLS12 or 16 * (i + 1) < n_ct  # TLS 1.3: the last block holds the type
    for seq in range(seq0, seq0 + MAX_NONCES):
        nonce = R.record_nonce(iv, version, R.CHACHA, seq)
        r, s = R.poly1305_key(R.chacha20_block(key, 0, nonce)[:32])
        if version == R.TLS13:
            inner = rng.randbytes(n_ct - 1) + b"\x17"
            ct = bytearray(R._xor(inner, R.aead_keystream(R.CHACHA, key, nonce, n_ct)))
            aad = bytes([23, 3, 3]) + (n_ct + 16).to_bytes(2, "big")
        else:
            ct = bytearray(rng.randbytes(n_ct))
            aad = seq.to_bytes(8, "big") + bytes([23, 3, 3]) + n_ct.to_bytes(2, "big")
        if r == 0:
            continue
        blocks = R.poly1305_blocks(R.chachapoly_mac_data(aad, bytes(ct)))
        n, pos = len(blocks), 1 + i
        T = target(s)
        assert 0 <= T < P
        rest = sum(m * pow(r, n - k, P) for k, m in enumerate(blocks) if k != pos) % P
        x = (T - rest) * pow(r, -(n - pos), P) % P
        if not (1 << 128) <= x < (1 << 129):
            continue
        ct[16 * i:16 * i + 16] = (x - (1 << 128)).to_bytes(16, "little")
        blocks = R.poly1305_blocks(R.chachapoly_mac_data(aad, bytes(ct)))
        assert R.poly1305_h(r, blocks) == T
        rec = R.record_from_ciphertext(key, iv, version, R.CHACHA, seq, 23, bytes(ct))
        assert int.from_bytes(rec[-16:], "little") == (T + s) % (1 << 128)
        return seq, rec, T
    raise AssertionError("no nonce in %d gave a valid block" % MAX_NONCES)


def solved_vectors():
    rng = random.Random(SEED)
    cc = {k["version"]: k for k in KINDS if k["cipher"] == R.CHACHA}
    out = []

    def add(label, target, version, n_ct, i):
        seq0 = 1000 + MAX_NONCES * len(out)
        seq, rec, T = solve(cc[version], seq0, n_ct, i, target, rng)
        e = entry(cc[version], seq, rec,
                  "Poly1305 accumulator ends at h mod p = %s (ciphertext block %d of %d solved)"
                  % (label, i, n_ct // 16), target=label, h_mod_p=hex(T), solved_block=i)
        assert e["status"] == R.REC_OK
        out.append(e)

    for t, (label, T) in enumerate(SMALL_TARGETS):
        for j in range(8):
            version = R.TLS12 if (j + t) % 2 == 0 else R.TLS13
            add(label, lambda s, T=T: T, version, *COMBOS[version][j])
    for t, (label, fn) in enumerate(SPECIAL_TARGETS):
        for j, version in enumerate((R.TLS12, R.TLS13)):
            add(label, fn, version, *COMBOS[version][(2 * t + j) % 8])
    return out


# ---- pattern records -----------------------------------------------------------------------


def pattern_names(n_ct):
    """the patterns of a ciphertext of n_ct bytes (a multiple of 16 for the single bits)"""
    names = ["zero", "ff"]
    nb = n_ct // 16
    for blk in sorted({b for b in (0, 1, 63, 64, nb - 1) if 0 <= b < nb}):
        names += ["bit0@%d" % blk, "bit127@%d" % blk]
    return names


def pattern_ciphertext(name, n_ct):
    if name == "zero":
        return bytes(n_ct)
    if name == "ff":
        return b"\xff" * n_ct
    bit, blk = name.split("@")
    ct = bytearray(n_ct)
    if bit == "bit0":
        ct[16 * int(blk)] = 0x01
    else:
        ct[16 * int(blk) + 15] = 0x80
    return bytes(ct)


def pattern_entry(kind, seq, name, n_ct):
    rec = R.record_from_ciphertext(kind["key"], kind["iv"], kind["version"], kind["cipher"], seq,
                                   23, pattern_ciphertext(name, n_ct))
    return entry(kind, seq, rec, "ciphertext pattern %s, %d bytes" % (name, n_ct),
                 pattern=name, ct_len=n_ct)


def pattern_vectors():
    out = []
    for kind in KINDS:
        for n_ct in (16, 1024, 1040):
            for name in pattern_names(n_ct):
                out.append(pattern_entry(kind, 500000 + len(out), name, n_ct))
    return out


def generate():
    return {"generator": "tests/golden/make_tls_edge_vectors.py", "seed": SEED,
            "solved": solved_vectors(), "pattern": pattern_vectors()}


def main():
    doc = generate()
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(OUT, len(doc["solved"]), "solved,", len(doc["pattern"]), "pattern")


if __name__ == "__main__":
    main()
