"""An independent reference of the TLS record crypto, for the tests only.

Everything is written from the specifications on plain Python integers (numpy only to run the
ChaCha20 and AES block functions over many counters at once); it shares no code with oracle/
and does not use the C bindings of tests/_oracle.py:

  Poly1305          RFC 8439 §2.5: h = (h + block) * r mod 2^130 - 5 on Python ints, no limbs
  ChaCha20          RFC 8439 §2.3
  AES-128 / -256    FIPS-197, the S-box computed from the GF(2^8) inverse and the affine map
  GHASH, GCM        SP 800-38D Algorithm 1 (bit-serial multiply), Algorithms 2 and 4, 96-bit IV
  AEAD_CHACHA20_POLY1305   RFC 8439 §2.8
  TLS records       the header comment of include/uvhttp_tls_amd.h (RFC 8446 §5.2-5.3,
                    RFC 5288 §3, RFC 7905 §2)
"""
import numpy as np

TLS12, TLS13 = 0x0303, 0x0304
AES_GCM, CHACHA = 0, 1
REC_OK, REC_CONTROL, REC_BAD_MAC, REC_EMPTY = 0, 3, -2, -5

P1305 = (1 << 130) - 5

# ---- Poly1305 ----------------------------------------------------------------------------


def poly1305_key(key32: bytes):
    """(r, s) of a 32-byte one-time key, r clamped"""
    r = int.from_bytes(key32[:16], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
    return r, int.from_bytes(key32[16:32], "little")


def poly1305_blocks(msg: bytes):
    """the message's blocks as integers, each with its 2^(8 len) bit"""
    return [int.from_bytes(msg[i:i + 16], "little") + (1 << (8 * len(msg[i:i + 16])))
            for i in range(0, len(msg), 16)]


def poly1305_h(r: int, blocks) -> int:
    h = 0
    for b in blocks:
        h = (h + b) * r % P1305
    return h


def poly1305(key32: bytes, msg: bytes) -> bytes:
    r, s = poly1305_key(key32)
    return ((poly1305_h(r, poly1305_blocks(msg)) + s) % (1 << 128)).to_bytes(16, "little")


# ---- ChaCha20 ----------------------------------------------------------------------------


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def chacha20_blocks(key: bytes, counter: int, nonce: bytes, n: int) -> bytes:
    """n consecutive 64-byte keystream blocks from `counter` on (one column per counter)"""
    n = max(n, 1)
    st = np.empty((16, n), np.uint32)
    st[0:4] = np.array([0x61707865, 0x3320646e, 0x79622d32, 0x6b206574], np.uint32)[:, None]
    st[4:12] = np.frombuffer(key, "<u4").astype(np.uint32)[:, None]
    st[12] = ((counter + np.arange(n, dtype=np.uint64)) & np.uint64(0xffffffff)).astype(np.uint32)
    st[13:16] = np.frombuffer(nonce, "<u4").astype(np.uint32)[:, None]
    x = st.copy()

    def qr(a, b, c, d):
        x[a] += x[b]
        x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]
        x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]
        x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]
        x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    x += st
    return np.ascontiguousarray(x.T).astype("<u4").tobytes()


def chacha20_block(key: bytes, counter: int, nonce: bytes) -> bytes:
    return chacha20_blocks(key, counter, nonce, 1)


# ---- AES ---------------------------------------------------------------------------------


def _gf8_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = (a << 1) ^ (0x11b if a & 0x80 else 0)
        b >>= 1
    return r


def _make_sbox():
    box = []
    for x in range(256):
        inv = 0
        if x:
            inv = x
            for _ in range(253):  # x^254 = x^-1 in GF(2^8)
                inv = _gf8_mul(inv, x)
        y = 0x63
        for k in range(5):  # b ^ rotl(b, 1..4) ^ 0x63
            y ^= ((inv << k) | (inv >> (8 - k))) & 0xff
        box.append(y)
    return box


SBOX = _make_sbox()
_SBOX_NP = np.array(SBOX, np.uint8)
# ShiftRows on the column-major state: byte 4 c + r comes from column (c + r) mod 4
_SHIFT = np.array([4 * ((c + r) % 4) + r for c in range(4) for r in range(4)])


def aes_expand_key(key: bytes):
    """FIPS-197 §5.2 -> round keys, 16 bytes each"""
    nk = len(key) // 4
    assert nk in (4, 8)
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _gf8_mul(rcon, 2)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return [np.array(sum(w[4 * r:4 * r + 4], []), np.uint8) for r in range(nr + 1)]


def _xtime(a):
    return ((a << 1) & 0xff).astype(np.uint8) ^ (np.uint8(0x1b) * (a >> 7))


def aes_encrypt_blocks(key: bytes, blocks: np.ndarray) -> np.ndarray:
    """FIPS-197 §5.1 on an (n, 16) uint8 array of blocks"""
    rk = aes_expand_key(key)
    s = blocks.astype(np.uint8) ^ rk[0]
    for rnd in range(1, len(rk)):
        s = _SBOX_NP[s][:, _SHIFT]
        if rnd != len(rk) - 1:
            c = s.reshape(-1, 4, 4)  # [block, column, row]
            a0, a1, a2, a3 = c[:, :, 0], c[:, :, 1], c[:, :, 2], c[:, :, 3]
            m = np.stack([_xtime(a0) ^ _xtime(a1) ^ a1 ^ a2 ^ a3,
                          a0 ^ _xtime(a1) ^ _xtime(a2) ^ a2 ^ a3,
                          a0 ^ a1 ^ _xtime(a2) ^ _xtime(a3) ^ a3,
                          _xtime(a0) ^ a0 ^ a1 ^ a2 ^ _xtime(a3)], axis=2)
            s = m.reshape(-1, 16)
        s = s ^ rk[rnd]
    return s


def aes_encrypt_block(key: bytes, block: bytes) -> bytes:
    return aes_encrypt_blocks(key, np.frombuffer(block, np.uint8).reshape(1, 16)).tobytes()


# ---- GHASH and GCM -----------------------------------------------------------------------

_R = 0xe1 << 120


def gf128_mul(x: int, y: int) -> int:
    """SP 800-38D Algorithm 1; blocks as big-endian integers (bit 0 of the text = bit 127)"""
    z, v = 0, y
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= v
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    return z


def _pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def ghash(h: int, data: bytes) -> int:
    y = 0
    for i in range(0, len(data), 16):
        y = gf128_mul(y ^ int.from_bytes(data[i:i + 16], "big"), h)
    return y


def _gcm_ctr(key: bytes, iv: bytes, first: int, n: int) -> np.ndarray:
    """E(K, iv || be32(first + i)), i < n"""
    blk = np.zeros((max(n, 1), 16), np.uint8)
    blk[:, :12] = np.frombuffer(iv, np.uint8)
    ctr = (first + np.arange(max(n, 1), dtype=np.uint64)) & np.uint64(0xffffffff)
    blk[:, 12:] = ctr.astype(">u4").view(np.uint8).reshape(-1, 4)
    return aes_encrypt_blocks(key, blk)


def gcm_keystream(key: bytes, iv: bytes, n: int) -> bytes:
    assert len(iv) == 12
    return _gcm_ctr(key, iv, 2, (n + 15) // 16).tobytes()[:n]


def gcm_tag(key: bytes, iv: bytes, aad: bytes, ct: bytes) -> bytes:
    assert len(iv) == 12
    h = int.from_bytes(aes_encrypt_block(key, bytes(16)), "big")
    s = ghash(h, _pad16(aad) + _pad16(ct) + (8 * len(aad)).to_bytes(8, "big")
              + (8 * len(ct)).to_bytes(8, "big"))
    return (s ^ int.from_bytes(_gcm_ctr(key, iv, 1, 1).tobytes(), "big")).to_bytes(16, "big")


# ---- the two AEADs -----------------------------------------------------------------------


def _xor(a: bytes, b: bytes) -> bytes:
    return (np.frombuffer(a, np.uint8) ^ np.frombuffer(b[:len(a)], np.uint8)).tobytes()


def chachapoly_mac_data(aad: bytes, ct: bytes) -> bytes:
    return (_pad16(aad) + _pad16(ct) + len(aad).to_bytes(8, "little")
            + len(ct).to_bytes(8, "little"))


def aead_keystream(cipher, key: bytes, nonce: bytes, n: int) -> bytes:
    if cipher == CHACHA:
        return chacha20_blocks(key, 1, nonce, (n + 63) // 64)[:n]
    return gcm_keystream(key, nonce, n)


def aead_tag(cipher, key: bytes, nonce: bytes, aad: bytes, ct: bytes) -> bytes:
    if cipher == CHACHA:
        return poly1305(chacha20_block(key, 0, nonce)[:32], chachapoly_mac_data(aad, ct))
    return gcm_tag(key, nonce, aad, ct)


def aead_seal(cipher, key, nonce, aad, pt):
    ct = _xor(pt, aead_keystream(cipher, key, nonce, len(pt)))
    return ct, aead_tag(cipher, key, nonce, aad, ct)


def aead_open(cipher, key, nonce, aad, ct, tag):
    """-> plaintext, or None when the tag does not match"""
    if aead_tag(cipher, key, nonce, aad, ct) != tag:
        return None
    return _xor(ct, aead_keystream(cipher, key, nonce, len(ct)))


# ---- TLS records -------------------------------------------------------------------------


def explicit_len(version, cipher):
    return 8 if version == TLS12 and cipher == AES_GCM else 0


def record_nonce(iv: bytes, version, cipher, seq, explicit: bytes = b"") -> bytes:
    if explicit_len(version, cipher):
        return iv[:4] + explicit
    return _xor(iv, bytes(4) + seq.to_bytes(8, "big"))


def record_from_ciphertext(key, iv, version, cipher, seq, type_, ct: bytes) -> bytes:
    """The wire record whose AEAD ciphertext is `ct` as given, with its tag: outer type 23 for
    TLS 1.3, `type_` for TLS 1.2; the TLS 1.2 AES-GCM explicit nonce is be64(seq)."""
    ex = seq.to_bytes(8, "big") if explicit_len(version, cipher) else b""
    n = len(ex) + len(ct) + 16
    assert n <= 0xffff
    if version == TLS13:
        hdr = bytes([23, 3, 3]) + n.to_bytes(2, "big")
        aad = hdr
    else:
        hdr = bytes([type_, 3, 3]) + n.to_bytes(2, "big")
        aad = seq.to_bytes(8, "big") + bytes([type_, 3, 3]) + len(ct).to_bytes(2, "big")
    nonce = record_nonce(iv, version, cipher, seq, ex)
    return hdr + ex + ct + aead_tag(cipher, key, nonce, aad, ct)


def record_keystream(key, iv, version, cipher, seq, n) -> bytes:
    """keystream under the record's ciphertext (explicit nonce be64(seq) for TLS 1.2 AES-GCM)"""
    ex = seq.to_bytes(8, "big") if explicit_len(version, cipher) else b""
    return aead_keystream(cipher, key, record_nonce(iv, version, cipher, seq, ex), n)


def seal_record(key, iv, version, cipher, seq, type_, content: bytes, pad=0) -> bytes:
    inner = content + bytes([type_]) + bytes(pad) if version == TLS13 else content
    ct = _xor(inner, record_keystream(key, iv, version, cipher, seq, len(inner)))
    return record_from_ciphertext(key, iv, version, cipher, seq, type_, ct)


def open_record(key, iv, version, cipher, seq, rec: bytes):
    """One complete record whose header passed the walk's checks -> (status, type, content)"""
    ex_n = explicit_len(version, cipher)
    n = int.from_bytes(rec[3:5], "big")
    assert len(rec) == 5 + n and n >= ex_n + 16
    ex, ct, tag = rec[5:5 + ex_n], rec[5 + ex_n:len(rec) - 16], rec[-16:]
    if version == TLS13:
        aad = rec[:5]
    else:
        aad = seq.to_bytes(8, "big") + bytes([rec[0], 3, 3]) + len(ct).to_bytes(2, "big")
    pt = aead_open(cipher, key, record_nonce(iv, version, cipher, seq, ex), aad, ct, tag)
    if pt is None:
        return REC_BAD_MAC, 0, b""
    type_ = rec[0]
    if version == TLS13:
        pt = pt.rstrip(b"\0")
        if not pt:
            return REC_EMPTY, 0, b""
        type_, pt = pt[-1], pt[:-1]
    return (REC_OK if type_ == 23 else REC_CONTROL), type_, pt


def split_records(wire: bytes):
    """the complete records of a connection's bytes"""
    out, pos = [], 0
    while len(wire) - pos >= 5:
        n = int.from_bytes(wire[pos + 3:pos + 5], "big")
        if len(wire) - pos - 5 < n:
            break
        out.append(wire[pos:pos + 5 + n])
        pos += 5 + n
    return out
