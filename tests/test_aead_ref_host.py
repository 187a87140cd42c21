"""CPU checks that tie the TLS oracle (oracle/tls_oracle.c) to an independent reference on plain
Python integers (tests/_aead_ref.py).

The reference is pinned first: the published vectors of tests/golden/tls_known_answers.json
and the seven OpenSSL sessions.  Then the oracle's seal must equal the reference's byte for
byte, and the oracle must open the directed vectors of tests/golden/tls_edge_vectors.json —
Poly1305 accumulators solved to end at 0..4, p-1, p-2, 2^128.., a tag of all zeros / ones, a
full ripple carry of h + s; all-0x00 / all-0xff / single-bit ciphertexts — to the status and
content the reference predicts.  These are the value-dependent branches (the final "subtract
p", the h + s carry chain) that random data takes with probability about 2^-128.
"""
import base64
import hashlib
import importlib.util
import json
import os
import random

import numpy as np
import pytest

import _aead_ref as R
import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _json(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_tls_edge_vectors", os.path.join(GOLD, "make_tls_edge_vectors.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen():
    return _generator()


@pytest.fixture(scope="module")
def vectors():
    return _json("tls_edge_vectors.json")


def _key(e):
    return O.tls_key(bytes.fromhex(e["key"]), bytes.fromhex(e["iv"]), e["version"], e["cipher"])


# ---- the reference against published vectors and OpenSSL -----------------------------------


def test_reference_known_answers():
    ka = _json("tls_known_answers.json")
    for c in ka["aes"]:
        assert R.aes_encrypt_block(bytes.fromhex(c["key"]), bytes.fromhex(c["pt"])).hex() == c["ct"], c["id"]
    for x, y in ka["sbox"].items():
        assert R.SBOX[int(x, 16)] == int(y, 16)
    assert sorted(R.SBOX) == list(range(256))
    for c in ka["gcm"]:
        k, iv, aad, pt = (bytes.fromhex(c[n]) for n in ("key", "iv", "aad", "pt"))
        ct, tag = R.aead_seal(R.AES_GCM, k, iv, aad, pt)
        assert (ct.hex(), tag.hex()) == (c["ct"], c["tag"]), c["id"]
        assert R.aead_open(R.AES_GCM, k, iv, aad, ct, tag) == pt
        assert R.aead_open(R.AES_GCM, k, iv, aad, ct, bytes([tag[0] ^ 1]) + tag[1:]) is None
    for c in ka["chacha20_block"]:
        assert R.chacha20_block(bytes.fromhex(c["key"]), c["counter"],
                                bytes.fromhex(c["nonce"])).hex() == c["out"], c["id"]
    for c in ka["poly1305"]:
        assert R.poly1305(bytes.fromhex(c["key"]), bytes.fromhex(c["msg"])).hex() == c["tag"], c["id"]
    for c in ka["chachapoly"]:
        k, n, aad, pt = (bytes.fromhex(c[x]) for x in ("key", "nonce", "aad", "pt"))
        ct, tag = R.aead_seal(R.CHACHA, k, n, aad, pt)
        assert (ct.hex(), tag.hex()) == (c["ct"], c["tag"]), c["id"]
        assert R.aead_open(R.CHACHA, k, n, aad, ct, tag) == pt
        assert R.aead_open(R.CHACHA, k, n, aad, ct, bytes([tag[0] ^ 4]) + tag[1:]) is None


@pytest.mark.parametrize("idx", range(7))
def test_reference_opens_openssl_sessions(idx):
    s = _json("tls_openssl_records.json")["sessions"][idx]
    key, iv = bytes.fromhex(s["key"]), bytes.fromhex(s["iv"]).ljust(12, b"\0")
    got, stop = b"", None
    for j, rec in enumerate(R.split_records(base64.b64decode(s["wire_b64"]))):
        status, type_, content = R.open_record(key, iv, s["version"], s.get("cipher", 0),
                                               s["seq"] + j, rec)
        if status != R.REC_OK:
            stop = (status, type_)
            break
        got += content
    assert stop == (R.REC_CONTROL, s["stop_type"])
    assert len(got) == s["plaintext_len"]
    assert hashlib.sha256(got).hexdigest() == s["plaintext_sha256"]


# ---- the fixture ---------------------------------------------------------------------------


def test_fixture_is_reproduced(gen, vectors):
    """the generator rewrites the fixture bit for bit (solved and pattern sections)"""
    doc = json.loads(json.dumps(gen.generate()))
    assert doc["solved"] == vectors["solved"]
    assert doc["pattern"] == vectors["pattern"]
    assert doc == vectors


def test_solved_vectors_cover_the_targets(vectors):
    sv = vectors["solved"]
    by = {}
    for e in sv:
        by.setdefault(e["target"], []).append(e)
    p = R.P1305
    for label, T in [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("4", 4), ("p-1", p - 1), ("p-2", p - 2)]:
        assert len(by[label]) == 8 and all(int(e["h_mod_p"], 16) == T for e in by[label])
    for label, T in [("2^128-1", (1 << 128) - 1), ("2^128", 1 << 128), ("2^129", 1 << 129),
                     ("2^130-6", (1 << 130) - 6)]:
        assert all(int(e["h_mod_p"], 16) == T for e in by[label]) and by[label]
    def tags(prefix):
        return {base64.b64decode(e["record_b64"])[-16:] for e in sv if e["target"].startswith(prefix)}
    assert tags("tag all zeros") == {bytes(16)} and tags("words ~s") == {bytes(16)}
    assert tags("tag all ones") == {b"\xff" * 16}
    assert {e["solved_block"] for e in sv} >= {0, 1, 3, 4, 63, 64, 65}
    assert {e["version"] for e in sv} == {R.TLS12, R.TLS13}
    # every solved record authenticates under the definition, with the accumulator at T
    for e in sv:
        rec = base64.b64decode(e["record_b64"])
        key, iv = bytes.fromhex(e["key"]), bytes.fromhex(e["iv"])
        ct = rec[5:-16]
        aad = rec[:5] if e["version"] == R.TLS13 else \
            e["seq"].to_bytes(8, "big") + rec[:3] + len(ct).to_bytes(2, "big")
        otk = R.chacha20_block(key, 0, R.record_nonce(iv, e["version"], R.CHACHA, e["seq"]))
        r, s = R.poly1305_key(otk[:32])
        h = R.poly1305_h(r, R.poly1305_blocks(R.chachapoly_mac_data(aad, ct)))
        assert h == int(e["h_mod_p"], 16)
        assert (h + s) % (1 << 128) == int.from_bytes(rec[-16:], "little")


# ---- the oracle against the reference ------------------------------------------------------


def _oracle_open_one(e, rec=None):
    rec = base64.b64decode(e["record_b64"]) if rec is None else rec
    st = np.zeros(1, O.TLS_STREAM_DT)
    st[0]["len"], st[0]["seq"] = len(rec), e["seq"]
    recs, res, out = O.tls_open_batch(np.frombuffer(rec, np.uint8), _key(e), st)
    assert len(recs) == 1
    r = recs[0]
    content = out[int(res[0]["out_off"]):int(res[0]["out_off"]) + int(res[0]["plain_len"])].tobytes()
    return int(r["status"]), int(r["type"]), int(r["content_len"]), content


@pytest.mark.parametrize("section", ["solved", "pattern"])
def test_oracle_opens_directed_vectors(vectors, section):
    for i, e in enumerate(vectors[section]):
        status, type_, clen, content = _oracle_open_one(e)
        assert (status, type_, clen) == (e["status"], e["type"], e["content_len"]), (i, e["why"])
        if status == O.REC_OK:
            assert hashlib.sha256(content).hexdigest() == e["content_sha256"], (i, e["why"])
        rec = bytearray(base64.b64decode(e["record_b64"]))
        rec[-1] ^= 0x80  # a tag bit
        assert _oracle_open_one(e, bytes(rec))[0] == O.REC_BAD_MAC, (i, e["why"])
        rec[-1] ^= 0x80
        rec[-17] ^= 0x01  # a ciphertext bit
        assert _oracle_open_one(e, bytes(rec))[0] == O.REC_BAD_MAC, (i, e["why"])


@pytest.mark.parametrize("section", ["solved", "pattern"])
def test_oracle_seals_directed_vectors(vectors, section):
    """the oracle's seal of a vector's plaintext gives the fixture's wire bytes"""
    n = 0
    for i, e in enumerate(vectors[section]):
        if e["seal_type"] is None:
            continue
        rec = base64.b64decode(e["record_b64"])
        key, iv = bytes.fromhex(e["key"]), bytes.fromhex(e["iv"])
        ex = R.explicit_len(e["version"], e["cipher"])
        ct = rec[5 + ex:-16]
        pt = R._xor(ct, R.record_keystream(key, iv, e["version"], e["cipher"], e["seq"], len(ct)))
        content = pt[:len(pt) - e["seal_pad"] - 1] if e["version"] == R.TLS13 else pt
        assert O.tls_seal(_key(e), e["seq"], e["seal_type"], content, e["seal_pad"]) == rec, (i, e["why"])
        n += 1
    assert n > 0.9 * len(vectors[section])


def sweep_lengths():
    """every content length 0..1100, and within +-24 of each multiple of 1024 up to 16384"""
    s = set(range(1101))
    for m in range(1024, 16385, 1024):
        s.update(range(m - 24, min(m + 24, 16384) + 1))
    return sorted(s)


def test_oracle_seal_matches_reference_random(gen):
    rng = random.Random(0xA11CE)
    for kind in gen.KINDS:
        k = O.tls_key(kind["key"], kind["iv"], kind["version"], kind["cipher"])
        for n in (0, 1, 15, 16, 17, 63, 64, 65, 255, 1000, 4096, 16384):
            seq = rng.randrange(1 << 64)
            t = rng.choice([23, 23, 21, 22])
            pad = rng.choice([0, 1, 77]) if kind["version"] == R.TLS13 else 0
            c = rng.randbytes(n)
            want = R.seal_record(kind["key"], kind["iv"], kind["version"], kind["cipher"], seq, t, c, pad)
            assert O.tls_seal(k, seq, t, c, pad) == want, (kind["name"], n)


def test_oracle_seal_matches_reference_sweep_sample(gen):
    rng = random.Random(0x5EEB)
    lengths = sweep_lengths()
    assert len(lengths) == 1101 + 14 * 49 + 25  # 1024 +- 24 lies within 0..1100
    edges = [1023, 1024, 1025, 4095, 4096, 4097, 4104, 4105, 8191, 8192, 8193, 16383, 16384]
    for kind in gen.KINDS:
        k = O.tls_key(kind["key"], kind["iv"], kind["version"], kind["cipher"])
        for n in edges + rng.sample(lengths, 27):
            seq = rng.randrange(1 << 48)
            c = rng.randbytes(n)
            want = R.seal_record(kind["key"], kind["iv"], kind["version"], kind["cipher"], seq, 23, c)
            assert O.tls_seal(k, seq, 23, c) == want, (kind["name"], n)
