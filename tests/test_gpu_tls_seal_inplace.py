"""uvhttp_tls_gpu_seal_records in place: with src = out and src_off = out_off + the record's header
length (5, + 8 for the explicit nonce of TLS 1.2 AES-GCM) a record's content lies where its
ciphertext will, and the call writes the bytes it writes out of place (and the oracle's).  This is
the property uvhttp_tls_gpu_seal_parts_coalesced rests on: every 16-byte (AES-GCM)
or 64-byte (ChaCha20-Poly1305) piece of a record is loaded and stored by the same lane, load first;
the header, the nonce, the TLS 1.3 type byte and the tag occupy bytes that hold no plaintext."""
import random

import numpy as np
import pytest

import _oracle as O
import _tls_coalesce_ref as K
import _tls_send_ref as R

pytestmark = pytest.mark.gpu

LENS = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 16384]
GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def eng(torch):
    import uvhttp_amd as U
    e = U.TlsEngine(0)
    yield e
    e.close()


@pytest.mark.parametrize("kind", range(6))
def test_in_place_equals_out_of_place(torch, eng, kind):
    rng = random.Random(600 + kind)
    keys = np.concatenate([R.make_key(rng, R.KEY_KINDS[kind]), R.make_key(rng, R.KEY_KINDS[kind])])
    over, hdr = R.overhead(keys[0]), K.header_len(keys[0])
    contents = [rng.randbytes(n) for n in LENS]
    packed = b"".join(contents)
    apart, inplace = np.zeros(len(LENS), O.TLS_SEAL_DT), np.zeros(len(LENS), O.TLS_SEAL_DT)
    total = 3  # the first record starts at an odd offset
    src_pos, want = 0, bytearray(b"\xA5" * total)
    staged = np.full(total + sum(LENS) + over * len(LENS), FILL, np.uint8)
    for i, c in enumerate(contents):
        seq = (1 << 32) - 3 + i
        apart[i] = (src_pos, total, seq, len(c), i % 2, 23, 0)
        inplace[i] = (total + hdr, total, seq, len(c), i % 2, 23, 0)
        staged[total + hdr:total + hdr + len(c)] = np.frombuffer(c, np.uint8)
        want += O.tls_seal(keys[i % 2:i % 2 + 1], seq, 23, c)
        src_pos += len(c)
        total += len(c) + over
    assert total == len(want) == staged.size
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")  # noqa: E731
    d_keys = dev(keys)
    out_a = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    eng.seal_records(dev(np.frombuffer(packed, np.uint8)), dev(apart), len(LENS), d_keys, 2, out_a[:total])
    big = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    buf = big[GUARD:GUARD + total]
    buf.copy_(dev(staged))
    eng.seal_records(buf, dev(inplace), len(LENS), d_keys, 2, buf)
    torch.cuda.synchronize()
    a, b = out_a.cpu().numpy(), big.cpu().numpy()
    assert a[:total].tobytes() == bytes(want) and (a[total:] == FILL).all()
    assert b[GUARD:GUARD + total].tobytes() == bytes(want)
    assert (b[:GUARD] == FILL).all() and (b[GUARD + total:] == FILL).all()
