"""Host UTF-8 check (uvhttp_ws_utf8_feed / uvhttp_ws_utf8_finish, include/uvhttp_ws_amd.h)
against CPython's strict decoder (tests/_utf8_ref.py): known answers, every string of length
1-4 over an alphabet holding every boundary byte, the fuzz corpus fed in pieces, and the ABI of
the new structs.  No GPU."""
import ctypes as C
import itertools
import random

import pytest

import _utf8_ref as R
import uvhttp_amd as U

ALPHABET = bytes([0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1,
                  0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF])


def _feed(pieces):
    """-> (feed rc of the first failing piece or 0, finish rc, state)"""
    st = U.Utf8State()
    for p in pieces:
        if U.utf8_feed(st, p) != 0:
            return -1, None, st
    return 0, U.utf8_finish(st), st


@pytest.mark.parametrize("hexs", R.KNOWN_VALID)
def test_known_valid(hexs):
    b = bytes.fromhex(hexs)
    assert R.is_valid(b)
    rc, fin, st = _feed([b])
    assert (rc, fin, st.n) == (0, 0, 0)


@pytest.mark.parametrize("hexs", R.KNOWN_INVALID)
def test_known_invalid(hexs):
    b = bytes.fromhex(hexs)
    assert not R.is_valid(b)
    assert _feed([b])[0] == -1


@pytest.mark.parametrize("hexs,n", R.KNOWN_TRUNCATED)
def test_known_truncated(hexs, n):
    b = bytes.fromhex(hexs)
    rc, fin, st = _feed([b])
    assert rc == 0 and fin != 0
    assert st.n == n and bytes(st.pend)[:n] == b  # the state is the open sequence's bytes
    assert R.prefix_verdict(b) == (R.PREFIX, n)


@pytest.mark.parametrize("hexs", ["eda0", "f490", "e09f"])
def test_fail_fast(hexs):
    """no continuation can make these valid: feed refuses them at once"""
    assert _feed([bytes.fromhex(hexs)])[0] == -1
    assert R.prefix_verdict(bytes.fromhex(hexs)) == (R.INVALID, 0)


def test_exhaustive_short_strings():
    """every string of length 1-4 over the 24-byte alphabet: feed + finish == bytes.decode, feed
    alone == the prefix reference (and its state's n == the reference tail)"""
    L = U.lib()
    st = U.Utf8State()
    n = 0
    for k in range(1, 5):
        for t in itertools.product(ALPHABET, repeat=k):
            b = bytes(t)
            C.memset(C.byref(st), 0, 4)
            rc = L.uvhttp_ws_utf8_feed(C.byref(st), b, k)
            status, tail = R.prefix_verdict(b)
            if status == R.INVALID:
                assert rc == -1, b.hex()
            else:
                assert rc == 0 and st.n == tail, b.hex()
                assert (L.uvhttp_ws_utf8_finish(C.byref(st)) == 0) == R.is_valid(b), b.hex()
            n += 1
    assert n == 24 + 24 ** 2 + 24 ** 3 + 24 ** 4


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_split_feeds(seed):
    """each fuzz message in one piece and in 1-4 random pieces: the same verdict, the
    reference's"""
    rng = random.Random(100 + seed)
    invalid = 0
    for _, b in R.fuzz_messages(seed):
        rc, fin, st = _feed([b])
        status, tail = R.prefix_verdict(b)
        assert (rc == 0) == (status == R.PREFIX), b.hex()
        if rc == 0:
            assert st.n == tail and (fin == 0) == R.is_valid(b)
        cuts = sorted(rng.randrange(len(b) + 1) for _ in range(rng.randrange(4)))
        pieces = [b[a:z] for a, z in zip([0] + cuts, cuts + [len(b)])]
        rc2, fin2, st2 = _feed(pieces)
        assert (rc2, fin2) == (rc, fin), (b.hex(), cuts)
        if rc == 0:
            assert (st2.n, bytes(st2.pend)) == (st.n, bytes(st.pend))
        invalid += not R.is_valid(b)
    assert 0.2 <= invalid / 2000 <= 0.6


def test_resume_from_device_tail():
    """the state after a device PREFIX verdict is the last `tail` bytes of the message"""
    whole = "grüße 😀 €".encode("utf-8")
    for cut in range(len(whole) + 1):
        head = whole[:cut]
        status, tail = R.prefix_verdict(head)
        assert status == R.PREFIX
        st = U.Utf8State()
        st.n = tail
        for i, x in enumerate(head[len(head) - tail:]):
            st.pend[i] = x
        assert U.utf8_feed(st, whole[cut:]) == 0 and U.utf8_finish(st) == 0


def test_bad_state_and_null():
    st = U.Utf8State()
    st.n = 4
    assert U.utf8_feed(st, b"a") == -1
    L = U.lib()
    assert L.uvhttp_ws_utf8_feed(None, b"a", 1) == -1
    assert L.uvhttp_ws_utf8_finish(None) != 0
    ok = U.Utf8State()
    assert L.uvhttp_ws_utf8_feed(C.byref(ok), None, 0) == 0


def test_abi_sizes_and_einval():
    assert C.sizeof(U.Utf8Verdict) == 4
    assert C.sizeof(U.Utf8Summary) == 16
    assert C.sizeof(U.Utf8State) == 4
    assert (U.UTF8_VALID, U.UTF8_INVALID, U.UTF8_NOT_TEXT, U.UTF8_PREFIX, U.UTF8_BAD_RANGE) == \
        (R.VALID, R.INVALID, R.NOT_TEXT, R.PREFIX, R.BAD_RANGE)
    # no engine: EINVAL, with or without a device
    assert U.lib().uvhttp_ws_gpu_validate_utf8(None, None, 0, None, 0, None, 0, None, None, None) == -1
    assert U.test_hooks_library().uvhttp_ws_gpu_validate_utf8(None, None, 0, None, 0, None, 0, None,
                                                              None, None) == -1


def test_struct_sizes_in_the_header():
    """the C side agrees: a tiny program against the public header"""
    import os
    import subprocess
    import tempfile
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include "uvhttp_ws_amd.h"\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu\\n",'
           'sizeof(uvhttp_ws_utf8_verdict_t),sizeof(uvhttp_ws_utf8_summary_t),'
           'sizeof(uvhttp_ws_utf8_state_t));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.run(["cc", "-I", os.path.join(repo, "include"), "-o", exe, c], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["4", "16", "4"]
