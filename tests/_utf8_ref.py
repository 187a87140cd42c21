"""Reference verdicts for the UTF-8 validation tests (test_utf8_host.py, test_gpu_utf8.py).

A complete message is valid iff CPython's strict decoder, bytes.decode("utf-8"), accepts it
(RFC 3629: no surrogates, no overlongs, nothing above U+10FFFF).  A prefix (the message still
open after a batch) is PREFIX iff SOME extension is accepted by bytes.decode, else INVALID —
not Python's incremental decoder, which defers ED A0.  Extensions of 0-3 bytes drawn from
{80, 8F, 90, 9F, A0, BF} are enough: the alphabet holds every endpoint of every second-byte
range.  tail = the smallest k such that dropping k bytes leaves a fully valid string."""
import functools
import itertools
import random

VALID, INVALID, NOT_TEXT, PREFIX, BAD_RANGE = range(5)

EXT_ALPHABET = (0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF)
_EXTS = [bytes(e) for k in range(0, 4) for e in itertools.product(EXT_ALPHABET, repeat=k)]


def is_valid(b: bytes) -> bool:
    try:
        bytes(b).decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@functools.lru_cache(maxsize=None)
def _extendable(rest: bytes) -> bool:
    return any(is_valid(rest + e) for e in _EXTS)


def complete_verdict(b: bytes):
    return (VALID, 0) if is_valid(b) else (INVALID, 0)


def prefix_verdict(b: bytes):
    """(PREFIX, tail) or (INVALID, 0) of a message that may still continue"""
    b = bytes(b)
    try:
        b.decode("utf-8")
        return PREFIX, 0
    except UnicodeDecodeError as e:
        rest = b[e.start:]  # b[:e.start] is the longest valid prefix
    # an extension can only complete a sequence cut off at the very end (1-3 bytes)
    if len(rest) <= 3 and _extendable(rest):
        return PREFIX, len(rest)
    return INVALID, 0


def judge(data: bytes, table, data_len=None, open_index=None):
    """verdicts [(status, tail)] and the summary dict for a message table
    [(arena_off, len, opcode)] over data[0, data_len); entry open_index is judged as a prefix"""
    data_len = len(data) if data_len is None else data_len
    out = []
    for i, (off, ln, op) in enumerate(table):
        if op != 1:
            out.append((NOT_TEXT, 0))
        elif off + ln > data_len:
            out.append((BAD_RANGE, 0))
        elif i == open_index:
            out.append(prefix_verdict(data[off:off + ln]))
        else:
            out.append(complete_verdict(data[off:off + ln]))
    bad = [i for i, (s, _) in enumerate(out) if s in (INVALID, BAD_RANGE)]
    ov = 0
    if open_index is not None and open_index < len(out):
        ov = out[open_index][0] | (out[open_index][1] << 8)
    summary = {"n_text": sum(1 for s, _ in out if s != NOT_TEXT), "n_invalid": len(bad),
               "first_invalid": bad[0] if bad else 0xFFFFFFFF, "open_verdict": ov}
    return out, summary


# the known answers of the issue (RFC 3629 edge code points and their neighbours)
KNOWN_VALID = ["", "68656c6c6f", "c280", "e0a080", "ed9fbf", "ee8080", "efbfbf", "f0908080", "f48fbfbf"]
KNOWN_INVALID = ["c080", "c1bf", "e09fbf", "eda080", "f08fbfbf", "f4908080", "f5808080", "ff", "80"]
KNOWN_TRUNCATED = [("c2", 1), ("e282", 2), ("f09f98", 3)]

FUZZ_LENGTHS = (0, 1, 2, 3, 5, 15, 16, 17, 40, 246, 1000, 5000)


def _char(rng):
    r = rng.random()
    if r < 0.4:
        return chr(rng.randrange(0x80))
    if r < 0.6:
        return chr(rng.randrange(0x80, 0x800))
    if r < 0.8:
        c = rng.randrange(0x800, 0x10000 - 0x800)  # no surrogates
        return chr(c if c < 0xD800 else c + 0x800)
    return chr(rng.randrange(0x10000, 0x110000))


@functools.lru_cache(maxsize=None)
def fuzz_messages(seed, n=2000):
    """[(opcode, payload)]: lengths in characters from FUZZ_LENGTHS; 40 % ASCII and 20 % each of
    2-, 3- and 4-byte characters; half the non-empty messages mutated once (a byte set to a
    random value, truncated at a random byte, or one of 80 BF C0 ED F4 FF inserted); one
    message in 10 BINARY"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        b = bytearray("".join(_char(rng) for _ in range(rng.choice(FUZZ_LENGTHS))).encode("utf-8"))
        if b and rng.random() < 0.5:
            kind = rng.randrange(3)
            if kind == 0:
                b[rng.randrange(len(b))] = rng.randrange(256)
            elif kind == 1:
                del b[rng.randrange(len(b)):]
            else:
                b.insert(rng.randrange(len(b) + 1), rng.choice((0x80, 0xBF, 0xC0, 0xED, 0xF4, 0xFF)))
        out.append((2 if rng.random() < 0.1 else 1, bytes(b)))
    return tuple(out)
