"""tests/digest_ref.py, the model the device is held to, against known answers: Spark's documented examples, hashlib / zlib,
the xxhash package where it imports, and Murmur3's signed tail worked out by hand."""
import random

import pytest

import digest_ref as R


def test_spark_known_answers():
    # hash('Spark', array(123), 2): an array hashes element by element
    assert R.spark_hash(["utf8", "i32", "i32"], ["Spark", 123, 2]) == -1321691492
    assert R.spark_xxhash64(["utf8", "i32", "i32"], ["Spark", 123, 2]) == 5602566077635097486
    assert R.digest(R.MD5, "Spark") == b"8cde774d6f7333752ed72cacddb05126"
    assert R.digest(R.SHA1, "Spark") == b"85f5955f4b27a9a4c2aab6ffe5d7189fc298b92c"
    assert R.digest(R.sha2_kind(256), "Spark") == b"529bc3b07127ecb7e53a4dcf1991d9152c24537d919178022b2c42657f79a26b"
    assert R.digest(R.sha2_kind(0), "Spark") == R.digest(R.SHA256, "Spark")
    assert R.crc32("Spark") == 1557323817


def test_digest_widths_and_nulls():
    for kind, width in enumerate(R.HEX_BYTES):
        assert len(R.digest(kind, b"")) == width
        assert R.digest(kind, None) is None
    assert R.crc32(None) is None and R.crc32(b"") == 0
    with pytest.raises(KeyError):
        R.sha2_kind(128)


def test_nulls_leave_the_running_hash_alone():
    for fn in (R.spark_hash, R.spark_xxhash64):
        assert fn(["i32", "utf8", "i64"], [None, None, None], seed=7) == 7
        assert fn(["i32", "utf8", "i64"], [5, None, 9]) == fn(["i32", "i64"], [5, 9])


def test_xxh64_against_the_xxhash_package():
    xxhash = pytest.importorskip("xxhash")
    rng = random.Random(3)
    for n in list(range(0, 201)) + [255, 256, 257, 1000]:
        b = rng.randbytes(n)
        seed = rng.choice([0, 42, rng.getrandbits(64)])
        assert R.xx64_hash_bytes(b, seed) == xxhash.xxh64(b, seed=seed).intdigest(), (n, seed)
    assert R.xx64_hash_int(123, 42) == xxhash.xxh64((123).to_bytes(4, "little"), seed=42).intdigest()
    assert R.xx64_hash_long(-5, 42) == xxhash.xxh64((-5 & R.M64).to_bytes(8, "little"), seed=42).intdigest()


def test_murmur3_signed_tail_by_hand():
    """b'caf\\xc3\\xa9' ("café"), seed 42: one word 0x c3 66 61 63 little-endian, then the byte 0xA9 alone as -87."""
    def rotl(x, r):
        return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF

    def round_(h, k):
        k = (k * 0xCC9E2D51) & 0xFFFFFFFF
        k = rotl(k, 15)
        k = (k * 0x1B873593) & 0xFFFFFFFF
        h ^= k
        h = rotl(h, 13)
        return (h * 5 + 0xE6546B64) & 0xFFFFFFFF

    row = b"caf\xc3\xa9"
    assert len(row) == 5 and row[-1] == 0xA9
    h = round_(42, 0xC3666163)
    h = round_(h, (-87) & 0xFFFFFFFF)              # the SIGNED byte: 0xFFFFFFA9, not 0x000000A9
    h ^= 5
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    assert R.mm3_hash_bytes(row, 42) == h
    unsigned = round_(round_(42, 0xC3666163), 0xA9)
    assert R.mm3_hash_bytes(row, 42) != R._fmix32(unsigned, 5)
    # a last byte of 0xE9, length 5
    row2 = b"abcd\xe9"
    h2 = round_(round_(0, int.from_bytes(b"abcd", "little")), (0xE9 - 256) & 0xFFFFFFFF)
    assert R.mm3_hash_bytes(row2, 0) == R._fmix32(h2, 5)


def test_canonical_floats_and_extensions():
    for kind in (R.MURMUR3_32, R.XXHASH64):
        assert R.hash_value(kind, "f32", -0.0, 42) == R.hash_value(kind, "f32", 0.0, 42)
        assert R.hash_value(kind, "f64", -0.0, 42) == R.hash_value(kind, "f64", 0.0, 42)
        assert R.hash_value(kind, "f64", ("bits", 0xFFF8000000000123), 42) == R.hash_value(kind, "f64", float("nan"), 42)
        assert R.hash_value(kind, "f32", ("bits", 0x7FC00001), 42) == R.hash_value(kind, "f32", float("nan"), 42)
        assert R.hash_value(kind, "i8", -1, 42) == R.hash_value(kind, "i32", -1, 42)
        assert R.hash_value(kind, "u8", 255, 42) == R.hash_value(kind, "i32", 255, 42)
        assert R.hash_value(kind, "u32", 0xFFFFFFFF, 42) == R.hash_value(kind, "i32", -1, 42)
        assert R.hash_value(kind, "bool", True, 42) == R.hash_value(kind, "i32", 1, 42)
        assert R.hash_value(kind, "u64", 2**64 - 1, 42) == R.hash_value(kind, "i64", -1, 42)
