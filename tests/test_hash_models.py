"""The Python models of tests/hash_models.py against the header the kernels include (rust_dataframe_amd/csrc/rdf_hash.h, built
into tests/cpp/test_hash.cpp with g++): the same hash on more than 10 000 seeded inputs, and every collision the GPU tests
use (tests/hash_fixtures.py) distinct, valid UTF-8 and equal under the HEADER's hash — which is what makes those tests
meaningful for the multi-key join, whose route cannot be observed from outside."""
import os
import random
import subprocess
import tempfile
import time

import pytest

import hash_fixtures as F
import hash_models as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROW_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 4096 + 3)


@pytest.fixture(scope="module")
def header():
    """ask(lines) -> the answers of the header's program, one per request."""
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_hash_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_hash.cpp"), "-o", exe])

    def ask(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out = p.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out

    yield ask
    os.remove(exe)


def header_row_hashes(ask, rows):
    return [int(x, 16) for x in ask(["U " + (r.hex() or "-") for r in rows])]


def header_tuple_hashes(ask, tuples, dtypes):
    return [int(x, 16) for x in ask(["T " + " ".join("%x" % H.key_bits(v, d) for v, d in zip(t, dtypes)) for t in tuples])]


def test_mixers_invert():
    rng = random.Random(1)
    xs = [0, 1, H.M, H.K_CS_EMPTY, 1 << 63] + [rng.getrandbits(64) for _ in range(5000)]
    for x in xs:
        assert H.mix64_inv(H.mix64(x)) == x and H.mix64(H.mix64_inv(x)) == x
        assert H.join_mix_inv(H.join_mix(x)) == x and H.join_mix(H.join_mix_inv(x)) == x


def test_constants_and_mixers_equal_the_header(header):
    empty, long_row, streams = header(["K"])[0].split()
    assert (int(empty, 16), int(long_row, 16), int(streams, 16)) == (H.K_CS_EMPTY, H.LONG_ROW, H.STREAMS)
    rng = random.Random(2)
    xs = [0, 1, H.M] + [rng.getrandbits(64) for _ in range(1000)]
    assert [int(v, 16) for v in header(["M %x" % x for x in xs])] == [H.mix64(x) for x in xs]
    assert [int(v, 16) for v in header(["J %x" % x for x in xs])] == [H.join_mix(x) for x in xs]


def test_row_hash_equals_the_header_on_10000_rows(header):
    rng = random.Random(3)
    rows = []
    for n in ROW_LENGTHS:                                           # every length of the list: random bytes, all 0x00, all 0xFF
        reps = 4 if n > 600 else 40
        rows += [bytes(rng.getrandbits(8) for _ in range(n)) for _ in range(reps)] + [b"\0" * n, b"\xff" * n]
    while len(rows) < 10_000:                                       # and short lengths at random
        rows.append(bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 40))))
    assert header_row_hashes(header, rows) == [H.utf8_hash(r) for r in rows]


def test_tuple_hash_equals_the_header_on_10000_tuples(header):
    rng = random.Random(4)
    kinds = (H.I64, H.I32, H.F64, H.F32)
    edge = {H.I64: (0, -1, -(1 << 63), (1 << 63) - 1), H.I32: (0, -1, -(1 << 31), (1 << 31) - 1),
            H.F64: (0.0, -0.0, float("inf"), -float("inf"), 5e-324, 0x7FF8000000000001, 0xFFF8000000000000),
            H.F32: (0.0, -0.0, float("inf"), -float("inf"), 0x00000001, 0x7FC00001, 0xFFC00000)}
    asked, want = [], []
    for i in range(10_002):
        nk = 2 + i % 3
        dt = tuple(rng.choice(kinds) for _ in range(nk))
        t = tuple(rng.choice(edge[d]) if rng.random() < 0.2 else H.value_of_bits(rng.getrandbits(H.WIDTH[d]), d) for d in dt)
        asked.append("T " + " ".join("%x" % H.key_bits(v, d) for v, d in zip(t, dt)))
        want.append(H.tuple_hash(t, dt))
    assert [int(x, 16) for x in header(asked)] == want


def test_key_bits_follow_the_order_of_the_values():
    import struct
    f64 = [-float("inf"), -1.5, -5e-324, -0.0, 0.0, 5e-324, 2.0, float("inf")]
    assert [H.key_bits(v, H.F64) for v in f64] == sorted(H.key_bits(v, H.F64) for v in f64)
    assert len({H.key_bits(v, H.F64) for v in f64}) == len(f64)     # -0.0 and +0.0 are two keys
    f32 = [struct.unpack("<f", struct.pack("<f", v))[0] for v in (-3.0, -0.0, 0.0, 1e-45, 7.0)]
    assert [H.key_bits(v, H.F32) for v in f32] == sorted(H.key_bits(v, H.F32) for v in f32)
    for d, vals in ((H.I64, [-(1 << 63), -1, 0, 1, (1 << 63) - 1]), (H.I32, [-(1 << 31), -1, 0, 1, (1 << 31) - 1])):
        assert [H.key_bits(v, d) for v in vals] == sorted(H.key_bits(v, d) for v in vals)
        assert all(H.value_of_bits(H.key_bits_inv(H.key_bits(v, d), d), d) == v for v in vals)


def test_every_utf8_fixture_collides_under_the_header(header):
    t0 = time.perf_counter()
    fx = F.utf8_fixtures()
    built = time.perf_counter() - t0
    for name, rows in fx.items():
        assert len(set(rows)) == len(rows) >= 2, name
        for r in rows:
            assert r.decode("utf-8").encode("utf-8") == r and max(r) < 0x80, name
        got = header_row_hashes(header, rows)
        assert len(set(got)) == 1, (name, [hex(h) for h in got])
        assert got == [H.utf8_hash(r) for r in rows]
        # a control differs from its collider in one byte and leaves the hash
        ctl = bytes([rows[0][0] ^ 1]) + rows[0][1:]
        assert header_row_hashes(header, [ctl])[0] != got[0], name
    assert [len(r) for r in fx["tail_7_bytes"]] == [15, 15]
    assert sorted(len(r) for r in fx["lengths_15_16"]) == [15, 16]
    assert [len(r) for r in fx["long_512"]] == [512, 512] and [len(r) for r in fx["long_1040_round_2"]] == [1040, 1040]
    a, b = fx["long_1040_round_2"]
    assert [w for w in range(130) if a[8 * w:8 * w + 8] != b[8 * w:8 * w + 8]] == [70, 129]
    a, b = fx["long_512_words_62_63"]
    assert [w for w in range(64) if a[8 * w:8 * w + 8] != b[8 * w:8 * w + 8]] == [62, 63]
    a, b = fx["tail_7_bytes"]
    assert a[:8] != b[:8] and a[8:] != b[8:]
    e0, e1 = fx["free_word"]
    assert (H.utf8_hash_raw(e0), H.utf8_hash_raw(e1)) == (H.K_CS_EMPTY, H.K_CS_EMPTY ^ 1)
    assert len(fx["group_32"]) == 32
    assert built < 5.0, built


def test_every_tuple_fixture_collides_under_the_header(header):
    for nk, (dt, x, y, z) in F.tuple_fixtures().items():
        assert len(dt) == nk and H.F64 in dt and H.I32 in dt
        assert x != y and [H.key_bits(v, d) for v, d in zip(x, dt)] != [H.key_bits(v, d) for v, d in zip(y, dt)]
        hx, hy, hz = header_tuple_hashes(header, [x, y, z], dt)
        assert hx == hy == H.tuple_hash(x, dt) and hx != 0
        assert hz == 0 == H.tuple_hash(z, dt)


def test_constructors_for_other_shapes(header):
    """utf8_partner on any two words of rows of any length (same stream, different streams, a partial tail), and
    utf8_with_hash / tuple_with_hash on arbitrary targets."""
    rng = random.Random(6)
    for n, words in ((16, (1, 0)), (23, (1, 2)), (600, (3, 67)), (600, (74, 10)), (1100, (1, 129)), (1100, (137, 9))):
        a = bytes(rng.randint(0x20, 0x7E) for _ in range(n))
        b = H.utf8_partner(a, words, True, seed=n)
        assert len(b) == n and a != b
        assert sorted(w for w in range((n + 7) // 8) if a[8 * w:8 * w + 8] != b[8 * w:8 * w + 8]) == sorted(words)
        ha, hb = header_row_hashes(header, [a, b])
        assert ha == hb
    for n in (12, 15, 16, 40, 513, 1040):
        t = rng.getrandbits(64)
        r = H.utf8_with_hash(t, n, True, seed=n)
        assert len(r) == n and header_row_hashes(header, [r])[0] == t
    dt = (H.I64, H.F32, H.I32, H.F64)
    for _ in range(20):
        t = rng.getrandbits(64)
        z = H.tuple_with_hash(t, dt, (rng.randint(-9, 9), 1.5, 7))
        assert header_tuple_hashes(header, [z], dt)[0] == t
