"""The colliding keys of tests/test_hash_collisions_gpu.py, constructed once with tests/hash_models.py.  They live in a
module without GPU imports so that tests/test_hash_models.py can hold every one of them to the header's own hash on the CPU.
Building all of them takes about 0.3 s (measured with time.perf_counter around utf8_fixtures() and tuple_fixtures())."""
import functools
import random

import hash_models as H


def _ascii(rng, n):
    return bytes(rng.randint(0x20, 0x7E) for _ in range(n))


UTF8_NAMES = ("adjacent", "far_apart", "two_chunks", "rep_is_the_other", "behind_nulls", "tail_7_bytes", "lengths_15_16", "long_512",
              "long_1040_round_2", "long_512_words_62_63", "free_word", "group_32")


@functools.lru_cache(maxsize=None)
def utf8_fixtures():
    """name -> list of distinct rows that share one hash."""
    rng = random.Random(20)
    fx = {}
    for i, name in enumerate(UTF8_NAMES[:5]):   # 16-byte pairs
        a = _ascii(rng, 16)
        fx[name] = [a, H.utf8_partner(a, (0, 1), True, seed=100 + i)]
    a = _ascii(rng, 15)
    fx["tail_7_bytes"] = [a, H.utf8_partner(a, (0, 1), True, seed=110)]          # the last two words, the last one partial
    a = _ascii(rng, 16)
    fx["lengths_15_16"] = [a, H.utf8_with_hash(H.utf8_hash(a), 15, True, seed=111)]
    a = _ascii(rng, 512)
    fx["long_512"] = [a, H.utf8_partner(a, (5, 40), True, seed=112)]             # the wave path, one word per stream
    a = _ascii(rng, 1040)
    fx["long_1040_round_2"] = [a, H.utf8_partner(a, (70, 129), True, seed=113)]  # chained streams: words of the second round (and the third)
    a = _ascii(rng, 512)
    fx["long_512_words_62_63"] = [a, H.utf8_partner(a, (62, 63), True, seed=114)]
    fx["free_word"] = [H.utf8_with_hash(H.K_CS_EMPTY, 16, True, seed=115), H.utf8_with_hash(H.K_CS_EMPTY ^ 1, 16, True, seed=116)]
    fx["group_32"] = H.utf8_group(32, 16, seed=117)
    assert tuple(fx) == UTF8_NAMES
    return fx


TUPLE_DTYPES = {2: (H.I32, H.F64), 3: (H.I32, H.F64, H.I64), 4: (H.F32, H.I32, H.F64, H.I64)}


@functools.lru_cache(maxsize=None)
def tuple_fixtures():
    """nkeys -> (dtypes, X, Y, Z): X != Y share a hash, Z's hash is 0 (the hash NULL rows are given).  Float columns hold bits."""
    out = {}
    for nk, dt in TUPLE_DTYPES.items():
        rng = random.Random(30 + nk)
        x = tuple(H.random_value(rng, d) for d in dt)
        y = H.tuple_partner(x, dt, seed=40 + nk)
        z = H.tuple_with_hash(0, dt, tuple(H.random_value(rng, d) for d in dt[:-1]))
        x = tuple(H.raw_bits(v, d) if d in (H.F64, H.F32) else v for v, d in zip(x, dt))
        out[nk] = (dt, x, y, z)
    return out
