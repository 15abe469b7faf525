"""The executable model of rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32: what the device must return, row by row.

hash / xxhash64 over columns c0..c(k-1) with a seed (Spark's default: 42): h = seed; for each column in order, a row that
is not NULL there gives h = H(value, h), a NULL leaves h as it is; the result is never NULL.

    dtype            hashed as                             dtype         hashed as
    bool             hashInt(1 / 0)                        i64 / u64     hashLong of the bits
    i8 / i16 / i32   hashInt of the sign-extended value    f32           hashInt(floatToIntBits)
    u8 / u16         hashInt of the zero-extended value    f64           hashLong(doubleToLongBits)
    u32              hashInt of its bits                   utf8          hashUnsafeBytes

Spark has no unsigned types: the rows above define them here.  Every NaN hashes as the canonical quiet NaN and -0.0 as +0.0.
Murmur3 is Spark's Murmur3_x86_32: after the 4-byte words every remaining byte is taken alone, as a SIGNED byte, through a
full mixK1 / mixH1 round, and the final mix uses the byte length.  XXH64 is the standard one with the running hash as seed;
hashInt / hashLong are XXH64 of the 4 / 8 little-endian bytes.  The digests and crc32 ARE hashlib / zlib.
"""
import hashlib
import random
import struct
import zlib

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
MURMUR3_32, XXHASH64 = 0, 1
MD5, SHA1, SHA224, SHA256, SHA384, SHA512 = range(6)
DIGEST_NAMES = ("md5", "sha1", "sha224", "sha256", "sha384", "sha512")
HEX_BYTES = (32, 40, 56, 64, 96, 128)
DTYPES = ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "f32", "f64", "bool")   # rdf_dtype order


def _rotl32(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _rotl64(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


# ---- Murmur3_x86_32, Spark's
def _mix_k1(k1):
    k1 = (k1 * 0xCC9E2D51) & M32
    k1 = _rotl32(k1, 15)
    return (k1 * 0x1B873593) & M32


def _mix_h1(h1, k1):
    h1 ^= k1
    h1 = _rotl32(h1, 13)
    return (h1 * 5 + 0xE6546B64) & M32


def _fmix32(h1, length):
    h1 ^= length & M32
    h1 ^= h1 >> 16
    h1 = (h1 * 0x85EBCA6B) & M32
    h1 ^= h1 >> 13
    h1 = (h1 * 0xC2B2AE35) & M32
    return h1 ^ (h1 >> 16)


def mm3_hash_int(v, seed):
    return _fmix32(_mix_h1(seed & M32, _mix_k1(v & M32)), 4)


def mm3_hash_long(v, seed):
    h1 = _mix_h1(seed & M32, _mix_k1(v & M32))
    h1 = _mix_h1(h1, _mix_k1((v >> 32) & M32))
    return _fmix32(h1, 8)


def mm3_hash_bytes(b, seed):
    h1 = seed & M32
    aligned = len(b) - len(b) % 4
    for i in range(0, aligned, 4):
        h1 = _mix_h1(h1, _mix_k1(int.from_bytes(b[i:i + 4], "little")))
    for i in range(aligned, len(b)):
        signed = b[i] - 256 if b[i] >= 128 else b[i]
        h1 = _mix_h1(h1, _mix_k1(signed & M32))
    return _fmix32(h1, len(b))


# ---- XXH64
P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _xx_round(acc, v):
    return (_rotl64((acc + v * P2) & M64, 31) * P1) & M64


def _xx_merge(h, v):
    return ((h ^ _xx_round(0, v)) * P1 + P4) & M64


def xx64_hash_bytes(b, seed):
    seed &= M64
    n = len(b)
    i = 0
    if n >= 32:
        v = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed, (seed - P1) & M64]
        while i + 32 <= n:
            for k in range(4):
                v[k] = _xx_round(v[k], int.from_bytes(b[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (_rotl64(v[0], 1) + _rotl64(v[1], 7) + _rotl64(v[2], 12) + _rotl64(v[3], 18)) & M64
        for k in range(4):
            h = _xx_merge(h, v[k])
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while i + 8 <= n:
        h ^= _xx_round(0, int.from_bytes(b[i:i + 8], "little"))
        h = (_rotl64(h, 27) * P1 + P4) & M64
        i += 8
    if i + 4 <= n:
        h ^= (int.from_bytes(b[i:i + 4], "little") * P1) & M64
        h = (_rotl64(h, 23) * P2 + P3) & M64
        i += 4
    while i < n:
        h ^= (b[i] * P5) & M64
        h = (_rotl64(h, 11) * P1) & M64
        i += 1
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    return h ^ (h >> 32)


def xx64_hash_int(v, seed):
    return xx64_hash_bytes(struct.pack("<I", v & M32), seed)


def xx64_hash_long(v, seed):
    return xx64_hash_bytes(struct.pack("<Q", v & M64), seed)


# ---- values
def _f32_bits(x):
    bits = struct.unpack("<I", struct.pack("<f", x))[0]
    if (bits & 0x7FFFFFFF) > 0x7F800000:
        return 0x7FC00000
    return 0 if bits == 0x80000000 else bits


def _f64_bits(x):
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    if (bits & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000:
        return 0x7FF8000000000000
    return 0 if bits == 0x8000000000000000 else bits


def hash_value(kind, dtype, value, h):
    """One non-NULL value folded into the running hash h.  dtype: one of DTYPES or "utf8" (value: bytes or str); f32 / f64
    values may be given as floats or, to carry a NaN payload, as ("bits", integer)."""
    hint, hlong, hbytes = (mm3_hash_int, mm3_hash_long, mm3_hash_bytes) if kind == MURMUR3_32 else (xx64_hash_int, xx64_hash_long, xx64_hash_bytes)
    if dtype == "utf8":
        return hbytes(value.encode() if isinstance(value, str) else bytes(value), h)
    if dtype == "bool":
        return hint(1 if value else 0, h)
    if dtype in ("f32", "f64"):
        if isinstance(value, tuple):
            value = struct.unpack("<f", struct.pack("<I", value[1]))[0] if dtype == "f32" else struct.unpack("<d", struct.pack("<Q", value[1]))[0]
            # (a signalling NaN may be quieted on the way: every NaN hashes alike, so the payload does not matter)
        return hint(_f32_bits(value), h) if dtype == "f32" else hlong(_f64_bits(value), h)
    if dtype in ("i64", "u64"):
        return hlong(int(value) & M64, h)
    return hint(int(value) & M32, h)      # sign extension of i8 / i16 / i32 is Python's two's complement under the mask


def hash_row(kind, dtypes, values, seed=42):
    """values[k] is the row's value in column k, None = NULL.  The raw unsigned hash (32 or 64 bits)."""
    h = seed & (M32 if kind == MURMUR3_32 else M64)
    for dt, v in zip(dtypes, values):
        if v is not None:
            h = hash_value(kind, dt, v, h)
    return h


def as_signed(h, bits):
    return h - (1 << bits) if h >> (bits - 1) else h


def spark_hash(dtypes, values, seed=42):
    return as_signed(hash_row(MURMUR3_32, dtypes, values, seed), 32)


def spark_xxhash64(dtypes, values, seed=42):
    return as_signed(hash_row(XXHASH64, dtypes, values, seed), 64)


def digest(kind, row):
    """Lowercase hex text of the row's digest as bytes; None for a NULL row."""
    if row is None:
        return None
    return hashlib.new(DIGEST_NAMES[kind], row.encode() if isinstance(row, str) else bytes(row)).hexdigest().encode()


def sha2_kind(bits):
    """sha2(col, bits): 0 means 256; anything but 0, 224, 256, 384, 512 is an error here (Spark returns NULL)."""
    return {0: SHA256, 224: SHA224, 256: SHA256, 384: SHA384, 512: SHA512}[bits]


def crc32(row):
    if row is None:
        return None
    return zlib.crc32(row.encode() if isinstance(row, str) else bytes(row)) & M32


# ---- the table tests/cpp/test_digest_host.cpp reads
FUNCTIONS = ("murmur3", "xxhash64", "crc32") + DIGEST_NAMES


def apply_bytes(fn, row, seed):
    """The function's result over one byte row as text: the unsigned integer, or the hex digest."""
    if fn == "murmur3":
        return str(mm3_hash_bytes(row, seed))
    if fn == "xxhash64":
        return str(xx64_hash_bytes(row, seed))
    if fn == "crc32":
        return str(crc32(row))
    return digest(DIGEST_NAMES.index(fn), row).decode()


def write_host_table(path, nrandom=10_000):
    """A case a line: `<function> <seed> <row as hex, '-' = empty, 'N' = the row [nullptr, nullptr)> <expected>`, and for the
    fixed-width forms `int <kind> <dtype> <raw bits> <seed> <expected>`.  Every length 0..300, nrandom random rows per
    function, the empty row without a pointer, rows of 4 KiB + 1.  Returns the number of lines."""
    rng = random.Random(19)
    lines = []
    for fi, fn in enumerate(FUNCTIONS):
        r = random.Random(100 + fi)
        rows = [r.randbytes(n) for n in range(301)]
        rows += [r.randbytes(r.randrange(0, 200) if r.random() < 0.9 else r.randrange(200, 700)) for _ in range(nrandom)]
        rows += [r.randbytes(4097), bytes([0xFF]) * 4097, b"Spark"]
        for row in rows:
            seed = r.choice([0, 42, M32, r.getrandbits(32)]) if fn == "murmur3" else (r.choice([0, 42, M64, r.getrandbits(64)]) if fn == "xxhash64" else 0)
            lines.append(f"{fn} {seed} {row.hex() or '-'} {apply_bytes(fn, row, seed)}")
        lines.append(f"{fn} 42 N {apply_bytes(fn, b'', 42 if fn in ('murmur3', 'xxhash64') else 0)}")
    edge = {"f32": [0x00000000, 0x80000000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x3F800000],
            "f64": [0, 1 << 63, 0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FF0000000000000, 0xFFF0000000000000]}
    for kind in (MURMUR3_32, XXHASH64):
        for di, dt in enumerate(DTYPES):
            width = {"i8": 8, "u8": 8, "i16": 16, "u16": 16, "i32": 32, "u32": 32, "f32": 32, "bool": 1}.get(dt, 64)
            raws = [0, (1 << width) - 1, 1 << (width - 1)] + edge.get(dt, []) + [rng.getrandbits(width) for _ in range(200)]
            for raw in raws:
                seed = rng.choice([0, 42, rng.getrandbits(32)])
                if dt in ("f32", "f64"):
                    value = ("bits", raw)
                elif dt.startswith("i") and raw >> (width - 1):
                    value = raw - (1 << width)
                else:
                    value = raw
                lines.append(f"int {kind} {di} {raw} {seed} {hash_value(kind, dt, value, seed)}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
