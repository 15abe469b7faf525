"""rdf_lexsort_to_indices on the MI355X: sorting by Utf8 columns, alone or mixed with numeric keys.  Every case runs over
host and device memory and compares the row order exactly (not as sets).  Small cases are held to Python's stable
sorted() over the rows' bytes; large ones are built so that the order is known in advance."""
import csv
import os

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMS = ["host", "device"]


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


# ---------------------------------------------------------------- inputs

def utf8(rows, row_offset=0, data_offset=0):
    """rows: bytes or None.  row_offset junk rows before them and data_offset junk bytes before the data make the chunk
    look like a slice (value offsets that do not start at 0, validity at an odd bit offset)."""
    enc = [b"j" * (i % 3 + 1) for i in range(row_offset)] + [b"" if r is None else r for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xee" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    nulls = sum(r is None for r in rows)
    valid = None
    if nulls:
        valid = A.pack_bits(np.array([True] * row_offset + [r is not None for r in rows], dtype=bool))
    return A.HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), data_offset, nulls)


def utf8_fixed(mat):
    """A chunk of equally long rows from a [rows, width] uint8 matrix, built without a Python loop."""
    n, w = mat.shape
    offs = (np.arange(n + 1, dtype=np.int64) * w).astype(np.int32)
    data = np.concatenate([mat.reshape(-1), np.zeros(8, dtype=np.uint8)])
    return A.HostUtf8(offs, data, None, 0, n, 0, 0)


def num(values, valid=None):
    return A.HostArray.from_numpy(np.asarray(values), valid)


def to_device(x):
    if isinstance(x, A.HostUtf8):
        return A.DeviceUtf8.from_host(x)
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def run(api, keys, mem):
    """keys: [(chunks, descending)] of host chunks -> the row order as a numpy array."""
    n = sum(c.length for c in keys[0][0])
    if mem == "host":
        r = api.lexsort_to_indices(keys)
        assert r.length == n
        return np.asarray(r.values[:n]).astype(np.int64)
    dkeys = [([to_device(c) for c in chunks], d) for chunks, d in keys]
    t = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    out = A.DeviceArray(t.data_ptr(), None, 0, n, A.U32, 0, keep=t)
    api.lexsort_to_indices(dkeys, out=out)
    assert out.length == n
    return t[:n].cpu().numpy().view(np.uint32).astype(np.int64)


# ---------------------------------------------------------------- references

def ref_order(cols):
    """cols: [(values, descending)], values a list with None for NULL.  Stable, NULLs last in both directions."""
    n = len(cols[0][0])
    order = list(range(n))
    for vals, desc in reversed(cols):
        live = [i for i in order if vals[i] is not None]
        dead = [i for i in order if vals[i] is None]
        order = sorted(live, key=lambda i: vals[i], reverse=desc) + dead
    return np.array(order, dtype=np.int64)


def both(api, keys, expected):
    for mem in MEMS:
        got = run(api, keys, mem)
        assert np.array_equal(got, expected), (mem, np.nonzero(got != expected)[0][:10])


# ---------------------------------------------------------------- small cases

def test_empty_null_and_prefix_rows(api):
    rows = [b"abc", None, b"", b"ab", b"b", None, b"abc", b"", b"a", b"abd", b"ab"]
    for desc in (False, True):
        both(api, [([utf8(rows)], desc)], ref_order([(rows, desc)]))


def test_embedded_zero_bytes_and_high_bytes(api):
    rows = [b"a\0b", b"b", b"a", b"a\0", b"\0", b"", b"\x80", b"\xff", b"z", b"\xc3\xa9", b"e\xcc\x81", b"a\0\0", b"\x7f",
            b"a\xff", b"a\x00\xff", None]
    assert ref_order([(rows, False)]).tolist()[:4] == [5, 4, 2, 3]    # "" < "\0" < "a" < "a\0"
    for desc in (False, True):
        both(api, [([utf8(rows)], desc)], ref_order([(rows, desc)]))


def test_every_length_up_to_40(api):
    rng = np.random.default_rng(1)
    base = bytes(rng.integers(97, 100, 40, dtype=np.uint8))
    rows = [base[:L] for L in range(41)]                                              # every prefix of one string
    rows += [bytes(rng.integers(97, 100, L, dtype=np.uint8)) for L in range(41) for _ in range(6)]
    rows += [base[:L] + b"\0" for L in range(40)] + [None] * 5
    perm = rng.permutation(len(rows))
    rows = [rows[i] for i in perm]
    for desc in (False, True):
        both(api, [([utf8(rows)], desc)], ref_order([(rows, desc)]))


def test_many_chunks_with_offsets_and_odd_validity(api):
    rng = np.random.default_rng(2)
    chunks, allrows = [], []
    for c in range(9):
        k = int(rng.integers(0, 40))
        rows = [None if rng.random() < 0.2 else bytes(rng.integers(97, 101, int(rng.integers(0, 12)), dtype=np.uint8)) for _ in range(k)]
        chunks.append(utf8(rows, row_offset=int(rng.integers(0, 13)), data_offset=int(rng.integers(0, 9))))
        allrows += rows
    for desc in (False, True):
        both(api, [(chunks, desc)], ref_order([(allrows, desc)]))


def test_one_mib_row_among_short_ones(api):
    rng = np.random.default_rng(3)
    rows = [bytes(rng.integers(108, 111, int(rng.integers(0, 9)), dtype=np.uint8)) for _ in range(3000)]
    big = b"m" * (1 << 20)
    rows[1234] = big
    rows[77] = big[:-1] + b"n"
    rows[78] = big + b"\0"
    for desc in (False, True):
        both(api, [([utf8(rows)], desc)], ref_order([(rows, desc)]))


def test_mixed_criteria(api):
    rng = np.random.default_rng(4)
    n = 5000
    s = [None if rng.random() < 0.1 else bytes(rng.integers(97, 100, int(rng.integers(0, 4)), dtype=np.uint8)) for _ in range(n)]
    f = rng.integers(-3, 4, n).astype(np.float64) * 0.5
    fv = rng.random(n) > 0.1
    i = rng.integers(-5, 5, n).astype(np.int64)
    fl = [float(x) if v else None for x, v in zip(f, fv)]
    il = [int(x) for x in i]
    us, fa, ia = utf8(s), num(f, fv), num(i)
    # [utf8 asc, f64 desc]
    both(api, [([us], False), ([fa], True)], ref_order([(s, False), (fl, True)]))
    # [i64 asc, utf8 desc]
    both(api, [([ia], False), ([us], True)], ref_order([(il, False), (s, True)]))
    # a Utf8 key whose ties are broken by a later key, and another Utf8 key after that
    t = [bytes([97 + int(x) % 2]) * 9 for x in rng.integers(0, 2, n)]
    both(api, [([us], True), ([ia], False), ([utf8(t)], False)], ref_order([(s, True), (il, False), (t, False)]))


def test_numeric_keys_equal_sort_to_indices(api):
    rng = np.random.default_rng(5)
    n = 70000
    f = rng.normal(size=n)
    f[rng.integers(0, n, 500)] = 0.0
    f[rng.integers(0, n, 500)] = -0.0
    f[rng.integers(0, n, 300)] = np.nan
    fv = rng.random(n) > 0.05
    i = rng.integers(-50, 50, n).astype(np.int64)
    a, b = num(f, fv), num(i)
    for desc in ([False, False], [True, False], [False, True]):
        want = api.sort_to_indices([[b], [a]], desc)
        want = np.asarray(want.values[:n]).astype(np.int64)
        both(api, [([b], desc[0]), ([a], desc[1])], want)


def test_uk_cities_by_city(api):
    with open(os.path.join(ROOT, "tests", "golden", "uk_cities_with_headers.csv"), newline="") as fh:
        rows = [r["city"].encode("utf-8") for r in csv.DictReader(fh)]
    for desc in (False, True):
        both(api, [([utf8(rows[:20]), utf8(rows[20:])], desc)], ref_order([(rows, desc)]))


# ---------------------------------------------------------------- large cases (order known in advance)

def digits(perm, width):
    """[n, width] uint8: perm[i] in decimal, zero-padded."""
    out = np.zeros((len(perm), width), dtype=np.uint8)
    v = np.asarray(perm, dtype=np.int64).copy()
    for k in range(width - 1, -1, -1):
        out[:, k] = 48 + v % 10
        v //= 10
    return out


def test_heavy_duplicates_keep_row_order(api):
    rng = np.random.default_rng(6)
    words = sorted({bytes(rng.integers(97, 123, int(rng.integers(1, 20)), dtype=np.uint8)) for _ in range(400)})[:100]
    assert len(words) == 100
    pick = rng.integers(0, 100, 1_000_000)
    lens = np.array([len(w) for w in words])[pick]
    offs = np.zeros(len(pick) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    blob = np.frombuffer(b"".join(words[k] for k in pick.tolist()) + b"\0" * 8, dtype=np.uint8).copy()
    col = A.HostUtf8(offs.astype(np.int32), blob, None, 0, len(pick), 0, 0)
    both(api, [([col], False)], np.argsort(pick, kind="stable"))
    both(api, [([col], True)], np.argsort(-pick, kind="stable"))


def test_long_shared_prefix(api):
    rng = np.random.default_rng(7)
    n = 20000
    perm = rng.permutation(n)
    mat = np.concatenate([np.full((n, 4096), 112, dtype=np.uint8), digits(perm, 6)], axis=1)
    both(api, [([utf8_fixed(mat)], False)], np.argsort(perm, kind="stable"))
    both(api, [([utf8_fixed(mat)], True)], np.argsort(-perm, kind="stable"))


def test_identical_64k_rows_finish_in_row_order(api):
    n, w = 20000, 65536
    mat = np.broadcast_to(np.arange(w, dtype=np.int64).astype(np.uint8) | 1, (n, w))
    col = utf8_fixed(np.ascontiguousarray(mat))                                  # 1.3 GB
    both(api, [([col], False)], np.arange(n))
    both(api, [([col], True)], np.arange(n))


def test_two_chunks_over_2_pow_31_bytes(api):
    rng = np.random.default_rng(8)
    per, w = 530000, 2048                                                        # 2 x 1.09 GB
    perm = rng.permutation(2 * per)
    chunks = []
    for c in range(2):
        mat = np.full((per, w), 113, dtype=np.uint8)
        mat[:, w - 7:] = digits(perm[c * per:(c + 1) * per], 7)
        mat[:, 5] = 114
        chunks.append(utf8_fixed(mat))
        del mat
    assert sum(len(c.data) for c in chunks) > 2**31
    both(api, [(chunks, False)], np.argsort(perm, kind="stable"))


def test_ten_million_random_short_rows(api):
    rng = np.random.default_rng(9)
    n = 10_000_000
    lens = rng.integers(0, 13, n)
    mat = rng.integers(0, 4, (n, 12), dtype=np.uint8) * 85                      # bytes 0, 85, 170, 255: ties and high bytes
    mat[np.arange(12)[None, :] >= lens[:, None]] = 0
    valid = rng.random(n) > 0.1
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    blob = np.concatenate([mat[np.arange(12)[None, :] < lens[:, None]], np.zeros(8, dtype=np.uint8)])
    col = A.HostUtf8(offs.astype(np.int32), blob, A.pack_bits(valid), 0, n, 0, int((~valid).sum()))
    # the order of (12 bytes zero-padded, length) is the byte order of the rows
    hi = (mat[:, :8].astype(np.uint64) << (np.arange(56, -1, -8, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
    lo = (mat[:, 8:].astype(np.uint64) << (np.arange(56, 31, -8, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64) | lens.astype(np.uint64)
    live = np.nonzero(valid)[0]
    for desc in (False, True):
        if desc:
            o = np.lexsort((~lo[live], ~hi[live]))
        else:
            o = np.lexsort((lo[live], hi[live]))
        expected = np.concatenate([live[o], np.nonzero(~valid)[0]])
        both(api, [([col], desc)], expected)
