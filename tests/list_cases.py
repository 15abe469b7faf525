"""The case table of the List suites and the checker both of them run: tests/test_list_ref.py holds the oracle to the model of
tests/list_ref.py on it (no GPU), tests/test_list_gpu.py the device kernels.  `check_case` works against any Api.

A case is a logical list column (or two, for the set functions) built so that one edge of rdf_list.hip is reached; how it is
laid out in memory — row offset, child offset, a child validity buffer, unreferenced child elements behind the last row — is
decided when it is materialised, and that is also what chooses the kernel form: the host looks at values.length / rows, so
unreferenced child elements behind the last row move a call from the row-per-lane kernels to the row-per-wave ones without
changing a single row.  A case whose referenced elements alone average 48 a row has the wave form only.

Thresholds restated here (rdf_list.hip / rdf_capi.cpp), each next to the cases built around it:
  48    values.length / rows at which the host picks a row per wave (find / extreme / remove; a + b for the set functions)
  1024  child elements 64 rows may span to be staged in LDS (kListStage: find / extreme / remove; kSortStage: sort)
  768   elements per input (and of the output) a run of rows may span in list_set_kernel (kSetStage)
  1024  elements per input of a row list_set_block_kernel takes (kSetBlockMax); longer rows: list_set_wave_kernel
  40    elements of a row list_sort_lane_kernel sorts (kSortLaneMax); 4096 those of list_sort_block_kernel (kSortBlockMax)
  24    total / rows below which the sort runs the lane kernel first
Values are drawn over the whole range of the type and salted with its extremes (floats: +-0, +-inf, denormals, NaNs of both
signs with payloads; the all-ones pattern, which is the bitonic network's pad key for 8-byte types, is among them)."""
import functools
import zlib

import numpy as np

import hash_models as H
import list_ref as R
from rust_dataframe_amd import _abi as A

DTYPES = {"i8": A.I8, "i16": A.I16, "i32": A.I32, "i64": A.I64, "u8": A.U8, "u16": A.U16, "u32": A.U32, "u64": A.U64, "f32": A.F32, "f64": A.F64}
WIDE = ("i32", "i64", "u32", "u64", "f32", "f64")      # the types with 200 values to a home slot
WAVE_AVG, LIST_STAGE, SET_STAGE, SET_BLOCK_MAX, SORT_LANE_MAX, SORT_BLOCK_MAX, SORT_LANE_AVG = 48, 1024, 768, 1024, 40, 4096, 24
SET_OPS = ("distinct", "except", "intersect", "union", "repeat")
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

KERNELS = {
    ("find", "lane"): "list_find_kernel", ("find", "wave"): "list_wave_kernel",
    ("extreme", "lane"): "list_extreme_kernel", ("extreme", "wave"): "list_wave_kernel",
    ("remove", "lane"): "list_remove_kernel", ("remove", "wave"): "list_remove_wave_kernel",
    ("set", "lane"): "list_set_kernel + list_set_wave_kernel", ("set", "wave"): "list_set_wave_kernel",
    ("sort", "inplace"): "list_sort_lane_kernel + list_sort_block_kernel",
    ("sort", "radix"): "list_row_ids_kernel + os_scatter_kernel + take_kernel",
}


# ---------------------------------------------------------------- values
def npdt(name):
    return np.dtype(A.NP_OF[DTYPES[name]])


def from_bits(bits, dt):
    return np.asarray(bits, dtype=_UINT[dt.itemsize]).view(dt)


def specials(dt):
    if dt.kind == "f":
        w = 8 * dt.itemsize
        mant = 23 if w == 32 else 52
        sign, inf, ones = 1 << (w - 1), ((1 << (w - mant - 1)) - 1) << mant, (1 << w) - 1
        bits = [0, sign, inf, inf | sign, 1, 1 | sign, (1 << mant) - 1,                       # +-0, +-inf, denormals
                inf | (1 << (mant - 1)), inf | sign | (1 << (mant - 1)),                        # the quiet NaN of either sign
                inf | 1, inf | sign | 0x2A, ones, ones ^ sign,                                   # payloads; all ones; the largest key
                inf - (1 << mant) | ((1 << mant) - 1), (inf - (1 << mant) | ((1 << mant) - 1)) | sign]   # +-max finite
        return from_bits(bits, dt)
    info = np.iinfo(dt)
    return np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1] + ([-1] if dt.kind == "i" else []), dtype=dt)


def random_values(rng, dt, n):
    """n values with uniformly drawn bits: the whole range of the type (for floats that includes a few NaNs and denormals)."""
    raw = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    return (raw >> np.uint64(64 - 8 * dt.itemsize)).astype(_UINT[dt.itemsize]).view(dt)


def make_pool(rng, dt, extra):
    return np.concatenate([specials(dt), random_values(rng, dt, extra)])


def draws(rng, pool, n):
    return pool[rng.integers(0, len(pool), size=n)] if n else pool[:0]


def distinct_values(rng, dt, n):
    """n values, pairwise different under == and none a NaN — as far as the type has that many (the one-byte types repeat)."""
    if dt.itemsize <= 2:
        allv = from_bits(rng.permutation(1 << (8 * dt.itemsize)), dt)
        return np.resize(allv, n)
    out = np.zeros(0, dt)
    while len(out) < n:
        v = np.concatenate([out, random_values(rng, dt, 2 * n), specials(dt)])
        if dt.kind == "f":
            v = v[~np.isnan(v)]
            v = v[~((v == 0) & np.signbit(v))]
        _, first = np.unique(v, return_index=True)
        out = v[np.sort(first)]
    return rng.permutation(out)[:n]


def without(values, needle):
    with np.errstate(invalid="ignore"):
        return values[values != needle]


def plain_needle(rng, dt, pool):
    """A value of the pool that is neither a NaN nor a zero."""
    ok = pool[(pool == pool) & (pool != 0)]
    return ok[int(rng.integers(0, len(ok)))]


def needles_for(rng, dt, pool):
    extra = [dt.type(np.nan), dt.type(-0.0)] if dt.kind == "f" else [np.iinfo(dt).min]
    return [plain_needle(rng, dt, pool)] + extra


# ---------------------------------------------------------------- logical lists
class LL:
    """off: int64 [rows + 1]; valid: bool [rows] or None; child: the child values (head before off[0] and tail behind off[-1] included)."""

    def __init__(self, lens, valid, child=None, head=0, tail=0):
        self.off = head + np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)
        self.head, self.tail, self.child = head, tail, child
        self.n = len(self.off) - 1

    def fill(self, rng, pool):
        self.child = draws(rng, pool, int(self.off[-1]) + self.tail)
        return self

    def row(self, i):
        return self.child[int(self.off[i]):int(self.off[i + 1])]

    def set_row(self, i, values):
        self.child[int(self.off[i]):int(self.off[i + 1])] = values


class Built:
    def __init__(self, a, b=None, needles=(), counts=(0, 1, 3), sort="inplace"):
        self.a, self.b, self.needles, self.counts, self.sort = a, b, list(needles), tuple(counts), sort
        self.cache = {}

    def forms(self):
        """The kernel forms this case can be materialised in (set functions: a + b together)."""
        used = len(self.a.child) + (len(self.b.child) if self.b is not None else 0)
        return ("lane", "wave") if self.a.n and used // self.a.n < WAVE_AVG else ("wave",)

    def sort_form(self):
        total = int(self.a.off[-1] - self.a.off[0])
        return "lane" if total // max(self.a.n, 1) < SORT_LANE_AVG else "block"


def nulls(rng, n, frac):
    return rng.uniform(size=n) >= frac


# ---------------------------------------------------------------- the cases
CASES = {}


def case(name, group, dtypes=tuple(DTYPES), sort_form=None, forms=("lane", "wave")):
    def deco(fn):
        CASES[name] = dict(name=name, group=group, build=fn, dtypes=tuple(dtypes), sort_form=sort_form, forms=tuple(forms))
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def built(name, dtname):
    c = CASES[name]
    dt = npdt(dtname)
    rng = np.random.default_rng([zlib.crc32(name.encode()), DTYPES[dtname]])
    b = c["build"](rng, dt)
    if c["group"] != "sort":
        assert b.forms() == c["forms"], f"{name}: built for {c['forms']}, its shape gives {b.forms()}"
    else:
        assert b.sort_form() == c["sort_form"], f"{name}: built for the {c['sort_form']} form, its shape gives {b.sort_form()}"
    return b


# ---- one row per lane: contains / position / max / min / remove
def _rows_case(nrows):
    def build(rng, dt):
        pool = make_pool(rng, dt, 6)
        a = LL(rng.integers(0, 13, nrows), nulls(rng, nrows, 0.15), head=2, tail=3).fill(rng, pool)
        return Built(a, needles=needles_for(rng, dt, pool))
    return build


for _n in (1, 63, 64, 65, 129, 300):
    case(f"rows{_n}", "reduce")(_rows_case(_n))

MANY_ROWS = 9000      # more rows than one launch of the wave-form kernels covers at a wave a row: 2048 blocks of 4 waves
MANY_DTYPES = ("i16", "u32", "f64")


@case("rows9000", "reduce", dtypes=MANY_DTYPES)
def _rows_many(rng, dt):
    """9000 rows of 0 - 3 elements.  In the wave form (8192 waves in flight) list_wave_kernel and list_remove_wave_kernel go
    round their grid-stride loops; in the lane form the call spreads over 36 blocks."""
    pool = make_pool(rng, dt, 3)
    a = LL(rng.integers(0, 4, MANY_ROWS), nulls(rng, MANY_ROWS, 0.1), head=1, tail=0).fill(rng, pool)
    return Built(a, needles=needles_for(rng, dt, pool)[:2])


def _span_case(span):
    """A 64-row group spanning exactly kListStage (staged in LDS) or one element more (every lane walks its row); the NULL
    rows own elements, every one of them equal to the needle."""
    def build(rng, dt):
        pool = make_pool(rng, dt, 6)
        lens = np.full(64, 16)
        lens[20] += span - 1024
        valid = np.ones(64, bool)
        valid[[0, 10, 11, 40, 63]] = False
        a = LL(lens, valid, head=1, tail=2).fill(rng, pool)
        assert int(a.off[-1] - a.off[0]) == span
        needle = plain_needle(rng, dt, pool)
        for r in np.flatnonzero(~valid):
            a.set_row(r, needle)
        return Built(a, needles=[needle] + needles_for(rng, dt, pool)[1:])
    return build


case("span1024", "reduce")(_span_case(1024))
case("span1025", "reduce")(_span_case(1025))

MASK_LENS = [63, 1, 1, 62, 2, 63, 65, 0, 64, 127, 1, 64, 3, 61, 128, 5]      # rows that start at bit 63, end at bit 64 / 65, ...


def _maskword_case(where, head):
    """The needle sits only in the last element of the even rows ("last": for the odd rows it is the element just before them)
    or only in the first element of the odd rows ("first": for the even rows the element just after them)."""
    def build(rng, dt):
        pool = make_pool(rng, dt, 6)
        needle = plain_needle(rng, dt, pool)
        valid = np.ones(len(MASK_LENS), bool)
        valid[12] = False
        a = LL(MASK_LENS, valid, head=head, tail=2).fill(rng, without(pool, needle))
        starts = (a.off[:-1] - head).tolist()
        assert 63 in starts and 64 in starts and 65 in starts and int(a.off[-1] - a.off[0]) <= LIST_STAGE
        for r, n in enumerate(MASK_LENS):
            if n and where == "last" and r % 2 == 0:
                a.child[a.off[r + 1] - 1] = needle
            if n and where == "first" and r % 2 == 1:
                a.child[a.off[r]] = needle
        return Built(a, needles=[needle])
    return build


case("maskword_last", "reduce")(_maskword_case("last", 0))
case("maskword_first", "reduce")(_maskword_case("first", 0))
case("maskword_last_head1", "reduce")(_maskword_case("last", 1))


@case("one_row_spans", "reduce")
def _one_row_spans(rng, dt):
    """Three groups of 64 rows, in each one row covers the whole span (the first, a middle and the last lane) and the others
    are empty; the needle is the row's last element and nothing else."""
    pool = make_pool(rng, dt, 6)
    needle = plain_needle(rng, dt, pool)
    lens = np.zeros(192, int)
    lens[[31, 64, 191]] = 1000
    a = LL(lens, None, head=0, tail=1).fill(rng, without(pool, needle))
    for r in (31, 64, 191):
        a.child[a.off[r + 1] - 1] = needle
    return Built(a, needles=[needle])


# ---- one row per wave
@case("wave_lens", "reduce", forms=("wave",))
def _wave_lens(rng, dt):
    """Rows of 0 / 1 / 63 / 64 / 65 / 129 elements; row 5 has its first match in lane 63 of the first stride and another in
    lane 0 of the second, row 6 only the latter, row 2 in its last element; row 3 is NULL and owns 64 needles."""
    pool = make_pool(rng, dt, 6)
    needle = plain_needle(rng, dt, pool)
    lens = [0, 1, 63, 64, 65, 129, 129, 64]
    valid = np.ones(len(lens), bool)
    valid[3] = False
    a = LL(lens, valid, head=3, tail=5).fill(rng, without(pool, needle))
    a.set_row(3, needle)
    a.child[a.off[5] + 63] = a.child[a.off[5] + 64] = a.child[a.off[6] + 64] = a.child[a.off[3] - 1] = needle
    return Built(a, needles=[needle])


@case("wave_nan", "reduce", forms=("wave",))
def _wave_nan(rng, dt):
    """Rows that hold nothing but NaNs (both signs, several payloads), rows with a single NaN, a NULL row that owns elements."""
    pool = make_pool(rng, dt, 6)
    lens = [64, 65, 129, 1, 70, 100, 50]
    valid = np.ones(len(lens), bool)
    valid[4] = False
    a = LL(lens, valid, head=0, tail=0).fill(rng, pool)
    if dt.kind == "f":
        nans = specials(dt)[np.isnan(specials(dt))]
        numbers = pool[~np.isnan(pool)]
        for r in (0, 2, 3):
            a.set_row(r, draws(rng, nans, lens[r]))
        for r in (1, 5, 6):
            a.set_row(r, draws(rng, numbers, lens[r]))
            a.child[a.off[r] + int(rng.integers(0, lens[r]))] = nans[r % len(nans)]
    return Built(a, needles=needles_for(rng, dt, pool))


def _wave_rows_case(nrows):
    def build(rng, dt):
        pool = make_pool(rng, dt, 6)
        a = LL(rng.integers(50, 80, nrows), nulls(rng, nrows, 0.2), head=1, tail=0).fill(rng, pool)
        return Built(a, needles=needles_for(rng, dt, pool))
    return build


case("wave_rows33", "reduce", forms=("wave",))(_wave_rows_case(33))
case("wave_rows45", "reduce", forms=("wave",))(_wave_rows_case(45))


# ---- set functions, one row per lane
@case("set_rows", "set")
def _set_rows(rng, dt):
    pool = make_pool(rng, dt, 6)
    n = 129
    a = LL(rng.integers(0, 13, n), nulls(rng, n, 0.15), head=2, tail=3).fill(rng, pool)
    b = LL(rng.integers(0, 9, n), nulls(rng, n, 0.3), head=1, tail=1).fill(rng, pool)      # b's validity must not be looked at
    return Built(a, b)


@case("set_rows9000", "set", dtypes=MANY_DTYPES)
def _set_rows_many(rng, dt):
    """9000 rows of 0 - 3 elements: in the wave form list_set_block_kernel (one row per block, 2048 blocks), its write kernel
    and list_set_wave_kernel (8192 waves) go round their grid-stride loops."""
    pool = make_pool(rng, dt, 3)
    a = LL(rng.integers(0, 4, MANY_ROWS), nulls(rng, MANY_ROWS, 0.1), head=0, tail=1).fill(rng, pool)
    b = LL(rng.integers(0, 4, MANY_ROWS), None, head=2, tail=0).fill(rng, pool)
    return Built(a, b, counts=(2,))


def _set_span_case(which, span):
    """One run of 64 rows spanning exactly kSetStage elements of one input, or one element more (then the run is cut in two)."""
    def build(rng, dt):
        pool = make_pool(rng, dt, 10)
        long_, short = np.full(64, 12), np.full(64, 3)
        long_[37] += span - 768
        valid = np.ones(64, bool)
        valid[[5, 50]] = False
        a = LL(long_ if which == "a" else short, valid, head=1, tail=0).fill(rng, pool)
        b = LL(short if which == "a" else long_, None, head=0, tail=2).fill(rng, pool)
        assert int((a if which == "a" else b).off[-1] - (a if which == "a" else b).off[0]) == span
        return Built(a, b)
    return build


for _w in ("a", "b"):
    for _s in (768, 769):
        case(f"set_{_w}{_s}", "set")(_set_span_case(_w, _s))


def _union_out_case(total):
    """Rows whose a and b are disjoint and without repeats, so the union of the 64-row run holds exactly `total` elements:
    768 leaves through the LDS staging area of the output, 769 is written straight to memory."""
    def build(rng, dt):
        la, lb = np.full(64, 6), np.full(64, 6)
        lb[9] += total - 768
        a, b = LL(la, None, tail=1), LL(lb, None, head=2)
        a.child, b.child = np.zeros(int(a.off[-1]) + 1, dt), np.zeros(int(b.off[-1]), dt)
        for r in range(64):
            v = distinct_values(rng, dt, int(la[r] + lb[r]))
            a.set_row(r, v[:la[r]])
            b.set_row(r, v[la[r]:])
        got = R.set_op("union", a.off, None, a.child, b.off, b.child)[0][-1]
        assert got == total, got
        return Built(a, b)
    return build


case("union_out768", "set")(_union_out_case(768))
case("union_out769", "set")(_union_out_case(769))


@case("repeat_out768", "set")
def _repeat_out(rng, dt):
    """64 rows of 4 elements: count 3 gives a run of exactly 768 output elements, count 4 one of 1024."""
    pool = make_pool(rng, dt, 6)
    valid = np.ones(64, bool)
    a = LL(np.full(64, 4), valid, head=0, tail=0).fill(rng, pool)
    return Built(a, None, counts=(0, 1, 3, 4))


# ---- set functions, one row per block (tables in LDS)
def _short_rows(rng, n, hi):
    return rng.integers(0, hi + 1, n)


def _place(lens, where, what):
    for r, n in zip(where, what):
        lens[r] = n
    return lens


def _set_block_len_case(which):
    """Rows of 769 / 1024 / 1025 elements in one input (the other short) between 150 short rows: 769 and 1024 are the block
    kernel's, 1025 the wave kernel's; a NULL row that owns 800 elements lies between them."""
    def build(rng, dt):
        pool = make_pool(rng, dt, 400)
        n = 150
        long_ = _place(_short_rows(rng, n, 4), (10, 40, 70, 100), (769, 800, 1024, 1025))
        short = _short_rows(rng, n, 4)
        valid = nulls(rng, n, 0.05)
        valid[[10, 70, 100]] = True
        valid[40] = False
        a = LL(long_ if which == "a" else short, valid, head=1, tail=1).fill(rng, pool)
        b = LL(short if which == "a" else long_, None, head=0, tail=0).fill(rng, pool)
        return Built(a, b, counts=(2,))
    return build


case("set_block_len_a", "set")(_set_block_len_case("a"))
case("set_block_len_b", "set")(_set_block_len_case("b"))


@case("set_block_patterns", "set")
def _set_block_patterns(rng, dt):
    """All-distinct rows of 512 / 513 / 1024 elements (tables of 1024 / 2048 / 2048 slots, the last at its load limit), 1024 copies
    of one value, 1024 alternating 0.0 / -0.0 (integers: 0 / 1), 1024 NaNs (integers: the maximum).  b holds a few members of a."""
    pool = make_pool(rng, dt, 20)
    n = 170
    where, what = (3, 30, 64, 90, 127, 169), (512, 513, 1024, 1024, 1024, 1024)
    la, lb = _place(_short_rows(rng, n, 4), where, what), _place(_short_rows(rng, n, 4), where, (9,) * 6)
    a = LL(la, nulls(rng, n, 0.05), head=0, tail=2).fill(rng, pool)
    a.valid[list(where)] = True
    b = LL(lb, None, head=3, tail=0).fill(rng, pool)
    for r in where[:3]:
        a.set_row(r, distinct_values(rng, dt, int(la[r])))
    a.set_row(90, plain_needle(rng, dt, pool))
    nan = specials(dt)[np.isnan(specials(dt))] if dt.kind == "f" else np.array([np.iinfo(dt).max], dt)
    a.set_row(127, np.tile(np.array([0.0, -0.0] if dt.kind == "f" else [0, 1], dt), 512))
    a.set_row(169, draws(rng, nan, 1024))
    for r in where:
        ra = a.row(r)
        b.set_row(r, np.concatenate([ra[[5, 0, len(ra) - 1, 5]], draws(rng, pool, 3), nan[:1], np.array([-0.0 if dt.kind == "f" else 0], dt)]))
    return Built(a, b, counts=(2,))


def table_size_lds(n):
    size = 2
    while size < 2 * n:
        size <<= 1
    return size


@functools.lru_cache(maxsize=None)
def colliders(dt, size, slot, lds, want):
    return H.set_colliders(dt, size, slot, lds, want, seed=size, draws=1 << 20)


def colliding_row(rng, dt, n, size, lds, fresh, again):
    """n elements for a table of `size` slots: `fresh` values sharing the home slot size - 3 (a probe chain that long runs past
    the last slot and wraps), `again` repeats of them (contention on one slot: the smallest index must win), the rest drawn
    freely.  Returns (row, every colliding value found, in order)."""
    found = colliders(dt, size, size - 3, lds, fresh + 60)
    assert len(found) >= max(200, fresh + 50), (dt, size, len(found))
    home = H.set_home_lds if lds else H.set_home_wave
    assert {home(H.set_hash(H.set_hashed_bits(v, dt)), size) for v in found} == {size - 3}      # the collision itself
    row = np.concatenate([found[:fresh], draws(rng, found[:fresh], again), distinct_values(rng, dt, n - fresh - again)])
    return rng.permutation(row), found


@case("set_block_collide", "set", dtypes=WIDE)
def _set_block_collide(rng, dt):
    """Rows of 512 and 1024 elements (tables of 1024 and 2048 slots, both at the load limit of one element per two slots) made of
    values with one home slot three before the table's end; b's rows collide in their own tables and share members with a."""
    pool = make_pool(rng, dt, 6)
    n = 100
    la, lb = _place(_short_rows(rng, n, 3), (7, 64), (512, 1024)), _place(_short_rows(rng, n, 3), (7, 64), (300, 600))
    a, b = LL(la, None, head=1).fill(rng, pool), LL(lb, None, tail=1).fill(rng, pool)
    for r, na, nb in ((7, 512, 300), (64, 1024, 600)):
        assert table_size_lds(na) == 2 * na
        row, found = colliding_row(rng, dt, na, table_size_lds(na), True, 210, 150)
        a.set_row(r, row)
        rowb, _ = colliding_row(rng, dt, nb, table_size_lds(nb), True, 200, 60)
        rowb[:40] = found[190:230]          # colliding values of a's table: 20 members of a, 20 that are not
        b.set_row(r, rowb)
    return Built(a, b, counts=(1,))


# ---- set functions, one row per wave (tables in device memory)
def _wave_set_rows(rng, dt):
    pool = make_pool(rng, dt, 300)
    la, lb = [1025, 200, 3000, 1500, 0, 1100, 2], [100, 50, 100, 0, 1500, 1100, 3]
    valid = np.array([True, False, True, True, True, True, True])
    a, b = LL(la, valid, head=2, tail=1).fill(rng, pool), LL(lb, None, head=0, tail=3).fill(rng, pool)
    a.set_row(0, distinct_values(rng, dt, 1025))
    a.set_row(2, distinct_values(rng, dt, 3000))
    for r in (0, 2):
        b.set_row(r, np.concatenate([a.row(r)[:50][::-1], draws(rng, pool, 50)]))
    b.set_row(5, np.concatenate([a.row(5)[:500], draws(rng, pool, 600)]))
    return a, b


@case("set_wave_long", "set", forms=("wave",))
def _set_wave_long(rng, dt):
    """1025 and 3000 all-distinct elements, a long with b empty and the reverse, 1100 against 1100, a NULL row that owns 200
    elements between the long rows."""
    return Built(*_wave_set_rows(rng, dt), counts=(2,))


@case("set_wave_sparse", "set")
def _set_wave_sparse(rng, dt):
    """The rows of set_wave_long followed by 500 short ones: the call takes the row-per-lane form and the long rows reach the
    table kernels through its worklist."""
    a0, b0 = _wave_set_rows(rng, dt)
    pool = make_pool(rng, dt, 6)
    m = 500
    la, lb = np.concatenate([np.diff(a0.off), _short_rows(rng, m, 2)]), np.concatenate([np.diff(b0.off), _short_rows(rng, m, 2)])
    a = LL(la, np.concatenate([a0.valid, nulls(rng, m, 0.1)]), head=2).fill(rng, pool)
    b = LL(lb, None).fill(rng, pool)
    a.child[2:len(a0.child) - 1] = a0.child[2:-1]
    b.child[:len(b0.child) - 3] = b0.child[:-3]
    return Built(a, b, counts=(2,))


@case("set_wave_collide", "set", dtypes=WIDE, forms=("wave",))
def _set_wave_collide(rng, dt):
    """Rows of 1100 (a) and 1030 (b) elements: tables of 2200 and 2060 slots addressed by (hash * size) >> 32, filled with
    values whose home is three slots before the end."""
    la, lb = [1100, 5, 1100], [1030, 4, 1030]
    pool = make_pool(rng, dt, 6)
    a, b = LL(la, None).fill(rng, pool), LL(lb, None).fill(rng, pool)
    for r in (0, 2):
        row, found = colliding_row(rng, dt, 1100, 2200, False, 230, 200)
        a.set_row(r, row)
        rowb, _ = colliding_row(rng, dt, 1030, 2060, False, 220, 100)
        rowb[:40] = found[210:250]
        b.set_row(r, rowb)
    return Built(a, b, counts=(1,))


# ---- sort
def _patterns(rng, dt, n):
    v = R.from_bit_key(np.sort(R.bit_key(random_values(rng, dt, n))), dt)
    return v, v[::-1].copy(), np.full(n, v[n // 2], dt)


@case("sort_lane", "sort", sort_form="lane")
def _sort_lane(rng, dt):
    """Short rows; among them rows of 40 (the lane kernel's longest) and 41 (the block kernel's, through the worklist), rows of
    0 / 1 / 2 / 3, ascending / descending / all-equal rows, NULL rows that own elements (they are sorted too)."""
    pool = make_pool(rng, dt, 40)
    n = 200
    lens = rng.integers(0, 13, n)
    _place(lens, (5, 6, 7, 8, 60, 61, 62, 63, 64, 65, 130, 131, 199), (40, 41, 40, 40, 0, 1, 2, 3, 41, 40, 41, 41, 41))
    a = LL(lens, nulls(rng, n, 0.1), head=3, tail=2).fill(rng, pool)
    a.valid[5] = False
    for r, p in zip((6, 7, 8), _patterns(rng, dt, 41)):
        a.set_row(r, p[:lens[r]])
    for r, p in zip((130, 131, 199), _patterns(rng, dt, 41)):
        a.set_row(r, p)
    return Built(a)


@case("sort_run1024", "sort", sort_form="lane")
def _sort_run(rng, dt):
    """64 rows spanning exactly kSortStage elements (one run), then 64 spanning one more (two runs)."""
    lens = np.full(128, 16)
    lens[100] = 17
    a = LL(lens, None, head=3, tail=0).fill(rng, make_pool(rng, dt, 100))
    assert a.off[64] - a.off[0] == 1024 and a.off[128] - a.off[64] == 1025
    return Built(a)


BLOCK_LENS = (41, 64, 65, 255, 256, 257, 4095, 4096, 0, 1, 2, 3, 300, 300, 300)


def _sort_block_rows(rng, dt, extra):
    pool = make_pool(rng, dt, 3000)
    lens = np.concatenate([np.array(BLOCK_LENS), _short_rows(rng, extra, 3)])
    valid = np.ones(len(lens), bool)
    valid[[3, 9]] = False
    a = LL(lens, valid, head=1, tail=1).fill(rng, pool)
    for r, p in zip((12, 13, 14), _patterns(rng, dt, 300)):
        a.set_row(r, p)
    return Built(a)


@case("sort_block", "sort", sort_form="block")
def _sort_block(rng, dt):
    """Rows of 41 .. 4096 elements on both sides of every power of two the network is padded to, ascending / descending /
    all-equal rows, and rows of 0 / 1 / 2 / 3 elements that go through the block kernel because the long rows raised the average."""
    return _sort_block_rows(rng, dt, 0)


@case("sort_block_sparse", "sort", sort_form="lane")
def _sort_block_sparse(rng, dt):
    """The rows of sort_block followed by 600 short ones: the lane kernel runs first and hands the long rows over."""
    return _sort_block_rows(rng, dt, 600)


@case("sort_radix", "sort", sort_form="block")
def _sort_radix(rng, dt):
    """One row of 4097 elements: the whole call goes through the radix sort, the short rows with it."""
    a = LL([5, 4097, 0, 41, 1, 300], np.array([True, True, True, False, True, True]), head=2, tail=1).fill(rng, make_pool(rng, dt, 2000))
    return Built(a, sort="radix")


def cases_of(*groups):
    return [(n, d) for n, c in CASES.items() if c["group"] in groups for d in c["dtypes"]]


LAYOUT_CASES = ("rows129", "span1025", "wave_lens", "set_rows", "set_block_len_a", "set_wave_long", "sort_lane", "sort_block", "sort_radix")


# ---------------------------------------------------------------- materialising
def host_list(ll, code, form=None, other_len=0, layout="plain", row_offset=None):
    """The HostList of a logical list.  form "wave": unreferenced child elements (copies of referenced ones) are appended until
    (values.length + other_len) / rows reaches 48 (the set functions pad a alone: distinct and repeat never see b); "lane" / None: the child array as built.  layout "offsets": a row offset of
    3, a child offset of 5 and a child validity buffer full of zeros (it must be ignored)."""
    dt = np.dtype(A.NP_OF[code])
    rng = np.random.default_rng(len(ll.child) + 7 * ll.n)
    child = ll.child
    if form == "wave" and ll.n:
        want = WAVE_AVG * ll.n - other_len
        if len(child) < want:
            pad = child[rng.integers(0, len(child), want - len(child))] if len(child) else np.zeros(want - len(child), dt)
            child = np.concatenate([child, pad])
    ro = row_offset if row_offset is not None else (3 if layout == "offsets" else 0)
    co = 5 if layout == "offsets" else 0
    buf = np.ascontiguousarray(np.concatenate([random_values(rng, dt, co), child, np.zeros(1, dt)]))
    cval = np.zeros((len(buf) + 7) // 8 + 16, np.uint8) if layout == "offsets" else None
    values = A.HostArray(buf, cval, co, len(child), code, len(child) if cval is not None else 0)
    offs = np.ascontiguousarray(np.concatenate([np.zeros(ro, np.int64), ll.off]).astype(np.int32))
    bits = None
    if ll.valid is not None:
        bits = A.pack_bits(np.concatenate([rng.integers(0, 2, ro).astype(bool), ll.valid]))
    return A.HostList(offs, values, bits, ro, ll.n)


def materialise(b, code, form, layout="plain", row_offset=None):
    """-> (HostList a, HostList b or None)"""
    lb = host_list(b.b, code, None, 0, layout, 2 if layout == "offsets" else None) if b.b is not None else None      # b behind another row offset than a
    la = host_list(b.a, code, form, 0, layout, row_offset)      # a alone reaches 48 a row: distinct and repeat do not see b
    if form is not None and b.a.n:
        total = la.values.length + (lb.values.length if lb is not None and form == "lane" else 0)
        assert (total // b.a.n >= WAVE_AVG) == (form == "wave"), "the case cannot take this form"
    return la, lb


# ---------------------------------------------------------------- running one function and what the model says of it
def run(api, fn, la, lb=None, needle=None, count=0, dev=None):
    """One call -> the whole result as numpy arrays.  `dev` (tests/test_list_gpu.py) supplies device-resident inputs and outputs."""
    n, code = la.length, la.values.dtype
    out = (lambda *a: dev.out(*a)) if dev else (lambda *a: None)
    fetch = dev.fetch if dev else (lambda x: x)
    xa, xb = (dev.put(la), dev.put(lb) if lb is not None else None) if dev else (la, lb)
    if fn in ("contains", "position", "max", "min"):
        if fn == "contains":
            r = api.list_contains(xa, needle, out=out(A.BOOL, n, True))
        elif fn == "position":
            r = api.list_position(xa, needle, out=out(A.I32, n, False))
        else:
            r = api.list_extreme(xa, fn == "max", out=out(code, n, True))
        r = fetch(r)
        return dict(values=r.to_numpy().copy(), valid=r.valid_mask(), null_count=r.null_count, length=r.length)
    if fn == "sort":
        r = fetch(api.list_sort(xa, out=out(code, max(1, la.values.length), False)))
        return dict(values=r.to_numpy().copy(), null_count=r.null_count, length=r.length)
    if fn == "remove":
        outs = (out(A.I32, n + 1, False), out(code, max(1, la.values.length), False)) if dev else None
        oo, ov = api.list_remove(xa, needle, outs=outs)
    else:
        cap = {"union": la.values.length + (lb.values.length if lb is not None else 0), "repeat": la.values.length * count}.get(fn, la.values.length)
        outs = (out(A.I32, n + 1, False), out(code, max(1, cap), False)) if dev else None
        oo, ov = api.list_set(fn, xa, xb if fn in ("except", "intersect", "union") else None, count=count, outs=outs)
    oo, ov = fetch(oo), fetch(ov)
    return dict(offsets=oo.to_numpy().copy(), offsets_length=oo.length, values=ov.to_numpy().copy(), length=ov.length,
                null_count=ov.null_count, offsets_null_count=oo.null_count)


def model(b, fn, needle=None, count=0):
    """The same dictionary from tests/list_ref.py (cached on the case)."""
    key = (fn, None if needle is None else np.asarray(needle).tobytes(), count)
    if key in b.cache:
        return b.cache[key]
    a, o = b.a, b.b
    if fn in ("contains", "position"):
        has, ok, pos = R.find(a.off, a.valid, a.child, needle)
        b.cache[("contains",) + key[1:]] = dict(values=has, valid=ok, null_count=int((~ok).sum()), length=a.n)
        b.cache[("position",) + key[1:]] = dict(values=pos, valid=np.ones(a.n, bool), null_count=0, length=a.n)
    elif fn in ("max", "min"):
        v, ok, nan_only = R.extreme(a.off, a.valid, a.child, fn == "max")
        b.cache[key] = dict(values=v, valid=ok, null_count=int((~ok).sum()), length=a.n, nan_only=nan_only)
    elif fn == "sort":
        v = R.sort(a.off, a.valid, a.child)
        b.cache[key] = dict(values=v, null_count=0, length=len(v))
    else:
        if fn == "remove":
            off, v = R.remove(a.off, a.valid, a.child, needle)
        else:
            off, v = R.set_op(fn, a.off, a.valid, a.child, o.off if o is not None else None, o.child if o is not None else None, count)
        b.cache[key] = dict(offsets=off.astype(np.int32), offsets_length=a.n + 1, values=v, length=len(v), null_count=0, offsets_null_count=0)
    return b.cache[key]


def same(got, want, what):
    """Everything the call returned against the model, bit for bit (a max / min of nothing but NaNs: some NaN)."""
    nan_only = want.get("nan_only")
    for k, w in want.items():
        if k == "nan_only":
            continue
        g = got[k]
        if isinstance(w, np.ndarray):
            assert len(g) == len(w), f"{what}: {k} has {len(g)} entries, expected {len(w)}"
            if k == "values" and nan_only is not None and nan_only.any():
                assert np.isnan(g[nan_only]).all(), f"{what}: a row of NaNs must give a NaN"
                g, w = g[~nan_only], w[~nan_only]
            if w.dtype != bool:
                assert g.dtype == w.dtype, f"{what}: {k} is {g.dtype}, expected {w.dtype}"
                g, w = np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)
            if not np.array_equal(g, w):
                bad = np.flatnonzero(g != w)
                raise AssertionError(f"{what}: {k} differs in {len(bad)} bytes / bits, first at {bad[:5].tolist()}")
        else:
            assert g == w, f"{what}: {k} = {g}, expected {w}"


def calls_of(b, group):
    """(function, needle, count) of every call a case makes."""
    if group == "reduce":
        return [(f, nd, 0) for nd in b.needles for f in ("contains", "position", "remove")] + [("max", None, 0), ("min", None, 0)]
    if group == "sort":
        return [("sort", None, 0)]
    ops = SET_OPS if b.b is not None else ("distinct", "repeat")
    return [(op, None, c) for op in ops for c in (b.counts if op == "repeat" else (0,))]


def kernel_of(fn, form, b):
    kind = "find" if fn in ("contains", "position") else "extreme" if fn in ("max", "min") else fn if fn in ("remove", "sort") else "set"
    return KERNELS[(kind, b.sort if fn == "sort" else form)]


def check_case(api, name, dtname, form=None, layout="plain", row_offset=None, last_kernel=None, dev=None):
    """Every function of the case's group over one materialisation, against the model.  last_kernel: a callable naming the
    kernel the call ran (the product's rdf_last_kernel); it must be the one the case and the form were built for."""
    c, b, code = CASES[name], built(name, dtname), DTYPES[dtname]
    form = form or b.forms()[0]
    la, lb = materialise(b, code, None if c["group"] == "sort" else form, layout, row_offset)
    results = {}
    for fn, needle, count in calls_of(b, c["group"]):
        what = f"{name} {dtname} {fn} form={form} layout={layout}" + (f" needle={needle!r}" if needle is not None else "") + (f" count={count}" if fn == "repeat" else "")
        got = run(api, fn, la, lb, needle, count, dev)
        if last_kernel is not None:
            assert last_kernel() == kernel_of(fn, form, b), f"{what}: ran {last_kernel()}"
        same(got, model(b, fn, needle, count), what)
        results[(fn, None if needle is None else np.asarray(needle).tobytes(), count)] = got
    return results


def check_zero_rows(api, dtname, with_validity, layout="plain", dev=None):
    """Every function over a list of no rows (value_offsets of one entry) whose child array is not empty."""
    dt, code = npdt(dtname), DTYPES[dtname]
    rng = np.random.default_rng(code)
    pool = make_pool(rng, dt, 4)
    a = LL([], np.zeros(0, bool) if with_validity else None, head=4, tail=3).fill(rng, pool)
    b = Built(a, LL([], None, head=0, tail=2).fill(rng, pool), needles=[plain_needle(rng, dt, pool)], counts=(0, 3))
    la, lb = materialise(b, code, None, layout)
    for group in ("reduce", "set", "sort"):
        for fn, needle, count in calls_of(b, group):
            same(run(api, fn, la, lb, needle, count, dev), model(b, fn, needle, count), f"zero rows {dtname} {fn} validity={with_validity}")
